// Stand-alone host program (test fixture, never shipped): the arithmetic of
// the two diagonal kernels as the plan headers state it, at the device's
// block width, on data it is given. tests/test_diag_bits_cpu.py builds it
// under -fsanitize=address,undefined with -ffp-contract=off (every fused
// multiply-add below is then one the headers ask for by name, none the
// compiler's choice) and compares the numpy restatements the GPU tests use
// (tests/_fma.py, _getrf_cases.eliminate_restated,
// _trsm_cases.substitute_restated) with its output bit for bit.
//
//   diag_bits_check <problem file> <result file>
//
// Both files are sequences of records of native-endian int32 and element
// words. A problem record is  kind, fp32, then
//   kind 0  fma:    count; x[count], y[count], z[count]
//                   -> __builtin_fma(f)(x, y, z)[count]
//   kind 1  getrf:  nv; block[128 * 128], column-major at pitch 128
//                   -> the block after mx_getrf_eliminate, perm[128] (int32),
//                      first_zero (int32)
//   kind 2  trsm:   side, tt, rev, unit, nv, r; T[128 * 128] as stored,
//                   column-major at pitch 128; the strip, 128 x r at pitch
//                   128 (left) or r x 128 at pitch r (right)
//                   -> the strip after the substitution: L staged through
//                      mx_trsm_stage, each right-hand side gathered through
//                      mx_trsm_orig, solved by mx_trsm_substitute.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "getrf_plan.h"
#include "trsm_plan.h"

static const int W = 128;

static bool get(FILE* f, void* p, size_t bytes) {
  return bytes == 0 || fread(p, 1, bytes, f) == bytes;
}
static bool put(FILE* f, const void* p, size_t bytes) {
  return bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
}

static float fused(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
static double fused(double x, double y, double z) { return __builtin_fma(x, y, z); }

template <typename T>
static int do_fma(FILE* in, FILE* out) {
  int32_t count;
  if (!get(in, &count, 4) || count < 0) return 1;
  std::vector<T> x((size_t)count), y(x), z(x), o(x);
  const size_t bytes = (size_t)count * sizeof(T);
  if (!get(in, x.data(), bytes) || !get(in, y.data(), bytes) ||
      !get(in, z.data(), bytes))
    return 1;
  for (size_t i = 0; i < x.size(); i++) o[i] = fused(x[i], y[i], z[i]);
  return put(out, o.data(), bytes) ? 0 : 1;
}

template <typename T>
static int do_getrf(FILE* in, FILE* out) {
  int32_t nv;
  if (!get(in, &nv, 4) || nv < 0 || nv > W) return 1;
  std::vector<T> block((size_t)W * W);
  if (!get(in, block.data(), block.size() * sizeof(T))) return 1;
  int32_t perm[W];
  int first_zero = 0;
  mx_getrf_eliminate(W, (int)nv, block.data(), (int64_t)W, perm, &first_zero);
  const int32_t fz = first_zero;
  return put(out, block.data(), block.size() * sizeof(T)) &&
                 put(out, perm, sizeof perm) && put(out, &fz, 4)
             ? 0 : 1;
}

template <typename T>
static int do_trsm(FILE* in, FILE* out) {
  int32_t h[6];
  if (!get(in, h, sizeof h)) return 1;
  const int side = h[0], tt = h[1], rev = h[2], unit = h[3], nv = h[4];
  const int64_t r = h[5];
  if (((side | tt | rev | unit) & ~1) || nv < 0 || nv > W || r < 0 ||
      r > (1 << 16))
    return 1;
  std::vector<T> Tm((size_t)W * W), B((size_t)(W * r)), L((size_t)W * W);
  if (!get(in, Tm.data(), Tm.size() * sizeof(T)) ||
      !get(in, B.data(), B.size() * sizeof(T)))
    return 1;
  for (int a = 0; a < W; a++)
    for (int b = 0; b < W; b++) {
      int64_t off = 0;
      const int kind = mx_trsm_stage(W, tt, rev, unit, nv, a, b, W, &off);
      L[(size_t)(a * W + b)] = kind == MX_TRSM_LOAD ? Tm.at((size_t)off)
                                                    : T(kind);
    }
  for (int64_t c = 0; c < r; c++) {
    T y[W];
    for (int a = 0; a < W; a++) {
      const int oa = mx_trsm_orig(W, rev, a);
      y[a] = B.at((size_t)(side ? c + oa * r : oa + c * W));
    }
    mx_trsm_substitute(W, L.data(), y);
    for (int a = 0; a < W; a++) {
      const int oa = mx_trsm_orig(W, rev, a);
      B.at((size_t)(side ? c + oa * r : oa + c * W)) = y[a];
    }
  }
  return put(out, B.data(), B.size() * sizeof(T)) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: diag_bits_check <problem file> <result file>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = in ? fopen(argv[2], "wb") : nullptr;
  if (!in || !out) {
    fprintf(stderr, "diag_bits_check: cannot open the files\n");
    return 2;
  }
  long records = 0;
  int32_t head[2];
  while (fread(head, 1, sizeof head, in) == sizeof head) {
    const int kind = head[0], fp32 = head[1];
    int rc = 1;
    if (fp32 == 0 || fp32 == 1) {
      if (kind == 0) rc = fp32 ? do_fma<float>(in, out) : do_fma<double>(in, out);
      if (kind == 1) rc = fp32 ? do_getrf<float>(in, out) : do_getrf<double>(in, out);
      if (kind == 2) rc = fp32 ? do_trsm<float>(in, out) : do_trsm<double>(in, out);
    }
    if (rc) {
      fprintf(stderr, "diag_bits_check: bad record %ld\n", records);
      return 1;
    }
    records++;
  }
  if (fclose(out) != 0) return 1;
  fclose(in);
  printf("diag_bits OK %ld records\n", records);
  return 0;
}
