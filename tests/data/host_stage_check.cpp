// Stand-alone host program (test fixture, never shipped): runs the staging
// code of the host-buffer entries itself (marlin_amd/csrc/host_stage.h:
// the images, mx_image_bytes, mx_stage_in, mx_stage_out) with a heap
// backend, on malloc blocks of exactly the size the entry would allocate,
// pre-filled with 0xff bytes. Built with -fsanitize=address,undefined by
// tests/test_host_stage.py, so any extent that leaves a block aborts the
// run and a size product formed before it is known to fit traps. Output:
//   gemm_op_layout OK <n>                      the multiply forms, numerically
//   host_stage OK <n> images <n> size checks   every other image; the sizes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_stage.h"

typedef __int128 i128;

#define REQUIRE(x)                                                    \
  do {                                                                \
    if (!(x)) {                                                       \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);             \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// the three operations on host memory (copy2d: hipMemcpy2D semantics)
struct heap_stage {
  long zeros = 0, copies2d = 0, copies = 0;
  int zero(void* p, int64_t bytes) {
    zeros++;
    memset(p, 0, (size_t)bytes);
    return 0;
  }
  int copy2d(void* dst, int64_t dpitch, const void* src, int64_t spitch,
             int64_t width, int64_t cols) {
    copies2d++;
    for (int64_t c = 0; c < cols; c++)
      memcpy((char*)dst + c * dpitch, (const char*)src + c * spitch,
             (size_t)width);
    return 0;
  }
  int copy(void* dst, const void* src, int64_t bytes) {
    copies++;
    memcpy(dst, src, (size_t)bytes);
    return 0;
  }
};

// an exact-size block of 0xff bytes, as a stale workspace would be NaN
static void* stale_block(const mx_op_image& im, int64_t elem) {
  int64_t bytes = -1;
  if (!mx_image_bytes(im, elem, &bytes) || bytes != im.elems() * elem)
    return nullptr;
  void* p = malloc((size_t)bytes);
  if (p) memset(p, 0xff, (size_t)bytes);
  return p;
}

static int check(int ta, int tb, int64_t m, int64_t k, int64_t n) {
  mx_op_image ia, ib, ic;
  mx_gemm_op_layout(ta, tb, m, k, n, &ia, &ib, &ic);
  const int64_t mp = mx_op_round_up(m, 128), np = mx_op_round_up(n, 128),
                kp = mx_op_round_up(k, 16);
  // the workspaces are sized mp*kp, kp*np, mp*np whatever the form
  if (ia.elems() != mp * kp || ib.elems() != kp * np || ic.elems() != mp * np)
    return 1;
  // pitch contract of mxk_gemm_op: covers the run, 16-byte multiple
  if (ia.pitch < (ta ? kp : mp) || ib.pitch < (tb ? np : kp) || ic.pitch < mp)
    return 2;
  if (ia.pitch % 2 || ib.pitch % 2 || ic.pitch % 2) return 3;
  if (ia.rows * ia.cols != m * k || ib.rows * ib.cols != k * n) return 4;

  // exact-size heap buffers: host operands tight, images padded
  std::vector<double> A((size_t)(m * k)), B((size_t)(k * n)), C((size_t)(m * n));
  for (size_t i = 0; i < A.size(); i++) A[i] = (double)(i % 7) - 3;
  for (size_t i = 0; i < B.size(); i++) B[i] = (double)(i % 5) - 2;
  double* dA = (double*)stale_block(ia, 8);
  double* dB = (double*)stale_block(ib, 8);
  double* dC = (double*)stale_block(ic, 8);
  if (!dA || !dB || !dC) return 7;
  heap_stage be;
  if (mx_stage_in(be, dA, ia, 8, A.data())) return 8;
  if (mx_stage_in(be, dB, ib, 8, B.data())) return 8;

  // what the kernel reads: op(A) mp x kp, op(B) kp x np, through the
  // pitches handed to it; pads must contribute exact zeros
  int bad = 0;
  for (int64_t j = 0; j < np; j++)
    for (int64_t i = 0; i < mp; i++) {
      double acc = 0;
      for (int64_t l = 0; l < kp; l++) {
        double a = ta ? dA[i * ia.pitch + l] : dA[l * ia.pitch + i];
        double b = tb ? dB[l * ib.pitch + j] : dB[j * ib.pitch + l];
        acc += a * b;
      }
      dC[j * ic.pitch + i] = acc;
      if ((i >= m || j >= n) && acc != 0) bad = 5;
    }
  if (mx_stage_out(be, C.data(), dC, ic, 8)) return 8;
  for (int64_t j = 0; j < n && !bad; j++)
    for (int64_t i = 0; i < m; i++) {
      double acc = 0;
      for (int64_t l = 0; l < k; l++)
        acc += (ta ? A[i * k + l] : A[l * m + i]) *
               (tb ? B[l * n + j] : B[j * k + l]);
      if (acc != C[j * m + i]) { bad = 6; break; }
    }
  free(dA); free(dB); free(dC);
  return bad;
}

// ---------------------------------------------------------------------------
// One image, byte for byte: in, then out.
static long g_images = 0;

static bool all_bytes(const unsigned char* p, int64_t n, unsigned char v) {
  for (int64_t i = 0; i < n; i++)
    if (p[i] != v) return false;
  return true;
}

static int image_case(const mx_op_image& im, int64_t elem) {
  g_images++;
  REQUIRE(im.rows >= 0 && im.cols >= 0 && im.rows <= im.pitch &&
          im.cols <= im.cap_cols);
  int64_t bytes = -1;
  REQUIRE(mx_image_bytes(im, elem, &bytes));
  REQUIRE(bytes == im.pitch * im.cap_cols * elem);
  const int64_t run = im.rows * elem, host_bytes = run * im.cols;
  // host bytes are never 0x00 or 0xff
  std::vector<unsigned char> host((size_t)host_bytes),
      back((size_t)host_bytes, 0xaa);
  for (int64_t i = 0; i < host_bytes; i++)
    host[i] = (unsigned char)(1 + i % 250);
  unsigned char* dev = (unsigned char*)stale_block(im, elem);
  REQUIRE(dev);
  heap_stage be;
  REQUIRE(mx_stage_in(be, dev, im, elem, host.data()) == 0);
  if (im.empty()) {                     // skipped, not refused
    REQUIRE(be.zeros + be.copies + be.copies2d == 0);
    REQUIRE(all_bytes(dev, bytes, 0xff));
  } else {
    REQUIRE(be.zeros == (im.padded() ? 1 : 0));
    REQUIRE(im.cols == 1 ? (be.copies == 1 && be.copies2d == 0)
                         : (be.copies == 0 && be.copies2d == 1));
    if (!im.padded()) REQUIRE(memcmp(dev, host.data(), (size_t)bytes) == 0);
    const int64_t col = im.pitch * elem;
    for (int64_t c = 0; c < im.cap_cols; c++) {
      const unsigned char* p = dev + c * col;
      if (c < im.cols) {
        REQUIRE(memcmp(p, &host[c * run], (size_t)run) == 0);
        REQUIRE(all_bytes(p + run, col - run, 0));
      } else {
        REQUIRE(all_bytes(p, col, 0));
      }
    }
  }
  REQUIRE(mx_stage_out(be, back.data(), dev, im, elem) == 0);
  if (im.empty()) REQUIRE(all_bytes(back.data(), host_bytes, 0xaa));
  else REQUIRE(back == host);
  free(dev);
  return 0;
}

static const int64_t ROWS[] = {0, 1, 5, 127, 128, 129, 257};  // 0: empty shard
static const int64_t KS[] = {0, 1, 15, 16, 17, 130};

static bool same(const mx_op_image& x, int64_t rows, int64_t cols,
                 int64_t pitch, int64_t cap) {
  return x.rows == rows && x.cols == cols && x.pitch == pitch &&
         x.cap_cols == cap;
}

static int sweep_images() {
  for (int64_t elem : {(int64_t)4, (int64_t)8}) {
    for (int64_t mi : ROWS)
      for (int64_t nj : ROWS) {
        const int64_t mip = mx_op_round_up(mi, 128),
                      njp = mx_op_round_up(nj, 128);
        for (int64_t kx : KS) {
          const int64_t kp = mx_op_round_up(kx, 16);
          mx_op_image a, b, c, ka, kb, kc;
          // the entries' pitches and allocations, restated
          mx_summa_host_layout(mi, nj, mip, njp, kx, kx, &a, &b, &c);
          REQUIRE(same(a, mi, kx, mip, kx));
          REQUIRE(same(b, kx, nj, kp, nj));
          REQUIRE(same(c, mi, nj, mip, njp));
          mx_summa_kres_layout(mi, nj, mip, njp, kx, kp, &ka, &kb, &kc);
          REQUIRE(same(ka, mi, kx, mip, kp));
          REQUIRE(same(kb, kx, nj, kp, njp));
          REQUIRE(same(kc, mi, nj, mip, njp));
          // A depends on (mi, k) and B on (k, nj) only: once each
          if (nj == ROWS[1]) {
            if (image_case(a, elem) || image_case(ka, elem)) return 1;
          }
          if (mi == ROWS[1]) {
            if (image_case(b, elem) || image_case(kb, elem)) return 1;
          }
        }
        mx_op_image c = {mi, nj, mip, njp};
        if (image_case(c, elem)) return 1;
        // add_c and the transposed output of the fused epilogue
        const mx_op_image t = mx_epilogue_image(mi, nj, mip, njp);
        REQUIRE(same(t, nj, mi, njp, mip));
        REQUIRE(t.elems() == c.elems());
        if (image_case(t, elem)) return 1;
      }
    // flat: mx_map / mx_sum (n, 1), mx_transpose / mx_dgemv (m, n)
    for (int64_t len : ROWS)
      for (int64_t count : KS) {
        mx_op_image f;
        REQUIRE(mx_flat_image(len, count, &f));
        REQUIRE(same(f, len * count, 1, len * count, 1));
        REQUIRE(!f.padded());
        if (image_case(f, elem)) return 1;
      }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// mx_image_bytes and mx_flat_image against 128-bit arithmetic.
static long g_sizes = 0;
static const int64_t BIG = INT64_MAX;
static const int64_t CAPS[] = {-1, 0, 1, 2, 3, 4, 7, 8, 16, 128,
                               ((int64_t)1 << 28), ((int64_t)1 << 29),
                               ((int64_t)1 << 30), ((int64_t)1 << 31) - 1,
                               ((int64_t)1 << 31), ((int64_t)1 << 31) + 1,
                               ((int64_t)1 << 32), ((int64_t)1 << 59),
                               ((int64_t)1 << 60), ((int64_t)1 << 61),
                               ((int64_t)1 << 62), BIG / 8, BIG / 8 + 1,
                               BIG / 4, BIG / 4 + 1, BIG - 1, BIG, INT64_MIN};

static int size_case(int64_t pitch, int64_t cap, int64_t elem, long* acc,
                     long* ref) {
  g_sizes++;
  const mx_op_image im = {0, 0, pitch, cap};
  int64_t bytes = -7;
  const bool ok = mx_image_bytes(im, elem, &bytes);
  // pitch * cap is below 2^126; times elem only where that fits 64 bits
  const bool want = pitch >= 0 && cap >= 0 && (i128)pitch * cap <= BIG &&
                    (i128)pitch * cap * elem <= BIG;
  REQUIRE(ok == want);
  if (ok) REQUIRE((i128)bytes == (i128)pitch * cap * elem);
  (ok ? *acc : *ref)++;
  mx_op_image f = {-3, -3, -3, -3};
  const bool fok = mx_flat_image(pitch, cap, &f);
  REQUIRE(fok == (pitch >= 0 && cap >= 0 && (i128)pitch * cap <= BIG));
  if (fok) REQUIRE((i128)f.rows == (i128)pitch * cap && f.pitch == f.rows &&
                   f.cols == 1 && f.cap_cols == 1);
  return 0;
}

static int sweep_sizes() {
  for (int64_t elem : {(int64_t)4, (int64_t)8}) {
    const int64_t b31 = (int64_t)1 << 31, b62 = ((int64_t)1 << 62) / elem,
                  bmax = BIG / elem;
    const struct { const char* name; int64_t v[5]; } bounds[] = {
        {"2^31", {b31 - 2, b31 - 1, b31, b31 + 1, b31 + 2}},
        {"2^62/elem", {b62 - 2, b62 - 1, b62, b62 + 1, b62 + 2}},
        {"INT64_MAX/elem", {bmax - 1, bmax, bmax + 1, BIG - 1, BIG}},
    };
    for (const auto& bd : bounds) {
      long acc = 0, ref = 0;
      for (int64_t x : bd.v)
        for (int64_t y : CAPS)
          if (size_case(x, y, elem, &acc, &ref) ||
              size_case(y, x, elem, &acc, &ref))
            return 1;
      printf("size elem %d boundary %s accepted %ld refused %ld\n", (int)elem,
             bd.name, acc, ref);
      REQUIRE(acc > 0);                 // not vacuous either way
      REQUIRE(ref > 0);
    }
    long acc = 0, ref = 0;
    for (int64_t x : CAPS)
      for (int64_t y : CAPS)
        if (size_case(x, y, elem, &acc, &ref)) return 1;
  }
  // a call fits when every one of its images does (m = n = 2^31, k = 16)
  const mx_op_image a16 = {0, 0, (int64_t)1 << 31, 16},
                    c31 = {0, 0, (int64_t)1 << 31, (int64_t)1 << 31};
  REQUIRE(mx_images_fit(8, {a16, a16}) && !mx_images_fit(4, {a16, a16, c31}));
  REQUIRE(mx_op_can_round(1, 2, 3) && !mx_op_can_round(1, BIG, 3));
  REQUIRE(mx_op_can_round(BIG - 128) && !mx_op_can_round(BIG - 127));
  REQUIRE(mx_op_round_up(BIG - 128, 128) == BIG - 127);
  return 0;
}

int main() {
  const int64_t shapes[][3] = {{1, 1, 1},     {5, 3, 7},    {128, 16, 128},
                               {129, 17, 127}, {100, 33, 260}, {257, 15, 1},
                               {2, 130, 3}};
  int runs = 0;
  for (auto& s : shapes)
    for (int ta = 0; ta < 2; ta++)
      for (int tb = 0; tb < 2; tb++) {
        int rc = check(ta, tb, s[0], s[1], s[2]);
        if (rc) {
          printf("FAIL %d form %d%d shape %lldx%lldx%lld\n", rc, ta, tb,
                 (long long)s[0], (long long)s[1], (long long)s[2]);
          return 1;
        }
        runs++;
      }
  printf("gemm_op_layout OK %d\n", runs);
  if (sweep_images() || sweep_sizes()) return 1;
  printf("host_stage OK %ld images %ld size checks\n", g_images, g_sizes);
  return 0;
}
