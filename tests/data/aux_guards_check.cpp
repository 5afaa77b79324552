// Stand-alone host program (test fixture, never shipped): drives the
// argument checks of the auxiliary entries (marlin_amd/csrc/aux_guards.h)
// over small values and over values near INT64_MAX.
// tests/test_aux_guards.py builds it under -fsanitize=address,undefined:
// every accepted small case replays the addressing of the kernel or copy
// behind that entry on a heap block of exactly the buffer's size, so an
// accepted call that would leave the buffer traps, and a check that formed
// an overflowing product would trap too. Every decision is compared with a
// restatement in 128-bit arithmetic. Output:
//   decide <check> <args...> <0|1>     a handful, for the Python restatement
//   check <name> accepted <n> refused <n>
//   aux_guards OK <count> checks
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aux_guards.h"

typedef __int128 i128;

static long g_checks = 0;
#define REQUIRE(x)                                                    \
  do {                                                                \
    g_checks++;                                                       \
    if (!(x)) {                                                       \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);             \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static const int64_t BIG = INT64_MAX;
// small values around the edges the sweeps use, and values whose products
// or sums leave 64 bits
static const int64_t SMALL[] = {-1, 0, 1, 2, 3, 4, 5, 7, 8, 9};
static const int64_t WIDE[] = {-1, 0, 1, 2, 3, 5, 8, 9, 16, 17,
                               ((int64_t)1 << 31), ((int64_t)1 << 32) + 1,
                               ((int64_t)1 << 62), BIG / 8, BIG / 8 + 1,
                               BIG / 4 + 1, BIG / 2 + 1, BIG - 1, BIG,
                               INT64_MIN};
static const int64_t SIZES[] = {0, 1, 7, 8, 15, 16, 64, 71, 72, 73, 96, 200};
static const int64_t HUGE_SIZES[] = {BIG, BIG - 7, ((int64_t)1 << 40)};

struct tally {
  const char* name;
  long acc = 0, ref = 0;
  void add(bool ok) { (ok ? acc : ref)++; }
};
static int finish(const tally& t) {
  printf("check %s accepted %ld refused %ld\n", t.name, t.acc, t.ref);
  REQUIRE(t.acc > 0);          // not vacuous either way
  REQUIRE(t.ref > 0);
  return 0;
}

// rows x cols at pitch ld, off_bytes in: the last byte touched, in 128 bits
static bool fits128(int64_t bytes, int64_t elem, int64_t off_bytes,
                    int64_t ld, int64_t rows, int64_t cols) {
  if (off_bytes < 0 || off_bytes > bytes) return false;
  if (rows == 0 || cols == 0) return true;
  const i128 elems = ((i128)cols - 1) * ld + rows;
  // whole elements counted from the offset, as the entries do
  return elems <= ((i128)bytes - off_bytes) / elem;
}

struct heap_buf {
  std::vector<unsigned char> mem;
  mx_dbuf d;
  explicit heap_buf(int64_t bytes) : mem((size_t)bytes) {
    // a non-null pointer even for an empty block, distinct per buffer
    d.ptr = bytes ? (void*)mem.data() : (void*)this;
    d.bytes = bytes;
  }
};
static const int64_t REPLAY_MAX = 4096;   // replay only what a block holds

static int sweep_fill() {
  tally t{"fill_random"};
  for (int fp32 = 0; fp32 < 2; fp32++) {
    const int64_t elem = fp32 ? 4 : 8;
    for (int64_t bytes : SIZES) {
      heap_buf b(bytes);
      for (int64_t n = -2; n <= bytes / elem + 2; n++) {
        const bool ok = mx_aux_fill_ok(&b.d, fp32, n);
        REQUIRE(ok == (n >= 0 && fits128(bytes, elem, 0, 1, 1, n)));
        REQUIRE(ok == (n >= 0 && (i128)n * elem <= bytes));
        if (ok)
          for (int64_t i = 0; i < n; i++) memset(&b.mem[i * elem], 1, elem);
        t.add(ok);
        if (bytes == 72)
          printf("decide fill %d %lld %lld %d\n", fp32, (long long)bytes,
                 (long long)n, (int)ok);
      }
    }
    for (int64_t bytes : HUGE_SIZES) {
      const mx_dbuf d = {(void*)&t, bytes};
      for (int64_t n : WIDE) {
        const bool ok = mx_aux_fill_ok(&d, fp32, n);
        REQUIRE(ok == (n >= 0 && (i128)n * elem <= bytes));
        t.add(ok);
      }
    }
  }
  return finish(t);
}

static int sweep_zero_pad() {
  tally t{"zero_pad"};
  for (int fp32 = 0; fp32 < 2; fp32++) {
    const int64_t elem = fp32 ? 4 : 8;
    for (int64_t bytes : {(int64_t)0, (int64_t)64, (int64_t)96, (int64_t)200}) {
      heap_buf b(bytes);
      for (int64_t rt : SMALL) for (int64_t ct : SMALL) for (int64_t ld : SMALL)
        for (int64_t m : {(int64_t)-1, (int64_t)0, rt - 1, rt, rt + 1})
          for (int64_t n : {(int64_t)-1, (int64_t)0, ct - 1, ct, ct + 1}) {
            const bool ok = mx_aux_zero_pad_ok(&b.d, fp32, rt, ct, ld, m, n);
            const bool want = 0 <= m && m <= rt && rt <= ld && 0 <= n &&
                              n <= ct && fits128(bytes, elem, 0, ld, rt, ct);
            REQUIRE(ok == want);
            if (ok)          // the kernel's stores: c * ld + r, r < rt, c < ct
              for (int64_t c = 0; c < ct; c++)
                for (int64_t r = 0; r < rt; r++)
                  if (r >= m || c >= n)
                    memset(&b.mem[(c * ld + r) * elem], 0, elem);
            t.add(ok);
            if (bytes == 200 && fp32 == 0 && ct == 3 && (ld == 8 || ld == 9) &&
                m == rt && n == ct)
              printf("decide zero_pad %d %lld %lld %lld %lld %lld %lld %d\n",
                     fp32, (long long)bytes, (long long)rt, (long long)ct,
                     (long long)ld, (long long)m, (long long)n, (int)ok);
          }
    }
    for (int64_t bytes : HUGE_SIZES) {
      const mx_dbuf d = {(void*)&t, bytes};
      for (int64_t rt : WIDE) for (int64_t ct : WIDE) for (int64_t ld : WIDE) {
        const bool ok = mx_aux_zero_pad_ok(&d, fp32, rt, ct, ld, 0, 0);
        const bool want = 0 <= rt && rt <= ld && 0 <= ct &&
                          fits128(bytes, elem, 0, ld, rt, ct);
        REQUIRE(ok == want);
        t.add(ok);
      }
    }
  }
  return finish(t);
}

static int sweep_transpose() {
  tally t{"transpose"};
  for (int fp32 = 0; fp32 < 2; fp32++) {
    const int64_t elem = fp32 ? 4 : 8;
    for (int64_t bi : SIZES) for (int64_t bo : SIZES) {
      if (bi > 96 || bo > 96) continue;
      heap_buf in(bi), out(bo);
      for (int64_t m : SMALL) for (int64_t n : SMALL) {
        const bool ok = mx_aux_transpose_ok(fp32, m, n, &in.d, &out.d);
        const bool want = m >= 0 && n >= 0 && (i128)m * n * elem <= bi &&
                          (i128)m * n * elem <= bo;
        REQUIRE(ok == want);
        if (ok)              // out[c * n + r] = in[r * m + c]
          for (int64_t r = 0; r < n; r++)
            for (int64_t c = 0; c < m; c++)
              memcpy(&out.mem[(c * n + r) * elem], &in.mem[(r * m + c) * elem],
                     elem);
        t.add(ok);
        if (bi == 72 && (bo == 72 || bo == 64) && m == 3)
          printf("decide transpose %d %lld %lld %lld %lld %d\n", fp32,
                 (long long)bi, (long long)bo, (long long)m, (long long)n,
                 (int)ok);
      }
    }
    // in place: refused whatever the sizes, by handle and by pointer
    heap_buf a(64);
    mx_dbuf alias = a.d;
    REQUIRE(!mx_aux_transpose_ok(fp32, 1, 1, &a.d, &a.d));
    REQUIRE(!mx_aux_transpose_ok(fp32, 1, 1, &a.d, &alias));
    REQUIRE(!mx_aux_transpose_ok(fp32, 0, 0, &a.d, &alias));
    t.add(false);
    for (int64_t bytes : HUGE_SIZES) {
      const mx_dbuf di = {(void*)&t, bytes}, dn = {(void*)&a, bytes};
      for (int64_t m : WIDE) for (int64_t n : WIDE) {
        const bool ok = mx_aux_transpose_ok(fp32, m, n, &di, &dn);
        REQUIRE(ok == (m >= 0 && n >= 0 && (i128)m * n <= bytes / elem));
        t.add(ok);
      }
    }
  }
  return finish(t);
}

static int sweep_gemv() {
  tally t{"gemv"};
  for (int64_t bytes : SIZES) {
    heap_buf b(bytes);
    for (int64_t m : SMALL) for (int64_t n : SMALL) for (int64_t lda : SMALL) {
      const bool ok = mx_aux_gemv_ok(&b.d, m, n, lda);
      const bool want = m >= 1 && n >= 1 && lda >= m &&
                        fits128(bytes, 8, 0, lda, m, n);
      REQUIRE(ok == want);
      if (ok) {              // the kernel's loads: A[j * lda + r]
        unsigned sum = 0;
        for (int64_t j = 0; j < n; j++)
          for (int64_t r = 0; r < m; r++)
            for (int e = 0; e < 8; e++) sum += b.mem[(j * lda + r) * 8 + e];
        REQUIRE(sum == 0);
      }
      t.add(ok);
      if (bytes == 200 && n == 3 && (m == 7 || m == 8 || m == 9))
        printf("decide gemv %lld %lld %lld %lld %d\n", (long long)bytes,
               (long long)m, (long long)n, (long long)lda, (int)ok);
    }
  }
  for (int64_t bytes : HUGE_SIZES) {
    const mx_dbuf d = {(void*)&t, bytes};
    for (int64_t m : WIDE) for (int64_t n : WIDE) for (int64_t lda : WIDE) {
      const bool ok = mx_aux_gemv_ok(&d, m, n, lda);
      REQUIRE(ok == (m >= 1 && n >= 1 && lda >= m &&
                     fits128(bytes, 8, 0, lda, m, n)));
      t.add(ok);
    }
  }
  return finish(t);
}

static int sweep_copy2d() {
  tally t{"copy2d"};
  for (int elem : {0, 1, 2, 4, 8, 16, -4})
    for (int64_t bytes : {(int64_t)0, (int64_t)64, (int64_t)100,
                          (int64_t)200}) {
      heap_buf b(bytes);
      for (int64_t off : {(int64_t)-8, (int64_t)0, (int64_t)4, (int64_t)8,
                          bytes - 8, bytes, bytes + 1})
        for (int64_t m : SMALL) for (int64_t n : SMALL)
          for (int64_t pitch : SMALL) {
            const bool ok = mx_aux_copy2d_ok(&b.d, elem, off, pitch, m, n);
            const bool want = (elem == 4 || elem == 8) && m >= 1 && n >= 1 &&
                              pitch >= m &&
                              fits128(bytes, elem, off, pitch, m, n);
            REQUIRE(ok == want);
            if (ok)          // hipMemcpy2D's rows: n runs of m * elem bytes
              for (int64_t j = 0; j < n; j++)
                memset(&b.mem[off + j * pitch * elem], 2, (size_t)(m * elem));
            t.add(ok);
            if (bytes == 200 && elem == 8 && (off == 0 || off == 8) &&
                n == 3 && pitch == 8 && m >= 7)
              printf("decide copy2d %d %lld %lld %lld %lld %lld %d\n", elem,
                     (long long)bytes, (long long)off, (long long)pitch,
                     (long long)m, (long long)n, (int)ok);
          }
    }
  for (int elem : {4, 8})
    for (int64_t bytes : HUGE_SIZES) {
      const mx_dbuf d = {(void*)&t, bytes};
      for (int64_t off : {(int64_t)0, (int64_t)8, bytes - 8, bytes, BIG,
                          INT64_MIN})
        for (int64_t m : WIDE) for (int64_t n : WIDE) for (int64_t p : WIDE) {
          const bool ok = mx_aux_copy2d_ok(&d, elem, off, p, m, n);
          REQUIRE(ok == (m >= 1 && n >= 1 && p >= m &&
                         fits128(bytes, elem, off, p, m, n)));
          t.add(ok);
        }
    }
  return finish(t);
}

static int sweep_bytes_and_op() {
  tally tb{"bytes"}, to{"map_op"};
  for (int64_t bytes : SIZES) {
    const mx_dbuf d = {(void*)&tb, bytes};
    for (int64_t ask : {(int64_t)-1, (int64_t)0, bytes - 1, bytes, bytes + 1,
                        BIG, INT64_MIN}) {
      const bool ok = mx_aux_bytes_ok(&d, ask);
      REQUIRE(ok == (ask >= 0 && ask <= bytes));
      tb.add(ok);
    }
  }
  for (int op : {INT32_MIN, -9, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 255,
                 INT32_MAX}) {
    const bool ok = mx_aux_map_op_ok(op);
    REQUIRE(ok == (op >= 0 && op <= 8));
    REQUIRE(mx_aux_map_binary(op) == (op >= 0 && op <= 2));
    printf("decide map_op %d %d\n", op, (int)ok);
    to.add(ok);
  }
  REQUIRE(MX_OP_ADD == 0 && MX_OP_EMUL == 2 && MX_OP_RDIVS == 8);
  return finish(tb) || finish(to);
}

int main() {
  if (sweep_fill() || sweep_zero_pad() || sweep_transpose() || sweep_gemv() ||
      sweep_copy2d() || sweep_bytes_and_op())
    return 1;
  printf("aux_guards OK %ld checks\n", g_checks);
  return 0;
}
