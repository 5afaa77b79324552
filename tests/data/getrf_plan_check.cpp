// Stand-alone host program (test fixture, never shipped): drives the LU
// factorisation plan (marlin_amd/csrc/getrf_plan.h) without a GPU.
// tests/test_getrf_plan.py builds it under -fsanitize=address,undefined.
//   1. the argument check over small values and values near INT64_MAX,
//      every decision compared with a restatement in 128-bit arithmetic,
//      and named rows (negative n, short and misaligned pitch, an image one
//      byte too large for its buffer, a short dPiv, overlap, NULLs);
//   2. the blocked sweep EXECUTED on the CPU at block width 4, n = 0 .. 13,
//      fp64 and fp32: mx_getrf_eliminate on the diagonal block, a plain-loop
//      row permutation, the two substitutions staged through mx_trsm_stage
//      the way the solve's diagonal kernel does, a plain-loop update, on a
//      heap block of exactly the image's size (an access outside traps).
//      Inputs A = P^T (L U) with exact data, so that every operation is
//      exact: required are A[piv] == L U, the known L, U and P, the pads
//      zero, piv a permutation inside each block, and bit equality with an
//      unblocked block-pivoted elimination written here independently;
//   3. the tie rule and the zero-pivot report.
// Output:
//   decide <n> <lda> <bytesA> <bytesP> <rc> <empty>   for the Python restatement
//   check <name> ...
//   getrf_plan OK <count> checks
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "getrf_plan.h"
#include "trsm_plan.h"

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

// ---------------------------------------------------------------------------
// 1. the guard: the contract of include/marlin_gpu.h, restated without a
// 64-bit product
static int want_rc(int64_t w, int fp32, int64_t n, const mx_dbuf* dA,
                   int64_t lda, const mx_dbuf* dP, const int* info,
                   bool* empty) {
  *empty = false;
  if (fp32 != 0 && fp32 != 1) return MX_EINVAL;
  if (n < 0 || !info) return MX_EINVAL;
  if (n == 0) { *empty = true; return MX_OK; }
  if (!dA || !dP || !dA->ptr || !dP->ptr) return MX_EINVAL;
  const i128 np = ((i128)n + w - 1) / w * w;
  if (np > INT32_MAX) return MX_EINVAL;            // int32 row indices
  const int64_t elem = fp32 ? 4 : 8, e16 = 16 / elem;
  if (lda < np || lda % e16) return MX_EINVAL;
  if (dA->bytes < 0 || dP->bytes < 0) return MX_EINVAL;
  if ((np - 1) * lda + np > (i128)(dA->bytes / elem)) return MX_EINVAL;
  if (np * 4 > (i128)dP->bytes) return MX_EINVAL;
  if (dA == dP) return MX_EINVAL;
  const i128 a0 = (i128)(uintptr_t)dA->ptr, p0 = (i128)(uintptr_t)dP->ptr;
  if (a0 < p0 + dP->bytes && p0 < a0 + dA->bytes) return MX_EINVAL;
  return MX_OK;
}

static int sweep_guard() {
  long acc = 0, ref = 0, emp = 0;
  static unsigned char arena[4096];
  int info = 0;
  for (int flag : {-1, 0, 1, 2}) {
    const mx_dbuf dA = {arena, 8 * 8 * 8}, dP = {arena + 2048, 32};
    bool e;
    const int rc = mx_getrf_check(4, flag, 5, &dA, 8, &dP, &info, &e);
    REQUIRE(rc == ((flag == 0 || flag == 1) ? MX_OK : MX_EINVAL));
    (rc ? ref : acc)++;
  }
  const int64_t NS[] = {-1, 0, 1, 3, 4, 5, 8, 9};
  const int64_t LDS[] = {0, 3, 4, 6, 7, 8, 10, 12};
  const int64_t BYTES[] = {0, 8, 128, 248, 255, 256, 448, 511, 512, 1024};
  const int64_t PBYTES[] = {0, 3, 4, 15, 16, 31, 32, 64};
  for (int fp32 = 0; fp32 < 2; fp32++)
    for (int64_t n : NS) for (int64_t lda : LDS)
      for (int64_t ba : BYTES) for (int64_t bp : PBYTES) {
        const mx_dbuf dA = {arena, ba}, dP = {arena + 1024, bp};
        bool e1, e2;
        const int rc = mx_getrf_check(4, fp32, n, &dA, lda, &dP, &info, &e1);
        REQUIRE(rc == want_rc(4, fp32, n, &dA, lda, &dP, &info, &e2));
        REQUIRE(e1 == e2);
        (rc ? ref : e1 ? emp : acc)++;
        if (fp32 == 0 && (n == 4 || n == 5) && (lda == 7 || lda == 8) &&
            (ba == 448 || ba == 512) && (bp == 31 || bp == 32))
          printf("decide %lld %lld %lld %lld %d %d\n", (long long)n,
                 (long long)lda, (long long)ba, (long long)bp, rc, (int)e1);
      }
  // the named rows, n = 5 at w = 4: np = 8, the tight image is 8 * 8 * 8 =
  // 512 bytes, dPiv 32
  {
    const mx_dbuf a = {arena, 512}, p = {arena + 2048, 32};
    const mx_dbuf a_short = {arena, 511}, p_short = {arena + 2048, 31};
    const mx_dbuf a_pitch10 = {arena, (7 * 10 + 8) * 8};
    const mx_dbuf a_pitch10_short = {arena, (7 * 10 + 8) * 8 - 1};
    const mx_dbuf p_same = {arena, 32}, p_over = {arena + 508, 32},
                  p_touch = {arena + 512, 32}, p_before = {arena + 2048 - 32, 32};
    const mx_dbuf a_late = {arena + 2048, 512};
    const mx_dbuf null = {nullptr, 512};
    bool e;
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &p, &info, &e) == MX_OK && !e);
    REQUIRE(mx_getrf_check(4, 0, -1, &a, 8, &p, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 7, &p, &info, &e) == MX_EINVAL);   // short pitch
    REQUIRE(mx_getrf_check(4, 0, 5, &a_pitch10, 9, &p, &info, &e) == MX_EINVAL);  // misaligned
    REQUIRE(mx_getrf_check(4, 0, 5, &a_pitch10, 10, &p, &info, &e) == MX_OK);
    REQUIRE(mx_getrf_check(4, 0, 5, &a_pitch10_short, 10, &p, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a_short, 8, &p, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &p_short, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &a, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &p_same, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &p_over, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a_late, 8, &p, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &p_touch, &info, &e) == MX_OK);
    REQUIRE(mx_getrf_check(4, 0, 5, &a_late, 8, &p_before, &info, &e) == MX_OK);
    REQUIRE(mx_getrf_check(4, 0, 5, &null, 8, &p, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &null, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, nullptr, 8, &p, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, nullptr, &info, &e) == MX_EINVAL);
    REQUIRE(mx_getrf_check(4, 0, 5, &a, 8, &p, nullptr, &e) == MX_EINVAL);
    // the empty call looks at neither buffer, but info must be there
    REQUIRE(mx_getrf_check(4, 0, 0, nullptr, 0, nullptr, &info, &e) == MX_OK && e);
    REQUIRE(mx_getrf_check(4, 0, 0, nullptr, 0, nullptr, nullptr, &e) == MX_EINVAL);
  }
  // wide: w = 128, values whose sums and products leave 64 bits
  const int64_t WIDE[] = {-1, 0, 1, 127, 128, 129, 256,
                          ((int64_t)1 << 31) - 128, ((int64_t)1 << 31) - 127,
                          ((int64_t)1 << 31), ((int64_t)1 << 32) + 128,
                          ((int64_t)1 << 38), ((int64_t)1 << 62), BIG / 8,
                          BIG / 8 + 1, BIG / 2 + 1, BIG - 127, BIG - 126,
                          BIG - 1, BIG, INT64_MIN};
  const int64_t HUGE_BYTES[] = {BIG, BIG - 7, (int64_t)1 << 40, 1 << 20, -8};
  for (int fp32 = 0; fp32 < 2; fp32++)
    for (int64_t n : WIDE) for (int64_t lda : WIDE)
      for (int64_t ba : HUGE_BYTES) for (int64_t bp : HUGE_BYTES) {
        // far apart, unless the image's size reaches dPiv: then both say so
        const mx_dbuf a = {(void*)(uintptr_t)4096, ba},
                      p = {(void*)((uintptr_t)1 << 62), bp};
        bool e1, e2;
        const int rc = mx_getrf_check(128, fp32, n, &a, lda, &p, &info, &e1);
        REQUIRE(rc == want_rc(128, fp32, n, &a, lda, &p, &info, &e2));
        REQUIRE(e1 == e2);
        (rc ? ref : e1 ? emp : acc)++;
      }
  printf("check guard accepted %ld refused %ld empty %ld\n", acc, ref, emp);
  REQUIRE(acc > 100 && ref > 1000 && emp > 10);
  return 0;
}

// ---------------------------------------------------------------------------
// 2. the sweep, executed
static const int W = 4;

template <typename T>
struct image {                       // exactly (cols - 1) * ld + rows elements
  std::vector<T> mem;
  int64_t ld;
  mx_dbuf d;
  image(int64_t rows, int64_t cols, int64_t ld_)
      : mem((size_t)((cols - 1) * ld_ + rows),
            std::numeric_limits<T>::quiet_NaN()), ld(ld_) {
    d.ptr = mem.data();
    d.bytes = (int64_t)(mem.size() * sizeof(T));
  }
  T& at(int64_t i, int64_t j) { return mem.at((size_t)(i + j * ld)); }
};

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static int rnd(int lo, int hi) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (int)((g_rng >> 33) % (uint64_t)(hi - lo + 1));
}

// what the solve's diagonal kernel does with one w x w block of the image
// against r right-hand sides: L staged through mx_trsm_stage, forward
// substitution, X in place and -X into the workspace
template <typename T>
static void diag_solve(int side, int tt, int rev, int unit, int nv,
                       image<T>& A, int64_t t_off, int64_t x_off, int64_t r,
                       std::vector<T>& ws) {
  T L[W][W];
  for (int a = 0; a < W; a++)
    for (int b = 0; b < W; b++) {
      int64_t off = 0;
      const int kind = mx_trsm_stage(W, tt, rev, unit, nv, a, b, A.ld, &off);
      L[a][b] = kind == MX_TRSM_LOAD ? A.mem.at((size_t)(t_off + off))
                                     : (T)kind;
    }
  for (int64_t c = 0; c < r; c++) {
    T y[W];
    for (int a = 0; a < W; a++) {
      const int oa = mx_trsm_orig(W, rev, a);
      T* x = side ? &A.mem.at((size_t)(x_off + c + oa * A.ld))
                  : &A.mem.at((size_t)(x_off + oa + c * A.ld));
      T v = *x;
      for (int b = 0; b < a; b++) v -= L[a][b] * y[b];
      y[a] = v / L[a][a];
      *x = y[a];
      ws.at((size_t)(side ? c + oa * r : oa + c * W)) = -y[a];
    }
  }
}

// the whole entry on the host: what mx_getrf_device enqueues, step by step
template <typename T>
static int run_sweep(int64_t n, image<T>& A, std::vector<int>& piv,
                     int* info) {
  mx_getrf_plan p;
  mx_getrf_steps(W, n, A.ld, &p);
  const int64_t np = p.np;
  REQUIRE(np == (n + W - 1) / W * W && (int64_t)p.steps.size() == np / W);
  REQUIRE(p.ws_elems == W * (np - W) && p.ws_pitch == W);
  std::vector<T> ws((size_t)p.ws_elems, std::numeric_limits<T>::quiet_NaN());
  *info = 0;
  int64_t done = 0;
  for (const mx_getrf_step& st : p.steps) {
    REQUIRE(st.o == done && st.nv == (n - st.o < W ? n - st.o : W));
    REQUIRE(st.nv >= 1 && st.rest == np - st.o - W);
    REQUIRE(st.left_cols == st.o && st.right_col0 == st.o + W &&
            st.right_cols == st.rest);
    REQUIRE(st.nv == W || st.rest == 0);       // only the last block is ragged
    // (1) the diagonal block
    int perm[W], fz = 0;
    mx_getrf_eliminate<T>(W, st.nv, &A.mem.at((size_t)st.d_off), A.ld, perm,
                          &fz);
    for (int g = 0; g < W; g++) piv.at((size_t)(st.o + g)) = (int)st.o + perm[g];
    if (fz && !*info) *info = (int)st.o + fz;
    // (2) the row permutation of the other columns
    for (int side = 0; side < 2; side++) {
      const int64_t c0 = side ? st.right_col0 : 0;
      const int64_t nc = side ? st.right_cols : st.left_cols;
      for (int64_t c = c0; c < c0 + nc; c++) {
        T tmp[W];
        for (int g = 0; g < W; g++) tmp[g] = A.at(st.o + g, c);
        for (int g = 0; g < W; g++) A.at(st.o + g, c) = tmp[perm[g]];
      }
    }
    if (st.rest) {
      // (3) L21 = A21 U11^-1: right, upper, non-unit -> tt = 1, rev = 0
      diag_solve<T>(1, 1, 0, 0, st.nv, A, st.d_off, st.l21_off, st.rest, ws);
      // (4) U12 = L11^-1 A12: left, lower, unit -> tt = 0, rev = 0
      diag_solve<T>(0, 0, 0, 1, st.nv, A, st.d_off, st.u12_off, st.rest, ws);
      // (5) A22 += L21 * (-U12), B from the workspace at pitch w
      for (int64_t j = 0; j < st.rest; j++)
        for (int64_t i = 0; i < st.rest; i++) {
          T acc = A.mem.at((size_t)(st.a22_off + i + j * A.ld));
          for (int k = 0; k < W; k++)
            acc += A.mem.at((size_t)(st.l21_off + i + k * A.ld)) *
                   ws.at((size_t)(k + j * p.ws_pitch));
          A.mem.at((size_t)(st.a22_off + i + j * A.ld)) = acc;
        }
    }
    done += W;
  }
  return 0;
}

// independent: unblocked right-looking elimination of the whole n x n
// matrix, the pivot of column j searched among the rows of j's block only
template <typename T>
static void unblocked(int64_t n, std::vector<T>& a, std::vector<int>& piv,
                      int* info) {
  *info = 0;
  for (int64_t g = 0; g < n; g++) piv[(size_t)g] = (int)g;
  for (int64_t j = 0; j < n; j++) {
    const int64_t end = (j / W + 1) * W < n ? (j / W + 1) * W : n;
    int64_t p = j;
    T best = -1;
    for (int64_t i = j; i < end; i++) {
      const T v = a[(size_t)(i + j * n)];
      if (std::fabs(v) > best) { best = std::fabs(v); p = i; }
    }
    if (p != j) {
      for (int64_t k = 0; k < n; k++)
        std::swap(a[(size_t)(j + k * n)], a[(size_t)(p + k * n)]);
      std::swap(piv[(size_t)j], piv[(size_t)p]);
    }
    const T d = a[(size_t)(j + j * n)];
    if (d == 0) { if (!*info) *info = (int)j + 1; }
    else for (int64_t i = j + 1; i < n; i++) a[(size_t)(i + j * n)] /= d;
    for (int64_t k = j + 1; k < n; k++)
      for (int64_t i = j + 1; i < n; i++)
        a[(size_t)(i + k * n)] -= a[(size_t)(i + j * n)] * a[(size_t)(j + k * n)];
  }
}

// fills the padded image (zero pads, NaN in the pitch pad) from dense n x n
template <typename T>
static void fill_image(image<T>& A, int64_t n, int64_t np,
                       const std::vector<T>& dense) {
  for (int64_t j = 0; j < np; j++)
    for (int64_t i = 0; i < np; i++)
      A.at(i, j) = i < n && j < n ? dense[(size_t)(i + j * n)] : T(0);
}

template <typename T>
static int run_exact(int64_t n, int64_t pad) {
  const int64_t np = (n + W - 1) / W * W;
  // L unit-lower in {0, +-1/4, +-1/2}, U upper integers in [-4, 4] with a
  // diagonal in +-{1, 2, 4}, P a permutation inside each block
  static const T LV[] = {0, 0.25, -0.25, 0.5, -0.5};
  static const T DV[] = {1, -1, 2, -2, 4, -4};
  std::vector<T> L((size_t)(n * n), 0), U((size_t)(n * n), 0),
      LUm((size_t)(n * n), 0), dense((size_t)(n * n), 0);
  for (int64_t j = 0; j < n; j++)
    for (int64_t i = 0; i < n; i++) {
      if (i > j) L[(size_t)(i + j * n)] = LV[rnd(0, 4)];
      else if (i == j) { L[(size_t)(i + j * n)] = 1; U[(size_t)(i + j * n)] = DV[rnd(0, 5)]; }
      else U[(size_t)(i + j * n)] = (T)rnd(-4, 4);
    }
  for (int64_t j = 0; j < n; j++)
    for (int64_t i = 0; i < n; i++) {
      T s = 0;
      for (int64_t k = 0; k < n; k++)
        s += L[(size_t)(i + k * n)] * U[(size_t)(k + j * n)];
      LUm[(size_t)(i + j * n)] = s;
    }
  std::vector<int> P((size_t)n);
  for (int64_t g = 0; g < n; g++) P[(size_t)g] = (int)g;
  for (int64_t o = 0; o < n; o += W) {
    const int64_t len = n - o < W ? n - o : W;
    for (int64_t g = len - 1; g > 0; g--)
      std::swap(P[(size_t)(o + g)], P[(size_t)(o + rnd(0, (int)g))]);
  }
  // A[P[g]] = (L U)[g]
  for (int64_t j = 0; j < n; j++)
    for (int64_t g = 0; g < n; g++)
      dense[(size_t)(P[(size_t)g] + j * n)] = LUm[(size_t)(g + j * n)];

  image<T> A(np, np, np + pad);
  fill_image(A, n, np, dense);
  mx_dbuf dP = {nullptr, 0};
  std::vector<int> piv((size_t)np, -1);
  dP.ptr = piv.data(); dP.bytes = np * 4;
  bool empty; int info = -1;
  REQUIRE(mx_getrf_check(W, sizeof(T) == 4, n, &A.d, A.ld, &dP, &info, &empty)
          == MX_OK && !empty);
  if (run_sweep<T>(n, A, piv, &info)) return 1;
  REQUIRE(info == 0);
  // the known factors and permutation, bit for bit; the pads zero; the
  // pitch pad still NaN
  for (int64_t j = 0; j < np; j++)
    for (int64_t i = 0; i < np; i++) {
      const T want = i < n && j < n
          ? (i > j ? L[(size_t)(i + j * n)] : U[(size_t)(i + j * n)]) : T(0);
      REQUIRE(A.at(i, j) == want);
    }
  for (int64_t j = 0; j + 1 < np; j++)
    for (int64_t i = np; i < A.ld; i++) REQUIRE(std::isnan(A.at(i, j)));
  for (int64_t g = 0; g < np; g++) {
    REQUIRE(piv[(size_t)g] == (g < n ? P[(size_t)g] : (int)g));
    REQUIRE(piv[(size_t)g] / W == g / W);                  // inside its block
  }
  std::vector<char> seen((size_t)np, 0);
  for (int64_t g = 0; g < np; g++) {
    REQUIRE(!seen[(size_t)piv[(size_t)g]]);
    seen[(size_t)piv[(size_t)g]] = 1;
  }
  // A[piv] == L U with the factors as READ from the image
  for (int64_t j = 0; j < n; j++)
    for (int64_t g = 0; g < n; g++) {
      T s = 0;
      for (int64_t k = 0; k <= (g < j ? g : j); k++)
        s += (k == g ? T(1) : A.at(g, k)) * A.at(k, j);
      REQUIRE(s == dense[(size_t)(piv[(size_t)g] + j * n)]);
    }
  // the unblocked elimination gives the same bits
  std::vector<T> ub = dense;
  std::vector<int> upiv((size_t)n);
  int uinfo = -1;
  unblocked<T>(n, ub, upiv, &uinfo);
  REQUIRE(uinfo == 0);
  for (int64_t j = 0; j < n; j++)
    for (int64_t i = 0; i < n; i++)
      REQUIRE(ub[(size_t)(i + j * n)] == A.at(i, j));
  for (int64_t g = 0; g < n; g++) REQUIRE(upiv[(size_t)g] == piv[(size_t)g]);
  return 0;
}

// ---------------------------------------------------------------------------
// 3. ties and zero pivots, n = 9 (three blocks, the last ragged)
template <typename T>
static int run_special() {
  const int64_t n = 9, np = 12;
  // a tie: column 4 (first of block 1) holds 2, -2, 2, 1 in rows 4..7 after
  // block 0 is eliminated; block 0 is the identity, so nothing changes it.
  // The lowest row, 4, must be the pivot: no swap in that column.
  {
    std::vector<T> d((size_t)(n * n), 0);
    for (int64_t i = 0; i < n; i++) d[(size_t)(i + i * n)] = 4;
    d[4 + 4 * n] = 2; d[5 + 4 * n] = -2; d[6 + 4 * n] = 2; d[7 + 4 * n] = 1;
    // and one where the later row is strictly larger: column 0 rows 0..3
    d[0 + 0 * n] = 1; d[2 + 0 * n] = -2; d[3 + 0 * n] = 2;
    image<T> A(np, np, np);
    fill_image(A, n, np, d);
    std::vector<int> piv((size_t)np, -1);
    int info = -1;
    if (run_sweep<T>(n, A, piv, &info)) return 1;
    REQUIRE(info == 0);
    REQUIRE(piv[4] == 4 && piv[0] == 2);        // the lowest of the maxima
    std::vector<T> ub = d;
    std::vector<int> upiv((size_t)n);
    int uinfo;
    unblocked<T>(n, ub, upiv, &uinfo);
    for (int64_t j = 0; j < n; j++)
      for (int64_t i = 0; i < n; i++)
        REQUIRE(ub[(size_t)(i + j * n)] == A.at(i, j));
    for (int64_t g = 0; g < n; g++) REQUIRE(upiv[(size_t)g] == piv[(size_t)g]);
    printf("check tie piv0 %d piv4 %d\n", piv[0], piv[4]);
  }
  // a NaN is passed over while another entry remains
  {
    T blk[W * W] = {};
    blk[0] = std::numeric_limits<T>::quiet_NaN(); blk[1] = 1; blk[2] = 0;
    blk[3] = 0; blk[5] = 1; blk[10] = 1; blk[15] = 1;
    int perm[W], fz;
    mx_getrf_eliminate<T>(W, W, blk, W, perm, &fz);
    REQUIRE(perm[0] == 1 && blk[0] == 1);
  }
  // zero pivots: identity with columns 6 and 8 (1-based: 7 and 9) zeroed in
  // and below the diagonal inside their blocks; info is the FIRST, the sweep
  // completes, and the columns before it are the identity's
  {
    std::vector<T> d((size_t)(n * n), 0);
    for (int64_t i = 0; i < n; i++) d[(size_t)(i + i * n)] = 2;
    d[6 + 6 * n] = 0; d[8 + 8 * n] = 0;
    d[1 + 6 * n] = 3;                            // above the block: not a candidate
    image<T> A(np, np, np);
    fill_image(A, n, np, d);
    std::vector<int> piv((size_t)np, -1);
    int info = -1;
    if (run_sweep<T>(n, A, piv, &info)) return 1;
    REQUIRE(info == 7);
    for (int64_t g = 0; g < np; g++) REQUIRE(piv[(size_t)g] == (int)g);
    // what lies below the block of the zero pivot is divided by that zero
    // when L21 is formed (0 / 0 from column 6 on); everything else is the
    // input's, unchanged
    for (int64_t j = 0; j < np; j++)
      for (int64_t i = 0; i < np; i++) {
        if (i >= 8 && j >= 6) continue;
        REQUIRE(A.at(i, j) == (i < n && j < n ? d[(size_t)(i + j * n)] : T(0)));
      }
    REQUIRE(std::isnan(A.at(8, 6)));
    printf("check zero info %d\n", info);
  }
  return 0;
}

template <typename T>
static int sweep_exec(const char* name) {
  long cases = 0;
  bool empty; int info = -1;
  // n == 0: the no-op, which looks at no buffer
  REQUIRE(mx_getrf_check(W, sizeof(T) == 4, 0, nullptr, 0, nullptr, &info,
                         &empty) == MX_OK && empty);
  cases++;
  for (int64_t n = 1; n <= 13; n++)
    for (int rep = 0; rep < 4; rep++) {
      // tight and padded pitches (a multiple of 16 bytes in both types)
      if (run_exact<T>(n, (rep % 2) * 4)) return 1;
      if (rep == 0) cases++;
    }
  if (run_special<T>()) return 1;
  printf("check exec %s orders %ld\n", name, cases);
  return 0;
}

int main() {
  if (sweep_guard() || sweep_exec<double>("fp64") || sweep_exec<float>("fp32"))
    return 1;
  printf("getrf_plan OK %ld checks\n", g_checks);
  return 0;
}
