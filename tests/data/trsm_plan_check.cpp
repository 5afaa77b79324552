// Stand-alone host program (test fixture, never shipped): drives the
// triangular-solve plan (marlin_amd/csrc/trsm_plan.h) without a GPU.
// tests/test_trsm_plan.py builds it under -fsanitize=address,undefined.
//   1. the argument check over small values and values near INT64_MAX,
//      every decision compared with a restatement in 128-bit arithmetic;
//   2. the plan EXECUTED on the CPU at block width 4: a naive diagonal
//      solve that stages its block through mx_trsm_stage, the way the
//      kernel does, and a naive GEMM that reads exactly what a step names,
//      on heap blocks of exactly the images' sizes (an access outside one
//      traps). All 16 forms, orders around the block edges, exact-integer
//      data, NaN in everything the contract says is never read; the result
//      is compared with the known X and with direct substitution on the
//      whole matrix.
// Output:
//   decide <args...> <rc> <empty>      a handful, for the Python restatement
//   steps <side> <lower> <trans> <n> : <j0>/<rest0>/<rest_len> ...
//   check <name> accepted <n> refused <n>
//   trsm_plan OK <count> checks
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

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
static const double QNAN = std::numeric_limits<double>::quiet_NaN();

// ---------------------------------------------------------------------------
// 1. the guard
static bool fits128(int64_t bytes, int64_t elem, int64_t ld, i128 rows,
                    i128 cols) {
  if (rows == 0 || cols == 0) return true;
  return (cols - 1) * ld + rows <= (i128)(bytes / elem);
}

// the contract of include/marlin_gpu.h, restated without a 64-bit product
static int want_rc(int64_t w, int fp32, int side, int lower, int trans,
                   int unit, int64_t n, int64_t r, const mx_dbuf* dT,
                   int64_t ldt, const mx_dbuf* dB, int64_t ldb, bool* empty) {
  *empty = false;
  for (int f : {fp32, side, lower, trans, unit})
    if (f != 0 && f != 1) return MX_EINVAL;
  if (n < 0 || r < 0 || r % w) return MX_EINVAL;
  if (n == 0 || r == 0) { *empty = true; return MX_OK; }
  if (!dT || !dB || !dT->ptr || !dB->ptr) return MX_EINVAL;
  const i128 np = ((i128)n + w - 1) / w * w;
  if (np > BIG) return MX_EINVAL;
  const int64_t elem = fp32 ? 4 : 8, e16 = 16 / elem;
  const i128 brows = side ? (i128)r : np, bcols = side ? np : (i128)r;
  if (ldt < np || ldb < brows || ldt % e16 || ldb % e16) return MX_EINVAL;
  if (!fits128(dT->bytes, elem, ldt, np, np)) return MX_EINVAL;
  if (!fits128(dB->bytes, elem, ldb, brows, bcols)) return MX_EINVAL;
  if ((np / w) * (r / w) > INT32_MAX || (i128)(r / w) * 2 > INT32_MAX)
    return MX_EINVAL;
  if (dT == dB) return MX_EINVAL;
  const i128 t0 = (i128)(uintptr_t)dT->ptr, b0 = (i128)(uintptr_t)dB->ptr;
  if (t0 < b0 + dB->bytes && b0 < t0 + dT->bytes) return MX_EINVAL;
  return MX_OK;
}

static int sweep_guard() {
  long acc = 0, ref = 0, emp = 0;
  static unsigned char arena[4096];
  // small: w = 4, fp64 (pitches even), every size around the edges
  for (int flag : {-1, 0, 1, 2})
    for (int which = 0; which < 5; which++) {
      int f[5] = {0, 0, 1, 0, 0};
      f[which] = flag;
      const mx_dbuf dT = {arena, 8 * 8 * 8}, dB = {arena + 2048, 8 * 8 * 8};
      bool e1, e2;
      const int rc = mx_trsm_check(4, f[0], f[1], f[2], f[3], f[4], 5, 8, &dT,
                                   8, &dB, 8, &e1);
      REQUIRE(rc == want_rc(4, f[0], f[1], f[2], f[3], f[4], 5, 8, &dT, 8, &dB,
                            8, &e2));
      REQUIRE(rc == ((flag == 0 || flag == 1) ? MX_OK : MX_EINVAL));
      (rc ? ref : acc)++;
    }
  const int64_t NS[] = {-1, 0, 1, 3, 4, 5, 8, 9};
  const int64_t RS[] = {-4, 0, 3, 4, 8};
  const int64_t LDS[] = {0, 3, 4, 6, 7, 8, 10, 12};
  const int64_t BYTES[] = {0, 8, 128, 248, 256, 448, 512, 1024};
  for (int fp32 = 0; fp32 < 2; fp32++) for (int side = 0; side < 2; side++)
    for (int64_t n : NS) for (int64_t r : RS)
      for (int64_t ldt : LDS) for (int64_t ldb : LDS)
        for (int64_t bt : BYTES) for (int64_t bb : BYTES) {
          const mx_dbuf dT = {arena, bt}, dB = {arena + 1024, bb};
          bool e1, e2;
          const int rc = mx_trsm_check(4, fp32, side, 1, 0, 0, n, r, &dT, ldt,
                                       &dB, ldb, &e1);
          REQUIRE(rc == want_rc(4, fp32, side, 1, 0, 0, n, r, &dT, ldt, &dB,
                                ldb, &e2));
          REQUIRE(e1 == e2);
          (rc ? ref : e1 ? emp : acc)++;
          if (fp32 == 0 && side == 0 && r == 4 && ldb == 8 && bb == 256 &&
              (n == 4 || n == 5) && (ldt == 7 || ldt == 8) &&
              (bt == 448 || bt == 512))
            printf("decide %lld %lld %lld %lld %lld %lld %d %d\n",
                   (long long)n, (long long)r, (long long)ldt, (long long)ldb,
                   (long long)bt, (long long)bb, rc, (int)e1);
        }
  // aliasing: one handle; two handles on overlapping or touching ranges
  {
    const mx_dbuf a = {arena, 512}, same = {arena, 512},
                  over = {arena + 504, 512}, touch = {arena + 512, 512},
                  null = {nullptr, 512};
    bool e;
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &a, 4, &a, 4, &e) == MX_EINVAL);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &a, 4, &same, 4, &e) == MX_EINVAL);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &a, 4, &over, 4, &e) == MX_EINVAL);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &over, 4, &a, 4, &e) == MX_EINVAL);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &a, 4, &touch, 4, &e) == MX_OK);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &touch, 4, &a, 4, &e) == MX_OK);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &null, 4, &a, 4, &e) == MX_EINVAL);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 4, &a, 4, nullptr, 4, &e) == MX_EINVAL);
    // the empty call looks at neither
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 0, 4, nullptr, 0, nullptr, 0, &e) == MX_OK && e);
    REQUIRE(mx_trsm_check(4, 0, 0, 1, 0, 0, 4, 0, &a, 1, &a, 1, &e) == MX_OK && e);
    ref += 6; acc += 2; emp += 2;
  }
  // wide: w = 128, values whose sums and products leave 64 bits
  const int64_t WIDE[] = {-1, 0, 1, 127, 128, 129, 256,
                          ((int64_t)1 << 31), ((int64_t)1 << 32) + 128,
                          ((int64_t)1 << 38), ((int64_t)1 << 62), BIG / 8,
                          BIG / 8 + 1, BIG / 2 + 1, BIG - 127, BIG - 126,
                          BIG - 1, BIG, INT64_MIN};
  const int64_t HUGE_BYTES[] = {BIG, BIG - 7, (int64_t)1 << 40, 1 << 20};
  for (int fp32 = 0; fp32 < 2; fp32++) for (int side = 0; side < 2; side++)
    for (int64_t n : WIDE) for (int64_t r : WIDE)
      for (int64_t ldt : WIDE) for (int64_t ldb : WIDE)
        for (int64_t bytes : HUGE_BYTES) {
          // far apart; the huge size goes to one buffer at a time, and
          // where T's then reaches B both sides say so
          mx_dbuf t = {(void*)(uintptr_t)4096, 1 << 20},
                  b = {(void*)((uintptr_t)1 << 62), 1 << 20};
          for (int which = 0; which < 2; which++) {
            t.bytes = which ? (1 << 20) : bytes;
            b.bytes = which ? bytes : (1 << 20);
            bool e1, e2;
            const int rc = mx_trsm_check(128, fp32, side, 0, 1, 1, n, r, &t,
                                         ldt, &b, ldb, &e1);
            REQUIRE(rc == want_rc(128, fp32, side, 0, 1, 1, n, r, &t, ldt, &b,
                                  ldb, &e2));
            REQUIRE(e1 == e2);
            (rc ? ref : e1 ? emp : acc)++;
          }
        }
  printf("check guard accepted %ld refused %ld empty %ld\n", acc, ref, emp);
  REQUIRE(acc > 100 && ref > 1000 && emp > 10);
  return 0;
}

// ---------------------------------------------------------------------------
// 2. the plan, executed
static const int W = 4;

struct image {                       // exactly (cols - 1) * ld + rows doubles
  std::vector<double> mem;
  int64_t ld;
  mx_dbuf d;
  image(int64_t rows, int64_t cols, int64_t ld_) : mem((size_t)((cols - 1) * ld_ + rows), QNAN), ld(ld_) {
    d.ptr = mem.data();
    d.bytes = (int64_t)(mem.size() * 8);
  }
  double& at(int64_t i, int64_t j) { return mem.at((size_t)(i + j * ld)); }
};

// deterministic small integers
static uint64_t g_rng = 0x243F6A8885A308D3ull;
static int rnd(int lo, int hi) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (int)((g_rng >> 33) % (uint64_t)(hi - lo + 1));
}

// op(T)[i][j] of the logical matrix (host copy `full`, n x n, dense)
static double opT(const std::vector<double>& full, int64_t n, int trans,
                  int64_t i, int64_t j) {
  return trans ? full[(size_t)(j + i * n)] : full[(size_t)(i + j * n)];
}

// the diagonal kernel's arithmetic: stage L through mx_trsm_stage, forward
// substitution per right-hand side, X into B and -X into the workspace
static void diag_solve(int side, const mx_trsm_plan& p, const mx_trsm_step& st,
                       int unit, image& T, image& B, std::vector<double>& ws,
                       int64_t r) {
  double L[W * W];
  for (int a = 0; a < W; a++)
    for (int b = 0; b < W; b++) {
      int64_t off = 0;
      const int kind = mx_trsm_stage(W, p.tt, p.rev, unit, st.nv, a, b, T.ld,
                                     &off);
      L[a * W + b] = kind == MX_TRSM_LOAD ? T.mem.at((size_t)(st.t_off + off))
                                          : (double)kind;
    }
  for (int64_t c = 0; c < r; c++) {
    double y[W];
    double* x[W];
    for (int a = 0; a < W; a++) {
      const int oa = mx_trsm_orig(W, p.rev, a);
      x[a] = side ? &B.mem.at((size_t)(st.x_off + c + oa * B.ld))
                  : &B.mem.at((size_t)(st.x_off + oa + c * B.ld));
      y[a] = *x[a];
    }
    // the header's substitution: mx_trsm_update in ascending b, mx_trsm_quot
    mx_trsm_substitute(W, L, y);
    for (int a = 0; a < W; a++) {
      const int oa = mx_trsm_orig(W, p.rev, a);
      *x[a] = y[a];
      ws.at((size_t)(side ? c + oa * r : oa + c * W)) = -y[a];
    }
  }
}

// the update GEMM as a step names it: C += op(A) * op(B), every operand
// block read whole
static void gemm_step(int side, const mx_trsm_step& st, image& T, image& B,
                      std::vector<double>& ws) {
  const double* A = side ? ws.data() : T.mem.data();
  const double* Bm = side ? T.mem.data() : ws.data();
  const size_t asz = side ? ws.size() : T.mem.size();
  const size_t bsz = side ? T.mem.size() : ws.size();
  for (int64_t j = 0; j < st.gn; j++)
    for (int64_t i = 0; i < st.gm; i++) {
      double acc = B.mem.at((size_t)(st.c_off + i + j * st.ldc));
      for (int64_t k = 0; k < st.gk; k++) {
        const size_t ai = (size_t)(st.a_off + (st.trans_a ? k + i * st.lda
                                                          : i + k * st.lda));
        const size_t bi = (size_t)(st.b_off + (st.trans_b ? j + k * st.ldb
                                                          : k + j * st.ldb));
        if (ai >= asz || bi >= bsz) { printf("FAIL gemm operand outside\n"); return; }
        acc += A[ai] * Bm[bi];
      }
      B.mem.at((size_t)(st.c_off + i + j * st.ldc)) = acc;
    }
}

static int run_case(int side, int lower, int trans, int unit, int64_t n,
                    int64_t r, int64_t padt, int64_t padb, bool show) {
  const int64_t np = (n + W - 1) / W * W;
  const int64_t brows = side ? r : np, bcols = side ? np : r;
  image T(np, np, np + padt), B(brows, bcols, brows + padb);
  // logical T: referenced triangle small integers, diagonal a power of two
  std::vector<double> full((size_t)(n * n), 0.0);
  static const double DIAG[] = {0.5, -0.5, 1, -1, 2, -2, 4, -4};
  for (int64_t j = 0; j < n; j++)
    for (int64_t i = 0; i < n; i++) {
      const bool ref = lower ? i >= j : i <= j;
      if (!ref) continue;
      full[(size_t)(i + j * n)] = i == j ? (unit ? 1.0 : DIAG[rnd(0, 7)])
                                         : (double)rnd(-2, 2);
    }
  // the stored image: NaN wherever the contract says "never read" (the
  // constructor's fill), zeros in the pad of the off-diagonal blocks
  const int64_t lastblk = (np - W);
  for (int64_t j = 0; j < np; j++)
    for (int64_t i = 0; i < np; i++) {
      const bool ref = lower ? i >= j : i <= j;
      const bool in_last_diag = i >= lastblk && j >= lastblk;
      if (i < n && j < n) {
        if (ref && !(unit && i == j)) T.at(i, j) = full[(size_t)(i + j * n)];
      } else if (ref && !in_last_diag) {
        T.at(i, j) = 0.0;            // pad of an off-diagonal block: read, zero
      }
    }
  // X known; B = op(T) X (left) or X op(T) (right), exactly
  std::vector<double> X((size_t)(n * r));
  for (auto& x : X) x = rnd(-8, 8);
  for (int64_t c = 0; c < r; c++)
    for (int64_t i = 0; i < np; i++) {
      double s = 0;
      if (i < n)
        for (int64_t k = 0; k < n; k++)
          s += side ? X[(size_t)(c + k * r)] * opT(full, n, trans, k, i)
                    : opT(full, n, trans, i, k) * X[(size_t)(k + c * n)];
      if (side) B.at(c, i) = s; else B.at(i, c) = s;
    }
  const std::vector<double> b0 = B.mem;

  bool empty;
  REQUIRE(mx_trsm_check(W, 0, side, lower, trans, unit, n, r, &T.d, T.ld, &B.d,
                        B.ld, &empty) == MX_OK && !empty);
  mx_trsm_plan p;
  mx_trsm_steps(W, side, lower, trans, n, r, T.ld, B.ld, &p);
  REQUIRE((int64_t)p.steps.size() == np / W && p.np == np);
  REQUIRE(p.ws_elems == W * r);
  std::vector<double> ws((size_t)p.ws_elems, QNAN);
  if (show) printf("steps %d %d %d %lld :", side, lower, trans, (long long)n);
  int64_t done = 0;
  for (const mx_trsm_step& st : p.steps) {
    if (show) printf(" %lld/%lld/%lld", (long long)st.j0, (long long)st.rest0,
                     (long long)st.rest_len);
    // the solved blocks and the rest partition the others
    REQUIRE(st.rest_len == np - W - done);
    REQUIRE(st.rest0 == 0 || st.rest0 == st.j0 + W);
    REQUIRE(st.nv == (n - st.j0 < W ? n - st.j0 : W) && st.nv >= 1);
    REQUIRE(st.gk == W && st.gm % W == 0 && st.gn % W == 0);
    diag_solve(side, p, st, unit, T, B, ws, r);
    if (st.rest_len) gemm_step(side, st, T, B, ws);
    done += W;
  }
  if (show) printf("\n");
  // X, bit for bit; the pad of B zero; the pitch pad still NaN
  for (int64_t c = 0; c < r; c++)
    for (int64_t i = 0; i < np; i++) {
      const double got = side ? B.at(c, i) : B.at(i, c);
      const double want = i < n ? (side ? X[(size_t)(c + i * r)]
                                        : X[(size_t)(i + c * n)]) : 0.0;
      REQUIRE(got == want);
    }
  for (int64_t j = 0; j + 1 < bcols; j++)
    for (int64_t i = brows; i < B.ld; i++) REQUIRE(std::isnan(B.at(i, j)));
  // direct substitution on the whole matrix gives the same
  const int eff_lower = lower ^ trans;
  const bool fwd = side ? !eff_lower : eff_lower;
  for (int64_t c = 0; c < r; c++) {
    std::vector<double> y((size_t)n);
    for (int64_t s = 0; s < n; s++) {
      const int64_t i = fwd ? s : n - 1 - s;
      double v = side ? b0[(size_t)(c + i * B.ld)] : b0[(size_t)(i + c * B.ld)];
      for (int64_t t = 0; t < s; t++) {
        const int64_t k = fwd ? t : n - 1 - t;
        v -= (side ? opT(full, n, trans, k, i) : opT(full, n, trans, i, k)) *
             y[(size_t)k];
      }
      y[(size_t)i] = v / opT(full, n, trans, i, i);
      REQUIRE(y[(size_t)i] == (side ? B.at(c, i) : B.at(i, c)));
    }
  }
  return 0;
}

static int sweep_exec() {
  long cases = 0;
  for (int side = 0; side < 2; side++) for (int lower = 0; lower < 2; lower++)
    for (int trans = 0; trans < 2; trans++) for (int unit = 0; unit < 2; unit++)
      for (int64_t n : {1, 3, 4, 5, 7, 8, 9, 13})
        for (int64_t r : {4, 8}) {
          const int64_t pad = (n % 2) * 2;       // tight and padded pitches
          if (run_case(side, lower, trans, unit, n, r, pad, 2 - pad,
                       unit == 0 && r == 4 && n == 9))
            return 1;
          cases++;
        }
  printf("check exec cases %ld\n", cases);
  return 0;
}

// the staging function alone: what is loaded is inside the referenced
// triangle, below the order, and off a unit diagonal
static int sweep_stage() {
  for (int tt = 0; tt < 2; tt++) for (int rev = 0; rev < 2; rev++)
    for (int unit = 0; unit < 2; unit++) for (int nv = 1; nv <= W; nv++)
      for (int a = 0; a < W; a++) for (int b = 0; b < W; b++) {
        int64_t off = -1;
        const int kind = mx_trsm_stage(W, tt, rev, unit, nv, a, b, 10, &off);
        if (kind != MX_TRSM_LOAD) {
          REQUIRE(off == -1);                // no address was formed
          REQUIRE(kind == MX_TRSM_ZERO || (kind == MX_TRSM_ONE && a == b));
          REQUIRE(a != b || kind == MX_TRSM_ONE);
          continue;
        }
        const int64_t row = off % 10, col = off / 10;   // in T as stored
        REQUIRE(row < nv && col < nv && a >= b);
        REQUIRE(!(unit && row == col));
        // M is lower unless rev; T holds M or its transpose
        const bool t_lower = (rev == 0) != (tt == 1);
        REQUIRE(t_lower ? row >= col : row <= col);
      }
  return 0;
}

int main() {
  if (sweep_guard() || sweep_stage() || sweep_exec()) return 1;
  printf("trsm_plan OK %ld checks\n", g_checks);
  return 0;
}
