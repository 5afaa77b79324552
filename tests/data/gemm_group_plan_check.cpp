// Stand-alone host program (test fixture, never shipped): drives the
// grouped-GEMM plan (marlin_amd/csrc/gemm_group_plan.h) on generated
// tables. The buffers are real heap blocks of exactly the stated size, and
// every corner element of every planned region is touched through the
// pointers of the device table, so under -fsanitize=address (which
// tests/test_gemm_group_plan.py builds with) a region the plan should have
// refused aborts the run. Checked: block id -> (problem, bm, bn) through
// tile_start and a host copy of the kernel's block_remap is a bijection
// onto all tiles of all launched problems; skipped problems own no block;
// the order is descending k and stable; every rejection rule fires on its
// minimal counter-example while the nearest legal table passes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <set>
#include <tuple>
#include <vector>

#include "gemm_group_plan.h"

// kernels.hip block_remap, restated for the host
static void block_remap(int id, int nbn, int nbm, int band, int& bm, int& bn) {
  int abands = band < 0 ? -band : band;
  int per_band = nbm * abands;
  int b0 = id / per_band;
  int w = id - b0 * per_band;
  int first_bn = b0 * abands;
  int bw = std::min(abands, nbn - first_bn);
  if (band < 0) {
    bn = first_bn + w / nbm;
    bm = w % nbm;
  } else {
    int sh = 8 * bw;
    int t = w / sh, l = w - t * sh;
    bm = t * 8 + l / bw;
    bn = first_bn + l % bw;
  }
}

// the kernel's search: largest p with tile_start[p] <= id
static int find_problem(const std::vector<int32_t>& ts, int count, int id) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (ts[mid] <= id) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct pool {
  std::vector<mx_dbuf*> v;
  mx_dbuf* mk(int64_t bytes) {
    mx_dbuf* b = new mx_dbuf();
    b->ptr = malloc((size_t)(bytes > 0 ? bytes : 1));
    b->bytes = bytes;
    v.push_back(b);
    return b;
  }
  ~pool() {
    for (mx_dbuf* b : v) { free(b->ptr); delete b; }
  }
};

static int g_checks = 0;
#define REQUIRE(x)                                                    \
  do {                                                                \
    g_checks++;                                                       \
    if (!(x)) {                                                       \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);             \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static int rnd(int n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (int)((rng_state >> 33) % (uint64_t)n);
}

static mx_gemm_problem_t prob(int64_t m, int64_t k, int64_t n, mx_dbuf* a,
                              int64_t ao, int64_t lda, mx_dbuf* b, int64_t bo,
                              int64_t ldb, mx_dbuf* c, int64_t co,
                              int64_t ldc) {
  mx_gemm_problem_t q;
  q.m = m; q.k = k; q.n = n;
  q.dA = a; q.a_off = ao; q.lda = lda;
  q.dB = b; q.b_off = bo; q.ldb = ldb;
  q.dC = c; q.c_off = co; q.ldc = ldc;
  return q;
}

// touch the four corners of a rows x cols region (ASan checks the bounds)
template <typename T>
static void touch(const void* base, int64_t ld, int64_t rows, int64_t cols) {
  volatile T* p = (volatile T*)base;
  p[0] = p[0]; p[rows - 1] = p[rows - 1];
  p[(cols - 1) * ld] = p[(cols - 1) * ld];
  p[(cols - 1) * ld + rows - 1] = p[(cols - 1) * ld + rows - 1];
}

// One generated table: each problem in buffers of its own, exactly sized.
static int check_table(const std::vector<std::tuple<int, int, int>>& shapes,
                       int fp32, int ta, int tb, int bandw, int plain) {
  const int64_t elem = fp32 ? 4 : 8;
  pool P;
  std::vector<mx_gemm_problem_t> t;
  for (auto& s : shapes) {
    const int64_t m = 128 * std::get<0>(s), n = 128 * std::get<1>(s),
                  k = 16 * std::get<2>(s);
    const int64_t ar = ta ? k : m, ac = ta ? m : k;
    const int64_t br = tb ? n : k, bc = tb ? k : n;
    const int64_t pad = 16 / elem * rnd(3), off = 16 / elem * rnd(4);
    const int64_t lda = ar + pad, ldb = br + pad, ldc = m + pad;
    auto bytes = [&](int64_t o, int64_t ld, int64_t r, int64_t c) {
      return (r && c) ? (o + (c - 1) * ld + r) * elem : o * elem;
    };
    t.push_back(prob(m, k, n, P.mk(bytes(off, lda, ar, ac)), off, lda,
                     P.mk(bytes(off, ldb, br, bc)), off, ldb,
                     P.mk(bytes(off, ldc, m, n)), off, ldc));
  }
  mx_group_plan plan;
  REQUIRE(mx_gemm_group_plan(fp32, 0, ta, tb, bandw, plain, (int)t.size(),
                             t.data(), &plan) == MX_OK);
  // launched = non-empty with k > 0, by descending k, stable
  std::vector<int> want;
  for (int i = 0; i < (int)t.size(); i++)
    if (t[i].m && t[i].n && t[i].k) want.push_back(i);
  std::stable_sort(want.begin(), want.end(),
                   [&](int a, int b) { return t[a].k > t[b].k; });
  REQUIRE(plan.order == want);
  const int count = (int)plan.entries.size();
  REQUIRE(count == (int)want.size());
  REQUIRE((int)plan.tile_start.size() == count + 1);
  REQUIRE(plan.tile_start[0] == 0);
  size_t zeros = 0;
  double flops = 0;
  for (auto& q : t) {
    if (q.m && q.n && !q.k) zeros++;
    flops += 2.0 * q.m * q.k * q.n;
  }
  REQUIRE(plan.zeros.size() == zeros);      // beta 0: k == 0 regions cleared
  REQUIRE(plan.flops == flops);
  int64_t total = 0;
  for (int e = 0; e < count; e++) {
    const mx_gemm_problem_t& q = t[want[e]];
    const mx_group_entry& g = plan.entries[e];
    REQUIRE(e == 0 || plan.entries[e - 1].ntiles >= g.ntiles);
    REQUIRE(g.ntiles == q.k / 16 && g.nbm == q.m / 128 && g.nbn == q.n / 128);
    REQUIRE(g.lda == q.lda && g.ldb == q.ldb && g.ldc == q.ldc);
    REQUIRE(g.A == (char*)q.dA->ptr + q.a_off * elem);
    REQUIRE(g.B == (char*)q.dB->ptr + q.b_off * elem);
    REQUIRE(g.C == (char*)q.dC->ptr + q.c_off * elem);
    REQUIRE(g.band == (plain ? -1 : 1) * std::min<int>(g.nbn, bandw));
    REQUIRE(plan.tile_start[e] == total);
    total += (int64_t)g.nbm * g.nbn;
    if (fp32) {
      touch<float>(g.A, g.lda, ta ? q.k : q.m, ta ? q.m : q.k);
      touch<float>(g.B, g.ldb, tb ? q.n : q.k, tb ? q.k : q.n);
      touch<float>(g.C, g.ldc, q.m, q.n);
    } else {
      touch<double>(g.A, g.lda, ta ? q.k : q.m, ta ? q.m : q.k);
      touch<double>(g.B, g.ldb, tb ? q.n : q.k, tb ? q.k : q.n);
      touch<double>(g.C, g.ldc, q.m, q.n);
    }
  }
  REQUIRE(plan.blocks() == total);
  // block id -> (problem, bm, bn) is a bijection onto all launched tiles
  std::set<std::tuple<int, int, int>> seen;
  for (int id = 0; id < total; id++) {
    const int p = find_problem(plan.tile_start, count, id);
    REQUIRE(plan.tile_start[p] <= id && id < plan.tile_start[p + 1]);
    const mx_group_entry& g = plan.entries[p];
    int bm = -1, bn = -1;
    block_remap(id - plan.tile_start[p], g.nbn, g.nbm, g.band, bm, bn);
    REQUIRE(bm >= 0 && bm < g.nbm && bn >= 0 && bn < g.nbn);
    REQUIRE(seen.insert(std::make_tuple(p, bm, bn)).second);
  }
  REQUIRE((int64_t)seen.size() == total);
  return 0;
}

static int plan_rc(std::vector<mx_gemm_problem_t> t, int fp32 = 0, int ta = 0,
                   int tb = 0, int beta = 0) {
  mx_group_plan plan;
  return mx_gemm_group_plan(fp32, beta, ta, tb, 8, 0, (int)t.size(), t.data(),
                            &plan);
}
#define LEGAL(...) REQUIRE(plan_rc(__VA_ARGS__) == MX_OK)
#define REFUSED(...) REQUIRE(plan_rc(__VA_ARGS__) == MX_EINVAL)

static int check_rejections() {
  pool P;
  const int64_t E = 128 * 16 + 0;                     // fp64 elems of A / B
  mx_dbuf* a = P.mk(128 * 16 * 8);                    // 128 x 16, tight
  mx_dbuf* b = P.mk(16 * 128 * 8);                    // 16 x 128, tight
  mx_dbuf* c = P.mk(128 * 128 * 8);
  (void)E;
  const mx_gemm_problem_t ok = prob(128, 16, 128, a, 0, 128, b, 0, 16, c, 0, 128);
  mx_group_plan plan;
  LEGAL({ok});
  // the call as a whole
  REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, -1, &ok, &plan) == MX_EINVAL);
  REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, 1, nullptr, &plan) == MX_EINVAL);
  REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, 0, nullptr, &plan) == MX_OK);
  REQUIRE(plan.blocks() == 0 && plan.entries.empty());
  REQUIRE(mx_gemm_group_plan(0, 0, 2, 0, 8, 0, 1, &ok, &plan) == MX_EINVAL);
  REQUIRE(mx_gemm_group_plan(0, 0, 0, -1, 8, 0, 1, &ok, &plan) == MX_EINVAL);
  REQUIRE(mx_gemm_group_plan(0, 0, 1, 1, 8, 0, 0, nullptr, &plan) == MX_OK);
  // dims
  { auto q = ok; q.m = 127; REFUSED({q}); }
  { auto q = ok; q.n = 64; REFUSED({q}); }
  { auto q = ok; q.k = 8; REFUSED({q}); }
  { auto q = ok; q.m = -128; REFUSED({q}); }
  { auto q = ok; q.k = -16; REFUSED({q}); }
  // NULL buffers: refused in a non-empty problem, ignored in an empty one
  { auto q = ok; q.dA = nullptr; REFUSED({q}); q.m = 0; LEGAL({q}); }
  { auto q = ok; q.dB = nullptr; REFUSED({q}); q.n = 0; LEGAL({q}); }
  { auto q = ok; q.dC = nullptr; REFUSED({q}); q.k = 0; REFUSED({q}); }
  // pitches: cover the leading dimension, multiple of 16 bytes
  { mx_dbuf* big = P.mk(130 * 128 * 8);
    auto q = ok; q.dC = big; q.ldc = 130; LEGAL({q});
    q.ldc = 129; REFUSED({q}); q.ldc = 126; REFUSED({q}); }
  { auto q = ok; q.lda = 126; REFUSED({q}); }
  { auto q = ok; q.ldb = 14; REFUSED({q}); }
  // trans_* meaning of lda / ldb: A stored 16 x 128 needs lda >= 16 only
  { auto q = ok; q.lda = 16; q.ldb = 128; LEGAL({q}, 0, 1, 1);
    REFUSED({q}, 0, 0, 0); q.ldb = 16; REFUSED({q}, 0, 1, 1); }
  // offsets: multiple of 16 bytes, not negative
  { mx_dbuf* big = P.mk((128 * 128 + 2) * 8);
    auto q = ok; q.dC = big; q.c_off = 2; LEGAL({q});
    q.c_off = 1; REFUSED({q}); q.c_off = -2; REFUSED({q}); }
  { mx_dbuf* big = P.mk((128 * 128 + 4) * 4), *a4 = P.mk(128 * 16 * 4),
            *b4 = P.mk(16 * 128 * 4);
    auto q = prob(128, 16, 128, a4, 0, 128, b4, 0, 16, big, 4, 128);
    LEGAL({q}, 1); q.c_off = 2; REFUSED({q}, 1); }
  // extents: one element past bytes
  { mx_dbuf* c1 = P.mk(128 * 128 * 8 - 8);
    auto q = ok; q.dC = c1; REFUSED({q}); }
  { mx_dbuf* a1 = P.mk(128 * 16 * 8 - 8);
    auto q = ok; q.dA = a1; REFUSED({q}); }
  { mx_dbuf* b1 = P.mk(16 * 128 * 8 - 8);
    auto q = ok; q.dB = b1; REFUSED({q}); }
  { mx_dbuf* c2 = P.mk((128 * 128 + 2) * 8);
    auto q = ok; q.dC = c2; q.c_off = 2; LEGAL({q}); q.c_off = 4; REFUSED({q}); }
  // a huge pitch must not wrap the extent arithmetic
  { auto q = ok; q.ldc = (int64_t)1 << 62; REFUSED({q}); }
  // aliasing. One 256-pitch image of 256 x 256 holds four 128 x 128 blocks
  { mx_dbuf* img = P.mk(256 * 256 * 8);
    auto c00 = prob(128, 16, 128, a, 0, 128, b, 0, 16, img, 0, 256);
    auto c10 = c00; c10.c_off = 128;                 // row-adjacent: legal
    auto c01 = c00; c01.c_off = 128 * 256;
    LEGAL({c00, c10}); LEGAL({c00, c10, c01});
    auto cov = c00; cov.c_off = 126;                 // two rows overlapping
    REFUSED({c00, cov});
    REFUSED({c00, c00});                             // the same C twice
    auto cp = c10; cp.ldc = 258;                     // spans cross, pitches differ
    REFUSED({c00, cp});
    // a C region against an A / B region of the call
    auto ain = prob(128, 16, 128, img, 128 * 256, 256, b, 0, 16, img, 0, 256);
    LEGAL({ain});                                    // A is block (0,1): disjoint
    auto aov = ain; aov.a_off = 127 * 256;           // A's first column in C
    REFUSED({aov});
    auto bin = prob(128, 16, 128, a, 0, 128, img, 128, 256, img, 0, 256);
    LEGAL({bin});                                    // B rows 128..143: disjoint
    bin.b_off = 126; REFUSED({bin});
    // another problem's A may not be this problem's C either
    auto rd = prob(128, 16, 128, img, 0, 256, b, 0, 16, c, 0, 128);
    REFUSED({c00, rd}); LEGAL({c10, rd});
    // a region that wraps a column is never a rectangle
    mx_dbuf* wide = P.mk((256 * 129 + 64) * 8);
    auto w0 = prob(128, 16, 128, a, 0, 128, b, 0, 16, wide, 192, 256);
    auto w1 = prob(128, 16, 128, a, 0, 128, b, 0, 16, wide, 64, 256);
    LEGAL({w0}); LEGAL({w1});
    REFUSED({w0, w1}); }
  // A and B may repeat and overlap; dA == dB (Gram form) stays legal
  { mx_dbuf* g = P.mk(16 * 128 * 8), *c2 = P.mk(128 * 128 * 8);
    auto q = prob(128, 16, 128, g, 0, 16, g, 0, 16, c, 0, 128);
    LEGAL({q}, 0, 1, 0);
    auto r = q; r.dC = c2; LEGAL({q, r}, 0, 1, 0); }
  // k == 0: C zeroed without accumulate, left alone with it; no block
  { auto q = ok; q.k = 0;
    REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, 1, &q, &plan) == MX_OK);
    REQUIRE(plan.entries.empty() && plan.zeros.size() == 1 &&
            plan.blocks() == 0);
    REQUIRE(plan.zeros[0].C == c->ptr && plan.zeros[0].m == 128);
    REQUIRE(mx_gemm_group_plan(0, 1, 0, 0, 8, 0, 1, &q, &plan) == MX_OK);
    REQUIRE(plan.entries.empty() && plan.zeros.empty()); }
  // a pitch of 2^26 elements takes the whole launch off the pipelined loop
  { auto q = ok; q.n = 0; q.ldb = (int64_t)1 << 26;
    REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, 1, &q, &plan) == MX_OK);
    REQUIRE(plan.pitch32);                           // skipped: no say
    // (a stated size only: the plan never dereferences a buffer)
    mx_dbuf huge;
    huge.ptr = a->ptr;
    huge.bytes = (((int64_t)127 << 26) + 16) * 8;
    auto r = prob(128, 16, 128, a, 0, 128, &huge, 0, (int64_t)1 << 26, c, 0, 128);
    REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, 1, &r, &plan) == MX_OK);
    REQUIRE(!plan.pitch32 && plan.entries.size() == 1);
    r.ldb -= 2;
    REQUIRE(mx_gemm_group_plan(0, 0, 0, 0, 8, 0, 1, &r, &plan) == MX_OK);
    REQUIRE(plan.pitch32);
    huge.bytes -= 8; r.ldb += 2; REFUSED({r}); }
  return 0;
}

int main() {
  int tables = 0;
  // fixed tables: the ragged second band (nbn = 9), the ragged supertile
  // (nbm = 9), both, skipped problems in every position
  const std::vector<std::vector<std::tuple<int, int, int>>> fixed = {
      {{1, 1, 1}},
      {{1, 9, 2}}, {{9, 1, 2}}, {{9, 9, 1}}, {{17, 3, 1}}, {{3, 17, 1}},
      {{1, 1, 1}, {1, 1, 2}, {2, 1, 3}, {1, 3, 1}, {3, 2, 5}, {1, 9, 2},
       {9, 1, 2}},
      {{0, 1, 1}, {1, 0, 1}, {1, 1, 0}},
      {{0, 1, 1}, {2, 2, 2}, {1, 0, 1}, {1, 1, 0}, {1, 9, 2}, {0, 0, 0}},
      {{1, 1, 3}, {1, 1, 3}, {1, 1, 1}, {1, 1, 3}, {1, 1, 2}},
  };
  for (auto& s : fixed)
    for (int cfg = 0; cfg < 16; cfg++) {
      if (check_table(s, cfg & 1, (cfg >> 1) & 1, (cfg >> 2) & 1, 8, cfg >> 3))
        return 1;
      tables++;
    }
  // generated tables, band widths other than 8 included
  for (int it = 0; it < 40; it++) {
    std::vector<std::tuple<int, int, int>> s;
    const int np = 1 + rnd(12);
    for (int i = 0; i < np; i++)
      s.push_back({rnd(11), rnd(11), rnd(6)});
    const int bandw = it % 4 == 3 ? 1 + rnd(10) : 8;
    if (check_table(s, rnd(2), rnd(2), rnd(2), bandw, rnd(2))) return 1;
    tables++;
  }
  if (check_rejections()) return 1;
  printf("gemm_group_plan OK %d tables %d checks\n", tables, g_checks);
  return 0;
}
