// gemm_launch_policy.h — host-only statement of which gemm_mfma_kernel
// instantiation a GEMM launch runs, and with which remap arguments:
// (MARLIN_GEMM_* knobs, type, beta, op form, shape, pitches) -> variant.
// kernels.hip launches what these functions select and nothing else. No HIP
// here, so a plain CPU program can check it
// (tests/test_gemm_launch_policy.py builds one under AddressSanitizer).
#ifndef MARLIN_GEMM_LAUNCH_POLICY_H
#define MARLIN_GEMM_LAUNCH_POLICY_H

#include <stdint.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

// Pitches (elements) at or above this bound take the two-barrier loop: the
// pipelined loop adds 32-bit per-lane byte offsets (up to 15 columns of B,
// 1 of A, plus one 1 KiB run; checked at the largest admitted pitch by
// tests/test_gemm_stage_layout.py) to its running pointers. A transposed
// operand takes the other operand's offsets with its own pitch, so the one
// bound on both pitches covers every form.
constexpr int64_t MX_GEMM_PITCH32_BOUND = (int64_t)1 << 26;

static inline bool mx_gemm_pitch32(int64_t lda, int64_t ldb) {
  return lda < MX_GEMM_PITCH32_BOUND && ldb < MX_GEMM_PITCH32_BOUND;
}

// Pitch contract of the GEMM kernels: every column start must stay
// 16-byte aligned (global_load_lds moves 16-byte chunks; the fused
// epilogue stores float4), and a pitch must cover its leading dimension.
static inline bool pitch_ok(int64_t ld, int64_t rows, int64_t elems16) {
  return ld >= rows && ld % elems16 == 0;
}

// ---------------------------------------------------------------------------
// The MARLIN_GEMM_* knobs, decoded.
enum { MX_GEOM_DEFAULT = 0, MX_GEOM_BK32 = 1, MX_GEOM_BM256 = 2 };
enum { MX_LOOP_UNSET = -1, MX_LOOP_TWOBAR = 0, MX_LOOP_PIPE = 1 };

struct mx_gemm_knobs {
  int band_width = 8;            // MARLIN_GEMM_BAND: block-columns per band
  int plain_bands = 0;           // MARLIN_GEMM_REMAP=bands: no supertiles
  int geometry = MX_GEOM_DEFAULT;  // MARLIN_GEMM_CFG=bk32 / =bm256 request
  int phase_mask = 0;            // MARLIN_GEMM_PHASE: k-phase stagger, 0 off
  int loop = MX_LOOP_UNSET;      // MARLIN_GEMM_LOOP=twobar / =pipe
};

// The parameter `getenv` is the lookup, name -> string or nullptr: the C
// library's getenv in kernels.hip (which latches the result once per
// process), a table in the check program.
template <class Lookup>
static inline mx_gemm_knobs mx_gemm_parse_knobs(Lookup&& getenv) {
  mx_gemm_knobs k;
  const char* band = getenv("MARLIN_GEMM_BAND");
  k.band_width = band ? atoi(band) : 8;
  if (k.band_width < 1) k.band_width = 8;
  // default: supertiled bands; MARLIN_GEMM_REMAP=bands -> plain bands
  const char* remap = getenv("MARLIN_GEMM_REMAP");
  k.plain_bands = remap && remap[0] == 'b';
  // default BK=16/BM=128, 2x256-thread blocks per CU (measured winner);
  // MARLIN_GEMM_CFG=bk32 -> 512-thread BK=32; =bm256 -> 256x128 tile /
  // 512-thread (halves DMA-per-flop and barrier rate at 1 block/CU)
  const char* cfg = getenv("MARLIN_GEMM_CFG");
  if (cfg && cfg[0] == 'b' && cfg[1] == 'k') k.geometry = MX_GEOM_BK32;
  if (cfg && cfg[0] == 'b' && cfg[1] == 'm') k.geometry = MX_GEOM_BM256;
  // k-phase stagger mask (experiment; see the kernel comment). 0 = off.
  const char* phase = getenv("MARLIN_GEMM_PHASE");
  k.phase_mask = phase ? atoi(phase) : 0;
  const char* loop = getenv("MARLIN_GEMM_LOOP");
  k.loop = !loop ? MX_LOOP_UNSET : loop[0] == 't' ? MX_LOOP_TWOBAR
         : loop[0] == 'p' ? MX_LOOP_PIPE : MX_LOOP_UNSET;
  return k;
}

// ---------------------------------------------------------------------------
// One launch: the template arguments of gemm_mfma_kernel as integers (T: 0
// = double, 1 = float; EPI: 0 = store, 1 = fused transpose/add; GRP: 1 =
// grouped table) and the two remap arguments.
struct mx_gemm_variant {
  int T, BETA, BK, BM, WM, WN, PIPE, TA, TB, EPI, GRP;
  int band;         // block_remap band: > 0 supertiled, < 0 plain
  int phase_mask;
};

static inline bool mx_gemm_same_kernel(const mx_gemm_variant& a,
                                       const mx_gemm_variant& b) {
  return a.T == b.T && a.BETA == b.BETA && a.BK == b.BK && a.BM == b.BM &&
         a.WM == b.WM && a.WN == b.WN && a.PIPE == b.PIPE && a.TA == b.TA &&
         a.TB == b.TB && a.EPI == b.EPI && a.GRP == b.GRP;
}

// The k-loop, one rule for every launcher. Decided per variant by paired
// runs on one box (profiles/r03_pipelined_loop.md): the pipelined
// one-barrier loop won for every fp64 variant (+6.5% default, +6.2% bk32,
// +9.9% bm256) and for fp32 bk32 (+7.2%), and lost for fp32 BK=16 (-3.0%;
// presumably its 4 waves/SIMD already cover the loop top), which keeps the
// two-barrier loop. MARLIN_GEMM_LOOP=twobar / =pipe force one loop
// everywhere (paired comparisons, tests). A pitch so large that the
// pipelined loop's 32-bit per-lane DMA offsets could overflow
// (MX_GEMM_PITCH32_BOUND) always takes the two-barrier loop.
static inline int mx_gemm_pipelined(const mx_gemm_knobs& k, int is_fp32,
                                    int bk, bool pitch32) {
  if (!pitch32) return 0;
  if (k.loop != MX_LOOP_UNSET) return k.loop == MX_LOOP_PIPE;
  return !(is_fp32 && bk == 16);
}

static inline int mx_gemm_band(const mx_gemm_knobs& k, int64_t nbn) {
  const int band = nbn < k.band_width ? (int)nbn : k.band_width;
  return k.plain_bands ? -band : band;
}

// Plain and transposed-operand launches (mxk_gemm_op). M, N, K are padded
// (multiples of 128, 128, 16). bk32 needs K % 32 == 0, bm256 fp64 and
// M % 256 == 0; the transposed forms exist in the default geometry only.
static inline mx_gemm_variant mx_gemm_select(const mx_gemm_knobs& k,
                                             int is_fp32, int beta_one,
                                             int trans_a, int trans_b,
                                             int64_t M, int64_t N, int64_t K,
                                             int64_t lda, int64_t ldb) {
  const bool nn = !trans_a && !trans_b;
  const bool bm256 = nn && k.geometry == MX_GEOM_BM256 && !is_fp32 &&
                     M % 256 == 0;
  const bool bk32 = nn && k.geometry == MX_GEOM_BK32 && K % 32 == 0;
  mx_gemm_variant v = {is_fp32 ? 1 : 0, beta_one ? 1 : 0, 16, 128, 2, 2, 0,
                       trans_a ? 1 : 0, trans_b ? 1 : 0, 0, 0,
                       mx_gemm_band(k, N / 128), k.phase_mask};
  if (bm256)     { v.BM = 256; v.WM = 4; v.WN = 2; }
  else if (bk32) { v.BK = 32; v.WM = 2; v.WN = 4; }
  v.PIPE = mx_gemm_pipelined(k, v.T, v.BK, mx_gemm_pitch32(lda, ldb));
  return v;
}

// Grouped launch (mxk_gemm_grouped): the default geometry, phase 0; band0
// is the band of the first table entry and is only what the record shows
// (the kernel takes each problem's band from the table); pitch32 covers
// every A and B pitch of the table.
static inline mx_gemm_variant mx_gemm_select_grouped(const mx_gemm_knobs& k,
                                                     int is_fp32, int beta_one,
                                                     int trans_a, int trans_b,
                                                     int band0, bool pitch32) {
  mx_gemm_variant v = {is_fp32 ? 1 : 0, beta_one ? 1 : 0, 16, 128, 2, 2, 0,
                       trans_a ? 1 : 0, trans_b ? 1 : 0, 0, 1, band0, 0};
  v.PIPE = mx_gemm_pipelined(k, v.T, v.BK, pitch32);
  return v;
}

// Fused transpose/add epilogue (mxk_sgemm_tn_epilogue): the fp32 default
// geometry on the two-barrier loop, supertiled bands of 8, no k-phase
// stagger, whatever the MARLIN_GEMM_* knobs say.
static inline mx_gemm_variant mx_gemm_select_epilogue(int64_t N) {
  const int64_t nbn = N / 128;
  return {1, 0, 16, 128, 2, 2, 0, 0, 0, 1, 0, nbn < 8 ? (int)nbn : 8, 0};
}

// ---------------------------------------------------------------------------
// The closed list of instantiations the library contains: f is called with
// one mx_gemm_inst per kernel. kernels.hip dispatches over this list, so it
// compiles these kernels and no others; the selections above never leave it
// (the check program sweeps them).
//   per (type, beta, loop): the four op forms, plain and grouped, in the
//   default geometry, and bk32 NN            2 * 2 * 2 * (8 + 1) = 72
//   fp64 bm256 NN per (beta, loop)                                  4
//   the fused epilogue                                              1
template <int T_, int BETA_, int BK_, int BM_, int WM_, int WN_, int PIPE_,
          int TA_, int TB_, int EPI_, int GRP_>
struct mx_gemm_inst {
  static constexpr int T = T_, BETA = BETA_, BK = BK_, BM = BM_, WM = WM_,
                       WN = WN_, PIPE = PIPE_, TA = TA_, TB = TB_,
                       EPI = EPI_, GRP = GRP_;
  static constexpr mx_gemm_variant variant() {
    return {T, BETA, BK, BM, WM, WN, PIPE, TA, TB, EPI, GRP, 0, 0};
  }
};

template <class F>
static inline void mx_each01(F&& f) {
  f(std::integral_constant<int, 0>{});
  f(std::integral_constant<int, 1>{});
}

template <class F>
static inline void mx_gemm_for_each_instantiation(F&& f) {
  mx_each01([&](auto t) { mx_each01([&](auto beta) { mx_each01([&](auto pipe) {
    constexpr int T = decltype(t)::value, B = decltype(beta)::value,
                  P = decltype(pipe)::value;
    mx_each01([&](auto ta) { mx_each01([&](auto tb) { mx_each01([&](auto grp) {
      f(mx_gemm_inst<T, B, 16, 128, 2, 2, P, decltype(ta)::value,
                     decltype(tb)::value, 0, decltype(grp)::value>{});
    }); }); });
    f(mx_gemm_inst<T, B, 32, 128, 2, 4, P, 0, 0, 0, 0>{});
    if constexpr (T == 0) f(mx_gemm_inst<0, B, 16, 256, 4, 2, P, 0, 0, 0, 0>{});
  }); }); });
  f(mx_gemm_inst<1, 0, 16, 128, 2, 2, 0, 0, 0, 1, 0>{});
}

static inline std::vector<mx_gemm_variant> mx_gemm_instantiations() {
  std::vector<mx_gemm_variant> out;
  mx_gemm_for_each_instantiation(
      [&](auto i) { out.push_back(decltype(i)::variant()); });
  return out;
}

#endif  // MARLIN_GEMM_LAUNCH_POLICY_H
