// gemm_splitk_plan.h — host-only integer code of the split-K GEMM entry
// (mx_gemm_device_splitk): how many k-slices a product is cut into and
// where each slice starts. No HIP here, so a plain CPU program can check it
// (tests/test_gemm_splitk_plan.py builds one under AddressSanitizer).
//
// Everything is counted in k-steps of 16, the kernel's BK: a slice is a
// whole number of steps, so each slice is a legal problem of the grouped
// entry (k a multiple of 16) and its operand offset a multiple of 16 bytes.
#ifndef MARLIN_GEMM_SPLITK_PLAN_H
#define MARLIN_GEMM_SPLITK_PLAN_H

#include <stdint.h>

// The two measured constants of the auto policy, fixed by the sweep of
// profiles/gemm_splitk.md (fp64 / fp32, TN / NN, 1..256 tiles, k = 512..2^20,
// explicit S in powers of two against the unsplit launch, 256 CUs).
//
// MX_SPLITK_FILL_DIV: auto fills the device to resident / 2 blocks, that is
// one block per CU in fp64 and two in fp32, not to the resident count.
// A doubling of S up to that fill bought 1.9x (median, k >= 32768); the
// last doubling, to the resident count, ranged from -63% to +13% in fp64
// (above +2% only from k = 2^19 on) and from -68% to +5% in fp32, and in
// fp64 at 256 tiles S = 2 lost to the unsplit launch at every k up to 8192.
//
// MX_SPLITK_MIN_KSTEPS: fewest k-steps auto leaves a slice. The smallest
// power of two at which, with that fill, no swept point where auto picks
// S > 1 ran slower than plain beyond the plain arm's own spread. At 32 and
// 64 one point did by 1% (fp32, 256 tiles, TN, k = 2048, S = 2: 0.174 ->
// 0.176 ms); at 16 the fp32 256-tile k = 512 points lost 25-28%: the reduce
// pass over S * m * n elements costs more than two short slices save. The
// price is paid at few tiles and short k, where slices of 4-8 steps still
// won; a single constant cannot take those and keep the 256-tile points.
constexpr int64_t MX_SPLITK_FILL_DIV = 2;
constexpr int64_t MX_SPLITK_MIN_KSTEPS = 128;

// Blocks of the default GEMM geometry the device holds at once: 2 per CU in
// fp64, 4 in fp32 (the occupancy column of profiles/gemm_grouped.md).
static inline int64_t mx_splitk_resident(int is_fp32, int cus) {
  return (int64_t)(cus > 0 ? cus : 0) * (is_fp32 ? 4 : 2);
}

// The slice count of slices == 0 (auto). A launch whose tiles reach the fill
// target is left alone; otherwise k is cut until the S * tiles blocks reach
// it (never more than one wave of resident blocks, which also bounds the
// workspace by resident * 128 * 128 elements), as long as every slice
// keeps MX_SPLITK_MIN_KSTEPS steps. m, n, k are the padded dims.
static inline int mx_splitk_auto(int is_fp32, int64_t m, int64_t n, int64_t k,
                                 int cus) {
  const int64_t target = mx_splitk_resident(is_fp32, cus) / MX_SPLITK_FILL_DIV;
  const int64_t nbm = m / 128, nbn = n / 128;
  if (nbm <= 0 || nbn <= 0 || k <= 0) return 1;
  // tiles >= target without forming a product that could overflow
  if (nbm >= target || nbn >= target) return 1;
  const int64_t tiles = nbm * nbn;
  if (tiles >= target) return 1;
  const int64_t fill = target / tiles;
  const int64_t deep = (k / 16) / MX_SPLITK_MIN_KSTEPS;
  const int64_t s = fill < deep ? fill : deep;
  return s < 1 ? 1 : (int)s;
}

struct mx_splitk_slice {
  int64_t start, len;      // k-steps: the slice covers k in 16*[start, start+len)
};

// Cuts the k / 16 steps into S slices, S clamped to [1, k / 16] (1 when k
// has no step at all): contiguous, ascending, lengths as even as possible
// with the longer slices first, so they differ by at most one step. out
// holds at least the clamped count; out == NULL only counts. Returns the
// clamped S.
static inline int mx_splitk_slices(int64_t k, int S, mx_splitk_slice* out) {
  const int64_t steps = k > 0 ? k / 16 : 0;
  int64_t s = S < 1 ? 1 : S;
  if (s > steps) s = steps < 1 ? 1 : steps;
  if (!out) return (int)s;
  const int64_t base = steps / s, longer = steps % s;
  int64_t start = 0;
  for (int64_t i = 0; i < s; i++) {
    const int64_t len = base + (i < longer ? 1 : 0);
    out[i] = {start, len};
    start += len;
  }
  return (int)s;
}

#endif  // MARLIN_GEMM_SPLITK_PLAN_H
