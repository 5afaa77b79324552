// Stand-alone host program (test fixture, never shipped): drives the
// split-K slicing policy (marlin_amd/csrc/gemm_splitk_plan.h) over a sweep
// of (type, m, n, k, S, CU count). tests/test_gemm_splitk_plan.py builds it
// under -fsanitize=address,undefined: the slice list is written into a heap
// block of exactly the clamped count, and every sum below would trap on a
// signed overflow. It checks the properties the entry relies on and prints
// one line per auto decision for the Python restatement to compare:
//   const MX_SPLITK_MIN_KSTEPS <value>
//   const MX_SPLITK_FILL_DIV <value>
//   auto <is_fp32> <m> <n> <k> <cus> <S>
//   slices <k> <S asked> <S effective> <first len> <last len>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gemm_splitk_plan.h"

static long g_checks = 0;
#define REQUIRE(x)                                                    \
  do {                                                                \
    g_checks++;                                                       \
    if (!(x)) {                                                       \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);             \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static int check_slices(int64_t k, int S) {
  const int64_t steps = k / 16;
  const int eff = mx_splitk_slices(k, S, nullptr);
  // clamped to [1, k / 16]
  REQUIRE(eff >= 1);
  REQUIRE(steps < 1 || eff <= steps);
  REQUIRE(eff == (S < 1 ? 1 : S) || eff == (steps < 1 ? 1 : steps));
  REQUIRE(eff <= (S < 1 ? 1 : S));
  // a huge clamped count is only counted, not materialised
  if (eff > (1 << 20)) return 0;
  std::vector<mx_splitk_slice> out((size_t)eff);
  REQUIRE(mx_splitk_slices(k, S, out.data()) == eff);
  int64_t at = 0;
  for (int i = 0; i < eff; i++) {
    REQUIRE(out[i].start == at);                  // contiguous, ascending
    REQUIRE(steps < 1 || out[i].len >= 1);
    if (i > 0) {
      REQUIRE(out[i].len <= out[i - 1].len);      // longer first
      REQUIRE(out[0].len - out[i].len <= 1);      // differ by at most one
    }
    at += out[i].len;
  }
  REQUIRE(at == (steps < 0 ? 0 : steps));         // cover [0, k / 16) exactly
  printf("slices %lld %d %d %lld %lld\n", (long long)k, S, eff,
         (long long)out[0].len, (long long)out[eff - 1].len);
  return 0;
}

static int check_auto(int is_fp32, int64_t m, int64_t n, int64_t k, int cus,
                      int* s_out) {
  const int S = mx_splitk_auto(is_fp32, m, n, k, cus);
  const int64_t resident = mx_splitk_resident(is_fp32, cus);
  const int64_t tiles = (m / 128) * (n / 128);    // the sweep keeps it small
  REQUIRE(S >= 1);
  if (tiles >= resident) REQUIRE(S == 1);
  if (S > 1) {
    REQUIRE(S * tiles <= resident);               // one wave at the most
    std::vector<mx_splitk_slice> out((size_t)S);
    REQUIRE(mx_splitk_slices(k, S, out.data()) == S);   // never clamped
    for (const mx_splitk_slice& s : out)
      REQUIRE(s.len >= MX_SPLITK_MIN_KSTEPS);
  }
  printf("auto %d %lld %lld %lld %d %d\n", is_fp32, (long long)m,
         (long long)n, (long long)k, cus, S);
  *s_out = S;
  return 0;
}

int main() {
  printf("const MX_SPLITK_MIN_KSTEPS %lld\n", (long long)MX_SPLITK_MIN_KSTEPS);
  printf("const MX_SPLITK_FILL_DIV %lld\n", (long long)MX_SPLITK_FILL_DIV);
  REQUIRE(MX_SPLITK_MIN_KSTEPS >= 1);
  REQUIRE(MX_SPLITK_FILL_DIV >= 1);

  // k = 0 and k below one step: one (empty) slice, whatever is asked
  const int64_t ks[] = {0, 16, 32, 48, 112, 128, 1008, 4096, 65536 + 16,
                        (int64_t)1 << 20, ((int64_t)1 << 31) * 16};
  const int asks[] = {0, 1, 2, 3, 5, 7, 8, 64, 511, 512, 1024, 100000,
                      INT32_MAX};
  for (int64_t k : ks)
    for (int S : asks)
      if (check_slices(k, S)) return 1;
  // every (steps, S) pair of a small square: all remainders
  for (int64_t steps = 1; steps <= 40; steps++)
    for (int S = 1; S <= 44; S++)
      if (check_slices(steps * 16, S)) return 1;

  const int64_t dims[] = {128, 256, 512, 1024, 2048, 4096, 8192, 128 * 1000};
  const int cu_counts[] = {256, 304, 64, 1};
  for (int is_fp32 = 0; is_fp32 < 2; is_fp32++)
    for (int cus : cu_counts)
      for (int64_t m : dims)
        for (int64_t n : dims) {
          int prev = 1;
          for (int64_t k : ks) {                  // ascending: S monotone in k
            int S = 0;
            if (check_auto(is_fp32, m, n, k, cus, &S)) return 1;
            REQUIRE(S >= prev);
            prev = S;
          }
        }
  // dims whose tile product would overflow 64 bits: still S = 1, no trap
  int S = 0;
  const int64_t huge = ((int64_t)1 << 40) * 128;
  REQUIRE(mx_splitk_auto(0, huge, huge, 4096, 256) == 1);
  REQUIRE(mx_splitk_auto(1, 128, huge, ((int64_t)1 << 31) * 16, 256) == 1);
  // empty and degenerate inputs
  REQUIRE(mx_splitk_auto(0, 0, 128, 4096, 256) == 1);
  REQUIRE(mx_splitk_auto(0, 128, 128, 0, 256) == 1);
  REQUIRE(mx_splitk_auto(0, 128, 128, 4096, 0) == 1);
  (void)S;

  printf("gemm_splitk_plan OK %ld checks\n", g_checks);
  return 0;
}
