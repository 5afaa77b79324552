// Stand-alone host program (test fixture, never shipped): replays on the
// CPU the DMA that stages one operand tile of the GEMM kernels into LDS,
// for every (type, scheme, geometry) the kernels instantiate, using the
// kernels' own arithmetic (marlin_amd/csrc/gemm_stage.h), and checks that
// the image is a bijection of the tile, that the fragment reads find what
// the DMA put there, and that the source addresses are aligned and
// decompose as the pipelined loop assumes. Built with
// -fsanitize=address,undefined by tests/test_gemm_stage_layout.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gemm_stage.h"

#define REQUIRE(cond)                                                     \
  do {                                                                    \
    if (!(cond)) {                                                        \
      printf("FAIL %s line %d: %s\n", what, __LINE__, #cond);             \
      return 1;                                                           \
    }                                                                     \
  } while (0)

// One scheme instance S staging a D x BK tile of element size ES with NW
// waves; along_k tells which axis the source runs follow.
template <class S, int ES, bool ALONG_K, int D, int BK, int NW>
static int check_scheme(const char* what) {
  constexpr int E = 16 / ES;
  REQUIRE(S::E == E);
  // every wave moves PIECES KiB and together they move the tile
  REQUIRE((int64_t)S::PIECES * NW * 1024 == (int64_t)D * BK * ES);

  std::vector<int> written(D * BK, 0);           // per LDS slot
  std::vector<int> slot_of(D * BK, -1);          // [d * BK + kk] -> slot
  for (int w = 0; w < NW; w++)
    for (int i = 0; i < S::PIECES; i++)
      for (int lane = 0; lane < 64; lane++) {
        const stage_piece p = S::piece(w, i, lane);
        // wave-uniform parts must not depend on the lane
        const stage_piece p0 = S::piece(w, i, 0);
        REQUIRE(p.c == p0.c && p.lds == p0.lds);
        const int d = S::src_d(p), kk = S::src_kk(p);
        for (int e = 0; e < E; e++) {
          const int de = ALONG_K ? d : d + e, ke = ALONG_K ? kk + e : kk;
          // glds: LDS destination = piece base + lane * 16 bytes
          const int slot = p.lds + lane * E + e;
          REQUIRE(de >= 0 && de < D && ke >= 0 && ke < BK);
          REQUIRE(slot >= 0 && slot < D * BK);
          written[slot]++;
          REQUIRE(slot_of[de * BK + ke] == -1);  // loaded exactly once
          slot_of[de * BK + ke] = slot;
        }
      }
  for (int s = 0; s < D * BK; s++) REQUIRE(written[s] == 1);
  for (int d = 0; d < D; d++)
    for (int kk = 0; kk < BK; kk++) {
      REQUIRE(slot_of[d * BK + kk] >= 0);
      REQUIRE(S::frag(d, kk) == slot_of[d * BK + kk]);
    }

  // source addresses, for a tile away from the origin: 16-byte aligned
  // for any pitch that is a multiple of 16 bytes, and origin + uniform +
  // 32-bit lane offset is the direct address up to the largest pitch the
  // launcher admits to the pipelined loop
  const int64_t d0 = 3 * (int64_t)D, kbase = 5 * (int64_t)BK;
  const int64_t pitches[] = {8 * (int64_t)D, 8 * (int64_t)D + E,
                             1000003 * (int64_t)E,
                             ((int64_t)1 << 26) - E};
  for (int64_t ld : pitches) {
    REQUIRE(ld % E == 0 && ld < ((int64_t)1 << 26));
    const int64_t origin = S::origin_elems(ld, d0, kbase) * ES;
    for (int w = 0; w < NW; w++)
      for (int i = 0; i < S::PIECES; i++)
        for (int lane = 0; lane < 64; lane++) {
          const stage_piece p = S::piece(w, i, lane);
          const int64_t d = d0 + S::src_d(p), k = kbase + S::src_kk(p);
          const int64_t direct = (ALONG_K ? d * ld + k : k * ld + d) * ES;
          const int64_t lane_off = S::lane_bytes(p, ld);
          REQUIRE(direct % 16 == 0);
          REQUIRE(lane_off >= 0 && lane_off < ((int64_t)1 << 32));
          REQUIRE(origin + S::uni_bytes(p, ld) + (int64_t)(uint32_t)lane_off
                  == direct);
        }
  }
  return 0;
}

// One kernel geometry: op(A) BM x BK and op(B) 128 x BK, the scheme of
// each chosen by the form as the kernel chooses it.
template <typename T, int BK, int BM, int NW, int TA, int TB>
static int check_geometry(const char* what, int* combos) {
  constexpr int ES = (int)sizeof(T);
  int rc = TA ? check_scheme<stage_k<T, BM, BK, NW>, ES, true, BM, BK, NW>(what)
              : check_scheme<stage_r<T, BM, BK, NW>, ES, false, BM, BK, NW>(what);
  if (rc) return rc;
  rc = TB ? check_scheme<stage_r<T, 128, BK, NW>, ES, false, 128, BK, NW>(what)
          : check_scheme<stage_k<T, 128, BK, NW>, ES, true, 128, BK, NW>(what);
  if (rc) return rc;
  // the counted s_waitcnt vmcnt of both loops waits for one tile's pieces
  // of this wave: A's plus B's, i.e. this wave's share of both tiles
  constexpr int PA = TA ? stage_k<T, BM, BK, NW>::PIECES
                        : stage_r<T, BM, BK, NW>::PIECES;
  constexpr int PB = TB ? stage_r<T, 128, BK, NW>::PIECES
                        : stage_k<T, 128, BK, NW>::PIECES;
  REQUIRE((PA + PB) * NW * 1024 == (BM + 128) * BK * ES);
  *combos += 2;
  return 0;
}

int main() {
  int combos = 0;
  // every (type, geometry, form) mxk_gemm_op and mxk_sgemm_tn_epilogue
  // launch: the default geometry in all four forms, bk32, bm256 (fp64)
  if (check_geometry<double, 16, 128, 4, 0, 0>("f64 default NN", &combos) ||
      check_geometry<double, 16, 128, 4, 1, 0>("f64 default TN", &combos) ||
      check_geometry<double, 16, 128, 4, 0, 1>("f64 default NT", &combos) ||
      check_geometry<double, 16, 128, 4, 1, 1>("f64 default TT", &combos) ||
      check_geometry<float, 16, 128, 4, 0, 0>("f32 default NN", &combos) ||
      check_geometry<float, 16, 128, 4, 1, 0>("f32 default TN", &combos) ||
      check_geometry<float, 16, 128, 4, 0, 1>("f32 default NT", &combos) ||
      check_geometry<float, 16, 128, 4, 1, 1>("f32 default TT", &combos) ||
      check_geometry<double, 32, 128, 8, 0, 0>("f64 bk32", &combos) ||
      check_geometry<float, 32, 128, 8, 0, 0>("f32 bk32", &combos) ||
      check_geometry<double, 16, 256, 8, 0, 0>("f64 bm256", &combos))
    return 1;
  printf("gemm_stage OK %d\n", combos);
  return 0;
}
