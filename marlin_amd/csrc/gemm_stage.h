// gemm_stage.h — the LDS staging layout of the GEMM kernels, stated once:
// which 16 source bytes each lane of each wave DMAs for each piece of an
// operand tile, where they land in LDS, and which LDS element a fragment
// read takes. Integer arithmetic only and nothing from HIP, so a plain
// CPU program can prove that the DMA image and the fragment reads agree
// (tests/test_gemm_stage_layout.py). The includer may define STAGE_FN as
// the function qualifier (kernels.hip: __device__ __forceinline__).
#ifndef MARLIN_GEMM_STAGE_H
#define MARLIN_GEMM_STAGE_H

#include <stdint.h>

#ifndef STAGE_FN
#define STAGE_FN inline
#endif

// An operand tile is D (tile dimension d: row of op(A), column of op(B))
// by BK (k), loaded by NWAVES waves of 64 lanes, 16 bytes (E elements)
// per lane and piece. A "run" is a contiguous line of the stored matrix:
// source element = X[run * ld + along].
//
//   R  (ALONG_K = false) runs follow d: element (d, kk) is at run
//      kbase + kk, along d0 + d. LDS image [BK][D]; the 16-byte chunks of
//      a column are XORed with 8 (fp32: 4) where kk is odd. A piece is
//      64/(D/E) whole columns, or one 1 KiB part of a column of >= 1 KiB.
//      op(A) = A and op(B) = B^T.
//   K  (ALONG_K = true) runs follow k: element (d, kk) is at run d0 + d,
//      along kbase + kk. LDS image [D][BK]; the chunks of column d are
//      XORed with key(d) (none for fp32 at BK = 32). A piece is 64/(BK/E)
//      whole columns. op(B) = B and op(A) = A^T.
//
// glds forces a lane-linear LDS image (piece base + lane * 16 bytes), so
// both swizzles are applied to the lane's SOURCE address; each permutes
// 16-byte chunks within one 128-byte run, so HBM coalescing is unchanged.
// The MFMA lane map varies d by lane & 15 and kk by lane >> 4 for both
// operands, so the bank behaviour of a scheme is the same whichever
// operand uses it: R reads are conflict-free per 16-lane group with groups
// shifted by 32 banks; K reads hit 32 distinct banks per ds_read_b64 group
// (fp32, banks mod 32 for b32 reads: 2-way worst case). Without the
// swizzles the K reads measured 8-way conflicts, 88% of LDS cycles
// (profiles/r01_pmc_sq_pre_swizzle.csv vs r01_pmc_sq_post_swizzle.csv).
struct stage_piece {
    int c;           // wave-uniform: first run of the piece within the tile
    int lane_run;    // this lane's run, relative to c
    int lane_along;  // this lane's first element along the run (swizzled)
    int lds;         // wave-uniform: LDS element offset of the piece
};

template <typename T, bool ALONG_K, int D, int BK, int NWAVES>
struct gemm_stage {
    static constexpr int E = 16 / (int)sizeof(T);    // elements per chunk
    static constexpr int RUN = ALONG_K ? BK : D;     // tile elements per run
    static constexpr int RUNS = ALONG_K ? D : BK;    // runs per tile
    static constexpr int CH = RUN / E;               // chunks per run
    static constexpr int CPC = CH > 64 ? CH / 64 : 1;    // pieces per run
    static constexpr int RPP = CH < 64 ? 64 / CH : 1;    // runs per piece
    static constexpr int PIECES = RUNS * CPC / RPP / NWAVES;  // per wave, tile
    static_assert(PIECES * NWAVES * RPP == RUNS * CPC && CH * E == RUN &&
                  (CH >= 64 ? CH % 64 : 64 % CH) == 0,
                  "the waves' 1 KiB pieces tile the operand exactly");
    static_assert(ALONG_K ? CPC == 1 : true, "a k-run is shorter than 1 KiB");

    // chunk XOR key of a run: R keys on the parity of kk, K on d
    STAGE_FN static int key(int run) {
        if constexpr (!ALONG_K) return (run & 1) << (E == 2 ? 3 : 2);
        else if constexpr (E == 2) return (run >> (BK == 16 ? 1 : 0)) & (CH - 1);
        else if constexpr (BK == 16) return (run >> 1) & 3;
        else return 0;
    }

    // piece i of wave w, as lane `lane` sees it
    STAGE_FN static stage_piece piece(int w, int i, int lane) {
        const int q = w * PIECES + i;
        const int c = q / CPC * RPP, part = (q - q / CPC * CPC) * 64 * E;
        const int lane_run = lane / CH;
        return {c, lane_run, part + ((lane % CH) ^ key(c + lane_run)) * E,
                c * RUN + part};
    }
    // tile coordinates of the first of the E elements that lane loads
    STAGE_FN static int src_d(const stage_piece& p) {
        return ALONG_K ? p.c + p.lane_run : p.lane_along;
    }
    STAGE_FN static int src_kk(const stage_piece& p) {
        return ALONG_K ? p.lane_along : p.c + p.lane_run;
    }

    // Source address of a lane's 16 bytes = X + origin + uni + lane: the
    // tile's first element (tile at d0 of the d axis, kbase of k), a
    // wave-uniform piece offset and a per-lane offset that holds the
    // swizzle and does not depend on the tile. The lane part fits 32 bits
    // for every pitch below 2^26 elements (at most 15 runs plus 1 KiB).
    STAGE_FN static int64_t origin_elems(int64_t ld, int64_t d0, int64_t kbase) {
        return ALONG_K ? d0 * ld + kbase : kbase * ld + d0;
    }
    STAGE_FN static int64_t uni_bytes(const stage_piece& p, int64_t ld) {
        return (int64_t)p.c * ld * (int64_t)sizeof(T);
    }
    STAGE_FN static int64_t lane_bytes(const stage_piece& p, int64_t ld) {
        return ((int64_t)p.lane_run * ld + p.lane_along) * (int64_t)sizeof(T);
    }

    // LDS element a fragment read of tile element (d, kk) takes
    STAGE_FN static int frag(int d, int kk) {
        const int run = ALONG_K ? d : kk, along = ALONG_K ? kk : d;
        return run * RUN + (((along >> (E == 2 ? 1 : 2)) ^ key(run)) * E)
               + (along & (E - 1));
    }
};

template <typename T, int D, int BK, int NWAVES>
using stage_r = gemm_stage<T, false, D, BK, NWAVES>;
template <typename T, int D, int BK, int NWAVES>
using stage_k = gemm_stage<T, true, D, BK, NWAVES>;

#endif  // MARLIN_GEMM_STAGE_H
