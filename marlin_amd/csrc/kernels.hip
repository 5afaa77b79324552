// kernels.hip — hand-written CDNA4 (gfx950) kernels for the MI355X-native
// block-matrix multiply engine.
//
// This is the MI355X replacement of the reference's per-block compute:
// SubMatrix.multiply (SubMatrix.scala:87-105, Breeze * -> netlib JNI dgemm)
// and the reduceByKey partial-sum add (SubMatrix.scala:41-50) — the add is
// folded into the MFMA accumulator (BETA template parameter), so the
// reference's k-partial C tiles never materialise.
//
// Design:
//   - v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 tiles, 64-wide waves.
//   - 128x128 block tile, BK=16 K-step, 256 threads = 4 waves in a 2x2
//     wave grid, each wave owns a 64x64 sub-tile = 4x4 MFMA fragments.
//   - A/B staged through LDS with 16-byte global_load_lds (direct HBM->LDS
//     DMA), double-buffered, the next tile's DMA always a full k-step
//     ahead. The k-loop is software-pipelined across tiles: ONE raw
//     s_barrier per k-step, placed before the last quad's MFMAs, which
//     cover the next DMA issue and the next tile's first fragment reads;
//     DMA addresses are running wave-uniform pointers + constant lane
//     offsets. The earlier two-barrier loop stays selectable
//     (MARLIN_GEMM_LOOP=twobar) and is still fp32/BK=16's default.
//   - The staging layout (DMA source per lane, LDS image, swizzles,
//     fragment reads) is stated once, in gemm_stage.h, for every type,
//     geometry and operand form; both loops go through it. The fused
//     transpose/add epilogue of config 5 is the EPI parameter of the one
//     GEMM template.
//   - Many small products run as ONE launch over the union of their tiles
//     (GRP parameter of the same template, table of gemm_group_plan.h):
//     a block finds its problem in the prologue, then runs the same code.
//   - All matrices COLUMN-MAJOR with padded leading dims (multiples of the
//     tile) — the host pads, so the kernel has no edge paths.
//   - Grid is remapped into column bands so the ~512 resident blocks share
//     A-row and B-col panels in L2 (XCD-friendly; blocks land on XCD b%8).
//
// fp64 peak on gfx950: 256 CU x 4 SIMD x 32 FLOP/clk x 2.4 GHz = 78.6 TF
// (v_mfma_f64_16x16x4_f64 = 2048 flop / 64 cyc / SIMD).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "kernels.h"                // the launchers' prototypes
#include "gemm_group_plan.h"        // mx_group_entry (the device table)
#include "gemm_launch_policy.h"     // which instantiation a launch runs

typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

#define DEVFN __device__ __forceinline__

// ---------------------------------------------------------------------------
// MFMA wrappers (16x16x4 shape; one A/B element per lane):
//   a: A[row = lane&15][k = lane>>4]      (A is m x k)
//   b: B[k = lane>>4][col = lane&15]      (B is k x n)
//   acc (4 per lane): D[row = 4*j + (lane>>4)][col = lane&15]
//     (measured on MI355X — tools_dev/debug_mfma.py; the f64/f32 16x16x4
//      "SGEMM-class" row map is reg-major, unlike the bf16 16x16x32 map)
DEVFN v4d mfma_16x16x4(double a, double b, v4d c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
DEVFN v4f mfma_16x16x4(float a, float b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <typename T> struct acc_t;
template <> struct acc_t<double> { using type = v4d; };
template <> struct acc_t<float>  { using type = v4f; };

DEVFN void glds16(const void* g, void* lds) {
    // 16-byte direct-to-LDS DMA; LDS dest = wave-uniform base + lane*16.
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)g,
        (__attribute__((address_space(3))) uint32_t*)lds, 16, 0, 0);
}

// Block-uniform loads of the grouped table: the value is the same in every
// lane, and readfirstlane says so, which keeps it in scalar registers.
DEVFN int32_t sload(const int32_t* p) {
    return __builtin_amdgcn_readfirstlane(*p);
}
DEVFN int64_t sload(const int64_t* p) {
    const int64_t v = *p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
DEVFN const void* sload_ptr(const void* const* p) {
    return (const void*)(uintptr_t)sload((const int64_t*)p);
}
DEVFN void* sload_ptr(void* const* p) {
    return (void*)(uintptr_t)sload((const int64_t*)p);
}

// The LDS staging layout (schemes R and K: DMA source per lane, LDS image,
// swizzles, fragment reads) is stated once, in gemm_stage.h.
#define STAGE_FN DEVFN
#include "gemm_stage.h"

// One wave's DMA of its pieces of one operand tile into the LDS image at
// lds[img ...]; origin = the tile's first element (S::origin_elems).
template <class S, typename T>
DEVFN void issue_pieces(const char* origin, int64_t ld, T* lds, int img,
                        int wid, int lane) {
    #pragma unroll
    for (int i = 0; i < S::PIECES; i++) {
        const stage_piece p = S::piece(wid, i, lane);
        glds16(origin + S::uni_bytes(p, ld) + S::lane_bytes(p, ld),
               &lds[img + p.lds]);
    }
}

// Block remap: column bands of |band| block-cols, split into 8x8 block
// supertiles (band == 8 normally). Within a supertile the 8 blocks landing
// on one XCD (dispatch places block b on XCD b%8, and all the stride terms
// are multiples of 8) form one COLUMN: each XCD's L2 re-reads one B tile 8x
// and a contiguous 8-row A panel. band < 0: plain bm-fastest bands (A/B
// comparison fallback).
DEVFN void block_remap(int id, int nbn, int nbm, int band, int& bm, int& bn) {
    int abands = band < 0 ? -band : band;
    int per_band = nbm * abands;
    int b0 = id / per_band;
    int w = id - b0 * per_band;
    int first_bn = b0 * abands;
    int bw = min(abands, nbn - first_bn);
    if (band < 0) {                      // plain band order
        bn = first_bn + w / nbm;
        bm = w % nbm;
    } else {                             // supertiled band order
        int sh = 8 * bw;
        int t = w / sh, l = w - t * sh;
        bm = t * 8 + l / bw;
        bn = first_bn + l % bw;
    }
}

// ---------------------------------------------------------------------------
// Main GEMM kernel. C[MxN] (+)= A[MxK] * B[KxN], col-major, padded pitches:
// M a multiple of BM, N of 128, K of BK (the host pads to 128/16; the
// launcher only selects BK=32 / BM=256 configs when the padded dims
// divide). BETA == 1 accumulates into C (the SubMatrix.add combiner,
// folded into the MFMA accumulator chain).
//
// Geometry template: BN=128 fixed; wave grid WM x WN, wave tile
// (BM/WM) x (128/WN). Production config (measured winner): BK=16,
// BM=128, 2x2 waves = two 256-thread blocks per CU at 64 KB LDS each,
// 2 waves/SIMD. Alternates kept for re-evaluation behind MARLIN_GEMM_CFG:
// bk32 (512-thread, half barrier rate, 58.6 TF) and bm256 (256x128 tile,
// half DMA-per-flop, 63.6 TF) — both measured slower than the default's
// 67.9 TF at 20000^3 with the two-barrier loop. With the pipelined loop
// the default reaches 70.4 and bk32 62.6 at 20000^3, and at 20480^3 (the
// nearest size a 256-row tile divides) the default 71.4 vs bm256 70.2:
// the ranking holds (profiles/r03_pipelined_loop.md). With the fragment
// reads pinned and the steady state unrolled for a constant buffer the
// default reaches 73.6 and bk32 69.6 at 20000^3; at 20480^3 bm256 (75.6)
// is then 0.85% ahead of the default (75.0), which stays the default:
// 20000 pads to 20096 rows, which 256 does not divide
// (profiles/r05_loop_waits.md).
//
// PIPE selects the k-loop (both accumulate in the same order, so their
// results are bit-identical):
//   0  two barriers per k-step, DMA addresses rebuilt from kt each step
//      (MARLIN_GEMM_LOOP=twobar);
//   1  software-pipelined across tiles: one barrier per k-step, placed
//      ahead of the last quad's MFMAs, which cover the next-but-one
//      tile's DMA issue and the next tile's quad-0 fragment reads; DMA
//      sources are wave-uniform running pointers plus loop-invariant
//      32-bit lane offsets (see the comment above that loop).
//
// TA / TB select op(A) = A^T / op(B) = B^T: A is then stored k x m with
// lda the k-run pitch and staged by scheme K with d = row; B is stored
// n x k and staged by scheme R with d = col. A transposed operand is thus
// staged exactly as the other operand is untransposed; both schemes move
// the same number of pieces per wave and tile, so the vmcnt counts do not
// depend on the form. The MFMA operand meaning stays
// a = opA[row = l15][k = l4], b = opB[k = l4][col = l15], so every C
// element sees the accumulation chain NN gives on a materialised
// transpose. The launcher instantiates the transposed forms in the
// default geometry only.
//
// EPI selects the epilogue: EPI_STORE writes C (m x n); EPI_TN_ADD writes
// C_out[n x m] = (A*B)^T (+ addC) — see the end of the kernel.
enum { EPI_STORE = 0, EPI_TN_ADD = 1 };

// GRP = 1 is the grouped launch (mx_gemm_device_grouped): the grid is the
// union of the tiles of many problems and `grp` is the device table of
// gemm_group_plan.h (entries, then tile_start); the per-launch scalars are
// unused but for nbm_, which carries the entry count. The prologue finds
// the block's problem, loads its descriptor and takes the problem-local
// block id; from there the code below runs unchanged on that problem's
// A, lda, B, ldb, C, ldc, ntiles. Default geometry only, phase 0.
template <typename T, int BETA, int BK, int BM, int WM, int WN, int PIPE,
          int TA = 0, int TB = 0, int EPI = EPI_STORE, int GRP = 0>
__launch_bounds__(WM * WN * 64, 2)
__global__ void gemm_mfma_kernel(int64_t M, int64_t N, int64_t K,
                                 const T* __restrict__ A_, int64_t lda_,
                                 const T* __restrict__ B_, int64_t ldb_,
                                 T* __restrict__ C_, int64_t ldc_,
                                 int nbm_ /* grid rows = M/BM */,
                                 int band_ /* column-band width in blocks */,
                                 int phase_mask /* k-phase stagger mask */,
                                 const T* __restrict__ addC /* EPI_TN_ADD */,
                                 const mx_group_entry* __restrict__ grp) {
    constexpr int BN = 128;
    constexpr int NWAVES = WM * WN;
    constexpr int MT = (BM / WM) / 16;      // 16x16 frags per wave, m
    constexpr int NT = (BN / WN) / 16;      // 16x16 frags per wave, n
    using ACC = typename acc_t<T>::type;
    using SA = std::conditional_t<TA != 0, stage_k<T, BM, BK, NWAVES>,
                                           stage_r<T, BM, BK, NWAVES>>;
    using SB = std::conditional_t<TB != 0, stage_r<T, BN, BK, NWAVES>,
                                           stage_k<T, BN, BK, NWAVES>>;
    constexpr int P = SA::PIECES + SB::PIECES;   // DMA pieces per wave, tile

    const T* __restrict__ A = A_;
    const T* __restrict__ B = B_;
    T* __restrict__ C = C_;
    int64_t lda = lda_, ldb = ldb_, ldc = ldc_;
    int nbm = nbm_, nbn = (int)(N / BN), band = band_;
    int grp_ntiles = 0;
    int id = blockIdx.x;
    if constexpr (GRP != 0) {
        static_assert(BK == 16 && BM == 128 && WM == 2 && WN == 2 &&
                      EPI == EPI_STORE, "grouped: default geometry only");
        // wave-uniform binary search of tile_start (count + 1 entries
        // behind the descriptors) for the problem owning this block
        const int count = nbm_;
        const int32_t* __restrict__ tile_start = (const int32_t*)(grp + count);
        int lo = 0, hi = count - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (sload(&tile_start[mid]) <= id) lo = mid; else hi = mid - 1;
        }
        const mx_group_entry* __restrict__ e = grp + lo;
        A = (const T*)sload_ptr(&e->A);
        B = (const T*)sload_ptr(&e->B);
        C = (T*)sload_ptr(&e->C);
        lda = sload(&e->lda); ldb = sload(&e->ldb); ldc = sload(&e->ldc);
        grp_ntiles = sload(&e->ntiles);
        nbm = sload(&e->nbm); nbn = sload(&e->nbn); band = sload(&e->band);
        id -= sload(&tile_start[lo]);
    }
    int bn, bm;
    block_remap(id, nbn, nbm, band, bm, bn);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;  // wave grid coords (WM x WN)
    const int l15 = lane & 15, l4 = lane >> 4;   // MFMA fragment coords

    // --- LDS: two buffers of each operand's tile image (gemm_stage.h) ---
    __shared__ __align__(16) T sAB[2 * BK * BM + 2 * BN * BK];
    T* As = sAB;                              // [2][BK * BM]
    T* Bs = sAB + 2 * BK * BM;                // [2][BN * BK]

    const int64_t row0 = (int64_t)bm * BM;    // global row of tile
    const int64_t col0 = (int64_t)bn * BN;    // global col of tile

    // C/D row of accumulator element j for this lane (measured per type:
    // tools_dev/debug_mfma.py): f64 16x16x4 is reg-major (l4 + 4j),
    // f32 16x16x4 is contiguous (4*l4 + j).
    constexpr bool REGMAJOR = sizeof(T) == 8;
    const int rbase = REGMAJOR ? l4 : l4 * 4;
    constexpr int rstep = REGMAJOR ? 4 : 1;
    ACC acc[MT][NT];
    if (BETA) {
        #pragma unroll
        for (int mt = 0; mt < MT; mt++)
            #pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                int64_t r = row0 + wm * (MT * 16) + mt * 16 + rbase;
                int64_t cc = col0 + wn * (NT * 16) + nt * 16 + l15;
                const T* cp = C + cc * ldc + r;
                #pragma unroll
                for (int j = 0; j < 4; j++) acc[mt][nt][j] = cp[rstep * j];
            }
    } else {
        #pragma unroll
        for (int mt = 0; mt < MT; mt++)
            #pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = ACC{0};
    }

    const int ntiles = GRP != 0 ? grp_ntiles : (int)(K / BK);
    // k-phase stagger experiment (MARLIN_GEMM_PHASE): blocks matching
    // the mask start their k-loop half-way round (accumulation order
    // rotated per tile — still deterministic run-to-run), so the two
    // blocks sharing a CU do not hit their DMA-wait/barrier windows in
    // sync. Default off (phase_mask 0 = ascending k, reference order).
    const int ph = (phase_mask && (id & phase_mask)) ? (ntiles >> 1) : 0;

    // The halves of a quad: fragments of quad q (k = 4q .. 4q+3) of the
    // tile staged at At/Bt; then the quad's MT x NT MFMAs.
    // (s_setprio(1) around the MFMAs measured -5% — not used)
    auto read_quad = [&](const T* At, const T* Bt, int q, T (&a)[MT],
                         T (&b)[NT]) {
        const int kk = q * 4 + l4;
        #pragma unroll
        for (int mt = 0; mt < MT; mt++)
            a[mt] = At[SA::frag(wm * (MT * 16) + mt * 16 + l15, kk)];
        #pragma unroll
        for (int nt = 0; nt < NT; nt++)
            b[nt] = Bt[SB::frag(wn * (NT * 16) + nt * 16 + l15, kk)];
    };
    auto mfma_quad = [&](const T (&a)[MT], const T (&b)[NT]) {
        #pragma unroll
        for (int mt = 0; mt < MT; mt++)
            #pragma unroll
            for (int nt = 0; nt < NT; nt++)
                acc[mt][nt] = mfma_16x16x4(a[mt], b[nt], acc[mt][nt]);
    };

    if constexpr (!PIPE) {
    auto issue_tile = [&](int kt, int buf) {
        const int64_t kbase = (int64_t)kt * BK;
        issue_pieces<SA>((const char*)(A + SA::origin_elems(lda, row0, kbase)),
                         lda, As, buf * BK * BM, wid, lane);
        issue_pieces<SB>((const char*)(B + SB::origin_elems(ldb, col0, kbase)),
                         ldb, Bs, buf * BN * BK, wid, lane);
    };
    issue_tile(ph, 0);

    // Two barriers per k-step with the next tile's DMA issued EARLY and
    // kept in flight across the first barrier via a counted vmcnt (a
    // single-barrier variant with vmcnt(0)+late issue measured ~1% slower
    // fp64 / 4% slower fp32 - less DMA lead time).
    for (int s = 0; s < ntiles; s++) {
        const int buf = s & 1;
        if (s + 1 < ntiles) {
            int nxt = s + 1 + ph;
            if (nxt >= ntiles) nxt -= ntiles;
            issue_tile(nxt, buf ^ 1);
            // our own current-tile DMAs landed; next tile's stay in flight
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(P) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();        // all waves' tile visible

        const T* At = &As[buf * BK * BM];
        const T* Bt = &Bs[buf * BN * BK];
        #pragma unroll
        for (int q = 0; q < BK / 4; q++) {
            T a[MT], b[NT];
            read_quad(At, Bt, q, a, b);
            mfma_quad(a, b);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();        // readers done before overwrite
    }
    } else {
    // Pipelined loop: every wave hides its own loop-top work. Step s
    // (tile s in buffer s & 1) runs
    //     quads 0 .. Q-2:  MFMAs of quad q, with quad q+1's fragment reads
    //                      pinned behind the first of them (below)
    //     lgkmcnt(0)       quad Q-1's fragments are in registers: this
    //                      wave has finished reading tile s
    //     vmcnt(0)         this wave's pieces of tile s+1 (issued a full
    //                      step ago, the only DMAs outstanding) landed
    //     s_barrier        tile s+1 visible AND tile s's buffer free
    //     read quad 0 of tile s+1; issue tile s+2 into tile s's buffer
    //     MFMAs of quad Q-1 of tile s, with the line above interleaved
    //     behind them (one read, then one DMA piece, per MFMA)
    // so the DMA lead stays one full step and the one barrier does both
    // jobs of the two-barrier loop. The last two steps are peeled (no
    // tile left to issue / to read), which keeps the steady-state body
    // one branch-free block the scheduler hints can order.
    //
    // Every quad is a scheduling region of its own (sched_barrier(0)), and
    // inside it the reads of the next quad sit behind the first MFMAs.
    // Left free, the machine scheduler packed the reads of two quads into
    // one and issued the last of them 0..1 MFMAs ahead of an lgkmcnt(0):
    // twice per step, once right in front of the barrier, every wave sat
    // out an LDS round trip with no MFMA of its own queued. Now no wait of
    // the steady state forces a read younger than RD_TAIL MFMAs
    // (tools_dev/gemm_loop_waits.py prints the distances from the compiled
    // code, tests/test_gemm_loop_waits.py holds them;
    // profiles/r05_loop_waits.md).
    //
    // DMA sources: (wave-uniform running pointer + uniform per-piece
    // offset) + per-lane 32-bit byte offset. The lane offsets hold the
    // XOR swizzle and are loop-invariant; the pointers advance by one
    // tile per issue and are reset where the MARLIN_GEMM_PHASE rotation
    // wraps. The launcher guarantees the lane offsets fit 32 bits.
    constexpr int Q = BK / 4;
    static_assert(Q % 2 == 0, "fragment registers ping-pong per quad");
    // Placement of a quad's MT + NT fragment reads among the previous
    // quad's MT * NT MFMAs: RD_PER reads behind each of the first
    // RD_GROUPS MFMAs, so that at least RD_TAIL MFMAs (4 x 64 cycles, more
    // than an LDS round trip) lie between the last read and the wait in
    // front of the fragments' first use.
    constexpr int RD_TAIL = 4;
    static_assert(MT * NT > RD_TAIL, "a quad needs MFMAs ahead of its tail");
    constexpr int RD_PER = (MT + NT + MT * NT - RD_TAIL - 1) / (MT * NT - RD_TAIL);
    constexpr int RD_GROUPS = (MT + NT + RD_PER - 1) / RD_PER;
    // fp32 starts the reads RD_LEAD MFMAs into the quad: with the reads
    // right behind the first MFMA the BETA=1 A*B^T form needs 129 VGPRs
    // and drops from 4 to 3 waves per SIMD.
    constexpr int RD_LEAD =
        sizeof(T) == 4 ? (MT * NT - RD_GROUPS - RD_TAIL) / 2 : 0;
    // The last quad of a step puts the next tile's quad-0 reads behind its
    // first MFMAs and the DMA pieces behind the following ones. The 8-wave
    // geometries take two reads per MFMA there: bk32 has 8 MFMAs for 6
    // reads, and bm256's reads pair up less once the buffer is a constant,
    // which would take the loop-top wait from 11 MFMAs of distance to 9.
    constexpr int LQ_PER = NWAVES == 8 ? 2 : 1;
    constexpr int LQ_GROUPS = (MT + NT + LQ_PER - 1) / LQ_PER;
    // Steady state unrolled by two steps: the buffer is a constant in each
    // half, so the fragment addresses are loop-invariant VGPR bases with
    // immediate offsets and the DMA m0 values are SGPR constants (34 -> 8
    // non-MFMA VALU and 48 -> 39 SALU instructions per step in the fp64
    // default). One step at run-time parity follows when the steady-state
    // count is odd. Not for fp32 BETA=1 at BK=16: those forms sit at the
    // 128-VGPR limit of 4 waves per SIMD and the hoisted bases cost A^T*B
    // a wave (138 VGPRs).
    constexpr bool UNROLL2 = !(sizeof(T) == 4 && BETA && BK == 16);
    const int swid = __builtin_amdgcn_readfirstlane(wid);
    // These two loops stay in the kernel body: behind a function, struct
    // or lambda the same arithmetic gave the steady-state loop another
    // schedule, and fp64 bk32 measured 0.8% slower
    // (profiles/r04_stage_refactor.md).
    uint32_t a_lane[SA::PIECES], b_lane[SB::PIECES];   // per-lane byte offsets
    int64_t a_uni[SA::PIECES], b_uni[SB::PIECES];      // per-piece uniform offsets
    int a_lds[SA::PIECES], b_lds[SB::PIECES];          // LDS element offsets
    #pragma unroll
    for (int i = 0; i < SA::PIECES; i++) {
        const stage_piece p = SA::piece(swid, i, lane);
        a_lane[i] = (uint32_t)SA::lane_bytes(p, lda);
        a_uni[i] = SA::uni_bytes(p, lda);
        a_lds[i] = p.lds;
    }
    #pragma unroll
    for (int i = 0; i < SB::PIECES; i++) {
        const stage_piece p = SB::piece(swid, i, lane);
        b_lane[i] = (uint32_t)SB::lane_bytes(p, ldb);
        b_uni[i] = SB::uni_bytes(p, ldb);
        b_lds[i] = p.lds;
    }

    // tile 0 and the per-tile step of each running pointer
    const char* const pA0 = (const char*)(A + SA::origin_elems(lda, row0, 0));
    const char* const pB0 = (const char*)(B + SB::origin_elems(ldb, col0, 0));
    const int64_t stepA = SA::origin_elems(lda, 0, BK) * (int64_t)sizeof(T);
    const int64_t stepB = SB::origin_elems(ldb, 0, BK) * (int64_t)sizeof(T);
    const char* pA = pA0 + ph * stepA;       // tile the next issue loads
    const char* pB = pB0 + ph * stepB;
    int kt = ph;
    auto issue_next = [&](int buf) {
        #pragma unroll
        for (int i = 0; i < SA::PIECES; i++)
            glds16(pA + a_uni[i] + a_lane[i], &As[buf * BK * BM + a_lds[i]]);
        #pragma unroll
        for (int i = 0; i < SB::PIECES; i++)
            glds16(pB + b_uni[i] + b_lane[i], &Bs[buf * BN * BK + b_lds[i]]);
        kt++; pA += stepA; pB += stepB;
        if (kt == ntiles) { kt = 0; pA = pA0; pB = pB0; }      // phase wrap
    };

    T fa[2][MT], fb[2][NT];                  // fragments of quad q in [q & 1]
    issue_next(0);
    if (ntiles > 1) {
        issue_next(1);
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(P) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();            // tile 0 visible
    read_quad(As, Bs, 0, fa[0], fb[0]);

    // AHEAD: tiles that follow this step's tile; 2 or more = steady
    // state. bufc: the tile's buffer, an int or an integral_constant.
    auto step = [&](auto bufc, auto ahead) {
        constexpr int AHEAD = decltype(ahead)::value;
        const int buf = bufc;
        const T* At = &As[buf * BK * BM];
        const T* Bt = &Bs[buf * BN * BK];
        #pragma unroll
        for (int q = 0; q + 1 < Q; q++) {
            read_quad(At, Bt, q + 1, fa[(q + 1) & 1], fb[(q + 1) & 1]);
            mfma_quad(fa[q & 1], fb[q & 1]);
            // quad q+1's reads stay in quad q's region, RD_PER behind
            // each of its first MFMAs, and RD_TAIL or more MFMAs follow
            // the last read before the region ends
            if constexpr (RD_LEAD > 0)
                __builtin_amdgcn_sched_group_barrier(0x008, RD_LEAD, 0);
            #pragma unroll
            for (int g = 0; g < RD_GROUPS; g++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, RD_PER, 0);  // DS read
            }
            __builtin_amdgcn_sched_group_barrier(
                0x008, MT * NT - RD_LEAD - RD_GROUPS, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (AHEAD >= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            // reads first: the compiler keeps LDS reads and DMA writes in
            // source order, and the fragments are needed sooner
            read_quad(&As[(buf ^ 1) * BK * BM], &Bs[(buf ^ 1) * BN * BK], 0,
                      fa[0], fb[0]);
            if constexpr (AHEAD >= 2) issue_next(buf);
        }
        mfma_quad(fa[1], fb[1]);             // quad Q-1 of tile s
        if constexpr (AHEAD >= 1) {
            // LQ_PER fragment reads, then one DMA piece, behind each MFMA
            #pragma unroll
            for (int g = 0; g < LQ_GROUPS; g++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, LQ_PER, 0);  // DS read
            }
            if constexpr (AHEAD >= 2) {
                #pragma unroll
                for (int g = 0; g < P; g++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);  // VMEM (DMA)
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    using std::integral_constant;
    int s = 0;
    if constexpr (UNROLL2) {
        for (; s + 3 < ntiles; s += 2) {
            step(integral_constant<int, 0>{}, integral_constant<int, 2>{});
            step(integral_constant<int, 1>{}, integral_constant<int, 2>{});
        }
    }
    for (; s + 2 < ntiles; s++) step(s & 1, integral_constant<int, 2>{});
    if (s + 1 < ntiles) { step(s & 1, integral_constant<int, 1>{}); s++; }
    step(s & 1, integral_constant<int, 0>{});
    }

    if constexpr (EPI == EPI_TN_ADD) {
        // Fused transpose/add epilogue (BASELINE config 5): result element
        // (r, cc) of A*B goes to C[cc + r*ldc] (C is N x M col-major) —
        // contiguous output runs are (fixed r, varying cc). The store is
        // staged through LDS in two 64-row half-tiles, laid out
        // stage[r'*128 + cc], so every global write is a coalesced float4
        // run (the naive per-element store was 4-byte scattered and cost
        // ~8% at 40000^2). fp32 on the two-barrier loop only: that loop
        // leaves the k-loop buffers free behind its closing barrier.
        static_assert(std::is_same<T, float>::value && !BETA && !PIPE &&
                      BM == 128 && WM == 2 && WN == 2,
                      "fused epilogue: fp32 default geometry, two-barrier loop");
        static_assert(64 * BN == 2 * BK * BM + 2 * BN * BK,
                      "the 64x128 stage fills the k-loop buffers exactly");
        float* stage = sAB;                 // k-loop done; reuse the buffers
        v4f* stage4 = (v4f*)sAB;
        #pragma unroll
        for (int half = 0; half < 2; half++) {
            __builtin_amdgcn_s_barrier();   // prior phase's reads complete
            if (wm == half) {
                // this wave pair owns result rows half*64 .. half*64+63
                #pragma unroll
                for (int mt = 0; mt < 4; mt++)
                    #pragma unroll
                    for (int nt = 0; nt < 4; nt++) {
                        int rloc = mt * 16 + l4 * 4;      // 0..63
                        int cc = wn * 64 + nt * 16 + l15;
                        #pragma unroll
                        for (int j = 0; j < 4; j++)
                            stage[(rloc + j) * BN + cc] = acc[mt][nt][j];
                    }
            }
            __builtin_amdgcn_s_barrier();
            // 64 rows x 32 float4 = 2048 stores over 256 threads
            #pragma unroll
            for (int i = 0; i < 8; i++) {
                int idx = tid + i * 256;
                int rloc = idx >> 5;                      // 0..63
                int q = idx & 31;                         // float4 index in row
                int64_t r = row0 + half * 64 + rloc;
                int64_t off = col0 + 4 * q + r * ldc;
                v4f v = stage4[rloc * (BN / 4) + q];
                if (addC) {
                    const v4f* ap = (const v4f*)(addC + off);
                    v4f av = *ap;
                    v.x += av.x; v.y += av.y; v.z += av.z; v.w += av.w;
                }
                *(v4f*)(C + off) = v;
            }
        }
    } else {
    // --- plain store (row map per type, see above) -----------------------
    #pragma unroll
    for (int mt = 0; mt < MT; mt++)
        #pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            int64_t r = row0 + wm * (MT * 16) + mt * 16 + rbase;
            int64_t cc = col0 + wn * (NT * 16) + nt * 16 + l15;
            T* cp = C + cc * ldc + r;
            #pragma unroll
            for (int j = 0; j < 4; j++) cp[rstep * j] = acc[mt][nt][j];
        }
    }
}


// ---------------------------------------------------------------------------
// Deterministic synthetic input fill: splitmix64 of (seed + (idx+1)*gamma),
// idx = logical col-major linear index c*m + r; matches
// oracle.marlin_oracle.gen_matrix bit-for-bit (tests assert it). The
// randomDenVecMatrix stand-in (MTUtils.scala:63-73 semantics).
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

template <typename T>
__global__ void fill_random_kernel(T* __restrict__ buf, int64_t m, int64_t n,
                                   int64_t ld, uint64_t seed) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = m * n;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        int64_t c = i / m, r = i - c * m;
        uint64_t z = splitmix64(seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ULL);
        buf[c * ld + r] = (T)((double)(z >> 11) * (1.0 / 9007199254740992.0));
    }
}

// Zero an m x n padded region (pitch ld) — pad columns/rows stay zero.
template <typename T>
__global__ void zero_pad_kernel(T* __restrict__ buf, int64_t rows_total,
                                int64_t cols_total, int64_t ld,
                                int64_t m, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = rows_total * cols_total;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        int64_t c = i / rows_total, r = i - c * rows_total;
        if (r >= m || c >= n) buf[c * ld + r] = (T)0;
    }
}

// ---------------------------------------------------------------------------
// Elementwise / scalar op family — the BlockMatrix epilogue ops
// (BlockMatrix.scala:344-507: add/subtract matrix+scalar, subtractBy,
// divide, divideBy, dotProduct=element-wise multiply; DenseVecMatrix
// multiply(scalar)). HBM-bound map kernels; layout-agnostic (flat).
// Op codes: MX_OP_* of include/marlin_gpu.h (ADD/SUB/EMUL binary, then
// ADDS, SUBS, RSUBS = s - A, MULS, DIVS, RDIVS = s / A).

// c may be a or b (mx_map and mx_map_device both run it in place): element
// i is read before it is written and no other is touched, so the pointers
// are not declared __restrict__.
template <typename T>
__global__ void map_kernel(int op, int64_t n, const T* a, const T* b,
                           double scalar, T* c) {
    const T s = (T)scalar;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        T x = a[i];
        T y;
        switch (op) {
            case MX_OP_ADD:   y = x + b[i]; break;
            case MX_OP_SUB:   y = x - b[i]; break;
            case MX_OP_EMUL:  y = x * b[i]; break;
            case MX_OP_ADDS:  y = x + s; break;
            case MX_OP_SUBS:  y = x - s; break;
            case MX_OP_RSUBS: y = s - x; break;
            case MX_OP_MULS:  y = x * s; break;
            case MX_OP_DIVS:  y = x / s; break;
            default:          y = s / x; break;
        }
        c[i] = y;
    }
}

// sum reduction (DistributedMatrix.sum, BlockMatrix.scala sum tests):
// stage 1: per-block tree sums -> partials; stage 2: one block combines
// in fixed order (deterministic given the fixed grid).
template <typename T>
__global__ void sum_stage1_kernel(int64_t n, const T* __restrict__ a,
                                  double* __restrict__ partials) {
    __shared__ double sm[256];
    double acc = 0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) acc += (double)a[i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sm[0];
}

__global__ void sum_stage2_kernel(int nparts, const double* __restrict__ p,
                                  double* __restrict__ out) {
    __shared__ double sm[256];
    double acc = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += p[i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sm[0];
}

// Tiled transpose (BlockMatrix.transpose, BlockMatrix.scala:514-523):
// out[n x m] = in[m x n]^T, col-major, 32x32 LDS tiles (+1 pad), both
// sides coalesced.
template <typename T>
__global__ void transpose_kernel(int64_t m, int64_t n,
                                 const T* __restrict__ in,
                                 T* __restrict__ out) {
    __shared__ T tile[32][33];
    int64_t tm = (m + 31) / 32;
    int64_t bi = blockIdx.x % tm;           // tile row of input
    int64_t bj = blockIdx.x / tm;           // tile col of input
    int tx = threadIdx.x % 32, ty = threadIdx.x / 32;  // 32x8 threads
    int64_t r0 = bi * 32, c0 = bj * 32;
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        int64_t r = r0 + tx, c = c0 + ty + k * 8;
        if (r < m && c < n) tile[ty + k * 8][tx] = in[c * m + r];
    }
    __syncthreads();
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        int64_t r = c0 + tx, c = r0 + ty + k * 8;   // output coords
        if (r < n && c < m) out[c * n + r] = tile[tx][ty + k * 8];
    }
}

// ---------------------------------------------------------------------------
// Matrix-vector multiply (BlockMatrix.multiply(DistributedVector/BDV),
// BlockMatrix.scala:240-274): y = A x, col-major A. HBM-bound; row-slab
// blocks x column chunks with fp64 partials, reduced in ascending chunk
// order (deterministic). Reads of A are fully coalesced per column.
template <typename T>
__global__ void gemv_partial_kernel(int64_t m, int64_t n, int64_t lda,
                                    const T* __restrict__ A,
                                    const T* __restrict__ x,
                                    double* __restrict__ partial,
                                    int nchunks) {
    int64_t nrb = (m + 255) / 256;
    int64_t rb = blockIdx.x % nrb;
    int chunk = (int)(blockIdx.x / nrb);
    int64_t r = rb * 256 + threadIdx.x;
    int64_t clen = (n + nchunks - 1) / nchunks;
    int64_t c0 = chunk * clen;
    int64_t c1 = c0 + clen < n ? c0 + clen : n;
    if (r >= m) return;
    // 4 independent partial sums: keeps >=4 column loads in flight per
    // lane (the serial 1-acc loop measured latency-bound at 0.5-0.6
    // TB/s); summed in fixed order below -> still deterministic.
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int64_t j = c0;
    for (; j + 4 <= c1; j += 4) {
        a0 += (double)A[(j + 0) * lda + r] * (double)x[j + 0];
        a1 += (double)A[(j + 1) * lda + r] * (double)x[j + 1];
        a2 += (double)A[(j + 2) * lda + r] * (double)x[j + 2];
        a3 += (double)A[(j + 3) * lda + r] * (double)x[j + 3];
    }
    for (; j < c1; j++)
        a0 += (double)A[j * lda + r] * (double)x[j];
    partial[(int64_t)chunk * m + r] = ((a0 + a1) + (a2 + a3));
}

template <typename T>
__global__ void gemv_reduce_kernel(int64_t m, int nchunks,
                                   const double* __restrict__ partial,
                                   T* __restrict__ y) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    double acc = 0;
    for (int c = 0; c < nchunks; c++) acc += partial[(int64_t)c * m + r];
    y[r] = (T)acc;
}

// ---------------------------------------------------------------------------
// Split-K combine (mx_gemm_device_splitk): C += W_0 + W_1 + ... as a left
// fold, ((C + W_0) + W_1) + ..., in the element type. C is m x n at pitch
// ldc and already holds the first term (slice 0's product, or the caller's
// C when accumulating, which is why one kernel serves both betas); slab j
// is the tight m x n partial product at W + j * slab. It runs as its own
// launch behind the GEMM on the same stream, so stream order alone makes
// the partials visible: no fence, counter or atomic, and the order of the
// adds is the slice order whatever the schedule, so the bits are fixed.
// HBM-bound: one thread per 16-byte chunk of a C column (m is a multiple
// of 128, so a chunk never crosses into the pad rows [m, ldc), which are
// neither read nor written), capped grid, grid-stride. The slab loads of a
// chunk are independent and issued eight at a time ahead of their adds.
// They are nontemporal: a partial is read exactly once, and loading it
// without keeping it cached measured 6.2-6.8 TB/s inside the entry against
// 4.4-4.9 for plain loads at 4 and 8 slices of a 4096^2 fp64 C, and the
// same at 2 slices (profiles/gemm_splitk.md).
typedef double v2d __attribute__((ext_vector_type(2)));
template <typename T> struct chunk16_t;
template <> struct chunk16_t<double> { using type = v2d; };
template <> struct chunk16_t<float>  { using type = v4f; };

template <typename T>
__global__ void __launch_bounds__(256)
splitk_reduce_kernel(T* __restrict__ C, int64_t ldc, int64_t m, int64_t n,
                     const T* __restrict__ W, int64_t slab, int nslabs) {
    using V = typename chunk16_t<T>::type;
    constexpr int64_t E = 16 / sizeof(T);
    const int64_t per_col = m / E, total = per_col * n;
    const int64_t slab_v = slab / E;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        const int64_t col = i / per_col, r = i - col * per_col;
        V* cp = reinterpret_cast<V*>(C + col * ldc) + r;
        const V* wp = reinterpret_cast<const V*>(W) + i;   // tight: linear
        V acc = *cp;
        int j = 0;
        for (; j + 8 <= nslabs; j += 8) {
            V w[8];
            #pragma unroll
            for (int b = 0; b < 8; b++)
                w[b] = __builtin_nontemporal_load(&wp[(j + b) * slab_v]);
            #pragma unroll
            for (int b = 0; b < 8; b++) acc = acc + w[b];   // ascending
        }
        for (; j < nslabs; j++)
            acc = acc + __builtin_nontemporal_load(&wp[j * slab_v]);
        *cp = acc;
    }
}

// ---------------------------------------------------------------------------
// Triangular solve, the diagonal blocks (mx_trsm_device; the sweep around
// them is trsm_plan.h). One launch solves ONE 128 x 128 diagonal block of T
// against all r right-hand sides: X_j overwrites its strip of B and -X_j
// goes to the workspace panel, which the accumulating GEMM of the step then
// multiplies into every remaining block. It carries 128 / n of the flops
// and is one-shot and latency-bound, so it is built for fixed arithmetic
// and coalesced traffic, not for peak rate.
//
//   - One right-hand side per lane, 64 per block (one wave), r / 64 blocks.
//     Every lane runs the same forward substitution on a lower-triangular
//     L, y_a = (v_a - sum_{b<a} L[a][b] y_b) / L[a][a], subtracting in
//     ascending b: the order of a result's operations is fixed by the code
//     alone, no atomics, no cross-lane sums, and each operation is one of
//     trsm_plan.h's two (mx_trsm_update, one fused multiply-add, and
//     mx_trsm_quot, one division), so neither is the rounding left to the
//     compiler's contraction. Side, triangle, transpose and
//     unit diagonal are resolved when L is staged (mx_trsm_stage: transpose
//     on load, reversal of the index for an upper form, 1 on a unit
//     diagonal, the identity at an index >= nv), element by element, so
//     only the referenced triangle below the order of T is ever loaded.
//   - The strip of B lives in LDS as tile[a][lane] (pitch 65: the strip
//     loads and stores walk it along a, the substitution along the lanes,
//     neither with more than a 2-way bank conflict). It moves to and from
//     global memory in 16-byte chunks along whichever dimension is
//     contiguous there: the rows of the strip on the left side (a lane per
//     column would stride by the pitch), the right-hand sides on the right.
//   - L is staged 32 rows at a time as Lp[b][i], 32 KB in fp64, which with
//     the 65 KB tile fits the 160 KB of LDS where the whole block (128 KB)
//     would not. A lane keeps the 32 rows of its vector it is solving in
//     registers (64 VGPRs in fp64), never all 128; finished rows are read
//     back from the tile, L from Lp at a wave-uniform address (a broadcast).
#define TRSM_FN __host__ __device__ __forceinline__
#include "trsm_plan.h"

constexpr int TRSM_W = 128;              // order of a diagonal block
constexpr int TRSM_RB = 64;              // right-hand sides per block
constexpr int TRSM_PB = 32;              // rows of L staged at a time
constexpr int TRSM_TP = TRSM_RB + 1;     // pitch of the LDS tile

// The 128 x 64 strip between global memory and the tile. g is its first
// element: on the left side 128 contiguous rows by 64 columns of pitch
// `pitch`, on the right 64 contiguous right-hand sides by 128 columns.
template <typename T, int SIDE, int STORE>
DEVFN void trsm_strip_io(T* __restrict__ g, int64_t pitch, T* tile, int rev,
                         int lane, T sign) {
    using V = typename chunk16_t<T>::type;
    constexpr int E = 16 / sizeof(T);
    constexpr int D = SIDE ? TRSM_RB : TRSM_W;     // the contiguous extent
    constexpr int O = SIDE ? TRSM_W : TRSM_RB;     // the pitched one
    constexpr int STEP = 64 * E / D;               // columns per instruction
    const int u = (lane * E) % D, dv = (lane * E) / D;
    #pragma unroll 8
    for (int v = 0; v < O; v += STEP) {
        V* p = reinterpret_cast<V*>(g + u + (int64_t)(v + dv) * pitch);
        V x;
        if (!STORE) x = *p;
        #pragma unroll
        for (int e = 0; e < E; e++) {
            const int o = SIDE ? v + dv : u + e;   // index inside the block
            const int c = SIDE ? u + e : v + dv;   // right-hand side
            T* t = &tile[mx_trsm_orig(TRSM_W, rev, o) * TRSM_TP + c];
            if (STORE) x[e] = sign * *t; else *t = x[e];
        }
        if (STORE) *p = x;
    }
}

// One element of L as mx_trsm_stage defines it. The load is unconditional,
// so that an unrolled staging loop has all its loads in flight at once
// instead of one round trip per element: a lane with nothing to load reads
// this idle word instead, never an element of T outside the referenced
// triangle.
__device__ double mx_trsm_idle[2] = {0.0, 0.0};

template <typename T>
DEVFN T trsm_stage_elem(const T* __restrict__ Tjj, int64_t ldt, int tt,
                        int rev, int unit, int nv, int a, int b) {
    int64_t off = 0;
    const int kind = mx_trsm_stage(TRSM_W, tt, rev, unit, nv, a, b, ldt, &off);
    const T* src = kind == MX_TRSM_LOAD
                       ? Tjj + off
                       : reinterpret_cast<const T*>(mx_trsm_idle);
    const T v = *src;
    return kind == MX_TRSM_LOAD ? v : T(kind);
}

template <typename T, int SIDE>
__global__ void __launch_bounds__(TRSM_RB)
trsm_diag_kernel(const T* __restrict__ Tjj, int64_t ldt, T* __restrict__ X,
                 int64_t ldx, T* __restrict__ ws, int64_t ldw, int tt,
                 int rev, int unit, int nv) {
    __shared__ __attribute__((aligned(16)))
        T smem[TRSM_W * TRSM_PB + TRSM_W * TRSM_TP];
    T* Lp = smem;                        // Lp[b * 32 + i] = L[32 s + i][b]
    T* tile = smem + TRSM_W * TRSM_PB;   // tile[a * 65 + lane]
    const int lane = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * TRSM_RB;
    T* xg = X + (SIDE ? c0 : c0 * ldx);
    T* wg = ws + (SIDE ? c0 : c0 * ldw);
    trsm_strip_io<T, SIDE, 0>(xg, ldx, tile, rev, lane, T(1));

    #pragma unroll 1
    for (int s = 0; s < TRSM_W / TRSM_PB; s++) {
        const int a0 = s * TRSM_PB, cols = a0 + TRSM_PB;
        __syncthreads();                 // the previous panel is done with
        // stage rows [a0, a0 + 32) of L, columns [0, a0 + 32); the lanes
        // run along whichever index is contiguous in T as stored, eight
        // loads per lane in flight before the first is stored
        if (!tt) {
            const int i = lane & 31;
            for (int b0 = lane >> 5; b0 < cols; b0 += 16) {
                T v[8];
                #pragma unroll
                for (int q = 0; q < 8; q++)
                    v[q] = trsm_stage_elem(Tjj, ldt, tt, rev, unit, nv, a0 + i,
                                           b0 + 2 * q);
                #pragma unroll
                for (int q = 0; q < 8; q++)
                    Lp[(b0 + 2 * q) * TRSM_PB + i] = v[q];
            }
        } else {
            // columns [cols, 128) of Lp are written too (zeros: a < b
            // there); no later read of this panel looks at them
            for (int i0 = 0; i0 < TRSM_PB; i0 += 4) {
                T v[8];
                #pragma unroll
                for (int q = 0; q < 8; q++)
                    v[q] = trsm_stage_elem(Tjj, ldt, tt, rev, unit, nv,
                                           a0 + i0 + (q >> 1),
                                           lane + 64 * (q & 1));
                #pragma unroll
                for (int q = 0; q < 8; q++)
                    Lp[(lane + 64 * (q & 1)) * TRSM_PB + i0 + (q >> 1)] = v[q];
            }
        }
        __syncthreads();

        T y[TRSM_PB];
        #pragma unroll
        for (int i = 0; i < TRSM_PB; i++)
            y[i] = tile[(a0 + i) * TRSM_TP + lane];
        // the divisors of this panel, loaded ahead of the loop below so
        // that none is fetched between two dependent divisions
        T dg[TRSM_PB];
        #pragma unroll
        for (int i = 0; i < TRSM_PB; i++)
            dg[i] = Lp[(a0 + i) * TRSM_PB + i];
        // the rows solved by earlier panels
        for (int b = 0; b < a0; b++) {
            const T yb = tile[b * TRSM_TP + lane];
            const T* col = Lp + b * TRSM_PB;
            #pragma unroll
            for (int i = 0; i < TRSM_PB; i++)
                y[i] = mx_trsm_update(y[i], col[i], yb);
        }
        // the triangle of this panel, in registers
        #pragma unroll
        for (int i = 0; i < TRSM_PB; i++) {
            const T* col = Lp + (a0 + i) * TRSM_PB;
            y[i] = mx_trsm_quot(y[i], dg[i]);
            #pragma unroll
            for (int i2 = i + 1; i2 < TRSM_PB; i2++)
                y[i2] = mx_trsm_update(y[i2], col[i2], y[i]);
        }
        #pragma unroll
        for (int i = 0; i < TRSM_PB; i++)
            tile[(a0 + i) * TRSM_TP + lane] = y[i];
    }
    __syncthreads();
    trsm_strip_io<T, SIDE, 1>(xg, ldx, tile, rev, lane, T(1));
    trsm_strip_io<T, SIDE, 1>(wg, ldw, tile, rev, lane, T(-1));
}

// ---------------------------------------------------------------------------
// LU factorisation, the diagonal blocks and their row permutation
// (mx_getrf_device; the sweep around them is getrf_plan.h, whose
// mx_getrf_eliminate states the elimination these kernels perform: the
// element operations below are that header's, in its order).
//
// getrf_diag_kernel factors ONE 128 x 128 block with partial pivoting among
// its own rows. It is latency-bound by construction: one workgroup on one
// CU, 128 dependent columns with three barriers each, so its cost is to be
// compared with the host step it replaces (download, host LU, three
// uploads), not with a roofline.
//
//   - The block lives whole in LDS, column-major at the odd pitch 129
//     (fp64: 128 * 129 * 8 B = 132096 B of the 160 KB). The update and the
//     scale walk a column with one row per lane (consecutive addresses); the
//     row swap walks a row with one column per lane, a stride of 129
//     elements, which the odd pitch spreads over all banks.
//   - It moves between global memory and LDS in 16-byte chunks down the
//     contiguous columns. Nothing at a row or column index >= nv is loaded
//     or stored: the ragged block behaves as if continued by the identity,
//     whose columns pivot on themselves and update nothing, so the loop
//     ends at nv.
//   - Column j: wave 0 alone finds the pivot (two rows per lane, a butterfly
//     of mx_getrf_better over the wave, so no cross-wave step) and swaps
//     the two rows (two columns per lane); then every remaining row is
//     scaled by one division, then the rank-1 update runs over the whole
//     workgroup, a row per thread and every fourth column.
//   - No atomics, no cross-wave sums: the bits do not depend on the run.
#define GETRF_FN __host__ __device__ __forceinline__
#include "getrf_plan.h"

constexpr int GETRF_W = 128;                     // order of a diagonal block
constexpr int GETRF_P = GETRF_W + 1;             // pitch of the LDS image
constexpr int GETRF_NT = 512;                    // threads of the workgroup
constexpr int GETRF_CG = GETRF_NT / GETRF_W;     // column groups of the update
constexpr int GETRF_CT = 8;                      // columns per row-perm tile

// The leading nv x nv part of the block between global memory (pitch lda)
// and the LDS image, 16-byte chunks down the columns; a chunk that crosses
// nv goes element by element.
template <typename T, int STORE>
DEVFN void getrf_block_io(T* __restrict__ g, int64_t lda, T* S, int nv,
                          int tid) {
    using V = typename chunk16_t<T>::type;
    constexpr int E = 16 / sizeof(T);
    constexpr int CPC = GETRF_W / E;             // chunks per column
    for (int q = tid; q < CPC * GETRF_W; q += GETRF_NT) {
        const int r = (q % CPC) * E, c = q / CPC;
        if (c >= nv || r >= nv) continue;
        T* s = &S[r + c * GETRF_P];
        T* p = g + r + (int64_t)c * lda;
        if (r + E <= nv) {
            V x;
            if (!STORE) x = *reinterpret_cast<const V*>(p);
            #pragma unroll
            for (int e = 0; e < E; e++) {
                if (STORE) x[e] = s[e]; else s[e] = x[e];
            }
            if (STORE) *reinterpret_cast<V*>(p) = x;
        } else {
            for (int e = 0; r + e < nv; e++) {
                if (STORE) p[e] = s[e]; else s[e] = p[e];
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(GETRF_NT)
getrf_diag_kernel(T* __restrict__ Ajj, int64_t lda, int nv, int o,
                  int* __restrict__ piv, int* __restrict__ first_zero) {
    __shared__ __attribute__((aligned(16))) T S[GETRF_W * GETRF_P];
    __shared__ int perm[GETRF_W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = tid % GETRF_W, cg = tid / GETRF_W;
    if (tid < GETRF_W) perm[tid] = tid;
    getrf_block_io<T, 0>(Ajj, lda, S, nv, tid);
    int fz = 0;                          // thread 0's: first zero pivot, 1-based

    #pragma unroll 1
    for (int j = 0; j < nv; j++) {
        T* colj = S + j * GETRF_P;
        __syncthreads();                 // the update of column j - 1 is done
        if (wave == 0) {
            T key = T(-1);
            int p = j;
            #pragma unroll
            for (int h = 0; h < 2; h++) {
                const int i = lane + 64 * h;
                if (i >= j && i < nv) {
                    const T k2 = mx_getrf_key(colj[i]);
                    if (mx_getrf_better(k2, i, key, p)) { key = k2; p = i; }
                }
            }
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const T k2 = __shfl_xor(key, d);
                const int p2 = __shfl_xor(p, d);
                if (mx_getrf_better(k2, p2, key, p)) { key = k2; p = p2; }
            }
            if (p != j) {                // wave-uniform
                #pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int k = lane + 64 * h;
                    if (k < nv) {
                        const T a = S[j + k * GETRF_P], b = S[p + k * GETRF_P];
                        S[j + k * GETRF_P] = b;
                        S[p + k * GETRF_P] = a;
                    }
                }
                if (lane == 0) {
                    const int t = perm[j];
                    perm[j] = perm[p];
                    perm[p] = t;
                }
            }
        }
        __syncthreads();
        const T pivot = colj[j];
        if (pivot == T(0)) {
            if (tid == 0 && !fz) fz = j + 1;
        } else if (cg == 0 && row > j && row < nv) {
            colj[row] = mx_getrf_scale(colj[row], pivot);
        }
        __syncthreads();
        if (row > j && row < nv) {
            const T l = colj[row];
            #pragma unroll 4
            for (int k = j + 1 + cg; k < nv; k += GETRF_CG) {
                T* colk = S + k * GETRF_P;
                colk[row] = mx_getrf_update(colk[row], l, colk[j]);
            }
        }
    }
    __syncthreads();
    getrf_block_io<T, 1>(Ajj, lda, S, nv, tid);
    if (tid < GETRF_W) piv[tid] = o + perm[tid];
    if (tid == 0 && fz && *first_zero == 0) *first_zero = o + fz;
}

// Applies the block's permutation to rows [o, o + 128) of the other columns
// of the image, in place: `rows` is A + o, column cc of the ncols = np - 128
// handled is image column cc (cc < left_cols = o) or cc + 128. A workgroup
// owns 128 rows x 8 whole columns: it loads them straight into LDS (a column
// per half of the workgroup, consecutive lanes down it), and after the
// barrier stores row g from source row perm[g] - o. Columns are independent
// and a workgroup holds all 128 rows of its own, so in place is safe.
template <typename T>
__global__ void __launch_bounds__(256)
getrf_rowperm_kernel(T* __restrict__ rows, int64_t lda,
                     const int* __restrict__ piv, int o, int64_t left_cols,
                     int64_t ncols) {
    __shared__ T tile[GETRF_CT * GETRF_W];
    const int g = threadIdx.x % GETRF_W, h = threadIdx.x / GETRF_W;
    // a source row is inside the block by construction; the mask keeps a
    // corrupted entry from reading outside the tile
    const int src = (piv[g] - o) & (GETRF_W - 1);
    const int64_t c0 = (int64_t)blockIdx.x * GETRF_CT;
    #pragma unroll
    for (int cl = h; cl < GETRF_CT; cl += 2) {
        const int64_t cc = c0 + cl;
        if (cc < ncols) {
            const int64_t col = cc < left_cols ? cc : cc + GETRF_W;
            tile[g + cl * GETRF_W] = rows[g + col * lda];
        }
    }
    __syncthreads();
    #pragma unroll
    for (int cl = h; cl < GETRF_CT; cl += 2) {
        const int64_t cc = c0 + cl;
        if (cc < ncols) {
            const int64_t col = cc < left_cols ? cc : cc + GETRF_W;
            rows[g + col * lda] = tile[src + cl * GETRF_W];
        }
    }
}

// ---------------------------------------------------------------------------
// GEMM launch. Which instantiation a call runs is decided in
// gemm_launch_policy.h; here are the latched knobs, the record of the last
// launch, the one step from a selected variant to its compiled kernel, and
// the launchers, which differ in their checks, grid size and arguments.

// The MARLIN_GEMM_* knobs, read once per process.
static const mx_gemm_knobs& gemm_knobs() {
    static const mx_gemm_knobs k = mx_gemm_parse_knobs(getenv);
    return k;
}

// What mxk_gemm_op / mxk_gemm_grouped last launched (kernels.h).
static mxk_last_gemm_t g_last_gemm = {};

static void record_launch(const mx_gemm_variant& v) {
    g_last_gemm.cfg = mx_gemm_cfg_t{v.T, v.BETA, v.BK, v.BM, v.WM * v.WN,
                                    v.band, v.phase_mask};
    g_last_gemm.loop = v.PIPE;
    g_last_gemm.trans_a = v.TA;
    g_last_gemm.trans_b = v.TB;
}

// The kernel arguments of one launch, not yet typed.
struct gemm_args {
    int64_t M, N, K;
    const void* A; int64_t lda;
    const void* B; int64_t ldb;
    void* C; int64_t ldc;
    int nbm, band, phase_mask;
    const void* addC;
    const mx_group_entry* grp;
};

// Calls f(T{}, kernel) with the instantiation v names. It walks the closed
// list of gemm_launch_policy.h, so exactly that list is compiled; a variant
// outside it is a refused argument (-4), not a new kernel.
template <class F>
static int gemm_dispatch(const mx_gemm_variant& v, F&& f) {
    int rc = -4;
    mx_gemm_for_each_instantiation([&](auto inst) {
        using I = decltype(inst);
        if (!mx_gemm_same_kernel(I::variant(), v)) return;
        using T = std::conditional_t<I::T != 0, float, double>;
        f(T{}, gemm_mfma_kernel<T, I::BETA, I::BK, I::BM, I::WM, I::WN,
                                I::PIPE, I::TA, I::TB, I::EPI, I::GRP>);
        rc = 0;
    });
    return rc;
}

static int gemm_launch(const mx_gemm_variant& v, unsigned blocks,
                       const gemm_args& g, hipStream_t stream) {
    const int rc = gemm_dispatch(v, [&](auto t, auto kernel) {
        using T = decltype(t);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(v.WM * v.WN * 64), 0,
                           stream, g.M, g.N, g.K, (const T*)g.A, g.lda,
                           (const T*)g.B, g.ldb, (T*)g.C, g.ldc, g.nbm, g.band,
                           g.phase_mask, (const T*)g.addC, g.grp);
    });
    if (rc) return rc;
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

// ---------------------------------------------------------------------------
// C-visible launchers (called from marlin_gpu.cpp; prototypes in kernels.h).
extern "C" {

void mxk_last_gemm(mxk_last_gemm_t* out) { *out = g_last_gemm; }

void mxk_note_splitk(int slices, int64_t workspace_bytes) {
    g_last_gemm.splitk_slices = slices;
    g_last_gemm.splitk_ws_bytes = workspace_bytes;
}

// m a positive multiple of 128 and ldc one of 16 bytes are the GEMM
// entries' contract (checked again: the 16-byte chunks rely on both).
int mxk_splitk_reduce(int is_fp32, int64_t m, int64_t n, void* C, int64_t ldc,
                      const void* W, int nslabs, hipStream_t stream) {
    const int64_t e16 = is_fp32 ? 4 : 2;
    if (m <= 0 || n <= 0 || m % 128 || nslabs < 1 || !C || !W) return -4;
    if (!pitch_ok(ldc, m, e16)) return -4;
    // memory-bound idiom: a capped grid (16 blocks per CU), grid-stride the
    // rest
    const int64_t chunks = m / e16 * n;
    const int64_t want = (chunks + 255) / 256;
    const dim3 grid((unsigned)(want < 4096 ? want : 4096)), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(splitk_reduce_kernel<float>, grid, block, 0, stream,
                           (float*)C, ldc, m, n, (const float*)W, m * n,
                           nslabs);
    else
        hipLaunchKernelGGL(splitk_reduce_kernel<double>, grid, block, 0,
                           stream, (double*)C, ldc, m, n, (const double*)W,
                           m * n, nslabs);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

// One diagonal block of the triangular solve. Tjj is the block's first
// element in T (pitch ldt), X the first element of its strip of B (left:
// 128 rows x r columns, right: r rows x 128 columns, pitch ldx), ws the
// panel that receives -X (left: 128 x r at pitch 128, right: r x 128 at
// pitch r). tt, rev, unit, nv: mx_trsm_stage. r is a positive multiple of
// 128, so the r / 64 blocks cover it exactly and no lane is out of range.
int mxk_trsm_diag(int is_fp32, int side, int tt, int rev, int unit, int nv,
                  const void* Tjj, int64_t ldt, void* X, int64_t ldx,
                  void* ws, int64_t r, hipStream_t stream) {
    const int64_t e16 = is_fp32 ? 4 : 2;
    if ((is_fp32 | side | tt | rev | unit) & ~1) return -4;
    if (nv < 1 || nv > TRSM_W || r <= 0 || r % 128) return -4;
    if (r / TRSM_RB > INT32_MAX || !Tjj || !X || !ws) return -4;
    if (!pitch_ok(ldt, TRSM_W, e16) || !pitch_ok(ldx, side ? r : TRSM_W, e16))
        return -4;
    const dim3 grid((unsigned)(r / TRSM_RB)), block(TRSM_RB);
    const int64_t ldw = side ? r : TRSM_W;
    auto launch = [&](auto t, auto kernel) {
        using T = decltype(t);
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, (const T*)Tjj, ldt,
                           (T*)X, ldx, (T*)ws, ldw, tt, rev, unit, nv);
    };
    if (is_fp32) {
        if (side) launch(float{}, trsm_diag_kernel<float, 1>);
        else launch(float{}, trsm_diag_kernel<float, 0>);
    } else {
        if (side) launch(double{}, trsm_diag_kernel<double, 1>);
        else launch(double{}, trsm_diag_kernel<double, 0>);
    }
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

// One diagonal block of the LU factorisation, in place. Ajj is the block's
// first element (pitch lda), o its offset in the matrix, nv the order left
// inside it; piv receives the block's 128 entries (global source rows),
// *first_zero the 1-based global column of a zero pivot if it still holds 0.
int mxk_getrf_diag(int is_fp32, int nv, int64_t o, void* Ajj, int64_t lda,
                   int* piv, int* first_zero, hipStream_t stream) {
    const int64_t e16 = is_fp32 ? 4 : 2;
    if (is_fp32 & ~1) return -4;
    if (nv < 1 || nv > GETRF_W || o < 0 || o % GETRF_W) return -4;
    if (o > INT32_MAX - GETRF_W || !Ajj || !piv || !first_zero) return -4;
    if (!pitch_ok(lda, GETRF_W, e16)) return -4;
    if (is_fp32)
        hipLaunchKernelGGL(getrf_diag_kernel<float>, dim3(1), dim3(GETRF_NT),
                           0, stream, (float*)Ajj, lda, nv, (int)o, piv,
                           first_zero);
    else
        hipLaunchKernelGGL(getrf_diag_kernel<double>, dim3(1), dim3(GETRF_NT),
                           0, stream, (double*)Ajj, lda, nv, (int)o, piv,
                           first_zero);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

// The permutation of block o applied to rows [o, o + 128) of the columns
// [0, o) and [o + 128, np) of the np x np image A (pitch lda); piv is the
// block's 128 entries as mxk_getrf_diag wrote them. np == 128 has no other
// column: nothing is launched.
int mxk_getrf_rowperm(int is_fp32, int64_t o, int64_t np, void* A,
                      int64_t lda, const int* piv, hipStream_t stream) {
    const int64_t e16 = is_fp32 ? 4 : 2;
    if (is_fp32 & ~1) return -4;
    if (np < GETRF_W || np % GETRF_W || o < 0 || o % GETRF_W) return -4;
    if (o > np - GETRF_W || np > INT32_MAX || !A || !piv) return -4;
    if (!pitch_ok(lda, np, e16)) return -4;
    const int64_t ncols = np - GETRF_W;
    if (ncols == 0) return 0;
    const dim3 grid((unsigned)((ncols + GETRF_CT - 1) / GETRF_CT)), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(getrf_rowperm_kernel<float>, grid, block, 0, stream,
                           (float*)A + o, lda, piv, (int)o, o, ncols);
    else
        hipLaunchKernelGGL(getrf_rowperm_kernel<double>, grid, block, 0,
                           stream, (double*)A + o, lda, piv, (int)o, o, ncols);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

const mx_gemm_knobs* mxk_gemm_knobs(void) { return &gemm_knobs(); }

// One launch over the union of the tiles of plan's launched problems. The
// device table goes into `ws` (plan.table_bytes() or more) on `stream`
// ahead of the launch. ONE staging buffer suffices: every entry of the C
// ABI synchronises with its GEMM stream before it returns, so no earlier
// grouped launch can still be reading the table when the next call
// overwrites it; for the same reason the host vectors of `plan` only have
// to outlive the caller's synchronisation.
int mxk_gemm_grouped(int is_fp32, int beta_one, int trans_a, int trans_b,
                     const mx_group_plan* plan, void* ws, hipStream_t stream) {
    const int count = (int)plan->entries.size();
    if (count == 0) return 0;
    const size_t eb = (size_t)count * sizeof(mx_group_entry);
    if (hipMemcpyAsync(ws, plan->entries.data(), eb, hipMemcpyHostToDevice,
                       stream) != hipSuccess ||
        hipMemcpyAsync((char*)ws + eb, plan->tile_start.data(),
                       (size_t)(count + 1) * sizeof(int32_t),
                       hipMemcpyHostToDevice, stream) != hipSuccess)
        return -2;
    const unsigned blocks = (unsigned)plan->blocks();
    const mx_gemm_variant v = mx_gemm_select_grouped(
        gemm_knobs(), is_fp32, beta_one, trans_a, trans_b,
        plan->entries[0].band, plan->pitch32);
    record_launch(v);
    g_last_gemm.group_problems = count;
    g_last_gemm.group_blocks = blocks;
    // the per-launch scalars are unused but for nbm, the entry count
    const gemm_args g{0, 0, 0, nullptr, 0, nullptr, 0, nullptr, 0, count, 0, 0,
                      nullptr, (const mx_group_entry*)ws};
    return gemm_launch(v, blocks, g, stream);
}

// C (+)= op(A) * op(B). A transposed operand is the stored image of the
// other shape: A^T is k x m (lda covers K), B^T is n x k (ldb covers N).
int mxk_gemm_op(int is_fp32, int beta_one, int trans_a, int trans_b,
                int64_t M, int64_t N, int64_t K,
                const void* A, int64_t lda, const void* B, int64_t ldb,
                void* C, int64_t ldc, hipStream_t stream) {
    if ((trans_a | trans_b) & ~1) return -4;   // each is 0 or 1
    if (M < 0 || N < 0 || K < 0) return -4;
    if (M == 0 || N == 0) return 0;            // empty tile: nothing to do
    {
        const int64_t e16 = is_fp32 ? 4 : 2;   // elements per 16 bytes
        if (!pitch_ok(lda, trans_a ? K : M, e16) ||
            !pitch_ok(ldb, trans_b ? N : K, e16) ||
            !pitch_ok(ldc, M, e16))
            return -4;
    }
    if (K == 0) {                              // C = 0 (or unchanged if +=)
        if (!beta_one) {
            size_t es = is_fp32 ? 4 : 8;
            hipError_t e = hipMemset2DAsync(C, (size_t)ldc * es, 0,
                                            (size_t)M * es, (size_t)N, stream);
            if (e != hipSuccess) return -2;
        }
        return 0;
    }
    if (M % 128 || N % 128 || K % 16) return -4;
    const mx_gemm_variant v = mx_gemm_select(gemm_knobs(), is_fp32, beta_one,
                                             trans_a, trans_b, M, N, K, lda,
                                             ldb);
    record_launch(v);
    const int64_t nbm = M / v.BM;
    const gemm_args g{M, N, K, A, lda, B, ldb, C, ldc, (int)nbm, v.band,
                      v.phase_mask, nullptr, nullptr};
    return gemm_launch(v, (unsigned)(nbm * (N / 128)), g, stream);
}

int mxk_gemm(int is_fp32, int beta_one,
             int64_t M, int64_t N, int64_t K,
             const void* A, int64_t lda, const void* B, int64_t ldb,
             void* C, int64_t ldc, hipStream_t stream) {
    return mxk_gemm_op(is_fp32, beta_one, 0, 0, M, N, K, A, lda, B, ldb, C,
                       ldc, stream);
}

int mxk_sgemm_tn_epilogue(int64_t M, int64_t N, int64_t K,
                          const float* A, int64_t lda,
                          const float* B, int64_t ldb,
                          float* C, int64_t ldc, const float* addC,
                          hipStream_t stream) {
    // no empty-shape no-op here: the kernel prefetches k-tile 0
    // unconditionally and a zero-block grid is a launch error
    if (M <= 0 || N <= 0 || K <= 0) return -4;
    if (M % 128 || N % 128 || K % 16) return -4;
    // C/addC are N x M: float4 rows need ldc % 4 == 0 and ldc >= N
    if (!pitch_ok(lda, M, 4) || !pitch_ok(ldb, K, 4) || !pitch_ok(ldc, N, 4))
        return -4;
    // not recorded as the last launch (kernels.h)
    const mx_gemm_variant v = mx_gemm_select_epilogue(N);
    const int64_t nbm = M / 128;
    const gemm_args g{M, N, K, A, lda, B, ldb, C, ldc, (int)nbm, v.band,
                      v.phase_mask, addC, nullptr};
    return gemm_launch(v, (unsigned)(nbm * (N / 128)), g, stream);
}

int mxk_fill_random(int is_fp32, void* buf, int64_t m, int64_t n, int64_t ld,
                    uint64_t seed, hipStream_t stream) {
    dim3 grid(2048), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(fill_random_kernel<float>, grid, block, 0, stream,
                           (float*)buf, m, n, ld, seed);
    else
        hipLaunchKernelGGL(fill_random_kernel<double>, grid, block, 0, stream,
                           (double*)buf, m, n, ld, seed);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

int mxk_zero_pad(int is_fp32, void* buf, int64_t rows_total, int64_t cols_total,
                 int64_t ld, int64_t m, int64_t n, hipStream_t stream) {
    dim3 grid(2048), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(zero_pad_kernel<float>, grid, block, 0, stream,
                           (float*)buf, rows_total, cols_total, ld, m, n);
    else
        hipLaunchKernelGGL(zero_pad_kernel<double>, grid, block, 0, stream,
                           (double*)buf, rows_total, cols_total, ld, m, n);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

int mxk_map(int is_fp32, int op, int64_t n, const void* a, const void* b,
            double scalar, void* c, hipStream_t stream) {
    dim3 grid(2048), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(map_kernel<float>, grid, block, 0, stream, op, n,
                           (const float*)a, (const float*)b, scalar, (float*)c);
    else
        hipLaunchKernelGGL(map_kernel<double>, grid, block, 0, stream, op, n,
                           (const double*)a, (const double*)b, scalar,
                           (double*)c);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

int mxk_sum(int is_fp32, int64_t n, const void* a, double* partials,
            double* out, hipStream_t stream) {
    dim3 grid(1024), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(sum_stage1_kernel<float>, grid, block, 0, stream,
                           n, (const float*)a, partials);
    else
        hipLaunchKernelGGL(sum_stage1_kernel<double>, grid, block, 0, stream,
                           n, (const double*)a, partials);
    hipLaunchKernelGGL(sum_stage2_kernel, dim3(1), block, 0, stream, 1024,
                       partials, out);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

int mxk_transpose(int is_fp32, int64_t m, int64_t n, const void* in,
                  void* out, hipStream_t stream) {
    int64_t tm = (m + 31) / 32, tn = (n + 31) / 32;
    dim3 grid((unsigned)(tm * tn)), block(256);
    if (is_fp32)
        hipLaunchKernelGGL(transpose_kernel<float>, grid, block, 0, stream,
                           m, n, (const float*)in, (float*)out);
    else
        hipLaunchKernelGGL(transpose_kernel<double>, grid, block, 0, stream,
                           m, n, (const double*)in, (double*)out);
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

int mxk_gemv(int is_fp32, int64_t m, int64_t n, int64_t lda, const void* A,
             const void* x, double* partial, void* y, hipStream_t stream) {
    int64_t nrb = (m + 255) / 256;
    // 32 column chunks: at m=16384 that is 2048 workgroups (8 per CU),
    // enough in-flight loads to cover HBM latency (8 chunks measured
    // 0.53 TB/s -- only 2 blocks/CU; see profiles/r02_experiments.md)
    int nchunks = 32;
    dim3 grid((unsigned)(nrb * nchunks)), block(256);
    if (is_fp32) {
        hipLaunchKernelGGL(gemv_partial_kernel<float>, grid, block, 0, stream,
                           m, n, lda, (const float*)A, (const float*)x,
                           partial, nchunks);
        hipLaunchKernelGGL(gemv_reduce_kernel<float>, dim3((unsigned)nrb),
                           block, 0, stream, m, nchunks, partial, (float*)y);
    } else {
        hipLaunchKernelGGL(gemv_partial_kernel<double>, grid, block, 0, stream,
                           m, n, lda, (const double*)A, (const double*)x,
                           partial, nchunks);
        hipLaunchKernelGGL(gemv_reduce_kernel<double>, dim3((unsigned)nrb),
                           block, 0, stream, m, nchunks, partial, (double*)y);
    }
    return (int)hipGetLastError() == 0 ? 0 : -2;
}

}  // extern "C"
