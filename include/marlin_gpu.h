/* marlin_gpu.h — C ABI of the MI355X-native block-matrix multiply engine.
 *
 * This is the drop-in boundary replacing the reference's (PasaLab/marlin)
 * native hand-off point: Breeze `*` -> netlib-java JNI `dgemm` invoked at
 *   SubMatrix.scala:87-105  (per-tile dense multiply)
 *   SubMatrix.scala:41-50   (per-tile partial-sum add, reduceByKey combiner)
 * and the whole-multiply operator surface
 *   BlockMatrix.scala:149-220  (BlockMatrix.multiply)
 *   DenseVecMatrix.scala:109-141, 196-231 (split-mode multiply + dispatch).
 *
 * A JVM host (Marlin's Scala DenseVecMatrix/BlockMatrix) binds these entry
 * points over JNI (see INTEGRATION.md for the binding stub); the in-container
 * hosts are src/host/marlinx.cpp (C++ CLI) and marlin_amd/engine.py (ctypes).
 *
 * Conventions (match the reference):
 *   - All matrices are COLUMN-MAJOR fp64/fp32 (Breeze's layout,
 *     Matrices.scala:34-48), caller-owned host buffers, fully materialised.
 *   - All functions return int: 0 = ok, < 0 = error (mx_strerror).
 *   - Dimension checks mirror `require(numCols == other.numRows)`
 *     (BlockMatrix.scala:150-151) -> MX_EDIM.
 *   - An mx_ctx is externally synchronised (one call at a time — matches
 *     Spark's one-action-at-a-time driver); internally multi-stream.
 */
#ifndef MARLIN_GPU_H
#define MARLIN_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------- */
#define MX_OK            0
#define MX_EDIM         -1   /* dimension mismatch (require(...) analogue)  */
#define MX_EHIP         -2   /* HIP runtime failure                          */
#define MX_ENOMEM       -3   /* device allocation failure                    */
#define MX_EINVAL       -4   /* bad argument (null ptr, size<=0, bad grid)   */
#define MX_ENOCOMM      -5   /* distributed entry without mx_comm_init       */
#define MX_ERCCL        -6   /* RCCL failure                                 */
#define MX_ENODEV       -7   /* no MI355X device visible                     */

const char* mx_strerror(int code);

/* ---- context ----------------------------------------------------------- */
typedef struct mx_ctx mx_ctx;

/* Create a context bound to one GPU (one process per GPU).
 * device < 0 means "current HIP device". */
int mx_init(mx_ctx** out, int device);
int mx_shutdown(mx_ctx* ctx);

/* ---- distributed setup (SUMMA over RCCL/xGMI) --------------------------- */
/* 128-byte opaque RCCL unique id, exchanged out-of-band by the launcher
 * (bench.py uses torch.distributed/gloo as the control plane). */
#define MX_UNIQUE_ID_BYTES 128
int mx_comm_id(char unique_id[MX_UNIQUE_ID_BYTES]);  /* rank 0 calls this */

/* Collective: every rank of the job calls with the same unique_id.
 * Builds the world communicator plus the pr x pc grid row/col
 * sub-communicators (grids: 8=4x2, 4=2x2, 2=2x1, 1=1x1). */
int mx_comm_init(mx_ctx* ctx, int rank, int nranks,
                 const char unique_id[MX_UNIQUE_ID_BYTES]);

/* Device facts (CU count, max clock kHz) for on-box peak computation. */
int mx_device_info(mx_ctx* ctx, int* cus, int* clock_khz);

/* Grid geometry of this rank after mx_comm_init (pr,pc,row,col). */
int mx_grid(mx_ctx* ctx, int* pr, int* pc, int* prow, int* pcol);

/* ---- numerics of the GEMM and gemv entries ------------------------------ */
/* Every entry below that multiplies (host and device GEMMs in every op form
 * and kernel geometry, the fused epilogue, grouped, split-K, SUMMA, the
 * per-tile accumulate, gemv) computes in the element type with IEEE
 * round-to-nearest: full-width operands, an accumulator of the element
 * type (fp64 in gemv), plain adds in the epilogue and the split-K fold.
 * For every element of a result C^ of R = op(A)·op(B) (+ C0 | + add_c), with
 * S = |op(A)|·|op(B)| (+ |C0| | + |add_c|), u = 2^-24 (fp32) or 2^-53 (fp64):
 *
 *     |C^ - R| <= g(terms) * S + 2 * terms * eta,   g(t) = t*u / (1 - t*u)
 *
 *   - terms is the number of summands of the element: k for a product,
 *     k + 1 when accumulating or adding add_c, the sum of the k's over an
 *     mx_tile_dgemm_acc chain, k for a SUMMA panel loop (the chain continues
 *     across panels), n for gemv;
 *   - split-K with S slices changes the order of the sum (S chains, then a
 *     fold in slice order) and adds S to terms: k + S;
 *   - eta is half the smallest subnormal (2^-150, 2^-1075): subnormal inputs,
 *     products and results are honoured, never flushed, so this is all that
 *     underflow can cost; where S is 0 the result is exactly 0;
 *   - +-inf and NaN propagate as IEEE sums of products do (0 * inf is NaN).
 * The bound holds for any summation order, fused or not, so it does not
 * depend on a knob, a geometry or the schedule; which order a given entry
 * uses, and that it is fixed, is stated with the entry.
 * tests/test_gpu_gemm_rounding.py holds every entry to it, componentwise. */

/* ---- whole-multiply entries (the BlockMatrix.multiply replacement) ------ */
/* Every entry that takes host buffers (the multiplies, SUMMA and k-resident
 * host entries below, mx_tile_dgemm_acc, mx_map, mx_sum, mx_transpose,
 * mx_dgemv) stages them into padded device images: a call with an image
 * whose size in bytes does not fit int64_t returns MX_ENOMEM before it
 * touches the device. */
/* Single-GPU: C = A * B, host col-major buffers; the engine does
 * pad/H2D/tiled MFMA GEMM/D2H internally. */
int mx_dgemm(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
             const double* A, const double* B, double* C);
int mx_sgemm(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
             const float* A, const float* B, float* C);

/* C = op(A)·op(B), op(X) = X or X^T per trans_x in {0,1}, fp64
 * (is_fp32 = 0) or fp32. Host buffers, tight col-major: A is m x k (k x m
 * if trans_a), B is k x n (n x k if trans_b), C is m x n. Pad/H2D/GEMM/D2H
 * inside, as mx_dgemm; a transposed operand is uploaded as stored and
 * never copied into the other layout. m, k or n <= 0 is MX_EDIM. */
int mx_gemm_op(mx_ctx* ctx, int is_fp32, int trans_a, int trans_b,
               int64_t m, int64_t k, int64_t n,
               const void* A, const void* B, void* C);

/* fp32 multiply with fused epilogue (BASELINE config 5):
 * C_out = op(A*B) [+ add_c], op = transpose if transpose_c != 0.
 * If transpose_c: C is n x m col-major, add_c (optional, may be NULL)
 * n x m; else C is m x n. Epilogue runs on-device, fused into the
 * result store — replaces BlockMatrix transpose (BlockMatrix.scala:514-523)
 * + elementwise add (BlockMatrix.scala:344-452) composed after multiply. */
int mx_sgemm_epilogue(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                      const float* A, const float* B, float* C,
                      int transpose_c, const float* add_c);

/* Distributed SUMMA (replaces the Spark shuffle route,
 * BlockMatrix.scala:161-186): every rank passes ITS OWN shards.
 * Layout at rank (prow, pcol) of the pr x pc grid (see DESIGN.md §3;
 * ceil splits, last slab ragged — DenseVecMatrix.scala:1262-1265
 * semantics; my_x = mx_slab_len(x, parts, idx)):
 *   A_local: [my_m x my_ka]  rows slab prow of m,  k-cols slab pcol of k
 *   B_local: [my_kb x my_n]  k-rows slab prow of k, n-cols slab pcol of n
 *   C_local: [my_m x my_n]
 * Host-buffer entries take tight column-major shards; the engine pads
 * internally. Per k-panel the owning column broadcasts its A panel in
 * each grid row and the owning row its B panel in each grid column over
 * RCCL/xGMI, double-buffered against the MFMA stream; each C shard has
 * one owner, so no reduce exists. */
int mx_dgemm_summa(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                   const double* A_local, const double* B_local,
                   double* C_local);
int mx_sgemm_summa(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                   const float* A_local, const float* B_local,
                   float* C_local);

/* Distributed layout selector (CARMA semantics, MTUtils.scala:150-175):
 * returns 1 when splitMethod(m,k,n,nranks) leaves k unsplit (kSplit==1),
 * i.e. the k-RESIDENT layout applies — each rank keeps its A row-slab
 * with ALL K columns and its B col-slab with ALL K rows in HBM
 * (replicated across the other grid dimension) and the multiply is one
 * local GEMM with ZERO steady-state xGMI traffic (BASELINE config 4:
 * 50000x4096 · 4096x50000 on 8 GPUs). Returns 0 when the k-slabbed
 * panel-broadcast SUMMA applies. */
int mx_summa_kresident(int64_t m, int64_t k, int64_t n, int nranks);

/* k-resident distributed multiply. Shard layout at rank (prow, pcol):
 *   A_local: [my_m x K]   rows slab prow of m, ALL k columns
 *   B_local: [K x my_n]   ALL k rows, n-cols slab pcol of n
 *   C_local: [my_m x my_n]
 * Host entries take tight col-major shards; the device entry (declared
 * with the device-resident group below) takes padded pitches
 * (A roundup(my_m,128) x K cols, B roundup(K,16) x my_n,
 * C roundup(my_m,128)). No collective is issued. */
int mx_dgemm_summa_kres(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                        const double* A_local, const double* B_local,
                        double* C_local);
int mx_sgemm_summa_kres(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                        const float* A_local, const float* B_local,
                        float* C_local);

/* Ceil slab split helper (exact reference blocking semantics). */
int64_t mx_slab_len(int64_t total, int parts, int idx);
int64_t mx_slab_off(int64_t total, int parts, int idx);

/* ---- per-tile entries (the SubMatrix.multiply/add replacement) ----------
 * For a host that still does its own blocking (Marlin's Scala layer):
 * device-resident accumulate-GEMM per tile. beta_one=0: C=A*B;
 * beta_one=1: C+=A*B (the SubMatrix.add combiner folded in). */
int mx_tile_dgemm_acc(mx_ctx* ctx, int64_t tm, int64_t tk, int64_t tn,
                      const double* hA_tile, const double* hB_tile,
                      double* hC_tile, int beta_one);

/* ---- device-resident entries (buffers already in HBM; used by bench) ---- */
typedef struct mx_dbuf mx_dbuf;          /* opaque device buffer            */
int mx_alloc(mx_ctx* ctx, int64_t bytes, mx_dbuf** out);
int mx_free(mx_ctx* ctx, mx_dbuf* buf);
/* Argument contract of the auxiliary device-buffer entries (the transfers,
 * mx_fill_random, mx_zero_pad, mx_transpose_device, mx_dgemv_device and
 * mx_map; marlin_amd/csrc/aux_guards.h is the code): every argument is
 * checked before the device is selected or anything is enqueued, a
 * violation returns MX_EINVAL and has touched no buffer, and an extent is
 * compared with the size the buffer was allocated with, overflow-safely. */
/* Whole-buffer transfers: 0 <= bytes <= the buffer's size. */
int mx_upload(mx_ctx* ctx, mx_dbuf* dst, const void* src, int64_t bytes);
int mx_download(mx_ctx* ctx, void* dst, const mx_dbuf* src, int64_t bytes);
/* Fill the first n_elems elements of a device buffer, fp64 (is_fp32 = 0)
 * or fp32, with the deterministic U[0,1) stream of the randomDenVecMatrix
 * stand-in (MTUtils.scala:63-73 semantics: seeded, per-element
 * reproducible): element i is splitmix64(seed + (i+1) * 0x9E3779B97F4A7C15,
 * wrapping) >> 11, times 2^-53, and in fp32 that double rounded to nearest.
 * n_elems >= 0 and n_elems * elem <= the buffer's size, else MX_EINVAL;
 * n_elems == 0 is MX_OK and launches nothing. */
int mx_fill_random(mx_ctx* ctx, mx_dbuf* buf, int64_t n_elems,
                   uint64_t seed, int is_fp32);
/* Device-resident GEMM on padded-pitch device buffers created by the
 * helpers above. lda/ldb/ldc are element pitches.
 *
 * Pitch contract of every device GEMM entry (checked before any launch;
 * a violation returns MX_EINVAL and touches no buffer):
 *   - m and n are multiples of 128, k of 16 (the caller pads with zeros);
 *   - lda >= m, ldb >= k, ldc >= m (fused epilogue: ldc >= n, C is n x m);
 *   - every pitch is a multiple of 16 bytes, i.e. of 2 fp64 / 4 fp32
 *     elements: the kernels move 16-byte chunks (global_load_lds, float4
 *     epilogue stores), so each column start must stay 16-byte aligned;
 *   - rows [m, ldc) of C are never read or written.
 * m == 0 or n == 0 is a no-op and k == 0 means C = 0 (unchanged when
 * accumulating) on the plain entries; the fused epilogue entry has no
 * empty-shape no-op and rejects m, n or k <= 0. */
int mx_dgemm_device(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                    const mx_dbuf* dA, int64_t lda,
                    const mx_dbuf* dB, int64_t ldb,
                    mx_dbuf* dC, int64_t ldc);
int mx_sgemm_device(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                    const mx_dbuf* dA, int64_t lda,
                    const mx_dbuf* dB, int64_t ldb,
                    mx_dbuf* dC, int64_t ldc);
/* 2D pitched transfers + zeroing for device-resident matrices (the
 * RDD.cache() analog) and a beta-capable device GEMM.
 * The pitched transfers move a tight host m x n image to or from the
 * device image of pitch pitch_elems: elem is 4 or 8, m and n >= 1,
 * pitch_elems >= m, and the (n-1) * pitch_elems + m elements of the device
 * region fit the buffer, else MX_EINVAL. */
int mx_upload2d(mx_ctx* ctx, mx_dbuf* dst, int64_t pitch_elems,
                const void* src, int64_t m, int64_t n, int elem);
int mx_download2d(mx_ctx* ctx, void* dst, const mx_dbuf* src,
                  int64_t pitch_elems, int64_t m, int64_t n, int elem);
/* Zero the first bytes of the buffer: 0 <= bytes <= its size. */
int mx_memset(mx_ctx* ctx, mx_dbuf* buf, int64_t bytes);
/* out[n x m] = in[m x n]^T, both tight col-major device images. m, n >= 0
 * (either zero is a no-op MX_OK), m * n elements fit both buffers, and in
 * is not out, in handle or in device pointer (the kernel is out of place),
 * else MX_EINVAL. Elements beyond the first m * n of out are not written. */
int mx_transpose_device(mx_ctx* ctx, int is_fp32, int64_t m, int64_t n,
                        const mx_dbuf* in, mx_dbuf* out);
int mx_gemm_device_ex(mx_ctx* ctx, int is_fp32, int beta_one, int64_t m,
                      int64_t k, int64_t n, const mx_dbuf* dA, int64_t lda,
                      const mx_dbuf* dB, int64_t ldb, mx_dbuf* dC,
                      int64_t ldc);

/* Transposed-operand device GEMM: C (+)= op(A)·op(B); op(X) = X or X^T
 * per trans_x in {0,1} (any other value is MX_EINVAL). A transposed
 * operand is passed AS STORED, no transposed copy exists anywhere: the
 * kernel stages it through LDS the way it stages the other operand.
 * m, k, n are the dims of the product (op(A) m x k, op(B) k x n, C m x n).
 *
 * Pitch contract, extending the one above:
 *   - trans_a: the A image is k x m col-major with lda >= k;
 *   - trans_b: the B image is n x k col-major with ldb >= n;
 *   - rows past the logical extent up to the pitch are never read;
 *   - every pitch is still a multiple of 16 bytes, ldc >= m, and m, n
 *     are multiples of 128, k of 16. Empty shapes and k == 0 behave as on
 *     the plain entries.
 * dA == dB (one buffer in both roles, e.g. the Gram matrix A^T·A) is
 * allowed: both operands are read-only. dC must not alias either.
 * (trans_a, trans_b) = (0,0) launches the very kernel instantiation
 * mx_gemm_device_ex does. The transposed forms exist in the default
 * kernel geometry only (bk 16, bm 128, 4 waves): MARLIN_GEMM_CFG=bk32 /
 * =bm256 fall back to it for them, mx_last_gemm_config reports what ran;
 * MARLIN_GEMM_LOOP, _BAND, _REMAP and _PHASE apply as usual. The result
 * is bit-identical to the plain entry run on a materialised transpose.
 * Stats (flops, gemm_ms, gemm_launches) as mx_gemm_device_ex. */
int mx_gemm_device_op(mx_ctx* ctx, int is_fp32, int beta_one, int trans_a,
                      int trans_b, int64_t m, int64_t k, int64_t n,
                      const mx_dbuf* dA, int64_t lda, const mx_dbuf* dB,
                      int64_t ldb, mx_dbuf* dC, int64_t ldc);
/* op of the most recent plain GEMM launch (0,0 after an NN launch, and
 * before the first launch) */
int mx_last_gemm_op(mx_ctx* ctx, int* trans_a, int* trans_b);

/* Grouped GEMM: count independent products C_i (+)= op(A_i)·op(B_i) in ONE
 * kernel launch whose grid is the union of all their 128x128 C tiles, so
 * many small products fill the GPU the way one large one does. Type,
 * beta_one and the op form are uniform per call; shapes, pitches, buffers
 * and element offsets into the buffers are per problem. Each C tile runs
 * the k-loop the plain entry runs, so the result of a problem is
 * bit-identical to mx_gemm_device_op on that problem alone.
 *
 * Per problem the pitch contract is that of mx_gemm_device_op (m, n
 * multiples of 128, k of 16; the trans_* meaning of lda / ldb), and each
 * offset times the element size is a multiple of 16 bytes.
 *
 * The WHOLE table is validated before anything is enqueued; a violation
 * returns MX_EINVAL and touches no buffer. Refused: a contract violation,
 * a NULL buffer in a non-empty problem, a region that does not fit its
 * buffer (off + (cols-1)*ld + rows elements), count < 0, NULL problems
 * with count > 0, a trans_* outside {0,1}, and aliasing: every C region
 * must be disjoint from every other problem's C region and from every A
 * and B region of the call. Two regions of one buffer are disjoint only
 * when their byte spans are, or when their pitches are equal and they are
 * disjoint rectangles (rows off % ld .. +rows, columns off / ld .. +cols,
 * with off % ld + rows <= ld). A and B regions may repeat and overlap
 * freely (one panel feeding a row of updates; dA == dB, the Gram form).
 *
 * A problem with m == 0 or n == 0 is skipped; k == 0 zeroes the C region
 * when beta_one == 0 and leaves it alone otherwise; count == 0, or a call
 * with nothing left to launch, returns MX_OK and launches no kernel.
 *
 * The default kernel geometry only (bk 16, bm 128, 4 waves), as for the
 * transposed forms: MARLIN_GEMM_CFG is ignored, MARLIN_GEMM_LOOP is
 * honoured (default: fp64 pipelined, fp32 two-barrier; one pitch of 2^26
 * elements or more puts the whole launch on the two-barrier loop),
 * MARLIN_GEMM_BAND and _REMAP apply per problem, _PHASE is not applied.
 * Stats: flops = sum of 2mkn, gemm_ms = event time of the one launch,
 * gemm_launches = 1 (0 when nothing launched). mx_last_gemm_config (band
 * = that of the first table entry), _op and _loop report the launch. */
typedef struct {
  int64_t m, k, n;        /* dims of the product, padded: m, n % 128 == 0, k % 16 == 0 */
  const mx_dbuf* dA; int64_t a_off, lda;   /* offsets and pitches in elements */
  const mx_dbuf* dB; int64_t b_off, ldb;
  mx_dbuf*       dC; int64_t c_off, ldc;
} mx_gemm_problem_t;
int mx_gemm_device_grouped(mx_ctx* ctx, int is_fp32, int beta_one,
                           int trans_a, int trans_b, int count,
                           const mx_gemm_problem_t* problems);
/* Problems that reached the kernel and grid size (blocks) of the most
 * recent grouped launch in this process; zeros before the first. */
int mx_last_gemm_group(mx_ctx* ctx, int* problems_launched, int64_t* blocks);

/* Split-K GEMM: C (+)= op(A)·op(B) with k cut into S slices that run as S
 * times as many blocks, for products whose m/128 x n/128 tiles alone leave
 * the GPU idle (a tall-skinny Gram matrix, a small C with a long k).
 *
 * Arguments and pitch contract are mx_gemm_device_op's, empty shapes too
 * (m == 0 or n == 0 is a no-op, k == 0 clears C unless accumulating). In
 * addition every region must fit its buffer and C must be disjoint from A
 * and B, by the rules of mx_gemm_device_grouped (dA == dB stays allowed).
 * Everything is checked before anything is enqueued or allocated: a
 * refused call returns MX_EINVAL and touches no buffer.
 *
 * slices: 0 = auto, 1 = do not split, >= 2 = that many, clamped to k / 16;
 * < 0 is MX_EINVAL. Auto (gemm_splitk_plan.h) keeps S = 1 when the tiles
 * already reach its fill target (measured: one block per CU in fp64, two
 * in fp32, half of what the device holds) and otherwise cuts k until
 * S * tiles reaches it, never leaving a slice fewer than
 * MX_SPLITK_MIN_KSTEPS k-steps of 16.
 *
 * Effective S == 1 is the launch of mx_gemm_device_op, bit for bit, with
 * no workspace. For S >= 2 slice s covers the k-steps [start_s, start_s +
 * len_s) of 16: contiguous, ascending, lengths differing by at most one
 * step, the longer slices first. The slices run as ONE grouped launch, a
 * second kernel on the same stream then adds the partial products in
 * ascending slice order with plain adds in the element type:
 *     beta_one == 0:  C = ((P_0 + P_1) + P_2) + ...
 *     beta_one == 1:  C = (((C + P_0) + P_1) + P_2) + ...
 * where P_s is bit for bit what mx_gemm_device_op (beta 0) returns on
 * slice s alone. The result therefore depends on S, but for a given S not
 * on the schedule, the device's load or the run: no atomics are involved.
 * Partial products live in a workspace the context owns (tight m x n
 * slabs; S - 1 of them, slice 0 going straight into C, or S when
 * accumulating), grown on demand and freed by mx_shutdown; auto never needs
 * more than 64 MiB of it. Rows [m, ldc) of C are neither read nor written.
 *
 * The grouped entry's limits apply: the default kernel geometry only,
 * MARLIN_GEMM_LOOP, _BAND and _REMAP honoured, _CFG and _PHASE not, one
 * pitch of 2^26 elements or more puts the launch on the two-barrier loop.
 * Stats: flops = 2mkn, gemm_launches = 1, gemm_ms = event time over the
 * GEMM and the reduce. mx_last_gemm_group reports (S, S * tiles),
 * mx_last_gemm_config, _op and _loop the grouped launch (beta_one = 0 even
 * when accumulating: the accumulation happens in the reduce). */
int mx_gemm_device_splitk(mx_ctx* ctx, int is_fp32, int beta_one, int trans_a,
                          int trans_b, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* dA, int64_t lda,
                          const mx_dbuf* dB, int64_t ldb,
                          mx_dbuf* dC, int64_t ldc, int slices);
/* Effective S and workspace bytes used by the most recent split-K call in
 * this process: (1, 0) after an unsplit one, (0, 0) before the first. */
int mx_last_gemm_splitk(mx_ctx* ctx, int* slices, int64_t* workspace_bytes);

/* Triangular solve (BLAS TRSM with alpha = 1) on device images, fp64
 * (is_fp32 = 0) or fp32:
 *     side = 0:  op(T) * X = B,  B stored n x r   (r right-hand-side columns)
 *     side = 1:  X * op(T) = B,  B stored r x n   (r right-hand-side rows)
 * op(T) = T or T^T per trans, T triangular of order n, lower or upper per
 * lower, with an implied unit diagonal when unit_diag. X overwrites B. T is
 * read AS STORED: no transposed copy is made. All 16 forms exist in both
 * element types; every flag, is_fp32 included, is 0 or 1.
 *
 * Sizes and pitches. n is the logical order; np = n rounded up to 128.
 * r is a multiple of 128. The T image is np x np at pitch ldt >= np. The B
 * image is np x r with ldb >= np (left) or r x np with ldb >= r (right).
 * Both pitches are multiples of 16 bytes.
 *
 * What is read. Of T only the referenced triangle: the opposite triangle is
 * never read, and with unit_diag neither is the diagonal, so a packed L\U
 * factor serves as L (lower, unit) and as U (upper) from one buffer. Inside
 * the last diagonal block nothing at a row or column index >= n is read:
 * the block is continued as the identity. The off-diagonal 128 x 128 blocks
 * of the referenced triangle are read whole by a GEMM, so their part at an
 * index >= n must be zero (what a zero-initialised padded image holds).
 *
 * What is written. The pad rows (left) or columns (right) [n, np) of B must
 * be zero on entry and are zero on exit. Rows of B past np (left) or past r
 * (right), up to the pitch, are neither read nor written, nor is anything
 * past the last column of the image.
 *
 * Checks. Everything is checked before anything is enqueued or allocated
 * (marlin_amd/csrc/trsm_plan.h is the code): the flags, n and r >= 0 and r a
 * multiple of 128, NULL handles, the pitches, both images against the sizes
 * their buffers were allocated with (overflow-safely), and aliasing: dT and
 * dB must be different handles whose device ranges share no byte. A refused
 * call returns MX_EINVAL and has touched no buffer. n == 0 or r == 0 is a
 * no-op that returns MX_OK and looks at neither buffer. A zero on the
 * diagonal gives inf / NaN as in BLAS; no singularity check is made.
 *
 * Algorithm, fixed so that the result does not depend on the schedule or
 * the run. Blocks are 128 wide; with eff_lower = lower XOR trans the left
 * side sweeps the blocks forward when eff_lower and the right side when
 * !eff_lower, otherwise backward. Step j (a) solves diagonal block j against
 * all r right-hand sides with the diagonal kernel, substitution in
 * ascending order of the eliminated index, each update one fused
 * multiply-add and each quotient one division in both element types
 * (trsm_plan.h, mx_trsm_update and mx_trsm_quot), which writes X_j into B and -X_j
 * into a workspace panel of 128 * r elements the context owns (grown on
 * demand, freed by mx_shutdown), then (b) accumulates into ALL remaining
 * blocks with one launch of the plain GEMM (beta_one = 1, k = 128):
 *     left:   B_rest += op(T)[rest, j] * (-X_j)
 *     right:  B_rest += (-X_j) * op(T)[j, rest]
 * with op(T)'s block passed as stored under the GEMM's trans_a / trans_b.
 * No atomics; the GEMM is an existing instantiation of the closed list.
 *
 * Stats: flops = n * n * r, gemm_launches = the update GEMMs launched
 * (np / 128 - 1), gemm_ms = event time over the whole sweep, diagonal
 * kernels included; the other fields are zero. mx_last_gemm_config, _op and
 * _loop report the last update GEMM of the sweep (unchanged when n <= 128,
 * which has none). */
int mx_trsm_device(mx_ctx* ctx, int is_fp32, int side, int lower, int trans,
                   int unit_diag, int64_t n, int64_t r,
                   const mx_dbuf* dT, int64_t ldt, mx_dbuf* dB, int64_t ldb);

/* LU factorisation on a device image, in place: blocked, right-looking,
 * with the row permutation kept on the device. No host step and no PCIe
 * traffic inside the sweep; the factor stays where mx_trsm_device reads it.
 *
 * Layout. The order-n matrix is a column-major image of np rows and np
 * columns, np = n rounded up to 128, at pitch lda >= np, a multiple of 16
 * bytes. The pads (rows and columns [n, np)) must be zero on entry and are
 * zero on exit: the image Engine.upload_matrix makes. On return the image
 * holds packed L\U, L unit-lower and U upper, the form mx_trsm_device reads
 * as both factors. dPiv holds np int32: piv[g] for g < n is the source row
 * of output row g, so that A[piv] == L * U with WHOLE rows moved (the L
 * columns already finished are permuted with the rest; no fix-up remains
 * for the host); piv[g] = g on the pad.
 *
 * Pivoting is partial pivoting INSIDE each 128 x 128 diagonal block, the
 * reference's block-pivot scheme at the device's block width. In column j
 * of a block the pivot is the entry of largest magnitude among the block's
 * remaining rows; the test is |a| > best, so ties go to the lowest row
 * index and a NaN is never chosen while another entry remains. Limitation:
 * a pivot is never taken from another block row. A matrix whose diagonal
 * block is singular, or nearly so, when its step comes is therefore not
 * handled any better than the host path handles it at its base_size: an
 * exactly zero pivot is reported through info, a tiny one is divided by.
 *
 * info. *info is 0 on success. If a pivot is exactly zero, *info is the
 * 1-based global column of the FIRST such pivot; that column is left
 * unscaled and the factorisation runs to the end, as LAPACK's does (U is
 * then singular). The block itself is finished as stated; what lies below
 * it is solved against its U (step 3 below), so from that column on the
 * rows under the block, and the trailing matrix after them, hold inf / NaN.
 * info travels through one 4-byte device word that is read back once, after
 * the sweep.
 *
 * Algorithm, fixed so that the result does not depend on the schedule or
 * the run. Step j (block offset o = 128 j), in stream order: (1) the
 * diagonal kernel factors block (j, j) in LDS, elimination right-looking
 * with ascending columns and rows, multiplier a / pivot, update by one
 * fused multiply-add (marlin_amd/csrc/getrf_plan.h, mx_getrf_eliminate, is
 * the statement), and writes its 128 permutation entries; (2) the
 * row-permutation kernel applies them to rows [o, o + 128) of columns
 * [0, o) and [o + 128, np); (3) L21 = A21 U11^-1 and (4) U12 = L11^-1 (P
 * A12) by the triangular solve's diagonal kernel, the second leaving -U12
 * in the context's workspace panel; (5) A22 += L21 * (-U12), one launch of
 * the plain accumulating GEMM (k = 128). (3)-(5) only while blocks remain.
 * No atomics.
 *
 * Checks. Everything is checked before anything is allocated or enqueued
 * (getrf_plan.h is the code): the flag, n >= 0, NULL handles and a NULL
 * info, the pitch, the image and the np * 4 bytes of dPiv against the sizes
 * their buffers were allocated with (overflow-safely), and dA and dPiv as
 * different handles whose device ranges share no byte. A refused call
 * returns MX_EINVAL and has touched nothing (*info included). n == 0
 * returns MX_OK with *info = 0 and looks at neither buffer.
 *
 * Stats: flops = 2 n^3 / 3, gemm_launches = the update GEMMs launched
 * (np / 128 - 1), gemm_ms = event time over the whole sweep. */
int mx_getrf_device(mx_ctx* ctx, int is_fp32, int64_t n, mx_dbuf* dA,
                    int64_t lda, mx_dbuf* dPiv, int* info);

/* Introspection: the gemm_mfma_kernel instantiation and remap arguments
 * of the most recent plain GEMM launch in this process (any entry that
 * reaches the kernel launcher; all zero before the first launch). The
 * MARLIN_GEMM_CFG / _REMAP / _BAND / _PHASE knobs are latched per
 * process and fall back silently when a shape does not divide, so this
 * is how a test proves which variant it ran. */
typedef struct {
  int is_fp32;     /* 0 = fp64, 1 = fp32                                   */
  int beta_one;    /* 1 = accumulating instantiation (C += A*B)            */
  int bk;          /* k-step: 16 or 32                                     */
  int bm;          /* block tile rows: 128 or 256                          */
  int waves;       /* waves per block: 4 (2x2) or 8 (2x4, 4x2)             */
  int band;        /* block-column band width; < 0 = plain band order      */
  int phase_mask;  /* k-phase stagger mask, 0 = off                        */
} mx_gemm_cfg_t;
int mx_last_gemm_config(mx_ctx* ctx, mx_gemm_cfg_t* out);

/* The k-loop of that same launch: 1 = pipelined across tiles (one
 * barrier per k-step; the default of every variant but fp32 at bk 16),
 * 0 = two-barrier loop. The latched MARLIN_GEMM_LOOP=twobar / =pipe
 * knob forces one loop for every variant; a pitch of 2^26 elements or
 * more, which the pipelined loop's 32-bit lane offsets do not cover,
 * always takes the two-barrier loop. 0 before the first launch. Both
 * loops give bit-identical results. */
int mx_last_gemm_loop(mx_ctx* ctx, int* out);

/* SUMMA on device-resident local shards (bench hot loop: inputs already
 * in HBM when the timed region starts). Shard pitches are the PADDED
 * sizes: A_local pitch roundup(my_m,128) x my_ka cols; B_local pitch
 * roundup(my_kb,16) x my_n cols; C_local pitch roundup(my_m,128).
 * C_local is written as the whole padded image roundup(my_m,128) x
 * roundup(my_n,128). Pad contract: B_local's pad rows are never read and
 * the panel pack zeroes the k pad and the columns my_n..roundup(my_n,128)
 * of every B panel, so C_local's pad columns are exactly zero, and its
 * pad rows are exactly zero whenever A_local's pad rows are zero (the
 * image can feed the next device GEMM or transpose as it stands). */
int mx_dgemm_summa_device(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* dA_local, const mx_dbuf* dB_local,
                          mx_dbuf* dC_local);
int mx_sgemm_summa_device(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* dA_local, const mx_dbuf* dB_local,
                          mx_dbuf* dC_local);
/* k-resident layout on device-resident shards (see mx_summa_kresident). */
int mx_gemm_summa_kres_device(mx_ctx* ctx, int is_fp32, int64_t m, int64_t k,
                              int64_t n, const mx_dbuf* dA_local,
                              const mx_dbuf* dB_local, mx_dbuf* dC_local);
/* Virtual rank: the panel loop of mx_*_summa_device for position
 * (prow, pcol) of a pr x pc grid, on one GPU and without a communicator.
 * dA_row holds the pc shards A_local of (prow, j), dB_col the pr shards
 * B_local of (i, pcol), in the layouts above (an entry may be NULL where
 * that shard is empty). Each panel is packed from its root's shard into
 * this position's own panel buffers, which is what the broadcast would
 * have delivered; everything else (plan, k-padding, double buffering,
 * events, accumulate chain, pad contract) is the code the real entries
 * run. kb_max is the panel width, 0 = default / MARLIN_SUMMA_KB.
 * MX_EINVAL for a bad grid or position or NULL arrays; an empty shard
 * (my_m == 0 or my_n == 0) returns MX_OK and launches nothing. mx_stats
 * reports gemm_launches, comm_ms == 0. */
int mx_gemm_summa_virtual(mx_ctx* ctx, int is_fp32, int pr, int pc, int prow,
                          int pcol, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* const* dA_row,
                          const mx_dbuf* const* dB_col, mx_dbuf* dC_local,
                          int64_t kb_max);

/* Restore the zero-pad invariant of a rows_total x cols_total padded
 * image (pitch ld) whose logical content is m x n: pads outside m x n
 * are zeroed (used after mx_fill_random of a whole padded buffer); the
 * m x n interior, rows [rows_total, ld) and everything past column
 * cols_total are not written. 0 <= m <= rows_total <= ld, 0 <= n <=
 * cols_total, and the (cols_total-1) * ld + rows_total elements of the
 * image fit the buffer, else MX_EINVAL; an empty image (rows_total or
 * cols_total == 0) is a no-op MX_OK. */
int mx_zero_pad(mx_ctx* ctx, mx_dbuf* buf, int64_t rows_total,
                int64_t cols_total, int64_t ld, int64_t m, int64_t n,
                int is_fp32);

/* Download starting at a byte offset (one COLUMN of a padded col-major
 * image: off = j * pitch * elem). */
int mx_download_off(mx_ctx* ctx, void* dst, const mx_dbuf* src,
                    int64_t off_bytes, int64_t bytes);
/* Pitched download starting at a byte offset (one ROW of a col-major
 * image: off = i * elem, m = 1, n = cols, pitch = ld). The contract of
 * mx_download2d, with off_bytes >= 0 and the region counted from there. */
int mx_download2d_off(mx_ctx* ctx, void* dst, const mx_dbuf* src,
                      int64_t off_bytes, int64_t pitch_elems, int64_t m,
                      int64_t n, int elem);

/* Device-resident fused-epilogue GEMM (config 5 timed leg): C[n x m] =
 * (A*B)^T (+ addC), padded dims, ldc = padded-n pitch of C/addC;
 * dAdd may be NULL. */
int mx_sgemm_epilogue_device(mx_ctx* ctx, int64_t m, int64_t k, int64_t n,
                             const mx_dbuf* dA, int64_t lda,
                             const mx_dbuf* dB, int64_t ldb, mx_dbuf* dC,
                             int64_t ldc, const mx_dbuf* dAdd);

/* Failure-injection probe: issues an invalid RCCL collective
 * on the world communicator; a healthy engine surfaces MX_ERCCL (no
 * abort) and keeps serving calls afterwards. */
int mx_test_rccl_error(mx_ctx* ctx);

/* ---- elementwise / reduction / transpose (BlockMatrix epilogue ops,
 * BlockMatrix.scala:344-523; DenseVecMatrix.scala scalar ops) ---------- */
#define MX_OP_ADD   0   /* C = A + B          (add(other))              */
#define MX_OP_SUB   1   /* C = A - B          (subtract(other))         */
#define MX_OP_EMUL  2   /* C = A .* B         (dotProduct(other))       */
#define MX_OP_ADDS  3   /* C = A + s          (add(b))                  */
#define MX_OP_SUBS  4   /* C = A - s          (subtract(b))             */
#define MX_OP_RSUBS 5   /* C = s - A          (subtractBy(b))           */
#define MX_OP_MULS  6   /* C = A * s          (multiply(b))             */
#define MX_OP_DIVS  7   /* C = A / s          (divide(b))               */
#define MX_OP_RDIVS 8   /* C = s / A          (divideBy(b))             */
/* op is one of the codes above, anything else is MX_EINVAL; ADD, SUB and
 * EMUL read B, which must not be NULL for them. IEEE arithmetic in the
 * element type: NaN and infinities propagate, signed zeros are kept. */
int mx_map(mx_ctx* ctx, int op, int is_fp32, int64_t n, const void* A,
           const void* B /* null for scalar ops */, double scalar, void* C);
/* mx_map on device buffers, nothing crosses PCIe: the first n elements of
 * dA (and of dB for ADD, SUB, EMUL; NULL otherwise) into the first n of dC.
 * n >= 0 and n elements fit every buffer named, is_fp32 in {0,1}, op as
 * above, else MX_EINVAL; n == 0 is a no-op. dC may be dA or dB (in place). */
int mx_map_device(mx_ctx* ctx, int op, int is_fp32, int64_t n,
                  const mx_dbuf* dA, const mx_dbuf* dB, double scalar,
                  mx_dbuf* dC);
int mx_sum(mx_ctx* ctx, int is_fp32, int64_t n, const void* A, double* out);
int mx_transpose(mx_ctx* ctx, int is_fp32, int64_t m, int64_t n,
                 const void* A, void* C /* n x m col-major */);

/* Matrix-vector multiply (BlockMatrix.multiply(DistributedVector/BDV),
 * BlockMatrix.scala:240-274): y = A x, A col-major m x n. */
int mx_dgemv(mx_ctx* ctx, int64_t m, int64_t n, const double* A,
             const double* x, double* y);

/* Device-resident gemv on a cached matrix (mx_dbuf + pitch), fp64: y = A x
 * with A the m x n col-major image of pitch lda in dA, x and y host
 * vectors. m, n >= 1, lda >= m, and the (n-1) * lda + m elements of the
 * image fit dA, else MX_EINVAL. Rows [m, lda) of the image and anything
 * past column n are never read. */
int mx_dgemv_device(mx_ctx* ctx, int64_t m, int64_t n, const mx_dbuf* dA,
                    int64_t lda, const double* x, double* y);

/* ---- timing / stats (MTUtils.evaluate + RMMcompare.scala:47-51 analog) -- */
typedef struct {
  double h2d_ms;          /* host->device copies of the last call           */
  double d2h_ms;          /* device->host copies                            */
  double pack_ms;         /* padding/pack kernels                           */
  double gemm_ms;         /* sum of dgemm kernel time (hipEvent, gemm strm) */
  double comm_ms;         /* RCCL panel broadcast time (comm stream)        */
  double total_ms;        /* wall of the whole entry                        */
  int64_t gemm_launches;  /* number of GEMM kernel launches                 */
  double flops;           /* algorithmic flops of the last call (2mkn)      */
  double bytes_moved;     /* algorithmic HBM bytes (inputs+outputs, padded) */
} mx_stats_t;
int mx_stats(mx_ctx* ctx, mx_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MARLIN_GPU_H */
