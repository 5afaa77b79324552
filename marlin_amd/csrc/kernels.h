// kernels.h — the C-visible launchers of kernels.hip, as marlin_gpu.cpp
// calls them. Both files include this, so a signature cannot drift between
// the definition and its caller. Every launcher enqueues on `stream` and
// returns 0, -4 (refused argument: nothing enqueued) or -2 (HIP failure).
#ifndef MARLIN_KERNELS_H
#define MARLIN_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/marlin_gpu.h"   // mx_gemm_cfg_t
#include "gemm_group_plan.h"            // mx_group_plan

// What the last mxk_gemm / mxk_gemm_op / mxk_gemm_grouped launched (the
// mx_last_gemm_* entries): the env knobs are latched per process, so a test
// can only prove which instantiation it exercised by reading this back. A
// grouped launch writes every field, a plain one leaves the group fields
// alone, mxk_sgemm_tn_epilogue writes nothing. The split-K fields are the
// split-K entry's alone (mxk_note_splitk): no launcher touches them.
struct mxk_last_gemm_t {
  mx_gemm_cfg_t cfg;
  int loop;                 // 0 = two-barrier, 1 = pipelined
  int trans_a, trans_b;     // op(A), op(B): 1 = transposed
  int group_problems;       // last grouped launch: problems that ran
  int64_t group_blocks;     //                      and its grid size
  int splitk_slices;        // last split-K call: effective S (1 = unsplit)
  int64_t splitk_ws_bytes;  //                    and workspace it used
};

extern "C" {
void mxk_last_gemm(mxk_last_gemm_t* out);
void mxk_note_splitk(int slices, int64_t workspace_bytes);
// the latched MARLIN_GEMM_* knobs (what the grouped plan's bands need)
const mx_gemm_knobs* mxk_gemm_knobs(void);

int mxk_gemm(int is_fp32, int beta_one, int64_t M, int64_t N, int64_t K,
             const void* A, int64_t lda, const void* B, int64_t ldb,
             void* C, int64_t ldc, hipStream_t stream);
int mxk_gemm_op(int is_fp32, int beta_one, int trans_a, int trans_b,
                int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                const void* B, int64_t ldb, void* C, int64_t ldc,
                hipStream_t stream);
int mxk_gemm_grouped(int is_fp32, int beta_one, int trans_a, int trans_b,
                     const mx_group_plan* plan, void* ws, hipStream_t stream);
// C (m x n, pitch ldc) += W_0 + ... + W_{nslabs-1} as a left fold in the
// element type; slab j is the tight m x n image at W + j * m * n.
int mxk_splitk_reduce(int is_fp32, int64_t m, int64_t n, void* C, int64_t ldc,
                      const void* W, int nslabs, hipStream_t stream);
// One 128 x 128 diagonal block of mx_trsm_device against r right-hand
// sides: X overwrites its strip of B, -X fills the workspace panel ws
// (128 * r elements). tt, rev, unit, nv as mx_trsm_stage (trsm_plan.h).
int mxk_trsm_diag(int is_fp32, int side, int tt, int rev, int unit, int nv,
                  const void* Tjj, int64_t ldt, void* X, int64_t ldx,
                  void* ws, int64_t r, hipStream_t stream);
// One 128 x 128 diagonal block of mx_getrf_device, factored in place with
// pivoting among its own rows (mx_getrf_eliminate, getrf_plan.h): piv gets
// the block's 128 global source rows, *first_zero the 1-based global column
// of a zero pivot if it still holds 0. Then that permutation applied to
// rows [o, o + 128) of every other column of the np x np image.
int mxk_getrf_diag(int is_fp32, int nv, int64_t o, void* Ajj, int64_t lda,
                   int* piv, int* first_zero, hipStream_t stream);
int mxk_getrf_rowperm(int is_fp32, int64_t o, int64_t np, void* A,
                      int64_t lda, const int* piv, hipStream_t stream);
int mxk_sgemm_tn_epilogue(int64_t M, int64_t N, int64_t K, const float* A,
                          int64_t lda, const float* B, int64_t ldb, float* C,
                          int64_t ldc, const float* addC, hipStream_t stream);
int mxk_fill_random(int is_fp32, void* buf, int64_t m, int64_t n, int64_t ld,
                    uint64_t seed, hipStream_t stream);
int mxk_zero_pad(int is_fp32, void* buf, int64_t rows_total,
                 int64_t cols_total, int64_t ld, int64_t m, int64_t n,
                 hipStream_t stream);
int mxk_map(int is_fp32, int op, int64_t n, const void* a, const void* b,
            double scalar, void* c, hipStream_t stream);
int mxk_sum(int is_fp32, int64_t n, const void* a, double* partials,
            double* out, hipStream_t stream);
int mxk_transpose(int is_fp32, int64_t m, int64_t n, const void* in,
                  void* out, hipStream_t stream);
int mxk_gemv(int is_fp32, int64_t m, int64_t n, int64_t lda, const void* A,
             const void* x, double* partial, void* y, hipStream_t stream);
}

#endif  // MARLIN_KERNELS_H
