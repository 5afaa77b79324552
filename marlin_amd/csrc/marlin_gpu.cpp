// marlin_gpu.cpp — host runtime of the MI355X-native block-matrix multiply
// engine behind the C ABI of include/marlin_gpu.h.
//
// Replaces, MI355X-first, the reference's distributed machinery:
//   - Spark shuffle emit/join/reduce (BlockMatrix.scala:161-186,
//     DenseVecMatrix.scala:109-141) -> 2-D grid SUMMA with RCCL panel
//     broadcasts over xGMI, double-buffered against the MFMA stream.
//     Each C shard has ONE owner, so the reference's reduceByKey add
//     (SubMatrix.scala:41-50) disappears into the GEMM accumulator.
//   - MatrixMultPartitioner (MatrixMultPartitioner.scala:6-33) -> the
//     pr x pc rank grid + ceil slab ownership (mx_slab_*).
//   - MTUtils.evaluate timing (MTUtils.scala:218-220) -> hipEvent stage
//     timers surfaced through mx_stats.
//
// One process per GPU; mx_ctx is externally synchronized.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <utility>

#include "../../include/marlin_gpu.h"
#include "host_stage.h"          // the staging of the host-buffer entries
#include "gemm_group_plan.h"   // struct mx_dbuf, the grouped-GEMM plan
#include "gemm_splitk_plan.h"  // the split-K slicing policy
#include "trsm_plan.h"         // the triangular solve: check and step list
#include "getrf_plan.h"        // the LU factorisation: check and step list
#include "aux_guards.h"        // argument checks of the auxiliary entries
#include "kernels.h"           // the kernels.hip launchers

#define HIP_OK(x)                                                        \
  do {                                                                   \
    hipError_t _e = (x);                                                 \
    if (_e != hipSuccess) {                                              \
      fprintf(stderr, "[marlin_gpu] HIP error %s at %s:%d\n",            \
              hipGetErrorString(_e), __FILE__, __LINE__);                \
      return MX_EHIP;                                                    \
    }                                                                    \
  } while (0)

#define RCCL_OK(x)                                                       \
  do {                                                                   \
    ncclResult_t _e = (x);                                               \
    if (_e != ncclSuccess) {                                             \
      fprintf(stderr, "[marlin_gpu] RCCL error %s at %s:%d\n",           \
              ncclGetErrorString(_e), __FILE__, __LINE__);               \
      return MX_ERCCL;                                                   \
    }                                                                    \
  } while (0)

static inline int64_t round_up(int64_t x, int64_t a) {
  return (x + a - 1) / a * a;
}

// ceil slab split — DenseVecMatrix.scala:1262-1265 blocking semantics
int64_t mx_slab_len(int64_t total, int parts, int idx) {
  int64_t bl = (total + parts - 1) / parts;
  int64_t start = (int64_t)idx * bl;
  if (start >= total) return 0;
  return bl < total - start ? bl : total - start;
}
int64_t mx_slab_off(int64_t total, int parts, int idx) {
  int64_t bl = (total + parts - 1) / parts;
  return (int64_t)idx * bl;
}

// The C shard of grid position (prow, pcol) of an m x n product on a
// pr x pc grid: its logical size and the padded size of its device image.
struct shard_t {
  int64_t mi, nj, mip, njp;
};
static shard_t local_shard(int64_t m, int64_t n, int pr, int pc, int prow,
                           int pcol) {
  const int64_t mi = mx_slab_len(m, pr, prow), nj = mx_slab_len(n, pc, pcol);
  return {mi, nj, round_up(mi, 128), round_up(nj, 128)};
}

// The roles of the context's events.
enum mx_event {
  EV_TIMED_BEGIN, EV_TIMED_END,        // timed(): around what it enqueues
  EV_H2D_BEGIN, EV_H2D_END,            // gemm_host: around the stage-in
  EV_D2H,                              // gemm_host: kernel done, download
  EV_GEMM_DONE0, EV_GEMM_DONE1,        // SUMMA: GEMM done with panel buffer b
  EV_PANEL_READY0, EV_PANEL_READY1,    // SUMMA: panel buffer b packed
  EV_COUNT
};

struct mx_ctx {
  int device = 0;
  hipStream_t s_gemm = nullptr;
  hipStream_t s_copy = nullptr;
  hipStream_t s_comm = nullptr;
  hipEvent_t ev[EV_COUNT] = {};
  // distributed
  int rank = 0, nranks = 1;
  int pr = 1, pc = 1, prow = 0, pcol = 0;
  ncclComm_t world = nullptr, rowc = nullptr, colc = nullptr;
  bool have_comm = false;
  // cached workspaces for the host-buffer entries
  mx_dbuf wsA, wsB, wsC, wsPA[2], wsPB[2];
  // grouped GEMM: the device table's staging buffer and its host image
  mx_dbuf wsG;
  mx_group_plan group_plan;
  // split-K GEMM: the partial products (tight m x n slabs), the slice table
  // handed to the grouped plan, and the CU count the auto policy reads
  mx_dbuf wsK;
  std::vector<mx_splitk_slice> splitk_slices;
  std::vector<mx_gemm_problem_t> splitk_rows;
  int cus = 0;
  // triangular solve: the -X_j panel (128 * r elements) and the step list
  mx_dbuf wsT;
  mx_trsm_plan trsm_plan;
  // LU factorisation: the first-zero-pivot word (4 bytes) and the step list;
  // its -U12 panel is wsT
  mx_dbuf wsI;
  mx_getrf_plan getrf_plan;
  mx_stats_t st = {};
};

static int ensure(mx_ctx* c, mx_dbuf* b, int64_t bytes) {
  if (b->bytes >= bytes) return MX_OK;
  if (b->ptr) (void)hipFree(b->ptr);
  b->ptr = nullptr;
  b->bytes = 0;
  hipError_t e = hipMalloc(&b->ptr, (size_t)bytes);
  if (e != hipSuccess) return MX_ENOMEM;
  b->bytes = bytes;
  return MX_OK;
}

const char* mx_strerror(int code) {
  switch (code) {
    case MX_OK: return "ok";
    case MX_EDIM: return "dimension mismatch during matrix-matrix multiplication";
    case MX_EHIP: return "HIP runtime failure";
    case MX_ENOMEM: return "device allocation failure";
    case MX_EINVAL: return "invalid argument";
    case MX_ENOCOMM: return "distributed entry before mx_comm_init";
    case MX_ERCCL: return "RCCL failure";
    case MX_ENODEV: return "no GPU device visible";
    default: return "unknown error";
  }
}

// destroys the streams/events a ctx created (a partially-initialised one
// included) and the ctx itself
static void ctx_teardown(mx_ctx* c) {
  for (int i = 0; i < EV_COUNT; i++)
    if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  if (c->s_gemm) (void)hipStreamDestroy(c->s_gemm);
  if (c->s_copy) (void)hipStreamDestroy(c->s_copy);
  if (c->s_comm) (void)hipStreamDestroy(c->s_comm);
  delete c;
}

int mx_init(mx_ctx** out, int device) {
  if (!out) return MX_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MX_ENODEV;
  mx_ctx* c = new mx_ctx();
  c->device = device < 0 ? 0 : device;
  if (hipSetDevice(c->device) != hipSuccess) { delete c; return MX_ENODEV; }
  if (hipStreamCreate(&c->s_gemm) != hipSuccess ||
      hipStreamCreate(&c->s_copy) != hipSuccess ||
      hipStreamCreate(&c->s_comm) != hipSuccess) {
    ctx_teardown(c);
    return MX_EHIP;
  }
  for (int i = 0; i < EV_COUNT; i++)
    if (hipEventCreate(&c->ev[i]) != hipSuccess) { ctx_teardown(c); return MX_EHIP; }
  *out = c;
  return MX_OK;
}

int mx_shutdown(mx_ctx* c) {
  if (!c) return MX_EINVAL;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  if (c->rowc && c->rowc != c->world) ncclCommDestroy(c->rowc);
  if (c->colc && c->colc != c->world) ncclCommDestroy(c->colc);
  if (c->world) ncclCommDestroy(c->world);
  for (mx_dbuf* b : {&c->wsA, &c->wsB, &c->wsC,
                     &c->wsPA[0], &c->wsPA[1], &c->wsPB[0], &c->wsPB[1],
                     &c->wsG, &c->wsK, &c->wsT, &c->wsI})
    if (b->ptr) (void)hipFree(b->ptr);
  ctx_teardown(c);
  return MX_OK;
}

int mx_comm_id(char unique_id[MX_UNIQUE_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= MX_UNIQUE_ID_BYTES, "id size");
  ncclUniqueId id;
  RCCL_OK(ncclGetUniqueId(&id));
  memset(unique_id, 0, MX_UNIQUE_ID_BYTES);
  memcpy(unique_id, &id, sizeof(id));
  return MX_OK;
}

static void grid_shape(int nranks, int* pr, int* pc) {
  // MARLIN_GRID=RxC overrides (e.g. 2x4 for the 8-GPU grid sweep)
  const char* g = getenv("MARLIN_GRID");
  if (g) {
    int r = 0, cc = 0;
    if (sscanf(g, "%dx%d", &r, &cc) == 2 && r > 0 && cc > 0 &&
        r * cc == nranks) {
      *pr = r;
      *pc = cc;
      return;
    }
  }
  switch (nranks) {
    case 8: *pr = 4; *pc = 2; break;
    case 4: *pr = 2; *pc = 2; break;
    case 2: *pr = 2; *pc = 1; break;
    default: *pr = nranks; *pc = 1; break;
  }
}

int mx_comm_init(mx_ctx* c, int rank, int nranks,
                 const char unique_id[MX_UNIQUE_ID_BYTES]) {
  if (!c || rank < 0 || nranks <= 0 || rank >= nranks) return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  RCCL_OK(ncclCommInitRank(&c->world, nranks, id, rank));
  c->rank = rank;
  c->nranks = nranks;
  grid_shape(nranks, &c->pr, &c->pc);
  c->prow = rank / c->pc;
  c->pcol = rank % c->pc;
  if (nranks > 1) {
    RCCL_OK(ncclCommSplit(c->world, c->prow, c->pcol, &c->rowc, nullptr));
    RCCL_OK(ncclCommSplit(c->world, c->pcol, c->prow, &c->colc, nullptr));
  } else {
    c->rowc = c->world;
    c->colc = c->world;
  }
  c->have_comm = true;
  return MX_OK;
}

// Device facts for peak computation (confirm the fp64 MFMA
// peak from CU count x clock on the actual box, not just the 78.6 spec).
int mx_device_info(mx_ctx* c, int* cus, int* clock_khz) {
  if (!c) return MX_EINVAL;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, c->device));
  if (cus) *cus = prop.multiProcessorCount;
  if (clock_khz) *clock_khz = prop.clockRate;
  return MX_OK;
}

int mx_grid(mx_ctx* c, int* pr, int* pc, int* prow, int* pcol) {
  if (!c) return MX_EINVAL;
  if (pr) *pr = c->pr;
  if (pc) *pc = c->pc;
  if (prow) *prow = c->prow;
  if (pcol) *pcol = c->pcol;
  return MX_OK;
}

// ---------------------------------------------------------------------------
// device buffer helpers
int mx_alloc(mx_ctx* c, int64_t bytes, mx_dbuf** out) {
  if (!c || !out || bytes <= 0) return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  mx_dbuf* b = new mx_dbuf();
  int rc = ensure(c, b, bytes);
  if (rc != MX_OK) { delete b; return rc; }
  *out = b;
  return MX_OK;
}
int mx_free(mx_ctx* c, mx_dbuf* b) {
  if (!c || !b) return MX_EINVAL;
  if (b->ptr) (void)hipFree(b->ptr);
  delete b;
  return MX_OK;
}
int mx_upload(mx_ctx* c, mx_dbuf* dst, const void* src, int64_t bytes) {
  if (!c || !dst || !src || !mx_aux_bytes_ok(dst, bytes)) return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpy(dst->ptr, src, (size_t)bytes, hipMemcpyHostToDevice));
  return MX_OK;
}
int mx_download(mx_ctx* c, void* dst, const mx_dbuf* src, int64_t bytes) {
  if (!c || !dst || !src || !mx_aux_bytes_ok(src, bytes)) return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpy(dst, src->ptr, (size_t)bytes, hipMemcpyDeviceToHost));
  return MX_OK;
}
int mx_fill_random(mx_ctx* c, mx_dbuf* buf, int64_t n_elems, uint64_t seed,
                   int is_fp32) {
  if (!c || !buf || !mx_aux_fill_ok(buf, is_fp32, n_elems)) return MX_EINVAL;
  if (n_elems == 0) return MX_OK;
  HIP_OK(hipSetDevice(c->device));
  int rc = mxk_fill_random(is_fp32, buf->ptr, n_elems, 1, n_elems, seed,
                           c->s_gemm);
  if (rc) return rc;
  HIP_OK(hipStreamSynchronize(c->s_gemm));
  return MX_OK;
}

// Zero the pad region of an m x n logical image inside a rows_total x
// cols_total padded buffer (pitch ld) — restores the zero-pad invariant
// after a whole-buffer fill.
int mx_zero_pad(mx_ctx* c, mx_dbuf* buf, int64_t rows_total,
                int64_t cols_total, int64_t ld, int64_t m, int64_t n,
                int is_fp32) {
  if (!c || !buf ||
      !mx_aux_zero_pad_ok(buf, is_fp32, rows_total, cols_total, ld, m, n))
    return MX_EINVAL;
  if (rows_total == 0 || cols_total == 0) return MX_OK;   // empty image
  HIP_OK(hipSetDevice(c->device));
  if (mxk_zero_pad(is_fp32, buf->ptr, rows_total, cols_total, ld, m, n,
                   c->s_gemm))
    return MX_EHIP;
  HIP_OK(hipStreamSynchronize(c->s_gemm));
  return MX_OK;
}

// Download starting at a byte offset into the device buffer (e.g. one
// column of a padded col-major image: offset = j * pitch * elem).
int mx_download_off(mx_ctx* c, void* dst, const mx_dbuf* src,
                    int64_t off_bytes, int64_t bytes) {
  if (!c || !dst || !src || off_bytes < 0 || bytes <= 0 ||
      off_bytes + bytes > src->bytes)
    return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpy(dst, (const char*)src->ptr + off_bytes, (size_t)bytes,
                   hipMemcpyDeviceToHost));
  return MX_OK;
}

// 2D pitched download starting at a byte offset (e.g. one ROW of a
// col-major image: offset = i * elem, m = 1, n = cols, pitch = ld).
int mx_download2d_off(mx_ctx* c, void* dst, const mx_dbuf* src,
                      int64_t off_bytes, int64_t pitch_elems, int64_t m,
                      int64_t n, int elem) {
  if (!c || !dst || !src ||
      !mx_aux_copy2d_ok(src, elem, off_bytes, pitch_elems, m, n))
    return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpy2D(dst, (size_t)(m * elem),
                     (const char*)src->ptr + off_bytes,
                     (size_t)(pitch_elems * elem), (size_t)(m * elem),
                     (size_t)n, hipMemcpyDeviceToHost));
  return MX_OK;
}

// ---------------------------------------------------------------------------
// A GEMM launcher's code (kernels.h) as a code of the ABI.
static inline int launch_status(int rc) {
  return rc == 0 ? MX_OK : rc == -4 ? MX_EINVAL : MX_EHIP;
}

// enqueue() puts work on s_gemm and returns a launcher's code; the event
// pair around it is waited for and its time added to the stats. Counting
// the launches is the caller's.
template <class Enqueue>
static int timed(mx_ctx* c, Enqueue&& enqueue) {
  HIP_OK(hipEventRecord(c->ev[EV_TIMED_BEGIN], c->s_gemm));
  if (int rc = enqueue()) return launch_status(rc);
  HIP_OK(hipEventRecord(c->ev[EV_TIMED_END], c->s_gemm));
  HIP_OK(hipEventSynchronize(c->ev[EV_TIMED_END]));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, c->ev[EV_TIMED_BEGIN], c->ev[EV_TIMED_END]));
  c->st.gemm_ms += ms;
  return MX_OK;
}

// One timed launch.
template <class Enqueue>
static int timed_gemm(mx_ctx* c, Enqueue&& enqueue) {
  if (int rc = timed(c, enqueue)) return rc;
  c->st.gemm_launches += 1;
  return MX_OK;
}

// device-resident GEMM (padded pitches required)
static int gemm_device(mx_ctx* c, int is_fp32, int beta_one, int64_t m,
                       int64_t k, int64_t n, const void* dA, int64_t lda,
                       const void* dB, int64_t ldb, void* dC, int64_t ldc,
                       int trans_a = 0, int trans_b = 0) {
  if (m % 128 || n % 128 || k % 16) return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  return timed_gemm(c, [&] {
    return mxk_gemm_op(is_fp32, beta_one, trans_a, trans_b, m, n, k, dA, lda,
                       dB, ldb, dC, ldc, c->s_gemm);
  });
}

int mx_dgemm_device(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                    const mx_dbuf* dA, int64_t lda, const mx_dbuf* dB,
                    int64_t ldb, mx_dbuf* dC, int64_t ldc) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  c->st.bytes_moved = 8.0 * (m * k + k * n + m * n);
  return gemm_device(c, 0, 0, m, k, n, dA->ptr, lda, dB->ptr, ldb, dC->ptr,
                     ldc);
}
int mx_sgemm_device(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                    const mx_dbuf* dA, int64_t lda, const mx_dbuf* dB,
                    int64_t ldb, mx_dbuf* dC, int64_t ldc) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  c->st.bytes_moved = 4.0 * (m * k + k * n + m * n);
  return gemm_device(c, 1, 0, m, k, n, dA->ptr, lda, dB->ptr, ldb, dC->ptr,
                     ldc);
}

// 2D pitched transfers for device-resident matrices (the RDD.cache()
// analog: DenseVecMatrix.cache(), DenseVecMatrix.scala:321,505 usage).
int mx_upload2d(mx_ctx* c, mx_dbuf* dst, int64_t pitch_elems,
                const void* src, int64_t m, int64_t n, int elem) {
  if (!c || !dst || !src || !mx_aux_copy2d_ok(dst, elem, 0, pitch_elems, m, n))
    return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpy2D(dst->ptr, (size_t)(pitch_elems * elem), src,
                     (size_t)(m * elem), (size_t)(m * elem), (size_t)n,
                     hipMemcpyHostToDevice));
  return MX_OK;
}
int mx_download2d(mx_ctx* c, void* dst, const mx_dbuf* src,
                  int64_t pitch_elems, int64_t m, int64_t n, int elem) {
  if (!c || !dst || !src || !mx_aux_copy2d_ok(src, elem, 0, pitch_elems, m, n))
    return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpy2D(dst, (size_t)(m * elem), src->ptr,
                     (size_t)(pitch_elems * elem), (size_t)(m * elem),
                     (size_t)n, hipMemcpyDeviceToHost));
  return MX_OK;
}
int mx_memset(mx_ctx* c, mx_dbuf* b, int64_t bytes) {
  if (!c || !b || !mx_aux_bytes_ok(b, bytes)) return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemset(b->ptr, 0, (size_t)bytes));
  return MX_OK;
}
// device-resident transpose (operates on the full padded image; pads
// are zero so the transposed pads stay zero)
int mx_transpose_device(mx_ctx* c, int is_fp32, int64_t m, int64_t n,
                        const mx_dbuf* in, mx_dbuf* out) {
  if (!c || !in || !out || !mx_aux_transpose_ok(is_fp32, m, n, in, out))
    return MX_EINVAL;
  if (m == 0 || n == 0) return MX_OK;   // empty: a zero-block grid is an error
  HIP_OK(hipSetDevice(c->device));
  if (mxk_transpose(is_fp32, m, n, in->ptr, out->ptr, c->s_gemm))
    return MX_EHIP;
  HIP_OK(hipStreamSynchronize(c->s_gemm));
  return MX_OK;
}

// beta-capable device-resident GEMM (C += A*B when beta_one)
int mx_gemm_device_ex(mx_ctx* c, int is_fp32, int beta_one, int64_t m,
                      int64_t k, int64_t n, const mx_dbuf* dA, int64_t lda,
                      const mx_dbuf* dB, int64_t ldb, mx_dbuf* dC,
                      int64_t ldc) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  return gemm_device(c, is_fp32, beta_one, m, k, n, dA->ptr, lda, dB->ptr,
                     ldb, dC->ptr, ldc);
}

// C (+)= op(A)·op(B) on device-resident images
int mx_gemm_device_op(mx_ctx* c, int is_fp32, int beta_one, int trans_a,
                      int trans_b, int64_t m, int64_t k, int64_t n,
                      const mx_dbuf* dA, int64_t lda, const mx_dbuf* dB,
                      int64_t ldb, mx_dbuf* dC, int64_t ldc) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  return gemm_device(c, is_fp32, beta_one, m, k, n, dA->ptr, lda, dB->ptr,
                     ldb, dC->ptr, ldc, trans_a, trans_b);
}

// Many independent products in one launch (include/marlin_gpu.h). The
// plan (gemm_group_plan.h) validates the whole table first; only then is
// anything enqueued.
int mx_gemm_device_grouped(mx_ctx* c, int is_fp32, int beta_one, int trans_a,
                           int trans_b, int count,
                           const mx_gemm_problem_t* problems) {
  if (!c) return MX_EINVAL;
  const mx_gemm_knobs* knobs = mxk_gemm_knobs();
  mx_group_plan& plan = c->group_plan;
  int rc = mx_gemm_group_plan(is_fp32, beta_one, trans_a, trans_b,
                              knobs->band_width, knobs->plain_bands, count,
                              problems, &plan);
  c->st = {};
  if (rc) return rc;
  c->st.flops = plan.flops;
  if (plan.entries.empty() && plan.zeros.empty()) return MX_OK;
  HIP_OK(hipSetDevice(c->device));
  const size_t es = is_fp32 ? 4 : 8;
  for (const mx_group_zero& z : plan.zeros)
    HIP_OK(hipMemset2DAsync(z.C, (size_t)z.ldc * es, 0, (size_t)z.m * es,
                            (size_t)z.n, c->s_gemm));
  if (plan.entries.empty()) {
    HIP_OK(hipStreamSynchronize(c->s_gemm));
    return MX_OK;
  }
  if ((rc = ensure(c, &c->wsG, plan.table_bytes()))) return rc;
  return timed_gemm(c, [&] {
    return mxk_gemm_grouped(is_fp32, beta_one, trans_a, trans_b, &plan,
                            c->wsG.ptr, c->s_gemm);
  });
}

// One product with k cut into slices (include/marlin_gpu.h): the slices
// run as one grouped launch of beta-0 problems, slice 0 straight into C
// (when not accumulating) and the rest into tight slabs of wsK; the reduce
// kernel then folds the slabs into C in slice order on the same stream.
int mx_gemm_device_splitk(mx_ctx* c, int is_fp32, int beta_one, int trans_a,
                          int trans_b, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* dA, int64_t lda, const mx_dbuf* dB,
                          int64_t ldb, mx_dbuf* dC, int64_t ldc, int slices) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  c->st = {};
  if (slices < 0) return MX_EINVAL;
  // The whole product as a table of one: the pitch contract, every region
  // inside its buffer, C disjoint from A and B. The slices are sub-regions
  // of these, so what passes here passes slice by slice.
  const mx_gemm_knobs* knobs = mxk_gemm_knobs();
  mx_group_plan& plan = c->group_plan;
  const mx_gemm_problem_t whole = {m, k, n, dA, 0, lda, dB, 0, ldb,
                                   dC, 0, ldc};
  int rc = mx_gemm_group_plan(is_fp32, beta_one, trans_a, trans_b,
                              knobs->band_width, knobs->plain_bands, 1, &whole,
                              &plan);
  if (rc) return rc;
  c->st.flops = 2.0 * m * k * n;
  if (m == 0 || n == 0) {               // empty: nothing to do
    mxk_note_splitk(1, 0);
    return MX_OK;
  }
  HIP_OK(hipSetDevice(c->device));
  int S = slices;
  if (S == 0) {
    if (c->cus == 0)
      HIP_OK(hipDeviceGetAttribute(&c->cus,
                                   hipDeviceAttributeMultiprocessorCount,
                                   c->device));
    S = mx_splitk_auto(is_fp32, m, n, k, c->cus);
  }
  S = mx_splitk_slices(k, S, nullptr);
  if (S == 1) {                         // the plain entry's launch (k == 0 too)
    rc = gemm_device(c, is_fp32, beta_one, m, k, n, dA->ptr, lda, dB->ptr,
                     ldb, dC->ptr, ldc, trans_a, trans_b);
    if (rc == MX_OK) mxk_note_splitk(1, 0);
    return rc;
  }

  const int64_t elem = is_fp32 ? 4 : 8;
  const int64_t slab = m * n;           // fits: the C region fits its buffer
  const int nslabs = beta_one ? S : S - 1;
  if (nslabs > INT64_MAX / (slab * elem)) return MX_ENOMEM;
  const int64_t ws_bytes = nslabs * slab * elem;
  if ((rc = ensure(c, &c->wsK, ws_bytes))) return rc;
  c->splitk_slices.resize((size_t)S);
  mx_splitk_slices(k, S, c->splitk_slices.data());
  c->splitk_rows.clear();
  for (int s = 0; s < S; s++) {
    const int64_t k0 = c->splitk_slices[s].start * 16;
    mx_gemm_problem_t q = {m, c->splitk_slices[s].len * 16, n,
                           dA, trans_a ? k0 : k0 * lda, lda,
                           dB, trans_b ? k0 * ldb : k0, ldb,
                           dC, 0, ldc};
    if (beta_one || s > 0) {
      q.dC = &c->wsK;
      q.c_off = (beta_one ? s : s - 1) * slab;
      q.ldc = m;
    }
    c->splitk_rows.push_back(q);
  }
  rc = mx_gemm_group_plan(is_fp32, 0, trans_a, trans_b, knobs->band_width,
                          knobs->plain_bands, S, c->splitk_rows.data(), &plan);
  if (rc) return rc;
  if ((rc = ensure(c, &c->wsG, plan.table_bytes()))) return rc;
  rc = timed_gemm(c, [&] {
    if (int e = mxk_gemm_grouped(is_fp32, 0, trans_a, trans_b, &plan,
                                 c->wsG.ptr, c->s_gemm))
      return e;
    return mxk_splitk_reduce(is_fp32, m, n, dC->ptr, ldc, c->wsK.ptr, nslabs,
                             c->s_gemm);
  });
  if (rc == MX_OK) mxk_note_splitk(S, ws_bytes);   // only a split that ran
  return rc;
}

// Triangular solve on device images (include/marlin_gpu.h). The check and
// the step list are trsm_plan.h; only a call that passed the whole check
// allocates or enqueues. Every step is the diagonal kernel, then one
// accumulating GEMM into all remaining blocks, in stream order on s_gemm.
int mx_trsm_device(mx_ctx* c, int is_fp32, int side, int lower, int trans,
                   int unit_diag, int64_t n, int64_t r, const mx_dbuf* dT,
                   int64_t ldt, mx_dbuf* dB, int64_t ldb) {
  if (!c) return MX_EINVAL;
  c->st = {};
  bool empty = false;
  int rc = mx_trsm_check(128, is_fp32, side, lower, trans, unit_diag, n, r, dT,
                         ldt, dB, ldb, &empty);
  if (rc) return rc;
  c->st.flops = (double)n * (double)n * (double)r;
  if (empty) return MX_OK;
  mx_trsm_plan& plan = c->trsm_plan;
  mx_trsm_steps(128, side, lower, trans, n, r, ldt, ldb, &plan);
  const int64_t elem = is_fp32 ? 4 : 8;
  HIP_OK(hipSetDevice(c->device));
  if (plan.ws_elems > INT64_MAX / elem) return MX_ENOMEM;
  if ((rc = ensure(c, &c->wsT, plan.ws_elems * elem))) return rc;
  const char* tp = (const char*)dT->ptr;
  char* bp = (char*)dB->ptr;
  return timed(c, [&] {               // the whole sweep; a launch per GEMM step
    for (const mx_trsm_step& st : plan.steps) {
      int e = mxk_trsm_diag(is_fp32, side, plan.tt, plan.rev, unit_diag, st.nv,
                            tp + st.t_off * elem, ldt, bp + st.x_off * elem,
                            ldb, c->wsT.ptr, r, c->s_gemm);
      if (e) return e;
      if (st.rest_len == 0) continue;
      const void* A = side ? c->wsT.ptr : (const void*)(tp + st.a_off * elem);
      const void* B = side ? (const void*)(tp + st.b_off * elem) : c->wsT.ptr;
      e = mxk_gemm_op(is_fp32, 1, st.trans_a, st.trans_b, st.gm, st.gn, st.gk,
                      A, st.lda, B, st.ldb, bp + st.c_off * elem, st.ldc,
                      c->s_gemm);
      if (e) return e;
      c->st.gemm_launches += 1;
    }
    return 0;
  });
}

// LU factorisation of a device image (include/marlin_gpu.h). The check and
// the step list are getrf_plan.h; only a call that passed the whole check
// allocates or enqueues. Every step is a stream of launches on s_gemm: the
// diagonal kernel, the row permutation, the two strip solves (the triangular
// solve's diagonal kernel; T and B are disjoint blocks of the one image,
// which only the public TRSM entry refuses) and one accumulating GEMM.
int mx_getrf_device(mx_ctx* c, int is_fp32, int64_t n, mx_dbuf* dA,
                    int64_t lda, mx_dbuf* dPiv, int* info) {
  if (!c) return MX_EINVAL;
  c->st = {};
  bool empty = false;
  int rc = mx_getrf_check(128, is_fp32, n, dA, lda, dPiv, info, &empty);
  if (rc) return rc;
  *info = 0;
  c->st.flops = 2.0 * (double)n * (double)n * (double)n / 3.0;
  if (empty) return MX_OK;
  mx_getrf_plan& plan = c->getrf_plan;
  mx_getrf_steps(128, n, lda, &plan);
  const int64_t elem = is_fp32 ? 4 : 8;
  HIP_OK(hipSetDevice(c->device));
  if (plan.ws_elems > INT64_MAX / elem) return MX_ENOMEM;
  if (plan.ws_elems && (rc = ensure(c, &c->wsT, plan.ws_elems * elem)))
    return rc;
  if ((rc = ensure(c, &c->wsI, 4))) return rc;
  char* ap = (char*)dA->ptr;
  int* piv = (int*)dPiv->ptr;
  int* word = (int*)c->wsI.ptr;
  rc = timed(c, [&] {
    if (hipMemsetAsync(word, 0, 4, c->s_gemm) != hipSuccess) return -2;
    for (const mx_getrf_step& st : plan.steps) {
      int e = mxk_getrf_diag(is_fp32, st.nv, st.o, ap + st.d_off * elem, lda,
                             piv + st.o, word, c->s_gemm);
      if (e) return e;
      e = mxk_getrf_rowperm(is_fp32, st.o, plan.np, ap, lda, piv + st.o,
                            c->s_gemm);
      if (e) return e;
      if (st.rest == 0) continue;
      // L21 = A21 U11^-1: right, upper, non-unit  (tt = 1, rev = 0)
      e = mxk_trsm_diag(is_fp32, 1, 1, 0, 0, st.nv, ap + st.d_off * elem, lda,
                        ap + st.l21_off * elem, lda, c->wsT.ptr, st.rest,
                        c->s_gemm);
      if (e) return e;
      // U12 = L11^-1 (P A12): left, lower, unit  (tt = 0, rev = 0); last,
      // so that the panel holds -U12
      e = mxk_trsm_diag(is_fp32, 0, 0, 0, 1, st.nv, ap + st.d_off * elem, lda,
                        ap + st.u12_off * elem, lda, c->wsT.ptr, st.rest,
                        c->s_gemm);
      if (e) return e;
      e = mxk_gemm_op(is_fp32, 1, 0, 0, st.rest, st.rest, 128,
                      ap + st.l21_off * elem, lda, c->wsT.ptr, plan.ws_pitch,
                      ap + st.a22_off * elem, lda, c->s_gemm);
      if (e) return e;
      c->st.gemm_launches += 1;
    }
    return 0;
  });
  if (rc) return rc;
  HIP_OK(hipMemcpy(info, word, 4, hipMemcpyDeviceToHost));
  return MX_OK;
}

// The mx_last_gemm_* entries: views of the one record kernels.hip keeps.
static mxk_last_gemm_t last_gemm() {
  mxk_last_gemm_t r;
  mxk_last_gemm(&r);
  return r;
}

int mx_last_gemm_group(mx_ctx* c, int* problems_launched, int64_t* blocks) {
  if (!c || !problems_launched || !blocks) return MX_EINVAL;
  const mxk_last_gemm_t r = last_gemm();
  *problems_launched = r.group_problems;
  *blocks = r.group_blocks;
  return MX_OK;
}

int mx_last_gemm_splitk(mx_ctx* c, int* slices, int64_t* workspace_bytes) {
  if (!c || !slices || !workspace_bytes) return MX_EINVAL;
  const mxk_last_gemm_t r = last_gemm();
  *slices = r.splitk_slices;
  *workspace_bytes = r.splitk_ws_bytes;
  return MX_OK;
}

int mx_last_gemm_op(mx_ctx* c, int* trans_a, int* trans_b) {
  if (!c || !trans_a || !trans_b) return MX_EINVAL;
  const mxk_last_gemm_t r = last_gemm();
  *trans_a = r.trans_a;
  *trans_b = r.trans_b;
  return MX_OK;
}

int mx_last_gemm_config(mx_ctx* c, mx_gemm_cfg_t* out) {
  if (!c || !out) return MX_EINVAL;
  *out = last_gemm().cfg;
  return MX_OK;
}

int mx_last_gemm_loop(mx_ctx* c, int* out) {
  if (!c || !out) return MX_EINVAL;
  *out = last_gemm().loop;
  return MX_OK;
}

// ---------------------------------------------------------------------------
// host-buffer entries: validate, lay out, stage in, run, stage out. The
// images, their sizes and the copies are host_stage.h; this is its HIP
// backend, bound to a stream and a direction.
struct hip_stage {
  hipStream_t s;
  hipMemcpyKind kind;
  int zero(void* p, int64_t bytes) {
    HIP_OK(hipMemsetAsync(p, 0, (size_t)bytes, s));
    return MX_OK;
  }
  int copy2d(void* dst, int64_t dpitch, const void* src, int64_t spitch,
             int64_t width, int64_t cols) {
    HIP_OK(hipMemcpy2DAsync(dst, (size_t)dpitch, src, (size_t)spitch,
                            (size_t)width, (size_t)cols, kind, s));
    return MX_OK;
  }
  int copy(void* dst, const void* src, int64_t bytes) {
    HIP_OK(hipMemcpyAsync(dst, src, (size_t)bytes, kind, s));
    return MX_OK;
  }
};

// Size the image, grow the workspace to it and, given a host matrix, stage
// it in on stream s (without one: room only).
static int stage_ws(mx_ctx* c, mx_dbuf* ws, const mx_op_image& im,
                    int64_t elem, const void* host = nullptr,
                    hipStream_t s = nullptr) {
  int64_t bytes;
  if (!mx_image_bytes(im, elem, &bytes)) return MX_ENOMEM;
  if (int rc = ensure(c, ws, bytes)) return rc;
  hip_stage h2d = {s, hipMemcpyHostToDevice};
  return host ? mx_stage_in(h2d, ws->ptr, im, elem, host) : MX_OK;
}

// Device image -> host matrix on stream s, complete on return.
static int unstage(void* host, const void* dev, const mx_op_image& im,
                   int64_t elem, hipStream_t s) {
  hip_stage d2h = {s, hipMemcpyDeviceToHost};
  if (int rc = mx_stage_out(d2h, host, dev, im, elem)) return rc;
  HIP_OK(hipStreamSynchronize(s));
  return MX_OK;
}

// Whole multiplies. elem = 8 (fp64) or 4 (fp32).
// A is tight col-major m x k (k x m if trans_a), B k x n (n x k if
// trans_b): each is uploaded as stored into its zero-padded image
// (mx_gemm_op_layout), no transposed copy is made anywhere.
static int gemm_host(mx_ctx* c, int is_fp32, int beta_one, int64_t m,
                     int64_t k, int64_t n, const void* A, const void* B,
                     void* C, int transpose_c, const void* addC,
                     int trans_a = 0, int trans_b = 0) {
  if (!c || !A || !B || !C) return MX_EINVAL;
  if ((trans_a | trans_b) & ~1) return MX_EINVAL;
  if (m <= 0 || k <= 0 || n <= 0) return MX_EDIM;
  // the fused transpose(+add) epilogue is fp32, plain operands only
  if (transpose_c && (!is_fp32 || trans_a || trans_b)) return MX_EINVAL;
  if (!mx_op_can_round(m, k, n)) return MX_ENOMEM;
  const int64_t elem = is_fp32 ? 4 : 8;
  const int64_t mp = round_up(m, 128), np = round_up(n, 128),
                kp = round_up(k, 16);
  mx_op_image ia, ib, ic;
  mx_gemm_op_layout(trans_a, trans_b, m, k, n, &ia, &ib, &ic);
  const mx_op_image it = mx_epilogue_image(m, n, mp, np);  // add_c and C^T
  if (!mx_images_fit(elem, {ia, ib, ic, it})) return MX_ENOMEM;
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  c->st.bytes_moved = (double)elem * (m * k + k * n + m * n);

  HIP_OK(hipSetDevice(c->device));
  int rc;
  // room first: an allocation inside the timed window would count as h2d
  if ((rc = stage_ws(c, &c->wsA, ia, elem))) return rc;
  if ((rc = stage_ws(c, &c->wsB, ib, elem))) return rc;
  if ((rc = stage_ws(c, &c->wsC, ic, elem))) return rc;

  HIP_OK(hipEventRecord(c->ev[EV_H2D_BEGIN], c->s_copy));
  if ((rc = stage_ws(c, &c->wsA, ia, elem, A, c->s_copy))) return rc;
  if ((rc = stage_ws(c, &c->wsB, ib, elem, B, c->s_copy))) return rc;
  if (beta_one && (rc = stage_ws(c, &c->wsC, ic, elem, C, c->s_copy)))
    return rc;
  HIP_OK(hipEventRecord(c->ev[EV_H2D_END], c->s_copy));
  HIP_OK(hipStreamWaitEvent(c->s_gemm, c->ev[EV_H2D_END], 0));

  if (transpose_c) {
    // add_c is n x m on the host; the SUMMA panel buffer doubles as its
    // staging area (no SUMMA call is in flight during a host multiply)
    const float* dAdd = nullptr;
    if (addC) {
      if ((rc = stage_ws(c, &c->wsPA[0], it, elem, addC, c->s_gemm)))
        return rc;
      dAdd = (const float*)c->wsPA[0].ptr;
    }
    rc = timed_gemm(c, [&] {
      return mxk_sgemm_tn_epilogue(mp, np, kp, (const float*)c->wsA.ptr, mp,
                                   (const float*)c->wsB.ptr, kp,
                                   (float*)c->wsC.ptr, np, dAdd, c->s_gemm);
    });
    if (rc) return rc;
    if ((rc = unstage(C, c->wsC.ptr, it, elem, c->s_gemm))) return rc;
  } else {
    if ((rc = gemm_device(c, is_fp32, beta_one, mp, kp, np, c->wsA.ptr,
                          ia.pitch, c->wsB.ptr, ib.pitch, c->wsC.ptr,
                          ic.pitch, trans_a, trans_b)))
      return rc;
    HIP_OK(hipEventRecord(c->ev[EV_D2H], c->s_gemm));
    HIP_OK(hipStreamWaitEvent(c->s_copy, c->ev[EV_D2H], 0));
    if ((rc = unstage(C, c->wsC.ptr, ic, elem, c->s_copy))) return rc;
  }
  float h2d = 0;
  HIP_OK(hipEventElapsedTime(&h2d, c->ev[EV_H2D_BEGIN], c->ev[EV_H2D_END]));
  c->st.h2d_ms = h2d;
  c->st.total_ms = c->st.h2d_ms + c->st.gemm_ms;  // d2h folded into total sync
  return MX_OK;
}

int mx_dgemm(mx_ctx* c, int64_t m, int64_t k, int64_t n, const double* A,
             const double* B, double* C) {
  return gemm_host(c, 0, 0, m, k, n, A, B, C, 0, nullptr);
}
int mx_sgemm(mx_ctx* c, int64_t m, int64_t k, int64_t n, const float* A,
             const float* B, float* C) {
  return gemm_host(c, 1, 0, m, k, n, A, B, C, 0, nullptr);
}
int mx_gemm_op(mx_ctx* c, int is_fp32, int trans_a, int trans_b, int64_t m,
               int64_t k, int64_t n, const void* A, const void* B, void* C) {
  return gemm_host(c, is_fp32 ? 1 : 0, 0, m, k, n, A, B, C, 0, nullptr,
                   trans_a, trans_b);
}
int mx_sgemm_epilogue(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                      const float* A, const float* B, float* C,
                      int transpose_c, const float* add_c) {
  if (!transpose_c && add_c) return MX_EINVAL;  // plain add: use mx_sgemm+axpy later
  if (!transpose_c) return gemm_host(c, 1, 0, m, k, n, A, B, C, 0, nullptr);
  return gemm_host(c, 1, 0, m, k, n, A, B, C, 1, add_c);
}
int mx_tile_dgemm_acc(mx_ctx* c, int64_t tm, int64_t tk, int64_t tn,
                      const double* hA, const double* hB, double* hC,
                      int beta_one) {
  return gemm_host(c, 0, beta_one, tm, tk, tn, hA, hB, hC, 0, nullptr);
}

// ---------------------------------------------------------------------------
// SUMMA — the Spark-shuffle replacement (BlockMatrix.scala:161-186).
//
// Layout on the pr x pc grid (ceil slabs, reference blocking semantics):
//   A_local at rank (i,j): rows slab i of M  x  k-cols slab j of K
//   B_local at rank (i,j): k-rows slab i of K x  n-cols slab j of N
//   C_local at rank (i,j): rows slab i of M  x  n-cols slab j of N
// Per k-panel: the owning column broadcasts its A panel within each grid
// row; the owning row broadcasts its B panel within each grid column;
// every rank runs a local MFMA GEMM accumulate. One C owner per shard ->
// no reduce. Panels are packed (and k-padded to 16) on the comm stream,
// double-buffered against the GEMM stream.

struct panel_t {
  int64_t k0, k1;  // global k range
  int rootA;       // grid column owning the A panel (key in row comm)
  int rootB;       // grid row owning the B panel (key in col comm)
};

static std::vector<panel_t> plan_panels(int64_t K, int pr, int pc,
                                        int64_t kb_max) {
  std::vector<int64_t> cuts = {0, K};
  for (int j = 1; j < pc; j++) {
    int64_t o = mx_slab_off(K, pc, j);
    if (o < K) cuts.push_back(o);
  }
  for (int i = 1; i < pr; i++) {
    int64_t o = mx_slab_off(K, pr, i);
    if (o < K) cuts.push_back(o);
  }
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
  std::vector<panel_t> out;
  for (size_t s = 0; s + 1 < cuts.size(); s++) {
    for (int64_t k0 = cuts[s]; k0 < cuts[s + 1]; k0 += kb_max) {
      panel_t p;
      p.k0 = k0;
      p.k1 = std::min(k0 + kb_max, cuts[s + 1]);
      int64_t blA = (K + pc - 1) / pc;
      int64_t blB = (K + pr - 1) / pr;
      p.rootA = (int)(k0 / blA);
      p.rootB = (int)(k0 / blB);
      out.push_back(p);
    }
  }
  return out;
}

// C-visible for CPU tests (panel plan correctness without a GPU).
extern "C" int mx_plan_panels(int64_t K, int pr, int pc, int64_t kb_max,
                              int64_t* k0s, int64_t* k1s, int* rootsA,
                              int* rootsB, int cap) {
  auto v = plan_panels(K, pr, pc, kb_max);
  if ((int)v.size() > cap) return -(int)v.size();
  for (size_t i = 0; i < v.size(); i++) {
    k0s[i] = v[i].k0;
    k1s[i] = v[i].k1;
    rootsA[i] = v[i].rootA;
    rootsB[i] = v[i].rootB;
  }
  return (int)v.size();
}

// RAII pool for the per-panel timing events: destroyed on EVERY exit path
// (early error returns included), so failed SUMMA calls leak nothing.
struct ev_pool {
  std::vector<hipEvent_t> v;
  hipEvent_t mk() {
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    v.push_back(e);
    return e;
  }
  ~ev_pool() {
    for (hipEvent_t e : v)
      if (e) (void)hipEventDestroy(e);
  }
};

// panel width: overlap granularity of the comm/MFMA pipeline.
// Default 2048 (measured: the 1-rank panel-loop machinery runs at
// 98.9% of the monolithic GEMM rate at KB=2048 vs 97.2% at 4096 —
// profiles/r02_experiments.md; broadcasts still hide under the
// ~3 ms per-panel GEMM at 8 GPUs). MARLIN_SUMMA_KB overrides (latched
// on first use).
static int64_t default_summa_kb() {
  static const char* kbenv = getenv("MARLIN_SUMMA_KB");
  return kbenv && atoll(kbenv) > 0 ? atoll(kbenv) : 2048;
}

// One grid position of the panel loop. srcA[j] is A_local of (prow, j) and
// srcB[i] is B_local of (i, pcol) where this process holds that shard, or
// nullptr where it does not: a panel is packed here exactly when its root's
// shard is present. A real rank holds only its own shard (srcA[pcol],
// srcB[prow]) and receives the other panels through the broadcasts; the
// virtual entry holds every shard of its grid row and column and issues no
// broadcast, so the pack delivers what the broadcast would have.
struct summa_pos {
  int pr, pc, prow, pcol;
  const void* const* srcA;  // pc entries
  const void* const* srcB;  // pr entries
  bool bcast;               // ncclBroadcast each panel (real, nranks > 1)
};

// Pack one k-panel into this position's panel buffers (comm stream):
// k-padded to kbp, A pitch mip, B pitch kbp with all njp columns defined.
static int pack_panel(mx_ctx* c, const summa_pos& g, const panel_t& pan,
                      int64_t k, int64_t elem, int64_t mip, int64_t nj,
                      int64_t njp, void* pa, void* pb) {
  const int64_t kb = pan.k1 - pan.k0;
  const int64_t kbp = round_up(kb, 16);
  if (kbp != kb) {
    if (mip > 0)
      HIP_OK(hipMemsetAsync(pa, 0, (size_t)(mip * kbp * elem), c->s_comm));
    if (njp > 0)
      HIP_OK(hipMemsetAsync(pb, 0, (size_t)(kbp * njp * elem), c->s_comm));
  }
  const void* dA = g.srcA[pan.rootA];
  if (dA && mip > 0) {
    // A panel: k-cols [k0-ka_off, k1-ka_off) of the root's A_local (pitch
    // mip) are contiguous -> one copy into the packed panel (pitch mip)
    const int64_t ka_off = mx_slab_off(k, g.pc, pan.rootA);
    const char* src = (const char*)dA + (pan.k0 - ka_off) * mip * elem;
    HIP_OK(hipMemcpyAsync(pa, src, (size_t)(mip * kb * elem),
                          hipMemcpyDeviceToDevice, c->s_comm));
  }
  const void* dB = g.srcB[pan.rootB];
  if (dB && njp > 0) {
    // B panel: k-rows [k0-kb_off, k1-kb_off) of the root's B_local (pitch
    // kbi_p): strided 2D copy into packed pitch kbp
    const int64_t kb_off = mx_slab_off(k, g.pr, pan.rootB);
    const int64_t kbi_p = round_up(mx_slab_len(k, g.pr, pan.rootB), 16);
    const char* src = (const char*)dB + (pan.k0 - kb_off) * elem;
    if (nj > 0)
      HIP_OK(hipMemcpy2DAsync(pb, kbp * elem, src, kbi_p * elem, kb * elem,
                              nj, hipMemcpyDeviceToDevice, c->s_comm));
    // the copy defines nj columns only: an aligned panel skipped the
    // memset above, so columns nj..njp would keep whatever the workspace
    // held and reach C_local's pad columns
    if (kbp == kb && nj < njp)
      HIP_OK(hipMemsetAsync((char*)pb + kbp * nj * elem, 0,
                            (size_t)(kbp * (njp - nj) * elem), c->s_comm));
  }
  return MX_OK;
}

static int summa_loop(mx_ctx* c, int is_fp32, const summa_pos& g, int64_t m,
                      int64_t k, int64_t n, void* dC, int64_t kb_max) {
  const int64_t elem = is_fp32 ? 4 : 8;
  const ncclDataType_t nty = is_fp32 ? ncclFloat32 : ncclFloat64;
  const shard_t sh = local_shard(m, n, g.pr, g.pc, g.prow, g.pcol);
  const int64_t nj = sh.nj, mip = sh.mip, njp = sh.njp;
  // Empty local shard (e.g. m < pr on tiny inputs): the reference path
  // handles any size, so this rank must still take part in every panel
  // broadcast (counts are uniform per row/col comm: mip is shared by the
  // whole grid row, njp by the whole grid column) but launches no GEMM.
  const bool has_tile = mip > 0 && njp > 0;
  // local shard pitches ARE the padded sizes (bench fills them that way;
  // host entry packs them that way)
  auto panels = plan_panels(k, g.pr, g.pc, kb_max);

  c->st = {};
  c->st.flops = 2.0 * m * k * n;  // whole-job flops (rank-aggregate metric)
  c->st.bytes_moved = (double)elem * (m * k + k * n + m * n);
  if (!has_tile && !g.bcast) return MX_OK;  // nobody waits for this position

  HIP_OK(hipSetDevice(c->device));
  int rc;
  const int64_t kbp_max = round_up(kb_max, 16);
  for (int b = 0; b < 2; b++) {
    if (mip > 0 && (rc = ensure(c, &c->wsPA[b], mip * kbp_max * elem)))
      return rc;
    if (njp > 0 && (rc = ensure(c, &c->wsPB[b], kbp_max * njp * elem)))
      return rc;
  }

  HIP_OK(hipEventRecord(c->ev[EV_GEMM_DONE0], c->s_gemm));
  HIP_OK(hipEventRecord(c->ev[EV_GEMM_DONE1], c->s_gemm));

  // deferred per-panel timing: events recorded in-loop, synchronised
  // only AFTER both streams drain (an in-loop sync would serialise the
  // comm/GEMM double-buffer pipeline)
  ev_pool tev;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> gemm_tv, comm_tv;

  for (size_t p = 0; p < panels.size(); p++) {
    const panel_t& pan = panels[p];
    const int buf = (int)(p & 1);
    const int64_t kbp = round_up(pan.k1 - pan.k0, 16);
    void* pa = c->wsPA[buf].ptr;
    void* pb = c->wsPB[buf].ptr;

    // comm stream: wait until the GEMM that read this buffer 2 panels ago
    // is done, then pack (root) and broadcast.
    HIP_OK(hipStreamWaitEvent(c->s_comm, c->ev[EV_GEMM_DONE0 + buf], 0));
    if ((rc = pack_panel(c, g, pan, k, elem, mip, nj, njp, pa, pb)))
      return rc;
    if (g.bcast) {
      hipEvent_t c0 = tev.mk(), c1 = tev.mk();
      HIP_OK(hipEventRecord(c0, c->s_comm));
      RCCL_OK(ncclGroupStart());
      RCCL_OK(ncclBroadcast(pa, pa, (size_t)(mip * kbp), nty, pan.rootA,
                            c->rowc, c->s_comm));
      RCCL_OK(ncclBroadcast(pb, pb, (size_t)(kbp * njp), nty, pan.rootB,
                            c->colc, c->s_comm));
      RCCL_OK(ncclGroupEnd());
      HIP_OK(hipEventRecord(c1, c->s_comm));
      comm_tv.push_back({c0, c1});
    }
    HIP_OK(hipEventRecord(c->ev[EV_PANEL_READY0 + buf], c->s_comm));

    // gemm stream: wait for the panel, accumulate
    HIP_OK(hipStreamWaitEvent(c->s_gemm, c->ev[EV_PANEL_READY0 + buf], 0));
    if (has_tile) {
      int beta = p == 0 ? 0 : 1;
      hipEvent_t g0 = tev.mk(), g1 = tev.mk();
      HIP_OK(hipEventRecord(g0, c->s_gemm));
      rc = mxk_gemm(is_fp32, beta, mip, njp, kbp, pa, mip, pb, kbp, dC, mip,
                    c->s_gemm);
      if (rc) return launch_status(rc);
      c->st.gemm_launches += 1;
      HIP_OK(hipEventRecord(g1, c->s_gemm));
      gemm_tv.push_back({g0, g1});
    }
    HIP_OK(hipEventRecord(c->ev[EV_GEMM_DONE0 + buf], c->s_gemm));
  }
  HIP_OK(hipStreamSynchronize(c->s_gemm));
  HIP_OK(hipStreamSynchronize(c->s_comm));
  for (auto& pr2 : gemm_tv) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, pr2.first, pr2.second);
    c->st.gemm_ms += ms;
  }
  for (auto& pr2 : comm_tv) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, pr2.first, pr2.second);
    c->st.comm_ms += ms;
  }
  return MX_OK;
}

// real entries: geometry from the context, only this rank's shards present
static int summa_device(mx_ctx* c, int is_fp32, int64_t m, int64_t k,
                        int64_t n, const void* dA, const void* dB, void* dC) {
  if (!c->have_comm) return MX_ENOCOMM;
  std::vector<const void*> srcA(c->pc, nullptr), srcB(c->pr, nullptr);
  srcA[c->pcol] = dA;
  srcB[c->prow] = dB;
  // a rank always joins the broadcasts, an empty one included; on one rank
  // the loop still runs (and records its events) as it always has
  const summa_pos g = {c->pr, c->pc, c->prow, c->pcol, srcA.data(),
                       srcB.data(), c->nranks > 1};
  return summa_loop(c, is_fp32, g, m, k, n, dC, default_summa_kb());
}

// Virtual rank: the same loop at an arbitrary position of a pr x pc grid on
// one GPU, every panel packed from its root's shard instead of broadcast.
int mx_gemm_summa_virtual(mx_ctx* c, int is_fp32, int pr, int pc, int prow,
                          int pcol, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* const* dA_row,
                          const mx_dbuf* const* dB_col, mx_dbuf* dC_local,
                          int64_t kb_max) {
  if (!c || !dA_row || !dB_col || !dC_local) return MX_EINVAL;
  if (pr <= 0 || pc <= 0 || prow < 0 || prow >= pr || pcol < 0 || pcol >= pc)
    return MX_EINVAL;
  if (m <= 0 || k <= 0 || n <= 0 || kb_max < 0) return MX_EINVAL;
  // every non-empty shard of the grid row / column must be there
  const bool empty = mx_slab_len(m, pr, prow) == 0 ||
                     mx_slab_len(n, pc, pcol) == 0;
  std::vector<const void*> srcA(pc, nullptr), srcB(pr, nullptr);
  for (int j = 0; j < pc; j++) {
    if (dA_row[j]) srcA[j] = dA_row[j]->ptr;
    else if (!empty && mx_slab_len(k, pc, j) > 0) return MX_EINVAL;
  }
  for (int i = 0; i < pr; i++) {
    if (dB_col[i]) srcB[i] = dB_col[i]->ptr;
    else if (!empty && mx_slab_len(k, pr, i) > 0) return MX_EINVAL;
  }
  const summa_pos g = {pr, pc, prow, pcol, srcA.data(), srcB.data(), false};
  return summa_loop(c, is_fp32, g, m, k, n, dC_local->ptr,
                    kb_max > 0 ? kb_max : default_summa_kb());
}

// ---------------------------------------------------------------------------
// k-resident distributed layout (BASELINE config 4).
//
// CARMA splitMethod (MTUtils.scala:150-175) halves the LARGEST of m,k,n
// per step; for tall-skinny x short-fat shapes (50000x4096 · 4096x50000 on
// 8 GPUs) it never splits k -> kSplit == 1. The MI355X layout mirrors that
// choice: each rank keeps its A row-slab with ALL K columns and its B
// col-slab with ALL K rows resident in HBM (replicated across the other
// grid dimension), so the multiply is ONE local MFMA GEMM with ZERO
// steady-state xGMI traffic — no panel broadcasts at all.
static void split_method_c(int64_t m, int64_t k, int64_t n, int cores,
                           int* ms, int* ks, int* ns) {
  // exact MTUtils.scala:150-175 semantics (n tested first, then m, else k)
  *ms = *ks = *ns = 1;
  int64_t _m = m, _k = k, _n = n;
  int c = cores;
  while (c > 1 && _m > 1 && _k > 1 && _n > 1) {
    if (_n >= _k && _n >= _m) { *ns *= 2; _n /= 2; }
    else if (_m >= _k && _m >= _n) { *ms *= 2; _m /= 2; }
    else { *ks *= 2; _k /= 2; }
    c /= 2;
  }
}

int mx_summa_kresident(int64_t m, int64_t k, int64_t n, int nranks) {
  if (nranks <= 1) return 0;
  int ms, ks, ns;
  split_method_c(m, k, n, nranks, &ms, &ks, &ns);
  return ks == 1 ? 1 : 0;
}

static int summa_kres_device(mx_ctx* c, int is_fp32, int64_t m, int64_t k,
                             int64_t n, const void* dA, const void* dB,
                             void* dC) {
  if (!c->have_comm) return MX_ENOCOMM;
  const int64_t elem = is_fp32 ? 4 : 8;
  const shard_t s = local_shard(m, n, c->pr, c->pc, c->prow, c->pcol);
  const int64_t kp = round_up(k, 16);
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  c->st.bytes_moved = (double)elem * (m * k + k * n + m * n);
  if (s.mip == 0 || s.njp == 0) return MX_OK;  // empty shard: nothing to do
  HIP_OK(hipSetDevice(c->device));
  return timed_gemm(c, [&] {
    return mxk_gemm(is_fp32, 0, s.mip, s.njp, kp, dA, s.mip, dB, kp, dC,
                    s.mip, c->s_gemm);
  });
}

int mx_gemm_summa_kres_device(mx_ctx* c, int is_fp32, int64_t m, int64_t k,
                              int64_t n, const mx_dbuf* dA, const mx_dbuf* dB,
                              mx_dbuf* dC) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  return summa_kres_device(c, is_fp32, m, k, n, dA->ptr, dB->ptr, dC->ptr);
}

int mx_dgemm_summa_device(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* dA, const mx_dbuf* dB, mx_dbuf* dC) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  return summa_device(c, 0, m, k, n, dA->ptr, dB->ptr, dC->ptr);
}
int mx_sgemm_summa_device(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                          const mx_dbuf* dA, const mx_dbuf* dB, mx_dbuf* dC) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  return summa_device(c, 1, m, k, n, dA->ptr, dB->ptr, dC->ptr);
}

// host-buffer distributed entries on tight col-major shards: the panel loop
// (A_local mi x kaj, B_local kbi x nj) or, kres, the k-resident layout
// (A_local mi x K, B_local K x nj, one local GEMM).
static int summa_host(mx_ctx* c, int is_fp32, bool kres, int64_t m, int64_t k,
                      int64_t n, const void* A, const void* B, void* C) {
  if (!c || !A || !B || !C) return MX_EINVAL;
  if (!c->have_comm) return MX_ENOCOMM;
  if (!mx_op_can_round(m, k, n)) return MX_ENOMEM;
  const int64_t elem = is_fp32 ? 4 : 8;
  const auto [mi, nj, mip, njp] =
      local_shard(m, n, c->pr, c->pc, c->prow, c->pcol);
  mx_op_image ia, ib, ic;
  if (kres)
    mx_summa_kres_layout(mi, nj, mip, njp, k, round_up(k, 16), &ia, &ib, &ic);
  else
    mx_summa_host_layout(mi, nj, mip, njp, mx_slab_len(k, c->pc, c->pcol),
                         mx_slab_len(k, c->pr, c->prow), &ia, &ib, &ic);
  if (!mx_images_fit(elem, {ia, ib, ic})) return MX_ENOMEM;
  HIP_OK(hipSetDevice(c->device));
  int rc;
  // an empty k-resident shard stages nothing: the device entry sets the stats
  if (!(kres && ic.empty())) {
    if ((rc = stage_ws(c, &c->wsA, ia, elem, A, c->s_copy))) return rc;
    if ((rc = stage_ws(c, &c->wsB, ib, elem, B, c->s_copy))) return rc;
    if ((rc = stage_ws(c, &c->wsC, ic, elem))) return rc;
    // complete, not merely ordered: summa_loop packs panels on s_comm
    // straight out of wsA and wsB
    HIP_OK(hipStreamSynchronize(c->s_copy));
  }
  if ((rc = (kres ? summa_kres_device : summa_device)(
           c, is_fp32, m, k, n, c->wsA.ptr, c->wsB.ptr, c->wsC.ptr)))
    return rc;
  return unstage(C, c->wsC.ptr, ic, elem, c->s_copy);
}

int mx_dgemm_summa(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                   const double* A, const double* B, double* C) {
  return summa_host(c, 0, false, m, k, n, A, B, C);
}
int mx_sgemm_summa(mx_ctx* c, int64_t m, int64_t k, int64_t n, const float* A,
                   const float* B, float* C) {
  return summa_host(c, 1, false, m, k, n, A, B, C);
}
int mx_dgemm_summa_kres(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                        const double* A, const double* B, double* C) {
  return summa_host(c, 0, true, m, k, n, A, B, C);
}
int mx_sgemm_summa_kres(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                        const float* A, const float* B, float* C) {
  return summa_host(c, 1, true, m, k, n, A, B, C);
}

// ---------------------------------------------------------------------------
// Elementwise / reduction / transpose host entries (the BlockMatrix
// epilogue-op family, BlockMatrix.scala:344-523). Host col-major buffers;
// elementwise ops are layout-agnostic (flat n elements).
int mx_map(mx_ctx* c, int op, int is_fp32, int64_t n, const void* A,
           const void* B, double scalar, void* C) {
  if (!c || !A || !C || n <= 0 || !mx_aux_map_op_ok(op)) return MX_EINVAL;
  const int binary = mx_aux_map_binary(op);
  if (binary && !B) return MX_EINVAL;
  const int64_t elem = is_fp32 ? 4 : 8;
  mx_op_image im;
  if (!mx_flat_image(n, 1, &im) || !mx_images_fit(elem, {im})) return MX_ENOMEM;
  HIP_OK(hipSetDevice(c->device));
  int rc;
  if ((rc = stage_ws(c, &c->wsA, im, elem, A, c->s_gemm))) return rc;
  if (binary && (rc = stage_ws(c, &c->wsB, im, elem, B, c->s_gemm))) return rc;
  if ((rc = mxk_map(is_fp32, op, n, c->wsA.ptr, binary ? c->wsB.ptr : nullptr,
                    scalar, c->wsA.ptr, c->s_gemm)))
    return MX_EHIP;
  return unstage(C, c->wsA.ptr, im, elem, c->s_gemm);
}

// mx_map on device buffers: the same kernel, nothing crosses PCIe.
int mx_map_device(mx_ctx* c, int op, int is_fp32, int64_t n, const mx_dbuf* dA,
                  const mx_dbuf* dB, double scalar, mx_dbuf* dC) {
  if (!c || !dA || !dC || (is_fp32 & ~1) || !mx_aux_map_op_ok(op))
    return MX_EINVAL;
  const int binary = mx_aux_map_binary(op);
  if (binary && !dB) return MX_EINVAL;
  if (!mx_aux_fill_ok(dA, is_fp32, n) || !mx_aux_fill_ok(dC, is_fp32, n) ||
      (binary && !mx_aux_fill_ok(dB, is_fp32, n)))
    return MX_EINVAL;
  if (n == 0) return MX_OK;
  HIP_OK(hipSetDevice(c->device));
  if (mxk_map(is_fp32, op, n, dA->ptr, binary ? dB->ptr : nullptr, scalar,
              dC->ptr, c->s_gemm))
    return MX_EHIP;
  HIP_OK(hipStreamSynchronize(c->s_gemm));
  return MX_OK;
}

int mx_sum(mx_ctx* c, int is_fp32, int64_t n, const void* A, double* out) {
  if (!c || !A || !out || n <= 0) return MX_EINVAL;
  const int64_t elem = is_fp32 ? 4 : 8;
  mx_op_image im;
  if (!mx_flat_image(n, 1, &im) || !mx_images_fit(elem, {im})) return MX_ENOMEM;
  const mx_op_image parts_im = {1024 + 1, 1, 1024 + 1, 1}, one = {1, 1, 1, 1};
  HIP_OK(hipSetDevice(c->device));
  int rc;
  if ((rc = stage_ws(c, &c->wsA, im, elem, A, c->s_gemm))) return rc;
  if ((rc = stage_ws(c, &c->wsB, parts_im, 8))) return rc;
  double* parts = (double*)c->wsB.ptr;
  if ((rc = mxk_sum(is_fp32, n, c->wsA.ptr, parts, parts + 1024, c->s_gemm)))
    return MX_EHIP;
  return unstage(out, parts + 1024, one, 8, c->s_gemm);
}

int mx_transpose(mx_ctx* c, int is_fp32, int64_t m, int64_t n, const void* A,
                 void* C) {
  if (!c || !A || !C || m <= 0 || n <= 0) return MX_EINVAL;
  const int64_t elem = is_fp32 ? 4 : 8;
  mx_op_image im;
  if (!mx_flat_image(m, n, &im) || !mx_images_fit(elem, {im})) return MX_ENOMEM;
  HIP_OK(hipSetDevice(c->device));
  int rc;
  if ((rc = stage_ws(c, &c->wsA, im, elem, A, c->s_gemm))) return rc;
  if ((rc = stage_ws(c, &c->wsB, im, elem))) return rc;
  if ((rc = mxk_transpose(is_fp32, m, n, c->wsA.ptr, c->wsB.ptr, c->s_gemm)))
    return MX_EHIP;
  return unstage(C, c->wsB.ptr, im, elem, c->s_gemm);
}

// Matrix-vector multiply (BlockMatrix.scala:240-274): y = A x.
int mx_dgemv(mx_ctx* c, int64_t m, int64_t n, const double* A,
             const double* x, double* y) {
  if (!c || !A || !x || !y || m <= 0 || n <= 0) return MX_EINVAL;
  mx_op_image ia;
  if (!mx_flat_image(m, n, &ia) || !mx_images_fit(8, {ia})) return MX_ENOMEM;
  // wsB holds x then y (m * n fits, so n + m does); wsC 32 chunk partials
  const mx_op_image ix = {n, 1, n, 1}, iy = {m, 1, m, 1},
                    ixy = {n + m, 1, n + m, 1}, iparts = {m, 32, m, 32};
  if (!mx_images_fit(8, {ixy, iparts})) return MX_ENOMEM;
  HIP_OK(hipSetDevice(c->device));
  int rc;
  if ((rc = stage_ws(c, &c->wsA, ia, 8, A, c->s_gemm))) return rc;
  if ((rc = stage_ws(c, &c->wsB, ixy, 8))) return rc;
  if ((rc = stage_ws(c, &c->wsB, ix, 8, x, c->s_gemm))) return rc;
  if ((rc = stage_ws(c, &c->wsC, iparts, 8))) return rc;
  double* dy = (double*)c->wsB.ptr + n;
  if ((rc = mxk_gemv(0, m, n, m, c->wsA.ptr, c->wsB.ptr, (double*)c->wsC.ptr,
                     dy, c->s_gemm)))
    return MX_EHIP;
  return unstage(y, dy, iy, 8, c->s_gemm);
}

// Device-resident gemv on a cached matrix (x, y host vectors; the
// matrix never crosses PCIe). lda = the DeviceMatrix pitch.
int mx_dgemv_device(mx_ctx* c, int64_t m, int64_t n, const mx_dbuf* dA,
                    int64_t lda, const double* x, double* y) {
  if (!c || !dA || !x || !y || !mx_aux_gemv_ok(dA, m, n, lda))
    return MX_EINVAL;
  HIP_OK(hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, &c->wsB, (n + m + 32 * m) * 8))) return rc;
  double* dx = (double*)c->wsB.ptr;
  double* dy = dx + n;
  double* parts = dy + m;
  HIP_OK(hipMemcpyAsync(dx, x, n * 8, hipMemcpyHostToDevice, c->s_gemm));
  if ((rc = mxk_gemv(0, m, n, lda, dA->ptr, dx, parts, dy, c->s_gemm)))
    return MX_EHIP;
  HIP_OK(hipMemcpyAsync(y, dy, m * 8, hipMemcpyDeviceToHost, c->s_gemm));
  HIP_OK(hipStreamSynchronize(c->s_gemm));
  return MX_OK;
}

int mx_stats(mx_ctx* c, mx_stats_t* out) {
  if (!c || !out) return MX_EINVAL;
  *out = c->st;
  return MX_OK;
}

// Device-resident fused-epilogue GEMM (BASELINE config 5 timed leg):
// C[n x m] = (A*B)^T (+ addC), all buffers already in HBM, padded dims
// (m,n mult of 128, k of 16). ldc is the padded n pitch of C/addC.
int mx_sgemm_epilogue_device(mx_ctx* c, int64_t m, int64_t k, int64_t n,
                             const mx_dbuf* dA, int64_t lda,
                             const mx_dbuf* dB, int64_t ldb, mx_dbuf* dC,
                             int64_t ldc, const mx_dbuf* dAdd) {
  if (!c || !dA || !dB || !dC) return MX_EINVAL;
  if (m % 128 || n % 128 || k % 16) return MX_EINVAL;
  c->st = {};
  c->st.flops = 2.0 * m * k * n;
  c->st.bytes_moved = 4.0 * (m * k + k * n + m * n + (dAdd ? m * n : 0));
  HIP_OK(hipSetDevice(c->device));
  return timed_gemm(c, [&] {
    return mxk_sgemm_tn_epilogue(
        m, n, k, (const float*)dA->ptr, lda, (const float*)dB->ptr, ldb,
        (float*)dC->ptr, ldc, dAdd ? (const float*)dAdd->ptr : nullptr,
        c->s_gemm);
  });
}

// Failure-injection probe (RCCL error codes surfaced through
// the ABI, never aborts): issues an INVALID collective (null buffer) on
// the world communicator and returns the surfaced error. A healthy
// engine returns MX_ERCCL here and keeps working afterwards.
int mx_test_rccl_error(mx_ctx* c) {
  if (!c) return MX_EINVAL;
  if (!c->have_comm) return MX_ENOCOMM;
  HIP_OK(hipSetDevice(c->device));
  // out-of-range root: validated for ANY comm size (a null-buffer
  // broadcast is short-circuited on a size-1 comm and never checked)
  ncclResult_t e = ncclBroadcast(nullptr, nullptr, 16, ncclFloat64,
                                 c->nranks + 7, c->world, c->s_comm);
  if (e != ncclSuccess) return MX_ERCCL;  // expected: invalid argument
  HIP_OK(hipStreamSynchronize(c->s_comm));
  return MX_OK;
}
