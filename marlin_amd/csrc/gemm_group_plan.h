// gemm_group_plan.h — host-only integer code of the grouped GEMM entry
// (mx_gemm_device_grouped): validation of the whole problem table and the
// device table the one launch reads. No HIP here, so a plain CPU program
// can check it (tests/test_gemm_group_plan.py builds one under
// AddressSanitizer).
//
// Contract checked here (include/marlin_gpu.h states it for callers):
//   per problem  m, n multiples of 128, k of 16, none negative; a problem
//                with m == 0 or n == 0 is empty and skipped unchecked;
//                otherwise no buffer is NULL, every pitch covers its
//                leading dimension and is a multiple of 16 bytes (the
//                trans_* meaning of lda / ldb as mx_gemm_device_op), every
//                offset is >= 0 and a multiple of 16 bytes, and every
//                region fits its buffer:
//                off + (cols - 1) * ld + rows <= bytes / elem;
//   per call     count >= 0, problems != NULL when count > 0, trans_* in
//                {0, 1}, at most 2^31 - 1 blocks in all;
//   aliasing     every C region is disjoint from every other problem's C
//                region and from every A and B region of the call. Two
//                regions of one buffer are disjoint when their byte spans
//                are, or when they share a pitch, neither wraps a column
//                (off % ld + rows <= ld) and they are disjoint rectangles
//                of that pitch's image. A and B regions may repeat and
//                overlap freely (they are only read).
#ifndef MARLIN_GEMM_GROUP_PLAN_H
#define MARLIN_GEMM_GROUP_PLAN_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/marlin_gpu.h"
#include "gemm_launch_policy.h"   // the pitch bound of the pipelined loop

// The device buffer behind the opaque handle of the C ABI; bytes is what
// lets the plan refuse a region that does not fit.
struct mx_dbuf {
  void* ptr = nullptr;
  int64_t bytes = 0;
};

// One launched problem as the kernel reads it: 64 bytes, every field
// block-uniform (the kernel keeps them in scalar registers).
struct mx_group_entry {
  const void* A;           // base pointers, offsets applied
  const void* B;
  void* C;
  int64_t lda, ldb, ldc;   // pitches in elements
  int32_t ntiles;          // k / 16
  int32_t nbm, nbn;        // m / 128, n / 128
  int32_t band;            // block_remap band: min(nbn, width), < 0 = plain
};
static_assert(sizeof(mx_group_entry) == 64, "device table entry layout");

// A C region to clear ahead of the launch (k == 0 without accumulate).
struct mx_group_zero {
  void* C;
  int64_t ldc, m, n;
};

// Device table = entries[launched] followed by tile_start[launched + 1]:
// block b belongs to the entry p with tile_start[p] <= b < tile_start[p+1]
// and is that problem's block b - tile_start[p].
struct mx_group_plan {
  std::vector<mx_group_entry> entries;
  std::vector<int32_t> tile_start;     // exclusive prefix sum, + the total
  std::vector<mx_group_zero> zeros;
  std::vector<int> order;              // entries[i] is problems[order[i]]
  double flops = 0;                    // sum of 2mkn over the whole table
  bool pitch32 = true;                 // every A/B pitch: mx_gemm_pitch32
  int64_t blocks() const { return tile_start.empty() ? 0 : tile_start.back(); }
  int64_t table_bytes() const {
    return (int64_t)(entries.size() * sizeof(mx_group_entry) +
                     tile_start.size() * sizeof(int32_t));
  }
};

// rows x cols elements at element offset off of buffer id, pitch ld
struct mx_group_region {
  const void* id;
  int64_t off, ld, rows, cols;
  bool empty() const { return rows == 0 || cols == 0; }
  int64_t span_end() const { return off + (cols - 1) * ld + rows; }
};

static inline bool mx_group_disjoint(const mx_group_region& a,
                                     const mx_group_region& b) {
  if (a.id != b.id || a.empty() || b.empty()) return true;
  if (a.span_end() <= b.off || b.span_end() <= a.off) return true;
  if (a.ld != b.ld) return false;
  const int64_t ar = a.off % a.ld, br = b.off % b.ld;
  if (ar + a.rows > a.ld || br + b.rows > b.ld) return false;
  const int64_t ac = a.off / a.ld, bc = b.off / b.ld;
  return ar + a.rows <= br || br + b.rows <= ar ||
         ac + a.cols <= bc || bc + b.cols <= ac;
}

// off, ld, rows, cols already non-negative. Division form: no product of
// two caller-chosen values is formed before it is known to fit.
static inline bool mx_group_fits(const mx_dbuf* buf, int64_t elem, int64_t off,
                                 int64_t ld, int64_t rows, int64_t cols) {
  if (rows == 0 || cols == 0) return true;
  const int64_t cap = buf->bytes / elem;
  if (off > cap || rows > cap - off) return false;
  return cols == 1 || ld <= (cap - off - rows) / (cols - 1);
}

// Validates the table and fills *out. band_width is the MARLIN_GEMM_BAND
// width (>= 1), plain_bands the MARLIN_GEMM_REMAP=bands choice. Returns
// MX_OK or MX_EINVAL; nothing is enqueued here, so a refused table has
// touched no buffer.
//
// Order: launched problems by descending k, stable. Blocks are dispatched
// in id order and a block's run time is proportional to its k, so the
// blocks that start last (the tail of the launch, when CUs begin to idle)
// are the short ones. Every C tile runs its own k-loop whatever its block
// id, so no result depends on the order.
static inline int mx_gemm_group_plan(int is_fp32, int beta_one, int trans_a,
                                     int trans_b, int band_width,
                                     int plain_bands, int count,
                                     const mx_gemm_problem_t* p,
                                     mx_group_plan* out) {
  *out = mx_group_plan();
  if (count < 0 || (count > 0 && !p)) return MX_EINVAL;
  if ((trans_a | trans_b) & ~1) return MX_EINVAL;
  if (band_width < 1) return MX_EINVAL;
  const int64_t elem = is_fp32 ? 4 : 8, e16 = 16 / elem;

  std::vector<mx_group_region> creg, abreg;
  std::vector<int> cowner;
  int64_t blocks = 0;
  for (int i = 0; i < count; i++) {
    const mx_gemm_problem_t& q = p[i];
    if (q.m < 0 || q.n < 0 || q.k < 0) return MX_EINVAL;
    if (q.m % 128 || q.n % 128 || q.k % 16) return MX_EINVAL;
    if (q.m == 0 || q.n == 0) continue;               // empty: skipped
    if (!q.dA || !q.dB || !q.dC) return MX_EINVAL;
    if (!q.dA->ptr || !q.dB->ptr || !q.dC->ptr) return MX_EINVAL;
    const int64_t ar = trans_a ? q.k : q.m, ac = trans_a ? q.m : q.k;
    const int64_t br = trans_b ? q.n : q.k, bc = trans_b ? q.k : q.n;
    if (q.lda < ar || q.ldb < br || q.ldc < q.m) return MX_EINVAL;
    if (q.lda % e16 || q.ldb % e16 || q.ldc % e16) return MX_EINVAL;
    if (q.a_off < 0 || q.b_off < 0 || q.c_off < 0) return MX_EINVAL;
    if (q.a_off % e16 || q.b_off % e16 || q.c_off % e16) return MX_EINVAL;
    if (!mx_group_fits(q.dA, elem, q.a_off, q.lda, ar, ac) ||
        !mx_group_fits(q.dB, elem, q.b_off, q.ldb, br, bc) ||
        !mx_group_fits(q.dC, elem, q.c_off, q.ldc, q.m, q.n))
      return MX_EINVAL;
    blocks += (q.m / 128) * (q.n / 128);
    if (q.m / 128 > INT32_MAX || q.n / 128 > INT32_MAX ||
        q.k / 16 > INT32_MAX || blocks > INT32_MAX)
      return MX_EINVAL;
    creg.push_back({q.dC, q.c_off, q.ldc, q.m, q.n});
    cowner.push_back(i);
    abreg.push_back({q.dA, q.a_off, q.lda, ar, ac});
    abreg.push_back({q.dB, q.b_off, q.ldb, br, bc});
  }
  for (size_t i = 0; i < creg.size(); i++) {
    for (size_t j = i + 1; j < creg.size(); j++)
      if (!mx_group_disjoint(creg[i], creg[j])) return MX_EINVAL;
    for (size_t j = 0; j < abreg.size(); j++)
      if (!mx_group_disjoint(creg[i], abreg[j])) return MX_EINVAL;
  }

  for (int i = 0; i < count; i++) {
    const mx_gemm_problem_t& q = p[i];
    out->flops += 2.0 * (double)q.m * (double)q.k * (double)q.n;
    if (q.m == 0 || q.n == 0) continue;
    char* cbase = (char*)q.dC->ptr + q.c_off * elem;
    if (q.k == 0) {                  // C = 0, or unchanged when accumulating
      if (!beta_one) out->zeros.push_back({cbase, q.ldc, q.m, q.n});
      continue;
    }
    out->order.push_back(i);
  }
  std::stable_sort(out->order.begin(), out->order.end(),
                   [&](int a, int b) { return p[a].k > p[b].k; });
  int64_t start = 0;
  for (int i : out->order) {
    const mx_gemm_problem_t& q = p[i];
    mx_group_entry e;
    e.A = (const char*)q.dA->ptr + q.a_off * elem;
    e.B = (const char*)q.dB->ptr + q.b_off * elem;
    e.C = (char*)q.dC->ptr + q.c_off * elem;
    e.lda = q.lda; e.ldb = q.ldb; e.ldc = q.ldc;
    e.ntiles = (int32_t)(q.k / 16);
    e.nbm = (int32_t)(q.m / 128);
    e.nbn = (int32_t)(q.n / 128);
    e.band = e.nbn < band_width ? e.nbn : band_width;
    if (plain_bands) e.band = -e.band;
    if (!mx_gemm_pitch32(q.lda, q.ldb)) out->pitch32 = false;
    out->entries.push_back(e);
    out->tile_start.push_back((int32_t)start);
    start += (int64_t)e.nbm * e.nbn;
  }
  out->tile_start.push_back((int32_t)start);
  return MX_OK;
}

#endif  // MARLIN_GEMM_GROUP_PLAN_H
