// host_stage.h — host-only statement of how every host-buffer entry
// (mx_dgemm / mx_sgemm / mx_gemm_op / mx_tile_dgemm_acc / mx_sgemm_epilogue,
// mx_[ds]gemm_summa, mx_[ds]gemm_summa_kres, mx_map, mx_sum, mx_transpose,
// mx_dgemv) stages its operands: the device image of each tight host
// matrix, the image's byte size with a verdict, and the copies in and out.
// No HIP here: the copies are written over a small backend type, so a plain
// CPU program runs this very code on heap blocks (tests/test_host_stage.py
// builds one under AddressSanitizer + UBSan).
#ifndef MARLIN_HOST_STAGE_H
#define MARLIN_HOST_STAGE_H

#include <stdint.h>

#include <initializer_list>

// A tight col-major host matrix rows x cols and its device image: pitch
// >= rows, cap_cols >= cols columns allocated; everything outside
// rows x cols is zero padding.
struct mx_op_image {
  int64_t rows, cols;      // stored (host) shape
  int64_t pitch, cap_cols; // device image: pitch x cap_cols elements
  int64_t elems() const { return pitch * cap_cols; }
  bool padded() const { return rows != pitch || cols != cap_cols; }
  bool empty() const { return rows == 0 || cols == 0; }
};

// x rounds up to the 128 tile (and so to the 16 k-step) inside int64_t.
static inline bool mx_op_can_round(int64_t x) { return x <= INT64_MAX - 128; }
static inline bool mx_op_can_round(int64_t m, int64_t k, int64_t n) {
  return mx_op_can_round(m) && mx_op_can_round(k) && mx_op_can_round(n);
}
static inline int64_t mx_op_round_up(int64_t x, int64_t a) {
  return (x + a - 1) / a * a;
}

// m, n pad to the 128 tile and k to the 16 k-step wherever they appear:
//   A   m x k  -> pitch mp, kp columns;   A^T  k x m -> pitch kp, mp columns
//   B   k x n  -> pitch kp, np columns;   B^T  n x k -> pitch np, kp columns
//   C   m x n  -> pitch mp, np columns
// The pitch of a transposed image is the pitch the kernel reads k-runs
// (A^T) resp. n-runs (B^T) with; both are multiples of 16 bytes.
static inline void mx_gemm_op_layout(int trans_a, int trans_b, int64_t m,
                                     int64_t k, int64_t n, mx_op_image* a,
                                     mx_op_image* b, mx_op_image* c) {
  const int64_t mp = mx_op_round_up(m, 128), np = mx_op_round_up(n, 128),
                kp = mx_op_round_up(k, 16);
  *a = trans_a ? mx_op_image{k, m, kp, mp} : mx_op_image{m, k, mp, kp};
  *b = trans_b ? mx_op_image{n, k, np, kp} : mx_op_image{k, n, kp, np};
  *c = mx_op_image{m, n, mp, np};
}

// The fused epilogue's add_c and its transposed output C^T: n x m at pitch
// np with mp columns (as many elements as the C image above).
static inline mx_op_image mx_epilogue_image(int64_t m, int64_t n, int64_t mp,
                                            int64_t np) {
  return {n, m, np, mp};
}

// One rank's shards of the panel-loop SUMMA (mi x nj of C, kaj k-columns of
// A, kbi k-rows of B; mip, njp the 128-padded shard). A and B keep their own
// column counts: pack_panel defines the pad columns of every panel itself.
static inline void mx_summa_host_layout(int64_t mi, int64_t nj, int64_t mip,
                                        int64_t njp, int64_t kaj, int64_t kbi,
                                        mx_op_image* a, mx_op_image* b,
                                        mx_op_image* c) {
  *a = {mi, kaj, mip, kaj};
  *b = {kbi, nj, mx_op_round_up(kbi, 16), nj};
  *c = {mi, nj, mip, njp};
}

// The k-resident shards: all of k on every rank, read by one GEMM, so both
// operands are padded in both directions (kp = k rounded to 16).
static inline void mx_summa_kres_layout(int64_t mi, int64_t nj, int64_t mip,
                                        int64_t njp, int64_t k, int64_t kp,
                                        mx_op_image* a, mx_op_image* b,
                                        mx_op_image* c) {
  *a = {mi, k, mip, kp};
  *b = {k, nj, kp, njp};
  *c = {mi, nj, mip, njp};
}

// The flat image of the elementwise entries: count runs of len elements
// back to back, as one column. False when len * count does not fit.
static inline bool mx_flat_image(int64_t len, int64_t count, mx_op_image* im) {
  if (len < 0 || count < 0) return false;
  if (len > 0 && count > INT64_MAX / len) return false;
  *im = {len * count, 1, len * count, 1};
  return true;
}

// bytes = pitch * cap_cols * elem in the division form of mx_group_fits
// (gemm_group_plan.h): no product is formed before it is known to fit.
// False when the size does not fit int64_t (or an extent is negative).
static inline bool mx_image_bytes(const mx_op_image& im, int64_t elem,
                                  int64_t* bytes) {
  if (im.pitch < 0 || im.cap_cols < 0) return false;
  *bytes = 0;
  if (im.pitch == 0 || im.cap_cols == 0) return true;
  if (im.pitch > INT64_MAX / elem / im.cap_cols) return false;
  *bytes = im.pitch * im.cap_cols * elem;
  return true;
}

// Every image of a call has a size: an entry checks this before it touches
// the device, and returns MX_ENOMEM where it does not hold.
static inline bool mx_images_fit(int64_t elem,
                                 std::initializer_list<mx_op_image> ims) {
  int64_t bytes;
  for (const mx_op_image& im : ims)
    if (!mx_image_bytes(im, elem, &bytes)) return false;
  return true;
}

// The copies, over a backend B with three operations, each returning 0 or
// an error code that is handed on:
//   zero(ptr, bytes)
//   copy2d(dst, dpitch, src, spitch, width, cols)   all but cols in bytes
//   copy(dst, src, bytes)
// One column moves with the linear copy, anything else with copy2d; an
// image without rows or columns (the empty SUMMA shard) is skipped.
template <class B>
static inline int mx_stage_copy(B& be, void* dst, int64_t dpitch,
                                const void* src, int64_t spitch,
                                const mx_op_image& im, int64_t elem) {
  if (im.cols == 1) return be.copy(dst, src, im.rows * elem);
  return be.copy2d(dst, dpitch * elem, src, spitch * elem, im.rows * elem,
                   im.cols);
}

// Host matrix -> device image. The workspaces are cached and shared by all
// entries, so the pad of an image holds whatever the previous call left
// there, and the kernels read the pad (stale * 0 is NaN for a stale NaN or
// Inf): a padded image is zeroed whole before the matrix goes in. An image
// without pad is defined in every byte by the copy alone.
template <class B>
static inline int mx_stage_in(B& be, void* dev, const mx_op_image& im,
                              int64_t elem, const void* host) {
  if (im.empty()) return 0;
  if (im.padded())
    if (int rc = be.zero(dev, im.elems() * elem)) return rc;
  return mx_stage_copy(be, dev, im.pitch, host, im.rows, im, elem);
}

// Device image -> host matrix: the logical rows x cols region only.
template <class B>
static inline int mx_stage_out(B& be, void* host, const void* dev,
                               const mx_op_image& im, int64_t elem) {
  if (im.empty()) return 0;
  return mx_stage_copy(be, host, im.rows, dev, im.pitch, im, elem);
}

#endif  // MARLIN_HOST_STAGE_H
