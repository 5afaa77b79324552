// aux_guards.h — host-only integer code of the auxiliary entries: the
// argument checks of mx_fill_random, mx_zero_pad, mx_transpose_device,
// mx_dgemv_device, mx_upload2d / mx_download2d / mx_download2d_off,
// mx_download / mx_memset and mx_map. No HIP here, so a plain CPU program
// can check it (tests/test_aux_guards.py builds one under AddressSanitizer
// + UBSan).
//
// Each entry calls its check before hipSetDevice or any enqueue: a refused
// call returns MX_EINVAL and has touched no buffer. include/marlin_gpu.h
// states the contract for callers. Every extent test is the division form
// of mx_group_fits (gemm_group_plan.h): no product of two caller-chosen
// values is formed before it is known to fit.
#ifndef MARLIN_AUX_GUARDS_H
#define MARLIN_AUX_GUARDS_H

#include <stdint.h>

#include "gemm_group_plan.h"   // struct mx_dbuf, mx_group_fits

// rows x cols elements at pitch ld, starting off_bytes into the buffer.
// ld, rows, cols already non-negative.
static inline bool mx_aux_fits(const mx_dbuf* buf, int64_t elem,
                               int64_t off_bytes, int64_t ld, int64_t rows,
                               int64_t cols) {
  if (off_bytes < 0 || buf->bytes < 0 || off_bytes > buf->bytes) return false;
  const mx_dbuf rest = {buf->ptr, buf->bytes - off_bytes};
  return mx_group_fits(&rest, elem, 0, ld, rows, cols);
}

// mx_fill_random: n_elems >= 0 and n_elems * elem <= bytes (0 = no-op).
static inline bool mx_aux_fill_ok(const mx_dbuf* buf, int is_fp32,
                                  int64_t n_elems) {
  if (n_elems < 0) return false;
  return mx_aux_fits(buf, is_fp32 ? 4 : 8, 0, 1, 1, n_elems);
}

// mx_zero_pad: 0 <= m <= rows_total <= ld, 0 <= n <= cols_total, and the
// rows_total x cols_total image at pitch ld fits (an empty image: no-op).
static inline bool mx_aux_zero_pad_ok(const mx_dbuf* buf, int is_fp32,
                                      int64_t rows_total, int64_t cols_total,
                                      int64_t ld, int64_t m, int64_t n) {
  if (m < 0 || m > rows_total || rows_total > ld) return false;
  if (n < 0 || n > cols_total) return false;
  return mx_aux_fits(buf, is_fp32 ? 4 : 8, 0, ld, rows_total, cols_total);
}

// mx_transpose_device: m, n >= 0 (either zero: no-op), the tight m x n
// image fits both buffers, and in is not out, in handle or in pointer.
static inline bool mx_aux_transpose_ok(int is_fp32, int64_t m, int64_t n,
                                       const mx_dbuf* in, const mx_dbuf* out) {
  if (m < 0 || n < 0) return false;
  if (in == out || (in->ptr && in->ptr == out->ptr)) return false;
  const int64_t elem = is_fp32 ? 4 : 8;
  return mx_aux_fits(in, elem, 0, m, m, n) &&
         mx_aux_fits(out, elem, 0, n, n, m);
}

// mx_dgemv_device (fp64): m, n >= 1, lda >= m, and the (n-1)*lda + m
// elements of the image fit dA.
static inline bool mx_aux_gemv_ok(const mx_dbuf* dA, int64_t m, int64_t n,
                                  int64_t lda) {
  if (m <= 0 || n <= 0 || lda < m) return false;
  return mx_aux_fits(dA, 8, 0, lda, m, n);
}

// The device side of a pitched copy (mx_upload2d, mx_download2d,
// mx_download2d_off): elem in {4, 8}, m, n >= 1, pitch_elems >= m, and
// the region, byte offset included, fits the buffer.
static inline bool mx_aux_copy2d_ok(const mx_dbuf* buf, int elem,
                                    int64_t off_bytes, int64_t pitch_elems,
                                    int64_t m, int64_t n) {
  if (elem != 4 && elem != 8) return false;
  if (m <= 0 || n <= 0 || pitch_elems < m) return false;
  return mx_aux_fits(buf, elem, off_bytes, pitch_elems, m, n);
}

// mx_download, mx_memset: 0 <= bytes <= the buffer's size.
static inline bool mx_aux_bytes_ok(const mx_dbuf* buf, int64_t bytes) {
  return bytes >= 0 && bytes <= buf->bytes;
}

// mx_map: a code of the MX_OP_* list; the first three read a second array.
static inline bool mx_aux_map_op_ok(int op) {
  return op >= MX_OP_ADD && op <= MX_OP_RDIVS;
}
static inline bool mx_aux_map_binary(int op) {
  return op >= MX_OP_ADD && op <= MX_OP_EMUL;
}

#endif  // MARLIN_AUX_GUARDS_H
