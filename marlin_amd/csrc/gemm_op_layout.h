// gemm_op_layout.h — host-only arithmetic of the host-buffer multiply
// entries (mx_dgemm / mx_sgemm / mx_gemm_op): the padded device image of
// each operand of C = op(A)·op(B). No HIP here, so a plain CPU program
// can check it (tests/test_gemm_op_layout.py builds one under
// AddressSanitizer).
#ifndef MARLIN_GEMM_OP_LAYOUT_H
#define MARLIN_GEMM_OP_LAYOUT_H

#include <stdint.h>

// A tight col-major host matrix rows x cols and its device image: pitch
// >= rows, cap_cols >= cols columns allocated; everything outside
// rows x cols is zero padding.
struct mx_op_image {
  int64_t rows, cols;      // stored (host) shape
  int64_t pitch, cap_cols; // device image: pitch x cap_cols elements
  int64_t elems() const { return pitch * cap_cols; }
  bool padded() const { return rows != pitch || cols != cap_cols; }
};

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

#endif  // MARLIN_GEMM_OP_LAYOUT_H
