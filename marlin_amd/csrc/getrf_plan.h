// getrf_plan.h — host-only integer code of the device LU factorisation
// (mx_getrf_device): the argument check, the list of steps of the blocked
// right-looking sweep, and the one statement of how a diagonal block is
// eliminated. No HIP here, so a plain CPU program can check it
// (tests/test_getrf_plan.py builds one under AddressSanitizer + UBSan and
// runs the whole sweep at a small block width).
//
// The sweep (include/marlin_gpu.h states the contract for callers). The
// np x np image (np = n rounded up to w, w = 128 on the device) is cut into
// w x w blocks. Step j, block offset o = w * j, nv = min(w, n - o):
//   (1) the diagonal kernel factors block (j, j) in place with partial
//       pivoting among ITS OWN rows (mx_getrf_eliminate is the statement of
//       it) and writes the block's w permutation entries;
//   (2) the row-permutation kernel moves rows [o, o + w) of every other
//       column of the image the same way: columns [0, o), the finished L
//       part, and [o + w, np);
//   (3) L21 = A21 U11^-1: the triangular solve's diagonal kernel, right /
//       upper / non-unit, on the column strip below the block;
//   (4) U12 = L11^-1 (P A12): the same kernel, left / lower / unit, on the
//       row strip to the right; it runs last, so that the workspace panel
//       holds -U12 (w x rest at pitch w);
//   (5) A22 += L21 * (-U12): ONE accumulating GEMM of k = w.
// (3)-(5) exist only while blocks remain (rest > 0); only the last block
// can be ragged, and it has no rest.
//
// Pivoting never leaves the diagonal block, so a matrix whose diagonal
// block is singular or nearly so at its step, where a pivot from a lower
// block row would have served, is not handled any better than the host
// path handles it at base_size: a zero pivot is reported, a tiny one is
// divided by.
#ifndef MARLIN_GETRF_PLAN_H
#define MARLIN_GETRF_PLAN_H

#include <stdint.h>

#ifndef GETRF_FN
#include <math.h>

#include <vector>

#include "gemm_group_plan.h"   // struct mx_dbuf, mx_group_fits
#define GETRF_FN static inline
#define MX_GETRF_HOST 1
#endif

// ---------------------------------------------------------------------------
// The element operations of the in-block elimination (shared with the
// kernel, which includes this header with GETRF_FN set to its device
// qualifier and performs exactly these on each element, in this order).
//
// Pivot rule. The key of a candidate is |a|, or -1 for a NaN; the pivot of
// column j is the row of the largest key among the remaining rows, the
// LOWEST row index among equal keys. That is the scan "if |a| > best" down
// the column from row j with best = -1: a tie keeps the earlier row and a
// NaN never passes the test (it is taken only where every remaining entry
// is a NaN, when row j stays).
template <typename T>
GETRF_FN T mx_getrf_key(T a) { return a == a ? (a < T(0) ? -a : a) : T(-1); }

// (key, row) `b` replaces `a`: strictly larger key, or the same key at a
// lower row. Associative and commutative, so a tree reduction in any shape
// finds what the scan finds.
template <typename T>
GETRF_FN bool mx_getrf_better(T key_b, int row_b, T key_a, int row_a) {
  return key_b > key_a || (key_b == key_a && row_b < row_a);
}

// The multiplier l_i = a / pivot: one division, not a multiplication by a
// reciprocal.
template <typename T>
GETRF_FN T mx_getrf_scale(T a, T pivot) { return a / pivot; }

// The update a_ik -= l_i * u_k is ONE fused multiply-add, fma(-l_i, u_k,
// a_ik): a single rounding, in the kernel and on the host alike.
GETRF_FN double mx_getrf_update(double a, double l, double u) {
  return __builtin_fma(-l, u, a);
}
GETRF_FN float mx_getrf_update(float a, float l, float u) {
  return __builtin_fmaf(-l, u, a);
}

#ifdef MX_GETRF_HOST
// ---------------------------------------------------------------------------
// The in-block elimination: right-looking, columns and rows ascending.
// `block` is W x W column-major at `pitch`; only its leading nv x nv part is
// touched (the ragged block behaves as if continued by the identity, which
// pivots on itself and updates nothing). perm[g] (g < W) is the source row
// of output row g, inside the block, the identity at g >= nv. Whole rows of
// the block are swapped, the finished L columns included. *first_zero is the
// 1-based column of the first exactly-zero pivot, else 0; such a column is
// left unscaled and the elimination goes on, as LAPACK's does.
template <typename T>
static inline void mx_getrf_eliminate(int W, int nv, T* block, int64_t pitch,
                                      int* perm, int* first_zero) {
  for (int g = 0; g < W; g++) perm[g] = g;
  *first_zero = 0;
  for (int j = 0; j < nv; j++) {
    int p = j;
    T best = T(-1);
    for (int i = j; i < nv; i++) {
      const T key = mx_getrf_key(block[i + j * pitch]);
      if (key > best) { best = key; p = i; }
    }
    if (p != j) {
      for (int k = 0; k < nv; k++) {
        const T t = block[j + k * pitch];
        block[j + k * pitch] = block[p + k * pitch];
        block[p + k * pitch] = t;
      }
      const int t = perm[j]; perm[j] = perm[p]; perm[p] = t;
    }
    const T pivot = block[j + j * pitch];
    if (pivot == T(0)) {
      if (!*first_zero) *first_zero = j + 1;
    } else {
      for (int i = j + 1; i < nv; i++)
        block[i + j * pitch] = mx_getrf_scale(block[i + j * pitch], pivot);
    }
    for (int k = j + 1; k < nv; k++) {
      const T u = block[j + k * pitch];
      for (int i = j + 1; i < nv; i++)
        block[i + k * pitch] =
            mx_getrf_update(block[i + k * pitch], block[i + j * pitch], u);
    }
  }
}

// ---------------------------------------------------------------------------
struct mx_getrf_step {
  int64_t o;                  // first index of diagonal block j
  int nv;                     // min(w, n - o): the order left inside it
  int64_t d_off;              // the diagonal block's first element
  // the row permutation: rows [o, o + w) of columns [0, left_cols) and of
  // [right_col0, right_col0 + right_cols)
  int64_t left_cols, right_col0, right_cols;
  int64_t rest;               // np - o - w: what (3)-(5) work on; 0 = none
  int64_t l21_off;            // column strip below: rest x w   (step 3)
  int64_t u12_off;            // row strip to the right: w x rest (step 4)
  int64_t a22_off;            // trailing matrix: rest x rest   (step 5)
};

struct mx_getrf_plan {
  int64_t np = 0;             // n rounded up to w
  int64_t ws_elems = 0;       // w * (np - w): the -U12 panel of step 0
  int64_t ws_pitch = 0;       // w: its pitch as the GEMM's B operand
  std::vector<mx_getrf_step> steps;   // every pitch in the image is lda
};

// The argument check. Returns MX_OK or MX_EINVAL; *empty is set for n == 0,
// the no-op, for which pitch and buffers are not looked at (info still must
// not be NULL). w is the block width, 128 on the device.
static inline int mx_getrf_check(int64_t w, int is_fp32, int64_t n,
                                 const mx_dbuf* dA, int64_t lda,
                                 const mx_dbuf* dPiv, const int* info,
                                 bool* empty) {
  *empty = false;
  if (is_fp32 & ~1) return MX_EINVAL;
  if (w < 1 || n < 0 || !info) return MX_EINVAL;
  if (n == 0) { *empty = true; return MX_OK; }
  if (!dA || !dPiv || !dA->ptr || !dPiv->ptr) return MX_EINVAL;
  // the permutation entries are int32 row indices
  if (w > INT32_MAX || n > INT32_MAX - (w - 1)) return MX_EINVAL;
  const int64_t np = (n + (w - 1)) / w * w;
  const int64_t elem = is_fp32 ? 4 : 8, e16 = 16 / elem;
  if (lda < np || lda % e16) return MX_EINVAL;
  if (dA->bytes < 0 || dPiv->bytes < 0) return MX_EINVAL;
  if (!mx_group_fits(dA, elem, 0, lda, np, np) ||
      !mx_group_fits(dPiv, 4, 0, np, np, 1))
    return MX_EINVAL;
  // the image and the permutation are different buffers: not one handle,
  // no shared byte
  if (dA == dPiv) return MX_EINVAL;
  const uintptr_t a0 = (uintptr_t)dA->ptr, p0 = (uintptr_t)dPiv->ptr;
  const bool a_before = a0 <= p0 && (uint64_t)dA->bytes <= p0 - a0;
  const bool p_before = p0 <= a0 && (uint64_t)dPiv->bytes <= a0 - p0;
  if (!a_before && !p_before) return MX_EINVAL;
  return MX_OK;
}

// The step list of a call that passed mx_getrf_check (and is not empty).
// Every offset stays inside the image, which fits its buffer, so none of the
// products below can overflow.
static inline void mx_getrf_steps(int64_t w, int64_t n, int64_t lda,
                                  mx_getrf_plan* out) {
  *out = mx_getrf_plan();
  const int64_t np = (n + (w - 1)) / w * w;
  out->np = np;
  out->ws_elems = w * (np - w);
  out->ws_pitch = w;
  for (int64_t o = 0; o < np; o += w) {
    mx_getrf_step st = {};
    st.o = o;
    st.nv = (int)(n - o < w ? n - o : w);
    st.d_off = o + o * lda;
    st.left_cols = o;
    st.right_col0 = o + w;
    st.right_cols = np - o - w;
    st.rest = np - o - w;
    st.l21_off = (o + w) + o * lda;
    st.u12_off = o + (o + w) * lda;
    st.a22_off = (o + w) + (o + w) * lda;
    out->steps.push_back(st);
  }
}
#endif  // MX_GETRF_HOST

#endif  // MARLIN_GETRF_PLAN_H
