// trsm_plan.h — host-only integer code of the triangular solve entry
// (mx_trsm_device): the argument check, the list of steps of the blocked
// sweep, and the one statement of how a diagonal block is staged and of the
// element operations of its substitution. No HIP here, so a plain CPU
// program can check it (tests/test_trsm_plan.py builds one under
// AddressSanitizer + UBSan and runs the plan at a small block width against
// direct substitution; tests/test_diag_bits_cpu.py runs the substitution
// at the device's width on rounding data).
//
// The sweep (include/marlin_gpu.h states the contract for callers). T is
// cut into w x w blocks, w = 128 on the device. With eff_lower = lower XOR
// trans the left side sweeps forward when eff_lower, the right side when
// !eff_lower, otherwise backward. Step j
//   (a) solves diagonal block j against all r right-hand sides (the
//       diagonal kernel): X_j overwrites its strip of B, -X_j goes to the
//       workspace panel (left: w x r at pitch w, right: r x w at pitch r);
//   (b) updates every remaining block at once with ONE accumulating GEMM
//       of k = w:   left   B_rest += op(T)[rest, j] * (-X_j)
//                   right  B_rest += (-X_j) * op(T)[j, rest]
//       where op(T)'s block is read AS STORED through the GEMM's trans flag.
// Only blocks of the referenced triangle appear in (b), and inside a
// diagonal block mx_trsm_stage decides element by element what is loaded.
#ifndef MARLIN_TRSM_PLAN_H
#define MARLIN_TRSM_PLAN_H

#include <stdint.h>

#ifndef TRSM_FN
#include <vector>

#include "gemm_group_plan.h"   // struct mx_dbuf, mx_group_fits
#define TRSM_FN static inline
#define MX_TRSM_HOST 1
#endif

// ---------------------------------------------------------------------------
// Staging of a diagonal block (shared with the kernel, which includes this
// header with TRSM_FN set to its device qualifier).
//
// Whatever (side, lower, trans, unit_diag) is, the diagonal kernel runs ONE
// substitution: forward, on a lower-triangular w x w matrix L, one
// right-hand-side vector v per lane,  y_a = (v_a - sum_{b<a} L[a][b] y_b) /
// L[a][a].  The form is resolved when L is staged:
//   tt  = trans XOR side   M = op(T) on the left, op(T)^T on the right, so
//                          M[x][y] is T[y][x] when tt, else T[x][y];
//   rev = !(lower XOR tt)  M is upper: canonical index a is original index
//                          w - 1 - a, of L and of the right-hand side both.
// L[a][b] for a >= b is then: the identity where an original index is >= nv
// (the block is continued past the order of T), 1 on a unit diagonal, and
// otherwise the one element of T at the returned offset from the block's
// first element. Nothing else of T is loaded.
enum { MX_TRSM_ZERO = 0, MX_TRSM_ONE = 1, MX_TRSM_LOAD = 2 };

TRSM_FN int mx_trsm_orig(int w, int rev, int a) { return rev ? w - 1 - a : a; }

TRSM_FN int mx_trsm_stage(int w, int tt, int rev, int unit, int nv, int a,
                          int b, int64_t ldt, int64_t* off) {
  // written without early returns: the kernel wants selects, not branches,
  // around its staging loads
  const int oa = mx_trsm_orig(w, rev, a), ob = mx_trsm_orig(w, rev, b);
  const bool inside = a >= b && oa < nv && ob < nv;
  const bool load = inside && !(a == b && unit);
  if (load) *off = tt ? ob + oa * ldt : oa + ob * ldt;
  return load ? MX_TRSM_LOAD : a == b ? MX_TRSM_ONE : MX_TRSM_ZERO;
}

// ---------------------------------------------------------------------------
// The element operations of the substitution (shared with the kernel, which
// performs exactly these on each element, in ascending b).
//
// The update acc -= l * y is ONE fused multiply-add, fma(-l, y, acc): a
// single rounding, in the kernel and on the host alike. Written as
// acc - l * y it would be left to the compiler's contraction, which fuses
// some of a kernel's updates and splits others into a multiply and a
// subtract (two roundings), differently from one compiler to the next.
TRSM_FN double mx_trsm_update(double acc, double l, double y) {
  return __builtin_fma(-l, y, acc);
}
TRSM_FN float mx_trsm_update(float acc, float l, float y) {
  return __builtin_fmaf(-l, y, acc);
}

// The quotient y = acc / d: one division, not a multiplication by a
// reciprocal.
TRSM_FN double mx_trsm_quot(double acc, double d) { return acc / d; }
TRSM_FN float mx_trsm_quot(float acc, float d) { return acc / d; }

#ifdef MX_TRSM_HOST
// ---------------------------------------------------------------------------
// The substitution on one right-hand side, in place: L is the staged w x w
// lower-triangular matrix, L[a * w + b] its element (a, b); v holds the
// right-hand side in canonical order on entry and y on return. Element a
// takes its updates in ascending b and then its one division, which is what
// the kernel does to it (there the loop runs the other way round, column b
// into every later row, and an element sees the same sequence).
template <typename T>
static inline void mx_trsm_substitute(int w, const T* L, T* v) {
  for (int a = 0; a < w; a++) {
    T acc = v[a];
    for (int b = 0; b < a; b++) acc = mx_trsm_update(acc, L[a * w + b], v[b]);
    v[a] = mx_trsm_quot(acc, L[a * w + a]);
  }
}

// ---------------------------------------------------------------------------
struct mx_trsm_step {
  int64_t j0;                 // first index of diagonal block j
  int nv;                     // min(w, n - j0): the order left inside it
  int64_t t_off;              // its first element in T
  int64_t x_off;              // first element of the X_j strip in B
  int64_t rest0, rest_len;    // the remaining indices [rest0, rest0 + len)
  // the update GEMM, C += op(A) * op(B), dims as mxk_gemm_op takes them;
  // the workspace operand has offset 0
  int64_t gm, gk, gn;
  int trans_a, trans_b;
  int64_t a_off, lda;         // left: in T;         right: the workspace
  int64_t b_off, ldb;         // left: the workspace; right: in T
  int64_t c_off, ldc;         // in B
};

struct mx_trsm_plan {
  int tt = 0, rev = 0;        // staging flags of every diagonal block
  int64_t np = 0;             // n rounded up to w
  int64_t ws_elems = 0;       // w * r
  std::vector<mx_trsm_step> steps;
};

// The argument check. Returns MX_OK or MX_EINVAL; *empty is set when the
// call is the no-op (n == 0 or r == 0), for which pitches and buffers are
// not looked at. w is the block width (128 on the device), of which r must
// be a multiple.
static inline int mx_trsm_check(int64_t w, int is_fp32, int side, int lower,
                                int trans, int unit_diag, int64_t n,
                                int64_t r, const mx_dbuf* dT, int64_t ldt,
                                const mx_dbuf* dB, int64_t ldb, bool* empty) {
  *empty = false;
  if ((is_fp32 | side | lower | trans | unit_diag) & ~1) return MX_EINVAL;
  if (w < 1 || n < 0 || r < 0 || r % w) return MX_EINVAL;
  if (n == 0 || r == 0) { *empty = true; return MX_OK; }
  if (!dT || !dB || !dT->ptr || !dB->ptr) return MX_EINVAL;
  if (n > INT64_MAX - (w - 1)) return MX_EINVAL;
  const int64_t np = (n + (w - 1)) / w * w;
  const int64_t elem = is_fp32 ? 4 : 8, e16 = 16 / elem;
  const int64_t brows = side ? r : np, bcols = side ? np : r;
  if (ldt < np || ldb < brows || ldt % e16 || ldb % e16) return MX_EINVAL;
  if (!mx_group_fits(dT, elem, 0, ldt, np, np) ||
      !mx_group_fits(dB, elem, 0, ldb, brows, bcols))
    return MX_EINVAL;
  // one launch of the update GEMM covers at most (np / w) x (r / w) tiles,
  // one of the diagonal kernel two blocks per w right-hand sides
  if (np / w > INT32_MAX / (r / w) || r / w > INT32_MAX / 2) return MX_EINVAL;
  // T and B are different buffers: not one handle, no shared byte
  if (dT == dB) return MX_EINVAL;
  const uintptr_t t0 = (uintptr_t)dT->ptr, b0 = (uintptr_t)dB->ptr;
  if (dT->bytes < 0 || dB->bytes < 0) return MX_EINVAL;
  const bool t_before = t0 <= b0 && (uint64_t)dT->bytes <= b0 - t0;
  const bool b_before = b0 <= t0 && (uint64_t)dB->bytes <= t0 - b0;
  if (!t_before && !b_before) return MX_EINVAL;
  return MX_OK;
}

// The step list of a call that passed mx_trsm_check (and is not empty).
// Every offset stays inside its region, which fits its buffer, so none of
// the products below can overflow.
static inline void mx_trsm_steps(int64_t w, int side, int lower, int trans,
                                 int64_t n, int64_t r, int64_t ldt,
                                 int64_t ldb, mx_trsm_plan* out) {
  *out = mx_trsm_plan();
  const int tt = trans ^ side;
  const int eff_lower = lower ^ trans;
  const bool forward = side ? !eff_lower : eff_lower;
  const int64_t np = (n + (w - 1)) / w * w, nblk = np / w;
  out->tt = tt;
  out->rev = forward ? 0 : 1;            // == !(lower ^ tt)
  out->np = np;
  out->ws_elems = w * r;
  for (int64_t s = 0; s < nblk; s++) {
    const int64_t j = forward ? s : nblk - 1 - s;
    mx_trsm_step st = {};
    st.j0 = j * w;
    st.nv = (int)(n - st.j0 < w ? n - st.j0 : w);
    st.t_off = st.j0 + st.j0 * ldt;
    st.x_off = side ? st.j0 * ldb : st.j0;
    st.rest0 = forward ? st.j0 + w : 0;
    st.rest_len = forward ? np - st.rest0 : st.j0;
    st.gk = w;
    st.ldc = ldb;
    if (!side) {                         // B_rest += op(T)[rest, j] * (-X_j)
      st.gm = st.rest_len; st.gn = r;
      st.trans_a = trans;
      st.a_off = trans ? st.j0 + st.rest0 * ldt : st.rest0 + st.j0 * ldt;
      st.lda = ldt;
      st.trans_b = 0; st.b_off = 0; st.ldb = w;
      st.c_off = st.rest0;
    } else {                             // B_rest += (-X_j) * op(T)[j, rest]
      st.gm = r; st.gn = st.rest_len;
      st.trans_a = 0; st.a_off = 0; st.lda = r;
      st.trans_b = trans;
      st.b_off = trans ? st.rest0 + st.j0 * ldt : st.j0 + st.rest0 * ldt;
      st.ldb = ldt;
      st.c_off = st.rest0 * ldb;
    }
    out->steps.push_back(st);
  }
}
#endif  // MX_TRSM_HOST

#endif  // MARLIN_TRSM_PLAN_H
