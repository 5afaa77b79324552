// Stand-alone host program (test fixture, never shipped): replays the
// copies mx_gemm_op makes -- zero the padded image, 2D-copy the tight host
// operand into it as stored, read the extent the kernel reads, copy C back
// -- on plain heap buffers sized exactly as the entry sizes them, using
// the entry's own arithmetic (marlin_amd/csrc/gemm_op_layout.h). Built
// with -fsanitize=address by tests/test_gemm_op_layout.py, so any extent
// that leaves a buffer aborts the run; the numeric result is checked too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_op_layout.h"

// hipMemcpy2D semantics on host memory
static void copy2d(double* dst, int64_t dpitch, const double* src,
                   int64_t spitch, int64_t rows, int64_t cols) {
  for (int64_t c = 0; c < cols; c++)
    memcpy(dst + c * dpitch, src + c * spitch, (size_t)rows * sizeof(double));
}

static int check(int ta, int tb, int64_t m, int64_t k, int64_t n) {
  mx_op_image ia, ib, ic;
  mx_gemm_op_layout(ta, tb, m, k, n, &ia, &ib, &ic);
  const int64_t mp = mx_op_round_up(m, 128), np = mx_op_round_up(n, 128),
                kp = mx_op_round_up(k, 16);
  // the workspaces are sized mp*kp, kp*np, mp*np whatever the form
  if (ia.elems() != mp * kp || ib.elems() != kp * np || ic.elems() != mp * np)
    return 1;
  // pitch contract of mxk_gemm_op: covers the run, 16-byte multiple
  if (ia.pitch < (ta ? kp : mp) || ib.pitch < (tb ? np : kp) || ic.pitch < mp)
    return 2;
  if (ia.pitch % 2 || ib.pitch % 2 || ic.pitch % 2) return 3;
  if (ia.rows * ia.cols != m * k || ib.rows * ib.cols != k * n) return 4;

  // exact-size heap buffers: host operands tight, images padded
  std::vector<double> A((size_t)(m * k)), B((size_t)(k * n)), C((size_t)(m * n));
  for (size_t i = 0; i < A.size(); i++) A[i] = (double)(i % 7) - 3;
  for (size_t i = 0; i < B.size(); i++) B[i] = (double)(i % 5) - 2;
  double* dA = (double*)malloc((size_t)ia.elems() * sizeof(double));
  double* dB = (double*)malloc((size_t)ib.elems() * sizeof(double));
  double* dC = (double*)malloc((size_t)ic.elems() * sizeof(double));
  memset(dA, 0xff, (size_t)ia.elems() * sizeof(double));
  memset(dB, 0xff, (size_t)ib.elems() * sizeof(double));
  if (ia.padded()) memset(dA, 0, (size_t)ia.elems() * sizeof(double));
  if (ib.padded()) memset(dB, 0, (size_t)ib.elems() * sizeof(double));
  copy2d(dA, ia.pitch, A.data(), ia.rows, ia.rows, ia.cols);
  copy2d(dB, ib.pitch, B.data(), ib.rows, ib.rows, ib.cols);

  // what the kernel reads: op(A) mp x kp, op(B) kp x np, through the
  // pitches handed to it; pads must contribute exact zeros
  int bad = 0;
  for (int64_t j = 0; j < np; j++)
    for (int64_t i = 0; i < mp; i++) {
      double acc = 0;
      for (int64_t l = 0; l < kp; l++) {
        double a = ta ? dA[i * ia.pitch + l] : dA[l * ia.pitch + i];
        double b = tb ? dB[l * ib.pitch + j] : dB[j * ib.pitch + l];
        acc += a * b;
      }
      dC[j * ic.pitch + i] = acc;
      if ((i >= m || j >= n) && acc != 0) bad = 5;
    }
  copy2d(C.data(), m, dC, ic.pitch, m, n);
  for (int64_t j = 0; j < n && !bad; j++)
    for (int64_t i = 0; i < m; i++) {
      double acc = 0;
      for (int64_t l = 0; l < k; l++)
        acc += (ta ? A[i * k + l] : A[l * m + i]) *
               (tb ? B[l * n + j] : B[j * k + l]);
      if (acc != C[j * m + i]) { bad = 6; break; }
    }
  free(dA); free(dB); free(dC);
  return bad;
}

int main() {
  const int64_t shapes[][3] = {{1, 1, 1},     {5, 3, 7},    {128, 16, 128},
                               {129, 17, 127}, {100, 33, 260}, {257, 15, 1},
                               {2, 130, 3}};
  int runs = 0;
  for (auto& s : shapes)
    for (int ta = 0; ta < 2; ta++)
      for (int tb = 0; tb < 2; tb++) {
        int rc = check(ta, tb, s[0], s[1], s[2]);
        if (rc) {
          printf("FAIL %d form %d%d shape %lldx%lldx%lld\n", rc, ta, tb,
                 (long long)s[0], (long long)s[1], (long long)s[2]);
          return 1;
        }
        runs++;
      }
  printf("gemm_op_layout OK %d\n", runs);
  return 0;
}
