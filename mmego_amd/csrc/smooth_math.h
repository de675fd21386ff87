// The arithmetic of mmego_smooth_frames and mmego_smooth_bones (smooth.hip), per tap and per column, as host + device functions: the
// kernels call them once per lane, scripts/smooth_host_check.hip calls them lane by lane on the CPU (under the host sanitizers) and
// compares with its own long-double sums.  The recipe is the comment of the two entry points in include/mmego_hip.h.
#pragma once
#include "bone_blend_math.h"

#define SM_MAX_H 31                      // one lane per tap: 2 H + 1 <= 63 taps fit one wave
#define SM_MAX_C 64                      // one lane per column

// Tap k's share of the moments S_m = sum_k w_k k^m, m = 0 .. 4 (an invalid tap shares nothing: the caller passes w = 0).
BL_HD void sm_tap_moments(double w, int k, double t[5]) {
  const double x = (double)k;
  double p = w;
  for (int m = 0; m < 5; ++m) t[m] = p, p *= x;
}

// The degree a frame with n valid taps is fitted with: min(D, n - 1).
BL_HD int sm_degree(int D, int n) { return D < n - 1 ? D : n - 1; }

// A = the first row of the inverse of the moment matrix [S_{i+j}], i, j <= deg, by cofactors (the matrix is symmetric: its first row
// of cofactors over the determinant); the entries beyond deg are 0.  deg + 1 distinct abscissae with positive weights: the matrix is
// positive definite, the determinant > 0.
BL_HD void sm_first_row(const double S[5], int deg, double A[3]) {
  A[0] = A[1] = A[2] = 0.0;
  if (deg <= 0) {
    A[0] = 1.0 / S[0];
  } else if (deg == 1) {
    const double det = S[0] * S[2] - S[1] * S[1];
    A[0] = S[2] / det, A[1] = -S[1] / det;
  } else {
    const double c0 = S[2] * S[4] - S[3] * S[3], c1 = S[2] * S[3] - S[1] * S[4], c2 = S[1] * S[3] - S[2] * S[2];
    const double det = S[0] * c0 + S[1] * c1 + S[2] * c2;
    A[0] = c0 / det, A[1] = c1 / det, A[2] = c2 / det;
  }
}

// c_k = w_k (A . [1, k, k^2]) (the entries of A beyond the degree are 0).
BL_HD double sm_coef(const double A[3], double w, int k) {
  const double x = (double)k;
  return w * (A[0] + A[1] * x + A[2] * (x * x));
}

// One tap's term of y = sum_k c_k x_k: the one spelling both kernels sum their columns with, so that a root of mmego_smooth_bones
// carries the bits of mmego_smooth_frames' column.
BL_HD double sm_acc(double acc, double c, float x) { return acc + c * (double)x; }

// moved of a frame from the sum over its C = 3 J columns of (y - x)^2: the RMS over the joints of |y_j - x_j|.
BL_HD float sm_moved(double total, int C) {
  const double q = total / (double)(C / 3);
  return q > 0.0 ? (float)sqrt(q) : 0.0f;
}
