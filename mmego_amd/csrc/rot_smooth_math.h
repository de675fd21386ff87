// What mmego_smooth_rot (smooth.hip) adds to smooth_math.h and rot_blend_math.h, per bone and tap, as host + device functions: the
// kernel calls them once per lane, scripts/rot_smooth_host_check.hip calls them lane by lane on the CPU (under the host sanitizers) and
// compares with its own long-double arithmetic.  The recipe is the comment of the entry point in include/mmego_hip.h.  Every array is
// indexed by constants only (the loops unroll), so on the device nothing lives in scratch memory.
#pragma once
#include "smooth_math.h"
#include "rot_blend_math.h"

// A = the rotation matrix of the stored quaternion (w, x, y, z), in double from its four floats (even in the quaternion).
BL_HD void rs_matrix(float qw, float qx, float qy, float qz, double A[9]) {
  const double q[4] = {(double)qw, (double)qx, (double)qy, (double)qz};
  br_matrix(q, A);
}

// One tap's term of S = sum_k c_k A_k and of W = sum_k |c_k|.
BL_HD void rs_acc(double S[9], double* W, double c, const double A[9]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) S[i] += c * A[i];
  *W += fabs(c);
}

// The filtered rotation of a bone from S, the frame's own rotation A0 (the fallback) and W: br_mean's quaternion qm, its matrix Q and
// *theta, the angle between Q and A0.  -> 1 for the fallback, else 0.
BL_HD int rs_mean(const double S[9], const double A0[9], double W, double qm[4], double Q[9], double* theta) {
  const int fell = br_mean(S, A0, W, qm);
  br_matrix(qm, Q);
  *theta = br_angle(Q, A0);
  return fell;
}

// rot_moved of a frame from the sum over its bones of theta_b^2: sqrt(total / NB); 0 where that is not positive.
BL_HD float rs_rot_moved(double total, int NB) {
  const double x = NB > 0 ? total / (double)NB : 0.0;
  return x > 0.0 ? (float)sqrt(x) : 0.0f;
}
