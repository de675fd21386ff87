// The arithmetic of mmego_blend_rot (blend_rot.hip), per bone, as host + device functions: the kernel calls them once per lane,
// scripts/rot_blend_host_check.hip calls them lane by lane on the CPU (under the host sanitizers) and compares with its own long-double
// arithmetic.  The recipe is the comment of the entry point in include/mmego_hip.h.  Matrices are nine doubles, row-major; every
// array is indexed by constants only (the loops below unroll), so on the device nothing lives in scratch memory.
#pragma once
#include "blend_math.h"
#include "quat_eig.h"

#define BR_MAX_J 21                      // one lane per joint; a row is at most 63 floats
#define BR_TINY 1e-9                     // eigenvalues of the mean's 4 x 4 matrix closer than BR_TINY W: no direction, the fallback

// A = Rh^T Q for two row-major 3 x 3 float matrices, in double: the world-frame rotation of a bone whose head-frame rotation is Q,
// the head-to-world transform being p <- Rh^T p + t.
BL_HD void br_world(const float* __restrict__ Rh, const float* __restrict__ Q, double A[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      A[3 * i + j] = ((double)Rh[i] * (double)Q[j] + (double)Rh[3 + i] * (double)Q[3 + j]) + (double)Rh[6 + i] * (double)Q[6 + j];
}

// One bone's pass over the cover entries [k0, k1) of a frame, in CSR order; an entry whose row lies outside [0, nrows) is skipped as
// bl_blend_col skips it.  *wsum: the sum of the valid entries' weights (bl_blend_col's own sum, the same bits), *nvalid their number,
// *one the last valid row.  With a rotation (ri >= 0; q [nrows][NQ][9], Rh [nrows][9]): S = sum_k w_k A_k, A_k = br_world(Rh[r_k],
// q[r_k][ri]), and best = the A_k of the valid entry with the largest weight, the first such entry on ties.  ri < 0: S, best stay 0.
BL_HD void br_gather(const float* __restrict__ q, const float* __restrict__ Rh, long nrows, int NQ, const int* __restrict__ cov_row,
                     const float* __restrict__ cov_w, long long k0, long long k1, int ri, double S[9], double best[9], double* wsum,
                     int* nvalid, long* one) {
  double ws = 0.0, wbest = 0.0;
  int n = 0;
  long last = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) S[i] = best[i] = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const long r = (long)cov_row[k];
    if (r < 0 || r >= nrows) continue;
    const double w = (double)cov_w[k];
    if (ri >= 0) {
      double A[9];
      br_world(Rh + r * 9, q + (r * NQ + ri) * 9, A);
      const bool take = n == 0 || w > wbest;
      wbest = take ? w : wbest;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        S[i] += w * A[i];
        best[i] = take ? A[i] : best[i];
      }
    }
    ws += w;
    last = r;
    ++n;
  }
  *wsum = ws, *nvalid = n, *one = last;
}

// The unit quaternion (w, x, y, z) of the proper rotation Q that maximises tr(Q^T S): the eigenvector of the largest eigenvalue of
// the symmetric 4 x 4 matrix of S below (for a rotation S it is S's own quaternion).  -> that eigenvalue; *second the next one.
BL_HD double br_quat_of(const double S[9], double quat[4], double* second) {
  double N[4][4];
  N[0][0] = S[0] + S[4] + S[8];
  N[1][1] = S[0] - S[4] - S[8];
  N[2][2] = -S[0] + S[4] - S[8];
  N[3][3] = -S[0] - S[4] + S[8];
  N[0][1] = N[1][0] = S[7] - S[5];
  N[0][2] = N[2][0] = S[2] - S[6];
  N[0][3] = N[3][0] = S[3] - S[1];
  N[1][2] = N[2][1] = S[1] + S[3];
  N[1][3] = N[3][1] = S[2] + S[6];
  N[2][3] = N[3][2] = S[5] + S[7];
  return mt_top_two_eigenpair(N, quat, second);
}

// The blended rotation of a bone from br_gather's S and best under the weight sum W, as a unit quaternion of canonical sign (its
// first non-zero component positive): br_quat_of(S) where the two largest eigenvalues lie more than BR_TINY W apart; otherwise the
// fallback, br_quat_of(best).  -> 1 for the fallback, else 0.
BL_HD int br_mean(const double S[9], const double best[9], double W, double quat[4]) {
  double second;
  const double top = br_quat_of(S, quat, &second);
  int fell = 0;
  if (!(top - second > BR_TINY * W)) {
    br_quat_of(best, quat, &second);
    fell = 1;
  }
  const double lead = quat[0] != 0.0 ? quat[0] : (quat[1] != 0.0 ? quat[1] : (quat[2] != 0.0 ? quat[2] : quat[3]));
  if (lead < 0.0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) quat[i] = -quat[i];
  }
  return fell;
}

// The rotation matrix of a unit quaternion (w, x, y, z).
BL_HD void br_matrix(const double quat[4], double Q[9]) {
  const double w = quat[0], x = quat[1], y = quat[2], z = quat[3];
  Q[0] = 1.0 - 2.0 * (y * y + z * z), Q[1] = 2.0 * (x * y - w * z), Q[2] = 2.0 * (x * z + w * y);
  Q[3] = 2.0 * (x * y + w * z), Q[4] = 1.0 - 2.0 * (x * x + z * z), Q[5] = 2.0 * (y * z - w * x);
  Q[6] = 2.0 * (x * z - w * y), Q[7] = 2.0 * (y * z + w * x), Q[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Q b for a rest bone vector b (floats), in double.
BL_HD void br_lay(const double Q[9], const float* __restrict__ b, double out[3]) {
  const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = (Q[3 * i] * b0 + Q[3 * i + 1] * b1) + Q[3 * i + 2] * b2;
}

// The angle in [0, pi] of D = Q^T A: atan2(|v|, (tr D - 1) / 2) with v = (D32 - D23, D13 - D31, D21 - D12) / 2 -- accurate at 0, where
// the arc cosine of the trace is not, and at pi.
BL_HD double br_angle(const double Q[9], const double A[9]) {
  double D[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = (Q[i] * A[j] + Q[3 + i] * A[3 + j]) + Q[6 + i] * A[6 + j];
  const double v0 = 0.5 * (D[7] - D[5]), v1 = 0.5 * (D[2] - D[6]), v2 = 0.5 * (D[3] - D[1]);
  return atan2(sqrt((v0 * v0 + v1 * v1) + v2 * v2), 0.5 * (((D[0] + D[4]) + D[8]) - 1.0));
}

// One bone's share of rot_spread: sum over the same valid entries of w_k theta_k^2, theta_k = br_angle(Q, A_k), in CSR order.
BL_HD double br_spread_bone(const float* __restrict__ q, const float* __restrict__ Rh, long nrows, int NQ,
                            const int* __restrict__ cov_row, const float* __restrict__ cov_w, long long k0, long long k1, int ri,
                            const double Q[9]) {
  double s = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const long r = (long)cov_row[k];
    if (r < 0 || r >= nrows) continue;
    double A[9];
    br_world(Rh + r * 9, q + (r * NQ + ri) * 9, A);
    const double th = br_angle(Q, A);
    s += (double)cov_w[k] * (th * th);
  }
  return s;
}

// rot_spread of a frame from the sum of br_spread_bone over its NB bones: sqrt(total / (NB wsum)); 0 where that is not positive.
BL_HD float br_rot_spread(double total, double wsum, int NB) {
  const double x = (wsum != 0.0 && NB > 0) ? total / ((double)NB * wsum) : 0.0;
  return x > 0.0 ? (float)sqrt(x) : 0.0f;
}
