// Aligned evaluation metrics (not in the reference): per frame, the predicted skeleton is compared with the target root-relative,
// after a rigid fit (proper rotation + shift) and after a similarity fit (Procrustes: scale as well), plus PCK on the absolute
// errors; per sequence, the error of the joints' second differences over time.  Together they split the reference's absolute joint
// error (mmego_pose_errors) into the articulated pose and the placement of the body by the head pose R, t.
//
// The fit is Horn's closed form (J. Opt. Soc. Am. A 4(4), 1987): the unit quaternion of the best proper rotation is the eigenvector of
// the largest eigenvalue of a symmetric 4 x 4 matrix made from the cross-covariance of the centred joints; the optimal scale is that
// eigenvalue over the spread of the prediction.  A reflection is never chosen -- the search space is the rotations -- which is what
// the SVD solution needs a determinant correction for.  The eigenpair comes from cyclic Jacobi sweeps, a fixed number of them.
//
// One thread per frame (per sequence and joint for the second differences), all arithmetic in double from the fp32 inputs converted
// exactly, float stores.  A thread re-reads its 63 + 63 floats in three passes over the joints (they stay in its cache lines) instead
// of holding them: the 4 x 4 matrix and its eigenvectors are 32 doubles, and every array below is indexed by constants only, so
// nothing lives in scratch memory.  Every sum runs over the joints (the frames of a sequence) in index order: two launches, same bits.
#include "common.h"
#include "quat_eig.h"        // MT_HD, MT_SWEEPS, mt_top_eigenpair: the cyclic Jacobi eigen-solver (shared with blend_rot.hip)

#define MT_MAX_THR 8

// Joint j of the J compared ones: prediction and target as doubles.
// J = 21: the assembled skeleton of pose_errors_kernel (geom.hip) -- joints 12..19 from `lower` (it overwrites the shared hips 12 and
// 16), the others from `upper` at their position in upper_joint_map [0..12, 16, 20].  J = 15: `upper` against target[upper_joint_map].
template <int J>
MT_HD void mt_joint(const float* __restrict__ upper, const float* __restrict__ lower, const float* __restrict__ target, long f, int j,
                    double* p, double* g) {
  const float* ps;
  const float* gs;
  if (J == 21) {
    ps = (j >= 12 && j < 20) ? lower + (f * 8 + (j - 12)) * 3 : upper + (f * 15 + (j == 20 ? 14 : j)) * 3;
    gs = target + (f * 21 + j) * 3;
  } else {
    ps = upper + (f * 15 + j) * 3;
    gs = target + (f * 21 + (j < 13 ? j : (j == 13 ? 16 : 20))) * 3;
  }
  p[0] = (double)ps[0]; p[1] = (double)ps[1]; p[2] = (double)ps[2];
  g[0] = (double)gs[0]; g[1] = (double)gs[1]; g[2] = (double)gs[2];
}

// One frame's row of mmego_pose_errors_aligned (the layout is in include/mmego_hip.h).
template <int J>
MT_HD void mt_aligned_frame(const float* __restrict__ upper, const float* __restrict__ lower, const float* __restrict__ target, long f,
                            const float* __restrict__ thr, int nthr, float* __restrict__ row) {
  double p[3], g[3], p0[3], g0[3];
  double thrv[MT_MAX_THR];
  int hit[MT_MAX_THR];
#pragma unroll
  for (int k = 0; k < MT_MAX_THR; ++k) {
    thrv[k] = k < nthr ? (double)thr[k] : -1.0;          // (no distance is <= -1: an unused counter stays 0)
    hit[k] = 0;
  }
  // pass 1: centroids, root-relative errors, PCK of the absolute errors
  mt_joint<J>(upper, lower, target, f, 0, p0, g0);
  double sp[3] = {0.0, 0.0, 0.0}, sg[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int j = 0; j < J; ++j) {
    mt_joint<J>(upper, lower, target, f, j, p, g);
    double e2 = 0.0, d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      sp[i] += p[i];
      sg[i] += g[i];
      const double e = (p[i] - p0[i]) - (g[i] - g0[i]), d = p[i] - g[i];
      e2 += e * e;
      d2 += d * d;
    }
    row[j] = (float)sqrt(e2);
    const double dist = sqrt(d2);
#pragma unroll
    for (int k = 0; k < MT_MAX_THR; ++k) hit[k] += dist <= thrv[k] ? 1 : 0;
  }
  double shift2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sp[i] /= (double)J;
    sg[i] /= (double)J;
    shift2 += (sp[i] - sg[i]) * (sp[i] - sg[i]);
  }
  // pass 2: cross-covariance S[a][b] = sum (p - pbar)_a (g - gbar)_b and the spread of the prediction
  double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, pp = 0.0;
#pragma unroll 1
  for (int j = 0; j < J; ++j) {
    mt_joint<J>(upper, lower, target, f, j, p, g);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double pa = p[a] - sp[a];
      pp += pa * pa;
#pragma unroll
      for (int b = 0; b < 3; ++b) S[a][b] += pa * (g[b] - sg[b]);
    }
  }
  double N[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2];
  N[1][1] = S[0][0] - S[1][1] - S[2][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
  N[0][1] = N[1][0] = S[1][2] - S[2][1];
  N[0][2] = N[2][0] = S[2][0] - S[0][2];
  N[0][3] = N[3][0] = S[0][1] - S[1][0];
  N[1][2] = N[2][1] = S[0][1] + S[1][0];
  N[1][3] = N[3][1] = S[2][0] + S[0][2];
  N[2][3] = N[3][2] = S[1][2] + S[2][1];
  double q[4];
  const double lam = mt_top_eigenpair(N, q);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  // (a prediction without spread has a zero covariance: q = (1, 0, 0, 0) above, R = I, angle 0; its scale is defined as 0)
  const double scale = pp > 0.0 ? lam / pp : 0.0;
  // pass 3: residuals of the rigid and of the similarity fit
#pragma unroll 1
  for (int j = 0; j < J; ++j) {
    mt_joint<J>(upper, lower, target, f, j, p, g);
    double r2 = 0.0, s2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double rp = (R[a][0] * (p[0] - sp[0]) + R[a][1] * (p[1] - sp[1])) + R[a][2] * (p[2] - sp[2]);
      const double gc = g[a] - sg[a];
      r2 += (rp - gc) * (rp - gc);
      s2 += (scale * rp - gc) * (scale * rp - gc);
    }
    row[J + j] = (float)sqrt(r2);
    row[2 * J + j] = (float)sqrt(s2);
  }
  row[3 * J] = (float)(2.0 * atan2(sqrt(x * x + y * y + z * z), fabs(w)) * (180.0 / 3.14159265358979323846));
  row[3 * J + 1] = (float)sqrt(shift2);
  row[3 * J + 2] = (float)scale;
#pragma unroll
  for (int k = 0; k < MT_MAX_THR; ++k)
    if (k < nthr) row[3 * J + 3 + k] = (float)((double)hit[k] / (double)J);
}

// Joint j of sequence b: mean over t = 1 .. T-2 of |(p[t-1] - 2 p[t] + p[t+1]) - (g[t-1] - 2 g[t] + g[t+1])|, summed in t order.
template <int J>
MT_HD float mt_accel_joint(const float* __restrict__ upper, const float* __restrict__ lower, const float* __restrict__ target, long b,
                           int T, int j) {
  double pa[3], pb[3], pc[3], ga[3], gb[3], gc[3];
  mt_joint<J>(upper, lower, target, b * T, j, pa, ga);
  mt_joint<J>(upper, lower, target, b * T + 1, j, pb, gb);
  double sum = 0.0;
#pragma unroll 1
  for (int t = 1; t < T - 1; ++t) {
    mt_joint<J>(upper, lower, target, b * T + t + 1, j, pc, gc);
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double d = ((pa[i] - 2.0 * pb[i]) + pc[i]) - ((ga[i] - 2.0 * gb[i]) + gc[i]);
      d2 += d * d;
      pa[i] = pb[i]; pb[i] = pc[i];
      ga[i] = gb[i]; gb[i] = gc[i];
    }
    sum += sqrt(d2);
  }
  return (float)(sum / (double)(T - 2));
}

template <int J>
__global__ __launch_bounds__(128) void pose_errors_aligned_kernel(const float* __restrict__ upper, const float* __restrict__ lower,
                                                                  const float* __restrict__ target, long F,
                                                                  const float* __restrict__ thr, int nthr, float* __restrict__ A,
                                                                  long lda) {
  const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  mt_aligned_frame<J>(upper, lower, target, f, thr, nthr, A + f * lda);
}

template <int J>
__global__ __launch_bounds__(128) void pose_accel_errors_kernel(const float* __restrict__ upper, const float* __restrict__ lower,
                                                                const float* __restrict__ target, long B, int T,
                                                                float* __restrict__ Acc, long lda) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * J) return;
  const long b = i / J;
  const int j = (int)(i - b * J);
  Acc[b * lda + j] = mt_accel_joint<J>(upper, lower, target, b, T, j);
}

extern "C" int mmego_pose_errors_aligned_width(int J, int nthr) { return 3 * J + 3 + nthr; }

extern "C" int mmego_pose_errors_aligned(void* stream, const float* upper, const float* lower, const float* target, long F,
                                         const float* thr, int nthr, float* A, long lda) {
  const int J = lower ? 21 : 15;
  MMEGO_REQUIRE(upper && target && A && F > 0 && nthr >= 0 && nthr <= MT_MAX_THR && (thr || nthr == 0) &&
                lda >= mmego_pose_errors_aligned_width(J, nthr));
  if (lower)
    hipLaunchKernelGGL(pose_errors_aligned_kernel<21>, dim3(cdiv(F, 128)), dim3(128), 0, (hipStream_t)stream, upper, lower, target, F, thr,
                       nthr, A, lda);
  else
    hipLaunchKernelGGL(pose_errors_aligned_kernel<15>, dim3(cdiv(F, 128)), dim3(128), 0, (hipStream_t)stream, upper, lower, target, F, thr,
                       nthr, A, lda);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_pose_accel_errors(void* stream, const float* upper, const float* lower, const float* target, long B, int T,
                                       float* Acc, long lda) {
  const int J = lower ? 21 : 15;
  MMEGO_REQUIRE(upper && target && Acc && B > 0 && T >= 3 && lda >= J);
  if (lower)
    hipLaunchKernelGGL(pose_accel_errors_kernel<21>, dim3(cdiv(B * J, 128)), dim3(128), 0, (hipStream_t)stream, upper, lower, target, B, T,
                       Acc, lda);
  else
    hipLaunchKernelGGL(pose_accel_errors_kernel<15>, dim3(cdiv(B * J, 128)), dim3(128), 0, (hipStream_t)stream, upper, lower, target, B, T,
                       Acc, lda);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
