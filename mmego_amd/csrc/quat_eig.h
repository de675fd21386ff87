// The eigen-solver of the quaternion fits, as host + device functions: the largest eigenvalue of a symmetric 4 x 4 matrix and its unit
// eigenvector by cyclic Jacobi sweeps, a fixed number of them.  metrics.hip fits a rotation to two point sets with it (Horn's closed
// form), blend_rot.hip averages rotations with it (rot_blend_math.h); scripts/rot_blend_host_check.hip runs it on the CPU.  Every array
// is indexed by constants only, so on the device nothing of it lives in scratch memory.
#pragma once

#define MT_HD __host__ __device__ __forceinline__

#define MT_SWEEPS 10       // cyclic Jacobi converges quadratically; a 4 x 4 matrix is at rounding level after 5 or 6 sweeps

// One Jacobi rotation of the symmetric a in the (P, Q) plane, accumulated into the eigenvector columns of v.  A rotation whose
// off-diagonal element is zero, or vanishes against both diagonal elements, is skipped (theta = (a_qq - a_pp) / (2 a_pq) would
// overflow when squared); where it only vanishes against their difference, t = a_pq / (a_qq - a_pp) is the small-angle limit.
template <int P, int Q>
MT_HD void mt_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  const double big = 100.0 * fabs(apq);
  if (apq == 0.0 || (fabs(a[P][P]) + big == fabs(a[P][P]) && fabs(a[Q][Q]) + big == fabs(a[Q][Q]))) {
    a[P][Q] = a[Q][P] = 0.0;
    return;
  }
  const double h = a[Q][Q] - a[P][P];
  double t;
  if (fabs(h) + big == fabs(h)) {
    t = apq / h;
  } else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double x = a[r][P], y = a[r][Q];
      a[r][P] = a[P][r] = x - s * (y + tau * x);
      a[r][Q] = a[Q][r] = y + s * (x - tau * y);
    }
    const double x = v[r][P], y = v[r][Q];
    v[r][P] = x - s * (y + tau * x);
    v[r][Q] = y + s * (x - tau * y);
  }
}

// Largest eigenvalue of the symmetric a (destroyed) and its unit eigenvector q.  Of equal diagonal elements the first one wins, so the
// zero matrix gives q = (1, 0, 0, 0): the identity.
MT_HD double mt_top_eigenpair(double (&a)[4][4], double* q) {
  double v[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < MT_SWEEPS; ++sweep) {
    mt_rotate<0, 1>(a, v); mt_rotate<0, 2>(a, v); mt_rotate<0, 3>(a, v);
    mt_rotate<1, 2>(a, v); mt_rotate<1, 3>(a, v); mt_rotate<2, 3>(a, v);
  }
  double lam = a[0][0];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = v[r][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = a[k][k] > lam;
    lam = up ? a[k][k] : lam;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = up ? v[r][k] : q[r];
  }
  const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));      // (1 up to rounding: the columns of v are rotations of I)
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] /= n;
  return lam;
}

// The same, and *second receives the second-largest eigenvalue (counted with multiplicity: equal to the largest where that one is
// double): the sweeps and the choice among equal diagonal elements are mt_top_eigenpair's, so are the bits of q and of the result.
MT_HD double mt_top_two_eigenpair(double (&a)[4][4], double* q, double* second) {
  double v[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < MT_SWEEPS; ++sweep) {
    mt_rotate<0, 1>(a, v); mt_rotate<0, 2>(a, v); mt_rotate<0, 3>(a, v);
    mt_rotate<1, 2>(a, v); mt_rotate<1, 3>(a, v); mt_rotate<2, 3>(a, v);
  }
  double lam = a[0][0], sec = a[1][1];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = v[r][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const double d = a[k][k];
    const bool up = d > lam;
    sec = up ? lam : ((k == 1 || d > sec) ? d : sec);
    lam = up ? d : lam;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = up ? v[r][k] : q[r];
  }
  const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] /= n;
  *second = sec;
  return lam;
}
