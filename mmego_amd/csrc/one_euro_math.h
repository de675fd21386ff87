// The arithmetic of mmego_one_euro and mmego_one_euro_bones (one_euro.hip), per joint and frame, as host + device functions: the kernels
// call them once per lane and step, scripts/one_euro_host_check.hip calls them step by step on the CPU (under the host sanitizers) and
// compares with its own long-double recursion.  The recipe is the comment of the two entry points in include/mmego_hip.h.  Every
// multiply-add is spelt as fma(): the two kernels and the host give a root the same bits whatever the compiler would contract.
#pragma once
#include "smooth_math.h"                 // (sm_moved: moved is mmego_smooth_frames' figure; bb_direction through it)

#define OE_TWO_PI 6.283185307179586476925286766559

// alpha(fc) = w / (w + 1), w = 2 pi fc: the weight of the newest sample of an exponential filter of cutoff fc cycles per frame.
BL_HD double oe_alpha(double fc) {
  const double w = OE_TWO_PI * fc;
  return w / (w + 1.0);
}

// One frame of the recursion on a 3-vector x: d = x - xhat, dhat += alpha(DC) (d - dhat), s = |dhat|, xhat += alpha(FC + B s) d.
// ad = alpha(DC), taken once by the caller.  xhat and dhat are the state, in double, updated in place.
BL_HD void oe_step(const double x[3], double fc, double beta, double ad, double xhat[3], double dhat[3]) {
  const double d0 = x[0] - xhat[0], d1 = x[1] - xhat[1], d2 = x[2] - xhat[2];
  dhat[0] = fma(ad, d0 - dhat[0], dhat[0]), dhat[1] = fma(ad, d1 - dhat[1], dhat[1]), dhat[2] = fma(ad, d2 - dhat[2], dhat[2]);
  const double s = sqrt(fma(dhat[2], dhat[2], fma(dhat[1], dhat[1], dhat[0] * dhat[0])));
  const double a = oe_alpha(fma(beta, s, fc));
  xhat[0] = fma(a, d0, xhat[0]), xhat[1] = fma(a, d1, xhat[1]), xhat[2] = fma(a, d2, xhat[2]);
}

// v = x_c - x_p of a bone from its child's and its parent's three floats, every difference formed in double.
BL_HD void oe_bone_vector(const float c[3], const float p[3], double v[3]) {
  for (int i = 0; i < 3; ++i) v[i] = (double)c[i] - (double)p[i];
}

// One frame of a bone with the vector v = x_c - x_p: the recursion on v with the state vhat (unnormalised), dhat; then the unit
// direction u of the bone of length L: vhat / |vhat| where |vhat| > 1e-9 L, else -- the fallback -- the frame's own v normalised, or the
// zero vector where that is zero too (bb_direction with W = 1).  -> 1 for the fallback, else 0.
BL_HD int oe_bone_step(const double v[3], double fc, double beta, double ad, double L, double vhat[3], double dhat[3], double u[3]) {
  oe_step(v, fc, beta, ad, vhat, dhat);
  return bb_direction(vhat, v, 1.0, L, u);
}
