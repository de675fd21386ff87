// The arithmetic of mmego_blend_bones and mmego_bone_length_dev (blend_bones.hip), per joint, as host + device functions: the kernels
// call them once per lane, scripts/bone_blend_host_check.hip calls them lane by lane on the CPU (under the host sanitizers) and
// compares with its own long-double sums.  The recipe is the comment of the two entry points in include/mmego_hip.h.
#pragma once
#include "blend_math.h"

#define BB_MAX_J 21                      // one lane per joint; a row is at most 63 floats
#define BB_TINY 1e-9                     // a bone's summed vector below BB_TINY W L has no direction: the fallback

// One joint's pass over the cover entries [k0, k1) of a frame, in CSR order; an entry whose row lies outside [0, nrows) is skipped as
// bl_blend_col skips it.  *wsum: the sum of the valid entries' weights (bl_blend_col's own sum, the same bits), *nvalid their number,
// *one the last valid row.  With a parent (p >= 0), joint c being a bone's child: s = sum_k w_k (x_kc - x_kp), every difference formed
// in double, and best = the difference of the valid entry with the largest weight, the first such entry on ties.  p < 0: s, best stay 0.
BL_HD void bb_gather(const float* __restrict__ src, long nrows, int C, const int* __restrict__ cov_row, const float* __restrict__ cov_w,
                     long long k0, long long k1, int c, int p, double s[3], double best[3], double* wsum, int* nvalid, long* one) {
  double ws = 0.0, wbest = 0.0;
  int n = 0;
  long last = 0;
  s[0] = s[1] = s[2] = 0.0;
  best[0] = best[1] = best[2] = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const long r = (long)cov_row[k];
    if (r < 0 || r >= nrows) continue;
    const double w = (double)cov_w[k];
    if (p >= 0) {
      const float* x = src + r * C;
      const double d0 = (double)x[3 * c] - (double)x[3 * p], d1 = (double)x[3 * c + 1] - (double)x[3 * p + 1],
                   d2 = (double)x[3 * c + 2] - (double)x[3 * p + 2];
      s[0] += w * d0, s[1] += w * d1, s[2] += w * d2;
      if (n == 0 || w > wbest) wbest = w, best[0] = d0, best[1] = d1, best[2] = d2;
    }
    ws += w;
    last = r;
    ++n;
  }
  *wsum = ws, *nvalid = n, *one = last;
}

// The unit direction u of a bone of length L from bb_gather's s and best under the weight sum W: s / |s| where |s| > BB_TINY W L (and
// > 0: no 0 / 0 under a negative W); otherwise the fallback, best / |best|, or the zero vector where best is zero too.  -> 1 for the
// fallback, else 0.
BL_HD int bb_direction(const double s[3], const double best[3], double W, double L, double u[3]) {
  const double n = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
  if (n > BB_TINY * W * L && n > 0.0) {
    u[0] = s[0] / n, u[1] = s[1] / n, u[2] = s[2] / n;
    return 0;
  }
  const double m = sqrt(best[0] * best[0] + best[1] * best[1] + best[2] * best[2]);
  u[0] = u[1] = u[2] = 0.0;
  if (m > 0.0) u[0] = best[0] / m, u[1] = best[1] / m, u[2] = best[2] / m;
  return 1;
}

// | |x_c - x_p| - L | of one row x of 3-vectors, in double.
BL_HD double bb_length_dev(const float* __restrict__ x, int c, int p, double L) {
  const double d0 = (double)x[3 * c] - (double)x[3 * p], d1 = (double)x[3 * c + 1] - (double)x[3 * p + 1],
               d2 = (double)x[3 * c + 2] - (double)x[3 * p + 2];
  return fabs(sqrt(d0 * d0 + d1 * d1 + d2 * d2) - L);
}
