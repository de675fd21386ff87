// The arithmetic of mmego_blend_windows and mmego_colsum_phase (blend.hip), per output column, as host + device functions: the kernels
// call them once per lane, scripts/blend_host_check.hip calls them lane by lane on the CPU (under the host sanitizers) and compares
// with its own long-double sums.  The recipe is the comment of the two entry points in include/mmego_hip.h.
#pragma once

#define BL_HD __host__ __device__ __forceinline__

// Column c of one frame's blend over the cover entries [k0, k1): the weighted mean in double, products and sums in CSR order.
// *wsum receives the sum of the weights.  An entry whose row lies outside [0, nrows) is skipped (the caller answers for the cover;
// this only keeps a bad one from reading outside src).  No entries, or weights that sum to zero: 0.
BL_HD double bl_blend_col(const float* __restrict__ src, long nrows, int C, const int* __restrict__ cov_row,
                          const float* __restrict__ cov_w, long long k0, long long k1, int c, double* wsum) {
  double acc = 0.0, ws = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const long r = (long)cov_row[k];
    if (r < 0 || r >= nrows) continue;
    const double w = (double)cov_w[k];
    acc += w * (double)src[r * C + c];
    ws += w;
  }
  *wsum = ws;
  return ws != 0.0 ? acc / ws : 0.0;
}

// The same entries' weighted squared distance from the blend m (the double, before its rounding) in column c: sum_k w_k (x_k - m)^2.
BL_HD double bl_spread_col(const float* __restrict__ src, long nrows, int C, const int* __restrict__ cov_row,
                           const float* __restrict__ cov_w, long long k0, long long k1, int c, double m) {
  double s = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const long r = (long)cov_row[k];
    if (r < 0 || r >= nrows) continue;
    const double d = (double)src[r * C + c] - m;
    s += (double)cov_w[k] * (d * d);
  }
  return s;
}

// spread of a frame from the sum of bl_spread_col over its C = 3 J columns: sqrt(total / (J wsum)); 0 where that is not positive.
BL_HD float bl_spread(double total, double wsum, int C) {
  const double q = wsum != 0.0 ? total / ((double)(C / 3) * wsum) : 0.0;
  return q > 0.0 ? (float)sqrt(q) : 0.0f;
}

// Column c of phase p: rows i = first, first + step, ... of the n rows of that phase (row i of phase p is row i * period + p of X),
// summed in double in ascending order.
BL_HD double bl_phase_partial(const float* __restrict__ X, long ldx, long n, int period, int p, int c, int first, int step) {
  double s = 0.0;
  for (long i = first; i < n; i += step) s += (double)X[(i * period + p) * ldx + c];
  return s;
}
