// Dense inference (dense.dense_infer): every frame's pose blended from the overlapping windows that cover it, and the per-row
// error table of all windows folded by position in the window.  Both kernels are memory-bound gathers of whole rows of at most 64
// floats: one lane per column, so a row is one coalesced read of the wave; no atomics, every sum in a fixed order (two launches give
// the same bits), double inside, one float store.  The arithmetic per column is blend_math.h; the recipe is the comment of the two
// entry points in include/mmego_hip.h, tests/dense_ref.py restates it in numpy.
#include "common.h"
#include "blend_math.h"

#define BL_WAVES 4                       // blend: one wave per output frame, four per workgroup (no barrier: a wave behind F leaves)
#define BL_MAX_C 64                      // one lane per column
#define CP_WAVES 16                      // phase sums: one workgroup per phase, its rows dealt round-robin to 16 waves

__global__ __launch_bounds__(64 * BL_WAVES) void blend_windows_kernel(const float* __restrict__ src, long nrows, int C,
                                                                     const long long* __restrict__ cov_off,
                                                                     const int* __restrict__ cov_row, const float* __restrict__ cov_w,
                                                                     long F, float* __restrict__ dst, long ldd, float* __restrict__ spread) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * BL_WAVES + wave;
  if (f >= F) return;
  const long long k0 = cov_off[f], k1 = cov_off[f + 1];
  const bool col = lane < C;
  const int c = col ? lane : 0;          // (the lanes behind the row re-read column 0 and store nothing)
  double wsum;
  const double m = bl_blend_col(src, nrows, C, cov_row, cov_w, k0, k1, c, &wsum);
  if (col) dst[f * ldd + lane] = (float)m;
  if (spread) {
    const double s = wave_sum_d(col ? bl_spread_col(src, nrows, C, cov_row, cov_w, k0, k1, c, m) : 0.0);
    if (lane == 0) spread[f] = bl_spread(s, wsum, C);
  }
}

__global__ __launch_bounds__(64 * CP_WAVES) void colsum_phase_kernel(const float* __restrict__ X, long ldx, long n, int C, int period,
                                                                    float* __restrict__ out, long ldo) {
  __shared__ double part[CP_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x;
  part[wave][lane] = bl_phase_partial(X, ldx, n, period, p, lane < C ? lane : 0, wave, CP_WAVES);
  __syncthreads();
  if (wave == 0 && lane < C) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) s += part[w][lane];
    out[(long)p * ldo + lane] = (float)s;
  }
}

extern "C" int mmego_blend_windows(void* stream, const float* src, long nrows, int C, const long long* cov_off, const int* cov_row,
                                   const float* cov_w, long F, float* dst, long ldd, float* spread) {
  MMEGO_REQUIRE(src && cov_off && cov_row && cov_w && dst);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && nrows >= 0 && C >= 1 && C <= BL_MAX_C && ldd >= C);
  MMEGO_REQUIRE(!spread || C % 3 == 0);
  hipLaunchKernelGGL(blend_windows_kernel, dim3((unsigned)cdiv(F, BL_WAVES)), dim3(64 * BL_WAVES), 0, (hipStream_t)stream, src, nrows, C,
                     cov_off, cov_row, cov_w, F, dst, ldd, spread);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_colsum_phase(void* stream, const float* X, long ldx, long rows, int C, int period, float* out, long ldo) {
  MMEGO_REQUIRE(X && out && rows >= 1 && period >= 1 && period <= 64 && rows % period == 0);
  MMEGO_REQUIRE(C >= 1 && C <= BL_MAX_C && ldx >= C && ldo >= C);
  hipLaunchKernelGGL(colsum_phase_kernel, dim3((unsigned)period), dim3(64 * CP_WAVES), 0, (hipStream_t)stream, X, ldx, rows / period, C,
                     period, out, ldo);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
