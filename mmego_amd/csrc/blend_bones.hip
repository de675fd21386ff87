// Dense inference's bone-length-preserving blend (dense.dense_infer, blend_space="bones"): every frame's skeleton from the window
// rows that cover it, its roots blended as mmego_blend_windows blends them, every bone's DIRECTION blended over the cover, set to the
// body's bone length and laid along the kinematic tree -- rotation about a bone's own axis moves no joint, so directions are all a
// rigid blend of joints needs.  And the check of the result: every row's deviation from the bone lengths.  Like blend.hip a memory-bound
// gather of whole rows of at most 63 floats: one wave per frame, one lane per JOINT (its three columns and its parent's), a parent's
// position handed from lane to lane by wave shuffles, no LDS, no atomics, every sum in a fixed order (two launches give the same
// bits), double inside, one float store.  The arithmetic per joint is bone_blend_math.h; the recipe is the comment of the two entry
// points in include/mmego_hip.h, tests/bone_blend_ref.py restates it in numpy.
#include "common.h"
#include "bone_blend_math.h"
#include "skeleton_walk.h"

#define BB_WAVES 4                       // one wave per output frame, four per workgroup (no barrier: a wave behind F leaves)

__global__ __launch_bounds__(64 * BB_WAVES) void blend_bones_kernel(const float* __restrict__ src, long nrows, int J,
                                                                   const long long* __restrict__ cov_off,
                                                                   const int* __restrict__ cov_row, const float* __restrict__ cov_w,
                                                                   long F, const int* __restrict__ bones,
                                                                   const float* __restrict__ bone_len, int NB, float* __restrict__ dst,
                                                                   long ldd, float* __restrict__ spread, int* __restrict__ fallback) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * BB_WAVES + wave;
  if (f >= F) return;
  const long long k0 = cov_off[f], k1 = cov_off[f + 1];
  const int C = 3 * J;
  const bool joint = lane < J;
  const int j = joint ? lane : 0;        // (the lanes behind the row re-read joint 0 and store nothing)
  int mine, parent;                      // this lane's bone: the one whose child it is
  sw_lane_bone(bones, NB, J, lane, &mine, &parent);
  double s[3], best[3], u[3] = {0.0, 0.0, 0.0}, pos[3] = {0.0, 0.0, 0.0}, W;
  int n;
  long one;
  bb_gather(src, nrows, C, cov_row, cov_w, k0, k1, j, parent, s, best, &W, &n, &one);      // (W, n and one: the same in every lane)
  int fell = 0;
  if (n == 1 && W != 0.0) {              // covered once: the row itself
    for (int i = 0; i < 3; ++i) pos[i] = (double)src[one * C + 3 * j + i];
  } else if (n >= 1 && W != 0.0) {
    const double L = mine >= 0 ? (double)bone_len[mine] : 0.0;
    if (mine >= 0) {
      fell = bb_direction(s, best, W, L, u);
    } else {
      double ws;
      for (int i = 0; i < 3; ++i) pos[i] = bl_blend_col(src, nrows, C, cov_row, cov_w, k0, k1, 3 * j + i, &ws);
    }
    sw_walk(bones, NB, J, mine, L, u, pos);
  }
  sw_store(dst + f * ldd, J, lane, pos);
  if (spread) {
    double q = 0.0;
    if (joint)
      for (int i = 0; i < 3; ++i) q += bl_spread_col(src, nrows, C, cov_row, cov_w, k0, k1, 3 * j + i, pos[i]);
    q = wave_sum_d(q);
    if (lane == 0) spread[f] = bl_spread(q, W, C);   // (no entry, or weights that sum to zero: 0)
  }
  if (fallback) sw_count(fallback + f, lane, mine >= 0 && fell);
}

__global__ __launch_bounds__(256) void bone_length_dev_kernel(const float* __restrict__ X, long ldx, long n, int J,
                                                              const int* __restrict__ bones, const float* __restrict__ bone_len, int NB,
                                                              float* __restrict__ out, long ldo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * NB) return;
  const long r = i / NB;
  const int b = (int)(i - r * NB);
  const int c = bones[2 * b], p = bones[2 * b + 1];
  const bool inside = c >= 0 && c < J && p >= 0 && p < J;      // (a bone outside the row: 0, nothing read)
  out[r * ldo + b] = inside ? (float)bb_length_dev(X + r * ldx, c, p, (double)bone_len[b]) : 0.0f;
}

extern "C" int mmego_blend_bones(void* stream, const float* src, long nrows, int J, const long long* cov_off, const int* cov_row,
                                 const float* cov_w, long F, const int* bones, const float* bone_len, int NB, float* dst, long ldd,
                                 float* spread, int* fallback) {
  MMEGO_REQUIRE(src && cov_off && cov_row && cov_w && dst);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && nrows >= 0 && J >= 1 && J <= BB_MAX_J && ldd >= 3 * J);
  MMEGO_REQUIRE(NB >= 0 && NB <= J - 1 && (NB == 0 || (bones && bone_len)));
  hipLaunchKernelGGL(blend_bones_kernel, dim3((unsigned)cdiv(F, BB_WAVES)), dim3(64 * BB_WAVES), 0, (hipStream_t)stream, src, nrows, J,
                     cov_off, cov_row, cov_w, F, bones, bone_len, NB, dst, ldd, spread, fallback);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_bone_length_dev(void* stream, const float* X, long ldx, long n, int J, const int* bones, const float* bone_len,
                                     int NB, float* out, long ldo) {
  MMEGO_REQUIRE(X && bones && bone_len && out);
  MMEGO_REQUIRE(n >= 1 && n < (1L << 26) && J >= 1 && J <= BB_MAX_J && NB >= 1 && NB <= J - 1 && ldx >= 3 * J && ldo >= NB);
  hipLaunchKernelGGL(bone_length_dev_kernel, dim3((unsigned)cdiv(n * NB, 256)), dim3(256), 0, (hipStream_t)stream, X, ldx, n, J, bones,
                     bone_len, NB, out, ldo);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
