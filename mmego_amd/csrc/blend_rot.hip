// Dense inference's blend in rotation space (dense.dense_infer, blend_space="rot"): every frame's skeleton from the ROTATIONS the
// nets predicted for it in the windows that cover it.  Per bone the world-frame rotations Rh^T q of the cover are averaged -- the
// weighted chordal mean, the proper rotation nearest their weighted sum, whose quaternion is the top eigenvector of a symmetric 4 x 4
// matrix (quat_eig.h) -- and the nets' own forward kinematics lays the rest bones along the averaged rotations from the vector-blended
// roots: the frames are rigid by construction, the twist about every bone is kept, and the quaternions are an output of their own.
// Like blend_bones.hip: one wave per frame, one lane per JOINT (the bone whose child it is), a parent's position handed from lane to
// lane by wave shuffles, no LDS, no atomics, every sum in a fixed order (two launches give the same bits), double inside, one float
// store per column and one float4 store per quaternion.  The arithmetic per bone is rot_blend_math.h; the recipe is the comment of the
// entry point in include/mmego_hip.h, tests/rot_blend_ref.py restates it in numpy by another method (SVD).
#include "common.h"
#include "rot_blend_math.h"
#include "skeleton_walk.h"

#define BR_WAVES 4                       // one wave per output frame, four per workgroup (no barrier: a wave behind F leaves)

__global__ __launch_bounds__(64 * BR_WAVES) void blend_rot_kernel(const float* __restrict__ src, long nrows, int J,
                                                                 const float* __restrict__ q, int NQ, const float* __restrict__ Rh,
                                                                 const long long* __restrict__ cov_off,
                                                                 const int* __restrict__ cov_row, const float* __restrict__ cov_w,
                                                                 long F, const int* __restrict__ bones,
                                                                 const int* __restrict__ rot_idx, const float* __restrict__ body,
                                                                 int NB, float* __restrict__ dst, long ldd, float* __restrict__ quat,
                                                                 float* __restrict__ spread, float* __restrict__ rot_spread,
                                                                 int* __restrict__ fallback) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * BR_WAVES + wave;
  if (f >= F) return;
  const long long k0 = cov_off[f], k1 = cov_off[f + 1];
  const int C = 3 * J;
  const bool joint = lane < J;
  const int j = joint ? lane : 0;        // (the lanes behind the row re-read joint 0 and store nothing)
  int mine, parent;                      // this lane's bone: the one whose child it is; one whose rotation lies outside the NQ of a
  sw_lane_bone(bones, NB, J, lane, &mine, &parent);      // row is left out as well: its child stays a root
  int ri = mine >= 0 ? rot_idx[mine] : -1;
  if (ri < 0 || ri >= NQ) mine = ri = -1;
  double S[9], best[9], Q[9], qm[4] = {0.0, 0.0, 0.0, 0.0}, lay[3] = {0.0, 0.0, 0.0}, pos[3] = {0.0, 0.0, 0.0}, W;
  int n;
  long one;
  br_gather(q, Rh, nrows, NQ, cov_row, cov_w, k0, k1, ri, S, best, &W, &n, &one);          // (W, n and one: the same in every lane)
  const bool covered = n >= 1 && W != 0.0;
  int fell = 0;
  if (covered && mine >= 0) {
    fell = br_mean(S, best, W, qm);
    br_matrix(qm, Q);
    br_lay(Q, body + 3 * mine, lay);
  }
  if (covered && n == 1) {               // covered once: the row itself
    for (int i = 0; i < 3; ++i) pos[i] = (double)src[one * C + 3 * j + i];
  } else if (covered) {
    if (mine < 0) {
      double ws;
      for (int i = 0; i < 3; ++i) pos[i] = bl_blend_col(src, nrows, C, cov_row, cov_w, k0, k1, 3 * j + i, &ws);
    }
    sw_walk(bones, NB, J, mine, 1.0, lay, pos);      // (1.0 * x rounds to x, and fma(1.0, x, p) as p + x does)
  }
  sw_store(dst + f * ldd, J, lane, pos);
  if (mine >= 0)                         // (no cover: the zero quaternion)
    reinterpret_cast<float4*>(quat)[f * NB + mine] = make_float4((float)qm[0], (float)qm[1], (float)qm[2], (float)qm[3]);
  if (spread) {
    double s = 0.0;
    if (joint)
      for (int i = 0; i < 3; ++i) s += bl_spread_col(src, nrows, C, cov_row, cov_w, k0, k1, 3 * j + i, pos[i]);
    s = wave_sum_d(s);
    if (lane == 0) spread[f] = bl_spread(s, W, C);   // (no entry, or weights that sum to zero: 0)
  }
  if (rot_spread) {
    double s = 0.0;
    if (covered && n > 1 && mine >= 0) s = br_spread_bone(q, Rh, nrows, NQ, cov_row, cov_w, k0, k1, ri, Q);
    s = wave_sum_d(s);
    if (lane == 0) rot_spread[f] = br_rot_spread(s, W, NB);       // (a frame covered once has nothing to disagree with: 0)
  }
  if (fallback) sw_count(fallback + f, lane, mine >= 0 && fell);
}

extern "C" int mmego_blend_rot(void* stream, const float* src, long nrows, int J, const float* q, int NQ, const float* Rh,
                               const long long* cov_off, const int* cov_row, const float* cov_w, long F, const int* bones,
                               const int* rot_idx, const float* body, int NB, float* dst, long ldd, float* quat, float* spread,
                               float* rot_spread, int* fallback) {
  MMEGO_REQUIRE(src && q && Rh && cov_off && cov_row && cov_w && dst && quat && bones && rot_idx && body);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && nrows >= 0 && nrows < (1L << 31) && J >= 2 && J <= BR_MAX_J && ldd >= 3 * J);
  MMEGO_REQUIRE(NB >= 1 && NB <= J - 1 && NQ >= 1 && NQ <= 64 && ((size_t)quat & 15) == 0);
  hipLaunchKernelGGL(blend_rot_kernel, dim3((unsigned)cdiv(F, BR_WAVES)), dim3(64 * BR_WAVES), 0, (hipStream_t)stream, src, nrows, J, q,
                     NQ, Rh, cov_off, cov_row, cov_w, F, bones, rot_idx, body, NB, dst, ldd, quat, spread, rot_spread, fallback);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
