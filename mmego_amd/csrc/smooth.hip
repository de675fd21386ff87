// Dense inference's last stage (dense.dense_infer, smooth=(H, order, taper)): a zero-phase local-polynomial filter along time over
// every recording's stitched frames -- frame f's row becomes the value at f of the weighted least-squares polynomial of degree <= 2
// through the rows f-H .. f+H of its own segment.  In the column form every column is filtered on its own; in the bones form the roots
// are, and every bone's DIRECTION is filtered, set to the body's bone length and laid along the kinematic tree, as blend_bones.hip
// blends: the frames stay rigid skeletons.  Like blend.hip a memory-bound gather of at most 63 rows of at most 64 floats: one wave per
// frame, no barrier, no LDS, no atomics, every sum in a fixed order (two launches give the same bits), double inside, one float store.
// A wave works in two roles.  First lane = TAP: lane l reads seg[f + l - H], one ballot gives the valid taps (the same mask in every
// lane), the moments are wave sums, so every lane holds the first row A of the inverse moment matrix and lane l the coefficient of its
// own tap.  Then lane = COLUMN (or JOINT): the valid taps are walked in ascending order, the tap's coefficient handed over by a double
// shuffle, its row one coalesced read.  The taper is a table the host makes: the kernel knows none.  The arithmetic is smooth_math.h;
// the recipe is the comment of the two entry points in include/mmego_hip.h, tests/smooth_ref.py restates it in numpy by another route.
// The rotation form (mmego_smooth_rot, under blend_space="rot") filters every bone's world ROTATION: the same taps and coefficients, per
// lane nine accumulators of S = sum_k c_k A_k from one 16-byte quaternion load per tap, then mmego_blend_rot's projection onto the
// rotations (rot_blend_math.h, quat_eig.h) and its walk; rot_smooth_math.h holds what is new, tests/rot_smooth_ref.py restates it.
#include "common.h"
#include "smooth_math.h"
#include "rot_smooth_math.h"
#include "skeleton_walk.h"

#define SM_WAVES 4                       // one wave per output frame, four per workgroup (no barrier: a wave behind F leaves)

// Lane = tap k = lane - H of frame f: -> c_k in the lane of every valid tap (0 elsewhere) and the ballot of the valid taps, bit l for
// tap l - H.  Fewer than two valid taps: nothing is summed, the caller copies the row.  Every lane of the wave has to call this.
__device__ __forceinline__ double sm_wave_coefs(const int* __restrict__ seg, const float* __restrict__ w, long F, long f, int H, int D,
                                                int lane, unsigned long long* mask) {
  const int k = lane - H;
  const long g = f + k;
  const int s0 = seg[f];
  const bool valid = lane <= 2 * H && g >= 0 && g < F && s0 >= 0 && seg[g] == s0;
  const unsigned long long m = __ballot(valid);
  *mask = m;
  const int n = __popcll(m);
  if (n <= 1) return 0.0;
  const int deg = sm_degree(D, n);
  const double wk = valid ? (double)w[lane] : 0.0;
  double t[5], S[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, A[3];
  sm_tap_moments(wk, k, t);
  for (int i = 0; i <= 2 * deg; ++i) S[i] = wave_sum_d(t[i]);      // (deg is the same in every lane)
  sm_first_row(S, deg, A);
  return sm_coef(A, wk, k);
}

__global__ __launch_bounds__(64 * SM_WAVES) void smooth_frames_kernel(const float* __restrict__ src, long lds, long F, int C,
                                                                     const int* __restrict__ seg, const float* __restrict__ w, int H, int D,
                                                                     float* __restrict__ dst, long ldd, float* __restrict__ moved) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * SM_WAVES + wave;
  if (f >= F) return;
  unsigned long long mask;
  const double ck = sm_wave_coefs(seg, w, F, f, H, D, lane, &mask);
  const bool col = lane < C;
  const int c = col ? lane : 0;          // (the lanes behind the row re-read column 0 and store nothing)
  const float own = src[f * lds + c];
  if (__popcll(mask) <= 1) {             // outside every segment, or alone in its own: the row itself
    if (col) dst[f * ldd + lane] = own;
    if (moved && lane == 0) moved[f] = 0.0f;
    return;
  }
  double y = 0.0;
  for (int t = 0; t <= 2 * H; ++t) {     // (the mask is the same in every lane: the whole wave shuffles or none of it)
    if (!((mask >> t) & 1)) continue;
    const double ct = shfl_d(ck, t);
    y = sm_acc(y, ct, src[(f + t - H) * lds + c]);
  }
  if (col) dst[f * ldd + lane] = (float)y;
  if (moved) {
    const double d = y - (double)own;
    const double q = wave_sum_d(col ? d * d : 0.0);
    if (lane == 0) moved[f] = sm_moved(q, C);
  }
}

__global__ __launch_bounds__(64 * SM_WAVES) void smooth_bones_kernel(const float* __restrict__ src, long lds, long F, int J,
                                                                    const int* __restrict__ seg, const float* __restrict__ w, int H, int D,
                                                                    const int* __restrict__ bones, const float* __restrict__ bone_len,
                                                                    int NB, float* __restrict__ dst, long ldd, float* __restrict__ moved,
                                                                    int* __restrict__ fallback) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * SM_WAVES + wave;
  if (f >= F) return;
  unsigned long long mask;
  const double ck = sm_wave_coefs(seg, w, F, f, H, D, lane, &mask);
  const bool joint = lane < J;
  const int j = joint ? lane : 0;        // (the lanes behind the row re-read joint 0 and store nothing)
  const float* own = src + f * lds;
  if (__popcll(mask) <= 1) {             // outside every segment, or alone in its own: the row itself
    if (joint)
      for (int i = 0; i < 3; ++i) dst[f * ldd + 3 * lane + i] = own[3 * j + i];
    if (moved && lane == 0) moved[f] = 0.0f;
    if (fallback && lane == 0) fallback[f] = 0;
    return;
  }
  int mine, parent;                      // this lane's bone: the one whose child it is
  sw_lane_bone(bones, NB, J, lane, &mine, &parent);
  // a root: its three columns, as mmego_smooth_frames sums them; a bone's child: s = sum_k c_k (x_child - x_parent)
  double s[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, pos[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t <= 2 * H; ++t) {     // (the mask is the same in every lane: the whole wave shuffles or none of it)
    if (!((mask >> t) & 1)) continue;
    const double ct = shfl_d(ck, t);
    const float* x = src + (f + t - H) * lds;
    if (mine >= 0) {
      for (int i = 0; i < 3; ++i) s[i] += ct * ((double)x[3 * j + i] - (double)x[3 * parent + i]);
    } else {
      for (int i = 0; i < 3; ++i) pos[i] = sm_acc(pos[i], ct, x[3 * j + i]);
    }
  }
  const double L = mine >= 0 ? (double)bone_len[mine] : 0.0;
  int fell = 0;
  if (mine >= 0) {
    const double best[3] = {(double)own[3 * j] - (double)own[3 * parent], (double)own[3 * j + 1] - (double)own[3 * parent + 1],
                            (double)own[3 * j + 2] - (double)own[3 * parent + 2]};     // the frame's own bone (tap 0): the fallback
    fell = bb_direction(s, best, 1.0, L, u);                                            // (the coefficients sum to 1)
  }
  sw_walk(bones, NB, J, mine, L, u, pos);
  sw_store(dst + f * ldd, J, lane, pos);
  if (moved) {
    double q = 0.0;
    if (joint)
      for (int i = 0; i < 3; ++i) {
        const double d = pos[i] - (double)own[3 * j + i];
        q += d * d;
      }
    q = wave_sum_d(q);
    if (lane == 0) moved[f] = sm_moved(q, 3 * J);
  }
  if (fallback) sw_count(fallback + f, lane, mine >= 0 && fell);
}

__global__ __launch_bounds__(64 * SM_WAVES) void smooth_rot_kernel(const float* __restrict__ src, long lds, long F, int J,
                                                                  const float* __restrict__ quat, int NB, const int* __restrict__ seg,
                                                                  const float* __restrict__ w, int H, int D,
                                                                  const int* __restrict__ bones, const float* __restrict__ body,
                                                                  float* __restrict__ dst, long ldd, float* __restrict__ quat_out,
                                                                  float* __restrict__ moved, float* __restrict__ rot_moved,
                                                                  int* __restrict__ fallback) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * SM_WAVES + wave;
  if (f >= F) return;
  unsigned long long mask;
  const double ck = sm_wave_coefs(seg, w, F, f, H, D, lane, &mask);
  const bool joint = lane < J;
  const int j = joint ? lane : 0;        // (the lanes behind the row re-read joint 0 and store nothing)
  const float* own = src + f * lds;
  const float4* __restrict__ q4 = reinterpret_cast<const float4*>(quat);
  float4* __restrict__ q4_out = reinterpret_cast<float4*>(quat_out);
  int mine, parent;                      // this lane's bone: the one whose child it is
  sw_lane_bone(bones, NB, J, lane, &mine, &parent);
  if (__popcll(mask) <= 1) {             // outside every segment, or alone in its own: the row and its quaternions themselves
    if (joint)
      for (int i = 0; i < 3; ++i) dst[f * ldd + 3 * lane + i] = own[3 * j + i];
    if (mine >= 0) q4_out[f * NB + mine] = q4[f * NB + mine];
    if (moved && lane == 0) moved[f] = 0.0f;
    if (rot_moved && lane == 0) rot_moved[f] = 0.0f;
    if (fallback && lane == 0) fallback[f] = 0;
    return;
  }
  // a root: its three columns, as mmego_smooth_frames sums them; a bone's child: S = sum_k c_k A_k of the bone's rotations
  double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, W = 0.0, pos[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t <= 2 * H; ++t) {     // (the mask is the same in every lane: the whole wave shuffles or none of it)
    if (!((mask >> t) & 1)) continue;
    const double ct = shfl_d(ck, t);
    const long g = f + t - H;
    if (mine >= 0) {
      const float4 v = q4[g * NB + mine];
      double A[9];
      rs_matrix(v.x, v.y, v.z, v.w, A);
      rs_acc(S, &W, ct, A);
    } else {
      const float* x = src + g * lds;
      for (int i = 0; i < 3; ++i) pos[i] = sm_acc(pos[i], ct, x[3 * j + i]);
    }
  }
  double qm[4] = {0.0, 0.0, 0.0, 0.0}, lay[3] = {0.0, 0.0, 0.0}, theta = 0.0;
  int fell = 0;
  if (mine >= 0) {
    const float4 v = q4[f * NB + mine];  // the frame's own rotation (tap 0): the fallback, and what rot_moved is measured from
    double A0[9], Q[9];
    rs_matrix(v.x, v.y, v.z, v.w, A0);
    fell = rs_mean(S, A0, W, qm, Q, &theta);
    br_lay(Q, body + 3 * mine, lay);
  }
  sw_walk(bones, NB, J, mine, 1.0, lay, pos);        // (1.0 * x rounds to x, and fma(1.0, x, p) as p + x does)
  sw_store(dst + f * ldd, J, lane, pos);
  if (mine >= 0) q4_out[f * NB + mine] = make_float4((float)qm[0], (float)qm[1], (float)qm[2], (float)qm[3]);
  if (moved) {
    double q = 0.0;
    if (joint)
      for (int i = 0; i < 3; ++i) {
        const double d = pos[i] - (double)own[3 * j + i];
        q += d * d;
      }
    q = wave_sum_d(q);
    if (lane == 0) moved[f] = sm_moved(q, 3 * J);
  }
  if (rot_moved) {
    const double s = wave_sum_d(mine >= 0 ? theta * theta : 0.0);
    if (lane == 0) rot_moved[f] = rs_rot_moved(s, NB);
  }
  if (fallback) sw_count(fallback + f, lane, mine >= 0 && fell);
}

// true where the F rows of n columns at a (row stride lda) and at b (row stride ldb) share a byte
static bool sm_rows_overlap(const float* a, long lda, const float* b, long ldb, long F, int n) {
  const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + (F - 1) * lda + n), b0 = (uintptr_t)b, b1 = (uintptr_t)(b + (F - 1) * ldb + n);
  return a0 < b1 && b0 < a1;
}

extern "C" int mmego_smooth_frames(void* stream, const float* src, long lds, long F, int C, const int* seg, const float* w, int H, int D,
                                   float* dst, long ldd, float* moved) {
  MMEGO_REQUIRE(src && seg && w && dst);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && C >= 1 && C <= SM_MAX_C && lds >= C && ldd >= C);
  MMEGO_REQUIRE(H >= 1 && H <= SM_MAX_H && D >= 0 && D <= 2);
  MMEGO_REQUIRE(!moved || C % 3 == 0);
  MMEGO_REQUIRE(!sm_rows_overlap(src, lds, dst, ldd, F, C));
  hipLaunchKernelGGL(smooth_frames_kernel, dim3((unsigned)cdiv(F, SM_WAVES)), dim3(64 * SM_WAVES), 0, (hipStream_t)stream, src, lds, F, C,
                     seg, w, H, D, dst, ldd, moved);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_smooth_bones(void* stream, const float* src, long lds, long F, int J, const int* seg, const float* w, int H, int D,
                                  const int* bones, const float* bone_len, int NB, float* dst, long ldd, float* moved, int* fallback) {
  MMEGO_REQUIRE(src && seg && w && dst);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && J >= 1 && J <= BB_MAX_J && lds >= 3 * J && ldd >= 3 * J);
  MMEGO_REQUIRE(H >= 1 && H <= SM_MAX_H && D >= 0 && D <= 2);
  MMEGO_REQUIRE(NB >= 0 && NB <= J - 1 && (NB == 0 || (bones && bone_len)));
  MMEGO_REQUIRE(!sm_rows_overlap(src, lds, dst, ldd, F, 3 * J));
  hipLaunchKernelGGL(smooth_bones_kernel, dim3((unsigned)cdiv(F, SM_WAVES)), dim3(64 * SM_WAVES), 0, (hipStream_t)stream, src, lds, F, J,
                     seg, w, H, D, bones, bone_len, NB, dst, ldd, moved, fallback);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_smooth_rot(void* stream, const float* src, long lds, long F, int J, const float* quat, int NB, const int* seg,
                                const float* w, int H, int D, const int* bones, const float* body, float* dst, long ldd, float* quat_out,
                                float* moved, float* rot_moved, int* fallback) {
  MMEGO_REQUIRE(src && quat && seg && w && bones && body && dst && quat_out);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && J >= 2 && J <= BR_MAX_J && lds >= 3 * J && ldd >= 3 * J);
  MMEGO_REQUIRE(H >= 1 && H <= SM_MAX_H && D >= 0 && D <= 2);
  MMEGO_REQUIRE(NB >= 1 && NB <= J - 1 && ((uintptr_t)quat & 15) == 0 && ((uintptr_t)quat_out & 15) == 0);
  MMEGO_REQUIRE(!sm_rows_overlap(src, lds, dst, ldd, F, 3 * J));
  MMEGO_REQUIRE(!sm_rows_overlap(quat, 4L * NB, quat_out, 4L * NB, F, 4 * NB));
  hipLaunchKernelGGL(smooth_rot_kernel, dim3((unsigned)cdiv(F, SM_WAVES)), dim3(64 * SM_WAVES), 0, (hipStream_t)stream, src, lds, F, J,
                     quat, NB, seg, w, H, D, bones, body, dst, ldd, quat_out, moved, rot_moved, fallback);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
