// Dense inference's causal filter (dense.dense_infer, one_euro=(fc, beta, dc)): the one-euro filter (Casiez et al. 2012) along time over
// every recording's blended frames -- an exponential low-pass whose cutoff rises with the joint's own filtered speed, so it never reads
// a frame ahead of the one it writes.  Unlike every other dense stage this is a RECURSION: frame i needs the state frame i - 1 left, so
// the launch is sequential in time and parallel over the runs (the host cuts [0, F) into maximal stretches of one segment) and the
// joints: one wave per run, lane = joint, the state (xhat, dhat: six doubles) in registers for the whole run.  The dependent chain per
// frame is a square root, a division and a handful of fused multiply-adds in double; the rows' addresses do not depend on the state, so
// the loads are issued OE_AHEAD frames ahead of their use into a register ring (how many of them the compiler's waits leave in flight
// is in NOTES.md); moved's wave sums are taken OE_AHEAD
// frames at a time behind their steps, off the chain.  No LDS, no atomics, a fixed order: two
// launches give the same bits.  A run with run_on == 0 is copied bit for bit.  In the bones form the roots are filtered as joints and
// every bone carries the recursion on its vector child - parent; the filtered vector is set to the body's bone length and laid along
// the kinematic tree (skeleton_walk.h), as smooth.hip's bones form does: the frames stay rigid.  The arithmetic is one_euro_math.h; the
// recipe is the comment of the two entry points in include/mmego_hip.h, tests/one_euro_ref.py restates it in numpy.
#include "common.h"
#include "one_euro_math.h"
#include "skeleton_walk.h"

#define OE_WAVES 4                       // one wave per run, four per workgroup (no barrier: a wave behind R leaves)
#define OE_AHEAD 8                       // frames between a row's load and its use

// Run r's frames [*a, *e), clipped to [0, F): a bad table (the caller answers for it) cannot send a wave outside the rows.
__device__ __forceinline__ void oe_run(const long long* __restrict__ run_off, int r, long F, long* a, long* e) {
  const long long lo = run_off[r], hi = run_off[r + 1];
  *a = lo < 0 ? 0 : (long)lo;
  *e = hi > (long long)F ? F : (long)hi;
}

// The frames [a, e) of a copy run, or the first frame of a filter run: 3 J floats a row bit for bit, moved and fallback 0.
__device__ __forceinline__ void oe_copy(const float* __restrict__ src, long lds, long a, long e, int J, int lane, float* __restrict__ dst,
                                        long ldd, float* __restrict__ moved, int* __restrict__ fallback) {
  for (long f = a; f < e; ++f) {
    for (int c = lane; c < 3 * J; c += 64) dst[f * ldd + c] = src[f * lds + c];
    if (moved && lane == 0) moved[f] = 0.0f;
    if (fallback && lane == 0) fallback[f] = 0;
  }
}

// moved of the frames i .. i + OE_AHEAD - 1 of a run of n frames (moved: the run's first frame) from every lane's share sq: the wave sums
// of OE_AHEAD frames taken TOGETHER behind their steps -- independent butterflies that overlap, where one sum per step would put its
// six dependent shuffles into every step of the recursion.  Every lane of the wave has to call this.
__device__ __forceinline__ void oe_moved(const double* sq, long i, long n, int J, int lane, float* __restrict__ moved) {
  double q[OE_AHEAD];
#pragma unroll
  for (int k = 0; k < OE_AHEAD; ++k) q[k] = sq[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {     // wave_sum_d's butterfly, the same order of additions, OE_AHEAD sums abreast
#pragma unroll
    for (int k = 0; k < OE_AHEAD; ++k) q[k] += __shfl_xor(q[k], o, 64);
  }
#pragma unroll
  for (int k = 0; k < OE_AHEAD; ++k)
    if (lane == 0 && i + k < n) moved[i + k] = sm_moved(q[k], 3 * J);
}

__global__ __launch_bounds__(64 * OE_WAVES) void one_euro_kernel(const float* __restrict__ src, long lds, long F, int J,
                                                                const long long* __restrict__ run_off, const int* __restrict__ run_on,
                                                                int R, double fc, double beta, double ad, float* __restrict__ dst,
                                                                long ldd, float* __restrict__ moved) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * OE_WAVES + wave;
  if (r >= R) return;
  long a, e;
  oe_run(run_off, r, F, &a, &e);
  if (a >= e) return;
  const bool on = run_on[r] != 0;
  oe_copy(src, lds, a, on ? a + 1 : e, J, lane, dst, ldd, moved, nullptr);
  if (!on) return;
  const bool joint = lane < J;
  const int j = joint ? lane : 0;        // (the lanes behind the row re-read joint 0 and store nothing)
  const long n = e - a;
  const float* __restrict__ x = src + a * lds + 3 * j;
  float* __restrict__ y = dst + a * ldd + 3 * j;
  double xhat[3] = {(double)x[0], (double)x[1], (double)x[2]}, dhat[3] = {0.0, 0.0, 0.0};
  float ring[OE_AHEAD][3];               // slot k holds frame i + k of the unrolled loop below; behind the run: its last frame again
#pragma unroll
  for (int k = 0; k < OE_AHEAD; ++k) {
    const long g = 1 + k < n ? 1 + k : n - 1;
    ring[k][0] = x[g * lds], ring[k][1] = x[g * lds + 1], ring[k][2] = x[g * lds + 2];
  }
  for (long i = 1; i < n; i += OE_AHEAD) {
    double sq[OE_AHEAD];                 // this lane's share of moved, frame i + k
#pragma unroll
    for (int k = 0; k < OE_AHEAD; ++k) sq[k] = 0.0;
#pragma unroll
    for (int k = 0; k < OE_AHEAD; ++k) {
      const long g = i + k;
      if (g >= n) break;                 // (the same in every lane)
      const double xi[3] = {(double)ring[k][0], (double)ring[k][1], (double)ring[k][2]};
      const long h = g + OE_AHEAD < n ? g + OE_AHEAD : n - 1;
      ring[k][0] = x[h * lds], ring[k][1] = x[h * lds + 1], ring[k][2] = x[h * lds + 2];
      oe_step(xi, fc, beta, ad, xhat, dhat);
      if (joint) y[g * ldd] = (float)xhat[0], y[g * ldd + 1] = (float)xhat[1], y[g * ldd + 2] = (float)xhat[2];
      const double m0 = xhat[0] - xi[0], m1 = xhat[1] - xi[1], m2 = xhat[2] - xi[2];
      sq[k] = joint ? m0 * m0 + m1 * m1 + m2 * m2 : 0.0;
    }
    if (moved) oe_moved(sq, i, n, J, lane, moved + a);
  }
}

__global__ __launch_bounds__(64 * OE_WAVES) void one_euro_bones_kernel(const float* __restrict__ src, long lds, long F, int J,
                                                                      const long long* __restrict__ run_off,
                                                                      const int* __restrict__ run_on, int R, double fc, double beta,
                                                                      double ad, const int* __restrict__ bones,
                                                                      const float* __restrict__ bone_len, int NB, float* __restrict__ dst,
                                                                      long ldd, float* __restrict__ moved, int* __restrict__ fallback) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * OE_WAVES + wave;
  if (r >= R) return;
  long a, e;
  oe_run(run_off, r, F, &a, &e);
  if (a >= e) return;
  const bool on = run_on[r] != 0;
  oe_copy(src, lds, a, on ? a + 1 : e, J, lane, dst, ldd, moved, fallback);
  if (!on) return;
  const bool joint = lane < J;
  const int j = joint ? lane : 0;        // (the lanes behind the row re-read joint 0 and store nothing)
  int mine, parent;                      // this lane's bone: the one whose child it is
  sw_lane_bone(bones, NB, J, lane, &mine, &parent);
  const int p = mine >= 0 ? parent : j;  // (a root reads its own joint twice: its vector is never used)
  const double L = mine >= 0 ? (double)bone_len[mine] : 0.0;
  const long n = e - a;
  const float* __restrict__ xc = src + a * lds + 3 * j;
  const float* __restrict__ xp = src + a * lds + 3 * p;
  // the state: a root's position, as mmego_one_euro keeps it; a bone's vector child - parent, unnormalised
  double st[3] = {(double)xc[0], (double)xc[1], (double)xc[2]}, dhat[3] = {0.0, 0.0, 0.0};
  if (mine >= 0) {
    const float c0[3] = {xc[0], xc[1], xc[2]}, p0[3] = {xp[0], xp[1], xp[2]};
    oe_bone_vector(c0, p0, st);
  }
  float ring[OE_AHEAD][6];               // slot k: the child's and the parent's floats of frame i + k
#pragma unroll
  for (int k = 0; k < OE_AHEAD; ++k) {
    const long g = 1 + k < n ? 1 + k : n - 1;
    for (int t = 0; t < 3; ++t) ring[k][t] = xc[g * lds + t], ring[k][3 + t] = xp[g * lds + t];
  }
  for (long i = 1; i < n; i += OE_AHEAD) {
    double sq[OE_AHEAD];                 // this lane's share of moved, frame i + k
#pragma unroll
    for (int k = 0; k < OE_AHEAD; ++k) sq[k] = 0.0;
#pragma unroll
    for (int k = 0; k < OE_AHEAD; ++k) {
      const long g = i + k;
      if (g >= n) break;                 // (the same in every lane)
      const float c[3] = {ring[k][0], ring[k][1], ring[k][2]}, q[3] = {ring[k][3], ring[k][4], ring[k][5]};
      const long h = g + OE_AHEAD < n ? g + OE_AHEAD : n - 1;
      for (int t = 0; t < 3; ++t) ring[k][t] = xc[h * lds + t], ring[k][3 + t] = xp[h * lds + t];
      double u[3] = {0.0, 0.0, 0.0}, pos[3] = {0.0, 0.0, 0.0};
      int fell = 0;
      if (mine >= 0) {
        double v[3];
        oe_bone_vector(c, q, v);
        fell = oe_bone_step(v, fc, beta, ad, L, st, dhat, u);
      } else {
        const double xi[3] = {(double)c[0], (double)c[1], (double)c[2]};
        oe_step(xi, fc, beta, ad, st, dhat);
        pos[0] = st[0], pos[1] = st[1], pos[2] = st[2];
      }
      sw_walk(bones, NB, J, mine, L, u, pos);
      sw_store(dst + (a + g) * ldd, J, lane, pos);
      const double m0 = pos[0] - (double)c[0], m1 = pos[1] - (double)c[1], m2 = pos[2] - (double)c[2];
      sq[k] = joint ? m0 * m0 + m1 * m1 + m2 * m2 : 0.0;
      if (fallback) sw_count(fallback + a + g, lane, mine >= 0 && fell);
    }
    if (moved) oe_moved(sq, i, n, J, lane, moved + a);
  }
}

// true where the F rows of n columns at a (row stride lda) and at b (row stride ldb) share a byte
static bool oe_rows_overlap(const float* a, long lda, const float* b, long ldb, long F, int n) {
  const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + (F - 1) * lda + n), b0 = (uintptr_t)b, b1 = (uintptr_t)(b + (F - 1) * ldb + n);
  return a0 < b1 && b0 < a1;
}

static bool oe_params_ok(double fc, double beta, double dc) {
  return std::isfinite(fc) && fc > 0.0 && std::isfinite(beta) && beta >= 0.0 && std::isfinite(dc) && dc > 0.0;
}

extern "C" int mmego_one_euro(void* stream, const float* src, long lds, long F, int J, const long long* run_off, const int* run_on, int R,
                              double fc, double beta, double dc, float* dst, long ldd, float* moved) {
  MMEGO_REQUIRE(src && run_off && run_on && dst);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && J >= 1 && J <= BB_MAX_J && lds >= 3 * J && ldd >= 3 * J);
  MMEGO_REQUIRE(R >= 1 && R <= F);
  MMEGO_REQUIRE(oe_params_ok(fc, beta, dc));
  MMEGO_REQUIRE(!oe_rows_overlap(src, lds, dst, ldd, F, 3 * J));
  hipLaunchKernelGGL(one_euro_kernel, dim3((unsigned)cdiv(R, OE_WAVES)), dim3(64 * OE_WAVES), 0, (hipStream_t)stream, src, lds, F, J,
                     run_off, run_on, R, fc, beta, oe_alpha(dc), dst, ldd, moved);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_one_euro_bones(void* stream, const float* src, long lds, long F, int J, const long long* run_off, const int* run_on,
                                    int R, double fc, double beta, double dc, const int* bones, const float* bone_len, int NB, float* dst,
                                    long ldd, float* moved, int* fallback) {
  MMEGO_REQUIRE(src && run_off && run_on && dst);
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && J >= 1 && J <= BB_MAX_J && lds >= 3 * J && ldd >= 3 * J);
  MMEGO_REQUIRE(R >= 1 && R <= F);
  MMEGO_REQUIRE(oe_params_ok(fc, beta, dc));
  MMEGO_REQUIRE(NB >= 0 && NB <= J - 1 && (NB == 0 || (bones && bone_len)));
  MMEGO_REQUIRE(!oe_rows_overlap(src, lds, dst, ldd, F, 3 * J));
  hipLaunchKernelGGL(one_euro_bones_kernel, dim3((unsigned)cdiv(R, OE_WAVES)), dim3(64 * OE_WAVES), 0, (hipStream_t)stream, src, lds, F, J,
                     run_off, run_on, R, fc, beta, oe_alpha(dc), bones, bone_len, NB, dst, ldd, moved, fallback);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
