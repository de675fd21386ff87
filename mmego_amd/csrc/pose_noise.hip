// Head-pose noise on the device (--pose_noise_deg, --pose_noise_t; train_step.StageStep, processors._epoch_eval / dense_infer): every
// frame's head pose (R, t) perturbed by a small random rotation and shift drawn from a DEVICE seed word, so that a launch captured into
// a HIP graph draws afresh on every replay once the host has rewritten the word.  One thread per row: a row is 12 floats in and 12
// out, no LDS, no atomics, the draw a pure function of (word, row's draw number): two launches with one word give the same bytes.  The
// arithmetic per row is pose_noise_math.h, the draws are noise_draw.h (the cloud packer's); the recipe is the comment of the entry point
// in include/mmego_hip.h, tests/pose_noise_ref.py restates it in numpy.
#include "common.h"
#include "noise_draw.h"
#include "pose_noise_math.h"

#define PN_SALT 0x504F5345u              // "POSE": the launch's stream under the seed word

static inline int pn_blocks(long total) {                            // (the element-wise launchers' cap: 2048 workgroups, strided beyond)
  long b = (total + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// R_out may be R and t_out may be t exactly: a thread reads its whole row before it writes it, and no other thread touches the row (the
// pointers carry no __restrict__).  sigma_rad == 0 copies R, sigma_t == 0 copies t.
__global__ __launch_bounds__(256) void pose_jitter_kernel(const float* R, const float* t, long n, double sigma_rad, double sigma_t,
                                                          const long long* __restrict__ seed_word, const long long* __restrict__ ids,
                                                          float* R_out, float* t_out) {
  const unsigned K = dropout_key((unsigned long long)seed_word[0], PN_SALT);
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    const long long d = ids ? ids[i] : (long long)i;
    const unsigned b = hash32(K ^ hash32((unsigned)d));
    float r[9], o[9], s[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = R[i * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = t[i * 3 + k];
    if (sigma_rad != 0.0) {
      double E[9];
      pn_rotation(sigma_rad, fp_noise_z(b, 0), fp_noise_z(b, 1), fp_noise_z(b, 2), E);
      pn_compose(E, r, o);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) o[k] = r[k];
    }
    if (sigma_t != 0.0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = pn_shift(s[k], sigma_t, fp_noise_z(b, 3 + k));
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R_out[i * 9 + k] = o[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t_out[i * 3 + k] = s[k];
  }
}

// [a, a + na) and [b, b + nb) share a byte
static inline bool pn_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

extern "C" int mmego_pose_jitter(void* stream, const float* R, const float* t, long n, double sigma_deg, double sigma_t,
                                 const long long* seed_word, const long long* ids, float* R_out, float* t_out) {
  MMEGO_REQUIRE(R && t && R_out && t_out && seed_word && n >= 1 && n < (1L << 40));
  MMEGO_REQUIRE(sigma_deg >= 0.0 && sigma_deg < (double)INFINITY && sigma_t >= 0.0 && sigma_t < (double)INFINITY);      // (false for a NaN as well)
  MMEGO_REQUIRE(sigma_deg != 0.0 || sigma_t != 0.0);                // nothing to draw
  MMEGO_REQUIRE((((uintptr_t)seed_word) & 7) == 0 && (((uintptr_t)ids) & 7) == 0);
  const size_t nR = (size_t)n * 36, nt = (size_t)n * 12;
  // in place means the SAME rows: an output is its own input exactly, or shares no byte with either input or the other output
  MMEGO_REQUIRE(R_out == R || !pn_overlap(R_out, nR, R, nR));
  MMEGO_REQUIRE(t_out == t || !pn_overlap(t_out, nt, t, nt));
  MMEGO_REQUIRE(!pn_overlap(R_out, nR, t_out, nt) && !pn_overlap(R_out, nR, t, nt) && !pn_overlap(t_out, nt, R, nR));
  hipLaunchKernelGGL(pose_jitter_kernel, dim3(pn_blocks(n)), dim3(256), 0, (hipStream_t)stream, R, t, n, sigma_deg * PN_RAD_PER_DEG,
                     sigma_t, seed_word, ids, R_out, t_out);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
