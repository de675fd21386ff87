// IMU sensor noise and bias on the device (--imu_noise_* / --imu_bias_*; train_step.ImuStep / StageStep, processors._epoch_eval /
// dense_infer): every IMU sample (15 floats: orientation, accelerometer, gyroscope) on its way into IMU_Net perturbed by white noise of
// its own and by an offset that is constant over its window, both drawn from a DEVICE seed word, so that a launch captured into a HIP
// graph draws afresh on every replay once the host has rewritten the word.  One thread per SAMPLE: 15 floats in and 15 out, no LDS, no
// atomics; a wave reads and writes 3840 contiguous bytes.  Every thread of a window derives the window's nine bias draws and its rotation
// again for itself -- a few dozen integer hashes and one sincos beside a launch that is a few microseconds of latency at the training
// shape (10 240 samples, 614 KB) -- so the output is a pure function of (word, ids, input) and two launches with one word give the same
// bytes.  The arithmetic per sample is imu_noise_math.h, the draws are noise_draw.h (the cloud packer's); the recipe is the comment of the
// entry point in include/mmego_hip.h, tests/imu_noise_ref.py restates it in numpy.
#include "common.h"
#include "noise_draw.h"
#include "imu_noise_math.h"

#define IN_SALT_SAMPLE 0x494D554Eu       // "IMUN": the launch's white-noise stream under the seed word
#define IN_SALT_WINDOW 0x494D5542u       // "IMUB": the launch's bias stream

struct InSigmas {                        // rotations in radians, the additive groups in the recordings' units
  double noise_rot, noise_acc, noise_gyro, bias_rot, bias_acc, bias_gyro;
};

static inline int in_blocks(long total) {                            // (the element-wise launchers' cap: 2048 workgroups, strided beyond)
  long b = (total + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// out may be imu exactly: a thread reads its whole sample before it writes it, and no other thread touches the sample (the pointers
// carry no __restrict__).  A group both of whose sigmas are 0 is copied.
__global__ __launch_bounds__(256) void imu_jitter_kernel(const float* imu, long total, long TS, int S, InSigmas sg,
                                                         const long long* __restrict__ seed_word, const long long* __restrict__ row_ids,
                                                         const long long* __restrict__ win_ids, float* out) {
  const unsigned K_s = dropout_key((unsigned long long)seed_word[0], IN_SALT_SAMPLE);
  const unsigned K_w = dropout_key((unsigned long long)seed_word[0], IN_SALT_WINDOW);
  const bool rot = sg.noise_rot != 0.0 || sg.bias_rot != 0.0;
  const bool acc = sg.noise_acc != 0.0 || sg.bias_acc != 0.0, gyro = sg.noise_gyro != 0.0 || sg.bias_gyro != 0.0;
  const long step = (long)gridDim.x * 256;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total; j += step) {
    const long i = j / S, w = j / TS;                                // the sample's row and window
    const long long d = row_ids ? row_ids[i] : (long long)i;
    const long long u = win_ids ? win_ids[w] : (long long)w;
    const unsigned e = (unsigned)d * (unsigned)S + (unsigned)(j - i * S);      // the low 32 bits of d S + s
    const unsigned b_s = hash32(K_s ^ hash32(e)), b_w = hash32(K_w ^ hash32((unsigned)u));
    float x[IN_CH], y[IN_CH];
#pragma unroll
    for (int k = 0; k < IN_CH; ++k) y[k] = x[k] = imu[j * IN_CH + k];
    if (rot) {
      // (a draw whose sigma is 0 is never used: it is not made)
      float zs[3] = {0.f, 0.f, 0.f}, zw[3] = {0.f, 0.f, 0.f};
      if (sg.noise_rot != 0.0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) zs[k] = fp_noise_z(b_s, k);
      }
      if (sg.bias_rot != 0.0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) zw[k] = fp_noise_z(b_w, k);
      }
      double E[9];
      in_rotation(sg.noise_rot, zs, sg.bias_rot, zw, E);
      pn_compose(E, x, y);
    }
    if (acc) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        y[9 + k] = in_add(x[9 + k], sg.bias_acc, sg.bias_acc != 0.0 ? fp_noise_z(b_w, 3 + k) : 0.f, sg.noise_acc,
                          sg.noise_acc != 0.0 ? fp_noise_z(b_s, 3 + k) : 0.f);
    }
    if (gyro) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        y[12 + k] = in_add(x[12 + k], sg.bias_gyro, sg.bias_gyro != 0.0 ? fp_noise_z(b_w, 6 + k) : 0.f, sg.noise_gyro,
                           sg.noise_gyro != 0.0 ? fp_noise_z(b_s, 6 + k) : 0.f);
    }
#pragma unroll
    for (int k = 0; k < IN_CH; ++k) out[j * IN_CH + k] = y[k];
  }
}

// [a, a + n) and [b, b + n) share a byte
static inline bool in_overlap(const void* a, const void* b, size_t n) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + n && b0 < a0 + n;
}

static inline bool in_sigma_ok(double s) { return s >= 0.0 && s < (double)INFINITY; }      // (false for a NaN as well)

extern "C" int mmego_imu_jitter(void* stream, const float* imu, long n_rows, int T, int S, double noise_rot_deg, double noise_acc,
                                double noise_gyro, double bias_rot_deg, double bias_acc, double bias_gyro, const long long* seed_word,
                                const long long* row_ids, const long long* win_ids, float* out) {
  MMEGO_REQUIRE(imu && out && seed_word && n_rows >= 1 && T >= 1 && S >= 1 && n_rows % T == 0);
  MMEGO_REQUIRE(n_rows < (1L << 40) / S);                           // (samples and their float offsets stay far inside a long)
  MMEGO_REQUIRE(in_sigma_ok(noise_rot_deg) && in_sigma_ok(noise_acc) && in_sigma_ok(noise_gyro) && in_sigma_ok(bias_rot_deg) &&
                in_sigma_ok(bias_acc) && in_sigma_ok(bias_gyro));
  MMEGO_REQUIRE(noise_rot_deg != 0.0 || noise_acc != 0.0 || noise_gyro != 0.0 || bias_rot_deg != 0.0 || bias_acc != 0.0 ||
                bias_gyro != 0.0);                                  // nothing to draw
  MMEGO_REQUIRE((((uintptr_t)seed_word) & 7) == 0 && (((uintptr_t)row_ids) & 7) == 0 && (((uintptr_t)win_ids) & 7) == 0);
  const long total = n_rows * S;
  // in place means the SAME samples: the output is its input exactly, or shares no byte with it
  MMEGO_REQUIRE(out == imu || !in_overlap(out, imu, (size_t)total * IN_CH * sizeof(float)));
  const InSigmas sg = {noise_rot_deg * PN_RAD_PER_DEG, noise_acc, noise_gyro, bias_rot_deg * PN_RAD_PER_DEG, bias_acc, bias_gyro};
  hipLaunchKernelGGL(imu_jitter_kernel, dim3(in_blocks(total)), dim3(256), 0, (hipStream_t)stream, imu, total, (long)T * S, S, sg,
                     seed_word, row_ids, win_ids, out);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
