// upper_front_eval with fp32 operands (front_eval.h has the kernel): v_mfma_f32_16x16x4_f32, operands fetched with one ds_read_b128
// per four MFMA steps through a k-permutation shared by both operands (lane (r, q) holds k = 16 c + 4 q + s at step s of chunk c);
// row strides K + 4 floats keep those 16-byte reads conflict-free.  Accumulators in VGPRs and NaNs honoured (build.py's FILE_FLAGS).
#include "common.h"

struct FrF32 {
  typedef float elem;
  typedef f32x4 vec;
  static constexpr bool W_IN_SH = true;
  static __device__ __forceinline__ float* weights(float* sh, float*) { return sh; }
  static __device__ __forceinline__ float store(float x) { return x; }
  static __device__ __forceinline__ f32x4 cols(float a, float b, float c, float d) { return f32x4{a, b, c, d}; }
  template <int NCT>
  static __device__ __forceinline__ void mma(const f32x4 (&w)[NCT], f32x4 x, f32x4 (&acc)[NCT]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[ct][s], x[s], acc[ct], 0, 0, 0);
  }
  static __device__ __forceinline__ float relu(float x) { return fmaxf(x, 0.f); }
  template <int NCT>
  static __device__ __forceinline__ void act(const f32x4 (&acc)[NCT], f32x4 (&out)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[ct][i] = relu(acc[ct][i]);
  }
};

#define FRONT_EVAL_KERNEL upper_front_eval_kernel
#define FRONT_EVAL_OPERANDS FrF32
#include "front_eval.h"

extern "C" int mmego_upper_front_eval(void* stream, float* x, const float* x_src, const float* R, const float* t, long F, int N,
                                      const float* const* w, float eps, float* vec, float* attn) {
  // 37 KB of LDS: four workgroups per CU
  return upper_front_eval_launch(upper_front_eval_kernel, 1024, stream, x, x_src, R, t, F, N, w, eps, vec, attn);
}
