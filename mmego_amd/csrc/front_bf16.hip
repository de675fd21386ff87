// upper_front_eval with bf16 operands (front_eval.h has the kernel; opt-in precision mode, eval forwards: UpperNet.precision = "bf16";
// BASELINE config 5 "bf16 forward / fp32 accumulate"): the (BatchNorm-folded) weights are rounded once while they are staged, every
// activation tile is rounded when it is handed to the next stage, products are exact in fp32 and accumulate in fp32 on
// v_mfma_f32_16x16x16_bf16 (one MFMA per 16 k instead of four 16x16x4 fp32 steps: an eighth of the matrix time).  Transform2H, the
// write-back of the transformed points (Q1), biases, ReLU, scores and the online softmax stay fp32.
// Lane (r, q) of a 16x16x16 MFMA holds k = 4 q .. 4 q + 3 of row / column r: one 8-byte LDS read per operand and 16 k (8-byte aligned
// rows).  With the transposed stages of r06 bias, ReLU and the bf16 rounding happen in registers (before: 36 two-byte LDS stores and the
// reads behind them per slab and wave, a latency chain of six round trips; 591 us at config 5, VALU / LDS issue bound).
#include "common.h"
#include "bf16_pack.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

struct FrBf16 {
  typedef bf16_t elem;
  typedef s16x4 vec;
  static constexpr bool W_IN_SH = false;
  static __device__ __forceinline__ bf16_t* weights(float*, bf16_t* own) { return own; }
  static __device__ __forceinline__ bf16_t store(float x) { return (bf16_t)f2bf(x); }
  static __device__ __forceinline__ s16x4 cols(float a, float b, float c, float d) {
    return __builtin_bit_cast(s16x4, make_uint2(f2bf2(a, b), f2bf2(c, d)));
  }
  template <int NCT>
  static __device__ __forceinline__ void mma(const s16x4 (&w)[NCT], s16x4 x, f32x4 (&acc)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w[ct], x, acc[ct], 0, 0, 0);
  }
  // max(x, 0).  One v_max_f32 only because build.py compiles this file with -fno-honor-nans: otherwise the compiler first canonicalises
  // an MFMA result it cannot prove quiet (a second v_max per value; it rewrites v_med3 the same way).  An inline-asm v_max_f32 is NOT an
  // option: the hazard recogniser does not see an MFMA result being read inside an asm block and leaves out the wait states (measured:
  // results changing from run to run).
  static __device__ __forceinline__ float relu(float x) { return fmaxf(x, 0.f); }
  // relu(D^T) rounded to bf16: accumulator tile ct (lane (point, fq), register i: feature 16 ct + 4 fq + i) IS k block ct of the next
  // stage's B operand
  template <int NCT>
  static __device__ __forceinline__ void act(const f32x4 (&acc)[NCT], s16x4 (&out)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) out[ct] = cols(relu(acc[ct][0]), relu(acc[ct][1]), relu(acc[ct][2]), relu(acc[ct][3]));
  }
};

#ifndef FRONT_BF16_WAVES
#define FRONT_BF16_WAVES 0
#endif
#if FRONT_BF16_WAVES
#define FRONT_EVAL_KERNEL_ATTRS __attribute__((amdgpu_waves_per_eu(FRONT_BF16_WAVES, FRONT_BF16_WAVES)))
#endif
#define FRONT_EVAL_KERNEL upper_front_eval_bf16_kernel
#define FRONT_EVAL_OPERANDS FrBf16
#include "front_eval.h"

extern "C" int mmego_upper_front_eval_bf16(void* stream, float* x, const float* x_src, const float* R, const float* t, long F, int N,
                                      const float* const* w, float eps, float* vec, float* attn) {
  // 23 KB of LDS: four workgroups per CU
  return upper_front_eval_launch(upper_front_eval_bf16_kernel, 1024, stream, x, x_src, R, t, F, N, w, eps, vec, attn);
}
