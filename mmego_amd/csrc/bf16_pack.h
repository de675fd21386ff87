// bf16 as the kernels carry it: raw bits, MFMA operand vectors and the fp32 -> bf16 conversions.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned short bf16_t;   // raw bf16 bits (the C ABI carries them as unsigned short)
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8;   // one lane's operand of a 16-k bf16 MFMA step
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));               // the same 16 bytes as they travel

// round to nearest even, NaN stays NaN: v_cvt_pk_bf16_f32 on gfx950 -- one instruction for two values (the integer form -- add
// 0x7fff + lsb, shift, a branch for NaN -- was five VALU instructions and a branch per value)
__device__ __forceinline__ unsigned int f2bf(float x) { return (unsigned int)__builtin_bit_cast(unsigned short, (__bf16)x); }
// lo in bits 15:0, hi in bits 31:16
__device__ __forceinline__ unsigned int f2bf2(float lo, float hi) {
  typedef float f32x2_ __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned int, __builtin_convertvector((f32x2_){lo, hi}, bf16x2_));
}
