// mlp3_eval with bf16 operands (mlp3_eval.h has the kernel; opt-in precision mode of eval forwards: LowerNet.precision = "bf16" routes
// BasePointNet through it; BASELINE config 5 "bf16 forward / fp32 accumulate"): operands rounded to bf16 -- the folded weights once
// while they are staged, every stage's input when it is written -- products exact in fp32, fp32 accumulation on
// v_mfma_f32_32x32x16_bf16: a lane's operand is 16 bytes of row lane % 32 (k = 8 (lane / 32) .. + 8 of a 16-k step), one ds_read_b128
// per operand and 16 k where the fp32 kernel issues sixteen ds_read_b32 and eight MFMAs.  Biases, ReLU and the output stay fp32.
#include "common.h"
#include "bf16_pack.h"

struct M3Bf16 {
  typedef bf16_t elem;
  // row strides of tiles with k <= 32: 80 B, k <= 64: 144 B -- 16-byte aligned rows on distinct bank groups
  static constexpr int S32 = 40, S64 = 72, KSTEP = 16;
  static __device__ __forceinline__ bf16_t store(float x) { return (bf16_t)f2bf(x); }
  static __device__ __forceinline__ f32x16 tile(const bf16_t* A, int as, const bf16_t* W, int ws, int K, int lane) {
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc = {0};
    const bf16_t* ap = A + r * as + 8 * h;
    const bf16_t* wp = W + r * ws + 8 * h;
    for (int k = 0; k < K; k += 16)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(ap + k), *reinterpret_cast<const bf16x8*>(wp + k), acc, 0, 0, 0);
    return acc;
  }
};

#define MLP3_EVAL_KERNEL mlp3_eval_bf16_kernel
#define MLP3_EVAL_OPERANDS M3Bf16
#include "mlp3_eval.h"

extern "C" int mmego_mlp3_eval_bf16(void* stream, const float* X, long ldx, long rows, int Cin, const float* W1, const float* b1, int C1,
                               const float* W2, const float* b2, int C2, const float* W3, const float* b3, int C3, float* Y,
                               long ldy, const float* const* bn, float eps, int pre) {
  // 32 KB of LDS: four workgroups per CU
  return mlp3_eval_launch(mlp3_eval_bf16_kernel, 4096, stream, X, ldx, rows, Cin, W1, b1, C1, W2, b2, C2, W3, b3, C3, Y, ldy, bn, eps, pre);
}
