// mlp3_eval with fp32 operands (mlp3_eval.h has the kernel): v_mfma_f32_32x32x2_f32 tiles, k padded to even; operands read from LDS
// as [row][k] with odd row strides (conflict-free), one ds_read_b32 per operand and MFMA.
#include "common.h"

struct M3F32 {
  typedef float elem;
  static constexpr int S32 = 33, S64 = 65, KSTEP = 2;
  static __device__ __forceinline__ float store(float x) { return x; }
  static __device__ __forceinline__ f32x16 tile(const float* A, int as, const float* W, int ws, int K, int lane) {
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc = {0};
    const float* ap = A + r * as + h;
    const float* wp = W + r * ws + h;
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], wp[k], acc, 0, 0, 0);
    return acc;
  }
};

#define MLP3_EVAL_KERNEL mlp3_eval_kernel
#define MLP3_EVAL_OPERANDS M3F32
#include "mlp3_eval.h"

extern "C" int mmego_mlp3_eval(void* stream, const float* X, long ldx, long rows, int Cin, const float* W1, const float* b1, int C1,
                               const float* W2, const float* b2, int C2, const float* W3, const float* b3, int C3, float* Y,
                               long ldy, const float* const* bn, float eps, int pre) {
  // 54 KB of LDS: two workgroups per CU
  return mlp3_eval_launch(mlp3_eval_kernel, 2048, stream, X, ldx, rows, Cin, W1, b1, C1, W2, b2, C2, W3, b3, C3, Y, ldy, bn, eps, pre);
}
