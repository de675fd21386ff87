// nn.LSTM(dropout=p)'s inverted inter-layer dropout as a streaming launch of its own, for the stacks whose step kernels do not carry it
// (IMU_Net's BiLSTM(512): imu_train.py), and the taking of one dropout seed word per training forward.
//
// The mask of an element is the counter-based hash of common.h (the one mmego_lstm64_forward applies while it stores): nothing but the
// seed word is kept for backward, which runs the same launch on the gradient with the same word and salt.
#include "common.h"

// taken[0] = seed_ctr[0]; seed_ctr[0] takes mmego_inc_i64's next value.  One thread.
__global__ void seed_take_kernel(unsigned long long* seed_ctr, unsigned long long* taken) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long s = seed_ctr[0];
    taken[0] = s;
    seed_ctr[0] = s * 6364136223846793005ULL + 1442695040888963407ULL;
  }
}

// Y[r][c] = X[r][c] * m(r * cols + c), m = 0 or 1/(1-p).  A lane takes four neighbouring elements of a row per iteration (cols % 4 == 0):
//   VEC   -- bases and leading dimensions are multiples of 4 floats: one 16-byte load and one 16-byte store;
//   DENSE -- ldx == ldy == cols: the memory offset IS the logical index (no division by the row length).
// Element indices are 32-bit (rows * cols < 2^32); the key comes from one (uniform, scalar) load of the seed word per wave.
// Y may be X exactly (same base, same leading dimension): a lane reads its four elements before it writes them, and no other lane
// touches them.  Any other overlap of the two operands would be a race between lanes; the entry point refuses it.
template <bool VEC, bool DENSE>
__global__ __launch_bounds__(256) void lstm_dropout_kernel(const float* X, long ldx, float* Y, long ldy, unsigned nquad, unsigned qpr,
                                                           float p, const unsigned long long* seed_word, unsigned salt) {
  const unsigned key = dropout_key(seed_word[0], salt);
  const float keep_scale = 1.0f / (1.0f - p);
  const unsigned step = gridDim.x * blockDim.x;
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += step) {
    const unsigned i = 4u * q;            // logical index of the first of the four
    const float* x;
    float* y;
    if (DENSE) {
      x = X + i;
      y = Y + i;
    } else {
      const unsigned r = q / qpr, c = 4u * (q - r * qpr);
      x = X + ((long)r * ldx + c);
      y = Y + ((long)r * ldy + c);
    }
    f32x4 v;
    if (VEC) {
      v = *(const f32x4*)x;
    } else {
      v = (f32x4){x[0], x[1], x[2], x[3]};
    }
    v.x *= dropout_keep(key, i, p) ? keep_scale : 0.f;
    v.y *= dropout_keep(key, i + 1u, p) ? keep_scale : 0.f;
    v.z *= dropout_keep(key, i + 2u, p) ? keep_scale : 0.f;
    v.w *= dropout_keep(key, i + 3u, p) ? keep_scale : 0.f;
    if (VEC) {
      *(f32x4*)y = v;
    } else {
      y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    }
  }
}

extern "C" int mmego_seed_take(void* stream, unsigned long long* seed_ctr, unsigned long long* taken) {
  MMEGO_REQUIRE(seed_ctr && taken);
  hipLaunchKernelGGL(seed_take_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, seed_ctr, taken);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_lstm_dropout(void* stream, const float* X, long ldx, float* Y, long ldy, long rows, long cols, float p,
                                  const unsigned long long* seed_word, int salt) {
  MMEGO_REQUIRE(X && Y && seed_word && rows > 0 && cols > 0 && cols % 4 == 0 && p > 0.f && p < 1.f);
  MMEGO_REQUIRE(cols < (1L << 32) && rows < (1L << 32) && rows * cols < (1L << 32) && ldx >= cols && ldy >= cols);
  // in place means the SAME elements: X == Y with one leading dimension; operands that overlap in any other way are refused
  const uintptr_t xb = (uintptr_t)X, yb = (uintptr_t)Y;
  const uintptr_t xe = xb + 4 * (uintptr_t)((rows - 1) * ldx + cols), ye = yb + 4 * (uintptr_t)((rows - 1) * ldy + cols);
  MMEGO_REQUIRE((xb == yb && ldx == ldy) || xe <= yb || ye <= xb);
  const unsigned nquad = (unsigned)(rows * cols / 4), qpr = (unsigned)(cols / 4);
  // 2048 workgroups of four waves: 32 waves per CU cover the HBM latency; the stage-1 tensor (10 240 x 1024) is five iterations per lane
  const unsigned nblk = nquad / 256 + (nquad % 256 != 0);
  const dim3 grid(nblk > 2048u ? 2048u : nblk), block(256);
  const bool vec = ((((uintptr_t)X) | ((uintptr_t)Y)) & 15) == 0 && ldx % 4 == 0 && ldy % 4 == 0;
  const bool dense = ldx == cols && ldy == cols;
  const unsigned s = (unsigned)salt;
  if (vec && dense) hipLaunchKernelGGL((lstm_dropout_kernel<true, true>), grid, block, 0, (hipStream_t)stream, X, ldx, Y, ldy, nquad, qpr, p, seed_word, s);
  else if (vec) hipLaunchKernelGGL((lstm_dropout_kernel<true, false>), grid, block, 0, (hipStream_t)stream, X, ldx, Y, ldy, nquad, qpr, p, seed_word, s);
  else if (dense) hipLaunchKernelGGL((lstm_dropout_kernel<false, true>), grid, block, 0, (hipStream_t)stream, X, ldx, Y, ldy, nquad, qpr, p, seed_word, s);
  else hipLaunchKernelGGL((lstm_dropout_kernel<false, false>), grid, block, 0, (hipStream_t)stream, X, ldx, Y, ldy, nquad, qpr, p, seed_word, s);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
