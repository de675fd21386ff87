// Fused multi-tensor Adam over one flat parameter buffer (replaces torch.optim.Adam's foreach chain,
// reference Processor/Train/Train_Upper.py:60,182), plus the dropout mask of the LSTM inter-layer dropout.
// Pure HBM streaming: 16 B/param read (p,g,m,v) + 12 B/param written (p,m,v) = 28 B/param, float4 accesses,
// grid-stride over <= 2048 workgroups.
// Global-norm clipping (FusedAdam(max_grad_norm=...)) is two launches: grad_sqnorm_kernel streams g once more (4 B/param) into one
// fp64 record per workgroup, adam_clipped_kernel sums the records in its prologue (the launch boundary is the only synchronisation:
// no atomics on floats, no workgroup waits for another) and runs the same update on g * cf.
// The skip ranges, the update loop (ADAM_UPDATE_LOOP), the clipped gradient, both steps' prologues and epilogues and the launchers' host
// helpers live in adam_update.h, which optim_ema.hip (the same two steps with a weight average) expands as well.
#include "adam_update.h"

// ---- global-norm clipping ---------------------------------------------------------------------------------------------------
// Pass 1: part[b] = sum over workgroup b's elements of (double)g * (double)g, the skip ranges left out.  Workgroup b reads float4
// b * 256 + lane of every grid-wide stride; GN_UNROLL strides form one trip, whose loads are all issued before the first is
// consumed.  Every lane adds in index order, the wave adds by wave_sum_d, one thread adds the four waves in wave order: the
// order of every addition is a function of n alone, so two runs over the same data give the same bits.
#define GN_UNROLL 4
#define GN_MAX_BLOCKS 1024

__device__ __forceinline__ double sq_accumulate(double acc, float4 x, long i, const AdamSkip& skip) {
  bool skipped = false;
#pragma unroll
  for (int r = 0; r < ADAM_MAX_SKIP; ++r) skipped |= (r < skip.n && i >= skip.lo[r] && i < skip.hi[r]);
  const float* xa = reinterpret_cast<const float*>(&x);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = skipped ? 0.0 : (double)xa[k];      // (a select on the value: the load itself is unconditional)
    acc = fma(d, d, acc);                                // (24-bit x 24-bit: the product is exact in fp64, only the addition rounds)
  }
  return acc;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, long n4, double* __restrict__ part,
                                                          AdamSkip skip) {
  __shared__ double ws[4];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double acc = 0.0;
  for (; i + (GN_UNROLL - 1) * stride < n4; i += GN_UNROLL * stride) {
    float4 x[GN_UNROLL];
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) x[u] = g4[i + u * stride];
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u) acc = sq_accumulate(acc, x[u], i + u * stride, skip);
  }
  for (; i < n4; i += stride) acc = sq_accumulate(acc, g4[i], i, skip);
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// Pass 2: adam_kernel's update on the clipped gradient.  Prologue: EVERY workgroup sums the records of pass 1 in the same fixed
// order (lane j adds records j, j + 256, ...; wave_sum_d; the four waves in wave order), so all of them hold the same bits of
//   norm = sqrt(sum),  c = min(1, max_norm / (norm + 1e-6))  in double,  cf = (float)c.
// A norm that is not finite (an inf or NaN anywhere in the gradient) skips the step: p, m, v and state stay as they are and the
// step count does not advance.  The workgroup that draws the last ticket also keeps the statistics:
// stats[0] this step's norm, [1] sum of the finite norms, [2] their maximum, [3] steps seen, [4] steps with c < 1, [5] steps
// skipped as non-finite, [6..7] reserved.
__global__ __launch_bounds__(256) void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long n4,
                                                           double* state, double lr, double beta1, double beta2d, int* ticket,
                                                           float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                           AdamSkip skip, const double* __restrict__ part, int npart,
                                                           double max_norm, double* stats) {
  ADAM_CLIPPED_PROLOGUE
  if (finite) {
    const double c = sh[4] > 1.0 ? 1.0 : sh[4];
    const float cf = (float)c, step_size = (float)sh[1], bc2_sqrt = (float)sh[2];
    ADAM_UPDATE_LOOP(ADAM_GRAD_CLIPPED)
  }
  ADAM_CLIPPED_EPILOGUE
}

// ---- the plain step (defined after the clipping kernels: it stays the last kernel of the file's code object) ----------------
// state[0] = step count (as double), state[1] = step_size = lr / (1 - b1^t), state[2] = sqrt(1 - b2^t)
// Kept in device memory so that a captured HIP graph replays with the right bias corrections.  The step count advances
// INSIDE the update launch: every workgroup reads state[0] = t-1 when it starts and works with t; the workgroup whose ticket
// add comes last (all the others have read the state by then: their add follows their read) stores the new state and puts the
// ticket back to 0.  No separate tick launch.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n4,
                                                   double* state, double lr, double beta1, double beta2d, int* ticket,
                                                   float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                   AdamSkip skip) {
  ADAM_PLAIN_PROLOGUE
  ADAM_UPDATE_LOOP(ADAM_GRAD_PLAIN)
  ADAM_PLAIN_EPILOGUE
}

extern "C" int mmego_adam_step(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                               double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                               int nskip, int* ticket) {
  MMEGO_REQUIRE(p && g && m && v && state && ticket && n > 0 && (n % 4) == 0);
  AdamSkip sk;
  MMEGO_REQUIRE(adam_skip_ranges(&sk, skip, nskip, n));
  MMEGO_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, st, p, g, m, v, n / 4, state, lr, beta1, beta2, ticket,
                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay, sk);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}


extern "C" int mmego_grad_norm_nblk(long n) {
  long b = (n / 4 + 255) / 256;
  return (int)(b > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : (b < 1 ? 1 : b));
}

extern "C" int mmego_grad_sqnorm(void* stream, const float* g, long n, const long* skip, int nskip, double* part, int npart) {
  MMEGO_REQUIRE(g && part && n > 0 && (n % 4) == 0 && npart == mmego_grad_norm_nblk(n));
  AdamSkip sk;
  MMEGO_REQUIRE(adam_skip_ranges(&sk, skip, nskip, n));
  MMEGO_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)part & 7) == 0);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(npart), dim3(256), 0, (hipStream_t)stream, g, n / 4, part, sk);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_adam_step_clipped(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                                       double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                                       int nskip, int* ticket, const double* part, int npart, double max_norm, double* stats) {
  MMEGO_REQUIRE(p && g && m && v && state && ticket && part && stats && n > 0 && (n % 4) == 0);
  MMEGO_REQUIRE(npart == mmego_grad_norm_nblk(n) && max_norm > 0.0);        // (NaN fails the comparison; +inf measures without clipping)
  AdamSkip sk;
  MMEGO_REQUIRE(adam_skip_ranges(&sk, skip, nskip, n));
  MMEGO_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  MMEGO_REQUIRE((((uintptr_t)part | (uintptr_t)stats) & 7) == 0);
  hipLaunchKernelGGL(adam_clipped_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n / 4, state, lr,
                     beta1, beta2, ticket, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
                     (float)weight_decay, sk, part, npart, max_norm, stats);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
