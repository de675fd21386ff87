// Fused multi-tensor Adam over one flat parameter buffer (replaces torch.optim.Adam's foreach chain,
// reference Processor/Train/Train_Upper.py:60,182), plus the dropout mask of the LSTM inter-layer dropout.
// Pure HBM streaming: 16 B/param read (p,g,m,v) + 12 B/param written (p,m,v) = 28 B/param, float4 accesses,
// grid-stride over <= 2048 workgroups.
// Global-norm clipping (FusedAdam(max_grad_norm=...)) is two launches: grad_sqnorm_kernel streams g once more (4 B/param) into one
// fp64 record per workgroup, adam_clipped_kernel sums the records in its prologue (the launch boundary is the only synchronisation:
// no atomics on floats, no workgroup waits for another) and runs the same update on g * cf.
#include "common.h"

// Ranges of the flat buffer (in float4 units) that the update leaves untouched: parameters that never receive a gradient.
// torch.optim.Adam skips a parameter whose .grad is None (IMU_Net.fc3, never used in forward: Net/IMU_Net.py:55), so with
// weight decay > 0 those tensors must not decay here either.
#define ADAM_MAX_SKIP 4
struct AdamSkip { long lo[ADAM_MAX_SKIP], hi[ADAM_MAX_SKIP]; int n; };

// The update itself, shared by adam_kernel (GRAD(x) = x: the gradient as it lies in g) and adam_clipped_kernel (GRAD(x) = the fp32
// product x * cf, rounded once on its own).  A macro and not an inlined function: through a function the compiler schedules
// adam_kernel's scalar loads differently, and the plain step is to stay instruction for instruction what it was.
#define ADAM_UPDATE_LOOP(GRAD)                                                                                                   \
  float4* p4 = reinterpret_cast<float4*>(p);                                                                                     \
  const float4* g4 = reinterpret_cast<const float4*>(g);                                                                         \
  float4* m4 = reinterpret_cast<float4*>(m);                                                                                     \
  float4* v4 = reinterpret_cast<float4*>(v);                                                                                     \
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {                        \
    bool skipped = false;                                                                                                        \
    _Pragma("unroll") for (int r = 0; r < ADAM_MAX_SKIP; ++r) skipped |= (r < skip.n && i >= skip.lo[r] && i < skip.hi[r]);      \
    if (skipped) continue; /* a tensor that never receives a gradient (torch.optim.Adam skips grad=None) */                      \
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];                                                                       \
    float* pa = reinterpret_cast<float*>(&pp);                                                                                   \
    float* ga = reinterpret_cast<float*>(&gg);                                                                                   \
    float* ma = reinterpret_cast<float*>(&mm);                                                                                   \
    float* va = reinterpret_cast<float*>(&vv);                                                                                   \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                              \
      float gr = GRAD(ga[k]);                                                                                                    \
      if (weight_decay != 0.f) gr = gr + weight_decay * pa[k];                                                                   \
      /* torch: exp_avg.lerp_(grad, 1-beta1) == m + (g - m) * (1 - beta1) */                                                     \
      ma[k] = ma[k] + (gr - ma[k]) * omb1;                                                                                       \
      va[k] = va[k] * beta2 + omb2 * gr * gr;                                                                                    \
      float denom = sqrtf(va[k]) / bc2_sqrt + eps;                                                                               \
      pa[k] = pa[k] - step_size * (ma[k] / denom);                                                                               \
    }                                                                                                                            \
    p4[i] = pp; m4[i] = mm; v4[i] = vv;                                                                                          \
  }
#define ADAM_GRAD_PLAIN(x) (x)

// g * cf as ONE rounded fp32 product: the empty asm keeps it out of any fused multiply-add with what follows.
__device__ __forceinline__ float clipped_grad(float g, float cf) {
  float r = __fmul_rn(g, cf);
  asm volatile("" : "+v"(r));
  return r;
}
#define ADAM_GRAD_CLIPPED(x) clipped_grad(x, cf)      /* (cf: the clip factor in the expanding kernel's scope) */

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
  __shared__ double sh[9];       // [0..2] the new state, [3] norm, [4] c before the clamp, [5..8] the waves' sums
  double acc = 0.0;
  for (int j = threadIdx.x; j < npart; j += 256) acc += part[j];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) sh[5 + (threadIdx.x >> 6)] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double norm = sqrt(((sh[5] + sh[6]) + sh[7]) + sh[8]);
    const double t = state[0] + 1.0;
    sh[0] = t;
    sh[1] = lr / (1.0 - pow(beta1, t));
    sh[2] = sqrt(1.0 - pow(beta2d, t));
    sh[3] = norm;
    sh[4] = max_norm / (norm + 1e-6);
  }
  __syncthreads();
  const double norm = sh[3];
  const bool finite = norm < (double)INFINITY;           // (false for NaN as well)
  if (finite) {
    const double c = sh[4] > 1.0 ? 1.0 : sh[4];
    const float cf = (float)c, step_size = (float)sh[1], bc2_sqrt = (float)sh[2];
    ADAM_UPDATE_LOOP(ADAM_GRAD_CLIPPED)
  }
  if (threadIdx.x == 0) {
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {
      stats[0] = norm;
      stats[3] += 1.0;
      if (finite) {
        state[0] = sh[0]; state[1] = sh[1]; state[2] = sh[2];
        stats[1] += norm;
        stats[2] = norm > stats[2] ? norm : stats[2];
        if (sh[4] < 1.0) stats[4] += 1.0;
      } else {
        stats[5] += 1.0;
      }
      *ticket = 0;
    }
  }
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
  __shared__ double bc[3];
  if (threadIdx.x == 0) {
    const double t = state[0] + 1.0;
    bc[0] = t;
    bc[1] = lr / (1.0 - pow(beta1, t));
    bc[2] = sqrt(1.0 - pow(beta2d, t));
  }
  __syncthreads();
  const float step_size = (float)bc[1];
  const float bc2_sqrt = (float)bc[2];
  ADAM_UPDATE_LOOP(ADAM_GRAD_PLAIN)
  if (threadIdx.x == 0) {
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {
      state[0] = bc[0]; state[1] = bc[1]; state[2] = bc[2];
      *ticket = 0;
    }
  }
}

static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// The HOST array of [begin, end) element ranges -> float4 units; false where a range is malformed.
static bool adam_skip_ranges(AdamSkip* sk, const long* skip, int nskip, long n) {
  if (!(nskip >= 0 && nskip <= ADAM_MAX_SKIP && (nskip == 0 || skip))) return false;
  sk->n = nskip;
  for (int r = 0; r < ADAM_MAX_SKIP; ++r) {
    sk->lo[r] = sk->hi[r] = 0;
    if (r < nskip) {
      if (!(skip[2 * r] >= 0 && skip[2 * r] <= skip[2 * r + 1] && skip[2 * r + 1] <= n && (skip[2 * r] % 4) == 0 &&
            (skip[2 * r + 1] % 4) == 0))
        return false;
      sk->lo[r] = skip[2 * r] / 4;
      sk->hi[r] = skip[2 * r + 1] / 4;
    }
  }
  return true;
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
