// The fused Adam update as optim.hip (plain and clipped step) and optim_ema.hip (the same steps with a weight average) share it: the
// skip ranges, the update loop, the clipped gradient, the clipped step's prologue and epilogue, the launchers' host helpers.
// Everything a kernel expands from here is a MACRO or a forceinline function that optim.hip held before the split: the tokens the
// compiler sees for adam_kernel and adam_clipped_kernel are the ones it saw then (scripts/isa_diff.py: identical).
#pragma once
#include "common.h"

// Ranges of the flat buffer (in float4 units) that the update leaves untouched: parameters that never receive a gradient.
// torch.optim.Adam skips a parameter whose .grad is None (IMU_Net.fc3, never used in forward: Net/IMU_Net.py:55), so with
// weight decay > 0 those tensors must not decay here either.
#define ADAM_MAX_SKIP 4
struct AdamSkip { long lo[ADAM_MAX_SKIP], hi[ADAM_MAX_SKIP]; int n; };

// The update itself, shared by adam_kernel (GRAD(x) = x: the gradient as it lies in g) and adam_clipped_kernel (GRAD(x) = the fp32
// product x * cf, rounded once on its own).  A macro and not an inlined function: through a function the compiler schedules
// adam_kernel's scalar loads differently, and the plain step is to stay instruction for instruction what it was.
// AVG_PTR / AVG_LOAD / AVG_ELEM / AVG_STORE: what a kernel with a weight average adds ahead of the loop, behind the four loads, behind
// element k's new parameter pa[k] (still in its register) and behind the three stores; all empty for the kernels without one.
#define ADAM_UPDATE_LOOP_(GRAD, AVG_PTR, AVG_LOAD, AVG_ELEM, AVG_STORE)                                                          \
  float4* p4 = reinterpret_cast<float4*>(p);                                                                                     \
  const float4* g4 = reinterpret_cast<const float4*>(g);                                                                         \
  float4* m4 = reinterpret_cast<float4*>(m);                                                                                     \
  float4* v4 = reinterpret_cast<float4*>(v);                                                                                     \
  AVG_PTR                                                                                                                        \
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {                        \
    bool skipped = false;                                                                                                        \
    _Pragma("unroll") for (int r = 0; r < ADAM_MAX_SKIP; ++r) skipped |= (r < skip.n && i >= skip.lo[r] && i < skip.hi[r]);      \
    if (skipped) continue; /* a tensor that never receives a gradient (torch.optim.Adam skips grad=None) */                      \
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];                                                                       \
    AVG_LOAD                                                                                                                     \
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
      AVG_ELEM                                                                                                                   \
    }                                                                                                                            \
    p4[i] = pp; m4[i] = mm; v4[i] = vv;                                                                                          \
    AVG_STORE                                                                                                                    \
  }
#define ADAM_UPDATE_LOOP(GRAD) ADAM_UPDATE_LOOP_(GRAD, , , , )
// With the weight average (ema: n floats beside p; omd = (float)(1 - decay) in the expanding kernel's scope): every element the
// update touches moves its average towards the NEW parameter by one explicit fp32 fma, ema += omd * (p_new - ema).  An element in a
// skip range leaves the loop before the average is read.
#define ADAM_UPDATE_LOOP_EMA(GRAD)                                                                                               \
  ADAM_UPDATE_LOOP_(GRAD, float4* e4 = reinterpret_cast<float4*>(ema);, float4 ee = e4[i]; float* ea = reinterpret_cast<float*>(&ee);, \
                    ea[k] = fmaf(omd, pa[k] - ea[k], ea[k]);, e4[i] = ee;)
#define ADAM_GRAD_PLAIN(x) (x)

// g * cf as ONE rounded fp32 product: the empty asm keeps it out of any fused multiply-add with what follows.
__device__ __forceinline__ float clipped_grad(float g, float cf) {
  float r = __fmul_rn(g, cf);
  asm volatile("" : "+v"(r));
  return r;
}
#define ADAM_GRAD_CLIPPED(x) clipped_grad(x, cf)      /* (cf: the clip factor in the expanding kernel's scope) */

// The clipped step around its update loop (optim.hip describes both above adam_clipped_kernel).  Prologue: EVERY workgroup sums the
// records of pass 1 in the same fixed order and leaves the new state in sh[0..2], the norm in sh[3], c before the clamp in sh[4];
// `norm` and `finite` are then in scope.  Epilogue: the workgroup that draws the last ticket stores the state and keeps the statistics.
// NSH / NBC, RATE, STATE3: the hooks of optim_sched.hip, whose kernels compute the step's rate themselves.  RATE stands behind `t` and
// declares the `lr` that the lines below it read (the kernels without a schedule have `lr` as a kernel argument and an empty RATE);
// it keeps the rate in one more word of the shared array (NSH / NBC: its length), which STATE3 stores as state[3] with the other three.
#define ADAM_CLIPPED_PROLOGUE_(NSH, RATE)                                                                                        \
  __shared__ double sh[NSH];     /* [0..2] the new state, [3] norm, [4] c before the clamp, [5..8] the waves' sums */            \
  double acc = 0.0;                                                                                                              \
  for (int j = threadIdx.x; j < npart; j += 256) acc += part[j];                                                                 \
  acc = wave_sum_d(acc);                                                                                                         \
  if ((threadIdx.x & 63) == 0) sh[5 + (threadIdx.x >> 6)] = acc;                                                                 \
  __syncthreads();                                                                                                               \
  if (threadIdx.x == 0) {                                                                                                        \
    const double norm = sqrt(((sh[5] + sh[6]) + sh[7]) + sh[8]);                                                                 \
    const double t = state[0] + 1.0;                                                                                             \
    RATE                                                                                                                         \
    sh[0] = t;                                                                                                                   \
    sh[1] = lr / (1.0 - pow(beta1, t));                                                                                          \
    sh[2] = sqrt(1.0 - pow(beta2d, t));                                                                                          \
    sh[3] = norm;                                                                                                                \
    sh[4] = max_norm / (norm + 1e-6);                                                                                            \
  }                                                                                                                              \
  __syncthreads();                                                                                                               \
  const double norm = sh[3];                                                                                                     \
  const bool finite = norm < (double)INFINITY;           /* (false for NaN as well) */
#define ADAM_CLIPPED_PROLOGUE ADAM_CLIPPED_PROLOGUE_(9, )
#define ADAM_CLIPPED_EPILOGUE_(STATE3)                                                                                           \
  if (threadIdx.x == 0) {                                                                                                        \
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {                                                                            \
      stats[0] = norm;                                                                                                           \
      stats[3] += 1.0;                                                                                                           \
      if (finite) {                                                                                                              \
        state[0] = sh[0]; state[1] = sh[1]; state[2] = sh[2];                                                                    \
        STATE3                                                                                                                   \
        stats[1] += norm;                                                                                                        \
        stats[2] = norm > stats[2] ? norm : stats[2];                                                                            \
        if (sh[4] < 1.0) stats[4] += 1.0;                                                                                        \
      } else {                                                                                                                   \
        stats[5] += 1.0;                                                                                                         \
      }                                                                                                                          \
      *ticket = 0;                                                                                                               \
    }                                                                                                                            \
  }
#define ADAM_CLIPPED_EPILOGUE ADAM_CLIPPED_EPILOGUE_()

// The plain step around its loop: thread 0 forms the new state (bc[0] = t, bc[1] = step_size, bc[2] = sqrt(1 - b2^t)) from state[0] = t-1;
// the workgroup whose ticket add comes last stores it (optim.hip, above adam_kernel).
#define ADAM_PLAIN_PROLOGUE_(NBC, RATE)                                                                                          \
  __shared__ double bc[NBC];                                                                                                     \
  if (threadIdx.x == 0) {                                                                                                        \
    const double t = state[0] + 1.0;                                                                                             \
    RATE                                                                                                                         \
    bc[0] = t;                                                                                                                   \
    bc[1] = lr / (1.0 - pow(beta1, t));                                                                                          \
    bc[2] = sqrt(1.0 - pow(beta2d, t));                                                                                          \
  }                                                                                                                              \
  __syncthreads();                                                                                                               \
  const float step_size = (float)bc[1];                                                                                          \
  const float bc2_sqrt = (float)bc[2];
#define ADAM_PLAIN_PROLOGUE ADAM_PLAIN_PROLOGUE_(3, )
#define ADAM_PLAIN_EPILOGUE_(STATE3)                                                                                             \
  if (threadIdx.x == 0) {                                                                                                        \
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {                                                                            \
      state[0] = bc[0]; state[1] = bc[1]; state[2] = bc[2];                                                                      \
      STATE3                                                                                                                     \
      *ticket = 0;                                                                                                               \
    }                                                                                                                            \
  }
#define ADAM_PLAIN_EPILOGUE ADAM_PLAIN_EPILOGUE_()

// ---- host side of the launchers ---------------------------------------------------------------------------------------------
static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// The weight average's arguments: 0 < decay < 1 (NaN fails both comparisons) and an aligned buffer.
static inline bool ema_args_ok(const float* ema, double ema_decay) {
  return ema && ((uintptr_t)ema & 15) == 0 && ema_decay > 0.0 && ema_decay < 1.0;
}

// The HOST array of [begin, end) element ranges -> float4 units; false where a range is malformed.
static inline bool adam_skip_ranges(AdamSkip* sk, const long* skip, int nskip, long n) {
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
