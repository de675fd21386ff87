// Fused multi-tensor Adam over one flat parameter buffer (replaces torch.optim.Adam's foreach chain,
// reference Processor/Train/Train_Upper.py:60,182).
// Pure HBM streaming: 16 B/param read (p,g,m,v) + 12 B/param written (p,m,v) = 28 B/param, float4 accesses,
// grid-stride over <= 2048 workgroups.
// One kernel template, adam_step_kernel<CLIP, EMA, SCHED>, holds the step and its three options; what an option adds stands under
// `if constexpr`, so the form without it carries none of it:
//   CLIP   global-norm clipping (FusedAdam(max_grad_norm=...)), two launches: grad_sqnorm_kernel streams g once more (4 B/param) into
//          one fp64 record per workgroup, the step sums the records in its prologue (the launch boundary is the only synchronisation:
//          no atomics on floats, no workgroup waits for another) and runs the update on g * cf.
//   EMA    an exponential moving average of the weights kept in the same trip (FusedAdam(ema_decay=...), --ema_decay): for every
//          element the update touches, ema = fmaf(omd, p_new - ema, ema), omd = (float)(1 - ema_decay), on the parameter just
//          computed, taken from its register.  ema is read and written as float4 with the others: 36 B/param against 28.
//   SCHED  the learning rate of step t formed INSIDE the launch (FusedAdam(lr_schedule=...), --lr_schedule / --lr_warmup).  lr is a
//          host double in the kernel arguments, so a captured graph replays the rate it was captured with; the step count t,
//          though, lives in state[0] on the device.  The one lane per workgroup that forms the bias corrections first forms
//          lr_t = lr * (w(t) * d(t)) (include/mmego_hip.h spells w and d out; all of it in double), and the step is the
//          unscheduled one at lr_t.  A handful of double operations (one cos or pow) in one lane per workgroup, nothing per element.
//   DECAY  weight decay a user can shape (FusedAdam(decoupled=..., no_decay=...), --weight_decay / --decay_mode / --no_decay_1d): a
//          mask of one bit per float4 says which elements decay at all, and a host flag selects the decoupled (AdamW) form,
//          p' = fmaf(-dw, p, p) with dw = (float)(lr_t * weight_decay) formed in double by the lane that forms the bias corrections,
//          ahead of an update whose gradient carries no decay term.  A wave's 64 lanes cover float4 64 k .. 64 k + 63 in every trip,
//          so the wave reads ONE 8-byte mask word per trip through a wave-uniform index and lane l tests bit l: 8 B per 64 float4,
//          1/32 B/param against 28.  Without DECAY the step is the coupled one over every element, as it always was.
// The options do not touch each other's arithmetic: p, m, v, state[0..2] (and stats, ema) of any form are bit for bit those of the
// form without an option, called with the same rate.
#include <math.h>
#include "common.h"

// Ranges of the flat buffer (in float4 units) that the update leaves untouched: parameters that never receive a gradient.
// torch.optim.Adam skips a parameter whose .grad is None (IMU_Net.fc3, never used in forward: Net/IMU_Net.py:55), so with
// weight decay > 0 those tensors must not decay here either.
#define ADAM_MAX_SKIP 4
struct AdamSkip { long lo[ADAM_MAX_SKIP], hi[ADAM_MAX_SKIP]; int n; };

// ---- global-norm clipping, pass 1 -------------------------------------------------------------------------------------------
// part[b] = sum over workgroup b's elements of (double)g * (double)g, the skip ranges left out.  Workgroup b reads float4
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

// ---- the step ---------------------------------------------------------------------------------------------------------------
// The arguments of every form; a form reads only what its options need (the launcher leaves the rest zero).
struct AdamArgs {
  float* p; const float* g; float* m; float* v; long n4;      // four flat buffers of n4 float4
  double* state; double lr, beta1, beta2d; int* ticket;       // (state and ticket: below, above adam_step_kernel)
  float beta2, omb1, omb2, eps, weight_decay;                 // omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2)
  AdamSkip skip;
  const double* part; int npart; double max_norm; double* stats;      // CLIP: the records of pass 1
  float* ema; float omd;                                              // EMA
  MmegoLrSchedule sched;                                              // SCHED
  const unsigned long long* mask; int decoupled; double wdd;          // DECAY: bit b of word w covers float4 64 w + b (NULL: all set)
};

// g * cf as ONE rounded fp32 product: the empty asm keeps it out of any fused multiply-add with what follows.
__device__ __forceinline__ float clipped_grad(float g, float cf) {
  float r = __fmul_rn(g, cf);
  asm volatile("" : "+v"(r));
  return r;
}

__device__ __forceinline__ double lr_multiplier(const MmegoLrSchedule& sc, double t) {
  const double w = (sc.warmup > 0.0 && t < sc.warmup) ? t / sc.warmup : 1.0;
  const double s = t - sc.warmup;
  if (!(s > 0.0)) return w;                               // warm-up and step W itself: d is exactly 1
  double d = 1.0;
  if (sc.kind == 1 || sc.kind == 2) {
    const double x = (s < sc.span ? s : sc.span) / sc.span;
    const double shape = sc.kind == 1 ? (1.0 + cos(M_PI * x)) / 2.0 : 1.0 - x;
    d = sc.floor + (1.0 - sc.floor) * shape;
  } else if (sc.kind == 3) {
    const double gk = pow(sc.gamma, floor(s / sc.every));
    d = gk > sc.floor ? gk : sc.floor;
  }
  return d;                                               // (s > 0: t > W, w is 1)
}

// The update itself.  CLIP: the gradient is the fp32 product g * cf, rounded once on its own; otherwise g as it lies there.  EMA: every
// element the update touches moves its average towards the NEW parameter (still in its register) by one explicit fp32 fma; an element
// in a skip range leaves the loop before the average is read.
// DECAY: `decays` is this float4's mask bit.  Coupled: the decay term joins the gradient where the bit is set, as above; decoupled: the
// parameter is scaled first, by ONE explicit fmaf (p - dw p rounded once; NOT p * (1 - dw), whose fp32 factor has a handful of values
// near 1 and would quantise the decay), and the update runs on it with the gradient alone.  A clear bit is the step at weight_decay 0.
template <bool CLIP, bool EMA, bool DECAY>
__device__ __forceinline__ void adam_update(const AdamArgs& a, float cf, float step_size, float bc2_sqrt, float dw) {
  float4* __restrict__ p4 = reinterpret_cast<float4*>(a.p);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(a.g);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(a.m);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(a.v);
  float4* __restrict__ e4 = reinterpret_cast<float4*>(a.ema);
  // (256: the workgroup size of the one launcher, as the record sum of the prologue has it)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += (long)gridDim.x * 256) {
    bool skipped = false;
#pragma unroll
    for (int r = 0; r < ADAM_MAX_SKIP; ++r) skipped |= (r < a.skip.n && i >= a.skip.lo[r] && i < a.skip.hi[r]);
    if (skipped) continue;      // a tensor that never receives a gradient (torch.optim.Adam skips grad=None)
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], ee;
    if constexpr (EMA) ee = e4[i];
    bool decays = true;
    if constexpr (DECAY) {
      // i >> 6 is the same in all 64 lanes of a wave (i = 256 * (blockIdx.x + trip * gridDim.x) + threadIdx.x): taken from the first
      // active lane it is a scalar.  The mask is never written while a step runs: read through the constant address space, so the
      // stores to p, m, v cannot be taken to alias it, the word arrives by one scalar 8-byte load per wave and trip
      typedef const __attribute__((address_space(4))) unsigned long long* ConstWords;
      const long w = __builtin_amdgcn_readfirstlane((int)(i >> 6));
      const unsigned long long word = a.mask ? ((ConstWords)a.mask)[w] : ~0ull;
      decays = (word >> (threadIdx.x & 63)) & 1ull;
    }
    float* pa = reinterpret_cast<float*>(&pp);
    float* ga = reinterpret_cast<float*>(&gg);
    float* ma = reinterpret_cast<float*>(&mm);
    float* va = reinterpret_cast<float*>(&vv);
    float* ea = reinterpret_cast<float*>(&ee);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gr = ga[k];
      if constexpr (CLIP) gr = clipped_grad(ga[k], cf);
      if constexpr (DECAY) {
        if (a.decoupled) {
          if (decays && dw != 0.f) pa[k] = fmaf(-dw, pa[k], pa[k]);
        } else if (decays && a.weight_decay != 0.f) {
          gr = gr + a.weight_decay * pa[k];
        }
      } else {
        if (a.weight_decay != 0.f) gr = gr + a.weight_decay * pa[k];
      }
      // torch: exp_avg.lerp_(grad, 1-beta1) == m + (g - m) * (1 - beta1)
      ma[k] = ma[k] + (gr - ma[k]) * a.omb1;
      va[k] = va[k] * a.beta2 + a.omb2 * gr * gr;
      float denom = sqrtf(va[k]) / bc2_sqrt + a.eps;
      pa[k] = pa[k] - step_size * (ma[k] / denom);
      if constexpr (EMA) ea[k] = fmaf(a.omd, pa[k] - ea[k], ea[k]);
    }
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
    if constexpr (EMA) e4[i] = ee;
  }
}

// state[0] = step count (as double), state[1] = step_size = lr / (1 - b1^t), state[2] = sqrt(1 - b2^t), with SCHED state[3] = the rate
// of the last step taken.  Kept in device memory so that a captured HIP graph replays with the right bias corrections.  The step count
// advances INSIDE the update launch: every workgroup reads state[0] = t-1 when it starts and works with t; the workgroup whose ticket
// add comes last (all the others have read the state by then: their add follows their read) stores the new state and puts the
// ticket back to 0.  No separate tick launch.
// CLIP.  Prologue: EVERY workgroup sums the records of pass 1 in the same fixed order (lane j adds records j, j + 256, ...;
// wave_sum_d; the four waves in wave order), so all of them hold the same bits of
//   norm = sqrt(sum),  c = min(1, max_norm / (norm + 1e-6))  in double,  cf = (float)c.
// A norm that is not finite (an inf or NaN anywhere in the gradient) skips the step: p, m, v, ema and state stay as they are, the
// step count does not advance and no schedule step is consumed.  The workgroup that draws the last ticket also keeps the statistics:
// stats[0] this step's norm, [1] sum of the finite norms, [2] their maximum, [3] steps seen, [4] steps with c < 1, [5] steps
// skipped as non-finite, [6..7] reserved.
// DECAY.  The lane that forms the bias corrections also forms dw = (float)(lr_t * weight_decay) in double -- lr_t the rate of THIS step,
// the scheduled one under SCHED, which under a captured graph exists nowhere but here -- and shares it beside step_size.  The clip
// factor scales the raw gradient only; a step skipped as non-finite decays nothing (the update does not run); the average takes the
// final parameter.
template <bool CLIP, bool EMA, bool SCHED, bool DECAY>
__global__ __launch_bounds__(256) void adam_step_kernel(AdamArgs a) {
  // [0..2] the new state; CLIP: [3] norm, [4] c before the clamp, [5..8] the waves' sums; SCHED: the rate in one more word; DECAY: dw in one more
  constexpr int NORM = 3, C = 4, WAVES = 5, RATE = CLIP ? 9 : 3, DW = RATE + SCHED;
  __shared__ double sh[3 + SCHED + (CLIP ? 6 : 0) + DECAY];
  if constexpr (CLIP) {
    double acc = 0.0;
    for (int j = threadIdx.x; j < a.npart; j += 256) acc += a.part[j];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[WAVES + (threadIdx.x >> 6)] = acc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double t = a.state[0] + 1.0;
    double lr = a.lr;
    if constexpr (SCHED) sh[RATE] = lr = a.lr * lr_multiplier(a.sched, t);
    sh[0] = t;
    sh[1] = lr / (1.0 - pow(a.beta1, t));
    sh[2] = sqrt(1.0 - pow(a.beta2d, t));
    if constexpr (DECAY) sh[DW] = (double)(float)(lr * a.wdd);
    if constexpr (CLIP) {
      const double norm = sqrt(((sh[WAVES] + sh[WAVES + 1]) + sh[WAVES + 2]) + sh[WAVES + 3]);
      sh[NORM] = norm;
      sh[C] = a.max_norm / (norm + 1e-6);
    }
  }
  __syncthreads();
  double norm = 0.0;
  bool finite = true;
  float cf = 1.f;
  if constexpr (CLIP) {
    norm = sh[NORM];
    finite = norm < (double)INFINITY;      // (false for NaN as well)
    cf = (float)(sh[C] > 1.0 ? 1.0 : sh[C]);
  }
  float dw = 0.f;
  if constexpr (DECAY) dw = (float)sh[DW];
  if (finite) adam_update<CLIP, EMA, DECAY>(a, cf, (float)sh[1], (float)sh[2], dw);
  if (threadIdx.x == 0) {
    if (atomicAdd(a.ticket, 1) == (int)gridDim.x - 1) {
      if constexpr (CLIP) {
        a.stats[0] = norm;
        a.stats[3] += 1.0;
      }
      if (finite) {
        a.state[0] = sh[0]; a.state[1] = sh[1]; a.state[2] = sh[2];
        if constexpr (SCHED) a.state[3] = sh[RATE];
        if constexpr (CLIP) {
          a.stats[1] += norm;
          a.stats[2] = norm > a.stats[2] ? norm : a.stats[2];
          if (sh[C] < 1.0) a.stats[4] += 1.0;
        }
      } else if constexpr (CLIP) {
        a.stats[5] += 1.0;
      }
      *a.ticket = 0;
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
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

// A count of steps held in a double: finite, whole and at least `least` (NaN fails the first comparison).
static inline bool whole_at_least(double x, double least) { return x >= least && x <= 9007199254740992.0 && x == floor(x); }

static inline bool sched_ok(const MmegoLrSchedule* sc) {
  if (!sc || sc->kind < 0 || sc->kind > 3 || sc->reserved != 0) return false;
  if (!whole_at_least(sc->warmup, 0.0)) return false;
  if (!(sc->floor >= 0.0 && sc->floor < 1.0)) return false;
  if ((sc->kind == 1 || sc->kind == 2) && !whole_at_least(sc->span, 1.0)) return false;
  if (sc->kind == 3 && !(whole_at_least(sc->every, 1.0) && sc->gamma > 0.0 && sc->gamma <= 1.0)) return false;
  return true;
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

// What every entry point has in common, as it arrives, and the fp32 constants the update reads.
static inline AdamArgs adam_args(float* p, const float* g, float* m, float* v, double* state, double lr, double beta1, double beta2,
                                 double eps, double weight_decay, int* ticket) {
  AdamArgs a = {};
  a.p = p; a.g = g; a.m = m; a.v = v; a.state = state; a.lr = lr; a.beta1 = beta1; a.beta2d = beta2; a.ticket = ticket;
  a.beta2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
  a.weight_decay = (float)weight_decay;
  return a;
}
static inline void adam_clip_args(AdamArgs* a, const double* part, int npart, double max_norm, double* stats) {
  a->part = part; a->npart = npart; a->max_norm = max_norm; a->stats = stats;
}

// The one launcher: every form's checks stand here once (what only mmego_adam_step_sched's convention adds -- absent options spelled as
// NULL / 0 -- it checks itself), then the members that are derived from the host values beside `a`: n4, the skip ranges, omd, the schedule.
static int adam_launch(void* stream, AdamArgs a, bool clip, bool ema, bool sched, long n, const long* skip, int nskip, double ema_decay,
                       const MmegoLrSchedule* sc, bool decay = false) {
  MMEGO_REQUIRE(a.p && a.g && a.m && a.v && a.state && a.ticket && n > 0 && (n % 4) == 0);
  MMEGO_REQUIRE(adam_skip_ranges(&a.skip, skip, nskip, n));
  MMEGO_REQUIRE((((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.m | (uintptr_t)a.v) & 15) == 0);
  if (clip) {
    MMEGO_REQUIRE(a.part && a.stats && a.npart == mmego_grad_norm_nblk(n));
    MMEGO_REQUIRE(a.max_norm > 0.0);                      // (NaN fails the comparison; +inf measures without clipping)
    MMEGO_REQUIRE((((uintptr_t)a.part | (uintptr_t)a.stats) & 7) == 0);
  }
  if (ema) {                                              // 0 < decay < 1 (NaN fails both comparisons) and an aligned buffer
    MMEGO_REQUIRE(a.ema && ((uintptr_t)a.ema & 15) == 0 && ema_decay > 0.0 && ema_decay < 1.0);
    a.omd = (float)(1.0 - ema_decay);
  }
  if (sched) {
    MMEGO_REQUIRE(((uintptr_t)a.state & 7) == 0);
    MMEGO_REQUIRE(sched_ok(sc));
    a.sched = *sc;
  }
  a.n4 = n / 4;
#define ADAM_FORMS(D)                                                                                                          \
  adam_step_kernel<false, false, false, D>, adam_step_kernel<false, false, true, D>, adam_step_kernel<false, true, false, D>,  \
      adam_step_kernel<false, true, true, D>, adam_step_kernel<true, false, false, D>, adam_step_kernel<true, false, true, D>, \
      adam_step_kernel<true, true, false, D>, adam_step_kernel<true, true, true, D>
  static void (*const form[16])(AdamArgs) = {ADAM_FORMS(false), ADAM_FORMS(true)};      // [DECAY * 8 + CLIP * 4 + EMA * 2 + SCHED]
#undef ADAM_FORMS
  hipLaunchKernelGGL(form[decay * 8 + clip * 4 + ema * 2 + sched], dim3(ew_blocks(a.n4)), dim3(256), 0, (hipStream_t)stream, a);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_adam_step(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                               double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                               int nskip, int* ticket) {
  AdamArgs a = adam_args(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, ticket);
  return adam_launch(stream, a, false, false, false, n, skip, nskip, 0.0, NULL);
}

extern "C" int mmego_adam_step_clipped(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                                       double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                                       int nskip, int* ticket, const double* part, int npart, double max_norm, double* stats) {
  AdamArgs a = adam_args(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, ticket);
  adam_clip_args(&a, part, npart, max_norm, stats);
  return adam_launch(stream, a, true, false, false, n, skip, nskip, 0.0, NULL);
}

extern "C" int mmego_adam_step_ema(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                                   double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                                   int nskip, int* ticket, float* ema, double ema_decay) {
  AdamArgs a = adam_args(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, ticket);
  a.ema = ema;
  return adam_launch(stream, a, false, true, false, n, skip, nskip, ema_decay, NULL);
}

extern "C" int mmego_adam_step_clipped_ema(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                                           double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                                           int nskip, int* ticket, const double* part, int npart, double max_norm, double* stats,
                                           float* ema, double ema_decay) {
  AdamArgs a = adam_args(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, ticket);
  adam_clip_args(&a, part, npart, max_norm, stats);
  a.ema = ema;
  return adam_launch(stream, a, true, true, false, n, skip, nskip, ema_decay, NULL);
}

// part == NULL: the plain step, else the clipped one; ema == NULL: no weight average.  An absent option's other arguments must say so too.
extern "C" int mmego_adam_step_sched(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip,
                                     int* ticket, const double* part, int npart, double max_norm, double* stats, float* ema,
                                     double ema_decay, const MmegoLrSchedule* sched) {
  if (!part) MMEGO_REQUIRE(npart == 0 && !stats);
  if (!ema) MMEGO_REQUIRE(ema_decay == 0.0);
  AdamArgs a = adam_args(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, ticket);
  adam_clip_args(&a, part, npart, max_norm, stats);
  a.ema = ema;
  return adam_launch(stream, a, part != NULL, ema != NULL, true, n, skip, nskip, ema_decay, sched);
}

// Every option in one entry point: mmego_adam_step_sched's arguments and conventions, sched == NULL the unscheduled step (three state
// words), then the decay mask (NULL: every element decays) and the decoupled flag.
extern "C" int mmego_adam_step_decay(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip,
                                     int* ticket, const double* part, int npart, double max_norm, double* stats, float* ema,
                                     double ema_decay, const MmegoLrSchedule* sched, const unsigned long long* decay_mask,
                                     int decoupled) {
  if (!part) MMEGO_REQUIRE(npart == 0 && !stats);
  if (!ema) MMEGO_REQUIRE(ema_decay == 0.0);
  MMEGO_REQUIRE(((uintptr_t)decay_mask & 7) == 0);
  MMEGO_REQUIRE(weight_decay >= 0.0 && weight_decay < (double)INFINITY);      // (NaN fails the first comparison)
  MMEGO_REQUIRE(decoupled == 0 || decoupled == 1);
  AdamArgs a = adam_args(p, g, m, v, state, lr, beta1, beta2, eps, weight_decay, ticket);
  adam_clip_args(&a, part, npart, max_norm, stats);
  a.ema = ema;
  a.mask = decay_mask; a.decoupled = decoupled; a.wdd = weight_decay;
  return adam_launch(stream, a, part != NULL, ema != NULL, sched != NULL, n, skip, nskip, ema_decay, sched, true);
}
