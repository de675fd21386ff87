// The fused Adam steps of optim.hip and optim_ema.hip with a learning-rate schedule evaluated INSIDE the launch
// (FusedAdam(lr_schedule=...), --lr_schedule / --lr_warmup).  lr is a host double in the kernel arguments, so a captured graph replays
// the rate it was captured with; the step count t, though, lives in state[0] on the device and advances inside the update launch.  Here
// the one lane per workgroup that forms the bias corrections first forms the rate of step t,
//   lr_t = lr * (w(t) * d(t))      (include/mmego_hip.h spells w and d out; all of it in double),
// and the step is the existing one at lr_t: adam_update.h's prologues, update loop and epilogues, token for token, reading `lr` as the
// name RATE declares.  So p, m, v, state[0..2] -- and stats, ema -- come out bit for bit as from the unscheduled entry points called
// with lr = lr_t.  state has a fourth word, the rate of the last step taken, stored by the workgroup that draws the last ticket; a step
// skipped as non-finite stores none of the four and so consumes no schedule step.
// Cost: a handful of double operations (one cos or pow) in one lane per workgroup, nothing per element: 28 B/param, 36 with the average.
// A file of its own, so that the code objects of optim.hip and optim_ema.hip stay as they are.
#include <math.h>
#include "adam_update.h"

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

#define SCHED_RATE(A, K) const double lr = lr0 * lr_multiplier(sched, t); A[K] = lr;

__global__ __launch_bounds__(256) void adam_sched_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, long n4,
                                                         double* state, double lr0, double beta1, double beta2d, int* ticket,
                                                         float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                         AdamSkip skip, MmegoLrSchedule sched) {
  ADAM_PLAIN_PROLOGUE_(4, SCHED_RATE(bc, 3))
  ADAM_UPDATE_LOOP(ADAM_GRAD_PLAIN)
  ADAM_PLAIN_EPILOGUE_(state[3] = bc[3];)
}

__global__ __launch_bounds__(256) void adam_ema_sched_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, long n4,
                                                             double* state, double lr0, double beta1, double beta2d, int* ticket,
                                                             float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                             AdamSkip skip, float* __restrict__ ema, float omd, MmegoLrSchedule sched) {
  ADAM_PLAIN_PROLOGUE_(4, SCHED_RATE(bc, 3))
  ADAM_UPDATE_LOOP_EMA(ADAM_GRAD_PLAIN)
  ADAM_PLAIN_EPILOGUE_(state[3] = bc[3];)
}

__global__ __launch_bounds__(256) void adam_clipped_sched_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v, long n4,
                                                                 double* state, double lr0, double beta1, double beta2d, int* ticket,
                                                                 float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                                 AdamSkip skip, const double* __restrict__ part, int npart,
                                                                 double max_norm, double* stats, MmegoLrSchedule sched) {
  ADAM_CLIPPED_PROLOGUE_(10, SCHED_RATE(sh, 9))
  if (finite) {
    const double c = sh[4] > 1.0 ? 1.0 : sh[4];
    const float cf = (float)c, step_size = (float)sh[1], bc2_sqrt = (float)sh[2];
    ADAM_UPDATE_LOOP(ADAM_GRAD_CLIPPED)
  }
  ADAM_CLIPPED_EPILOGUE_(state[3] = sh[9];)
}

__global__ __launch_bounds__(256) void adam_clipped_ema_sched_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                     float* __restrict__ m, float* __restrict__ v, long n4,
                                                                     double* state, double lr0, double beta1, double beta2d,
                                                                     int* ticket, float beta2, float omb1, float omb2, float eps,
                                                                     float weight_decay, AdamSkip skip,
                                                                     const double* __restrict__ part, int npart, double max_norm,
                                                                     double* stats, float* __restrict__ ema, float omd,
                                                                     MmegoLrSchedule sched) {
  ADAM_CLIPPED_PROLOGUE_(10, SCHED_RATE(sh, 9))
  if (finite) {
    const double c = sh[4] > 1.0 ? 1.0 : sh[4];
    const float cf = (float)c, step_size = (float)sh[1], bc2_sqrt = (float)sh[2];
    ADAM_UPDATE_LOOP_EMA(ADAM_GRAD_CLIPPED)
  }
  ADAM_CLIPPED_EPILOGUE_(state[3] = sh[9];)
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

extern "C" int mmego_adam_step_sched(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip,
                                     int* ticket, const double* part, int npart, double max_norm, double* stats, float* ema,
                                     double ema_decay, const MmegoLrSchedule* sched) {
  MMEGO_REQUIRE(p && g && m && v && state && ticket && n > 0 && (n % 4) == 0);
  AdamSkip sk;
  MMEGO_REQUIRE(adam_skip_ranges(&sk, skip, nskip, n));
  MMEGO_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  MMEGO_REQUIRE(((uintptr_t)state & 7) == 0);
  MMEGO_REQUIRE(sched_ok(sched));
  const bool clipped = part != NULL;
  if (clipped) {
    MMEGO_REQUIRE(stats && npart == mmego_grad_norm_nblk(n) && max_norm > 0.0);        // (as mmego_adam_step_clipped)
    MMEGO_REQUIRE((((uintptr_t)part | (uintptr_t)stats) & 7) == 0);
  } else {
    MMEGO_REQUIRE(npart == 0 && !stats);
  }
  if (ema) MMEGO_REQUIRE(ema_args_ok(ema, ema_decay));
  else MMEGO_REQUIRE(ema_decay == 0.0);
  const dim3 grid(ew_blocks(n / 4)), block(256);
  const long n4 = n / 4;
  const float b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2), epsf = (float)eps, wd = (float)weight_decay;
  const float omd = (float)(1.0 - ema_decay);
  hipStream_t st = (hipStream_t)stream;
  if (!clipped && !ema)
    hipLaunchKernelGGL(adam_sched_kernel, grid, block, 0, st, p, g, m, v, n4, state, lr, beta1, beta2, ticket, b2, omb1, omb2, epsf, wd, sk,
                       *sched);
  else if (!clipped)
    hipLaunchKernelGGL(adam_ema_sched_kernel, grid, block, 0, st, p, g, m, v, n4, state, lr, beta1, beta2, ticket, b2, omb1, omb2, epsf, wd,
                       sk, ema, omd, *sched);
  else if (!ema)
    hipLaunchKernelGGL(adam_clipped_sched_kernel, grid, block, 0, st, p, g, m, v, n4, state, lr, beta1, beta2, ticket, b2, omb1, omb2, epsf,
                       wd, sk, part, npart, max_norm, stats, *sched);
  else
    hipLaunchKernelGGL(adam_clipped_ema_sched_kernel, grid, block, 0, st, p, g, m, v, n4, state, lr, beta1, beta2, ticket, b2, omb1, omb2,
                       epsf, wd, sk, part, npart, max_norm, stats, ema, omd, *sched);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
