// The fused Adam steps of optim.hip with an exponential moving average of the weights kept in the same trip
// (FusedAdam(ema_decay=...), --ema_decay).  The Adam part is optim.hip's token for token (adam_update.h: the same prologues, update loop
// and epilogues), so p, m, v, state -- and stats, for the clipped step -- come out bit for bit as from the plain entry points.  On top,
// for every element the update touches:
//   ema = fmaf(omd, p_new - ema, ema),   omd = (float)(1 - ema_decay),
// one explicit fp32 fma on the parameter just computed, taken from its register.  ema is read and written as float4 with the others:
// 20 B/param read + 16 B/param written = 36 B/param against 28.  Elements in a skip range, and every element of a step that the clipped
// kernel skips as non-finite, leave ema as it is: an average that starts equal to the weights stays equal to them there.
// A file of its own, so that optim.hip's code object -- and with it the machine code of the kernels without an average -- stays as
// it is.
#include "adam_update.h"

__global__ __launch_bounds__(256) void adam_clipped_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v, long n4,
                                                               double* state, double lr, double beta1, double beta2d, int* ticket,
                                                               float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                               AdamSkip skip, const double* __restrict__ part, int npart,
                                                               double max_norm, double* stats, float* __restrict__ ema, float omd) {
  ADAM_CLIPPED_PROLOGUE
  if (finite) {
    const double c = sh[4] > 1.0 ? 1.0 : sh[4];
    const float cf = (float)c, step_size = (float)sh[1], bc2_sqrt = (float)sh[2];
    ADAM_UPDATE_LOOP_EMA(ADAM_GRAD_CLIPPED)
  }
  ADAM_CLIPPED_EPILOGUE
}

__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, long n4,
                                                       double* state, double lr, double beta1, double beta2d, int* ticket,
                                                       float beta2, float omb1, float omb2, float eps, float weight_decay,
                                                       AdamSkip skip, float* __restrict__ ema, float omd) {
  ADAM_PLAIN_PROLOGUE
  ADAM_UPDATE_LOOP_EMA(ADAM_GRAD_PLAIN)
  ADAM_PLAIN_EPILOGUE
}

extern "C" int mmego_adam_step_ema(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                                   double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                                   int nskip, int* ticket, float* ema, double ema_decay) {
  MMEGO_REQUIRE(p && g && m && v && state && ticket && n > 0 && (n % 4) == 0);
  AdamSkip sk;
  MMEGO_REQUIRE(adam_skip_ranges(&sk, skip, nskip, n));
  MMEGO_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  MMEGO_REQUIRE(ema_args_ok(ema, ema_decay));
  hipLaunchKernelGGL(adam_ema_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n / 4, state, lr, beta1,
                     beta2, ticket, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay, sk, ema,
                     (float)(1.0 - ema_decay));
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_adam_step_clipped_ema(void* stream, float* p, const float* g, float* m, float* v, long n, double* state,
                                           double lr, double beta1, double beta2, double eps, double weight_decay, const long* skip,
                                           int nskip, int* ticket, const double* part, int npart, double max_norm, double* stats,
                                           float* ema, double ema_decay) {
  MMEGO_REQUIRE(p && g && m && v && state && ticket && part && stats && n > 0 && (n % 4) == 0);
  MMEGO_REQUIRE(npart == mmego_grad_norm_nblk(n) && max_norm > 0.0);        // (as mmego_adam_step_clipped)
  AdamSkip sk;
  MMEGO_REQUIRE(adam_skip_ranges(&sk, skip, nskip, n));
  MMEGO_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  MMEGO_REQUIRE((((uintptr_t)part | (uintptr_t)stats) & 7) == 0);
  MMEGO_REQUIRE(ema_args_ok(ema, ema_decay));
  hipLaunchKernelGGL(adam_clipped_ema_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n / 4, state, lr,
                     beta1, beta2, ticket, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
                     (float)weight_decay, sk, part, npart, max_norm, stats, ema, (float)(1.0 - ema_decay));
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
