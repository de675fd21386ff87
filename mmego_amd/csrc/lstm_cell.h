// The LSTM cell of every recurrence kernel (PyTorch gate order i, f, g, o), written once: the fast activations, the cell forward
// and the cell backward.  The tests compare these kernels with each other bit for bit (fused against unfused steps, the LDS-DMA
// backward step against gemm32kq, two chains against one), so they have to share the expressions, not only the formula.
// -ffp-contract=on contracts within an expression: each product-sum below stays the single expression it is.
#pragma once
#include <hip/hip_runtime.h>

// rcp / v_exp_f32 based activations at a fraction of the libm forms' instruction count (libm expf is ~15 VALU instructions; a step
// kernel's cell update evaluates 40 of them per lane).  sigmoidf_ of common.h is the libm form, for other users.
// Accuracy (u = 2^-24; derivation in tests/lstm_ref.py, held by tests/test_lstm_kernels_gpu.py, figures in NOTES.md "Float64 tests of
// the LSTM recurrence kernels"), with v_exp_f32 and v_rcp_f32 taken as 1 ulp each:
//   fast_sigmoid  RELATIVE error <= (1 - s)(1.23 |x| + 2) u + 3 u: the rounding of x * log2(e) and of the fp32 constant grow with |x|
//                 where s is small (18 u at x = -20, 64 u at x = -80 in an fp32 emulation; 2-3 u for |x| <= 1); the ABSOLUTE error
//                 stays below 1.6 u everywhere.  exp overflows to inf for x < -88.7: s = 0 exactly, where sigmoid < 2^-126.
//   fast_tanh     ABSOLUTE error <= 2 r ((1 - r)(2.45 |x| + 2) + 3) u + |t| u with r = sigmoid(-2x): at most 4 u (2.4e-7), at x = 0
//                 (emulation: 3.1 u).  It is NOT a few ulp of tanh near zero: t = 1 - 2r cancels, so for |x| < 1e-3 the relative
//                 error reaches 1e-2 and beyond (|x| < 2^-24 may come out as 0 or with the wrong sign).  Harmless for the cell -- g
//                 and tanh(c) enter sums and products of order-1 terms -- but nothing may divide by it or take its logarithm.
// Saturation is exact: a sigmoid gate is 1.0f from x = 17 on (1 - g exactly 0 in the backward) and 0.0f below -88.7, and tanh is
// +-1.0f beyond |x| = 9.1 (1 - tc^2 exactly 0).
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

struct LstmCell {
  float i, f, g, o;   // post-activation gates (what the backward stashes)
  float c, h;
};

// pre-activations of the four gates (whatever sum of product, input projection and bias the caller forms) and c_{t-1}
__device__ __forceinline__ LstmCell lstm_cell_fwd(float pi, float pf, float pg, float po, float cprev) {
  LstmCell r;
  r.i = fast_sigmoid(pi);
  r.f = fast_sigmoid(pf);
  r.g = fast_tanh(pg);
  r.o = fast_sigmoid(po);
  r.c = r.f * cprev + r.i * r.g;
  r.h = r.o * fast_tanh(r.c);
  return r;
}

struct LstmCellGrad {
  float di, df, dg, dout;   // gradients of the four pre-activations
  float dcprev;
};

// tc = tanh(c_t) is an ARGUMENT: the stage-1 training kernels pass libm tanhf(c), the lstm64 backward passes fast_tanh(c) -- an
// observable difference that stays as it is.  dc: the gradient arriving at c_t from step t+1, dh: the one arriving at h_t.
__device__ __forceinline__ LstmCellGrad lstm_cell_bwd(float gi, float gf, float gg, float go, float tc, float cprev, float dc,
                                                      float dh) {
  const float dcv = dc + dh * go * (1.f - tc * tc);
  LstmCellGrad r;
  r.di = dcv * gg * gi * (1.f - gi);
  r.df = dcv * cprev * gf * (1.f - gf);
  r.dg = dcv * gi * (1.f - gg * gg);
  r.dout = dh * tc * go * (1.f - go);
  r.dcprev = dcv * gf;
  return r;
}
