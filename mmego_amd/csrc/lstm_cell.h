// The LSTM cell of every recurrence kernel (PyTorch gate order i, f, g, o), written once: the fast activations, the cell forward
// and the cell backward.  The tests compare these kernels with each other bit for bit (fused against unfused steps, the LDS-DMA
// backward step against gemm32kq, two chains against one), so they have to share the expressions, not only the formula.
// -ffp-contract=on contracts within an expression: each product-sum below stays the single expression it is.
#pragma once
#include <hip/hip_runtime.h>

// rcp / v_exp_f32 based activations: a few ulp from the libm forms at a fraction of their instruction count (libm expf is ~15 VALU
// instructions; a step kernel's cell update evaluates 40 of them per lane).  sigmoidf_ of common.h is the libm form, for other users.
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
