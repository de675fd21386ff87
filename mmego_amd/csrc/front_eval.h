// Eval-mode front end of Upper_Net in ONE kernel, the text that front.hip (fp32 operands) and front_bf16.hip (bf16 operands) share:
// Transform2H -> PointNet (6-8-16-24) -> concat with the first four point columns -> GlobalPointNet (28-32-48-64) -> softmax
// attention pooling over the frame's points.
// Replaces, for the frozen / evaluated Upper_Net (reference Net/Upper_Net.py:242-266 PointNet, :270-301 GlobalPointNet incl. its
// attention pooling, :381-393 UpperNet.forward up to the sequence model, Util/Universal_Util/Utils.py:284-292 Transform2H), the
// chain transform2h -> mlp3_eval -> mlp3_eval -> attn_pool_forward, whose 28- and 64-channel per-point tensors went through HBM
// between the launches.  Here a frame's points never leave the CU: per frame the kernel reads the radar tile (N x 6 floats), writes
// the transformed points back (quirk Q1: the caller's tensor is transformed in place and Lower_Net reads it afterwards) and
// emits 64 pooled floats + the N attention weights.
//
// Layout.  One workgroup (4 waves) walks frames; a wave owns 16-point SLABS of the frame (slab s of a frame goes to wave s & 3), and
// a slab runs through all six stages inside its wave, so NO workgroup barrier separates the stages; the (BatchNorm-folded,
// zero-padded) weights are staged once per workgroup and only read afterwards, K padded to multiples of 16, row strides K + 4
// elements.
// r06: the stages are computed TRANSPOSED -- D^T[feature][point] = W[feature][k] . X^T[k][point], the weight tile as the A operand --
// because the result layout of that product (lane (point, q), register i: feature 16 ct + 4 q + i) IS the B-operand layout of the next
// stage's MFMAs (lane (point, q): k = 16 c + 4 q .. + 3): bias (the first MFMA's addend), ReLU and any rounding happen in registers and
// a slab's activations never touch LDS.  The concat of GlobalPointNet's input keeps PointNet's 24 features where they are (k 0..23) and
// puts the four point columns BEHIND them (k 24..27); the weight columns of that layer are permuted to match when they are staged.
// The pooling is an online softmax per wave (running max / sum / weighted column sums over its slabs), accumulated per lane (its
// point, its 16 features), reduced over the points once per frame and combined across the four waves in a fixed order: deterministic.
//
// The file that includes this defines the kernel's name as FRONT_EVAL_KERNEL (FRONT_EVAL_KERNEL_ATTRS: more attributes for it, if any)
// and, as FRONT_EVAL_OPERANDS, a struct O of operand traits:
//   elem             the LDS element type of the weights
//   vec              a lane's operand of one 16-k block: its four k (16 c + 4 q .. + 3) of a weight row (A) or of a point (B)
//   W_IN_SH, weights(sh, own)   whether the weight tiles lie in front of the biases in the float array sh, or in an array of their own
//   store(x)         a float as a weight element
//   cols(a, b, c, d) four floats as a B operand
//   mma(w, x, acc)   acc[ct] += w[ct] . x over the block's 16 k, for the NCT feature tiles of a stage
//   relu(x)          max(x, 0)
//   act(acc, out)    relu of a stage's accumulators as the next stage's B operands
// (The kernel is defined HERE under the includer's name and not as a function template that a __global__ function calls: a
// parameter struct that reaches its readers through a call is read whole at the kernel's entry, where the kernel itself reads each
// field from the kernel-argument segment where it is used -- NOTES.md, "One body for the fp32 and bf16 eval kernels".)
#pragma once
#include "common.h"
#if !defined(FRONT_EVAL_KERNEL) || !defined(FRONT_EVAL_OPERANDS)
#error "define FRONT_EVAL_KERNEL (the kernel's name) and FRONT_EVAL_OPERANDS (its operand traits) in front of front_eval.h"
#endif
#ifndef FRONT_EVAL_KERNEL_ATTRS
#define FRONT_EVAL_KERNEL_ATTRS
#endif

#define FR_SLAB 16
// row strides (elements) of the [n][k] weight tiles: Kpad + 4
#define FR_S16 20
#define FR_S32 36
#define FR_S48 52

struct FrontLayer { const float* W; const float* b; const float* gamma; const float* beta; const float* rmean; const float* rvar; };
struct FrontP {
  float* x; const float* x_src; const float* R; const float* t; long F; int N;
  FrontLayer l[6];              // PointNet conv1..3, GlobalPointNet conv1..3, each with its eval-mode BatchNorm
  const float* attn_w; const float* attn_b; float eps;
  float* vec; float* attn;
};

// weights in LDS: [n][k] tiles with stride S; offsets in elements
#define FR_W1 0                               // 16 x 16 (8 x 6 real)
#define FR_W2 (FR_W1 + 16 * FR_S16)           // 16 x 16 (16 x 8)
#define FR_W3 (FR_W2 + 16 * FR_S16)           // 32 x 16 (24 x 16)
#define FR_G1 (FR_W3 + 32 * FR_S16)           // 32 x 32 (32 x 28)
#define FR_G2 (FR_G1 + 32 * FR_S32)           // 48 x 32
#define FR_G3 (FR_G2 + 48 * FR_S32)           // 64 x 48
#define FR_WEND (FR_G3 + 64 * FR_S48)
// the float array sh: the biases (16, 16, 32, 32, 48, 64), then the 64 score weights
#define FR_B1 0
#define FR_B2 (FR_B1 + 16)
#define FR_B3 (FR_B2 + 16)
#define FR_C1 (FR_B3 + 32)
#define FR_C2 (FR_C1 + 32)
#define FR_C3 (FR_C2 + 48)
#define FR_AW (FR_C3 + 64)
#define FR_SHARED_END (FR_AW + 64)
#define FR_MAXN 1024

__device__ __forceinline__ float fr_dot3_nofma(float a0, float a1, float a2, float b0, float b1, float b2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}

// one stage of a slab, transposed: D^T[NCT*16 features][16 points] = bias + W[NCT*16][KCH*16] . X^T, W in LDS ([n][k], stride SW) as
// the A operand, the activations' k blocks in registers as the B operand (lane (point fr, fq): k = 16 c + 4 fq .. + 3); the folded bias
// (lane (point, fq), register i: feature 16 ct + 4 fq + i -- the accumulator's own layout) is the first MFMA's addend: no add afterwards
template <class O, int NCT, int KCH, int SW>
__device__ __forceinline__ void fr_stage_t(const typename O::elem* W, const typename O::vec* x, const float* bias4, f32x4 (&acc)[NCT], int fr, int fq) {
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) acc[ct] = *reinterpret_cast<const f32x4*>(bias4 + ct * 16);
#pragma unroll
  for (int c = 0; c < KCH; ++c) {
    typename O::vec w[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) w[ct] = *reinterpret_cast<const typename O::vec*>(W + (ct * 16 + fr) * SW + 16 * c + 4 * fq);
    O::mma(w, x[c], acc);
  }
}

__global__ __launch_bounds__(256) FRONT_EVAL_KERNEL_ATTRS void FRONT_EVAL_KERNEL(FrontP p) {
  typedef FRONT_EVAL_OPERANDS O;
  typedef O::vec V;
  // the weight tiles lie in front of the biases in sh (O::W_IN_SH: floats, one base address for both) or in an array of their own
  constexpr int FB = O::W_IN_SH ? FR_WEND : 0;
  __shared__ __attribute__((aligned(16))) float sh_[FB + FR_SHARED_END];
  __shared__ __attribute__((aligned(16))) O::elem shw_[FR_WEND];      // (takes no LDS where it is not used)
  O::elem* const shw = O::weights(sh_, shw_);
  float* const sh = sh_ + FB;
  __shared__ float scale[208];                     // per-channel BatchNorm scales while the weights are folded
  __shared__ float sc[FR_MAXN];                    // raw scores of the frame's points
  __shared__ float comb[2][4][66];                 // per wave: running max, running sum, 64 weighted column sums (double buffered)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;

  // ---- weights -> LDS (BatchNorm folded: s = gamma / sqrt(var + eps); Wf = s W; bf = (b - mean) s + beta -- bn_fold_linear's
  // expressions), zero padded.  Two phases, as in mlp3_eval.h: per-channel scales and folded biases (threads 0..63, all 30 loads in
  // flight at once), then every thread's 26 weight elements -- every load unconditional on a clamped index and issued before the
  // first LDS store (a rolled loop was one dependent round trip per iteration: ~26 of them in front of the first point).
#define FR_PIN(v) asm volatile("" : "+v"(v))
  {
    constexpr int Cn[6] = {8, 16, 24, 32, 48, 64}, Kn[6] = {6, 8, 16, 28, 32, 48};
    constexpr int Cp[6] = {16, 16, 32, 32, 48, 64}, Kp[6] = {16, 16, 16, 32, 32, 48};
    constexpr int Sw[6] = {FR_S16, FR_S16, FR_S16, FR_S32, FR_S32, FR_S48};
    constexpr int Wo[6] = {FR_W1, FR_W2, FR_W3, FR_G1, FR_G2, FR_G3}, Bo[6] = {FR_B1, FR_B2, FR_B3, FR_C1, FR_C2, FR_C3};
    constexpr int So[6] = {0, 16, 32, 64, 96, 144};                    // per-channel scales
    if (tid < 64) {
      float g[6], v[6], m[6], e[6], c[6];
#pragma unroll
      for (int L = 0; L < 6; ++L) {
        const FrontLayer& q = p.l[L];
        const int nc = min(tid, Cn[L] - 1);
        g[L] = q.gamma[nc]; v[L] = q.rvar[nc]; m[L] = q.rmean[nc]; e[L] = q.beta[nc]; c[L] = q.b[nc];
      }
#pragma unroll
      for (int L = 0; L < 6; ++L) {
        FR_PIN(g[L]); FR_PIN(v[L]); FR_PIN(m[L]); FR_PIN(e[L]); FR_PIN(c[L]);
        const float sc_ = g[L] / sqrtf(v[L] + p.eps);
        const float bf = (c[L] - m[L]) * sc_ + e[L];
        if (tid < Cp[L]) { scale[So[L] + tid] = sc_; sh[Bo[L] + tid] = tid < Cn[L] ? bf : 0.f; }
      }
      sh[FR_AW + tid] = p.attn_w[tid];
    }
    __syncthreads();
    float w[26];
    int u0 = 0;
#pragma unroll
    for (int L = 0; L < 6; ++L) {
#pragma unroll
      for (int u = 0; u < Cp[L] * Kp[L] / 256; ++u) {
        const int i = tid + 256 * u, n = i / Kp[L], k = i - n * Kp[L];
        // GlobalPointNet conv1 (L = 3): tile column k < 24 holds input column 4 + k (PointNet feature k), 24..27 the point columns 0..3
        const int ks = L == 3 ? (k < 24 ? k + 4 : (k < 28 ? k - 24 : Kn[L] - 1)) : min(k, Kn[L] - 1);
        w[u0 + u] = p.l[L].W[min(n, Cn[L] - 1) * Kn[L] + ks];
      }
      u0 += Cp[L] * Kp[L] / 256;
    }
    u0 = 0;
#pragma unroll
    for (int L = 0; L < 6; ++L) {
#pragma unroll
      for (int u = 0; u < Cp[L] * Kp[L] / 256; ++u) {
        const int i = tid + 256 * u, n = i / Kp[L], k = i - n * Kp[L];
        FR_PIN(w[u0 + u]);
        shw[Wo[L] + n * Sw[L] + k] = O::store((n < Cn[L] && k < Kn[L]) ? scale[So[L] + n] * w[u0 + u] : 0.f);
      }
      u0 += Cp[L] * Kp[L] / 256;
    }
  }
#undef FR_PIN
  const float attn_b = p.attn_b ? p.attn_b[0] : 0.f;
  __syncthreads();

  const int N = p.N, nslab = N / FR_SLAB;
  int par = 0;
  for (long f = blockIdx.x; f < p.F; f += gridDim.x, par ^= 1) {
    const float* Rf = p.R + f * 9;
    const float* tf = p.t + f * 3;
    float r[9], tt[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = Rf[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tt[i] = tf[i];
    float* xf = p.x + f * (long)N * 6;
    const float* xs = p.x_src ? p.x_src + f * (long)N * 6 : xf;
    // running softmax state of this wave: the maximum (wave-uniform) and, per lane, its point's share of the denominator and of the
    // 16 weighted feature sums it holds (features 16 ct + 4 fq + i); the lanes are added once per frame
    float m_run = -INFINITY, s_part = 0.f;
    float col[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) col[ct][i] = 0.f;
    // the slab's 16 points: every lane loads the row of point (lane & 15) (24 bytes; the four 16-lane groups load the same rows:
    // no branch around the loads), and the NEXT slab's rows are requested before the current slab is computed
    float2 c01, c23, c45;
    {
      const long row = (long)min(wave, nslab - 1) * FR_SLAB + fr;
      c01 = *reinterpret_cast<const float2*>(xs + row * 6);
      c23 = *reinterpret_cast<const float2*>(xs + row * 6 + 2);
      c45 = *reinterpret_cast<const float2*>(xs + row * 6 + 4);
    }
    for (int s = wave; s < nslab; s += 4) {
      const float2 v01 = c01, v23 = c23, v45 = c45;
      {
        const long rown = (long)(s + 4 < nslab ? s + 4 : s) * FR_SLAB + fr;       // (past the last slab: this slab again)
        c01 = *reinterpret_cast<const float2*>(xs + rown * 6);
        c23 = *reinterpret_cast<const float2*>(xs + rown * 6 + 2);
        c45 = *reinterpret_cast<const float2*>(xs + rown * 6 + 4);
      }
      const float d0 = __fsub_rn(v01.x, tt[0]), d1 = __fsub_rn(v01.y, tt[1]), d2 = __fsub_rn(v23.x, tt[2]);
      const float h0 = fr_dot3_nofma(r[0], r[1], r[2], d0, d1, d2);
      const float h1 = fr_dot3_nofma(r[3], r[4], r[5], d0, d1, d2);
      const float h2 = fr_dot3_nofma(r[6], r[7], r[8], d0, d1, d2);
      if (lane < FR_SLAB) {
        const long row = (long)s * FR_SLAB + lane;
        *reinterpret_cast<float2*>(xf + row * 6) = make_float2(h0, h1);
        *reinterpret_cast<float2*>(xf + row * 6 + 2) = make_float2(h2, v23.y);
        if (p.x_src) *reinterpret_cast<float2*>(xf + row * 6 + 4) = v45;
      }
      // the point's six columns as the first stage's B operand (k = 4 fq + i): group 0: h0 h1 h2 x3, group 1: x4 x5 0 0, groups 2, 3: 0
      const V xcols = O::cols(h0, h1, h2, v23.y);
      const V x45 = O::cols(v45.x, v45.y, 0.f, 0.f);
      const V zero = O::cols(0.f, 0.f, 0.f, 0.f);
      const V bx = fq == 0 ? xcols : fq == 1 ? x45 : zero;
      f32x4 a1[1], a2[1], a3[2], g1[2], g2[3], g3[4];
      V p1[1], p2[1], f01[2], q01[2], r012[3];
      // (the biases and score weights are read from LDS in every slab -- the offset below is opaque to the compiler, which would
      //  otherwise keep all 17 float4 of them in registers across the loop: 68 VGPRs, a wave per SIMD less)
      int bo = 4 * fq;
      asm volatile("" : "+v"(bo));
      const float* const b4 = sh + bo;
      fr_stage_t<O, 1, 1, FR_S16>(shw + FR_W1, &bx, b4 + FR_B1, a1, fr, fq);
      O::act(a1, p1);
      fr_stage_t<O, 1, 1, FR_S16>(shw + FR_W2, p1, b4 + FR_B2, a2, fr, fq);
      O::act(a2, p2);
      fr_stage_t<O, 2, 1, FR_S16>(shw + FR_W3, p2, b4 + FR_B3, a3, fr, fq);
      O::act(a3, f01);
      // concat: features 0..15 | features 16..23, the four point columns, padding (the stage's padded outputs 24..31 are zero)
      if (fq == 2) f01[1] = xcols;
      fr_stage_t<O, 2, 2, FR_S32>(shw + FR_G1, f01, b4 + FR_C1, g1, fr, fq);
      O::act(g1, q01);
      fr_stage_t<O, 3, 2, FR_S32>(shw + FR_G2, q01, b4 + FR_C2, g2, fr, fq);
      O::act(g2, r012);
      fr_stage_t<O, 4, 3, FR_S48>(shw + FR_G3, r012, b4 + FR_C3, g3, fr, fq);
      // ---- scores and the online softmax update.  Lane (fr, fq), register i of tile ct: feature 16 ct + 4 fq + i of point fr.
      float y[4][4], part = 0.f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(b4 + FR_AW + ct * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          y[ct][i] = O::relu(g3[ct][i]);
          part += y[ct][i] * wv[i];
        }
      }
      part += __shfl_xor(part, 16, 64);
      part += __shfl_xor(part, 32, 64);                                          // sum over the four feature groups: the point's score
      part += attn_b;
      if (fq == 0) sc[s * FR_SLAB + fr] = part;
      float smax = part;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) smax = fmaxf(smax, __shfl_xor(smax, o, 64));   // max over the slab's 16 points
      const float m_new = fmaxf(m_run, smax);
      if (m_new != m_run) {                                                      // wave-uniform; rare after a frame's first slabs
        const float resc = __expf(m_run - m_new);                                // (exp(-inf) = 0 on the first slab)
        s_part *= resc;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int i = 0; i < 4; ++i) col[ct][i] *= resc;
        m_run = m_new;
      }
      const float e = __expf(part - m_run);
      s_part += e;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) col[ct][i] += e * y[ct][i];
    }
    // ---- add the 16 points' lanes (once per frame), then combine the four waves (fixed order) and emit the frame's outputs
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      s_part += __shfl_xor(s_part, o, 64);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) col[ct][i] += __shfl_xor(col[ct][i], o, 64);
    }
    if (fr == 0) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) comb[par][wave][2 + ct * 16 + 4 * fq + i] = col[ct][i];
      if (lane == 0) { comb[par][wave][0] = m_run; comb[par][wave][1] = s_part; }
    }
    __syncthreads();
    float M = comb[par][0][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, comb[par][w][0]);
    float S = 0.f, sw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) { sw[w] = __expf(comb[par][w][0] - M); S += comb[par][w][1] * sw[w]; }
    const float inv = 1.0f / S;
    if (tid < 64) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) v += comb[par][w][2 + tid] * sw[w];
      p.vec[f * 64 + tid] = v * inv;
    }
    for (int n = tid; n < N; n += 256) p.attn[f * (long)N + n] = __expf(sc[n] - M) * inv;
    // (sc is rewritten by the next frame's slabs: every wave must be past the loop above first; comb is double buffered)
    __syncthreads();
  }
}

// the entry points' argument checks and the launch.  w: host-side table of 38 device pointers: for PointNet conv1..3 then
// GlobalPointNet conv1..3: W, b, gamma, beta, running_mean, running_var of the layer's BatchNorm; then the attention Linear's weight
// [64] and bias [1].  One workgroup per frame, at most grid_cap of them (workgroups per CU x 256 CUs), frames walked persistently.
static inline int upper_front_eval_launch(void (*kernel)(FrontP), long grid_cap, void* stream, float* x, const float* x_src, const float* R,
                                          const float* t, long F, int N, const float* const* w, float eps, float* vec, float* attn) {
  MMEGO_REQUIRE(x && R && t && w && vec && attn && F > 0);
  MMEGO_REQUIRE(N >= FR_SLAB && N <= FR_MAXN && N % FR_SLAB == 0);
  MMEGO_REQUIRE((((uintptr_t)x | (uintptr_t)x_src) & 7) == 0);
  FrontP p;
  p.x = x; p.x_src = x_src; p.R = R; p.t = t; p.F = F; p.N = N;
  for (int L = 0; L < 6; ++L) {
    for (int j = 0; j < 6; ++j) MMEGO_REQUIRE(w[6 * L + j]);
    p.l[L] = {w[6 * L], w[6 * L + 1], w[6 * L + 2], w[6 * L + 3], w[6 * L + 4], w[6 * L + 5]};
  }
  MMEGO_REQUIRE(w[36]);
  p.attn_w = w[36]; p.attn_b = w[37]; p.eps = eps; p.vec = vec; p.attn = attn;
  const unsigned grid = (unsigned)(F < grid_cap ? F : grid_cap);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
