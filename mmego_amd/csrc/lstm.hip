// LSTM recurrences on the matrix cores (fp32, v_mfma_f32_16x16x4_f32), PyTorch gate order i,f,g,o.
//
//  (lstm_step kernels live in lstm_step.hip)
//  lstm_step_kernel   one timestep of a (bi)LSTM of any hidden size H (H % 32 == 0): gates = xproj_t +
//                     h_{t-1}.W_hh^T, fused cell update.  Used for IMU_Net's 2x(2-layer, H=512) BiLSTMs
//                     (reference Net/IMU_Net.py:58-62,77,82), 94 % of the path's FLOPs.  Both directions
//                     in one launch; a workgroup owns 64 batch rows x 32 hidden units x 4 gates so the
//                     cell update is register-local; workgroups that share a W_hh slice are placed on
//                     one XCD (its L2 then holds 1/8 of W_hh).
//  lstm64_fwd/bwd     whole-sequence persistent kernels for the three H=64 BiLSTMs of Upper_Net /
//                     Lower_Net (Upper_Net.py:333, Lower_Net.py:91): batch rows are independent through
//                     the recurrence, so a workgroup keeps W_hh in registers, 16 or 4 rows of h in LDS and c
//                     in registers and walks all T steps with no inter-workgroup traffic.  16 rows per
//                     workgroup on v_mfma_f32_16x16x4_f32 where that fills the chip, 4 rows on
//                     v_mfma_f32_4x4x1_16B_f32 for small batches (ROWS below; l64_rows chooses).
#include "common.h"
#include "lstm_cell.h"
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

// ---------------------------------------------------------------------------------------------
// H = 64 persistent sequence kernels
// ---------------------------------------------------------------------------------------------
struct Lstm64P {
  const float* xproj[2]; long xs;
  const float* whh[2];
  const float* bhh[2];
  const float* h0[2]; const float* c0[2];
  float* out; long os;
  float* hn[2]; float* cn[2];
  float* gates[2]; float* cst[2]; float* hprev[2];
  int B, T;
  // inverted inter-layer dropout fused into the output store (nn.LSTM(dropout=p) between stacked layers): drop_y / drop_mask
  // have out's layout; the mask of element i is a hash of (i, seed_ctr[0], salt)
  float* drop_y; float* drop_mask; float drop_p; const unsigned long long* seed_ctr; unsigned salt;
};
// The kernels' by-value parameter types are the ABI's descriptors (MmegoLstm64Fwd / MmegoLstm64Bwd of include/mmego_hip.h) under the names
// the kernels were compiled with: same size, and every field at the same offset with the same size.  l64_param copies one across.
#define L64_SAME_FIELD(P, D, f) && offsetof(P, f) == offsetof(D, f) && sizeof(P::f) == sizeof(D::f)
#define L64_SAME_LAYOUT(P, D, FIELDS) static_assert(sizeof(P) == sizeof(D) FIELDS(L64_SAME_FIELD, P, D), #D " is " #P)
#define L64_FWD_FIELDS(X, P, D)                                                                                                        \
  X(P, D, xproj) X(P, D, xs) X(P, D, whh) X(P, D, bhh) X(P, D, h0) X(P, D, c0) X(P, D, out) X(P, D, os) X(P, D, hn) X(P, D, cn)       \
  X(P, D, gates) X(P, D, cst) X(P, D, hprev) X(P, D, B) X(P, D, T) X(P, D, drop_y) X(P, D, drop_mask) X(P, D, drop_p) X(P, D, seed_ctr) \
  X(P, D, salt)
L64_SAME_LAYOUT(Lstm64P, MmegoLstm64Fwd, L64_FWD_FIELDS);
template <class P, class D>
static inline P l64_param(const D& d) { P p; memcpy(&p, &d, sizeof p); return p; }

// (the cell update runs on the fast activations of lstm_cell.h: the step loop of this kernel issued ~490 VALU instructions per 64
// MFMAs, most of them libm expf and 64-bit address arithmetic)

// Workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every outstanding global load / store
// (vmcnt(0)), which would put the prefetch of the next step's inputs and this step's stash stores back on the critical path.
#define L64_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

#define WLD 272  // 256 gate columns + 16: consecutive k rows land on disjoint bank halves

// Per-row pointers kept in arrays lose the "global memory" inference the compiler makes for plain kernel arguments and turn into
// FLAT loads / stores -- which count in lgkmcnt as well as vmcnt, so that every wait for an LDS read also waited for all global
// loads and stores in flight.  Explicit global address space keeps them global_load / global_store (vmcnt only).
typedef const float __attribute__((address_space(1)))* l64_gcptr;
typedef float __attribute__((address_space(1)))* l64_gptr;
typedef f32x4 __attribute__((address_space(1)))* l64_gptr4;
typedef const f32x4 __attribute__((address_space(1)))* l64_gcptr4;

// ROWS: the batch rows of a workgroup, 16 or 4.  One step of a 16-row workgroup is 64 v_mfma_f32_16x16x4_f32 per wave at 32 cycles
// each: 2048 cycles of one CU's matrix pipe that no schedule inside the CU shortens, on 2 B/16 workgroups (8 of 256 CUs at B = 64).
// Rows are independent through the recurrence, so small batches take 4-row workgroups instead: the same step is 64
// v_mfma_f32_4x4x1_16B_f32 per wave at 8 cycles each (512 cycles) on four times as many CUs.  The launchers choose (l64_rows).
//
// Who owns what.  ROWS = 16: lane (fq, fr) of wave w owns hidden unit 16 w + fr and rows 4 fq .. 4 fq + 3 (the 16x16 accumulator
// layout).  ROWS = 4: lane 4 b + r of wave w owns hidden unit 16 w + b and row r, ONE cell per lane.  Either way element (k, row) of
// the h tile is at k * ROWS + row -- for ROWS = 4 that is the thread index, and an operand read is 64 consecutive words: no bank
// conflict in either direction (the backward's gate-gradient tile: L64BwdProd<ROWS>::at).
template <int ROWS>
struct L64Map {
  static_assert(ROWS == 16 || ROWS == 4, "rows of a workgroup");
  static constexpr int RPL = ROWS / 4;        // rows (cells) per lane
  static __device__ __forceinline__ int unit(int wave, int lane) { return wave * 16 + (ROWS == 16 ? (lane & 15) : (lane >> 2)); }
  static __device__ __forceinline__ int row0(int lane) { return ROWS == 16 ? (lane >> 4) * 4 : (lane & 3); }   // this lane's first row
};

// One k of the 4-row product: D[block b][row i][column c] += A[ABID][row i] * B[b][c] -- the four rows of block ABID's A operand go
// to all 16 blocks (CBSZ = 4), so ONE register holds 16 k's of the h tile (lane 4 a + i: row i of k = a) and an h value is read from
// LDS once, not once per block.  (The broadcast fields are immediates: a template argument, not a loop variable.)
template <int ABID>
__device__ __forceinline__ f32x4 l64_mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, ABID, 0); }
// ONE accumulator chain, in a fixed order of the k's: the order in which the 16-row form's v_mfma_f32_16x16x4_f32 chain takes them
// (an instruction adds its four k's one after the other, each one fused multiply-add, as a 4x4x1 instruction adds its one), so that
// the two forms give the same bits.  X(a) expands to the instructions of block a.
#define L64_X16(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

// a[i] of lane q of a quad  <->  a[q] of lane i: two rounds of pairwise exchanges by DPP quad permutes (no LDS, no wait)
__device__ __forceinline__ float l64_quad_perm_b1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)); }  // [1,0,3,2]
__device__ __forceinline__ float l64_quad_perm_4e(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)); }  // [2,3,0,1]
__device__ __forceinline__ void l64_quad_transpose(float (&a)[4], int lane) {
  const bool o1 = lane & 1, o2 = lane & 2;
#pragma unroll
  for (int r = 0; r < 4; r += 2) {
    const float x = a[r], y = a[r + 1], got = l64_quad_perm_b1(o1 ? x : y);
    a[r] = o1 ? got : x;
    a[r + 1] = o1 ? y : got;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const float x = a[q], y = a[q + 2], got = l64_quad_perm_4e(o2 ? x : y);
    a[q] = o2 ? got : x;
    a[q + 2] = o2 ? y : got;
  }
}

// The recurrent product of the forward step, h_{t-1} . W_hh^T for this lane's cells: W_hh stationary in 64 registers per lane, loaded
// straight from global memory (no W_hh tile in LDS, no staging pass); run() reads the h tile and leaves pre[gate][cell].
template <int ROWS>
struct L64FwdProd;
template <>
struct L64FwdProd<16> {
  // at MFMA step s lane quad fq takes k = 16 fq + s (for h and W_hh alike: any k order is valid as long as both operands agree),
  // so the 16 values of a gate are 4 contiguous 16-B loads
  float wreg[16][4];
  __device__ __forceinline__ void load(const float* W, int wave, int lane) {
    const int fq = lane >> 4, j = wave * 16 + (lane & 15);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float* wrow = W + (g * 64 + j) * 64 + 16 * fq;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + 4 * q);
        wreg[4 * q + 0][g] = v.x; wreg[4 * q + 1][g] = v.y; wreg[4 * q + 2][g] = v.z; wreg[4 * q + 3][g] = v.w;
      }
    }
  }
  __device__ __forceinline__ void run(const float* hs, int lane, float (&pre)[4][4]) const {
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float hk[16];                    // all 16 operand reads in flight before the first MFMA (they were issued in pairs, each
#pragma unroll                       // pair followed by its own wait: eight LDS latencies per step)
    for (int k4 = 0; k4 < 16; ++k4) hk[k4] = hs[(16 * fq + k4) * 16 + fr];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k4 = 0; k4 < 16; ++k4) {
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(hk[k4], wreg[k4][g], acc[g], 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) pre[g][reg] = acc[g][reg];
  }
};
template <>
struct L64FwdProd<4> {
  // B operand: lane 4 b + g holds the column of (unit 16 w + b, gate g), one W_hh row of 64 k's (16 contiguous 16-B loads); A
  // operand register v: k = 16 v + a in block a.  The instruction's 64 columns are this wave's 16 units x 4 gates, so the gates of a
  // k share ONE instruction.  The 16-row form's chain of a gate takes k = 16 fq + s, fq = 0 .. 3 inside instruction s = 0 .. 15:
  // here that is block a = s of register v = fq, a outside and v inside, on one accumulator -- the same sum in the same order, the
  // same bits.  The result has the four rows of a (unit, gate) in one lane; the cell wants the four gates of a (unit, row): a 4 x 4
  // transpose inside each lane quad.
  float wreg[64];
  __device__ __forceinline__ void load(const float* W, int wave, int lane) {
    const float* wrow = W + ((lane & 3) * 64 + wave * 16 + (lane >> 2)) * 64;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + 4 * q);
      wreg[4 * q + 0] = v.x; wreg[4 * q + 1] = v.y; wreg[4 * q + 2] = v.z; wreg[4 * q + 3] = v.w;
    }
  }
  __device__ __forceinline__ void run(const float* hs, int lane, float (&pre)[4][1]) const {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    float hk[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) hk[v] = hs[64 * v + lane];
    __builtin_amdgcn_sched_barrier(0);
#define L64_FWD_K(A_)                                                                                                       \
  s = l64_mfma4<A_>(hk[0], wreg[A_], s); s = l64_mfma4<A_>(hk[1], wreg[16 + A_], s); s = l64_mfma4<A_>(hk[2], wreg[32 + A_], s); \
  s = l64_mfma4<A_>(hk[3], wreg[48 + A_], s);
    L64_X16(L64_FWD_K)
#undef L64_FWD_K
    float a[4] = {s.x, s.y, s.z, s.w};
    l64_quad_transpose(a, lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) pre[g][0] = a[g];
  }
};

// FULL: B is a multiple of the ROWS rows of a workgroup, so every `live` test is a compile-time true; STASH / DROP: the backward
// stashes (gates, cell states, h_{t-1}: all or none) / the fused inter-layer dropout.  Template parameters so that the step loop is
// straight-line code.  That matters more than it looks: with loads and stores predicated row by row (an s_cbranch_execz around
// each) and run-time branches on the optional outputs, the compiler could not count the outstanding memory operations across
// the loop and put ONE s_waitcnt vmcnt(0) into every step -- which waits for the previous step's ~28 stores per lane to be
// acknowledged, not only for the prefetched inputs (2.26 us per step; 1.96 us now).
template <bool FULL, bool STASH, bool DROP, int ROWS>
__device__ __forceinline__ void lstm64_fwd_body(const Lstm64P& p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using Map = L64Map<ROWS>;
  constexpr int R = Map::RPL;    // cells of this lane: rows rl .. rl + R - 1 of hidden unit j
  float* hs = smem;              // [64 k][ROWS rows]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.y, r0 = blockIdx.x * ROWS;
  const int B = p.B, T = p.T;
  const int j = Map::unit(wave, lane), rl = Map::row0(lane);
  float creg[R], hreg[R], bh[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bh[g] = p.bhh[d] ? p.bhh[d][g * 64 + j] : 0.f;
#pragma unroll
  for (int reg = 0; reg < R; ++reg) {
    int row = r0 + rl + reg;
    bool ok = row < B;
    creg[reg] = (ok && p.c0[d]) ? p.c0[d][row * 64 + j] : 0.f;
    hreg[reg] = (ok && p.h0[d]) ? p.h0[d][row * 64 + j] : 0.f;
    hs[j * ROWS + rl + reg] = hreg[reg];
  }
  __syncthreads();
  L64FwdProd<ROWS> prod;         // W_hh: stationary in registers for the whole sequence
  prod.load(p.whh[d], wave, lane);

  // The input projections do not depend on the recurrence: step s+1's values are fetched while step s computes, so
  // their latency (the longest thing in a step otherwise) is off the critical path.  All addresses advance by a
  // per-step stride from bases computed once (the address arithmetic used to outweigh the MFMAs).
  float xp[4][R], xpn[4][R];
  constexpr bool stash = STASH, keep_h = STASH, drop = DROP;
  const unsigned dkey = drop ? dropout_key(p.seed_ctr[0], p.salt) : 0u;
  const float keep_scale = drop ? 1.0f / (1.0f - p.drop_p) : 1.0f;
  const int t_first = d == 0 ? 0 : T - 1;
  const long dir = d == 0 ? 1 : -1;
  l64_gcptr xq[R];
  l64_gptr oq[R], hq[R], gq[R], cq[R];
  bool live[R];
#pragma unroll
  for (int reg = 0; reg < R; ++reg) {
    const int row = r0 + rl + reg;
    live[reg] = FULL || row < B;
    const long rt = (long)(live[reg] ? row : 0) * T + t_first;
    xq[reg] = (l64_gcptr)(p.xproj[d] + rt * p.xs + j);
    oq[reg] = (l64_gptr)(p.out + rt * p.os + d * 64 + j);
    hq[reg] = keep_h ? (l64_gptr)(p.hprev[d] + rt * 64 + j) : (l64_gptr)nullptr;
    const long tr = (long)t_first * B + (live[reg] ? row : 0);
    gq[reg] = stash ? (l64_gptr)(p.gates[d] + tr * 256 + 4 * j) : (l64_gptr)nullptr;   // gate stash: [t][b][unit][i,f,g,o]
    cq[reg] = stash ? (l64_gptr)(p.cst[d] + tr * 64 + j) : (l64_gptr)nullptr;
  }
  const long xstep = dir * p.xs, ostep = dir * p.os, hstep = dir * 64, gstep = dir * (long)B * 256,
             cstep = dir * (long)B * 64;
#define L64_LOAD_XP(DST)                                                                            \
  do {                                                                                              \
    _Pragma("unroll") for (int reg = 0; reg < R; ++reg) {                                           \
      _Pragma("unroll") for (int g = 0; g < 4; ++g) DST[g][reg] = (FULL || live[reg]) ? xq[reg][g * 64] : 0.f; \
      xq[reg] += xstep;                                                                             \
    }                                                                                               \
  } while (0)
  L64_LOAD_XP(xp);
  for (int s = 0; s < T; ++s) {
    // (unconditional: past the last step the previous address is loaded again -- no branch around the prefetch)
    if (s + 1 >= T) {
#pragma unroll
      for (int reg = 0; reg < R; ++reg) xq[reg] -= xstep;
    }
    L64_LOAD_XP(xpn);
    if (keep_h) {
#pragma unroll
      for (int reg = 0; reg < R; ++reg) {
        if (FULL || live[reg]) *hq[reg] = hreg[reg];
        hq[reg] += hstep;
      }
    }
    float acc[4][R];                 // h_{t-1} . W_hh^T of this lane's cells, per gate
    prod.run(hs, lane, acc);
    L64_LDS_BARRIER();  // everyone has finished reading hs for this step
#pragma unroll
    for (int reg = 0; reg < R; ++reg) {
      const LstmCell u = lstm_cell_fwd(acc[0][reg] + (xp[0][reg] + bh[0]), acc[1][reg] + (xp[1][reg] + bh[1]),
                                       acc[2][reg] + (xp[2][reg] + bh[2]), acc[3][reg] + (xp[3][reg] + bh[3]), creg[reg]);
      const float cn = u.c, hn = u.h;
      creg[reg] = cn;
      hreg[reg] = hn;
      hs[j * ROWS + rl + reg] = hn;
      if (FULL || live[reg]) {
        *oq[reg] = hn;
        if (drop) {
          const long off = oq[reg] - (l64_gptr)p.out;
          const float mk = dropout_keep(dkey, (unsigned)off, p.drop_p) ? keep_scale : 0.f;
          p.drop_mask[off] = mk;
          p.drop_y[off] = hn * mk;
        }
        if (stash) {
          *(l64_gptr4)gq[reg] = (f32x4){u.i, u.f, u.g, u.o};      // one 16-B store (was four dword stores 256 B apart)
          *cq[reg] = cn;
        }
      }
      oq[reg] += ostep;
      if (stash) { gq[reg] += gstep; cq[reg] += cstep; }
    }
    // (the copy stays HERE: hoisted into the MFMA block by the scheduler, it made every step wait for the loads it had just issued)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int reg = 0; reg < R; ++reg) xp[g][reg] = xpn[g][reg];
    L64_LDS_BARRIER();
  }
#undef L64_LOAD_XP
#pragma unroll
  for (int reg = 0; reg < R; ++reg) {
    int row = r0 + rl + reg;
    if (row < B) {
      if (p.hn[d]) p.hn[d][row * 64 + j] = hreg[reg];
      if (p.cn[d]) p.cn[d][row * 64 + j] = creg[reg];
    }
  }
}

template <bool FULL, bool STASH, bool DROP, int ROWS>
__global__ __launch_bounds__(256) void lstm64_fwd_kernel(Lstm64P p) { lstm64_fwd_body<FULL, STASH, DROP, ROWS>(p); }

// Several INDEPENDENT stacks' layers in one launch (grid z = stack): UpperNetwlocal's global and anchor BiLSTM(64) stacks have the same
// shape and no data in common (Net/Upper_Net.py:333-339 and :208-216) -- one after the other each layer was 8 workgroups on a 256-CU
// chip, twice.
#define L64_MAX_MULTI 4
struct Lstm64Multi { Lstm64P p[L64_MAX_MULTI]; };
template <bool FULL, bool STASH, bool DROP, int ROWS>
__global__ __launch_bounds__(256) void lstm64_fwd_multi_kernel(Lstm64Multi m) { lstm64_fwd_body<FULL, STASH, DROP, ROWS>(m.p[blockIdx.z]); }

// Rows per workgroup at batch size B: 4 while the 16-row grid -- 2 directions x ceil(B / 16) workgroups -- covers at most half of
// the chip's CUs (B <= 1024 on 256 CUs), 16 from there on: a large batch fills the chip with 16-row workgroups already (config 5's
// B = 2048: 256 of them) and four times the launch width buys it nothing.  Measured (scripts/bench_lstm64_rows.py, T = 8, forward /
// backward us per launch, 4-row against 16-row): B = 512 10.4 / 8.8 against 19.8 / 19.1; B = 1024 (two 4-row workgroups per CU) 15.8 /
// 12.9 against 21.1 / 20.1; B = 2048 (four per CU) 24.8 / 21.2 against 21.9 / 21.5.  A function of B and the device alone -- not of
// T, the options or the number of stacks of a _multi launch -- so that every launch of one shape takes the same form and sums in the
// same order.  MMEGO_LSTM64_ROWS = 4 | 16 forces one form (A/B runs and the tests; read per call: the tests switch it).
static int l64_rows(int B) {
  const char* env = getenv("MMEGO_LSTM64_ROWS");
  const int forced = env ? atoi(env) : 0;
  if (forced == 4 || forced == 16) return forced;
  return 2 * cdiv(B, 16) * 2 <= mmego_cu_count() ? 4 : 16;
}
extern "C" int mmego_lstm64_rows(int B) { return B > 0 ? l64_rows(B) : MMEGO_EBADARG; }

extern "C" int mmego_lstm64_forward(void* stream, int B, int T, const float* xproj0, const float* xproj1, long xs,
                                    const float* whh0, const float* whh1, const float* bhh0, const float* bhh1,
                                    const float* h0_0, const float* h0_1, const float* c0_0, const float* c0_1, float* out,
                                    long os, float* hn0, float* hn1,
                                    float* cn0, float* cn1, float* gates0, float* gates1, float* cst0, float* cst1,
                                    float* hprev0, float* hprev1, float* drop_y, float* drop_mask, float drop_p,
                                    const unsigned long long* seed_ctr, int salt) {
  MMEGO_REQUIRE((drop_mask == nullptr) == (drop_y == nullptr));
  MMEGO_REQUIRE(!drop_mask || (seed_ctr && drop_p > 0.f && drop_p < 1.f && (long)B * T * os < (1L << 32)));
  MMEGO_REQUIRE(B > 0 && T > 0 && xproj0 && xproj1 && whh0 && whh1 && out);
  MMEGO_REQUIRE((((uintptr_t)whh0 | (uintptr_t)whh1) & 15) == 0);
  MMEGO_REQUIRE((gates0 == nullptr) == (cst0 == nullptr) && (gates1 == nullptr) == (cst1 == nullptr));
  MMEGO_REQUIRE((((uintptr_t)gates0 | (uintptr_t)gates1) & 15) == 0);      // the gate stash is stored as f32x4
  Lstm64P p;
  p.xproj[0] = xproj0; p.xproj[1] = xproj1; p.xs = xs;
  p.whh[0] = whh0; p.whh[1] = whh1;
  p.bhh[0] = bhh0; p.bhh[1] = bhh1;
  p.h0[0] = h0_0; p.h0[1] = h0_1; p.c0[0] = c0_0; p.c0[1] = c0_1;
  p.out = out; p.os = os;
  p.hn[0] = hn0; p.hn[1] = hn1; p.cn[0] = cn0; p.cn[1] = cn1;
  p.gates[0] = gates0; p.gates[1] = gates1; p.cst[0] = cst0; p.cst[1] = cst1;
  p.hprev[0] = hprev0; p.hprev[1] = hprev1;
  p.B = B; p.T = T;
  p.drop_y = drop_y; p.drop_mask = drop_mask; p.drop_p = drop_p; p.seed_ctr = seed_ctr; p.salt = (unsigned)salt;
  const int rows = l64_rows(B);
  size_t lds = (size_t)(64 * rows) * sizeof(float);          // h tile only: W_hh lives in registers
  const bool full = B % rows == 0, st_ = gates0 != nullptr, dr = drop_mask != nullptr;
  MMEGO_REQUIRE((hprev0 != nullptr) == st_ && (hprev1 != nullptr) == st_ && (gates1 != nullptr) == st_);   // stashes: all or none
#define L64_FWD_LAUNCH_R(F_, S_, D_, R_)                                                                                     \
  do {                                                                                                                       \
    if (int e = mmego_allow_lds<lstm64_fwd_kernel<F_, S_, D_, R_>>(lds)) return e;                                           \
    hipLaunchKernelGGL((lstm64_fwd_kernel<F_, S_, D_, R_>), dim3(cdiv(B, R_), 2), dim3(256), lds, (hipStream_t)stream, p);   \
  } while (0)
#define L64_FWD_LAUNCH(F_, S_, D_) do { if (rows == 4) L64_FWD_LAUNCH_R(F_, S_, D_, 4); else L64_FWD_LAUNCH_R(F_, S_, D_, 16); } while (0)
  if (full) {
    if (st_ && dr) L64_FWD_LAUNCH(true, true, true);
    else if (st_) L64_FWD_LAUNCH(true, true, false);
    else if (dr) L64_FWD_LAUNCH(true, false, true);
    else L64_FWD_LAUNCH(true, false, false);
  } else {
    if (st_ && dr) L64_FWD_LAUNCH(false, true, true);
    else if (st_) L64_FWD_LAUNCH(false, true, false);
    else if (dr) L64_FWD_LAUNCH(false, false, true);
    else L64_FWD_LAUNCH(false, false, false);
  }
#undef L64_FWD_LAUNCH
#undef L64_FWD_LAUNCH_R
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

struct Lstm64BwdP {
  const float* dout; long dos;
  const float* gates[2]; const float* cst[2]; const float* c0[2];
  const float* whh[2];
  float* dgates[2]; long dgs;
  int B, T;
};
#define L64_BWD_FIELDS(X, P, D) \
  X(P, D, dout) X(P, D, dos) X(P, D, gates) X(P, D, cst) X(P, D, c0) X(P, D, whh) X(P, D, dgates) X(P, D, dgs) X(P, D, B) X(P, D, T)
L64_SAME_LAYOUT(Lstm64BwdP, MmegoLstm64Bwd, L64_BWD_FIELDS);

// The recurrent product of the backward step, dh_rec[row][k] = sum_n dgates[row][n] * W_hh[n][k] over the 256 gate columns n, from the
// gate-gradient tile dgs [256 n][ROWS] in LDS; W_hh stationary in 64 registers per lane, straight from global memory with all loads in
// flight.  run() follows the barrier behind the tile's stores; take() follows the step's closing barrier and leaves dh[cell].
template <int ROWS>
struct L64BwdProd;
template <>
struct L64BwdProd<16> {
  static constexpr int LDS_FLOATS = 256 * 16;
  static __device__ __forceinline__ int at(int n, int row) { return n * 16 + row; }      // where (n, row) of the tile lies
  // this wave owns k in [16 w, 16 w + 16): operand i is row n = 4 i + fq, column 16 w + fr
  float wreg[64];
  f32x4 dh4;
  __device__ __forceinline__ void load(const float* Whh, int wave, int lane) {
    const float* W = Whh + (lane >> 4) * 64 + wave * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 64; ++i) wreg[i] = W[i * 256];
  }
  __device__ __forceinline__ void run(float* dgs, int wave, int lane) {
    const int fr = lane & 15, fq = lane >> 4;
    // four accumulator chains (a dependent 16x16x4 MFMA can issue every 32 cycles, an independent one every 8) and the
    // operand reads in groups of 16 ahead of their MFMAs (fixed summation order: (a0 + a1) + (a2 + a3))
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, a3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nb = 0; nb < 64; nb += 16) {
      float dk[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) dk[u] = dgs[((nb + u) * 4 + fq) * 16 + fr];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 16; u += 4) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dk[u], wreg[nb + u], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dk[u + 1], wreg[nb + u + 1], a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(dk[u + 2], wreg[nb + u + 2], a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(dk[u + 3], wreg[nb + u + 3], a3, 0, 0, 0);
      }
    }
    dh4 = (a0 + a1) + (a2 + a3);
  }
  __device__ __forceinline__ void take(const float* dgs, int wave, int lane, float (&dh)[4]) const {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) dh[reg] = dh4[reg];
  }
};
template <>
struct L64BwdProd<4> {
  // One 4x4x1 instruction is 4 rows x 64 columns x one n, and the step has 64 output columns k in all: a wave cannot own a quarter of
  // the k's without leaving 48 of its 64 columns idle.  So every wave takes ALL 64 k's (lane = k) and a quarter of the sum, and the
  // four partial sums meet in LDS.  The quarter of wave w is accumulator chain w of the 16-row form -- the n's with (n mod 16) / 4 = w,
  // in rising order on one accumulator -- and dh of a cell is (p0 + p1) + (p2 + p3) as there: the same bits.  Register v, block a:
  // n = 16 (4 v + a / 4) + 4 w + a mod 4.  The tile keeps a wave's 64 n's together (at(): 272 words per wave, 16 past 256, so that the
  // two hidden-unit groups of a 32-lane store group land on different bank halves): operand reads are 64 consecutive words.
  // Partial sums: wave w's rows at part[w][row][k], rows 72 words apart: a ds_read_b32 is served in two groups of 32 lanes over 32
  // banks, and the 32 cells of a group (4 rows x 8 units) then read row * 8 + unit, 32 different banks.
  static constexpr int WLDS = 272, PART = 4 * WLDS, PLD = 72, LDS_FLOATS = PART + 4 * 4 * PLD;
  static __device__ __forceinline__ int at(int n, int row) { return ((n & 15) >> 2) * WLDS + (4 * (n >> 4) + (n & 3)) * 4 + row; }
  float wreg[64];
  __device__ __forceinline__ void load(const float* Whh, int wave, int lane) {
    const float* W = Whh + (long)(4 * wave) * 64 + lane;
#pragma unroll
    for (int i = 0; i < 64; ++i) wreg[i] = W[(16 * (i >> 2) + (i & 3)) * 64];
  }
  __device__ __forceinline__ void run(float* dgs, int wave, int lane) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    float dk[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) dk[v] = dgs[WLDS * wave + 64 * v + lane];
    __builtin_amdgcn_sched_barrier(0);
#define L64_BWD_K(A_) s = l64_mfma4<A_>(dk[V_], wreg[16 * V_ + A_], s);
#define V_ 0
    L64_X16(L64_BWD_K)
#undef V_
#define V_ 1
    L64_X16(L64_BWD_K)
#undef V_
#define V_ 2
    L64_X16(L64_BWD_K)
#undef V_
#define V_ 3
    L64_X16(L64_BWD_K)
#undef V_
#undef L64_BWD_K
    float* part = dgs + PART + wave * (4 * PLD) + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) part[i * PLD] = s[i];
  }
  __device__ __forceinline__ void take(const float* dgs, int wave, int lane, float (&dh)[1]) const {
    const float* part = dgs + PART + (lane & 3) * PLD + wave * 16 + (lane >> 2);
    const float p0 = part[0], p1 = part[4 * PLD], p2 = part[8 * PLD], p3 = part[12 * PLD];
    dh[0] = (p0 + p1) + (p2 + p3);
  }
};

// FULL as in lstm64_fwd_kernel: straight-line step loop (no row predicates, the prefetch unconditional, loads from explicit
// global pointers), so the compiler counts its waits instead of draining the memory pipe every step.
template <bool FULL, int ROWS>
__device__ __forceinline__ void lstm64_bwd_body(const Lstm64BwdP& p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using Map = L64Map<ROWS>;
  constexpr int R = Map::RPL;
  float* dgs = smem;              // [256 n][ROWS rows] (+ the 4-row form's partial sums)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.y, r0 = blockIdx.x * ROWS;
  const int B = p.B, T = p.T;
  const int j = Map::unit(wave, lane), rl = Map::row0(lane);
  L64BwdProd<ROWS> prod;
  prod.load(p.whh[d], wave, lane);
  float dcreg[R], dhrec[R];
#pragma unroll
  for (int reg = 0; reg < R; ++reg) dcreg[reg] = dhrec[reg] = 0.f;

  // Everything a step reads from memory (incoming dh, saved gates, cell states) is independent of the recurrence: the
  // next step's values are fetched while this step computes.  c_{t-1} of this step is c_t of the next one.
  float gin[R][6], gnx[R][6];        // per row: dh_in, i, f, g, o, c_prev
  float ccur[R];
  const l64_gcptr g_gates = (l64_gcptr)p.gates[d], g_dout = (l64_gcptr)p.dout, g_cst = (l64_gcptr)p.cst[d];
  const bool has_c0 = p.c0[d] != nullptr;
  const l64_gcptr g_c0 = has_c0 ? (l64_gcptr)p.c0[d] : g_cst;      // (a valid address either way: the value is masked below)
#define L64_LOAD_BWD(DST, step)                                                                                \
  do {                                                                                                         \
    const int tq_ = d == 0 ? (step) : T - 1 - (step);                                                          \
    const int tp_ = d == 0 ? tq_ - 1 : tq_ + 1;                                                                \
    _Pragma("unroll") for (int reg = 0; reg < R; ++reg) {                                                      \
      const int row_ = r0 + rl + reg;                                                                          \
      if (FULL || row_ < B) {                                                                                  \
        const f32x4 gv_ = *(l64_gcptr4)(g_gates + ((long)tq_ * B + row_) * 256 + 4 * j);                       \
        DST[reg][0] = g_dout[((long)row_ * T + tq_) * p.dos + d * 64 + j];                                     \
        DST[reg][1] = gv_.x; DST[reg][2] = gv_.y; DST[reg][3] = gv_.z; DST[reg][4] = gv_.w;                    \
        const l64_gcptr cp_ = ((step) > 0) ? g_cst + ((long)tp_ * B + row_) * 64 + j : g_c0 + (long)row_ * 64 + j; \
        const float cv_ = *cp_;                                                                                \
        DST[reg][5] = ((step) > 0 || has_c0) ? cv_ : 0.f;                                                      \
      } else {                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 6; ++q) DST[reg][q] = 0.f;                                       \
      }                                                                                                        \
    }                                                                                                          \
  } while (0)
  L64_LOAD_BWD(gin, T - 1);
  {
    const int tl = d == 0 ? T - 1 : 0;
#pragma unroll
    for (int reg = 0; reg < R; ++reg) {
      int row = r0 + rl + reg;
      ccur[reg] = (FULL || row < B) ? g_cst[((long)tl * B + row) * 64 + j] : 0.f;
    }
  }
  for (int s = T - 1; s >= 0; --s) {
    const int tt = d == 0 ? s : T - 1 - s;
    const int sn = s > 0 ? s - 1 : 0;          // (unconditional prefetch: the last step loads step 0's values again)
    L64_LOAD_BWD(gnx, sn);
    float dg4[4][R];
#pragma unroll
    for (int reg = 0; reg < R; ++reg) {
      int row = r0 + rl + reg;
      if (FULL || row < B) {
        float dh = gin[reg][0] + dhrec[reg];
        float gi = gin[reg][1], gf = gin[reg][2], gg = gin[reg][3], go = gin[reg][4];
        const LstmCellGrad o = lstm_cell_bwd(gi, gf, gg, go, fast_tanh(ccur[reg]), gin[reg][5], dcreg[reg], dh);   // (tanh: the forward's fast form)
        dg4[0][reg] = o.di;
        dg4[1][reg] = o.df;
        dg4[2][reg] = o.dg;
        dg4[3][reg] = o.dout;
        dcreg[reg] = o.dcprev;
        l64_gptr dst = (l64_gptr)p.dgates[d] + ((long)row * T + tt) * p.dgs + j;
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[g * 64] = dg4[g][reg];
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) dg4[g][reg] = 0.f;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) dgs[L64BwdProd<ROWS>::at(g * 64 + j, rl + reg)] = dg4[g][reg];
      ccur[reg] = gin[reg][5];
    }
    L64_LDS_BARRIER();
    prod.run(dgs, wave, lane);
    __builtin_amdgcn_sched_barrier(0);       // (keep the copy of the prefetched values at the end of the step: see the forward kernel)
#pragma unroll
    for (int reg = 0; reg < R; ++reg)
#pragma unroll
      for (int q = 0; q < 6; ++q) gin[reg][q] = gnx[reg][q];
    L64_LDS_BARRIER();
    prod.take(dgs, wave, lane, dhrec);
  }
#undef L64_LOAD_BWD
}

template <bool FULL, int ROWS>
__global__ __launch_bounds__(256) void lstm64_bwd_kernel(Lstm64BwdP p) { lstm64_bwd_body<FULL, ROWS>(p); }
struct Lstm64BwdMulti { Lstm64BwdP p[L64_MAX_MULTI]; };
template <bool FULL, int ROWS>
__global__ __launch_bounds__(256) void lstm64_bwd_multi_kernel(Lstm64BwdMulti m) { lstm64_bwd_body<FULL, ROWS>(m.p[blockIdx.z]); }

extern "C" int mmego_lstm64_backward(void* stream, int B, int T, const float* dout, long dos, const float* gates0,
                                     const float* gates1, const float* cst0, const float* cst1, const float* c0_0,
                                     const float* c0_1, const float* whh0, const float* whh1, float* dgates0,
                                     float* dgates1, long dgs) {
  MMEGO_REQUIRE(B > 0 && T > 0 && dout && gates0 && gates1 && cst0 && cst1 && whh0 && whh1 && dgates0 && dgates1);
  MMEGO_REQUIRE((((uintptr_t)whh0 | (uintptr_t)whh1) & 15) == 0);
  MMEGO_REQUIRE((((uintptr_t)gates0 | (uintptr_t)gates1) & 15) == 0);      // the gate stash is loaded as f32x4
  Lstm64BwdP p;
  p.dout = dout; p.dos = dos;
  p.gates[0] = gates0; p.gates[1] = gates1; p.cst[0] = cst0; p.cst[1] = cst1;
  p.c0[0] = c0_0; p.c0[1] = c0_1;
  p.whh[0] = whh0; p.whh[1] = whh1;
  p.dgates[0] = dgates0; p.dgates[1] = dgates1; p.dgs = dgs;
  p.B = B; p.T = T;
#define L64_BWD_LAUNCH(K_, R_, Z_, P_)                                                                                              \
  do {                                                                                                                              \
    const size_t lds = (size_t)L64BwdProd<R_>::LDS_FLOATS * sizeof(float);                                                          \
    if (B % R_ == 0) hipLaunchKernelGGL((K_<true, R_>), dim3(cdiv(B, R_), 2, Z_), dim3(256), lds, (hipStream_t)stream, P_);         \
    else hipLaunchKernelGGL((K_<false, R_>), dim3(cdiv(B, R_), 2, Z_), dim3(256), lds, (hipStream_t)stream, P_);                    \
  } while (0)
  if (l64_rows(B) == 4) L64_BWD_LAUNCH(lstm64_bwd_kernel, 4, 1, p);
  else L64_BWD_LAUNCH(lstm64_bwd_kernel, 16, 1, p);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

// n <= 4 independent stacks' layers per launch.  descs: n host structs MmegoLstm64Fwd / MmegoLstm64Bwd (include/mmego_hip.h: the argument
// lists of mmego_lstm64_forward / _backward as structs); every stack must have the same B and T and the same options (stashes for all or
// none, dropout for all or none).
extern "C" int mmego_lstm64_forward_multi(void* stream, int n, const MmegoLstm64Fwd* h) {
  MMEGO_REQUIRE(h && n >= 1 && n <= L64_MAX_MULTI);
  Lstm64Multi m;
  const int B = h[0].B, T = h[0].T;
  const bool st_ = h[0].gates[0] != nullptr, dr = h[0].drop_mask != nullptr;
  for (int i = 0; i < n; ++i) {
    const MmegoLstm64Fwd& p = h[i];
    MMEGO_REQUIRE(p.B == B && p.T == T && B > 0 && T > 0 && p.xproj[0] && p.xproj[1] && p.whh[0] && p.whh[1] && p.out);
    MMEGO_REQUIRE((((uintptr_t)p.whh[0] | (uintptr_t)p.whh[1]) & 15) == 0);
    MMEGO_REQUIRE((((uintptr_t)p.gates[0] | (uintptr_t)p.gates[1]) & 15) == 0);
    MMEGO_REQUIRE((p.drop_mask == nullptr) == (p.drop_y == nullptr) && (p.drop_mask != nullptr) == dr);
    MMEGO_REQUIRE(!p.drop_mask || (p.seed_ctr && p.drop_p > 0.f && p.drop_p < 1.f && (long)B * T * p.os < (1L << 32)));
    MMEGO_REQUIRE((p.gates[0] != nullptr) == st_ && (p.gates[1] != nullptr) == st_ && (p.cst[0] != nullptr) == st_ && (p.cst[1] != nullptr) == st_ &&
                  (p.hprev[0] != nullptr) == st_ && (p.hprev[1] != nullptr) == st_);
    m.p[i] = l64_param<Lstm64P>(p);
  }
  for (int i = n; i < L64_MAX_MULTI; ++i) m.p[i] = m.p[0];
  const int rows = l64_rows(B);
  const size_t lds = (size_t)(64 * rows) * sizeof(float);
  const bool full = B % rows == 0;
#define L64_FWDM_LAUNCH_R(F_, S_, D_, R_) hipLaunchKernelGGL((lstm64_fwd_multi_kernel<F_, S_, D_, R_>), dim3(cdiv(B, R_), 2, n), dim3(256), lds, (hipStream_t)stream, m)
#define L64_FWDM_LAUNCH(F_, S_, D_) do { if (rows == 4) L64_FWDM_LAUNCH_R(F_, S_, D_, 4); else L64_FWDM_LAUNCH_R(F_, S_, D_, 16); } while (0)
  if (full) {
    if (st_ && dr) L64_FWDM_LAUNCH(true, true, true);
    else if (st_) L64_FWDM_LAUNCH(true, true, false);
    else if (dr) L64_FWDM_LAUNCH(true, false, true);
    else L64_FWDM_LAUNCH(true, false, false);
  } else {
    if (st_ && dr) L64_FWDM_LAUNCH(false, true, true);
    else if (st_) L64_FWDM_LAUNCH(false, true, false);
    else if (dr) L64_FWDM_LAUNCH(false, false, true);
    else L64_FWDM_LAUNCH(false, false, false);
  }
#undef L64_FWDM_LAUNCH
#undef L64_FWDM_LAUNCH_R
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_lstm64_backward_multi(void* stream, int n, const MmegoLstm64Bwd* h) {
  MMEGO_REQUIRE(h && n >= 1 && n <= L64_MAX_MULTI);
  Lstm64BwdMulti m;
  const int B = h[0].B, T = h[0].T;
  for (int i = 0; i < n; ++i) {
    const MmegoLstm64Bwd& p = h[i];
    MMEGO_REQUIRE(p.B == B && p.T == T && B > 0 && T > 0 && p.dout && p.gates[0] && p.gates[1] && p.cst[0] && p.cst[1] && p.whh[0] && p.whh[1] &&
                  p.dgates[0] && p.dgates[1]);
    MMEGO_REQUIRE((((uintptr_t)p.whh[0] | (uintptr_t)p.whh[1]) & 15) == 0);
    MMEGO_REQUIRE((((uintptr_t)p.gates[0] | (uintptr_t)p.gates[1]) & 15) == 0);
    m.p[i] = l64_param<Lstm64BwdP>(p);
  }
  for (int i = n; i < L64_MAX_MULTI; ++i) m.p[i] = m.p[0];
  if (l64_rows(B) == 4) L64_BWD_LAUNCH(lstm64_bwd_multi_kernel, 4, n, m);
  else L64_BWD_LAUNCH(lstm64_bwd_multi_kernel, 16, n, m);
#undef L64_BWD_LAUNCH
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
