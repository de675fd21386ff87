// LDS-DMA (global_load_lds_dwordx4: global memory -> LDS, never through VGPRs) and the counted waits that go with it.
#pragma once
#include <hip/hip_runtime.h>

// One 16-byte request per lane: lane l's 16 B at gptr land at lptr + 16 l (lptr is wave-uniform: the LDS base of the wave's 1 KB).
#define GLDS16(gptr, lptr)                                                                                  \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),                   \
                                   (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

// s_waitcnt immediate of gfx9: vmcnt in bits 3:0 and 15:14, expcnt in 6:4, lgkmcnt in 11:8; a field at its maximum does not wait.
constexpr int waitcnt_imm(int vmcnt, int expcnt, int lgkmcnt) {
  return (vmcnt & 15) | ((vmcnt >> 4) << 14) | (expcnt << 4) | (lgkmcnt << 8);
}
static_assert(waitcnt_imm(0, 7, 15) == 0x0F70, "vmcnt(0)");
static_assert(waitcnt_imm(4, 7, 15) == (0x0F70 | (4 & 15) | ((4 >> 4) << 14)) && waitcnt_imm(6, 7, 15) == (0x0F70 | (6 & 15) | ((6 >> 4) << 14)) &&
              waitcnt_imm(8, 7, 15) == (0x0F70 | (8 & 15) | ((8 >> 4) << 14)) && waitcnt_imm(12, 7, 15) == (0x0F70 | (12 & 15) | ((12 >> 4) << 14)),
              "vmcnt(PC), vmcnt(2 PC) of the step kernels");
static_assert(waitcnt_imm(63, 7, 0) == 0xC07F, "lgkmcnt(0)");

// The waits go through the BUILTIN, not inline asm: the compiler's wait-count pass must see them, or it adds waits of its own for
// what these have already covered.
// At most N vector-memory operations of this wave still outstanding (they complete in issue order: all but the youngest N are done).
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
  __builtin_amdgcn_s_waitcnt(waitcnt_imm(N, 7, 15));
}
// Every LDS (and scalar-memory) operation of this wave has completed.
__device__ __forceinline__ void wait_lgkmcnt0() { __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, 7, 0)); }
