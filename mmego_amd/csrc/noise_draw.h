// The unit-variance draw shared by the kernels that add noise on the device: the cloud packer's return noise (frame_pack.hip) and the
// head-pose perturbation (pose_noise.hip).  Integer hashes and one exact conversion, so tests/point_noise_ref.py and
// tests/pose_noise_ref.py restate every bit in numpy.
#pragma once
#include "common.h"

#define FP_NOISE_SCALE 0x1.bb67aep-22f   // fp32 nearest to sqrt(3) 2^-22: the centred sum of four 22-bit uniforms -> unit variance

// z_c of the header's recipe: the centred sum of the four 22-bit draws h(c, 0 .. 3) of the return whose noise key is b, scaled to
// unit variance.  The sum stays below 2^24, so its conversion is exact.
__device__ __forceinline__ float fp_noise_z(unsigned b, unsigned c) {
  unsigned s = 0;
#pragma unroll
  for (unsigned i = 0; i < 4; ++i) s += hash32(b + (4u * c + i + 1u)) >> 10;
  return (float)((int)s - 8388606) * FP_NOISE_SCALE;
}
