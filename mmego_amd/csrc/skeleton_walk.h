// One wave per skeleton, one lane per JOINT: what blend_bones.hip, blend_rot.hip and smooth.hip's bones form share once every lane holds
// its own bone's vector.  Device only (wave shuffles and ballots); the arithmetic stays in the *_math.h files, which compile on the host.
#pragma once
#include "common.h"

// Joint ``lane``'s bone in the walk table bones[NB][2] of (child, parent): *mine the bone whose child it is, *parent that bone's parent;
// both -1 for a root and for the lanes behind the row's J joints.  A bone that names a joint outside the row is left out.
__device__ __forceinline__ void sw_lane_bone(const int* __restrict__ bones, int NB, int J, int lane, int* mine, int* parent) {
  *mine = *parent = -1;
  for (int b = 0; b < NB; ++b) {
    const int c = bones[2 * b], p = bones[2 * b + 1];
    if (lane < J && c == lane && p >= 0 && p < J && p != c) *mine = b, *parent = p;
  }
}

// The walk, parents before children: the child of bone b (the lane with mine == b) goes to its parent's pos + scale * dir.  pos holds
// the roots' positions on entry, every joint's on return.  Every lane of the wave has to call this.
__device__ __forceinline__ void sw_walk(const int* __restrict__ bones, int NB, int J, int mine, double scale, const double* dir,
                                        double* pos) {
  for (int b = 0; b < NB; ++b) {
    const int p = bones[2 * b + 1];
    if (p < 0 || p >= J) continue;       // (the same for every lane)
    const double p0 = shfl_d(pos[0], p), p1 = shfl_d(pos[1], p), p2 = shfl_d(pos[2], p);
    if (b == mine) pos[0] = p0 + scale * dir[0], pos[1] = p1 + scale * dir[1], pos[2] = p2 + scale * dir[2];
  }
}

// Joint ``lane``'s three columns of a row of J joints; the lanes behind the row store nothing.
__device__ __forceinline__ void sw_store(float* __restrict__ row, int J, int lane, const double* pos) {
  if (lane < J)
    for (int i = 0; i < 3; ++i) row[3 * lane + i] = (float)pos[i];
}

// *count = the lanes whose ``fell`` is set: the bones of a frame that took their fallback.  Every lane of the wave has to call this.
__device__ __forceinline__ void sw_count(int* __restrict__ count, int lane, bool fell) {
  const int n = __popcll(__ballot(fell));
  if (lane == 0) *count = n;
}
