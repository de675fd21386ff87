// The arithmetic of mmego_colsum_groups and mmego_hist_groups (breakdown.hip), per lane, as host + device functions: the kernels call
// them once per lane, scripts/breakdown_host_check.hip calls them lane by lane on the CPU (under the host sanitizers) and compares with
// its own long-double sums and exact counts.  The recipe is the comment of the two entry points in include/mmego_hip.h.
#pragma once

#define BD_HD __host__ __device__ __forceinline__
#define BD_BLOCK 64                      // rows per block of the grouped sums: one group id per lane, one bit per row in the block's mask
#define BD_BATCH 8                       // rows of a block whose loads are in flight together

// Bit j of a block's mask is set where row r0 + j belongs to the group.  This adds column c of those rows to s in ascending row order,
// BD_BATCH loads at a time; a batch that runs out of rows re-reads its last row (in bounds) and selects the value out.
BD_HD double bd_add_block(double s, const float* __restrict__ X, long ldx, long r0, unsigned long long mask, int c) {
  while (mask) {
    float v[BD_BATCH];
    bool on[BD_BATCH];
    int j = 0;
#pragma unroll
    for (int k = 0; k < BD_BATCH; ++k) {
      on[k] = mask != 0ULL;
      if (on[k]) {
        j = __builtin_ctzll(mask);
        mask &= mask - 1ULL;
      }
      v[k] = X[(r0 + j) * ldx + c];
    }
#pragma unroll
    for (int k = 0; k < BD_BATCH; ++k)
      if (on[k]) s += (double)v[k];
  }
  return s;
}

// The mask of block r0 as the host sees it: row r0 + j < rows with group[r0 + j] == g.  (The kernel forms the same mask with one id per
// lane and a wave ballot.)
static inline unsigned long long bd_block_mask(const int* group, long rows, long r0, int g) {
  unsigned long long m = 0ULL;
  for (int j = 0; j < BD_BLOCK; ++j)
    if (r0 + j < rows && group[r0 + j] == g) m |= 1ULL << j;
  return m;
}

// The bin of a value: -1 (not binned: NaN or < 0), the last bin where x * inv_width >= nbins - 1 (+Inf too), else (int)(x * inv_width);
// the product in fp32, the overflow decided by comparison before any conversion.
BD_HD int bd_bin(float x, float inv_width, int nbins) {
  if (!(x >= 0.0f)) return -1;
  const float t = x * inv_width;
  if (t >= (float)(nbins - 1)) return nbins - 1;
  return (int)t;
}
