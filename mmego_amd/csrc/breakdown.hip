// The error breakdown of the evaluation passes (evaluation.breakdown_launches): a per-row table reduced BY A GROUP ID PER ROW (the
// frame's action, its recording), and integer histograms of its values (the distribution behind the percentiles and the PCK curve).
// Both kernels give one workgroup a whole output (a group's row of sums, one histogram), so nothing is shared between workgroups: no
// global atomics, no pre-zeroed output, no workspace.  Sums in double in a fixed order, one float store; counts are integers, LDS
// integer adds commute: two launches give the same bits.  The arithmetic per lane is breakdown_math.h; the recipe is the comment of the
// two entry points in include/mmego_hip.h, tests/breakdown_ref.py restates it in numpy.
#include "common.h"
#include "breakdown_math.h"

#define BD_MAX_C 64                      // one lane per column
#define BD_MAX_G 65535
#define BD_MAX_BINS 4096                 // one LDS counter per bin: 16 KB
#define GS_WAVES 16                      // grouped sums: one workgroup per group, the 64-row blocks dealt round-robin to 16 waves
#define HG_THREADS 1024                  // histogram: one workgroup per histogram

__global__ __launch_bounds__(64 * GS_WAVES) void colsum_groups_kernel(const float* __restrict__ X, long ldx, long rows, int C,
                                                                     const int* __restrict__ group, float* __restrict__ out, long ldo,
                                                                     float* __restrict__ count) {
  __shared__ double part[GS_WAVES][64];
  __shared__ int members[GS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x, c = lane < C ? lane : 0;      // (the lanes behind the row re-read column 0 and store nothing)
  const long nblk = (rows + BD_BLOCK - 1) / BD_BLOCK;
  // a lane's id of its row of the block; -1, which is no group, behind the table.  The next block's ids are fetched ahead of the sums.
  auto id_of = [&](long b) {
    const long r = b * BD_BLOCK + lane;
    return b < nblk && r < rows ? group[r] : -1;
  };
  double s = 0.0;
  int n = 0;
  int id = id_of(wave);
  for (long b = wave; b < nblk; b += GS_WAVES) {
    const int next = id_of(b + GS_WAVES);
    const unsigned long long mask = __ballot(id == g);
    n += __popcll(mask);
    s = bd_add_block(s, X, ldx, b * BD_BLOCK, mask, c);
    id = next;
  }
  part[wave][lane] = s;
  if (lane == 0) members[wave] = n;
  __syncthreads();
  if (wave == 0) {
    double t = 0.0;
    int m = 0;
#pragma unroll
    for (int w = 0; w < GS_WAVES; ++w) {
      t += part[w][lane];
      m += members[w];
    }
    if (lane < C) out[(long)g * ldo + lane] = (float)t;
    if (count && lane == 0) count[g] = (float)m;
  }
}

// One workgroup per histogram: blockIdx.x = g (pooled) or g C + c (per column).
__global__ __launch_bounds__(HG_THREADS) void hist_groups_kernel(const float* __restrict__ X, long ldx, long rows, int C,
                                                                const int* __restrict__ group, float inv_width, int nbins, int pool,
                                                                int* __restrict__ hist, int* __restrict__ dropped) {
  __shared__ int bins[BD_MAX_BINS];
  __shared__ int lost;
  const int tid = threadIdx.x;
  for (int i = tid; i < nbins; i += HG_THREADS) bins[i] = 0;
  if (tid == 0) lost = 0;
  __syncthreads();
  const int g = pool ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)C), col = pool ? 0 : (int)(blockIdx.x % (unsigned)C);
  const long n = pool ? rows * C : rows;                  // (pooled: the table's elements in row-major order, one per thread and round)
  for (long i = tid; i < n; i += HG_THREADS) {
    const long r = pool ? i / C : i;
    const int c = pool ? (int)(i - r * C) : col;
    if ((group ? group[r] : 0) != g) continue;
    const int b = bd_bin(X[r * ldx + c], inv_width, nbins);
    atomicAdd(b < 0 ? &lost : &bins[b], 1);
  }
  __syncthreads();
  for (int i = tid; i < nbins; i += HG_THREADS) hist[(long)blockIdx.x * nbins + i] = bins[i];
  if (tid == 0) dropped[blockIdx.x] = lost;
}

extern "C" int mmego_colsum_groups(void* stream, const float* X, long ldx, long rows, int C, const int* group, int G, float* out, long ldo,
                                   float* count) {
  MMEGO_REQUIRE(X && group && out);
  MMEGO_REQUIRE(rows >= 1 && rows < (1L << 24) && C >= 1 && C <= BD_MAX_C && ldx >= C && ldo >= C && G >= 1 && G <= BD_MAX_G);
  hipLaunchKernelGGL(colsum_groups_kernel, dim3((unsigned)G), dim3(64 * GS_WAVES), 0, (hipStream_t)stream, X, ldx, rows, C, group, out, ldo,
                     count);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_hist_groups(void* stream, const float* X, long ldx, long rows, int C, const int* group, int G, float inv_width,
                                 int nbins, int pool, int* hist, int* dropped) {
  MMEGO_REQUIRE(X && hist && dropped);
  MMEGO_REQUIRE(rows >= 1 && rows < (1L << 24) && C >= 1 && C <= BD_MAX_C && ldx >= C && G >= 1 && G <= BD_MAX_G && (group || G == 1));
  MMEGO_REQUIRE(nbins >= 1 && nbins <= BD_MAX_BINS && (pool == 0 || pool == 1));
  MMEGO_REQUIRE(inv_width > 0.0f && inv_width < INFINITY);         // (false for NaN as well)
  hipLaunchKernelGGL(hist_groups_kernel, dim3((unsigned)(pool ? G : G * C)), dim3(HG_THREADS), 0, (hipStream_t)stream, X, ldx, rows, C,
                     group, inv_width, nbins, pool, hist, dropped);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
