// Dense inference's pictures (dense.dense_infer with render=..., mmego_amd/render.py): mmego_render_prims turns every frame -- the
// predicted and the recorded skeleton, the floor plane, the radar returns and a 2 x 4 camera -- into a table of 134 + N capsules and
// discs in pixel coordinates, in the layer order they are to be painted in; mmego_render_raster composites such tables into 8-bit RGB
// images, one workgroup per (image, 32 x 32 tile): cull 256 primitives at a time against the tile, compact the survivors in index order
// into LDS, composite them into four pixels per thread in registers, store 12 bytes per thread.  No atomics, every output byte has one
// owner, the order of the composite is the index order: two launches give the same bytes.  The arithmetic is render_math.h; the
// recipe is the comment of the two entry points in include/mmego_hip.h, tests/render_ref.py restates it in numpy.
#include "common.h"
#include "render_math.h"

#define RD_THREADS 256
#define RD_TILE 32
#define RD_WAVES (RD_THREADS / 64)

__global__ __launch_bounds__(RD_THREADS) void render_raster_kernel(const float* __restrict__ prims, int P, unsigned char* __restrict__ out,
                                                                   int W, int H, long row_pitch, long img_stride, int tiles_x, int tiles_y,
                                                                   float bg_r, float bg_g, float bg_b) {
  __shared__ RdPrim list[RD_THREADS];
  __shared__ int wave_n[RD_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long blk = blockIdx.x;
  const long img = blk / (tiles_x * tiles_y);
  const int tile = (int)(blk - img * (tiles_x * tiles_y));
  const int tx0 = (tile % tiles_x) * RD_TILE, ty0 = (tile / tiles_x) * RD_TILE;
  const int x = tx0 + 4 * (tid & 7), y = ty0 + (tid >> 3);         // the thread's four pixels: (x .. x + 3, y)
  const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
  const float bx0 = (float)tx0 + 0.5f, by0 = (float)ty0 + 0.5f;    // the tile's pixel centres
  const float bx1 = bx0 + (float)(RD_TILE - 1), by1 = by0 + (float)(RD_TILE - 1);
  const float* __restrict__ mine = prims + img * (long)P * RD_REC;
  float col[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) col[j][0] = bg_r, col[j][1] = bg_g, col[j][2] = bg_b;

  for (int p0 = 0; p0 < P; p0 += RD_THREADS) {
    const int p = p0 + tid;
    RdPrim q;
    bool keep = false;
    if (p < P) {
      float rec[RD_REC];
      const f32x4* src = (const f32x4*)(mine + (long)p * RD_REC);
      const f32x4 r0 = src[0], r1 = src[1], r2 = src[2];
      rec[0] = r0.x, rec[1] = r0.y, rec[2] = r0.z, rec[3] = r0.w, rec[4] = r1.x, rec[5] = r1.y, rec[6] = r1.z, rec[7] = r1.w, rec[8] = r2.x;
      rec[9] = rec[10] = rec[11] = 0.0f;
      keep = rd_load(rec, &q) && rd_touches(q, bx0, by0, bx1, by1);
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RD_WAVES; ++w) {
      const int n = wave_n[w];
      off += w < wave ? n : 0;
      total += n;
    }
    if (keep) list[off + __popcll(mask & ((1ULL << lane) - 1ULL))] = q;
    __syncthreads();
    for (int i = 0; i < total; ++i) {                              // (every lane reads the same address: an LDS broadcast)
      const RdPrim s = list[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) rd_over(s, rd_cover(s, cx + (float)j, cy), col[j]);
    }
    __syncthreads();                                               // (the next round overwrites the list and the counts)
  }

  if (x < W && y < H) {                                            // (W % 4 == 0: the four pixels are inside together)
    unsigned b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[3 * j + c] = rd_byte(col[j][c]);
    unsigned* dst = (unsigned*)(out + img * img_stride + (long)y * row_pitch + 3L * x);
#pragma unroll
    for (int d = 0; d < 3; ++d) dst[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  }
}

__global__ __launch_bounds__(RD_THREADS) void render_prims_kernel(const float* __restrict__ pred, long ldp, const float* __restrict__ tgt,
                                                                  long ldt, const float* __restrict__ ground,
                                                                  const float* __restrict__ cloud, int N, const int* __restrict__ seg,
                                                                  const float* __restrict__ cam, const float* __restrict__ ring, long F,
                                                                  double vmax, float* __restrict__ prims) {
  const int P = RD_FIXED + N;
  const long i = (long)blockIdx.x * RD_THREADS + threadIdx.x;
  if (i >= F * P) return;
  const long f = i / P;
  const int k = (int)(i - f * P);
  float o[RD_REC];
  rd_prim(k, N, pred + f * ldp, tgt + f * ldt, ground + 4 * f, cloud + f * (long)N * 6, seg[f], cam + 8 * f, ring, vmax, o);
  f32x4* dst = (f32x4*)(prims + i * RD_REC);
  dst[0] = f32x4{o[0], o[1], o[2], o[3]}, dst[1] = f32x4{o[4], o[5], o[6], o[7]}, dst[2] = f32x4{o[8], o[9], o[10], o[11]};
}

extern "C" int mmego_render_raster(void* stream, const float* prims, int I, int P, unsigned char* out, int W, int H, long row_pitch,
                                   long img_stride, int bg_r, int bg_g, int bg_b) {
  MMEGO_REQUIRE(prims && out);
  MMEGO_REQUIRE(I >= 1 && P >= 0 && P <= RD_MAX_P);
  MMEGO_REQUIRE(W >= 16 && W <= 2048 && H >= 16 && H <= 2048 && W % 4 == 0);
  MMEGO_REQUIRE(row_pitch >= 3L * W && row_pitch % 4 == 0 && row_pitch < (1L << 40));
  MMEGO_REQUIRE(img_stride >= (long)H * row_pitch && img_stride % 4 == 0 && img_stride < (1L << 40));
  MMEGO_REQUIRE((uintptr_t)out % 4 == 0 && (uintptr_t)prims % 16 == 0);
  MMEGO_REQUIRE(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255);
  const int tiles_x = cdiv(W, RD_TILE), tiles_y = cdiv(H, RD_TILE);
  const long blocks = (long)I * tiles_x * tiles_y;
  MMEGO_REQUIRE(blocks < (1L << 31));
  hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, prims, P, out, W, H, row_pitch,
                     img_stride, tiles_x, tiles_y, (float)bg_r, (float)bg_g, (float)bg_b);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_render_prims(void* stream, const float* pred, long ldp, const float* tgt, long ldt, const float* ground,
                                  const float* cloud, int N, const int* seg, const float* cam, const float* ring, long F, double vmax,
                                  float* prims) {
  MMEGO_REQUIRE(pred && tgt && ground && seg && cam && ring && prims);
  MMEGO_REQUIRE(N >= 0 && N <= RD_MAX_P - RD_FIXED && (cloud || N == 0));
  MMEGO_REQUIRE(F >= 1 && F < (1L << 31) && ldp >= 3 * RD_JOINTS && ldt >= 3 * RD_JOINTS);
  MMEGO_REQUIRE(vmax > 0.0 && vmax <= 1.7976931348623157e308);    // (finite; false for a NaN)
  MMEGO_REQUIRE((uintptr_t)prims % 16 == 0);
  const long threads = F * (long)(RD_FIXED + N);                   // (< 2^41)
  const long blocks = (threads + RD_THREADS - 1) / RD_THREADS;
  MMEGO_REQUIRE(blocks < (1L << 31));
  hipLaunchKernelGGL(render_prims_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, pred, ldp, tgt, ldt, ground,
                     cloud, N, seg, cam, ring, F, vmax, prims);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
