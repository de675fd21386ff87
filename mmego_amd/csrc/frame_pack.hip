// Point clouds packed on the device: raw radar returns -> [pc_no][6] frames, a fresh random packing per output frame
// (data.pack_points' layout and distribution; data.FrameStore under --point_keep), with or without noise on every kept return
// (--point_noise, --point_noise_v).  The recipes are the comments of mmego_pack_frames and mmego_pack_frames_noise in
// include/mmego_hip.h; tests/frame_pack_ref.py and tests/point_noise_ref.py restate them in numpy.
#include "common.h"
#include "noise_draw.h"                  // fp_noise_z, FP_NOISE_SCALE: the draw mmego_pose_jitter shares

#define FP_WAVES 4                       // one wave per output frame, four per workgroup
#define FP_SALT_KEEP 0x4b454550u         // the launch's keep stream
#define FP_SALT_ORDER 0x4f524452u        // the launch's ordering stream
#define FP_SALT_NOISE 0x4e4f4953u        // the launch's noise stream (mmego_pack_frames_noise)

// one output row from one raw point: (x, y, z, intensity, velocity) -> (x, y, z, r, velocity, intensity)
__device__ __forceinline__ void fp_row(float* __restrict__ dst, const float* __restrict__ p) {
  const float x = p[0], y = p[1], z = p[2];
  float2* d = (float2*)dst;
  d[0] = make_float2(x, y);
  d[1] = make_float2(z, sqrtf(x * x + y * y + z * z));
  d[2] = make_float2(p[4], p[3]);
}

// fp_row of the perturbed point: x, y, z += sigma_xyz z_0..2 and velocity += sigma_v z_3, each as one rounded product and one rounded
// sum (no fma: tests/point_noise_ref.py restates the bits); a channel whose sigma is 0 is copied, so that a -0.0 keeps its sign.
__device__ __forceinline__ void fp_row_noise(float* __restrict__ dst, const float* __restrict__ p, unsigned b, float sigma_xyz,
                                             float sigma_v) {
  float v[5] = {p[0], p[1], p[2], p[3], p[4]};
  if (sigma_xyz != 0.f) {
#pragma unroll
    for (unsigned c = 0; c < 3; ++c) v[c] = __fadd_rn(v[c], __fmul_rn(sigma_xyz, fp_noise_z(b, c)));
  }
  if (sigma_v != 0.f) v[4] = __fadd_rn(v[4], __fmul_rn(sigma_v, fp_noise_z(b, 3)));
  fp_row(dst, v);
}

// LDS per wave: keys[m] (m = max(max_n, pc_no): the ordering keys of the slots, or of the survivors), then kept[max_n] (the
// survivors' point numbers in increasing order).  Every wave meets the two workgroup barriers, whatever its frame holds; a wave
// behind the last output frame packs an empty frame into its own LDS slice and writes nothing.
// NOISE (mmego_pack_frames_noise) differs at the row write only: the kept return j of output frame q is perturbed under key(KN, q, j).
// The sigmas come last, so that the plain instantiation reads the arguments it read before them.
template <bool NOISE>
__global__ __launch_bounds__(64 * FP_WAVES) void pack_frames_kernel(const float* __restrict__ pts, const long long* __restrict__ off,
                                                                   const long long* __restrict__ fidx, long nout, int pc_no, int max_n,
                                                                   int m, float keep_p, unsigned long long seed, float* __restrict__ out,
                                                                   float sigma_xyz, float sigma_v) {
  extern __shared__ unsigned fp_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* keys = fp_lds + (size_t)wave * (m + max_n);
  unsigned* kept = keys + m;
  const long q = (long)blockIdx.x * FP_WAVES + wave;
  const bool live = q < nout;
  long base = 0;
  int n = 0;                             // the frame's points, clamped to what the LDS slice holds: never past its CSR range
  if (live) {
    const long long f = fidx[q];
    base = (long)off[f];
    const long long c = off[f + 1] - off[f];
    n = c < 0 ? 0 : (c > max_n ? max_n : (int)c);
  }
  const unsigned hq = hash32((unsigned)q);
  const unsigned fk = hash32(dropout_key(seed, FP_SALT_KEEP) ^ hq), fo = hash32(dropout_key(seed, FP_SALT_ORDER) ^ hq);

  // keep: compact the survivors' numbers, 64 points a round (n is the same in every lane of the wave)
  int cnt = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const bool keep = j < n && (hash32(fk ^ (unsigned)j) >> 8) * (1.0f / 16777216.0f) < keep_p;
    const unsigned long long b = __ballot(keep);
    if (keep) kept[cnt + __popcll(b & ((1ULL << lane) - 1ULL))] = (unsigned)j;
    cnt += __popcll(b);
  }
  if (n > 0 && cnt == 0) {               // a frame is never emptied: the point that is first in the ordering stream stays
    unsigned bk = 0xffffffffu;
    int bj = 0x7fffffff;
    for (int j = lane; j < n; j += 64) {
      const unsigned k = hash32(fo ^ (unsigned)j);
      if (k < bk || (k == bk && j < bj)) bk = k, bj = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned k2 = __shfl_xor(bk, o, 64);
      const int j2 = __shfl_xor(bj, o, 64);
      if (k2 < bk || (k2 == bk && j2 < bj)) bk = k2, bj = j2;
    }
    if (lane == 0) kept[0] = (unsigned)bj;
    cnt = 1;
  }
  const bool sub = cnt >= pc_no;         // more survivors than slots: an ordered subsample; else: the survivors scattered over the slots
  const int items = sub ? cnt : pc_no;   // what is ranked: the survivors, or the slots (items <= m)
  __syncthreads();
  for (int i = lane; i < items; i += 64) keys[i] = hash32(fo ^ (sub ? kept[i] : (unsigned)i));
  __syncthreads();
  if (!live) return;

  // rank by counting: every lane compares its items' (key, index) with all of them (broadcast LDS reads).  Survivors are stored in
  // increasing point number, so the tie-break by position is the tie-break by point number.
  float* o = out + (size_t)q * pc_no * 6;
  const unsigned fn = NOISE ? hash32(dropout_key(seed, FP_SALT_NOISE) ^ hq) : 0u;
  auto row = [&](float* dst, unsigned j) {                         // the row of the frame's return j
    const float* p = pts + (base + j) * 5;
    if constexpr (NOISE) fp_row_noise(dst, p, hash32(fn ^ j), sigma_xyz, sigma_v);
    else fp_row(dst, p);
  };
  for (int i = lane; i < items; i += 64) {
    const unsigned k = keys[i];
    int r = 0;
    for (int t = 0; t < items; ++t) {
      const unsigned kt = keys[t];
      r += (kt < k || (kt == k && t < i)) ? 1 : 0;
    }
    if (sub) {
      if (r < pc_no) row(o + (size_t)r * 6, kept[i]);
    } else if (r < cnt) {
      row(o + (size_t)i * 6, kept[r]);
    } else {
      float2* d = (float2*)(o + (size_t)i * 6);
      d[0] = d[1] = d[2] = make_float2(0.f, 0.f);
    }
  }
}

// What both entry points refuse, and the launch: sigma 0, 0 without NOISE is mmego_pack_frames.
template <bool NOISE>
static int pack_frames_launch(void* stream, const float* pts, const long long* frame_off, const long long* frame_idx, long nout, int pc_no,
                              int max_n, float keep_p, unsigned long long seed, float sigma_xyz, float sigma_v, float* out) {
  MMEGO_REQUIRE(pts && frame_off && frame_idx && out && nout >= 1 && nout < (1L << 31));
  MMEGO_REQUIRE(pc_no >= 1 && pc_no <= 1024 && max_n >= 1 && max_n <= 16384);
  MMEGO_REQUIRE(keep_p > 0.f && keep_p <= 1.f);                    // (false for a NaN as well)
  MMEGO_REQUIRE((((uintptr_t)out) & 7) == 0);
  const int m = max_n > pc_no ? max_n : pc_no;
  const size_t lds = (size_t)FP_WAVES * (size_t)(m + max_n) * sizeof(unsigned);
  MMEGO_REQUIRE(lds <= 64 * 1024);
  if (int e = mmego_allow_lds<pack_frames_kernel<NOISE>>(lds)) return e;
  hipLaunchKernelGGL(pack_frames_kernel<NOISE>, dim3((unsigned)cdiv(nout, FP_WAVES)), dim3(64 * FP_WAVES), lds, (hipStream_t)stream, pts,
                     frame_off, frame_idx, nout, pc_no, max_n, m, keep_p, seed, out, sigma_xyz, sigma_v);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_pack_frames(void* stream, const float* pts, const long long* frame_off, const long long* frame_idx, long nout,
                                 int pc_no, int max_n, float keep_p, unsigned long long seed, float* out) {
  return pack_frames_launch<false>(stream, pts, frame_off, frame_idx, nout, pc_no, max_n, keep_p, seed, 0.f, 0.f, out);
}

extern "C" int mmego_pack_frames_noise(void* stream, const float* pts, const long long* frame_off, const long long* frame_idx, long nout,
                                       int pc_no, int max_n, float keep_p, unsigned long long seed, float sigma_xyz, float sigma_v,
                                       float* out) {
  MMEGO_REQUIRE(sigma_xyz >= 0.f && sigma_xyz < INFINITY && sigma_v >= 0.f && sigma_v < INFINITY);      // (false for a NaN as well)
  if (sigma_xyz == 0.f && sigma_v == 0.f)                          // nothing to add: the plain kernel, the same bytes
    return pack_frames_launch<false>(stream, pts, frame_off, frame_idx, nout, pc_no, max_n, keep_p, seed, 0.f, 0.f, out);
  return pack_frames_launch<true>(stream, pts, frame_off, frame_idx, nout, pc_no, max_n, keep_p, seed, sigma_xyz, sigma_v, out);
}
