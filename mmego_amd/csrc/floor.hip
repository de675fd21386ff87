// Dense inference's notion of the ground (dense.dense_infer, floor=(mode, contact_cm, margin_cm)): every frame of a recording
// carries the floor plane in the frame of its own joints, so the height of a joint is n . x + d and needs no head pose.
// mmego_floor_stats turns the two feet of a lower-joint row into 22 per-row figures (penetration, contact by height against the recorded
// flags, the same for the target as the noise floor) that ops.colsum sums; mmego_floor_clamp raises a leg whose foot or ankle lies
// under the plane, a two-bone solve that moves the ankle straight up along the normal, finds the knee on the circle both bone lengths
// allow, on the side it was on, and carries the foot bone along unturned: every bone keeps the length it had in that frame.
// Both are a few dozen floats per row: one thread per row, no LDS, no atomics, every output word has one owner, double inside, one
// float store.  The arithmetic is floor_math.h; the recipe is the comment of the two entry points in include/mmego_hip.h,
// tests/floor_ref.py restates it in numpy.
#include "common.h"
#include "floor_math.h"

#define FL_THREADS 256

__global__ __launch_bounds__(FL_THREADS) void floor_stats_kernel(const float* __restrict__ lo, long ldl, const float* __restrict__ tgt,
                                                                 long ldt, const float* __restrict__ ground,
                                                                 const float* __restrict__ contact, const int* __restrict__ seg, long rows,
                                                                 double H, float* __restrict__ out) {
  const long r = (long)blockIdx.x * FL_THREADS + threadIdx.x;
  if (r >= rows) return;
  float o[FLOOR_W];
  for (int i = 0; i < FLOOR_W; ++i) o[i] = 0.0f;
  double p[4];
  if (seg[r] >= 0 && fl_plane(ground + 4 * r, p)) {
    for (int k = 0; k < 2; ++k) {                                  // foot k: local joint 3 / 7, target joint 15 / 19
      double xp[3], xt[3];
      fl_load3(lo + r * ldl + 3 * (3 + 4 * k), xp);
      fl_load3(tgt + r * ldt + 3 * (15 + 4 * k), xt);
      fl_foot_stats(fl_height(p, xp), fl_height(p, xt), (double)contact[2 * r + k], H, o + 11 * k);
    }
  }
  for (int i = 0; i < FLOOR_W; ++i) out[r * FLOOR_W + i] = o[i];
}

// (src and dst are not __restrict__: dst may be src; a thread reads its whole row before it writes it, and no other thread's)
__global__ __launch_bounds__(FL_THREADS) void floor_clamp_kernel(const float* src, long lds, const float* __restrict__ ground,
                                                                 const int* __restrict__ seg, long rows, double margin, float* dst, long ldd,
                                                                 float* __restrict__ lifted, int* __restrict__ fallback) {
  const long r = (long)blockIdx.x * FL_THREADS + threadIdx.x;
  if (r >= rows) return;
  float in[FL_COLS], o[FL_COLS];
  for (int i = 0; i < FL_COLS; ++i) o[i] = in[i] = src[r * lds + i];
  double p[4], up = 0.0;
  int fell = 0;
  if (seg[r] >= 0) {
    if (fl_plane(ground + 4 * r, p)) {
      for (int leg = 0; leg < 2; ++leg) {
        double l;
        fell += fl_leg(in + 12 * leg, p, margin, o + 12 * leg + 3, &l);
        if (l > up) up = l;
      }
    } else {
      fell = 2;
    }
  }
  for (int i = 0; i < FL_COLS; ++i) dst[r * ldd + i] = o[i];
  if (lifted) lifted[r] = (float)up;
  if (fallback) fallback[r] = fell;
}

extern "C" int mmego_floor_stats(void* stream, const float* lo, long ldl, const float* tgt, long ldt, const float* ground,
                                 const float* contact, const int* seg, long rows, double H, float* out) {
  MMEGO_REQUIRE(lo && tgt && ground && contact && seg && out);
  MMEGO_REQUIRE(rows >= 1 && rows < (1L << 31) && ldl >= FL_COLS && ldt >= 63);
  MMEGO_REQUIRE(H > 0.0 && H < 1e30);
  hipLaunchKernelGGL(floor_stats_kernel, dim3((unsigned)cdiv(rows, FL_THREADS)), dim3(FL_THREADS), 0, (hipStream_t)stream, lo, ldl, tgt,
                     ldt, ground, contact, seg, rows, H, out);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}

extern "C" int mmego_floor_clamp(void* stream, const float* src, long lds, const float* ground, const int* seg, long rows, double margin,
                                 float* dst, long ldd, float* lifted, int* fallback) {
  MMEGO_REQUIRE(src && ground && seg && dst);
  MMEGO_REQUIRE(rows >= 1 && rows < (1L << 31) && lds >= FL_COLS && ldd >= FL_COLS);
  MMEGO_REQUIRE(margin >= 0.0 && margin < 1e30);
  if (dst == src) {
    MMEGO_REQUIRE(ldd == lds);
  } else {                                                         // else the two share no byte
    const uintptr_t a0 = (uintptr_t)src, a1 = (uintptr_t)(src + (rows - 1) * lds + FL_COLS), b0 = (uintptr_t)dst,
                    b1 = (uintptr_t)(dst + (rows - 1) * ldd + FL_COLS);
    MMEGO_REQUIRE(!(a0 < b1 && b0 < a1));
  }
  hipLaunchKernelGGL(floor_clamp_kernel, dim3((unsigned)cdiv(rows, FL_THREADS)), dim3(FL_THREADS), 0, (hipStream_t)stream, src, lds, ground,
                     seg, rows, margin, dst, ldd, lifted, fallback);
  MMEGO_LAUNCH_CHECK();
  return MMEGO_OK;
}
