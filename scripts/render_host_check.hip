// CPU check of the arithmetic of mmego_render_prims / mmego_render_raster (mmego_amd/csrc/render_math.h), called as the kernels of
// render.hip call it, under the host sanitizers.  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/render_host_check.hip -o render_host_check && ./render_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Exit status 0: on 2 000 random frames (a third with seg < 0, a tenth with a plane of zero normal, padding rows in the cloud) every
// one of the 134 + N records has twelve floats, the absent ones are all zero and the others finite with alpha > 0; the ring's 32
// vertices lie in the plane, 1 m from the foot point; and on 20 000 random records against random tiles: a record that rd_touches
// rejects covers no pixel centre of the tile (rd_cover is exactly 0 there), and a record rd_load rejects is one the recipe skips.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/render_math.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}
static double normal() {                                   // Box-Muller
  const double a = uniform(), b = uniform();
  return std::sqrt(-2.0 * std::log(1.0 - a)) * std::cos(6.283185307179586 * b);
}

int main() {
  int bad = 0;
  std::vector<float> ring(64);
  for (int k = 0; k < 32; ++k) ring[2 * k] = (float)std::cos(6.283185307179586 * k / 32.0), ring[2 * k + 1] = (float)std::sin(6.283185307179586 * k / 32.0);
  // the scene
  for (int frame = 0; frame < 2000; ++frame) {
    const int N = (int)(uniform() * 9.0);
    std::vector<float> pred(63), tgt(63), ground(4), cloud(6 * N + (N == 0)), cam(8), out(RD_REC);
    for (int i = 0; i < 63; ++i) tgt[i] = (float)(0.4 * normal() + (i % 3 == 0 ? 0.8 : 0.1)), pred[i] = tgt[i] + (float)(0.06 * normal());
    for (int i = 0; i < 4; ++i) ground[i] = (float)normal();
    const bool no_plane = frame % 10 == 3;
    if (no_plane) ground[0] = ground[1] = ground[2] = 0.0f;
    for (int i = 0; i < 6 * N; ++i) cloud[i] = (float)normal();
    const int pad = N ? (int)(uniform() * N) : -1;
    if (pad >= 0 && frame % 2) cloud[6 * pad] = cloud[6 * pad + 1] = cloud[6 * pad + 2] = 0.0f;
    for (int i = 0; i < 8; ++i) cam[i] = (float)(100.0 * normal());
    const int seg = frame % 3 == 1 ? -1 : frame;
    double p[4], foot[3], t0[3];
    const int has_plane = fl_plane(ground.data(), p);
    if (has_plane == (int)no_plane) ++bad;
    for (int k = 0; k < RD_FIXED + N; ++k) {
      rd_prim(k, N, pred.data(), tgt.data(), ground.data(), N ? cloud.data() : nullptr, seg, cam.data(), ring.data(), 1.0, out.data());
      const bool in_plane = k < 52, of_pred = (k >= 32 && k < 52) || k >= 93 + N, is_pad = k - 93 == pad && frame % 2 && k >= 93 && k < 93 + N;
      const bool absent = (in_plane && !has_plane) || (of_pred && seg < 0) || is_pad;
      bool zero = true, finite = true;
      for (int i = 0; i < RD_REC; ++i) zero = zero && out[i] == 0.0f, finite = finite && std::isfinite(out[i]);
      if (absent != zero || !finite || (!absent && !(out[5] > 0.0f)) || out[9] != 0.0f || out[10] != 0.0f || out[11] != 0.0f) ++bad;
    }
    if (has_plane) {                                       // the ring's vertices: in the plane, 1 m from the foot point
      double e1[3], e2[3];
      fl_load3(tgt.data(), t0), rd_drop(p, t0, foot), rd_ring_axes(p, e1, e2);
      for (int k = 0; k < 32; ++k) {
        double v[3];
        for (int i = 0; i < 3; ++i) v[i] = foot[i] + (double)ring[2 * k] * e1[i] + (double)ring[2 * k + 1] * e2[i];
        if (std::fabs(fl_height(p, v)) > 1e-9 || std::fabs(rd_dist3(v, foot) - 1.0) > 1e-6) ++bad;
      }
    }
  }
  // the compositor's cull: whatever it rejects covers nothing on the tile
  int culled = 0, skipped = 0;
  for (int n = 0; n < 20000; ++n) {
    std::vector<float> rec(RD_REC, 0.0f);
    for (int i = 0; i < 4; ++i) rec[i] = (float)(uniform() * 200.0 - 50.0);
    if (n % 3 == 0) rec[2] = rec[0], rec[3] = rec[1];
    rec[4] = n % 5 == 0 ? 0.0f : (float)(uniform() * 4.0), rec[5] = n % 7 == 0 ? 0.0f : 0.35f;
    if (n % 11 == 0) rec[n % 9] = n % 2 ? NAN : INFINITY;
    if (n % 13 == 0) rec[4] = -0.5f;
    for (int i = 6; i < 9; ++i) rec[i] = (float)(uniform() * 255.0);
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(rec[i]);
    RdPrim q;
    const bool ok = rd_load(rec.data(), &q);
    if (ok != (finite && rec[5] > 0.0f && rec[4] >= 0.0f)) ++bad;
    if (!ok) { ++skipped; continue; }
    const float x0 = 32.0f * (float)(int)(uniform() * 3.0) + 0.5f, y0 = 32.0f * (float)(int)(uniform() * 3.0) + 0.5f;
    if (rd_touches(q, x0, y0, x0 + 31.0f, y0 + 31.0f)) continue;
    ++culled;
    for (int y = 0; y < 32; ++y)
      for (int x = 0; x < 32; ++x)
        if (rd_cover(q, x0 + (float)x, y0 + (float)y) != 0.0f) ++bad;
  }
  std::printf("render_host_check: %d culled records, %d skipped, %d failures\n", culled, skipped, bad);
  return bad || culled < 1000 || skipped < 1000 ? 1 : 0;
}
