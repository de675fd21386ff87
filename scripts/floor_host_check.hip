// CPU check of the arithmetic of mmego_floor_stats / mmego_floor_clamp (mmego_amd/csrc/floor_math.h), row by row as the kernels of
// floor.hip call it, under the host sanitizers, against a long-double solve written independently here (the knee from the law of
// cosines and a Gram-Schmidt frame, not from a and b).  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/floor_host_check.hip -o floor_host_check && ./floor_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Exit status 0: on 20 000 random legs every raised joint within 2e-5 m of the long-double solve where the knee stands 5 cm or more
// off the hip-ankle line, bone lengths kept to 2e-6 m, the foot bone's vector to 2e-7, no stored ankle or foot under the margin, the
// lift within 1e-6 m of the recipe's, legs above the margin copied bit for bit; the statistics' strict comparisons at h = 0 and h = H.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../mmego_amd/csrc/floor_math.h"

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

typedef long double ld;
static ld dot(const ld a[3], const ld b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

int main() {
  int bad = 0, lifted = 0, compared = 0, fell = 0;
  double worst = 0.0, worst_len = 0.0, worst_foot = 0.0, worst_lift = 0.0;
  for (int leg = 0; leg < 20000; ++leg) {
    std::vector<float> in(12), out(9), g(4);
    const double sig = 0.03 + 0.05 * uniform();
    double x[12] = {0.05 * normal(), 0.1 + 0.02 * normal(), 0.95 + 0.03 * normal()};
    const double step[3][3] = {{0.15, 0.0, -0.392}, {-0.13, 0.0, -0.357}, {0.12, 0.0, -0.16}};
    for (int j = 1; j < 4; ++j)
      for (int i = 0; i < 3; ++i) x[3 * j + i] = x[3 * j - 3 + i] + step[j - 1][i] + (j < 3 ? (i < 2 ? sig : 0.01) : 0.02) * normal();
    for (int i = 0; i < 12; ++i) in[i] = (float)x[i];
    g[0] = (float)(0.01 * normal()), g[1] = (float)(0.01 * normal()), g[2] = 1.0f, g[3] = (float)(-0.02 + 0.04 * normal());
    const double margin = leg % 2 ? 0.02 : 0.0;
    double p[4], lift;
    if (!fl_plane(g.data(), p)) { ++bad; continue; }
    const int fb = fl_leg(in.data(), p, margin, out.data(), &lift);
    fell += fb;
    ld P[4][3], n[3] = {(ld)g[0], (ld)g[1], (ld)g[2]};
    const ld nn = sqrtl(dot(n, n)), d = (ld)g[3] / nn;
    for (int i = 0; i < 3; ++i) n[i] /= nn;
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < 3; ++i) P[j][i] = (ld)in[3 * j + i];
    const ld hA = dot(n, P[2]) + d, hT = dot(n, P[3]) + d;
    ld want = 0.0L;
    if ((ld)margin - hT > want) want = (ld)margin - hT;
    if ((ld)margin - hA > want) want = (ld)margin - hA;
    if (want == 0.0L) {
      if (lift != 0.0 || fb || std::memcmp(out.data(), in.data() + 3, 9 * sizeof(float))) ++bad;
      continue;
    }
    ++lifted;
    if (fb) continue;
    // the recipe by another route: the angle at the hip from the law of cosines, in the frame (u, the knee's side)
    ld kh[3], ak[3], v[3], u[3], s[3];
    for (int i = 0; i < 3; ++i) kh[i] = P[1][i] - P[0][i], ak[i] = P[2][i] - P[1][i], v[i] = P[2][i] + want * n[i] - P[0][i];
    const ld l1 = sqrtl(dot(kh, kh)), l2 = sqrtl(dot(ak, ak)), D = sqrtl(dot(v, v));
    for (int i = 0; i < 3; ++i) u[i] = v[i] / D;
    const ld t = dot(kh, u);
    for (int i = 0; i < 3; ++i) s[i] = kh[i] - t * u[i];
    const ld sn = sqrtl(dot(s, s));
    const ld cosh = (l1 * l1 + D * D - l2 * l2) / (2.0L * l1 * D), sinh = sqrtl(1.0L - cosh * cosh);
    const bool conditioned = (double)(l1 * sinh) >= 0.05 && (double)sn >= 1e-3;
    double lenK = 0.0, lenA = 0.0, hmin = 1e30;
    for (int i = 0; i < 3; ++i) {
      const ld K2 = P[0][i] + l1 * (cosh * u[i] + sinh * s[i] / sn), A2 = P[0][i] + D * u[i], T2 = A2 + (P[3][i] - P[2][i]);
      if (conditioned) {
        worst = std::fmax(worst, std::fabs((double)out[i] - (double)K2));
        worst = std::fmax(worst, std::fabs((double)out[3 + i] - (double)A2));
        worst = std::fmax(worst, std::fabs((double)out[6 + i] - (double)T2));
      }
      const double dk = (double)out[i] - (double)in[i], da = (double)out[3 + i] - (double)out[i];
      lenK += dk * dk, lenA += da * da;
      worst_foot = std::fmax(worst_foot, std::fabs(((double)out[6 + i] - (double)out[3 + i]) - ((double)in[9 + i] - (double)in[6 + i])));
    }
    compared += conditioned;
    worst_len = std::fmax(worst_len, std::fmax(std::fabs(std::sqrt(lenK) - (double)l1), std::fabs(std::sqrt(lenA) - (double)l2)));
    worst_lift = std::fmax(worst_lift, std::fabs(lift - (double)want));
    for (int j = 1; j < 3; ++j) {
      const double xj[3] = {(double)out[3 * j], (double)out[3 * j + 1], (double)out[3 * j + 2]};
      hmin = std::fmin(hmin, fl_height(p, xj));
    }
    if (!(hmin >= margin)) ++bad;
  }
  // the statistics' comparisons are strict
  float st[11];
  fl_foot_stats(0.0, 0.0625, 1.0, 0.0625, st);
  if (st[2] != 0.0f || st[3] != 1.0f || st[4] != 1.0f || st[8] != 0.0f || st[9] != 0.0f || st[10] != 0.0f || st[0] != 0.0625f) ++bad;
  fl_foot_stats(-0.01, 0.03, 0.0, 0.0625, st);
  if (st[1] != 0.01f || st[2] != 1.0f || st[4] != 0.0f || st[5] != 0.0f || st[6] != 0.0f || st[7] != 0.0f || st[9] != 1.0f) ++bad;
  std::printf("%d legs lifted (%d compared, %d fallbacks): joints worst %.3e m, lengths %.3e, foot bone %.3e, lift %.3e; %d bad\n", lifted,
              compared, fell, worst, worst_len, worst_foot, worst_lift, bad);
  const bool ok = bad == 0 && lifted > 4000 && compared > 0.9 * lifted && worst <= 2e-5 && worst_len <= 2e-6 && worst_foot <= 2e-7 &&
                  worst_lift <= 1e-6;
  return ok ? 0 : 1;
}
