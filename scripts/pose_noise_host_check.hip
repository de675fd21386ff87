// CPU check of the arithmetic of mmego_pose_jitter (mmego_amd/csrc/pose_noise_math.h), row by row as the kernel of pose_noise.hip calls
// it, under the host sanitizers, against long-double arithmetic written independently here (the rotation from the matrix exponential's
// own power series, not from Rodrigues' closed form).  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/pose_noise_host_check.hip -o pose_noise_host_check && ./pose_noise_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_pose_noise_gpu.py).  Exit status 0: all inside, and on both sides
// of the series threshold E within 2e-15 of the long-double exponential (a few double roundings per entry) and orthonormal to 1e-14.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/pose_noise_math.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}
// a draw as the kernel's: the centred sum of four uniforms scaled to unit variance, rounded to float
static float draw() { return (float)((uniform() + uniform() + uniform() + uniform() - 2.0) * std::sqrt(3.0)); }

static double worst = 0.0, worst_orth = 0.0, worst_E = 0.0;
static void hold(double out, long double ref) {
  const double r = std::fabs(out - (double)ref) / (std::ldexp(1.0, -23) * std::fabs((double)ref) + 1e-7);
  if (!(r <= worst)) worst = r;                            // (a NaN lands here too)
}

// exp([w]x) in long double: the power series sum_k [w]x^k / k!, 30 terms (|w| <= 0.6 here)
static void expm(const long double w[3], long double E[9]) {
  const long double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  long double term[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 9; ++i) E[i] = term[i];
  for (int k = 1; k <= 30; ++k) {
    long double next[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) next[3 * i + j] = (term[3 * i] * K[j] + term[3 * i + 1] * K[3 + j] + term[3 * i + 2] * K[6 + j]) / k;
    for (int i = 0; i < 9; ++i) term[i] = next[i], E[i] += next[i];
  }
}

// a random rotation in floats: Gram-Schmidt of two random vectors and their cross product
static void random_rotation(float R[9]) {
  double a[3], b[3], c[3], n;
  do {
    for (int i = 0; i < 3; ++i) a[i] = 2.0 * uniform() - 1.0, b[i] = 2.0 * uniform() - 1.0;
    n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int i = 0; i < 3; ++i) a[i] /= n;
    const double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    for (int i = 0; i < 3; ++i) b[i] -= d * a[i];
    n = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  } while (n < 0.1);
  for (int i = 0; i < 3; ++i) b[i] /= n;
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
  for (int i = 0; i < 3; ++i) R[i] = (float)a[i], R[3 + i] = (float)b[i], R[6 + i] = (float)c[i];
}

static long rows = 0;
static void one_row(double sigma_deg, double sigma_t) {
  std::vector<float> R(9), t(3), z(6), Ro(9), to(3);
  std::vector<double> E(9);
  random_rotation(R.data());
  for (int i = 0; i < 3; ++i) t[i] = (float)(4.0 * uniform() - 2.0);
  for (int i = 0; i < 6; ++i) z[i] = draw();
  const double sr = sigma_deg * PN_RAD_PER_DEG;
  pn_rotation(sr, z[0], z[1], z[2], E.data());
  pn_compose(E.data(), R.data(), Ro.data());
  for (int i = 0; i < 3; ++i) to[i] = pn_shift(t[i], sigma_t, z[3 + i]);
  const long double pi = 3.141592653589793238462643383279502884L;
  const long double s = (long double)sigma_deg * pi / 180.0L;
  const long double w[3] = {s * z[0], s * z[1], s * z[2]};
  long double X[9];
  expm(w, X);
  for (int i = 0; i < 9; ++i) {
    const double e = std::fabs((double)((long double)E[i] - X[i]));
    if (!(e <= worst_E)) worst_E = e;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      hold(Ro[3 * i + j], X[3 * i] * R[j] + X[3 * i + 1] * R[3 + j] + X[3 * i + 2] * R[6 + j]);
      double g = 0.0;                                      // E E^T - I
      for (int k = 0; k < 3; ++k) g += E[3 * i + k] * E[3 * j + k];
      g = std::fabs(g - (i == j ? 1.0 : 0.0));
      if (!(g <= worst_orth)) worst_orth = g;
    }
  for (int i = 0; i < 3; ++i) hold(to[i], (long double)t[i] + (long double)sigma_t * z[3 + i]);
  ++rows;
}

int main() {
  // either side of the series threshold (theta = sigma_rad |z|, |z| about 1.7): 1e-6 .. 0.03 deg take the series, 0.04 .. 5 deg do not
  const double degs[] = {1e-6, 1e-3, 0.03, 0.04, 0.5, 1.0, 2.0, 5.0};
  for (double d : degs)
    for (int r = 0; r < 4000; ++r) one_row(d, r % 2 ? 0.02 : 0.05);
  // a zero rotation vector is the identity, exactly
  double E0[9];
  pn_rotation(0.3, 0.f, 0.f, 0.f, E0);
  bool ident = true;
  for (int i = 0; i < 9; ++i) ident = ident && E0[i] == (i % 4 == 0 ? 1.0 : 0.0);
  const bool ok = worst <= 1.0 && worst_orth <= 1e-14 && worst_E <= 2e-15 && ident;
  std::printf("pose_noise_host_check: %ld rows, worst error %.3f of the bound, |E E^T - I| <= %.2e, |E - exp| <= %.2e, zero vector %s: %s\n",
              rows, worst, worst_orth, worst_E, ident ? "identity" : "NOT identity", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
