// CPU check of the arithmetic of mmego_imu_jitter (mmego_amd/csrc/imu_noise_math.h), sample by sample as the kernel of imu_noise.hip
// calls it, under the host sanitizers, against long-double arithmetic written independently here (both rotation factors from the matrix
// exponential's own power series, their product and the compose in long double).  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/imu_noise_host_check.hip -o imu_noise_host_check && ./imu_noise_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_imu_noise_gpu.py).  Exit status 0: all inside; E = E_s E_w
// within 4e-15 of the long-double product of exponentials and orthonormal to 1e-14; a factor whose sigma is 0 left out exactly (E is
// the other factor's bits); no additive channel beyond 3.47 (bias + noise).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../mmego_amd/csrc/imu_noise_math.h"

static uint64_t rng_state = 0x2545F4914F6CDD1DULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}
// a draw as the kernel's: the centred sum of four uniforms scaled to unit variance, rounded to float
static float draw() { return (float)((uniform() + uniform() + uniform() + uniform() - 2.0) * std::sqrt(3.0)); }

static double worst = 0.0, worst_orth = 0.0, worst_E = 0.0, worst_move = 0.0;
static bool left_out = true;
static void hold(double out, long double ref) {
  const double r = std::fabs(out - (double)ref) / (std::ldexp(1.0, -23) * std::fabs((double)ref) + 1e-7);
  if (!(r <= worst)) worst = r;                            // (a NaN lands here too)
}

// exp([w]x) in long double: the power series sum_k [w]x^k / k!, 30 terms (|w| <= 1.1 here)
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
static void random_rotation(float* R) {
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

static long samples = 0;
// one sample under (noise_deg, bias_deg) on the orientation and (noise, bias) on both additive groups
static void one_sample(double noise_deg, double bias_deg, double noise, double bias) {
  std::vector<float> x(IN_CH), y(IN_CH), zs(9), zw(9);
  std::vector<double> E(9), F(9);
  random_rotation(x.data());
  for (int i = 9; i < IN_CH; ++i) x[i] = (float)(20.0 * uniform() - 10.0);
  for (int i = 0; i < 9; ++i) zs[i] = draw(), zw[i] = draw();
  const double nr = noise_deg * PN_RAD_PER_DEG, br = bias_deg * PN_RAD_PER_DEG;
  in_rotation(nr, zs.data(), br, zw.data(), E.data());
  pn_compose(E.data(), x.data(), y.data());
  for (int k = 0; k < 6; ++k) y[9 + k] = in_add(x[9 + k], bias, zw[3 + k], noise, zs[3 + k]);
  // a factor whose sigma is 0 is left out exactly: E is the other factor as pn_rotation alone makes it
  if (nr == 0.0 || br == 0.0) {
    if (nr == 0.0) pn_rotation(br, zw[0], zw[1], zw[2], F.data());
    else pn_rotation(nr, zs[0], zs[1], zs[2], F.data());
    left_out = left_out && std::memcmp(E.data(), F.data(), 9 * sizeof(double)) == 0;
  }
  const long double pi = 3.141592653589793238462643383279502884L;
  const long double sn = (long double)noise_deg * pi / 180.0L, sb = (long double)bias_deg * pi / 180.0L;
  const long double ws[3] = {sn * zs[0], sn * zs[1], sn * zs[2]}, ww[3] = {sb * zw[0], sb * zw[1], sb * zw[2]};
  long double Xs[9], Xw[9], X[9];
  expm(ws, Xs), expm(ww, Xw);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) X[3 * i + j] = Xs[3 * i] * Xw[j] + Xs[3 * i + 1] * Xw[3 + j] + Xs[3 * i + 2] * Xw[6 + j];
  for (int i = 0; i < 9; ++i) {
    const double e = std::fabs((double)((long double)E[i] - X[i]));
    if (!(e <= worst_E)) worst_E = e;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      hold(y[3 * i + j], X[3 * i] * x[j] + X[3 * i + 1] * x[3 + j] + X[3 * i + 2] * x[6 + j]);
      double g = 0.0;                                      // E E^T - I
      for (int k = 0; k < 3; ++k) g += E[3 * i + k] * E[3 * j + k];
      g = std::fabs(g - (i == j ? 1.0 : 0.0));
      if (!(g <= worst_orth)) worst_orth = g;
    }
  for (int k = 0; k < 6; ++k) {
    hold(y[9 + k], ((long double)x[9 + k] + (long double)bias * zw[3 + k]) + (long double)noise * zs[3 + k]);
    // the stated bound, with the output's own rounding (half an ulp of a value below 16) beside it
    const double m = (std::fabs((double)y[9 + k] - (double)x[9 + k]) - 1e-6) / (3.47 * (bias + noise));
    if (!(m <= worst_move)) worst_move = m;
  }
  ++samples;
}

int main() {
  // both factors, each alone, and either side of pn_rotation's series threshold (theta = sigma_rad |z|, |z| about 1.7)
  const double degs[][2] = {{1.0, 2.0}, {10.0, 10.0}, {1e-6, 1e-3}, {0.03, 0.04}, {0.0, 2.0}, {2.0, 0.0}, {0.5, 5.0}, {5.0, 1e-6}};
  const double adds[][2] = {{0.05, 0.02}, {0.0, 0.3}, {0.3, 0.0}, {1.0, 1.0}};
  for (auto& d : degs)
    for (int r = 0; r < 4000; ++r) one_sample(d[0], d[1], adds[r % 4][0], adds[r % 4][1]);
  const bool ok = worst <= 1.0 && worst_orth <= 1e-14 && worst_E <= 4e-15 && left_out && worst_move <= 1.0;
  std::printf("imu_noise_host_check: %ld samples, worst error %.3f of the bound, |E E^T - I| <= %.2e, |E - exp exp| <= %.2e, a zero sigma's "
              "factor %s, largest additive move %.3f of 3.47 (bias + noise): %s\n",
              samples, worst, worst_orth, worst_E, left_out ? "left out" : "NOT left out", worst_move, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
