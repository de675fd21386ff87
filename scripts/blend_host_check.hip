// CPU check of the arithmetic of mmego_blend_windows / mmego_colsum_phase (mmego_amd/csrc/blend_math.h), lane by lane as the kernels of
// blend.hip call it, under the host sanitizers, against long-double sums written independently here.  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/blend_host_check.hip -o blend_host_check && ./blend_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_blend_gpu.py).  Exit status 0: all inside.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/blend_math.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static double worst = 0.0;
static void hold(double out, long double ref) {
  const double r = std::fabs(out - (double)ref) / (std::ldexp(1.0, -23) * std::fabs((double)ref) + 1e-7);
  if (!(r <= worst)) worst = r;                            // (a NaN lands here too)
}

// what wave_sum_d does: the xor butterfly over 64 lanes
static double butterfly(std::vector<double> v) {
  for (int o = 32; o > 0; o >>= 1) {
    std::vector<double> n(64);
    for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ o];
    v = n;
  }
  return v[0];
}

static int check_blend(long F, int C, long nrows, int weights, long pad) {
  std::vector<float> src((size_t)nrows * C);
  for (auto& x : src) x = (float)(2.0 * uniform() - 1.0);
  std::vector<long long> off(F + 1, 0);
  std::vector<int> row;
  std::vector<float> w;
  for (long f = 0; f < F; ++f) {
    const int n = f == 0 ? 0 : (f == 1 ? 1 : (int)(uniform() * 22.0));           // an empty frame, a single cover, 0 .. 21
    for (int k = 0; k < n; ++k) {
      row.push_back((int)(uniform() * (double)nrows));
      const int p = k % 20;
      w.push_back(weights == 0 ? 1.0f : (weights == 1 ? (float)(p + 1 < 20 - p ? p + 1 : 20 - p) : (float)(0.5 + 1.5 * uniform())));
    }
    off[f + 1] = (long long)row.size();
  }
  if (row.empty()) row.push_back(0), w.push_back(1.0f);                            // (an address for the empty list; never read)
  const long ldd = C + pad;
  std::vector<float> dst((size_t)F * ldd, -12345.0f), spread(F, -12345.0f);
  const bool with_spread = C % 3 == 0;
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    std::vector<double> s(64, 0.0);
    double wsum = 0.0;
    for (int lane = 0; lane < 64; ++lane) {                                        // the kernel's body, lane by lane
      const bool col = lane < C;
      const int c = col ? lane : 0;
      const double m = bl_blend_col(src.data(), nrows, C, row.data(), w.data(), off[f], off[f + 1], c, &wsum);
      if (col) dst[f * ldd + lane] = (float)m;
      if (with_spread && col) s[lane] = bl_spread_col(src.data(), nrows, C, row.data(), w.data(), off[f], off[f + 1], c, m);
    }
    if (with_spread) spread[f] = bl_spread(butterfly(s), wsum, C);
    // the reference
    long double ws = 0.0L, tot = 0.0L;
    for (long long k = off[f]; k < off[f + 1]; ++k) ws += (long double)w[k];
    for (int c = 0; c < C; ++c) {
      long double acc = 0.0L;
      for (long long k = off[f]; k < off[f + 1]; ++k) acc += (long double)w[k] * (long double)src[(size_t)row[k] * C + c];
      const long double m = ws != 0.0L ? acc / ws : 0.0L;
      hold(dst[f * ldd + c], m);
      for (long long k = off[f]; k < off[f + 1]; ++k) {
        const long double d = (long double)src[(size_t)row[k] * C + c] - m;
        tot += (long double)w[k] * d * d;
      }
      if (off[f + 1] - off[f] == 1 && dst[f * ldd + c] != src[(size_t)row[off[f]] * C + c]) ++bad;     // one cover: the row, bit for bit
    }
    if (with_spread) hold(spread[f], ws != 0.0L ? sqrtl(tot / ((long double)(C / 3) * ws)) : 0.0L);
    for (long c = C; c < ldd; ++c)
      if (dst[f * ldd + c] != -12345.0f) ++bad;                                    // the padding columns stay
  }
  return bad;
}

static void check_phase(int period, long n, int C, long pad) {
  const long rows = n * period, ldx = C + pad;
  std::vector<float> X((size_t)rows * ldx);
  for (auto& x : X) x = (float)(200.0 * uniform() - 100.0);
  std::vector<float> out((size_t)period * C);
  for (int p = 0; p < period; ++p)
    for (int lane = 0; lane < C; ++lane) {
      double s = 0.0;
      for (int wave = 0; wave < 16; ++wave) s += bl_phase_partial(X.data(), ldx, n, period, p, lane, wave, 16);
      out[(size_t)p * C + lane] = (float)s;
      long double ref = 0.0L;
      for (long i = 0; i < n; ++i) ref += (long double)X[(size_t)(i * period + p) * ldx + lane];
      hold(out[(size_t)p * C + lane], ref);
    }
}

int main() {
  int bad = 0;
  const long Fs[] = {1, 3, 64, 65, 257};
  const int Cs[] = {24, 45, 63, 64, 1};
  for (long F : Fs)
    for (int C : Cs)
      for (int weights = 0; weights < 3; ++weights)
        for (long pad : {0L, 3L}) bad += check_blend(F, C, 400, weights, pad);
  const int periods[] = {1, 8, 20, 64};
  const long ns[] = {1, 7, 1000};
  const int PCs[] = {1, 43, 45, 64};
  for (int period : periods)
    for (long n : ns)
      for (int C : PCs)
        for (long pad : {0L, 5L}) check_phase(period, n, C, pad);
  std::printf("blend_host_check: worst error / bound %.4f, %d exact-copy or padding violations\n", worst, bad);
  return (worst <= 1.0 && bad == 0) ? 0 : 1;
}
