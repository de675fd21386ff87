// CPU check of the arithmetic of mmego_colsum_groups / mmego_hist_groups (mmego_amd/csrc/breakdown_math.h), lane by lane as the kernels
// of breakdown.hip call it, under the host sanitizers, against long-double sums and exact counts written independently here.  Needs no
// GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/breakdown_host_check.hip -o breakdown_host_check && ./breakdown_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every sum: |out - ref| <= 2^-23 (the group's sum of |x|) (tests/test_breakdown_kernels_gpu.py); counts and bins: equality.
// Exit status 0: all inside.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
#include "../mmego_amd/csrc/breakdown_math.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static double worst = 0.0;
static int bad = 0;

// kind 0: sorted ids; 1: shuffled; 2: shuffled with -1 and ids >= G mixed in; 3: every row outside
static void check_sums(long rows, int C, int G, int kind, long pad) {
  const long ldx = C + pad;
  std::vector<float> X((size_t)rows * ldx);
  std::vector<int> group(rows);
  for (long r = 0; r < rows; ++r) {
    int g = kind == 0 ? (int)(r * G / rows) : (int)(uniform() * G);
    if (kind == 2 && uniform() < 0.3) g = uniform() < 0.5 ? -1 : G + (int)(uniform() * 3.0);
    if (kind == 3) g = r & 1 ? -1 : G;
    if (G >= 3 && g == G - 2) g = G - 1;                  // (group G - 2 stays empty where there are that many)
    group[r] = g;
    const bool in = g >= 0 && g < G;
    for (long c = 0; c < ldx; ++c)                         // rows outside every group carry what must reach no sum
      X[(size_t)r * ldx + c] = in ? (float)(200.0 * uniform() - 100.0) : (c & 1 ? std::numeric_limits<float>::quiet_NaN() : INFINITY);
  }
  const long nblk = (rows + BD_BLOCK - 1) / BD_BLOCK;
  for (int g = 0; g < G; ++g) {
    long members = 0;
    for (int wave = 0; wave < 16; ++wave)
      for (long b = wave; b < nblk; b += 16) members += __builtin_popcountll(bd_block_mask(group.data(), rows, b * BD_BLOCK, g));
    long n_ref = 0;
    for (long r = 0; r < rows; ++r) n_ref += group[r] == g;
    if (members != n_ref || (G >= 3 && g == G - 2 && n_ref != 0)) ++bad;
    for (int lane = 0; lane < C; ++lane) {                 // the kernel's body, lane by lane
      double t = 0.0;
      for (int wave = 0; wave < 16; ++wave) {
        double s = 0.0;
        for (long b = wave; b < nblk; b += 16)
          s = bd_add_block(s, X.data(), ldx, b * BD_BLOCK, bd_block_mask(group.data(), rows, b * BD_BLOCK, g), lane);
        t += s;
      }
      const float out = (float)t;
      long double ref = 0.0L, mag = 0.0L;
      for (long r = 0; r < rows; ++r)
        if (group[r] == g) ref += (long double)X[(size_t)r * ldx + lane], mag += fabsl((long double)X[(size_t)r * ldx + lane]);
      if (n_ref == 0 && out != 0.0f) ++bad;
      const double err = std::fabs((double)out - (double)ref), bound = std::ldexp(1.0, -23) * (double)mag;
      const double ratio = err == 0.0 ? 0.0 : err / bound;
      if (!(ratio <= worst)) worst = ratio;                // (a NaN lands here too)
    }
  }
}

static void check_bins(int nbins, float inv_width) {
  std::vector<float> xs;
  for (int k = 0; k <= nbins + 2; ++k) {                   // on the edges (the product is exact for these inv_width), just beside them
    const float e = (float)k / inv_width;
    xs.push_back(e);
    xs.push_back(std::nextafterf(e, 0.0f));
    xs.push_back(std::nextafterf(e, INFINITY));
  }
  for (int i = 0; i < 2000; ++i) xs.push_back((float)((nbins + 3) * uniform() / inv_width));
  const float special[] = {0.0f, -0.0f, -1e-30f, -3.0f, INFINITY, -INFINITY, std::numeric_limits<float>::quiet_NaN(), 3e38f, 1e-45f};
  for (float s : special) xs.push_back(s);
  std::vector<long> hist(nbins, 0), ref(nbins, 0);
  long lost = 0, lost_ref = 0;
  for (float x : xs) {
    const int b = bd_bin(x, inv_width, nbins);
    if (b < -1 || b >= nbins) { ++bad; continue; }
    if (b < 0) ++lost; else ++hist[b];
    // the recipe again, in long double where the fp32 product is exact (the edge values) and by its own comparisons otherwise
    if (std::isnan(x) || x < 0.0f) { ++lost_ref; continue; }
    const float t = x * inv_width;
    int rb;
    if (std::isinf(t) || t >= (float)(nbins - 1)) rb = nbins - 1;
    else rb = (int)std::floor((double)t);
    ++ref[rb];
  }
  for (int i = 0; i < nbins; ++i) bad += hist[i] != ref[i];
  bad += lost != lost_ref;
}

int main() {
  for (long rows : {1L, 63L, 64L, 65L, 1025L, 5000L})
    for (int C : {1, 43, 64})
      for (int G : {1, 3, 13, 200})
        for (int kind = 0; kind < 4; ++kind) check_sums(rows, C, G, kind, kind & 1 ? 5 : 0);
  for (int nbins : {1, 2, 300, 4096})
    for (float inv_width : {1.0f, 16.0f, 2048.0f, 2000.0f}) check_bins(nbins, inv_width);
  std::printf("breakdown_host_check: worst error / bound %.4f, %d count, bin or zero-group violations\n", worst, bad);
  return (worst <= 1.0 && bad == 0) ? 0 : 1;
}
