// CPU check of the arithmetic of mmego_blend_bones / mmego_bone_length_dev (mmego_amd/csrc/bone_blend_math.h), lane by lane as the
// kernels of blend_bones.hip call it -- the wave shuffle of the walk being a read of the parent lane's slot -- under the host sanitizers,
// against long-double sums written independently here.  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/bone_blend_host_check.hip -o bone_blend_host_check && ./bone_blend_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_bone_blend_gpu.py).  Exit status 0: all inside, every blended
// bone within 2e-6 of its length, single covers copied bit for bit, the padding columns untouched, the designed fallback counted.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/bone_blend_math.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static double worst = 0.0, worst_len = 0.0;
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

struct Tree {
  int J, NB;
  std::vector<int> bones;                                  // (child, parent) in walk order
};
static const Tree upper = {15, 14, {3, 14, 2, 3, 1, 2, 4, 2, 8, 2, 5, 4, 6, 5, 7, 6, 9, 8, 10, 9, 11, 10, 0, 1, 12, 0, 13, 0}};
static const Tree lower = {8, 6, {1, 0, 2, 1, 3, 2, 5, 4, 6, 5, 7, 6}};
static const Tree chain = {21, 20, {1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6, 8, 7, 9, 8, 10, 9, 11, 10, 12, 11, 13, 12, 14, 13, 15, 14,
                                    16, 15, 17, 16, 18, 17, 19, 18, 20, 19}};
static const Tree lone = {1, 0, {}};

static void random_unit(double u[3]) {
  double n;
  do {
    for (int i = 0; i < 3; ++i) u[i] = 2.0 * uniform() - 1.0;
    n = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  } while (n < 0.1 || n > 1.0);
  for (int i = 0; i < 3; ++i) u[i] /= n;
}

// one frame as blend_bones_kernel computes it, lane by lane; -> the frame's fallback count
static int frame(const Tree& t, const std::vector<float>& src, long nrows, const int* row, const float* w, long long k0, long long k1,
                 const std::vector<float>& len, float* dst, float* spread) {
  const int J = t.J, C = 3 * J;
  std::vector<double> pos(64 * 3, 0.0), u(64 * 3, 0.0), L(64, 0.0), q(64, 0.0);
  std::vector<int> mine(64, -1), fell(64, 0);
  double W = 0.0;
  int n = 0;
  long one = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const int j = lane < J ? lane : 0;
    int parent = -1;
    for (int b = 0; b < t.NB; ++b)
      if (t.bones[2 * b] == j) mine[lane] = b, parent = t.bones[2 * b + 1];
    double s[3], best[3];
    bb_gather(src.data(), nrows, C, row, w, k0, k1, j, parent, s, best, &W, &n, &one);
    if (n == 1 && W != 0.0) {
      for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = (double)src[one * C + 3 * j + i];
    } else if (n >= 1 && W != 0.0) {
      if (mine[lane] >= 0) {
        L[lane] = (double)len[mine[lane]];
        fell[lane] = bb_direction(s, best, W, L[lane], &u[lane * 3]);
      } else {
        double ws;
        for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = bl_blend_col(src.data(), nrows, C, row, w, k0, k1, 3 * j + i, &ws);
      }
    }
  }
  if (n > 1 && W != 0.0)
    for (int b = 0; b < t.NB; ++b) {                       // the walk: every lane reads lane p's slot, the child's lane takes it
      const int p = t.bones[2 * b + 1];
      for (int lane = 0; lane < J; ++lane)
        if (mine[lane] == b)
          for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = pos[p * 3 + i] + L[lane] * u[lane * 3 + i];
    }
  int count = 0;
  for (int lane = 0; lane < J; ++lane) {
    for (int i = 0; i < 3; ++i) {
      dst[3 * lane + i] = (float)pos[lane * 3 + i];
      q[lane] += bl_spread_col(src.data(), nrows, C, row, w, k0, k1, 3 * lane + i, pos[lane * 3 + i]);
    }
    count += fell[lane];
  }
  *spread = bl_spread(butterfly(q), W, C);
  return count;
}

static int check_blend(const Tree& t, long F, long nrows, int weights, long pad) {
  const int J = t.J, C = 3 * J;
  std::vector<float> len(t.NB ? t.NB : 1);
  for (auto& l : len) l = (float)(0.05 + 0.5 * uniform());
  std::vector<float> src((size_t)nrows * C);
  std::vector<int> is_child(J, 0);
  for (int b = 0; b < t.NB; ++b) is_child[t.bones[2 * b]] = 1;
  for (long r = 0; r < nrows; ++r) {                       // rigid rows: roots within 3 m, every bone a random direction of its length
    std::vector<double> p((size_t)C);
    for (int j = 0; j < J; ++j)
      if (!is_child[j])
        for (int i = 0; i < 3; ++i) p[3 * j + i] = 6.0 * uniform() - 3.0;
    for (int b = 0; b < t.NB; ++b) {
      double u[3];
      random_unit(u);
      for (int i = 0; i < 3; ++i) p[3 * t.bones[2 * b] + i] = p[3 * t.bones[2 * b + 1] + i] + (double)len[b] * u[i];
    }
    for (int c = 0; c < C; ++c) src[(size_t)r * C + c] = (float)p[c];
  }
  std::vector<long long> off(F + 1, 0);
  std::vector<int> row;
  std::vector<float> w;
  for (long f = 0; f < F; ++f) {
    const int n = f == 0 ? 0 : (f == 1 ? 1 : (int)(uniform() * 22.0));           // an empty frame, a single cover, 0 .. 21
    for (int k = 0; k < n; ++k) {
      row.push_back(f == 2 && k == 0 ? (int)nrows : (f == 3 && k == 0 ? -1 : (int)(uniform() * (double)nrows)));     // two rows outside: skipped
      const int p = k % 20;
      w.push_back(weights == 0 ? 1.0f : (weights == 1 ? (float)(p + 1 < 20 - p ? p + 1 : 20 - p) : (float)(0.5 + 1.5 * uniform())));
    }
    off[f + 1] = (long long)row.size();
  }
  if (row.empty()) row.push_back(0), w.push_back(1.0f);                            // (an address for the empty list; never read)
  const long ldd = C + pad;
  std::vector<float> dst((size_t)F * ldd, -12345.0f), spread(F, -12345.0f);
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    const int fb = frame(t, src, nrows, row.data(), w.data(), off[f], off[f + 1], len, &dst[f * ldd], &spread[f]);
    // the reference, in long double
    std::vector<long long> ks;
    for (long long k = off[f]; k < off[f + 1]; ++k)
      if (row[k] >= 0 && row[k] < nrows) ks.push_back(k);
    long double W = 0.0L;
    for (long long k : ks) W += (long double)w[k];
    std::vector<long double> pos((size_t)C, 0.0L);
    if (ks.size() == 1) {
      for (int c = 0; c < C; ++c) {
        pos[c] = (long double)src[(size_t)row[ks[0]] * C + c];
        if (dst[f * ldd + c] != src[(size_t)row[ks[0]] * C + c]) ++bad;            // one cover: the row, bit for bit
      }
    } else if (ks.size() > 1) {
      for (int j = 0; j < J; ++j)
        if (!is_child[j])
          for (int i = 0; i < 3; ++i) {
            long double acc = 0.0L;
            for (long long k : ks) acc += (long double)w[k] * (long double)src[(size_t)row[k] * C + 3 * j + i];
            pos[3 * j + i] = acc / W;
          }
      for (int b = 0; b < t.NB; ++b) {
        const int c = t.bones[2 * b], p = t.bones[2 * b + 1];
        long double s[3] = {0.0L, 0.0L, 0.0L};
        for (long long k : ks)
          for (int i = 0; i < 3; ++i)
            s[i] += (long double)w[k] * ((long double)src[(size_t)row[k] * C + 3 * c + i] - (long double)src[(size_t)row[k] * C + 3 * p + i]);
        const long double n = sqrtl(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
        if (!(n > 1e-3L * W * (long double)len[b])) ++bad;                         // (random rows stay far from the fallback)
        for (int i = 0; i < 3; ++i) pos[3 * c + i] = pos[3 * p + i] + (long double)len[b] * s[i] / n;
        // the blended bone as stored: its length within two float-rounded endpoints of L
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) {
          const double d = (double)dst[f * ldd + 3 * c + i] - (double)dst[f * ldd + 3 * p + i];
          d2 += d * d;
        }
        const double e = std::fabs(std::sqrt(d2) - (double)len[b]);
        if (!(e <= worst_len)) worst_len = e;
      }
    }
    long double tot = 0.0L;
    for (int c = 0; c < C; ++c) {
      hold(dst[f * ldd + c], pos[c]);
      for (long long k : ks) {
        const long double d = (long double)src[(size_t)row[k] * C + c] - pos[c];
        tot += (long double)w[k] * d * d;
      }
    }
    hold(spread[f], W != 0.0L && tot > 0.0L ? sqrtl(tot / ((long double)J * W)) : 0.0L);
    if (fb != 0) ++bad;
    for (long c = C; c < ldd; ++c)
      if (dst[f * ldd + c] != -12345.0f) ++bad;                                    // the padding columns stay
    // the length table on the stored row
    for (int b = 0; b < t.NB; ++b) {
      const int c = t.bones[2 * b], p = t.bones[2 * b + 1];
      long double d2 = 0.0L;
      for (int i = 0; i < 3; ++i) {
        const long double d = (long double)dst[f * ldd + 3 * c + i] - (long double)dst[f * ldd + 3 * p + i];
        d2 += d * d;
      }
      hold((float)bb_length_dev(&dst[f * ldd], c, p, (double)len[b]), fabsl(sqrtl(d2) - (long double)len[b]));
    }
  }
  return bad;
}

// Two equal-weight rows whose first bone has exactly opposite differences (an offset of 0.25 along x, the parent at multiples of it):
// the sum cancels exactly, the bone takes the first row's direction, the fallback is counted once, the bone below is still placed.
static int check_fallback() {
  const Tree t = {3, 2, {1, 0, 2, 1}};
  std::vector<float> len = {0.25f, 0.5f};
  std::vector<float> src = {0.5f, 0.25f, -0.75f, 0.75f, 0.25f, -0.75f, 0.75f, 0.75f, -0.75f,      // bone 0: +x, bone 1: +y
                            0.5f, 0.25f, -0.75f, 0.25f, 0.25f, -0.75f, 0.25f, 0.25f, -0.25f};     // bone 0: -x, bone 1: +z
  std::vector<int> row = {0, 1};
  std::vector<float> w = {2.0f, 2.0f};
  std::vector<float> dst(9, -12345.0f);
  float spread;
  int bad = 0;
  if (frame(t, src, 2, row.data(), w.data(), 0, 2, len, dst.data(), &spread) != 1) ++bad;
  const double r = std::sqrt(0.5);
  const double want[9] = {0.5, 0.25, -0.75, 0.75, 0.25, -0.75, 0.75, 0.25 + 0.5 * r, -0.75 + 0.5 * r};
  for (int c = 0; c < 9; ++c) hold(dst[c], (long double)want[c]);
  w[1] = 3.0f;                                             // the second row weighs more: no cancellation, no fallback
  if (frame(t, src, 2, row.data(), w.data(), 0, 2, len, dst.data(), &spread) != 0) ++bad;
  hold(dst[3], 0.25L);
  // both differences zero as well: the zero vector, the child on its parent, no NaN
  std::vector<float> flat(18, 0.5f);
  w[1] = 2.0f;
  if (frame(t, flat, 2, row.data(), w.data(), 0, 2, len, dst.data(), &spread) != 2) ++bad;
  for (int c = 0; c < 9; ++c) hold(dst[c], 0.5L);
  return bad;
}

int main() {
  int bad = 0;
  const long Fs[] = {1, 4, 5, 67};
  const Tree* trees[] = {&upper, &lower, &chain, &lone};
  for (const Tree* t : trees)
    for (long F : Fs)
      for (int weights = 0; weights < 3; ++weights)
        for (long pad : {0L, 3L}) bad += check_blend(*t, F, 300, weights, pad);
  bad += check_fallback();
  std::printf("bone_blend_host_check: worst error / bound %.4f, worst bone length error %.3e, %d violations\n", worst, worst_len, bad);
  return (worst <= 1.0 && worst_len <= 2e-6 && bad == 0) ? 0 : 1;
}
