// CPU check of the arithmetic of mmego_smooth_frames / mmego_smooth_bones (mmego_amd/csrc/smooth_math.h), lane by lane as the kernels
// of smooth.hip call it -- the ballot being a loop over the lanes, wave_sum_d the xor butterfly, a wave shuffle a read of the other
// lane's slot -- under the host sanitizers, against long-double sums written independently here (the coefficients from a Gaussian
// elimination of the normal equations on the abscissae k / H, not from cofactors).  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/smooth_host_check.hip -o smooth_host_check && ./smooth_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_smooth_gpu.py).  Exit status 0: all inside, every filtered bone
// within 2e-6 of its length, rows outside a segment or alone in one copied bit for bit, the padding columns untouched, the roots of the
// bones form equal to the column form's bits, the designed fallback counted.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/smooth_math.h"

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

static double worst = 0.0, worst_len = 0.0, worst_coef = 0.0, worst_abs = 0.0;
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

// sm_wave_coefs of smooth.hip, lane by lane: -> c_k per lane, the mask of the valid taps
static uint64_t wave_coefs(const int* seg, const float* w, long F, long f, int H, int D, double ck[64]) {
  uint64_t mask = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const long g = f + lane - H;
    if (lane <= 2 * H && g >= 0 && g < F && seg[f] >= 0 && seg[g] == seg[f]) mask |= 1ULL << lane;
    ck[lane] = 0.0;
  }
  const int n = __builtin_popcountll(mask);
  if (n <= 1) return mask;
  const int deg = sm_degree(D, n);
  std::vector<std::vector<double>> t(5, std::vector<double>(64));
  std::vector<double> wk(64);
  for (int lane = 0; lane < 64; ++lane) {
    wk[lane] = (mask >> lane) & 1 ? (double)w[lane] : 0.0;
    double tl[5];
    sm_tap_moments(wk[lane], lane - H, tl);
    for (int m = 0; m < 5; ++m) t[m][lane] = tl[m];
  }
  double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, A[3];
  for (int m = 0; m <= 2 * deg; ++m) S[m] = butterfly(t[m]);
  sm_first_row(S, deg, A);
  for (int lane = 0; lane < 64; ++lane) ck[lane] = sm_coef(A, wk[lane], lane - H);
  return mask;
}

// the reference's coefficients in long double: the normal equations on x = k / H by Gaussian elimination with pivoting, e_0's solution
static void ref_coefs(const int* seg, const float* w, long F, long f, int H, int D, std::vector<int>& taps, std::vector<long double>& c) {
  taps.clear(), c.clear();
  for (int k = -H; k <= H; ++k)
    if (f + k >= 0 && f + k < F && seg[f] >= 0 && seg[f + k] == seg[f]) taps.push_back(k);
  const int n = (int)taps.size();
  if (n == 0) return;
  const int deg = D < n - 1 ? D : n - 1, m = deg + 1;
  long double M[3][4] = {{0}};
  for (int k : taps) {
    const long double x = (long double)k / (long double)H, wk = (long double)w[k + H];
    long double p[5] = {1.0L, x, x * x, x * x * x, x * x * x * x};
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) M[i][j] += wk * p[i + j];
  }
  M[0][m] = 1.0L;                                          // M a = e_0: a is the first column (= row) of the inverse
  for (int i = 0; i < m; ++i) {
    int piv = i;
    for (int r = i + 1; r < m; ++r)
      if (fabsl(M[r][i]) > fabsl(M[piv][i])) piv = r;
    for (int j = 0; j <= m; ++j) std::swap(M[i][j], M[piv][j]);
    for (int r = 0; r < m; ++r) {
      if (r == i) continue;
      const long double q = M[r][i] / M[i][i];
      for (int j = i; j <= m; ++j) M[r][j] -= q * M[i][j];
    }
  }
  for (int k : taps) {
    const long double x = (long double)k / (long double)H;
    long double v = 0.0L, p = 1.0L;
    for (int i = 0; i < m; ++i) v += M[i][m] / M[i][i] * p, p *= x;
    c.push_back((long double)w[k + H] * v);
  }
}

// the segments of the tests: a segment of 1, one of 2, a gap, one that ends at frame 63, one that starts at 64, a gap, the rest;
// layout 1: one segment over all frames
static std::vector<int> layout(long F, int which) {
  std::vector<int> seg;
  const int ids[] = {5, 2, -1, 7, 1, -1, 3}, lens[] = {1, 2, 1, 60, 100, 2, 1 << 20};
  for (int p = 0; p < 7; ++p)
    for (int i = 0; i < lens[p] && (long)seg.size() < F; ++i) seg.push_back(which ? 0 : ids[p]);
  return seg;
}

static std::vector<float> table(int H, int weights) {
  std::vector<float> w(2 * H + 1);
  for (int k = -H; k <= H; ++k)
    w[k + H] = weights == 0 ? 1.0f : (weights == 1 ? (float)std::exp(-2.0 * k * k / (double)(H * H)) : (float)(0.5 + 1.5 * uniform()));
  return w;
}

static int check_frames(long F, int C, int H, int D, int weights, int which, long pad) {
  const std::vector<int> seg = layout(F, which);
  const std::vector<float> w = table(H, weights);
  const long lds = C + pad, ldd = C + 2 * pad;
  std::vector<float> src((size_t)(F - 1) * lds + C), dst((size_t)(F - 1) * ldd + C, -12345.0f), moved(F, -12345.0f);
  for (auto& x : src) x = (float)(0.7 * normal());
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    double ck[64];
    const uint64_t mask = wave_coefs(seg.data(), w.data(), F, f, H, D, ck);
    const int n = __builtin_popcountll(mask);
    std::vector<int> taps;
    std::vector<long double> c;
    ref_coefs(seg.data(), w.data(), F, f, H, D, taps, c);
    if ((int)taps.size() != n) ++bad;
    if (n >= 2) {
      long double sum = 0.0L, sabs = 0.0L;
      for (size_t i = 0; i < taps.size(); ++i) {
        const double e = std::fabs(ck[taps[i] + H] - (double)c[i]);
        if (!(e <= worst_coef)) worst_coef = e;
        sum += c[i], sabs += fabsl(c[i]);
      }
      if (fabsl(sum - 1.0L) > 1e-13L) ++bad;
      if ((double)sabs > worst_abs) worst_abs = (double)sabs;
    }
    std::vector<double> q(64, 0.0);
    long double tot = 0.0L;
    for (int lane = 0; lane < C; ++lane) {                 // lane = column
      const float own = src[f * lds + lane];
      if (n <= 1) {
        dst[f * ldd + lane] = own;
        if (dst[f * ldd + lane] != src[f * lds + lane]) ++bad;
        continue;
      }
      double y = 0.0;
      for (int t = 0; t <= 2 * H; ++t)
        if ((mask >> t) & 1) y = sm_acc(y, ck[t], src[(f + t - H) * lds + lane]);
      dst[f * ldd + lane] = (float)y;
      q[lane] = (y - (double)own) * (y - (double)own);
      long double r = 0.0L;
      for (size_t i = 0; i < taps.size(); ++i) r += c[i] * (long double)src[(f + taps[i]) * lds + lane];
      hold(dst[f * ldd + lane], r);
      tot += (r - (long double)own) * (r - (long double)own);
    }
    if (C % 3 == 0) {
      moved[f] = n <= 1 ? 0.0f : sm_moved(butterfly(q), C);
      hold(moved[f], sqrtl(tot / (long double)(C / 3)));
      if (n <= 1 && moved[f] != 0.0f) ++bad;
    }
  }
  for (long f = 0; f + 1 < F; ++f)
    for (long c = C; c < ldd; ++c)
      if (dst[f * ldd + c] != -12345.0f) ++bad;            // the padding columns stay
  return bad;
}

struct Tree {
  int J, NB;
  std::vector<int> bones;                                  // (child, parent) in walk order
};
static const Tree upper = {15, 14, {3, 14, 2, 3, 1, 2, 4, 2, 8, 2, 5, 4, 6, 5, 7, 6, 9, 8, 10, 9, 11, 10, 0, 1, 12, 0, 13, 0}};
static const Tree lower = {8, 6, {1, 0, 2, 1, 3, 2, 5, 4, 6, 5, 7, 6}};
static const Tree lone = {1, 0, {}};

// one frame as smooth_bones_kernel computes it, lane by lane; -> the frame's fallback count
static int bones_frame(const Tree& t, const float* src, long lds, long F, long f, const int* seg, const float* w, int H, int D,
                       const std::vector<float>& len, float* dst, float* moved) {
  const int J = t.J;
  double ck[64];
  const uint64_t mask = wave_coefs(seg, w, F, f, H, D, ck);
  const float* own = src + f * lds;
  if (__builtin_popcountll(mask) <= 1) {
    for (int c = 0; c < 3 * J; ++c) dst[c] = own[c];
    *moved = 0.0f;
    return 0;
  }
  std::vector<double> pos(64 * 3, 0.0), u(64 * 3, 0.0), L(64, 0.0), q(64, 0.0);
  std::vector<int> mine(64, -1), fell(64, 0);
  for (int lane = 0; lane < J; ++lane) {
    int parent = -1;
    for (int b = 0; b < t.NB; ++b)
      if (t.bones[2 * b] == lane) mine[lane] = b, parent = t.bones[2 * b + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int tp = 0; tp <= 2 * H; ++tp) {
      if (!((mask >> tp) & 1)) continue;
      const float* x = src + (f + tp - H) * lds;
      for (int i = 0; i < 3; ++i) {
        if (mine[lane] >= 0) s[i] += ck[tp] * ((double)x[3 * lane + i] - (double)x[3 * parent + i]);
        else pos[lane * 3 + i] = sm_acc(pos[lane * 3 + i], ck[tp], x[3 * lane + i]);
      }
    }
    if (mine[lane] >= 0) {
      L[lane] = (double)len[mine[lane]];
      const double best[3] = {(double)own[3 * lane] - (double)own[3 * parent], (double)own[3 * lane + 1] - (double)own[3 * parent + 1],
                              (double)own[3 * lane + 2] - (double)own[3 * parent + 2]};
      fell[lane] = bb_direction(s, best, 1.0, L[lane], &u[lane * 3]);
    }
  }
  for (int b = 0; b < t.NB; ++b) {                         // the walk: every lane reads lane p's slot, the child's lane takes it
    const int p = t.bones[2 * b + 1];
    for (int lane = 0; lane < J; ++lane)
      if (mine[lane] == b)
        for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = pos[p * 3 + i] + L[lane] * u[lane * 3 + i];
  }
  int count = 0;
  for (int lane = 0; lane < J; ++lane) {
    for (int i = 0; i < 3; ++i) {
      dst[3 * lane + i] = (float)pos[lane * 3 + i];
      const double d = pos[lane * 3 + i] - (double)own[3 * lane + i];
      q[lane] += d * d;
    }
    count += fell[lane];
  }
  *moved = sm_moved(butterfly(q), 3 * J);
  return count;
}

static void random_unit(double u[3]) {
  double n;
  do {
    for (int i = 0; i < 3; ++i) u[i] = 2.0 * uniform() - 1.0;
    n = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  } while (n < 0.1 || n > 1.0);
  for (int i = 0; i < 3; ++i) u[i] /= n;
}

// Rigid rows that move slowly (a root that drifts, bone directions that turn by a small step a frame), so that no filtered direction
// comes near the fallback; D <= 1 here keeps every coefficient positive.
static int check_bones(const Tree& t, long F, int H, int D, int weights, int which, long pad) {
  const int J = t.J, C = 3 * J;
  const std::vector<int> seg = layout(F, which);
  const std::vector<float> w = table(H, weights);
  std::vector<float> len(t.NB ? t.NB : 1);
  for (auto& l : len) l = (float)(0.05 + 0.5 * uniform());
  const long lds = C + pad, ldd = C + 2 * pad;
  std::vector<float> src((size_t)(F - 1) * lds + C), dst((size_t)(F - 1) * ldd + C, -12345.0f), moved(F);
  std::vector<int> is_child(J, 0);
  for (int b = 0; b < t.NB; ++b) is_child[t.bones[2 * b]] = 1;
  std::vector<double> dir((size_t)(t.NB ? t.NB : 1) * 3), root((size_t)C);
  for (int b = 0; b < t.NB; ++b) random_unit(&dir[3 * b]);
  for (auto& r : root) r = 6.0 * uniform() - 3.0;
  for (long f = 0; f < F; ++f) {
    std::vector<double> p((size_t)C);
    for (int j = 0; j < J; ++j)
      if (!is_child[j])
        for (int i = 0; i < 3; ++i) p[3 * j + i] = (root[3 * j + i] += 0.02 * normal());
    for (int b = 0; b < t.NB; ++b) {
      double n = 0.0;
      for (int i = 0; i < 3; ++i) dir[3 * b + i] += 0.01 * normal(), n += dir[3 * b + i] * dir[3 * b + i];
      for (int i = 0; i < 3; ++i) dir[3 * b + i] /= std::sqrt(n);
      for (int i = 0; i < 3; ++i) p[3 * t.bones[2 * b] + i] = p[3 * t.bones[2 * b + 1] + i] + (double)len[b] * dir[3 * b + i];
    }
    for (int c = 0; c < C; ++c) src[f * lds + c] = (float)p[c];
  }
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    if (bones_frame(t, src.data(), lds, F, f, seg.data(), w.data(), H, D, len, &dst[f * ldd], &moved[f]) != 0) ++bad;
    std::vector<int> taps;
    std::vector<long double> c;
    ref_coefs(seg.data(), w.data(), F, f, H, D, taps, c);
    std::vector<long double> pos((size_t)C, 0.0L);
    if (taps.size() <= 1) {
      for (int k = 0; k < C; ++k) {
        pos[k] = (long double)src[f * lds + k];
        if (dst[f * ldd + k] != src[f * lds + k]) ++bad;   // the row, bit for bit
      }
      if (moved[f] != 0.0f) ++bad;
    } else {
      // the roots carry the column form's bits
      double ck[64];
      const uint64_t mask = wave_coefs(seg.data(), w.data(), F, f, H, D, ck);
      for (int j = 0; j < J; ++j)
        if (!is_child[j])
          for (int i = 0; i < 3; ++i) {
            double y = 0.0;
            for (int tp = 0; tp <= 2 * H; ++tp)
              if ((mask >> tp) & 1) y = sm_acc(y, ck[tp], src[(f + tp - H) * lds + 3 * j + i]);
            if (dst[f * ldd + 3 * j + i] != (float)y) ++bad;
            for (size_t a = 0; a < taps.size(); ++a) pos[3 * j + i] += c[a] * (long double)src[(f + taps[a]) * lds + 3 * j + i];
          }
      for (int b = 0; b < t.NB; ++b) {
        const int ch = t.bones[2 * b], p = t.bones[2 * b + 1];
        long double s[3] = {0.0L, 0.0L, 0.0L};
        for (size_t a = 0; a < taps.size(); ++a)
          for (int i = 0; i < 3; ++i)
            s[i] += c[a] * ((long double)src[(f + taps[a]) * lds + 3 * ch + i] - (long double)src[(f + taps[a]) * lds + 3 * p + i]);
        const long double n = sqrtl(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
        if (!(n > 1e-3L * (long double)len[b])) ++bad;     // (slow rows stay far from the fallback)
        for (int i = 0; i < 3; ++i) pos[3 * ch + i] = pos[3 * p + i] + (long double)len[b] * s[i] / n;
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) {
          const double d = (double)dst[f * ldd + 3 * ch + i] - (double)dst[f * ldd + 3 * p + i];
          d2 += d * d;
        }
        const double e = std::fabs(std::sqrt(d2) - (double)len[b]);
        if (!(e <= worst_len)) worst_len = e;
      }
    }
    long double tot = 0.0L;
    for (int k = 0; k < C; ++k) {
      hold(dst[f * ldd + k], pos[k]);
      const long double d = pos[k] - (long double)src[f * lds + k];
      tot += d * d;
    }
    hold(moved[f], sqrtl(tot / (long double)J));
  }
  for (long f = 0; f + 1 < F; ++f)
    for (long c = C; c < ldd; ++c)
      if (dst[f * ldd + c] != -12345.0f) ++bad;            // the padding columns stay
  return bad;
}

// A bone that reverses between two equally weighted taps under D = 0 (an offset of 0.25 along x, the parent at multiples of it): the
// sum cancels exactly, each frame keeps its own direction, the fallback is counted once a frame, the bone below is still placed.
static int check_fallback() {
  const Tree t = {3, 2, {1, 0, 2, 1}};
  const std::vector<float> len = {0.25f, 0.5f};
  const std::vector<float> src = {0.5f, 0.25f, -0.75f, 0.75f, 0.25f, -0.75f, 0.75f, 0.75f, -0.75f,       // bone 0: +x, bone 1: +y
                                  1.0f, 0.25f, -0.75f, 0.75f, 0.25f, -0.75f, 0.75f, 0.75f, -0.75f};      // bone 0: -x, bone 1: +y
  const std::vector<int> seg = {4, 4};
  const std::vector<float> w = {1.0f, 1.0f, 1.0f};
  std::vector<float> dst(18, -12345.0f), moved(2);
  int bad = 0;
  for (long f = 0; f < 2; ++f)
    if (bones_frame(t, src.data(), 9, 2, f, seg.data(), w.data(), 1, 0, len, &dst[9 * f], &moved[f]) != 1) ++bad;
  const double want[18] = {0.75, 0.25, -0.75, 1.0, 0.25, -0.75, 1.0, 0.75, -0.75, 0.75, 0.25, -0.75, 0.5, 0.25, -0.75, 0.5, 0.75, -0.75};
  for (int c = 0; c < 18; ++c) hold(dst[c], (long double)want[c]);
  // both frames the same degenerate row: the zero vector, the children on their parent, no NaN
  const std::vector<float> flat(18, 0.5f);
  for (long f = 0; f < 2; ++f)
    if (bones_frame(t, flat.data(), 9, 2, f, seg.data(), w.data(), 1, 2, len, &dst[9 * f], &moved[f]) != 2) ++bad;
  for (int c = 0; c < 18; ++c) hold(dst[c], 0.5L);
  return bad;
}

int main() {
  int bad = 0;
  const long Fs[] = {1, 3, 64, 65, 257};
  const int Cs[] = {24, 45, 63, 64}, Hs[] = {1, 3, 31};
  for (long F : Fs)
    for (int C : Cs)
      for (int H : Hs)
        for (int D = 0; D < 3; ++D)
          for (int weights = 0; weights < 3; ++weights)
            for (int which = 0; which < 2; ++which) bad += check_frames(F, C, H, D, weights, which, (C + H + D) % 2 ? 3 : 0);
  const Tree* trees[] = {&upper, &lower, &lone};
  for (const Tree* t : trees)
    for (long F : Fs)
      for (int H : Hs)
        for (int D = 0; D < 3; ++D)
          for (int weights = 0; weights < 3; ++weights)
            for (int which = 0; which < 2; ++which) bad += check_bones(*t, F, H, D, weights, which, (H + D) % 2 ? 3 : 0);
  bad += check_fallback();
  std::printf("smooth_host_check: worst error / bound %.4f, worst |c - c_ref| %.3e, largest sum |c_k| %.4f, worst bone length error %.3e, "
              "%d violations\n", worst, worst_coef, worst_abs, worst_len, bad);
  return (worst <= 1.0 && worst_coef <= 1e-12 && worst_len <= 2e-6 && bad == 0) ? 0 : 1;
}
