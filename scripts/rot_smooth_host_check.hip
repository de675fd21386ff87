// CPU check of the arithmetic of mmego_smooth_rot (mmego_amd/csrc/rot_smooth_math.h over smooth_math.h, rot_blend_math.h and
// quat_eig.h), lane by lane as smooth_rot_kernel of smooth.hip calls it -- the ballot being a loop over the lanes, wave_sum_d the xor
// butterfly, a wave shuffle a read of the other lane's slot -- under the host sanitizers, against long-double arithmetic written
// independently here: the coefficients from a Gaussian elimination of the normal equations on the abscissae k / H (not from
// cofactors), the filtered rotation by Newton's iteration for the polar factor of S = sum_k c_k A_k (X <- (X + X^-T) / 2), where the
// kernel takes a quaternion from Jacobi sweeps.  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/rot_smooth_host_check.hip -o rot_smooth_host_check && ./rot_smooth_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// The rows are those of tests/test_smooth_rot_gpu.py: per bone a base rotation times a rotation of at most 0.6 rad in every frame,
// quaternions rounded to float with random signs, roots N(0, 0.7), the tests' segment layout, H in {1, 3, 31}, D in {0, 1, 2}, the three
// weight tables.  Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7.  Exit status 0: all inside, every filtered bone within
// 2e-6 of its length, rows outside a segment or alone in one copied bit for bit with their quaternions, the padding columns untouched,
// no fallback on the random rows, the designed fallback counted.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/rot_smooth_math.h"

typedef long double ld;

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

static double worst = 0.0, worst_len = 0.0, worst_abs = 0.0, least_gap = 1e300;
static bool track_gap = true;                              // (off for the designed fallback, whose gap is 0)
static void hold(double out, ld ref) {
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
static void ref_coefs(const int* seg, const float* w, long F, long f, int H, int D, std::vector<int>& taps, std::vector<ld>& c) {
  taps.clear(), c.clear();
  for (int k = -H; k <= H; ++k)
    if (f + k >= 0 && f + k < F && seg[f] >= 0 && seg[f + k] == seg[f]) taps.push_back(k);
  const int n = (int)taps.size();
  if (n == 0) return;
  const int deg = D < n - 1 ? D : n - 1, m = deg + 1;
  ld M[3][4] = {{0}};
  for (int k : taps) {
    const ld x = (ld)k / (ld)H, wk = (ld)w[k + H];
    ld p[5] = {1.0L, x, x * x, x * x * x, x * x * x * x};
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
      const ld q = M[r][i] / M[i][i];
      for (int j = i; j <= m; ++j) M[r][j] -= q * M[i][j];
    }
  }
  for (int k : taps) {
    const ld x = (ld)k / (ld)H;
    ld v = 0.0L, p = 1.0L;
    for (int i = 0; i < m; ++i) v += M[i][m] / M[i][i] * p, p *= x;
    c.push_back((ld)w[k + H] * v);
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

struct Tree {
  int J, NB;
  std::vector<int> bones;                                  // (child, parent) in walk order
};
static const Tree upper = {15, 14, {3, 14, 2, 3, 1, 2, 4, 2, 8, 2, 5, 4, 6, 5, 7, 6, 9, 8, 10, 9, 11, 10, 0, 1, 12, 0, 13, 0}};
static const Tree lower = {8, 6, {1, 0, 2, 1, 3, 2, 5, 4, 6, 5, 7, 6}};

// a rotation of `angle` about a random axis (Rodrigues), row-major
static void rotation(double angle, ld R[9]) {
  double u[3], n;
  do {
    for (int i = 0; i < 3; ++i) u[i] = 2.0 * uniform() - 1.0;
    n = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  } while (n < 0.1 || n > 1.0);
  for (int i = 0; i < 3; ++i) u[i] /= n;
  const ld c = cosl((ld)angle), s = sinl((ld)angle), x = u[0], y = u[1], z = u[2];
  const ld M[9] = {c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s,
                   y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s,
                   z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)};
  for (int i = 0; i < 9; ++i) R[i] = M[i];
}
static void mul(const ld* A, const ld* B, ld* C, bool At = false) {      // C = A B, or A^T B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      ld s = 0.0L;
      for (int k = 0; k < 3; ++k) s += (At ? A[3 * k + i] : A[3 * i + k]) * B[3 * k + j];
      C[3 * i + j] = s;
    }
}
static ld det3(const ld* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
// the rotation nearest S (det S > 0, well conditioned): Newton's iteration for the orthogonal polar factor
static void polar(const ld* S, ld* Q) {
  ld X[9];
  for (int i = 0; i < 9; ++i) X[i] = S[i];
  for (int it = 0; it < 80; ++it) {
    const ld d = det3(X);
    const ld inv_t[9] = {(X[4] * X[8] - X[5] * X[7]) / d, (X[5] * X[6] - X[3] * X[8]) / d, (X[3] * X[7] - X[4] * X[6]) / d,
                         (X[2] * X[7] - X[1] * X[8]) / d, (X[0] * X[8] - X[2] * X[6]) / d, (X[1] * X[6] - X[0] * X[7]) / d,
                         (X[1] * X[5] - X[2] * X[4]) / d, (X[2] * X[3] - X[0] * X[5]) / d, (X[0] * X[4] - X[1] * X[3]) / d};
    for (int i = 0; i < 9; ++i) X[i] = 0.5L * (X[i] + inv_t[i]);
  }
  for (int i = 0; i < 9; ++i) Q[i] = X[i];
}
// (w, x, y, z) of a rotation matrix, its first non-zero component positive (Shepperd's branch of the largest component)
static void quaternion_of(const ld* R, ld* q) {
  const ld t = R[0] + R[4] + R[8];
  const ld c[4] = {t, R[0], R[4], R[8]};
  int k = 0;
  for (int i = 1; i < 4; ++i)
    if (c[i] > c[k]) k = i;
  if (k == 0) q[0] = 1 + t, q[1] = R[7] - R[5], q[2] = R[2] - R[6], q[3] = R[3] - R[1];
  else if (k == 1) q[0] = R[7] - R[5], q[1] = 1 + 2 * R[0] - t, q[2] = R[1] + R[3], q[3] = R[2] + R[6];
  else if (k == 2) q[0] = R[2] - R[6], q[1] = R[1] + R[3], q[2] = 1 + 2 * R[4] - t, q[3] = R[5] + R[7];
  else q[0] = R[3] - R[1], q[1] = R[2] + R[6], q[2] = R[5] + R[7], q[3] = 1 + 2 * R[8] - t;
  const ld n = sqrtl(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  ld lead = 0.0L;
  for (int i = 3; i >= 0; --i)
    if (q[i] != 0.0L) lead = q[i];
  for (int i = 0; i < 4; ++i) q[i] = (lead < 0.0L ? -q[i] : q[i]) / n;
}
// the recipe's matrix of a stored quaternion, in long double
static void matrix_of(const float* q, ld* A) {
  const ld w = q[0], x = q[1], y = q[2], z = q[3];
  const ld M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  for (int i = 0; i < 9; ++i) A[i] = M[i];
}
static ld angle_of(const ld* Q, const ld* A) {
  ld D[9];
  mul(Q, A, D, true);
  const ld v0 = 0.5L * (D[7] - D[5]), v1 = 0.5L * (D[2] - D[6]), v2 = 0.5L * (D[3] - D[1]);
  return atan2l(sqrtl(v0 * v0 + v1 * v1 + v2 * v2), 0.5L * (D[0] + D[4] + D[8] - 1.0L));
}

// one frame as smooth_rot_kernel computes it, lane by lane; -> the frame's fallback count
static int rot_frame(const Tree& t, const float* src, long lds, long F, long f, const float* quat, const int* seg, const float* w, int H,
                     int D, const std::vector<float>& body, float* dst, float* quat_out, float* moved, float* rot_moved) {
  const int J = t.J, NB = t.NB;
  double ck[64];
  const uint64_t mask = wave_coefs(seg, w, F, f, H, D, ck);
  const float* own = src + f * lds;
  if (__builtin_popcountll(mask) <= 1) {
    for (int c = 0; c < 3 * J; ++c) dst[c] = own[c];
    for (int i = 0; i < 4 * NB; ++i) quat_out[i] = quat[(size_t)f * NB * 4 + i];
    *moved = 0.0f, *rot_moved = 0.0f;
    return 0;
  }
  std::vector<double> pos(64 * 3, 0.0), lay(64 * 3, 0.0), q(64, 0.0), th2(64, 0.0);
  std::vector<int> mine(64, -1), fell(64, 0);
  for (int lane = 0; lane < J; ++lane) {
    for (int b = 0; b < NB; ++b)
      if (t.bones[2 * b] == lane) mine[lane] = b;
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, W = 0.0;
    for (int tp = 0; tp <= 2 * H; ++tp) {
      if (!((mask >> tp) & 1)) continue;
      const long g = f + tp - H;
      if (mine[lane] >= 0) {
        const float* v = quat + ((size_t)g * NB + mine[lane]) * 4;
        double A[9];
        rs_matrix(v[0], v[1], v[2], v[3], A);
        rs_acc(S, &W, ck[tp], A);
      } else {
        for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = sm_acc(pos[lane * 3 + i], ck[tp], src[g * lds + 3 * lane + i]);
      }
    }
    if (mine[lane] >= 0) {
      const float* v = quat + ((size_t)f * NB + mine[lane]) * 4;
      double A0[9], Q[9], qm[4], theta;
      rs_matrix(v[0], v[1], v[2], v[3], A0);
      fell[lane] = rs_mean(S, A0, W, qm, Q, &theta);
      br_lay(Q, &body[3 * mine[lane]], &lay[lane * 3]);
      th2[lane] = theta * theta;
      for (int i = 0; i < 4; ++i) quat_out[4 * mine[lane] + i] = (float)qm[i];
      double q4[4], second;                                // the gap the fallback rule looks at, for the summary line
      const double top = br_quat_of(S, q4, &second);
      if (track_gap && (top - second) / W < least_gap) least_gap = (top - second) / W;
      if (W > worst_abs) worst_abs = W;
    }
  }
  for (int b = 0; b < NB; ++b) {                           // the walk: every lane reads lane p's slot, the child's lane takes it
    const int p = t.bones[2 * b + 1];
    for (int lane = 0; lane < J; ++lane)
      if (mine[lane] == b)
        for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = pos[p * 3 + i] + lay[lane * 3 + i];
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
  *rot_moved = rs_rot_moved(butterfly(th2), NB);
  return count;
}

static int check_rot(const Tree& t, long F, int H, int D, int weights, int which, long pad) {
  const int J = t.J, C = 3 * J, NB = t.NB;
  const std::vector<int> seg = layout(F, which);
  const std::vector<float> w = table(H, weights);
  std::vector<float> body((size_t)NB * 3);
  std::vector<ld> len(NB);
  for (int b = 0; b < NB; ++b) {
    ld R[9];
    rotation(6.28 * uniform(), R);
    const double L = 0.05 + 0.5 * uniform();
    for (int i = 0; i < 3; ++i) body[3 * b + i] = (float)((double)R[3 * i] * L);
    len[b] = sqrtl((ld)body[3 * b] * body[3 * b] + (ld)body[3 * b + 1] * body[3 * b + 1] + (ld)body[3 * b + 2] * body[3 * b + 2]);
  }
  std::vector<ld> base((size_t)NB * 9);
  for (int b = 0; b < NB; ++b) rotation(6.28 * uniform(), &base[9 * b]);
  const long lds = C + pad, ldd = C + 2 * pad;
  std::vector<float> src((size_t)(F - 1) * lds + C), quat((size_t)F * NB * 4), dst((size_t)(F - 1) * ldd + C, -12345.0f),
      qout((size_t)F * NB * 4, -12345.0f), moved(F, -12345.0f), rmoved(F, -12345.0f);
  std::vector<int> is_child(J, 0);
  for (int b = 0; b < NB; ++b) is_child[t.bones[2 * b]] = 1;
  for (long f = 0; f < F; ++f) {
    std::vector<ld> p((size_t)C, 0.0L);
    for (int j = 0; j < J; ++j)
      if (!is_child[j])
        for (int i = 0; i < 3; ++i) p[3 * j + i] = 0.7 * normal();
    for (int b = 0; b < NB; ++b) {
      ld P[9], A[9], q[4];
      rotation(1.2 * uniform() - 0.6, P);
      mul(&base[9 * b], P, A);
      quaternion_of(A, q);
      const double sign = uniform() < 0.5 ? -1.0 : 1.0;
      for (int i = 0; i < 4; ++i) quat[((size_t)f * NB + b) * 4 + i] = (float)(sign * (double)q[i]);
      for (int i = 0; i < 3; ++i)
        p[3 * t.bones[2 * b] + i] = p[3 * t.bones[2 * b + 1] + i] + A[3 * i] * body[3 * b] + A[3 * i + 1] * body[3 * b + 1] + A[3 * i + 2] * body[3 * b + 2];
    }
    for (int c = 0; c < C; ++c) src[f * lds + c] = (float)p[c];
  }
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    if (rot_frame(t, src.data(), lds, F, f, quat.data(), seg.data(), w.data(), H, D, body, &dst[f * ldd], &qout[(size_t)f * NB * 4], &moved[f],
                  &rmoved[f]) != 0)
      ++bad;
    std::vector<int> taps;
    std::vector<ld> c;
    ref_coefs(seg.data(), w.data(), F, f, H, D, taps, c);
    if (taps.size() <= 1) {
      for (int k = 0; k < C; ++k)
        if (dst[f * ldd + k] != src[f * lds + k]) ++bad;   // the row, bit for bit
      for (int i = 0; i < 4 * NB; ++i)
        if (qout[(size_t)f * NB * 4 + i] != quat[(size_t)f * NB * 4 + i]) ++bad;
      if (moved[f] != 0.0f || rmoved[f] != 0.0f) ++bad;
      continue;
    }
    std::vector<ld> pos((size_t)C, 0.0L);
    for (int j = 0; j < J; ++j)
      if (!is_child[j])
        for (int i = 0; i < 3; ++i)
          for (size_t a = 0; a < taps.size(); ++a) pos[3 * j + i] += c[a] * (ld)src[(f + taps[a]) * lds + 3 * j + i];
    ld rtot = 0.0L;
    for (int b = 0; b < NB; ++b) {
      ld S[9] = {0}, A0[9], Q[9], qr[4];
      for (size_t a = 0; a < taps.size(); ++a) {
        ld A[9];
        matrix_of(&quat[((size_t)(f + taps[a]) * NB + b) * 4], A);
        for (int i = 0; i < 9; ++i) S[i] += c[a] * A[i];
      }
      polar(S, Q);
      quaternion_of(Q, qr);
      double lead = 0.0;
      for (int i = 3; i >= 0; --i) {
        const double v = (double)qout[((size_t)f * NB + b) * 4 + i];
        hold(v, qr[i]);
        if (v != 0.0) lead = v;
      }
      if (!(lead > 0.0)) ++bad;                            // canonical sign
      matrix_of(&quat[((size_t)f * NB + b) * 4], A0);
      const ld th = angle_of(Q, A0);
      rtot += th * th;
      const int ch = t.bones[2 * b], p = t.bones[2 * b + 1];
      for (int i = 0; i < 3; ++i)
        pos[3 * ch + i] = pos[3 * p + i] + Q[3 * i] * body[3 * b] + Q[3 * i + 1] * body[3 * b + 1] + Q[3 * i + 2] * body[3 * b + 2];
      double d2 = 0.0;                                     // the filtered bone as stored: within two float-rounded endpoints of its length
      for (int i = 0; i < 3; ++i) {
        const double d = (double)dst[f * ldd + 3 * ch + i] - (double)dst[f * ldd + 3 * p + i];
        d2 += d * d;
      }
      const double e = std::fabs(std::sqrt(d2) - (double)len[b]);
      if (!(e <= worst_len)) worst_len = e;
    }
    ld tot = 0.0L;
    for (int k = 0; k < C; ++k) {
      hold(dst[f * ldd + k], pos[k]);
      const ld d = pos[k] - (ld)src[f * lds + k];
      tot += d * d;
    }
    hold(moved[f], sqrtl(tot / (ld)J));
    hold(rmoved[f], sqrtl(rtot / (ld)NB));
  }
  for (long f = 0; f + 1 < F; ++f)
    for (long c = C; c < ldd; ++c)
      if (dst[f * ldd + c] != -12345.0f) ++bad;            // the padding columns stay
  return bad;
}

// Two frames of one segment under D = 0 and the box table of H = 1: both weigh their two valid taps 1 / 2 each.  Bone 0 is the identity
// in frame 0 and a half turn about z in frame 1: S = diag(0, 0, 1), the 4 x 4 matrix diag(1, -1, -1, 1), the two largest eigenvalues
// meet: each frame keeps its own rotation and counts one fallback; the bone below (the same rotation in both frames) is still placed.
static int check_fallback() {
  const Tree t = {3, 2, {1, 0, 2, 1}};
  const std::vector<float> body = {0.25f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f};
  const std::vector<float> quat = {1, 0, 0, 0, 1, 0, 0, 0, /* frame 1 */ 0, 0, 0, 1, 1, 0, 0, 0};
  const std::vector<float> src = {0.5f, 0.25f, -0.75f, 0.75f, 0.25f, -0.75f, 0.75f, 0.75f, -0.75f,
                                  1.0f, 0.25f, -0.75f, 0.75f, 0.25f, -0.75f, 0.75f, 0.75f, -0.75f};
  const std::vector<int> seg = {4, 4};
  const std::vector<float> w = {1.0f, 1.0f, 1.0f};
  std::vector<float> dst(18, -12345.0f), qout(16, -12345.0f), moved(2), rmoved(2);
  int bad = 0;
  track_gap = false;
  for (long f = 0; f < 2; ++f)
    if (rot_frame(t, src.data(), 9, 2, f, quat.data(), seg.data(), w.data(), 1, 0, body, &dst[9 * f], &qout[8 * f], &moved[f], &rmoved[f]) != 1)
      ++bad;
  const double want[18] = {0.75, 0.25, -0.75, 1.0, 0.25, -0.75, 1.0, 0.75, -0.75, 0.75, 0.25, -0.75, 0.5, 0.25, -0.75, 0.5, 0.75, -0.75};
  for (int c = 0; c < 18; ++c) hold(dst[c], (ld)want[c]);
  for (int i = 0; i < 16; ++i)
    if (qout[i] != quat[i]) ++bad;
  if (rmoved[0] != 0.0f || rmoved[1] != 0.0f) ++bad;
  track_gap = true;
  return bad;
}

int main() {
  int bad = 0;
  const long Fs[] = {1, 3, 64, 65, 257};
  const int Hs[] = {1, 3, 31};
  const Tree* trees[] = {&upper, &lower};
  for (const Tree* t : trees)
    for (long F : Fs)
      for (int H : Hs)
        for (int D = 0; D < 3; ++D)
          for (int weights = 0; weights < 3; ++weights)
            for (int which = 0; which < 2; ++which) bad += check_rot(*t, F, H, D, weights, which, (H + D) % 2 ? 3 : 0);
  bad += check_fallback();
  std::printf("rot_smooth_host_check: worst error / bound %.4f, largest sum |c_k| %.4f, least eigenvalue gap / sum |c_k| %.3f, "
              "worst bone length error %.3e, %d violations\n", worst, worst_abs, least_gap, worst_len, bad);
  return (worst <= 1.0 && worst_len <= 2e-6 && bad == 0) ? 0 : 1;
}
