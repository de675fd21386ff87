// CPU check of the arithmetic of mmego_blend_rot (mmego_amd/csrc/rot_blend_math.h with quat_eig.h), lane by lane as the kernel of
// blend_rot.hip calls it -- the wave shuffle of the walk being a read of the parent lane's slot -- under the host sanitizers, against
// long-double arithmetic written independently here: the mean rotation by Newton's iteration for the polar factor of the weighted sum
// (X <- (X + X^-T) / 2), where the kernel takes a quaternion from Jacobi sweeps.  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/rot_blend_host_check.hip -o rot_blend_host_check && ./rot_blend_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_rot_blend_gpu.py).  Exit status 0: all inside, every blended
// bone within 2e-6 of its length, single covers copied bit for bit, the padding columns untouched, the designed fallbacks counted.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../mmego_amd/csrc/rot_blend_math.h"

typedef long double ld;

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {                                  // splitmix64 -> [0, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static double worst = 0.0, worst_len = 0.0, least_gap = 1e300;
static bool track_gap = true;                              // (off for the designed fallbacks, whose gap is 0)
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

struct Tree {
  int J, NB, NQ;
  std::vector<int> bones;                                  // (child, parent) in walk order
  std::vector<int> rot;                                    // which of a row's NQ rotations turns bone b
};
static const Tree upper = {15, 14, 14, {3, 14, 2, 3, 1, 2, 4, 2, 8, 2, 5, 4, 6, 5, 7, 6, 9, 8, 10, 9, 11, 10, 0, 1, 12, 0, 13, 0},
                           {3, 2, 1, 4, 8, 5, 6, 7, 9, 10, 11, 0, 12, 13}};
static const Tree lower = {8, 6, 6, {1, 0, 2, 1, 3, 2, 5, 4, 6, 5, 7, 6}, {0, 1, 2, 3, 4, 5}};
static const Tree chain = {21, 20, 23, {1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6, 8, 7, 9, 8, 10, 9, 11, 10, 12, 11, 13, 12, 14, 13, 15, 14,
                                        16, 15, 17, 16, 18, 17, 19, 18, 20, 19},
                           {22, 0, 21, 1, 20, 2, 19, 3, 18, 4, 17, 5, 16, 6, 15, 7, 14, 8, 13, 9}};

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
  for (int it = 0; it < 60; ++it) {
    const ld d = det3(X);
    const ld inv_t[9] = {(X[4] * X[8] - X[5] * X[7]) / d, (X[5] * X[6] - X[3] * X[8]) / d, (X[3] * X[7] - X[4] * X[6]) / d,
                         (X[2] * X[7] - X[1] * X[8]) / d, (X[0] * X[8] - X[2] * X[6]) / d, (X[1] * X[6] - X[0] * X[7]) / d,
                         (X[1] * X[5] - X[2] * X[4]) / d, (X[2] * X[3] - X[0] * X[5]) / d, (X[0] * X[4] - X[1] * X[3]) / d};
    for (int i = 0; i < 9; ++i) X[i] = 0.5L * (X[i] + inv_t[i]);
  }
  for (int i = 0; i < 9; ++i) Q[i] = X[i];
}
// (w, x, y, z) of a rotation matrix, its first non-zero component positive
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
static ld angle_of(const ld* Q, const ld* A) {
  ld D[9];
  mul(Q, A, D, true);
  const ld v0 = 0.5L * (D[7] - D[5]), v1 = 0.5L * (D[2] - D[6]), v2 = 0.5L * (D[3] - D[1]);
  return atan2l(sqrtl(v0 * v0 + v1 * v1 + v2 * v2), 0.5L * (D[0] + D[4] + D[8] - 1.0L));
}

// one frame as blend_rot_kernel computes it, lane by lane; -> the frame's fallback count
static int frame(const Tree& t, const std::vector<float>& src, const std::vector<float>& q, const std::vector<float>& Rh, long nrows,
                 const int* row, const float* w, long long k0, long long k1, const std::vector<float>& body, float* dst, float* quat,
                 float* spread, float* rot_spread) {
  const int J = t.J, C = 3 * J;
  std::vector<double> pos(64 * 3, 0.0), lay(64 * 3, 0.0), Q(64 * 9, 0.0), qm(64 * 4, 0.0), sp(64, 0.0), rs(64, 0.0);
  std::vector<int> mine(64, -1), ri(64, -1), fell(64, 0);
  double W = 0.0;
  int n = 0;
  long one = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const bool joint = lane < J;
    const int j = joint ? lane : 0;
    for (int b = 0; b < t.NB; ++b)
      if (joint && t.bones[2 * b] == j) mine[lane] = b, ri[lane] = t.rot[b];
    double S[9], best[9];
    br_gather(q.data(), Rh.data(), nrows, t.NQ, row, w, k0, k1, ri[lane], S, best, &W, &n, &one);
    const bool covered = n >= 1 && W != 0.0;
    if (covered && mine[lane] >= 0) {
      fell[lane] = br_mean(S, best, W, &qm[lane * 4]);
      br_matrix(&qm[lane * 4], &Q[lane * 9]);
      br_lay(&Q[lane * 9], &body[3 * mine[lane]], &lay[lane * 3]);
      // the gap the fallback rule looks at, for the summary line
      double q4[4], second;
      const double top = br_quat_of(S, q4, &second);
      if (track_gap && (top - second) / W < least_gap) least_gap = (top - second) / W;
    }
    if (covered && n == 1) {
      for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = (double)src[one * C + 3 * j + i];
    } else if (covered && mine[lane] < 0) {
      double ws;
      for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = bl_blend_col(src.data(), nrows, C, row, w, k0, k1, 3 * j + i, &ws);
    }
  }
  const bool covered = n >= 1 && W != 0.0;
  if (covered && n > 1)
    for (int b = 0; b < t.NB; ++b) {                       // the walk: every lane reads lane p's slot, the child's lane takes it
      const int p = t.bones[2 * b + 1];
      for (int lane = 0; lane < J; ++lane)
        if (mine[lane] == b)
          for (int i = 0; i < 3; ++i) pos[lane * 3 + i] = pos[p * 3 + i] + lay[lane * 3 + i];
    }
  int count = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const bool joint = lane < J;
    const int j = joint ? lane : 0;
    if (joint)
      for (int i = 0; i < 3; ++i) {
        dst[3 * lane + i] = (float)pos[lane * 3 + i];
        sp[lane] += bl_spread_col(src.data(), nrows, C, row, w, k0, k1, 3 * j + i, pos[lane * 3 + i]);
      }
    if (mine[lane] >= 0) {
      for (int i = 0; i < 4; ++i) quat[4 * mine[lane] + i] = (float)qm[lane * 4 + i];
      if (covered && n > 1) rs[lane] = br_spread_bone(q.data(), Rh.data(), nrows, t.NQ, row, w, k0, k1, ri[lane], &Q[lane * 9]);
      count += fell[lane];
    }
  }
  *spread = bl_spread(butterfly(sp), W, C);
  *rot_spread = br_rot_spread(butterfly(rs), W, t.NB);
  return count;
}

static int check_blend(const Tree& t, long F, long nrows, int weights, long pad) {
  const int J = t.J, C = 3 * J, NB = t.NB, NQ = t.NQ;
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
  std::vector<float> src((size_t)nrows * C), q((size_t)nrows * NQ * 9), Rh((size_t)nrows * 9);
  std::vector<int> is_child(J, 0);
  for (int b = 0; b < NB; ++b) is_child[t.bones[2 * b]] = 1;
  for (long r = 0; r < nrows; ++r) {                       // rows as the nets make them: q = Rh G_b P, joints by FK in the world frame
    ld H[9];
    rotation(6.28 * uniform(), H);
    for (int i = 0; i < 9; ++i) Rh[(size_t)r * 9 + i] = (float)H[i];
    for (int k = 0; k < NQ; ++k)
      for (int i = 0; i < 9; ++i) q[((size_t)r * NQ + k) * 9 + i] = (i % 4 == 0) ? 1.0f : 0.0f;
    std::vector<ld> p((size_t)C, 0.0L);
    for (int j = 0; j < J; ++j)
      if (!is_child[j])
        for (int i = 0; i < 3; ++i) p[3 * j + i] = 6.0 * uniform() - 3.0;
    for (int b = 0; b < NB; ++b) {
      ld P[9], A[9], HA[9];
      rotation(uniform() - 0.5, P);
      mul(&base[9 * b], P, A);
      mul(H, A, HA);
      for (int i = 0; i < 9; ++i) q[((size_t)r * NQ + t.rot[b]) * 9 + i] = (float)HA[i];
      for (int i = 0; i < 3; ++i)
        p[3 * t.bones[2 * b] + i] = p[3 * t.bones[2 * b + 1] + i] + A[3 * i] * body[3 * b] + A[3 * i + 1] * body[3 * b + 1] + A[3 * i + 2] * body[3 * b + 2];
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
  std::vector<float> dst((size_t)F * ldd, -12345.0f), quat((size_t)F * NB * 4, -12345.0f), spread(F, -12345.0f), rspread(F, -12345.0f);
  int bad = 0;
  for (long f = 0; f < F; ++f) {
    const int fb = frame(t, src, q, Rh, nrows, row.data(), w.data(), off[f], off[f + 1], body, &dst[f * ldd], &quat[(size_t)f * NB * 4],
                         &spread[f], &rspread[f]);
    // the reference, in long double
    std::vector<long long> ks;
    for (long long k = off[f]; k < off[f + 1]; ++k)
      if (row[k] >= 0 && row[k] < nrows) ks.push_back(k);
    ld W = 0.0L;
    for (long long k : ks) W += (ld)w[k];
    std::vector<ld> pos((size_t)C, 0.0L);
    ld rtot = 0.0L;
    if (!ks.empty()) {
      std::vector<ld> Qb((size_t)NB * 9);
      for (int b = 0; b < NB; ++b) {
        ld S[9] = {0};
        std::vector<ld> As;
        for (long long k : ks) {
          ld H[9], Qk[9], A[9];
          for (int i = 0; i < 9; ++i) H[i] = (ld)Rh[(size_t)row[k] * 9 + i], Qk[i] = (ld)q[((size_t)row[k] * NQ + t.rot[b]) * 9 + i];
          mul(H, Qk, A, true);
          for (int i = 0; i < 9; ++i) S[i] += (ld)w[k] * A[i], As.push_back(A[i]);
        }
        polar(S, &Qb[9 * b]);
        // the kernel's quaternion against the polar factor's (Shepperd's branch of the largest component), canonical sign
        double qd[4];
        for (int i = 0; i < 4; ++i) qd[i] = (double)quat[((size_t)f * NB + b) * 4 + i];
        ld qr[4];
        quaternion_of(&Qb[9 * b], qr);
        for (int i = 0; i < 4; ++i) hold(qd[i], qr[i]);
        const double lead = qd[0] != 0.0 ? qd[0] : (qd[1] != 0.0 ? qd[1] : (qd[2] != 0.0 ? qd[2] : qd[3]));
        if (!(lead > 0.0)) ++bad;
        if (ks.size() > 1)
          for (size_t k = 0; k < ks.size(); ++k) {
            const ld th = angle_of(&Qb[9 * b], &As[9 * k]);
            rtot += (ld)w[ks[k]] * th * th;
          }
      }
      if (ks.size() == 1) {
        for (int c = 0; c < C; ++c) {
          pos[c] = (ld)src[(size_t)row[ks[0]] * C + c];
          if (dst[f * ldd + c] != src[(size_t)row[ks[0]] * C + c]) ++bad;          // one cover: the row, bit for bit
        }
      } else {
        for (int j = 0; j < J; ++j)
          if (!is_child[j])
            for (int i = 0; i < 3; ++i) {
              ld acc = 0.0L;
              for (long long k : ks) acc += (ld)w[k] * (ld)src[(size_t)row[k] * C + 3 * j + i];
              pos[3 * j + i] = acc / W;
            }
        for (int b = 0; b < NB; ++b) {
          const int c = t.bones[2 * b], p = t.bones[2 * b + 1];
          for (int i = 0; i < 3; ++i)
            pos[3 * c + i] = pos[3 * p + i] + Qb[9 * b + 3 * i] * body[3 * b] + Qb[9 * b + 3 * i + 1] * body[3 * b + 1] + Qb[9 * b + 3 * i + 2] * body[3 * b + 2];
          double d2 = 0.0;                                                         // the blended bone as stored: within two float-rounded endpoints of its length
          for (int i = 0; i < 3; ++i) {
            const double d = (double)dst[f * ldd + 3 * c + i] - (double)dst[f * ldd + 3 * p + i];
            d2 += d * d;
          }
          const double e = std::fabs(std::sqrt(d2) - (double)len[b]);
          if (!(e <= worst_len)) worst_len = e;
        }
      }
    } else {
      for (int i = 0; i < NB * 4; ++i)
        if (quat[(size_t)f * NB * 4 + i] != 0.0f) ++bad;                           // no cover: zero quaternions
    }
    ld tot = 0.0L;
    for (int c = 0; c < C; ++c) {
      hold(dst[f * ldd + c], pos[c]);
      for (long long k : ks) {
        const ld d = (ld)src[(size_t)row[k] * C + c] - pos[c];
        tot += (ld)w[k] * d * d;
      }
    }
    hold(spread[f], W != 0.0L && tot > 0.0L ? sqrtl(tot / ((ld)J * W)) : 0.0L);
    hold(rspread[f], W != 0.0L && rtot > 0.0L ? sqrtl(rtot / ((ld)NB * W)) : 0.0L);
    if (ks.size() == 1 && rspread[f] != 0.0f) ++bad;
    if (fb != 0) ++bad;
    for (long c = C; c < ldd; ++c)
      if (dst[f * ldd + c] != -12345.0f) ++bad;                                    // the padding columns stay
  }
  return bad;
}

// I and a half turn about z at equal weight cancel to diag(0, 0, 2 w): the two largest eigenvalues meet, the bone takes the first
// entry's rotation and the fallback is counted once; at weights 2 : 3 the heavier entry wins without a fallback; the bone below is
// still placed.
static int check_fallback() {
  const Tree t = {3, 2, 2, {1, 0, 2, 1}, {0, 1}};
  std::vector<float> body = {0.25f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f};
  std::vector<float> Rh = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::vector<float> q = {1, 0, 0, 0, 1, 0, 0, 0, 1, /* bone 1 */ 1, 0, 0, 0, 1, 0, 0, 0, 1,
                          -1, 0, 0, 0, -1, 0, 0, 0, 1, /* bone 1 */ 1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::vector<float> src = {0.5f, 0.25f, -0.75f, 0.75f, 0.25f, -0.75f, 0.75f, 0.75f, -0.75f,
                            0.5f, 0.25f, -0.75f, 0.25f, 0.25f, -0.75f, 0.25f, 0.75f, -0.75f};
  std::vector<int> row = {0, 1};
  std::vector<float> w = {2.0f, 2.0f};
  std::vector<float> dst(9, -12345.0f), quat(8, -12345.0f);
  float spread, rspread;
  int bad = 0;
  track_gap = false;
  if (frame(t, src, q, Rh, 2, row.data(), w.data(), 0, 2, body, dst.data(), quat.data(), &spread, &rspread) != 1) ++bad;
  const double want[9] = {0.5, 0.25, -0.75, 0.75, 0.25, -0.75, 0.75, 0.75, -0.75};
  for (int c = 0; c < 9; ++c) hold(dst[c], (ld)want[c]);
  const float first[8] = {1, 0, 0, 0, 1, 0, 0, 0};
  for (int i = 0; i < 8; ++i)
    if (quat[i] != first[i]) ++bad;
  w[1] = 3.0f;                                             // the second row weighs more: its half turn, no fallback
  if (frame(t, src, q, Rh, 2, row.data(), w.data(), 0, 2, body, dst.data(), quat.data(), &spread, &rspread) != 0) ++bad;
  hold(dst[3], 0.25L);
  const float second[4] = {0, 0, 0, 1};
  for (int i = 0; i < 4; ++i) hold(quat[i], (ld)second[i]);
  return bad;
}

int main() {
  int bad = 0;
  const long Fs[] = {1, 4, 5, 67};
  const Tree* trees[] = {&upper, &lower, &chain};
  for (const Tree* t : trees)
    for (long F : Fs)
      for (int weights = 0; weights < 3; ++weights)
        for (long pad : {0L, 3L}) bad += check_blend(*t, F, 300, weights, pad);
  bad += check_fallback();
  std::printf("rot_blend_host_check: worst error / bound %.4f, worst bone length error %.3e, least eigenvalue gap / W over the random covers %.3f, %d violations\n",
              worst, worst_len, least_gap, bad);
  return (worst <= 1.0 && worst_len <= 2e-6 && bad == 0) ? 0 : 1;
}
