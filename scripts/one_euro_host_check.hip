// CPU check of the arithmetic of mmego_one_euro / mmego_one_euro_bones (mmego_amd/csrc/one_euro_math.h), step by step as the kernels of
// one_euro.hip call it -- one lane per joint, the walk's shuffle a read of the parent's slot -- under the host sanitizers, against a
// long-double recursion written independently here (plain multiplies and adds, no fma).  Needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/one_euro_host_check.hip -o one_euro_host_check && ./one_euro_host_check
// Every buffer is an exactly sized heap allocation, so a read or write one element outside is an AddressSanitizer report.
// Runs: random rows, a constant, a step, a ramp, and a skeleton one of whose bones reverses every frame at alpha = 1/2.
// Bound on every output: |out - ref| <= 2^-23 |ref| + 1e-7 (tests/test_one_euro_gpu.py).  Exit status 0: all inside, the constant run
// back bit for bit, every run's first row bit for bit, every filtered bone within 2e-6 of its length, the roots of the bones form equal
// to the column form's bits, the designed fallback counted by both sides in the frame the recursion cancels in (and in no other).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../mmego_amd/csrc/one_euro_math.h"

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

static double worst = 0.0, worst_len = 0.0;
static int failures = 0;
static void hold(double out, long double ref) {
  const double r = std::fabs(out - (double)ref) / (std::ldexp(1.0, -23) * std::fabs((double)ref) + 1e-7);
  if (!(r <= worst)) worst = r;                            // (a NaN lands here too)
}
static void expect(bool ok, const char* what) {
  if (!ok) std::printf("FAILED: %s\n", what), ++failures;
}

static long double alpha_ld(long double fc) {
  const long double w = 2.0L * 3.14159265358979323846264338327950288L * fc;
  return w / (w + 1.0L);
}

// the long-double recursion on one run of 3-vectors x [n][3] -> y [n][3]
static void filter_ld(const std::vector<long double>& x, long n, long double fc, long double beta, long double dc,
                      std::vector<long double>& y) {
  y.assign(3 * n, 0.0L);
  long double xh[3] = {x[0], x[1], x[2]}, dh[3] = {0.0L, 0.0L, 0.0L};
  for (int t = 0; t < 3; ++t) y[t] = xh[t];
  for (long i = 1; i < n; ++i) {
    long double d[3], s = 0.0L;
    for (int t = 0; t < 3; ++t) d[t] = x[3 * i + t] - xh[t], dh[t] = dh[t] + alpha_ld(dc) * (d[t] - dh[t]), s += dh[t] * dh[t];
    const long double a = alpha_ld(fc + beta * sqrtl(s));
    for (int t = 0; t < 3; ++t) xh[t] = xh[t] + a * d[t], y[3 * i + t] = xh[t];
  }
}

// mmego_one_euro's filtered run on the CPU: src [n][lds] -> dst [n][ldd], moved [n]; lane = joint, oe_step per lane and frame
static void run_columns(const float* src, long lds, long n, int J, double fc, double beta, double dc, float* dst, long ldd,
                        float* moved) {
  const double ad = oe_alpha(dc);
  std::vector<double> xhat(3 * J), dhat(3 * J, 0.0);
  for (int c = 0; c < 3 * J; ++c) dst[c] = src[c], xhat[c] = (double)src[c];
  moved[0] = 0.0f;
  for (long i = 1; i < n; ++i) {
    double q = 0.0;
    for (int j = 0; j < J; ++j) {
      const double xi[3] = {(double)src[i * lds + 3 * j], (double)src[i * lds + 3 * j + 1], (double)src[i * lds + 3 * j + 2]};
      oe_step(xi, fc, beta, ad, &xhat[3 * j], &dhat[3 * j]);
      for (int t = 0; t < 3; ++t) {
        dst[i * ldd + 3 * j + t] = (float)xhat[3 * j + t];
        q += (xhat[3 * j + t] - xi[t]) * (xhat[3 * j + t] - xi[t]);
      }
    }
    moved[i] = sm_moved(q, 3 * J);
  }
}

// mmego_one_euro_bones' filtered run on the CPU: bones [NB][2] of (child, parent), parents first
static void run_bones(const float* src, long lds, long n, int J, double fc, double beta, double dc, const int* bones, const float* len,
                      int NB, float* dst, long ldd, int* fallback) {
  const double ad = oe_alpha(dc);
  std::vector<int> mine(J, -1), parent(J, -1);
  for (int b = 0; b < NB; ++b) mine[bones[2 * b]] = b, parent[bones[2 * b]] = bones[2 * b + 1];
  std::vector<double> st(3 * J), dhat(3 * J, 0.0);
  for (int j = 0; j < J; ++j) {
    for (int t = 0; t < 3; ++t) dst[3 * j + t] = src[3 * j + t], st[3 * j + t] = (double)src[3 * j + t];
    if (mine[j] >= 0) oe_bone_vector(src + 3 * j, src + 3 * parent[j], &st[3 * j]);
  }
  fallback[0] = 0;
  for (long i = 1; i < n; ++i) {
    const float* x = src + i * lds;
    std::vector<double> u(3 * J, 0.0), pos(3 * J, 0.0);
    int fell = 0;
    for (int j = 0; j < J; ++j) {
      if (mine[j] >= 0) {
        double v[3];
        oe_bone_vector(x + 3 * j, x + 3 * parent[j], v);
        fell += oe_bone_step(v, fc, beta, ad, (double)len[mine[j]], &st[3 * j], &dhat[3 * j], &u[3 * j]);
      } else {
        const double xi[3] = {(double)x[3 * j], (double)x[3 * j + 1], (double)x[3 * j + 2]};
        oe_step(xi, fc, beta, ad, &st[3 * j], &dhat[3 * j]);
        for (int t = 0; t < 3; ++t) pos[3 * j + t] = st[3 * j + t];
      }
    }
    for (int b = 0; b < NB; ++b) {                          // sw_walk: the child of bone b goes to its parent's pos + L u
      const int c = bones[2 * b], p = bones[2 * b + 1];
      for (int t = 0; t < 3; ++t) pos[3 * c + t] = pos[3 * p + t] + (double)len[b] * u[3 * c + t];
    }
    for (int c = 0; c < 3 * J; ++c) dst[i * ldd + c] = (float)pos[c];
    fallback[i] = fell;
  }
}

static std::vector<long double> column(const std::vector<float>& src, long lds, long n, int j) {
  std::vector<long double> x(3 * n);
  for (long i = 0; i < n; ++i)
    for (int t = 0; t < 3; ++t) x[3 * i + t] = (long double)src[i * lds + 3 * j + t];
  return x;
}

static void check_columns(const char* name, const std::vector<float>& src, long lds, long n, int J, double fc, double beta, double dc,
                          bool exact) {
  const long ldd = 3 * J + 5;
  std::vector<float> dst(n * ldd, -12345.0f), moved(n, -1.0f);
  run_columns(src.data(), lds, n, J, fc, beta, dc, dst.data(), ldd, moved.data());
  std::vector<long double> msum(n, 0.0L);
  for (int j = 0; j < J; ++j) {
    std::vector<long double> y;
    filter_ld(column(src, lds, n, j), n, fc, beta, dc, y);
    for (long i = 0; i < n; ++i)
      for (int t = 0; t < 3; ++t) {
        hold(dst[i * ldd + 3 * j + t], y[3 * i + t]);
        const long double m = y[3 * i + t] - (long double)src[i * lds + 3 * j + t];
        msum[i] += m * m;
        if (exact || i == 0) expect(std::memcmp(&dst[i * ldd + 3 * j + t], &src[i * lds + 3 * j + t], 4) == 0, name);
      }
  }
  for (long i = 0; i < n; ++i) {
    hold(moved[i], sqrtl(msum[i] / J));
    for (long c = 3 * J; c < ldd; ++c) expect(dst[i * ldd + c] == -12345.0f, "padding columns untouched");
    if (exact) expect(moved[i] == 0.0f, "a constant run does not move");
  }
  std::printf("%-28s n %3ld J %2d fc %.3f beta %4.1f: worst error / bound so far %.3f\n", name, n, J, fc, beta, worst);
}

int main() {
  const int JS[2] = {15, 8};
  const double FCS[2] = {0.02, 5.0}, BETAS[2] = {0.0, 40.0};
  for (int J : JS)
    for (double fc : FCS)
      for (double beta : BETAS)
        for (long n : {1L, 2L, 3L, 65L}) {
          const long lds = 3 * J + 3;
          std::vector<float> rnd(n * lds), cst(n * lds), stp(n * lds), rmp(n * lds);
          for (long i = 0; i < n; ++i)
            for (long c = 0; c < lds; ++c) {
              rnd[i * lds + c] = (float)(0.7 * normal());
              cst[i * lds + c] = (float)(0.1 * (double)(c + 1));
              stp[i * lds + c] = i < n / 2 ? 0.25f : 0.25f + 0.01f * (float)(c % 7);
              rmp[i * lds + c] = (float)(0.03 * (double)i * (double)(c % 5) - 0.4);
            }
          check_columns("random", rnd, lds, n, J, fc, beta, 0.1, false);
          check_columns("constant", cst, lds, n, J, fc, beta, 0.1, true);
          check_columns("step", stp, lds, n, J, fc, beta, 0.1, false);
          check_columns("ramp", rmp, lds, n, J, fc, beta, 0.1, false);
        }

  // the bones form: a chain 0 <- 1 <- 2 and a second root 3 with the child 4; slowly turning bones of the right lengths
  const int J = 5, NB = 3, bones[6] = {1, 0, 2, 1, 4, 3};
  const float len[3] = {0.31f, 0.27f, 0.12f};
  const long n = 65, lds = 3 * J;
  for (double fc : FCS)
    for (double beta : BETAS) {
      std::vector<float> src(n * lds);
      for (long i = 0; i < n; ++i) {
        double pos[15];
        for (int t = 0; t < 3; ++t) pos[t] = 0.5 + 0.01 * i + 0.02 * normal(), pos[9 + t] = -0.2 + 0.02 * normal();
        for (int b = 0; b < NB; ++b) {
          double d[3] = {std::cos(0.05 * i + b) + 0.1 * normal(), std::sin(0.05 * i + b) + 0.1 * normal(), 0.3 + 0.1 * normal()};
          const double m = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
          for (int t = 0; t < 3; ++t) pos[3 * bones[2 * b] + t] = pos[3 * bones[2 * b + 1] + t] + (double)len[b] * d[t] / m;
        }
        for (int c = 0; c < 15; ++c) src[i * lds + c] = (float)pos[c];
      }
      std::vector<float> dst(n * lds), col(n * lds), moved(n);
      std::vector<int> fb(n, -1);
      run_bones(src.data(), lds, n, J, fc, beta, 0.1, bones, len, NB, dst.data(), lds, fb.data());
      run_columns(src.data(), lds, n, J, fc, beta, 0.1, col.data(), lds, moved.data());
      for (long i = 0; i < n; ++i) {
        for (int r : {0, 3})
          expect(std::memcmp(&dst[i * lds + 3 * r], &col[i * lds + 3 * r], 12) == 0, "the roots carry the column form's bits");
        expect(fb[i] == 0, "no fallback on slowly turning bones");
        // against the long-double recursion on the bone vectors, laid along the tree
        for (int b = 0; b < NB; ++b) {
          const int c = bones[2 * b], p = bones[2 * b + 1];
          double l2 = 0.0;
          for (int t = 0; t < 3; ++t) l2 += ((double)dst[i * lds + 3 * c + t] - (double)dst[i * lds + 3 * p + t]) *
                                            ((double)dst[i * lds + 3 * c + t] - (double)dst[i * lds + 3 * p + t]);
          const double dev = std::fabs(std::sqrt(l2) - (double)len[b]);
          if (i >= 1 && !(dev <= worst_len)) worst_len = dev;
        }
      }
      std::vector<std::vector<long double>> vh(NB), rt(J);
      for (int b = 0; b < NB; ++b) {
        std::vector<long double> v(3 * n);
        for (long i = 0; i < n; ++i)
          for (int t = 0; t < 3; ++t)
            v[3 * i + t] = (long double)src[i * lds + 3 * bones[2 * b] + t] - (long double)src[i * lds + 3 * bones[2 * b + 1] + t];
        filter_ld(v, n, fc, beta, 0.1, vh[b]);
      }
      for (int r : {0, 3}) filter_ld(column(src, lds, n, r), n, fc, beta, 0.1, rt[r]);
      for (long i = 1; i < n; ++i) {
        long double pos[15];
        for (int r : {0, 3})
          for (int t = 0; t < 3; ++t) pos[3 * r + t] = rt[r][3 * i + t];
        for (int b = 0; b < NB; ++b) {
          const long double* v = &vh[b][3 * i];
          const long double m = sqrtl(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
          for (int t = 0; t < 3; ++t) pos[3 * bones[2 * b] + t] = pos[3 * bones[2 * b + 1] + t] + (long double)len[b] * v[t] / m;
        }
        for (int c = 0; c < 15; ++c) hold(dst[i * lds + c], pos[c]);
      }
      std::printf("bones fc %.3f beta %4.1f: worst error / bound so far %.3f, worst | |bone| - L | %.3e\n", fc, beta, worst, worst_len);
    }

  // a bone that reverses every frame at alpha = 1/2 (fc = 1 / (2 pi), beta = 0): vhat_1 = v + (-2 v) / 2 = 0, the frame keeps its own
  // direction -v and counts one fallback; from then on vhat_i = (vhat_{i-1} + x_i) / 2 = v / 2, -v / 4, 3 v / 8, ... never vanishes
  {
    const int J2 = 2, one[2] = {1, 0};
    const float L[1] = {0.25f};
    const long m = 6;
    std::vector<float> src(m * 6), dst(m * 6);
    std::vector<int> fb(m, -1);
    for (long i = 0; i < m; ++i) {
      const float sign = i % 2 ? -1.0f : 1.0f;
      src[i * 6] = 0.5f, src[i * 6 + 1] = -0.25f, src[i * 6 + 2] = 1.0f;
      src[i * 6 + 3] = 0.5f + sign * 0.25f, src[i * 6 + 4] = -0.25f, src[i * 6 + 5] = 1.0f;
    }
    run_bones(src.data(), 6, m, J2, 1.0 / OE_TWO_PI, 0.0, 0.1, one, L, 1, dst.data(), 6, fb.data());
    long double vh = 0.25L;
    for (long i = 1; i < m; ++i) {
      const long double x = i % 2 ? -0.25L : 0.25L;
      vh = vh + 0.5L * (x - vh);
      const bool fell = fabsl(vh) <= 1e-9L * 0.25L;
      expect(fb[i] == (fell ? 1 : 0) && fell == (i == 1), "the reversing bone falls back in frame 1 and in no other");
      const long double dir = fell ? (x > 0 ? 1.0L : -1.0L) : (vh > 0 ? 1.0L : -1.0L);
      hold(dst[i * 6 + 3], 0.5L + 0.25L * dir);
      expect(dst[i * 6 + 4] == -0.25f && dst[i * 6 + 5] == 1.0f && dst[i * 6] == 0.5f, "the reversing bone stays on its axis");
    }
    std::printf("reversing bone: fallback per frame %d %d %d %d %d %d\n", fb[0], fb[1], fb[2], fb[3], fb[4], fb[5]);
  }
  expect(worst <= 1.0, "every output within 2^-23 |ref| + 1e-7");
  expect(worst_len <= 2e-6, "every filtered bone within 2e-6 of its length");
  std::printf("worst error / bound %.3f, worst bone length deviation %.3e: %s\n", worst, worst_len, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
