// The arithmetic of mmego_floor_stats and mmego_floor_clamp (floor.hip), per frame, foot and leg, as host + device functions: the kernels
// call them once per thread, scripts/floor_host_check.hip calls them row by row on the CPU (under the host sanitizers) and compares
// with its own long-double solve.  The recipe is the comment of the two entry points in include/mmego_hip.h.
#pragma once
#include "blend_math.h"

#define FLOOR_W 22                       // columns of a statistics row: 11 per foot
#define FL_COLS 24                       // a lower-joint row: 8 joints, the legs (hip, knee, ankle, foot) = local (0, 1, 2, 3), (4, 5, 6, 7)
#define FL_MIN_NORM 1e-6                 // a plane whose |n| is not above this is no plane
#define FL_TINY 1e-9                     // an ankle target this close to the hip has no direction: the leg stays

// The plane (a, b, c, d) of a frame as p = (n / |n|, d / |n|).  -> 0 where |n| is not > FL_MIN_NORM (a NaN lands there too).
BL_HD int fl_plane(const float* __restrict__ g, double p[4]) {
  const double a = (double)g[0], b = (double)g[1], c = (double)g[2];
  const double n = sqrt(a * a + b * b + c * c);
  p[0] = p[1] = p[2] = p[3] = 0.0;
  if (!(n > FL_MIN_NORM)) return 0;
  p[0] = a / n, p[1] = b / n, p[2] = c / n, p[3] = (double)g[3] / n;
  return 1;
}

// h(x) = n . x + d: the height of a point above the plane.
BL_HD double fl_height(const double p[4], const double x[3]) { return p[0] * x[0] + p[1] * x[1] + p[2] * x[2] + p[3]; }

BL_HD void fl_load3(const float* __restrict__ x, double v[3]) { v[0] = (double)x[0], v[1] = (double)x[1], v[2] = (double)x[2]; }

// One foot's 11 statistics from the predicted height hp, the target's ht and the contact flag c; every comparison strict.
BL_HD void fl_foot_stats(double hp, double ht, double c, double H, float out[11]) {
  const double lowp = hp < H ? 1.0 : 0.0, lowt = ht < H ? 1.0 : 0.0;
  out[0] = (float)fabs(hp - ht);
  out[1] = (float)(hp < 0.0 ? -hp : 0.0);
  out[2] = hp < 0.0 ? 1.0f : 0.0f;
  out[3] = (float)lowp;
  out[4] = (float)(lowp * c);
  out[5] = (float)c;
  out[6] = (float)(c * (hp > 0.0 ? hp : 0.0));
  out[7] = (float)(ht < 0.0 ? -ht : 0.0);
  out[8] = ht < 0.0 ? 1.0f : 0.0f;
  out[9] = (float)lowt;
  out[10] = (float)(lowt * c);
}

BL_HD double fl_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// w = x minus its component along the unit vector u; -> |w|.
BL_HD double fl_reject(const double x[3], const double u[3], double w[3]) {
  const double t = fl_dot(x, u);
  for (int i = 0; i < 3; ++i) w[i] = x[i] - t * u[i];
  return sqrt(fl_dot(w, w));
}

// One leg: in = (hip, knee, ankle, foot) as 12 floats, out the 9 floats of knee, ankle and foot (the hip is the caller's copy).
// *lift: how far the leg was raised along the normal (0 where it stays).  -> 1 where the leg fell back (the target out of reach, so the
// ankle lands at reach along u and the floor is not guaranteed; or no direction / no finite solve, so the leg stays), else 0.
BL_HD int fl_leg(const float* __restrict__ in, const double p[4], double margin, float out[9], double* lift) {
  double Hp[3], K[3], A[3], T[3];
  fl_load3(in, Hp), fl_load3(in + 3, K), fl_load3(in + 6, A), fl_load3(in + 9, T);
  for (int i = 0; i < 9; ++i) out[i] = in[3 + i];
  *lift = 0.0;
  double up = 0.0;
  const double needT = margin - fl_height(p, T), needA = margin - fl_height(p, A);
  if (needT > up) up = needT;
  if (needA > up) up = needA;
  if (!(up > 0.0)) return 0;                                  // (a NaN height raises nothing)
  double kh[3], ak[3], ta[3], v[3], u[3], w[3];
  for (int i = 0; i < 3; ++i) kh[i] = K[i] - Hp[i], ak[i] = A[i] - K[i], ta[i] = T[i] - A[i];
  const double l1 = sqrt(fl_dot(kh, kh)), l2 = sqrt(fl_dot(ak, ak));
  const double near = fabs(l1 - l2) + 1e-6 * (l1 + l2), far = (l1 + l2) * (1.0 - 1e-6);
  float o[9];
  int fell = 0;
  // (a second round only where the stored floats' rounding left ankle or foot under the margin: the lift grows by what is missing and
  // by more than the rounding of a height, 2^-22 of the largest coordinate against sqrt(3) 2^-24, so that the saved feet respect it)
  for (int round = 0; round < 3; ++round) {
    for (int i = 0; i < 3; ++i) v[i] = A[i] + up * p[i] - Hp[i];
    const double D = sqrt(fl_dot(v, v));
    if (!(D > FL_TINY)) return 1;
    for (int i = 0; i < 3; ++i) u[i] = v[i] / D;
    double Dc = D > near ? D : near;
    if (far < Dc) Dc = far;
    fell = Dc != D;
    const double a = (l1 * l1 - l2 * l2 + Dc * Dc) / (2.0 * Dc);
    const double b2 = l1 * l1 - a * a, b = b2 > 0.0 ? sqrt(b2) : 0.0;
    // the side the knee bends to: the knee's own, else the foot bone's, else the coordinate axis u leans on least
    double wn = fl_reject(kh, u, w);
    if (wn < 1e-4 * l1 || wn == 0.0) {
      const double lt = sqrt(fl_dot(ta, ta));
      wn = fl_reject(ta, u, w);
      if (wn < 1e-4 * lt || wn == 0.0) {
        int ax = 0;
        if (fabs(u[1]) < fabs(u[ax])) ax = 1;
        if (fabs(u[2]) < fabs(u[ax])) ax = 2;
        const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
        wn = fl_reject(e, u, w);
      }
    }
    double sum = 0.0, big = 0.0, A2[3], T2[3];
    for (int i = 0; i < 3; ++i) {
      o[i] = (float)(Hp[i] + a * u[i] + b * (w[i] / wn));
      o[3 + i] = (float)(Hp[i] + Dc * u[i]);
      o[6 + i] = (float)((double)o[3 + i] + ta[i]);         // from the ankle as stored: the foot bone keeps its vector to one rounding
      A2[i] = (double)o[3 + i], T2[i] = (double)o[6 + i];
      sum += (double)o[i] + A2[i] + T2[i];
      if (fabs(A2[i]) > big) big = fabs(A2[i]);
      if (fabs(T2[i]) > big) big = fabs(T2[i]);
    }
    if (!(fabs(sum) < 1e30)) return 1;                        // no finite solve (a leg without length): it stays
    const double hA = fl_height(p, A2), hT = fl_height(p, T2), low = hA < hT ? hA : hT;
    if (fell || low >= margin) break;
    up += (margin - low) + 2.384185791015625e-07 * big;       // (2^-22)
  }
  for (int i = 0; i < 9; ++i) out[i] = o[i];
  *lift = up;
  return fell;
}
