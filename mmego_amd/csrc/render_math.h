// The arithmetic of mmego_render_raster and mmego_render_prims (render.hip), per pixel and per primitive, as host + device functions:
// the kernels call them once per thread, tests/render_ref.py restates them in numpy.  The recipe is the comment of the two entry
// points in include/mmego_hip.h.
#pragma once
#include "floor_math.h"

#define RD_REC 12                        // floats of a primitive record: ax, ay, bx, by, r, alpha, cr, cg, cb, 0, 0, 0
#define RD_RING 32                       // segments of the floor ring
#define RD_BONES 20                      // skeleton.BONES_ALL
#define RD_JOINTS 21
#define RD_FIXED (RD_RING + 3 * RD_BONES + 2 * RD_JOINTS)      // 134: the primitives of a frame beside its N cloud returns
#define RD_MAX_P 1024
#define RD_ERR_FULL 0.15                 // metres: the joint error at which the error colour is saturated

// A primitive as the compositor reads it: the segment as (a, b - a, 1 / |b - a|^2 or 0), the radius grown by the half pixel.
struct __attribute__((aligned(16))) RdPrim {
  float ax, ay, dx, dy, inv, R, alpha, cr, cg, cb, pad[2];       // (48 bytes: three 16-byte LDS reads)
};

BL_HD bool rd_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }         // (false for a NaN)

// The record rec[12] as an RdPrim.  -> false where the primitive contributes nothing (the recipe's rule).
BL_HD bool rd_load(const float* __restrict__ rec, RdPrim* q) {
  bool ok = true;
  for (int i = 0; i < 9; ++i) ok = ok && rd_finite(rec[i]);
  q->ax = rec[0], q->ay = rec[1], q->dx = rec[2] - rec[0], q->dy = rec[3] - rec[1];
  const float l2 = q->dx * q->dx + q->dy * q->dy;
  q->inv = l2 > 0.0f ? 1.0f / l2 : 0.0f;
  q->R = rec[4] + 0.5f, q->alpha = rec[5], q->cr = rec[6], q->cg = rec[7], q->cb = rec[8];
  return ok && rd_finite(l2) && rec[5] > 0.0f && rec[4] >= 0.0f;
}

// True where the primitive can reach a pixel centre in [x0, x1] x [y0, y1]: its segment's box grown by R, and by 2^-21 of the
// magnitudes involved on top (b is rebuilt as a + (b - a) here and rd_cover rounds t (b - a): a few ulps of the coordinates), meets
// that box.  Where this is false every centre in the box lies more than R from the segment by more than those roundings, and
// rd_cover is 0 there.
BL_HD bool rd_touches(const RdPrim& q, float x0, float y0, float x1, float y1) {
  const float bx = q.ax + q.dx, by = q.ay + q.dy;
  const float gx = q.R + 4.76837158e-7f * (fabsf(q.ax) + fabsf(bx) + q.R + fabsf(x0) + fabsf(x1));
  const float gy = q.R + 4.76837158e-7f * (fabsf(q.ay) + fabsf(by) + q.R + fabsf(y0) + fabsf(y1));
  return fminf(q.ax, bx) - gx <= x1 && fmaxf(q.ax, bx) + gx >= x0 && fminf(q.ay, by) - gy <= y1 && fmaxf(q.ay, by) + gy >= y0;
}

// c = clamp(r + 0.5 - d, 0, 1) alpha at the pixel centre (px, py).
BL_HD float rd_cover(const RdPrim& q, float px, float py) {
  const float ex = px - q.ax, ey = py - q.ay;
  const float t = fminf(fmaxf((ex * q.dx + ey * q.dy) * q.inv, 0.0f), 1.0f);
  const float fx = ex - t * q.dx, fy = ey - t * q.dy;
  return fminf(fmaxf(q.R - sqrtf(fx * fx + fy * fy), 0.0f), 1.0f) * q.alpha;
}

// One compositing step of a pixel's three channels.
BL_HD void rd_over(const RdPrim& q, float c, float col[3]) {
  col[0] += c * (q.cr - col[0]), col[1] += c * (q.cg - col[1]), col[2] += c * (q.cb - col[2]);
}

// The byte of a channel.
BL_HD unsigned rd_byte(float v) { return (unsigned)(int)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f); }

// ---- the scene ----

BL_HD void rd_project(const float* __restrict__ cam, const double x[3], double* px, double* py) {
  *px = (double)cam[0] * x[0] + (double)cam[1] * x[1] + (double)cam[2] * x[2] + (double)cam[3];
  *py = (double)cam[4] * x[0] + (double)cam[5] * x[1] + (double)cam[6] * x[2] + (double)cam[7];
}

// x dropped onto the plane p: x - h(x) u.
BL_HD void rd_drop(const double p[4], const double x[3], double y[3]) {
  const double h = fl_height(p, x);
  for (int i = 0; i < 3; ++i) y[i] = x[i] - h * p[i];
}

// The ring's in-plane axes of the unit normal u: e1 the coordinate axis with the smallest |u_i| (the first on ties) minus its
// component along u, normalised; e2 = u x e1.
BL_HD void rd_ring_axes(const double u[3], double e1[3], double e2[3]) {
  int ax = 0;
  if (fabs(u[1]) < fabs(u[ax])) ax = 1;
  if (fabs(u[2]) < fabs(u[ax])) ax = 2;
  const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
  double w[3];
  const double wn = fl_reject(e, u, w);
  for (int i = 0; i < 3; ++i) e1[i] = w[i] / wn;
  e2[0] = u[1] * e1[2] - u[2] * e1[1], e2[1] = u[2] * e1[0] - u[0] * e1[2], e2[2] = u[0] * e1[1] - u[1] * e1[0];
}

BL_HD double rd_dist3(const double a[3], const double b[3]) {
  const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  return sqrt(fl_dot(d, d));
}

// The error colour (0,170,0) -> (230,0,0) of a joint e metres from its target.
BL_HD void rd_error_colour(double e, double col[3]) {
  const double s = e / RD_ERR_FULL < 1.0 ? e / RD_ERR_FULL : 1.0;
  col[0] = 230.0 * s, col[1] = 170.0 - 170.0 * s, col[2] = 0.0;
}

BL_HD void rd_store(float* __restrict__ out, double ax, double ay, double bx, double by, double r, double alpha, const double col[3]) {
  out[0] = (float)ax, out[1] = (float)ay, out[2] = (float)bx, out[3] = (float)by, out[4] = (float)r, out[5] = (float)alpha;
  out[6] = (float)col[0], out[7] = (float)col[1], out[8] = (float)col[2];
}

// Primitive k of one frame's 134 + N, into out[12].  pred, tgt: the frame's 63 floats; ground its 4; cloud its [N][6]; cam its 8;
// ring [32][2].
BL_HD void rd_prim(int k, int N, const float* __restrict__ pred, const float* __restrict__ tgt, const float* __restrict__ ground,
                   const float* __restrict__ cloud, int seg, const float* __restrict__ cam, const float* __restrict__ ring, double vmax,
                   float out[RD_REC]) {
  const int bones[RD_BONES][2] = {{20, 3}, {3, 2}, {2, 1}, {2, 4}, {2, 8}, {4, 5}, {5, 6}, {6, 7}, {8, 9}, {9, 10}, {10, 11}, {1, 0},
                                  {0, 12}, {0, 16}, {12, 13}, {13, 14}, {14, 15}, {16, 17}, {17, 18}, {18, 19}};
  for (int i = 0; i < RD_REC; ++i) out[i] = 0.0f;
  double a[3], b[3], ax, ay, bx, by, col[3];
  if (k < RD_RING + RD_BONES) {                                    // the two layers that lie in the plane
    double p[4];
    if (!fl_plane(ground, p)) return;
    if (k < RD_RING) {
      double t0[3], foot[3], e1[3], e2[3];
      fl_load3(tgt, t0);
      rd_drop(p, t0, foot);
      rd_ring_axes(p, e1, e2);
      const int k1 = (k + 1) % RD_RING;
      const double c0 = (double)ring[2 * k], s0 = (double)ring[2 * k + 1], c1 = (double)ring[2 * k1], s1 = (double)ring[2 * k1 + 1];
      for (int i = 0; i < 3; ++i) a[i] = foot[i] + c0 * e1[i] + s0 * e2[i], b[i] = foot[i] + c1 * e1[i] + s1 * e2[i];
      col[0] = col[1] = col[2] = 170.0;
      rd_project(cam, a, &ax, &ay), rd_project(cam, b, &bx, &by);
      rd_store(out, ax, ay, bx, by, 0.5, 1.0, col);
      return;
    }
    if (seg < 0) return;
    const int* bone = bones[k - RD_RING];
    double xa[3], xb[3];
    fl_load3(pred + 3 * bone[0], xa), fl_load3(pred + 3 * bone[1], xb);
    rd_drop(p, xa, a), rd_drop(p, xb, b);
    col[0] = col[1] = col[2] = 60.0;
    rd_project(cam, a, &ax, &ay), rd_project(cam, b, &bx, &by);
    rd_store(out, ax, ay, bx, by, 2.0, 0.35, col);
    return;
  }
  k -= RD_RING + RD_BONES;
  if (k < RD_BONES) {                                              // target bones
    fl_load3(tgt + 3 * bones[k][0], a), fl_load3(tgt + 3 * bones[k][1], b);
    col[0] = col[1] = col[2] = 120.0;
    rd_project(cam, a, &ax, &ay), rd_project(cam, b, &bx, &by);
    rd_store(out, ax, ay, bx, by, 1.5, 1.0, col);
    return;
  }
  k -= RD_BONES;
  if (k < RD_JOINTS) {                                             // target joints
    fl_load3(tgt + 3 * k, a);
    col[0] = col[1] = col[2] = 90.0;
    rd_project(cam, a, &ax, &ay);
    rd_store(out, ax, ay, ax, ay, 2.5, 1.0, col);
    return;
  }
  k -= RD_JOINTS;
  if (k < N) {                                                     // cloud returns
    const float* row = cloud + 6 * k;
    if (row[0] == 0.0f && row[1] == 0.0f && row[2] == 0.0f) return;
    fl_load3(row, a);
    double s = 0.5 + (double)row[4] / (2.0 * vmax);
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);                       // (a NaN velocity stays a NaN: the rasteriser skips the record)
    col[0] = 40.0 + s * 190.0, col[1] = 90.0 - s * 30.0, col[2] = 220.0 - s * 180.0;
    rd_project(cam, a, &ax, &ay);
    rd_store(out, ax, ay, ax, ay, 1.5, 0.8, col);
    return;
  }
  k -= N;
  if (seg < 0) return;
  if (k < RD_BONES) {                                              // predicted bones, coloured by the child's error
    double tc[3];
    fl_load3(pred + 3 * bones[k][0], a), fl_load3(pred + 3 * bones[k][1], b), fl_load3(tgt + 3 * bones[k][1], tc);
    rd_error_colour(rd_dist3(b, tc), col);
    rd_project(cam, a, &ax, &ay), rd_project(cam, b, &bx, &by);
    rd_store(out, ax, ay, bx, by, 2.0, 1.0, col);
    return;
  }
  k -= RD_BONES;                                                   // predicted joints
  double tj[3];
  fl_load3(pred + 3 * k, a), fl_load3(tgt + 3 * k, tj);
  rd_error_colour(rd_dist3(a, tj), col);
  rd_project(cam, a, &ax, &ay);
  rd_store(out, ax, ay, ax, ay, 3.0, 1.0, col);
}
