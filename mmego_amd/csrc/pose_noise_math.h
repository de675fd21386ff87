// The arithmetic of mmego_pose_jitter (pose_noise.hip), per row, as host + device functions of the row's six unit-variance draws: the
// kernel calls them once per thread, scripts/pose_noise_host_check.hip calls them on the CPU (under the host sanitizers) and compares
// with long-double arithmetic.  The hashing that makes the draws stays device code (noise_draw.h).  The recipe is the comment of the
// entry point in include/mmego_hip.h.
#pragma once
#include "blend_math.h"

#define PN_RAD_PER_DEG 0.017453292519943295      // pi / 180
#define PN_SERIES_BELOW 1e-3                     // theta below this: the series of sin(theta)/theta and (1 - cos(theta))/theta^2

// E = I + a [w]x + b [w]x^2 (Rodrigues) of the rotation vector w = sigma_rad (z0, z1, z2), row-major in E[9]; [w]x^2 = w w^T - theta^2 I.
BL_HD void pn_rotation(double sigma_rad, float z0, float z1, float z2, double E[9]) {
  const double w0 = sigma_rad * (double)z0, w1 = sigma_rad * (double)z1, w2 = sigma_rad * (double)z2;
  const double q = w0 * w0 + w1 * w1 + w2 * w2, th = sqrt(q);
  double a, b;
  if (th < PN_SERIES_BELOW) {
    a = 1.0 - q / 6.0 + q * q / 120.0;
    b = 0.5 - q / 24.0 + q * q / 720.0;
  } else {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / q;
  }
  const double c = 1.0 - b * q;
  E[0] = c + b * w0 * w0, E[1] = b * w0 * w1 - a * w2, E[2] = b * w0 * w2 + a * w1;
  E[3] = b * w1 * w0 + a * w2, E[4] = c + b * w1 * w1, E[5] = b * w1 * w2 - a * w0;
  E[6] = b * w2 * w0 - a * w1, E[7] = b * w2 * w1 + a * w0, E[8] = c + b * w2 * w2;
}

// out = (float)(E R): R [3][3] row-major floats, every entry a three-term double sum in column order, one float rounding.
BL_HD void pn_compose(const double E[9], const float R[9], float out[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      out[3 * i + j] = (float)(E[3 * i] * (double)R[j] + E[3 * i + 1] * (double)R[3 + j] + E[3 * i + 2] * (double)R[6 + j]);
}

// t' = (float)((double)t + sigma_t z)
BL_HD float pn_shift(float t, double sigma_t, float z) { return (float)((double)t + sigma_t * (double)z); }
