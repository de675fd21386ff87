// The arithmetic of mmego_imu_jitter (imu_noise.hip), per IMU sample, as host + device functions of the sample's nine white draws z_s and
// its window's nine bias draws z_w: the kernel calls them once per thread, scripts/imu_noise_host_check.hip calls them on the CPU (under
// the host sanitizers) and compares with long-double arithmetic.  Rodrigues and the compose are pose_noise_math.h's; the hashing that
// makes the draws stays device code (noise_draw.h).  The recipe is the comment of the entry point in include/mmego_hip.h.
#pragma once
#include "pose_noise_math.h"

#define IN_CH 15                                 // floats per sample: O [3][3] row-major, accelerometer [3], gyroscope [3]

// E = E_s E_w, row-major in E[9]: E_s = pn_rotation(noise_rad, z_s[0..2]) the sample's white rotation error, E_w = pn_rotation(bias_rad,
// z_w[0..2]) its window's constant one; every entry of the product a three-term double sum in column order.  A factor whose sigma is 0 is
// left out exactly (E is the other factor's bits); both 0 is the caller's case (it copies).
BL_HD void in_rotation(double noise_rad, const float z_s[3], double bias_rad, const float z_w[3], double E[9]) {
  if (bias_rad == 0.0) {
    pn_rotation(noise_rad, z_s[0], z_s[1], z_s[2], E);
    return;
  }
  if (noise_rad == 0.0) {
    pn_rotation(bias_rad, z_w[0], z_w[1], z_w[2], E);
    return;
  }
  double A[9], B[9];
  pn_rotation(noise_rad, z_s[0], z_s[1], z_s[2], A);
  pn_rotation(bias_rad, z_w[0], z_w[1], z_w[2], B);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// a' = (float)(((double)a + bias z_w) + noise z_s): the window's offset first, then the sample's white noise, one float rounding.
BL_HD float in_add(float a, double bias, float z_w, double noise, float z_s) {
  return (float)(((double)a + bias * (double)z_w) + noise * (double)z_s);
}
