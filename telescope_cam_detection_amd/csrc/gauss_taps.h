// gauss_taps.h - THE tap rule of OpenCV's bit-exact 8-bit GaussianBlur(k x k, sigma 0): getGaussianKernelBitExact in units of 1/256.
// No HIP here: gauss8.h (motion.hip, mog2.hip: k <= 63, taps in registers) and facemask_host.h (k <= 99, a per-face table) share it, and
// tools/facemask_host_check.cpp runs it on a CPU.  The restatements are tests/motion_ref.py taps() and tests/face_ref.py taps().
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace gauss8 {

// c[0..k) for an odd k >= 1: fixed tables up to k = 7, error-diffused rounding above (the taps are symmetric, >= 0 and sum to 256)
static inline void tap_rule(int k, uint16_t* c) {
  static const uint16_t fixed[4][7] = {{256}, {64, 128, 64}, {16, 64, 96, 64, 16}, {8, 28, 56, 72, 56, 28, 8}};
  if (k <= 7) {
    for (int i = 0; i < k; ++i) c[i] = fixed[k / 2][i];
    return;
  }
  const double sigma = 0.15 * k + 0.35;
  std::vector<double> g(k);
  double sum = 0;
  for (int i = 0; i < k; ++i) {
    const double xx = i - (k - 1) / 2.0;
    g[i] = std::exp(-(xx * xx) / (2.0 * sigma * sigma));
    sum += g[i];
  }
  double e = 0;
  int off = 0;
  for (int i = 0; i < k / 2; ++i) {
    const double adj = 256.0 * (g[i] / sum) + e;
    const int v = (int)std::nearbyint(adj);         // round half to even (the default rounding mode), like cvRound
    e = adj - v;
    c[i] = c[k - 1 - i] = (uint16_t)v;
    off += v;
  }
  c[k / 2] = (uint16_t)(256 - 2 * off);
}

}  // namespace gauss8
