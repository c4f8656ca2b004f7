// enhance_tables.h - the host-built tables of the crop enhancement (csrc/enhance.hip): every transcendental function of the colour
// conversions and of the bilateral weights is evaluated here, once per handle, in double precision.  Plain C++ (no HIP): the formulas
// are the ones in the docstring of tests/enhance_ref.py, which the device path must match bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace enhance {

constexpr int LAB_SHIFT = 12, LAB_SHIFT2 = 15;
constexpr int INV_Q = 12, INV_S = 255 * 64;
constexpr int COLOR_W = 769;        // |db| + |dg| + |dr| <= 765

struct Tables {
  std::vector<uint16_t> gtab, ctab;          // 256, 3072
  int32_t C[9], Ci[9];                       // forward / inverse matrices, white point folded in, 12 fractional bits
  std::vector<int32_t> t_l, t_a, t_b, finv;  // 256 each; finv over [fmin, fmax]
  int32_t fmin = 0;
  std::vector<uint8_t> gi;                   // INV_S + 1
  int radius = 0;
  std::vector<float> space_w;                // (2 radius + 1)^2, row-major over (i, j); 0 outside the disc
  std::vector<float> color_w;                // COLOR_W
};

inline double sat(double v, double lo, double hi) { return std::min(std::max(v, lo), hi); }

inline int bilateral_radius(int d, double sigma_space) {
  const double ss = sigma_space > 0 ? sigma_space : 1.0;
  return std::max(d > 0 ? d / 2 : (int)rint(ss * 1.5), 1);
}

inline Tables make_tables(int d, double sigma_color, double sigma_space) {
  static const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
  static const double W[3] = {0.950456, 1.0, 1.088754};
  Tables t;
  t.gtab.resize(256);
  for (int i = 0; i < 256; ++i) {
    const double x = i / 255.0;
    const double g = x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
    t.gtab[i] = (uint16_t)sat(rint(255.0 * 8 * g), 0, 65535);
  }
  t.ctab.resize(3072);
  for (int i = 0; i < 3072; ++i) {
    const double x = i / (double)(255 * 8);
    t.ctab[i] = (uint16_t)sat(rint((double)(1 << LAB_SHIFT2) * (x < 0.008856 ? x * 7.787 + 0.13793103448275862 : cbrt(x))), 0, 65535);
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) t.C[3 * r + c] = (int32_t)rint((double)(1 << LAB_SHIFT) * M[r][c] / W[r]);
  // inverse of M by cofactors
  const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                     M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  double Mi[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;      // cofactor of M[c][r]
      Mi[r][c] = (M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]) / det;
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) t.Ci[3 * r + c] = (int32_t)rint((double)(1 << INV_Q) * Mi[r][c] * W[c]);
  t.t_l.resize(256), t.t_a.resize(256), t.t_b.resize(256);
  for (int i = 0; i < 256; ++i) {
    t.t_l[i] = (int32_t)rint((double)(1 << INV_Q) * (((double)(i * 100) / 255.0 + 16) / 116));
    t.t_a[i] = (int32_t)rint((double)((1 << INV_Q) * (i - 128)) / 500.0);
    t.t_b[i] = (int32_t)rint((double)((1 << INV_Q) * (i - 128)) / 200.0);
  }
  const int32_t lmin = t.t_l[0], lmax = t.t_l[255];
  t.fmin = std::min(lmin + t.t_a[0], lmin - t.t_b[255]);
  const int32_t fmax = std::max(lmax + t.t_a[255], lmax - t.t_b[0]);
  t.finv.resize(fmax - t.fmin + 1);
  for (int32_t k = t.fmin; k <= fmax; ++k) {
    const double x = k / (double)(1 << INV_Q);
    t.finv[k - t.fmin] = (int32_t)rint(INV_S * (x > 6.0 / 29 ? x * x * x : (x - 16.0 / 116) / 7.787));
  }
  t.gi.resize(INV_S + 1);
  for (int v = 0; v <= INV_S; ++v) {
    const double x = v / (double)INV_S;
    t.gi[v] = (uint8_t)sat(rint(255 * (x <= 0.0031308 ? x * 12.92 : 1.055 * pow(x, 1 / 2.4) - 0.055)), 0, 255);
  }
  const double sc = sigma_color > 0 ? sigma_color : 1.0, ss = sigma_space > 0 ? sigma_space : 1.0;
  const double gc = -0.5 / (sc * sc), gs = -0.5 / (ss * ss);
  t.radius = bilateral_radius(d, sigma_space);
  const int R = t.radius, D = 2 * R + 1;
  t.space_w.assign((size_t)D * D, 0.f);
  for (int i = -R; i <= R; ++i)
    for (int j = -R; j <= R; ++j)
      if (i * i + j * j <= R * R) t.space_w[(size_t)(i + R) * D + (j + R)] = (float)exp((i * i + j * j) * gs);
  t.color_w.resize(COLOR_W);
  for (int k = 0; k < COLOR_W; ++k) t.color_w[k] = (float)exp(k * k * gc);
  return t;
}

}  // namespace enhance
