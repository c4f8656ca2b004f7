// gauss8.h - OpenCV's bit-exact 8-bit GaussianBlur(k x k, sigma 0) with BORDER_REFLECT_101, shared by the empty-frame filter
// (motion.hip) and the motion filter's mask blur (mog2.hip).  The restatement the results must equal is tests/motion_ref.py.
//
// Taps are ufixedpoint16 (units of 1/256, sum 256).  Row pass: R = sum_j c_j Y[x + j], exact (<= 255 * 256, fits uint16).  Column pass:
// out = (sum_i c_i R[y + i] + 32768) >> 16, which is <= 255 (both passes together sum to 65536).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "gauss_taps.h"

namespace gauss8 {

constexpr int MAX_R = 31;                  // k <= 63

struct Taps {
  int radius;
  uint16_t c[2 * MAX_R + 1];
};

// taps of GaussianBlur(k, sigma = 0) on 8-bit input: the rule is gauss_taps.h's (tests/motion_ref.py taps())
static inline void make_taps(int k, Taps& t) {
  t.radius = k / 2;
  tap_rule(k, t.c);
}

// borderInterpolate(p, n, BORDER_REFLECT_101), reflecting repeatedly (a frame shorter than the radius)
__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

// the taps of a radius-R kernel in registers (the tap loops unroll; the values are wave-uniform)
template <int R>
__device__ __forceinline__ void load_taps(const Taps& taps, uint32_t (&cs)[2 * R + 1]) {
#pragma unroll
  for (int j = 0; j < 2 * R + 1; ++j) cs[j] = taps.c[j];
}

// Row pass over an LDS tile of gh rows x (TW + 2R) columns of 8-bit values into an LDS tile of gh rows x TW uint16 sums.  All THREADS
// threads of the workgroup take part; the caller synchronises before and after.
template <int R, int TW, int THREADS>
__device__ __forceinline__ void row_pass(const uint8_t* src, int gh, uint16_t* rowp, const uint32_t (&cs)[2 * R + 1]) {
  constexpr int gw = TW + 2 * R;
  const int tx = threadIdx.x % TW;
  for (int gy = threadIdx.x / TW; gy < gh; gy += THREADS / TW) {
    const uint8_t* g = src + gy * gw + tx;
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < 2 * R + 1; ++j) acc += cs[j] * g[j];
    rowp[gy * TW + tx] = (uint16_t)acc;
  }
}

// Column pass of one output: rp points at the row sum of the output's top halo row (row stride TW).  Returns the blurred 8-bit value.
template <int R, int TW>
__device__ __forceinline__ int col_pass(const uint16_t* rp, const uint32_t (&cs)[2 * R + 1]) {
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 2 * R + 1; ++i) acc += cs[i] * rp[i * TW];
  return (int)((acc + 32768u) >> 16);
}

}  // namespace gauss8
