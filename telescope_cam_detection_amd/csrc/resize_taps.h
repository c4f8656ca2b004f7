// resize_taps.h - OpenCV's resize for 8-bit INTER_LINEAR (imgproc/src/resize.cpp): the tables, made in its own double / float
// arithmetic, and the integer rule that turns four taps into one output value.  THE rule of the pixelate face mask (facemask_host.h,
// facemask.hip) and of the frame ingest's resize stage (ingest_host.h, ingest.hip), as gauss_taps.h is the blur's.  The restatement both
// must equal is tests/face_ref.py (linear_table, is_area2, resize_linear).  The tables are host code; the pixel rule (linear8, area8)
// compiles for the device too, and as plain C++ where there is no HIP (tools/ingest_host_check.cpp holds it to hand-worked values).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

namespace resize_taps {

struct LinEntry {            // one column (or row) of the INTER_LINEAR pass: S[i0] * w0 + S[i1] * w1.  12 bytes; the indices are int32, so a
  int32_t i0, i1;            // source extent of 65535 (the limit of every caller) fits, and the weights are 0 .. 2048
  int16_t w0, w1;
};

inline int cv_round(double v) { return (int)nearbyint(v); }     // cvRound: half to even (the default rounding mode)

// cv::resize: inv_scale = (double)dsize / ssize; hal::resize: scale = 1. / inv_scale
inline double resize_scale(int ssize, int dsize) {
  const double inv_scale = (double)dsize / ssize;
  return 1. / inv_scale;
}

// hal::resize: INTER_LINEAR becomes the 2 x 2 INTER_AREA mean when both scale factors are exactly 2 (is_area_fast && iscale == 2)
inline bool area2(int rw, int rh, int sw, int sh) {
  const double scale_x = resize_scale(rw, sw), scale_y = resize_scale(rh, sh);
  const int iscale_x = cv_round(scale_x), iscale_y = cv_round(scale_y);      // saturate_cast<int>(double)
  const bool is_area_fast = fabs(scale_x - iscale_x) < DBL_EPSILON && fabs(scale_y - iscale_y) < DBL_EPSILON;
  return is_area_fast && iscale_x == 2 && iscale_y == 2;
}

// resizeGeneric_'s table loops for INTER_LINEAR on 8-bit input: entry d of a pass from ssize to dsize samples.
// Columns: the fraction becomes 0 where the left sample is the first or the last column (so HResizeLinear's S[sx] * ONE beyond xmax
// is S[i0] * 2048 + S[i1] * 0 here).  Rows: the table keeps the fraction and resizeGeneric_Invoker clips the two row indices (an up-scale's
// first and last rows then blend a row with itself, each term rounded on its own, as cv2 does).
inline void linear_table(int ssize, int dsize, bool columns, LinEntry* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double scale = resize_scale(ssize, dsize);
  for (int d = 0; d < dsize; ++d) {
    double pos = (d + 0.5) * scale;                 // fx = (float)((dx + 0.5) * scale_x - 0.5), the product and the difference rounded
    pos -= 0.5;                                     // one after the other (two statements: never a fused multiply-add)
    float f = (float)pos;
    int s = (int)floorf(f);                         // cvFloor
    f -= (float)s;
    int s1;
    if (columns) {
      if (s < 0) f = 0, s = 0;
      if (s >= ssize - 1) f = 0, s = ssize - 1;
      s1 = std::min(s + 1, ssize - 1);
    } else {
      s1 = std::min(std::max(s + 1, 0), ssize - 1);                          // clip(sy0 + k, 0, ssize.height)
      s = std::min(std::max(s, 0), ssize - 1);
    }
    const float c0 = 1.f - f, c1 = f;
    out[d].i0 = s, out[d].i1 = s1;
    out[d].w0 = (int16_t)lrintf(c0 * 2048), out[d].w1 = (int16_t)lrintf(c1 * 2048);   // saturate_cast<short>(cbuf[k] * INTER_RESIZE_COEF_SCALE)
  }
}

// ---- the pixel rule: one channel of one output pixel from its four source values (0..255) ----------------------------------------------
#if defined(__HIPCC__)
#define RTD_TAPS_FN __host__ __device__ inline
#else
#define RTD_TAPS_FN inline
#endif

// a product of two values that fit 24 bits: on the device the full-rate multiply (a 32-bit one issues at a quarter of that rate)
RTD_TAPS_FN int mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(a, b);
#else
  return a * b;
#endif
}

// HResizeLinear<uchar, int, short, 2048> on the rows of p00 p01 and of p10 p11 with the column weights w0, w1, then
// VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>> with the row weights b0, b1.  Every value is non-negative, every
// product below 2^27 and the result at most 255: w0 + w1 and b0 + b1 are at most 2049 (linear_table)
RTD_TAPS_FN int linear8(int p00, int p01, int p10, int p11, int w0, int w1, int b0, int b1) {
  const int h0 = mul24(p00, w0) + mul24(p01, w1), h1 = mul24(p10, w0) + mul24(p11, w1);
  return ((mul24(b0, h0 >> 4) >> 16) + (mul24(b1, h1 >> 4) >> 16) + 2) >> 2;
}

// ResizeAreaFastVec / ResizeAreaFast_Invoker at scale 2: the rounded mean of a 2 x 2 block
RTD_TAPS_FN int area8(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

}  // namespace resize_taps
