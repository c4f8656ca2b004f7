// mog2.hip - the motion filter (the reference's src/motion_filter.py MotionFilter): OpenCV's MOG2 background model and the per-box
// motion count of its foreground mask, on the device.
//
// State pass: one fused launch per chunk of up to 32 model updates of the same frame (MotionFilter applies the frame once per detection).
// A thread owns one pixel: it reads the pixel's model (5 modes of weight, variance and C means, plus the modes-used count) once into
// registers, runs the chunk's updates with each update's alphaT / prune, writes the model back once, and writes one uint32 whose bit i
// says "update i of the chunk marked the pixel foreground (mask 255)".  The arithmetic is float32 in the operator order of the restatement
// (tests/mog2_ref.py), with contraction off; modes are kept in registers and every mode index is a compile-time constant, so the swaps
// of the sorting steps are register selects.
//
// ROI pass: one launch over a flattened list of 64 x 32 output tiles of every update's box.  A workgroup loads its tile plus a halo of the
// blur radius from the update's bit plane (reflect-101 at the FRAME edges) as 0 / 255 bytes, runs the shared 8-bit Gaussian blur
// (gauss8.h), counts outputs > 25 inside the box with ballot / popcount and adds its count with one global atomic.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "gauss8.h"

#pragma clang fp contract(off)

namespace mog2 {

using rtd::Error;
namespace bk = rtd::backend;
using bk::align_up;
using bk::guarded;
using gauss8::MAX_R;
using gauss8::Taps;
using gauss8::reflect101;

constexpr int NM = 5;                       // mixtures
constexpr int CHUNK = 32;                   // updates per state pass: the bits of one word
constexpr int STATE_THREADS = 256;
constexpr int TW = 64, TH = 32;             // ROI pass output tile
constexpr int ROI_THREADS = 256;
constexpr int ROWS_PER_THREAD = TH / (ROI_THREADS / TW);
constexpr int MASK_THRESHOLD = 25;          // threshold(blurred mask, 25): strict

// createBackgroundSubtractorMOG2 defaults
constexpr float TB = 0.9f, TG = 9.0f, VAR_INIT = 15.0f, VAR_MIN = 4.0f, VAR_MAX = 75.0f, TAU = 0.5f, FCT = 0.05f;

struct Chunk {
  float alpha_t[CHUNK];
  float prune[CHUNK];
  int n;                                    // updates in this chunk, 1..32
};

struct StateArgs {
  float* planes;                            // [NM][2 + C][npix]: weight, variance, mean_0 .. mean_{C-1}
  uint8_t* modes;                           // [npix] modes used
  const uint8_t* frame;                     // [npix][C]
  uint32_t* bits;                           // [npix] this chunk's foreground words
  int npix;
  float tb;                                 // (float) var_threshold
  int shadows;
};

template <int C>
__device__ __forceinline__ void swap_modes(float (&w)[NM], float (&v)[NM], float (&mu)[NM][C], int i, int j) {
  float t = w[i]; w[i] = w[j]; w[j] = t;
  t = v[i]; v[i] = v[j]; v[j] = t;
#pragma unroll
  for (int c = 0; c < C; ++c) { t = mu[i][c]; mu[i][c] = mu[j][c]; mu[j][c] = t; }
}

// detectShadowGMM on the updated model
template <int C>
__device__ __forceinline__ bool shadow(const float (&x)[C], int n, const float (&w)[NM], const float (&v)[NM], const float (&mu)[NM][C],
                                       float tb) {
  float tw = 0.f;
  bool done = false, sh = false;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    if (done || m >= n) continue;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      num = num + x[c] * mu[m][c];
      den = den + mu[m][c] * mu[m][c];
    }
    if (den == 0.f) { done = true; continue; }
    if (num <= den && num >= TAU * den) {
      const float a = num / den;
      float d2 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float dd = a * mu[m][c] - x[c];
        d2 = d2 + dd * dd;
      }
      if (d2 < tb * v[m] * a * a) { sh = true; done = true; continue; }
    }
    tw = tw + w[m];
    if (tw > TB) done = true;
  }
  return sh;
}

template <int C>
__global__ void __launch_bounds__(STATE_THREADS) mog2_state_kernel(StateArgs a, Chunk ch) {
  const int p = blockIdx.x * STATE_THREADS + threadIdx.x;
  if (p >= a.npix) return;
  constexpr int F = 2 + C;
  const size_t P = (size_t)a.npix;
  float x[C], w[NM], v[NM], mu[NM][C];
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] = (float)a.frame[(size_t)p * C + c];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    w[m] = a.planes[(m * F + 0) * P + p];
    v[m] = a.planes[(m * F + 1) * P + p];
#pragma unroll
    for (int c = 0; c < C; ++c) mu[m][c] = a.planes[(m * F + 2 + c) * P + p];
  }
  int n = a.modes[p];
  const float tb = a.tb;
  uint32_t word = 0;

  for (int u = 0; u < ch.n; ++u) {
    const float alpha_t = ch.alpha_t[u], prune = ch.prune[u];
    const float alpha1 = 1.f - alpha_t;
    bool background = false, fits = false;
    float total = 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      if (m >= n) continue;                 // n shrinks inside the loop when a mode is pruned
      float wm = alpha1 * w[m] + prune;
      bool fit_here = false;
      if (!fits) {
        float d[C];
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = mu[m][c] - x[c];
        float dist2 = d[0] * d[0];
        if (C == 1) dist2 = 0.f + dist2;
#pragma unroll
        for (int c = 1; c < C; ++c) dist2 = dist2 + d[c] * d[c];
        const float var = v[m];
        if (total < TB && dist2 < tb * var) background = true;
        if (dist2 < TG * var) {
          fits = fit_here = true;
          wm = wm + alpha_t;
          const float k = alpha_t / wm;
#pragma unroll
          for (int c = 0; c < C; ++c) mu[m][c] = mu[m][c] - k * d[c];
          float vn = var + k * (dist2 - var);
          vn = vn < VAR_MIN ? VAR_MIN : vn;
          vn = vn > VAR_MAX ? VAR_MAX : vn;
          v[m] = vn;
        }
      }
      const float wsort = wm;               // the sorting step compares the weight before the prune test
      if (wm < -prune) { wm = 0.f; --n; }
      w[m] = wm;                            // the matched mode carries its weight up with it
      bool go = fit_here;
#pragma unroll
      for (int i = m; i > 0; --i) {
        go = go && !(wsort < w[i - 1]);
        if (go) swap_modes<C>(w, v, mu, i, i - 1);
      }
      total = total + wm;
    }
    const float inv = fabsf(total) > FLT_EPSILON ? 1.f / total : 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m)
      if (m < n) w[m] = w[m] * inv;
    if (!fits && alpha_t > 0.f) {           // a new mode: replace the weakest or add one
      const int mn = n == NM ? NM - 1 : n++;
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        if (m == mn) {
          w[m] = n == 1 ? 1.f : alpha_t;
          v[m] = VAR_INIT;
#pragma unroll
          for (int c = 0; c < C; ++c) mu[m][c] = x[c];
        } else if (n != 1 && m < n - 1) {
          w[m] = w[m] * alpha1;
        }
      }
      bool go = true;
#pragma unroll
      for (int i = NM - 1; i > 0; --i) {
        if (i > n - 1) continue;
        go = go && !(alpha_t < w[i - 1]);
        if (go) swap_modes<C>(w, v, mu, i, i - 1);
      }
    }
    const bool fg = !background && !(a.shadows && shadow<C>(x, n, w, v, mu, tb));
    word |= (uint32_t)fg << u;
  }

#pragma unroll
  for (int m = 0; m < NM; ++m) {
    a.planes[(m * F + 0) * P + p] = w[m];
    a.planes[(m * F + 1) * P + p] = v[m];
#pragma unroll
    for (int c = 0; c < C; ++c) a.planes[(m * F + 2 + c) * P + p] = mu[m][c];
  }
  a.modes[p] = (uint8_t)n;
  a.bits[p] = word;
}

struct RoiDesc {
  int x1, y1, x2, y2;                       // clamped, non-empty
  int tiles_x;
  int tile0;                                // first tile of this box in the flattened list
  int plane;                                // the update's word plane (update / 32) and bit (update % 32)
  int bit;
  int out;                                  // index of the box's counter
};

// One instantiation per radius: the tap loops unroll and the LDS tiles are sized to the halo.
template <int R>
__global__ void __launch_bounds__(ROI_THREADS) mog2_roi_kernel(const RoiDesc* __restrict__ descs, int n_desc, const uint32_t* __restrict__ bits,
                                                               int rows, int cols, Taps taps, unsigned int* __restrict__ counts) {
  constexpr int k = 2 * R + 1, gw = TW + 2 * R, gh = TH + 2 * R;
  __shared__ uint8_t mask[gh * gw];
  __shared__ uint16_t rowp[gh * TW];
  __shared__ unsigned int block_count;

  const int tile = blockIdx.x;
  int lo = 0, hi = n_desc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const RoiDesc d = descs[lo];
  const int t = tile - d.tile0;
  const int x0 = d.x1 + (t % d.tiles_x) * TW, y0 = d.y1 + (t / d.tiles_x) * TH;
  const int tid = threadIdx.x;
  const uint32_t* plane = bits + (size_t)d.plane * rows * cols;
  uint32_t cs[k];
  gauss8::load_taps<R>(taps, cs);
  if (tid == 0) block_count = 0;

  // 1. tile + halo of the update's mask (threshold(mask, 200) leaves 0 / 255) -> LDS
  for (int i = tid; i < gh * gw; i += ROI_THREADS) {
    const int gy = i / gw, gx = i - gy * gw;
    const int sy = reflect101(y0 - R + gy, rows), sx = reflect101(x0 - R + gx, cols);
    mask[gy * gw + gx] = ((plane[(size_t)sy * cols + sx] >> d.bit) & 1u) ? 255 : 0;
  }
  __syncthreads();

  // 2. row pass
  gauss8::row_pass<R, TW, ROI_THREADS>(mask, gh, rowp, cs);
  __syncthreads();

  // 3. column pass in registers, threshold, count inside the box
  const int tx = tid % TW, ty0 = (tid / TW) * ROWS_PER_THREAD;
  const int x = x0 + tx;
  unsigned int count = 0;
#pragma unroll
  for (int j = 0; j < ROWS_PER_THREAD; ++j) {
    const int ty = ty0 + j, y = y0 + ty;
    const int val = gauss8::col_pass<R, TW>(rowp + ty * TW + tx, cs);
    const bool moving = x < d.x2 && y < d.y2 && val > MASK_THRESHOLD;
    count += (unsigned int)__popcll(__ballot(moving));   // wave-uniform
  }
  if ((tid & 63) == 0 && count) atomicAdd(&block_count, count);
  __syncthreads();
  if (tid == 0 && block_count) atomicAdd(counts + d.out, block_count);
}

template <int R>
static void launch_roi(int r, dim3 grid, hipStream_t s, const RoiDesc* descs, int n, const uint32_t* bits, int rows, int cols,
                       const Taps& taps, unsigned int* counts) {
  if (r == R) {
    rtd::rtd_launch(mog2_roi_kernel<R>, grid, dim3(ROI_THREADS), 0, s, descs, n, bits, rows, cols, taps, counts);
    return;
  }
  if constexpr (R < MAX_R) launch_roi<R + 1>(r, grid, s, descs, n, bits, rows, cols, taps, counts);
}

}  // namespace mog2

using namespace mog2;

struct rtd_mog2 : bk::Base {
  int history = 500;
  float tb = 16.f;
  int shadows = 1;
  bk::OwnStream q;
  // the model: [NM][2 + C][rows * cols] float planes, then rows * cols modes-used bytes (allocated on the first frame, reallocated on a
  // size or channel change)
  uint8_t* state = nullptr;
  int rows = 0, cols = 0, ch = 0;
  bool fresh = true;                         // the next update initialises the model (a new subtractor, or a new frame geometry)
  int64_t nframes = 0;
  // foreground words of the last call, [chunks][rows * cols]; grown on demand
  bk::DevBuf bits;
  int last_chunks = 0;
  // one upload per call: [box descriptors | counters | host frame]; pinned on the host, mirrored on the device, grown on demand
  bk::PinBuf pin;
  bk::DevBuf dev;
  int taps_k = 0;
  Taps taps{};
};

namespace mog2 {

static size_t npix(const rtd_mog2* g) { return (size_t)g->rows * g->cols; }
static size_t plane_bytes(const rtd_mog2* g) { return (size_t)NM * (2 + g->ch) * npix(g) * sizeof(float); }

static void check_params(int32_t history, double var_threshold) {
  RTD_CHECK(history >= 1, RTD_E_INVALID, "history must be >= 1, got " + std::to_string(history));
  RTD_CHECK(std::isfinite(var_threshold), RTD_E_INVALID, "var_threshold must be finite");
}

// the model for a rows x cols x ch frame: a new geometry frees the old buffer and allocates a new one (OpenCV re-initialises on it too)
static void ensure_model(rtd_mog2* g, int rows, int cols, int ch) {
  if (g->state && g->rows == rows && g->cols == cols && g->ch == ch) return;
  if (g->state) (void)hipFree(g->state);
  g->state = nullptr;
  g->rows = g->cols = g->ch = 0;
  const size_t p = (size_t)rows * cols;
  HIP_CHECK(hipMalloc((void**)&g->state, (size_t)NM * (2 + ch) * p * sizeof(float) + p));
  g->rows = rows;
  g->cols = cols;
  g->ch = ch;
  g->fresh = true;
}

static void apply(rtd_mog2* g, const uint8_t* frame, int on_device, int n, const int32_t* rects, int blur_size, int64_t* counts) {
  const size_t P = npix(g);
  const int chunks = (n + CHUNK - 1) / CHUNK;
  g->bits.reserve((size_t)chunks * P * sizeof(uint32_t));
  if (g->taps_k != blur_size) {
    gauss8::make_taps(blur_size, g->taps);
    g->taps_k = blur_size;
  }
  const size_t cnt_off = align_up(sizeof(RoiDesc) * n, 256);
  const size_t frame_off = align_up(cnt_off + sizeof(unsigned int) * n, 256);
  const size_t total = on_device ? frame_off : frame_off + P * g->ch;
  g->pin.reserve(total);
  g->dev.reserve(total);
  hipStream_t st = g->q.stream;
  uint8_t *pin = g->pin.p, *dev = g->dev.p;
  uint32_t* bits = (uint32_t*)g->bits.p;
  RoiDesc* descs = (RoiDesc*)pin;
  int nd = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* r = rects + 4 * i;
    if (r[2] <= r[0] || r[3] <= r[1]) continue;   // an empty box: count 0, but its update still happens
    RoiDesc& d = descs[nd++];
    d.x1 = r[0]; d.y1 = r[1]; d.x2 = r[2]; d.y2 = r[3];
    d.tiles_x = (r[2] - r[0] + TW - 1) / TW;
    d.tile0 = tiles;
    d.plane = i / CHUNK;
    d.bit = i % CHUNK;
    d.out = i;
    tiles += d.tiles_x * ((r[3] - r[1] + TH - 1) / TH);
  }
  memset(pin + cnt_off, 0, sizeof(unsigned int) * n);
  if (!on_device) memcpy(pin + frame_off, frame, P * g->ch);
  HIP_CHECK(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, st));
  if (g->fresh) {                                 // a new model: all zeros, nframes = 0
    HIP_CHECK(hipMemsetAsync(g->state, 0, plane_bytes(g) + P, st));
    g->nframes = 0;
    g->fresh = false;
  }
  StateArgs a;
  a.planes = (float*)g->state;
  a.modes = g->state + plane_bytes(g);
  a.frame = on_device ? frame : dev + frame_off;
  a.npix = (int)P;
  a.tb = g->tb;
  a.shadows = g->shadows;
  const dim3 grid((unsigned)((P + STATE_THREADS - 1) / STATE_THREADS));
  for (int c = 0; c < chunks; ++c) {
    Chunk chunk{};
    chunk.n = std::min(CHUNK, n - c * CHUNK);
    for (int j = 0; j < chunk.n; ++j) {
      ++g->nframes;
      const double lr = 1.0 / (double)std::min<int64_t>(2 * g->nframes, g->history);
      chunk.alpha_t[j] = (float)lr;
      chunk.prune[j] = (float)(-lr * FCT);
    }
    a.bits = bits + (size_t)c * P;
    if (g->ch == 3) rtd::rtd_launch(mog2_state_kernel<3>, grid, dim3(STATE_THREADS), 0, st, a, chunk);
    else rtd::rtd_launch(mog2_state_kernel<1>, grid, dim3(STATE_THREADS), 0, st, a, chunk);
    HIP_CHECK(hipGetLastError());
  }
  g->last_chunks = chunks;
  unsigned int* dcounts = (unsigned int*)(dev + cnt_off);
  if (tiles) {
    launch_roi<0>(g->taps.radius, dim3(tiles), st, (const RoiDesc*)dev, nd, bits, g->rows, g->cols, g->taps, dcounts);
    HIP_CHECK(hipGetLastError());
  }
  // the counters come back through the start of the pinned buffer (the descriptors there are no longer needed)
  HIP_CHECK(hipMemcpyAsync(pin, dcounts, sizeof(unsigned int) * n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const unsigned int* got = (const unsigned int*)pin;
  for (int i = 0; i < n; ++i) counts[i] = (int64_t)got[i];
}

}  // namespace mog2

extern "C" {

int rtd_mog2_create(int32_t device, int32_t history, double var_threshold, int32_t detect_shadows, rtd_mog2_handle* out) {
  return bk::create(out, rtd_mog2_destroy, [&](rtd_mog2* g) {
    check_params(history, var_threshold);
    bk::use_device(device);
    g->device = device;
    g->history = history;
    g->tb = (float)var_threshold;
    g->shadows = detect_shadows ? 1 : 0;
    g->q.open();
  });
}

int rtd_mog2_configure(rtd_mog2_handle g, int32_t history, double var_threshold, int32_t detect_shadows) {
  return guarded(g, [&] {
    check_params(history, var_threshold);
    g->history = history;
    g->tb = (float)var_threshold;
    g->shadows = detect_shadows ? 1 : 0;
    g->fresh = true;
    g->nframes = 0;
  });
}

int rtd_mog2_apply(rtd_mog2_handle g, const uint8_t* frame, const int32_t* hwc, int32_t frame_on_device, int32_t n, const int32_t* rects,
                   int32_t blur_size, int64_t* counts) {
  return guarded(g, [&] {
    RTD_CHECK(n >= 0, RTD_E_INVALID, "n must be >= 0");
    if (n == 0) return;
    RTD_CHECK(frame && hwc && rects && counts, RTD_E_INVALID, "null argument");
    const int rows = hwc[0], cols = hwc[1], ch = hwc[2];
    RTD_CHECK(rows >= 1 && cols >= 1 && (int64_t)rows * cols < (1ll << 31), RTD_E_INVALID, "the frame has a bad size");
    RTD_CHECK(ch == 1 || ch == 3, RTD_E_INVALID, "frames must have 1 or 3 channels");
    RTD_CHECK(blur_size >= 1 && blur_size <= 2 * MAX_R + 1 && blur_size % 2 == 1, RTD_E_INVALID,
              "blur_size must be odd and in 1..63, got " + std::to_string(blur_size));
    for (int i = 0; i < n; ++i) {
      const int32_t* r = rects + 4 * i;
      RTD_CHECK(r[0] >= 0 && r[1] >= 0 && r[2] <= cols && r[3] <= rows, RTD_E_INVALID,
                "box " + std::to_string(i) + " is not clamped to the frame");
    }
    HIP_CHECK(hipSetDevice(g->device));
    ensure_model(g, rows, cols, ch);
    try {
      mog2::apply(g, frame, frame_on_device, n, rects, blur_size, counts);
    } catch (...) {
      g->q.drain();                            // nothing of a failed launch may still read the staging buffers
      throw;
    }
  });
}

int rtd_mog2_wait_stream(rtd_mog2_handle g, void* producer_stream) {
  return guarded(g, [&] {
    HIP_CHECK(hipSetDevice(g->device));
    g->q.wait_for(producer_stream);
  });
}

const char* rtd_mog2_last_error(rtd_mog2_handle g) { return bk::last_error(g); }

void rtd_mog2_destroy(rtd_mog2_handle g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  g->q.drain();
  if (g->state) (void)hipFree(g->state);
  g->bits.release();
  g->dev.release();
  g->pin.release();
  g->q.close();
  delete g;
}

int rtd_debug_mog2_model(rtd_mog2_handle g, int32_t* hwc, int64_t* nframes, float* weight, float* variance, float* mean,
                         uint8_t* modes_used, size_t npix_out) {
  return guarded(g, [&] {
    RTD_CHECK(hwc && nframes, RTD_E_INVALID, "null argument");
    const bool live = g->state && !g->fresh;
    hwc[0] = live ? g->rows : 0;
    hwc[1] = live ? g->cols : 0;
    hwc[2] = live ? g->ch : 0;
    *nframes = live ? g->nframes : 0;
    if (!weight && !variance && !mean && !modes_used) return;
    RTD_CHECK(live, RTD_E_STATE, "the filter holds no model (new, reconfigured, or never applied)");
    RTD_CHECK(weight && variance && mean && modes_used && npix_out == npix(g), RTD_E_INVALID, "output buffers do not match the model");
    const size_t P = npix(g);
    const int C = g->ch, F = 2 + C;
    std::vector<float> planes(plane_bytes(g) / sizeof(float));
    HIP_CHECK(hipSetDevice(g->device));
    HIP_CHECK(hipMemcpyAsync(planes.data(), g->state, plane_bytes(g), hipMemcpyDeviceToHost, g->q.stream));
    HIP_CHECK(hipMemcpyAsync(modes_used, g->state + plane_bytes(g), P, hipMemcpyDeviceToHost, g->q.stream));
    HIP_CHECK(hipStreamSynchronize(g->q.stream));
    for (size_t p = 0; p < P; ++p)
      for (int m = 0; m < NM; ++m) {
        weight[p * NM + m] = planes[(m * F + 0) * P + p];
        variance[p * NM + m] = planes[(m * F + 1) * P + p];
        for (int c = 0; c < C; ++c) mean[(p * NM + m) * C + c] = planes[(m * F + 2 + c) * P + p];
      }
  });
}

int rtd_debug_mog2_fg_bits(rtd_mog2_handle g, uint32_t* out, size_t nwords) {
  return guarded(g, [&] {
    RTD_CHECK(g->last_chunks > 0 && g->state, RTD_E_STATE, "no call has updated the model yet");
    const size_t words = (size_t)g->last_chunks * npix(g);
    RTD_CHECK(out && nwords >= words, RTD_E_INVALID, "output buffer too small");
    HIP_CHECK(hipSetDevice(g->device));
    HIP_CHECK(hipMemcpyAsync(out, g->bits.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, g->q.stream));
    HIP_CHECK(hipStreamSynchronize(g->q.stream));
  });
}

}  // extern "C"
