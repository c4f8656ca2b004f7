// motion.hip - the empty-frame filter (the reference's src/empty_frame_filter.py) as one fused launch per batch of camera frames.
//
// Per frame: BGR -> gray (OpenCV's 14-bit fixed point), k x k Gaussian blur on OpenCV's bit-exact 8-bit path (ufixedpoint16 taps, exact
// integer row pass, column pass rounded once), |blur - stored| > threshold counted, the stored blurred frame replaced in place.  The
// restatement the results must equal bit for bit is tests/motion_ref.py; it lists the arithmetic.
//
// Work split: a flattened list of 64 x 32 output tiles over all frames of the call (frames may differ in size).  A workgroup loads its
// tile plus a halo of the kernel radius once (reflect-101 at the frame edges) and converts it to gray in LDS, runs the row pass into a
// uint16 LDS tile and the column pass in registers, compares with and overwrites the camera's stored frame at its own output pixels
// only (so the in-place update is race-free), and adds its count to the frame's counter with one global atomic.
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <new>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "gauss8.h"

namespace motion_gate {

using rtd::Error;
namespace bk = rtd::backend;
using bk::align_up;
using bk::guarded;
using gauss8::MAX_R;
using gauss8::Taps;
using gauss8::reflect101;

constexpr int TW = 64, TH = 32;            // output tile
constexpr int THREADS = 256;
constexpr int ROWS_PER_THREAD = TH / (THREADS / TW);   // column pass: 8 output rows per thread

struct FrameDesc {
  const uint8_t* src;     // HWC, C = 1 or 3
  uint8_t* state;         // rows x cols stored blurred frame (read, then overwritten)
  int rows, cols, ch;
  int first;              // 1: no stored frame to compare with - blur and store only
  int tiles_x;
  int tile0;              // first tile of this frame in the flattened list
};

// One instantiation per radius: the tap loops unroll, the taps stay in scalar registers and the LDS tiles are sized to the halo.
template <int R>
__global__ void __launch_bounds__(THREADS) motion_kernel(const FrameDesc* __restrict__ descs, int n_frames, Taps taps, int threshold,
                                                          unsigned int* __restrict__ area) {
  constexpr int k = 2 * R + 1, gw = TW + 2 * R, gh = TH + 2 * R;
  __shared__ uint8_t gray[gh * gw];
  __shared__ uint16_t rowp[gh * TW];
  __shared__ unsigned int block_count;

  // which frame: the last one whose first tile is <= this block (binary search over the descriptors)
  const int tile = blockIdx.x;
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const FrameDesc d = descs[lo];
  const int t = tile - d.tile0;
  const int x0 = (t % d.tiles_x) * TW, y0 = (t / d.tiles_x) * TH;
  const int tid = threadIdx.x;
  uint32_t cs[k];
  gauss8::load_taps<R>(taps, cs);
  if (tid == 0) block_count = 0;

  // 1. tile + halo -> gray (LDS)
  for (int i = tid; i < gh * gw; i += THREADS) {
    const int gy = i / gw, gx = i - gy * gw;
    const int sy = reflect101(y0 - R + gy, d.rows), sx = reflect101(x0 - R + gx, d.cols);
    const uint8_t* p = d.src + ((size_t)sy * d.cols + sx) * d.ch;
    uint32_t y;
    if (d.ch == 3) y = (1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14;
    else y = p[0];
    gray[gy * gw + gx] = (uint8_t)y;
  }
  __syncthreads();

  // 2. row pass: R = sum_j c_j Y[x + j], exact (<= 255 * 256)
  gauss8::row_pass<R, TW, THREADS>(gray, gh, rowp, cs);
  __syncthreads();

  // 3. column pass in registers, compare, store, count
  const int tx = tid % TW, ty0 = (tid / TW) * ROWS_PER_THREAD;
  const int x = x0 + tx;
  unsigned int count = 0;
#pragma unroll
  for (int j = 0; j < ROWS_PER_THREAD; ++j) {
    const int ty = ty0 + j, y = y0 + ty;
    const int v = gauss8::col_pass<R, TW>(rowp + ty * TW + tx, cs);
    bool moved = false;
    if (x < d.cols && y < d.rows) {
      uint8_t* s = d.state + (size_t)y * d.cols + x;
      if (!d.first) moved = abs(v - (int)*s) > threshold;
      *s = (uint8_t)v;
    }
    count += (unsigned int)__popcll(__ballot(moved));   // wave-uniform
  }
  if ((tid & 63) == 0 && count) atomicAdd(&block_count, count);
  __syncthreads();
  if (tid == 0 && block_count) atomicAdd(area + lo, block_count);
}

template <int R>
static void launch_radius(int r, dim3 grid, hipStream_t s, const FrameDesc* descs, int n, const Taps& taps, int threshold, unsigned int* area) {
  if (r == R) {
    rtd::rtd_launch(motion_kernel<R>, grid, dim3(THREADS), 0, s, descs, n, taps, threshold, area);   // the library's one launch path
    return;
  }
  if constexpr (R < MAX_R) launch_radius<R + 1>(r, grid, s, descs, n, taps, threshold, area);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Slot {
  uint8_t* buf = nullptr;
  int rows = 0, cols = 0;
  bool valid = false;       // holds a blurred frame to compare with
};

}  // namespace motion_gate

using namespace motion_gate;

struct rtd_motion : bk::Base {
  Taps taps{};
  bk::OwnStream q;
  std::map<int, Slot> slots;
  // one upload per launch: [descriptors | area counters | host frames]; pinned on the host, mirrored on the device, grown on demand
  bk::PinBuf pin;
  bk::DevBuf dev;
};

namespace motion_gate {

// one launch over frames [b, e) of the call, whose slots are all distinct
static void launch(rtd_motion* m, int b, int e, const uint8_t* const* frames, const int32_t* hwc, int on_device, const int32_t* slots,
                   int threshold, int64_t* area) {
  const int n = e - b;
  const size_t area_off = align_up(sizeof(FrameDesc) * n, 256);
  const size_t frames_off = align_up(area_off + sizeof(unsigned int) * n, 256);
  std::vector<size_t> foff;
  const size_t total = bk::stage_offsets(n, hwc + 3 * b, on_device, frames_off, foff);
  m->pin.reserve(total);
  m->dev.reserve(total);
  hipStream_t st = m->q.stream;
  uint8_t *pin = m->pin.p, *dev = m->dev.p;
  FrameDesc* descs = (FrameDesc*)pin;
  int tiles = 0;
  std::vector<char> first(n);
  for (int i = 0; i < n; ++i) {
    const int32_t* s = hwc + 3 * (b + i);
    Slot& sl = m->slots[slots[b + i]];
    const bool resized = sl.buf && (sl.rows != s[0] || sl.cols != s[1]);
    first[i] = !sl.valid || resized;
    if (resized) {                                       // a new size: a new state buffer (the old one is not read again)
      HIP_CHECK(hipFree(sl.buf));
      sl.buf = nullptr;
      sl.valid = false;
    }
    if (!sl.buf) {
      HIP_CHECK(hipMalloc((void**)&sl.buf, (size_t)s[0] * s[1]));
      sl.rows = s[0];
      sl.cols = s[1];
    }
    FrameDesc& d = descs[i];
    d.src = on_device ? frames[b + i] : dev + foff[i];
    d.state = sl.buf;
    d.rows = s[0];
    d.cols = s[1];
    d.ch = s[2];
    d.first = first[i] ? 1 : 0;
    d.tiles_x = (s[1] + TW - 1) / TW;
    d.tile0 = tiles;
    tiles += d.tiles_x * ((s[0] + TH - 1) / TH);
    if (!on_device) memcpy(pin + foff[i], frames[b + i], (size_t)s[0] * s[1] * s[2]);
  }
  memset(pin + area_off, 0, sizeof(unsigned int) * n);
  HIP_CHECK(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, st));
  launch_radius<0>(m->taps.radius, dim3(tiles), st, (const FrameDesc*)dev, n, m->taps, threshold, (unsigned int*)(dev + area_off));
  HIP_CHECK(hipGetLastError());
  // the counters come back through the start of the pinned buffer (the descriptors there are no longer needed)
  HIP_CHECK(hipMemcpyAsync(pin, dev + area_off, sizeof(unsigned int) * n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const unsigned int* got = (const unsigned int*)pin;
  for (int i = 0; i < n; ++i) {
    area[b + i] = first[i] ? -1 : (int64_t)got[i];
    m->slots[slots[b + i]].valid = true;
  }
}

}  // namespace motion_gate

extern "C" {

int rtd_motion_create(int32_t device, int32_t blur_size, rtd_motion_handle* out) {
  if (out && (blur_size < 1 || blur_size > 2 * MAX_R + 1 || blur_size % 2 == 0)) {   // refused before a handle exists: no HIP call is made
    *out = nullptr;
    bk::create_error<rtd_motion>() = "blur_size must be odd and in 1..63, got " + std::to_string(blur_size);
    return RTD_E_INVALID;
  }
  return bk::create(out, rtd_motion_destroy, [&](rtd_motion* m) {
    bk::use_device(device);
    m->device = device;
    gauss8::make_taps(blur_size, m->taps);
    m->q.open();
  });
}

int rtd_motion_check(rtd_motion_handle m, int32_t n, const uint8_t* const* frames, const int32_t* hwc, int32_t frames_on_device,
                     const int32_t* slots, int32_t threshold, int64_t* area) {
  return guarded(m, [&] {
    RTD_CHECK(n >= 0, RTD_E_INVALID, "n must be >= 0");
    if (n == 0) return;
    RTD_CHECK(frames && hwc && slots && area, RTD_E_INVALID, "null argument");
    for (int i = 0; i < n; ++i) {
      RTD_CHECK(frames[i], RTD_E_INVALID, "frame " + std::to_string(i) + " is null");
      RTD_CHECK(hwc[3 * i] >= 1 && hwc[3 * i + 1] >= 1 && (int64_t)hwc[3 * i] * hwc[3 * i + 1] < (1ll << 31), RTD_E_INVALID,
                "frame " + std::to_string(i) + " has a bad size");
      RTD_CHECK(hwc[3 * i + 2] == 1 || hwc[3 * i + 2] == 3, RTD_E_INVALID, "frames must have 1 or 3 channels");
      RTD_CHECK(slots[i] >= 0, RTD_E_INVALID, "slots must be >= 0");
    }
    HIP_CHECK(hipSetDevice(m->device));
    // a slot seen twice in one call: the later frame goes into the next launch (launches run in order on the handle's stream)
    int b = 0;
    while (b < n) {
      int e = b + 1;
      for (; e < n; ++e) {
        bool dup = false;
        for (int j = b; j < e && !dup; ++j) dup = slots[j] == slots[e];
        if (dup) break;
      }
      try {
        launch(m, b, e, frames, hwc, frames_on_device, slots, threshold, area);
      } catch (...) {
        m->q.drain();                                    // nothing of a failed launch may still read the staging buffers
        throw;
      }
      b = e;
    }
  });
}

int rtd_motion_reset(rtd_motion_handle m, int32_t slot) {
  return guarded(m, [&] {
    RTD_CHECK(slot >= -1, RTD_E_INVALID, "slot must be >= -1");
    for (auto& kv : m->slots)
      if (slot < 0 || kv.first == slot) kv.second.valid = false;
  });
}

int rtd_motion_wait_stream(rtd_motion_handle m, void* producer_stream) {
  return guarded(m, [&] {
    HIP_CHECK(hipSetDevice(m->device));
    m->q.wait_for(producer_stream);
  });
}

const char* rtd_motion_last_error(rtd_motion_handle m) { return bk::last_error(m); }

void rtd_motion_destroy(rtd_motion_handle m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  m->q.drain();
  for (auto& kv : m->slots)
    if (kv.second.buf) (void)hipFree(kv.second.buf);
  m->dev.release();
  m->pin.release();
  m->q.close();
  delete m;
}

int rtd_debug_motion_state(rtd_motion_handle m, int32_t slot, uint8_t* out, size_t nbytes) {
  return guarded(m, [&] {
    auto it = m->slots.find(slot);
    RTD_CHECK(it != m->slots.end(), RTD_E_INVALID, "unknown slot");
    const Slot& s = it->second;
    RTD_CHECK(s.valid, RTD_E_STATE, "the slot holds no frame (reset, or never checked)");
    RTD_CHECK(out && nbytes >= (size_t)s.rows * s.cols, RTD_E_INVALID, "output buffer too small");
    HIP_CHECK(hipSetDevice(m->device));
    HIP_CHECK(hipMemcpyAsync(out, s.buf, (size_t)s.rows * s.cols, hipMemcpyDeviceToHost, m->q.stream));
    HIP_CHECK(hipStreamSynchronize(m->q.stream));
  });
}

}  // extern "C"
