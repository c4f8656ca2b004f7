// backend.h - the host-side scaffold of all twelve handles (twelve handles, one scaffold): the detector engine (engine_internal.h) and the
// stand-alone back ends (motion, mog2, jpeg, overlay, enhance, esrgan, ingest, facemask, eva, yolox_post, yolox_net).  What a handle holds, how a C entry point turns exceptions into a
// return code and a message, how a handle is created, the buffers it grows on demand, and the scratch of one call (OpScratch).
// A back end writes its kernels, its argument checks and its extern "C" functions; nothing here generates an entry point.  Host only.
// The three that run a whole network on launch_conv (esrgan, eva, yolox_net) share more: net_plan.h, on top of this header.
#pragma once
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "call_parts.h"
#include "common.h"

namespace rtd {
namespace backend {

// (align_up, TileRef and sides_ok are call_parts.h's: the HIP-free headers share them)

// runs f; an exception becomes its return code, its message goes into `err`
template <typename F>
int caught(std::string& err, F&& f) {
  try {
    f();
    return RTD_OK;
  } catch (const Error& er) {
    err = er.what();
    return er.code;
  } catch (const std::bad_alloc&) {
    err = "host allocation failed";
    return RTD_E_OOM;
  } catch (const std::exception& ex) {
    err = ex.what();
    return RTD_E_HIP;
  }
}

// every handle derives from this
struct Base {
  int device = 0;
  std::mutex mu;
  std::string err;   // the last failed call's message (rtd_X_last_error(handle))
};

// a call on a handle: one at a time, the message kept on the handle
template <typename H, typename F>
int guarded(H* h, F&& f) {
  if (!h) return RTD_E_INVALID;
  std::lock_guard<std::mutex> lk(h->mu);
  return caught(h->err, f);
}

// what rtd_X_last_error(NULL) reports: the calling thread's last refused create of THIS back end
template <typename H>
std::string& create_error() {
  static thread_local std::string s;
  return s;
}

template <typename H>
const char* last_error(H* h) { return h ? h->err.c_str() : create_error<H>().c_str(); }

// init(h) fills the fresh handle and may throw; a handle that was not completed is destroyed and *out stays null
template <typename H, typename D, typename F>
int create(H** out, D destroy, F&& init) {
  if (!out) return RTD_E_INVALID;
  *out = nullptr;
  H* h = new (std::nothrow) H();
  if (!h) return RTD_E_OOM;
  const int rc = caught(create_error<H>(), [&] { init(h); });
  if (rc != RTD_OK) {
    destroy(h);
    return rc;
  }
  *out = h;
  return RTD_OK;
}

inline void use_device(int device) {
  int count = 0;
  HIP_CHECK(hipGetDeviceCount(&count));
  RTD_CHECK(device >= 0 && device < count, RTD_E_INVALID, "no such device");
  HIP_CHECK(hipSetDevice(device));
}

// a handle's own non-blocking stream, and the event through which it waits for a producer's stream
struct OwnStream {
  hipStream_t stream = nullptr;
  hipEvent_t ev_xs = nullptr;
  void open() {
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&ev_xs, hipEventDisableTiming));
  }
  void wait_for(void* producer) {
    HIP_CHECK(hipEventRecord(ev_xs, (hipStream_t)producer));
    HIP_CHECK(hipStreamWaitEvent(stream, ev_xs, 0));
  }
  void drain() {   // after a failed call (nothing of it may still read the staging buffers), and before the buffers are freed
    if (stream) (void)hipStreamSynchronize(stream);
  }
  void close() {
    if (ev_xs) (void)hipEventDestroy(ev_xs);
    if (stream) (void)hipStreamDestroy(stream);
    ev_xs = nullptr;
    stream = nullptr;
  }
};

// a device (or pinned host) buffer that grows on demand and is never shrunk.  hipFree waits for the device, so nothing enqueued earlier
// still uses a buffer that is replaced; the capacity at least doubles, so in the steady state nothing is allocated.
template <bool PINNED>
struct GrowBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  void reserve(size_t bytes) {
    if (bytes <= cap) return;
    const size_t want = std::max(bytes, cap * 2);
    release();
    void* q = nullptr;
    if (PINNED) HIP_CHECK(hipHostMalloc(&q, want, hipHostMallocDefault));
    else HIP_CHECK(hipMalloc(&q, want));
    p = (uint8_t*)q;
    cap = want;
  }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
};
using DevBuf = GrowBuf<false>;
using PinBuf = GrowBuf<true>;

// device buffers, events and streams of ONE call (the kernel-level test / bench / debug entry points, the staging of a filter upload):
// released when the call ends, on every path - a throwing RTD_CHECK / HIP_CHECK included.  The buffers go first: hipFree waits for the
// device, so nothing enqueued still uses what is released.
struct OpScratch {
  std::vector<void*> bufs;
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> streams;
  OpScratch() = default;
  OpScratch(const OpScratch&) = delete;
  OpScratch& operator=(const OpScratch&) = delete;
  template <typename T> T* get(size_t count) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, count ? count * sizeof(T) : 16));
    bufs.push_back(p);
    return (T*)p;
  }
  template <typename T> T* zeros(size_t count) {
    T* d = get<T>(count);
    HIP_CHECK(hipMemset(d, 0, count * sizeof(T)));
    return d;
  }
  template <typename T> T* upload(const T* host, size_t count) {
    T* d = get<T>(count);
    HIP_CHECK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  hipEvent_t event() {
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreate(&e));
    events.push_back(e);
    return e;
  }
  hipStream_t stream() {   // non-blocking
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    streams.push_back(s);
    return s;
  }
  void release() {
    for (void* p : bufs) (void)hipFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    bufs.clear(); events.clear(); streams.clear();
  }
  ~OpScratch() { release(); }
};

// frames that arrive from the host are staged one after the other from `at`, each on a 256-byte boundary: foff[i] is frame i's offset,
// the return value the end of the last one.  hwc = [n][3] rows, cols, channels.  Device-resident frames take no room.
inline size_t stage_offsets(int n, const int32_t* hwc, bool on_device, size_t at, std::vector<size_t>& foff) {
  foff.resize(n);
  for (int i = 0; i < n; ++i) {
    foff[i] = at;
    if (!on_device) at = align_up(at + (size_t)hwc[3 * i] * hwc[3 * i + 1] * hwc[3 * i + 2], 256);
  }
  return at;
}

// ---- the argument checks shared by the crop calls (enhance, esrgan): n crops cut from device-resident frames, frame_hw = [n][2],
// rects = [n][4] x1, y1, x2, y2.  The back end's own layout (its size limits) runs between the two.
constexpr int MAX_CROPS = 64;
inline void check_crop_call(int n, const uint8_t* const* frames, const int32_t* frame_hw, const int32_t* rects, const uint8_t* out) {
  RTD_CHECK(n >= 1 && n <= MAX_CROPS, RTD_E_INVALID, "1..64 crops per call");
  RTD_CHECK(frames && frame_hw && rects && out, RTD_E_INVALID, "null argument");
}
inline void check_crop_frame(int i, const uint8_t* const* frames, const int32_t* frame_hw, const int32_t* rects) {
  const std::string ci = "crop " + std::to_string(i);
  const int64_t fh = frame_hw[2 * i], fw = frame_hw[2 * i + 1];
  RTD_CHECK(frames[i], RTD_E_INVALID, ci + " has a null frame");
  RTD_CHECK(sides_ok(fh, fw), RTD_E_INVALID, ci + ": bad frame size (1..65535 per side)");
  RTD_CHECK(rects[4 * i + 2] <= fw && rects[4 * i + 3] <= fh, RTD_E_INVALID, ci + " leaves its frame");
}

}  // namespace backend
}  // namespace rtd
