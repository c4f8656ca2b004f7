// ingest.hip - 4:2:0 camera frames (NV12, NV21, I420) to tight HWC BGR device frames: OpenCV's COLOR_YUV2BGR_* fixed-point path, all in
// integers.  The restatement the bytes must equal is tests/yuv_ref.py; the host side (constants, checks, staging layout) is
// ingest_host.h.
//
// One launch covers the whole call.  The host lists the 256 x 16 pixel tiles of every frame; one workgroup per listed tile, and its
// frame's descriptor (planes, pitches, layout, constants) is the same for all its threads.  A thread owns 8 pixels of two rows: four
// 2 x 2 blocks, whose chroma it reads once.  Where every row of the planes and of the output starts on a 4-byte boundary (3 W and the
// pitches multiples of 4) a whole strip moves as dwords: 2 x 8 bytes of luma, 8 of chroma, 2 x 24 of BGR.  Any other frame, and the
// last strip of a row that is not 8 pixels long, moves byte by byte.  Either way a thread stores only the bytes of its own pixels:
// with an odd 3 W a dword of the output belongs to two rows, and nothing here reads the output.
#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "ingest_host.h"

namespace ingest {

using rtd::Error;
namespace bk = rtd::backend;
using bk::guarded;
using namespace ingest_host;

struct Words2 { uint32_t w[2]; };
struct Words6 { uint32_t w[6]; };

// the descriptor's pointers are global memory: said so, the loads and stores are global_* instead of flat_* instructions
#define RTD_GLOBAL __attribute__((address_space(1)))
typedef const RTD_GLOBAL uint8_t* GBytes;
typedef const RTD_GLOBAL uint32_t* GWord;
typedef RTD_GLOBAL uint8_t* GOut;
typedef RTD_GLOBAL uint32_t* GOutWord;

// dword-aligned rows are all a wide frame guarantees: adjacent dword accesses, which the compiler merges into dwordx2 / dwordx4 ones
__device__ inline Words2 load2(GBytes p) {
  const GWord q = (GWord)p;
  return {{q[0], q[1]}};
}
__device__ inline void store6(GOut p, const Words6& v) {
  const GOutWord q = (GOutWord)p;
#pragma unroll
  for (int k = 0; k < 6; ++k) q[k] = v.w[k];
}

// clip8(v >> 20) as a clamp of v itself and a logical shift: the same value for every int v.  Written as shift-then-clamp, hipcc (ROCm 7.2)
// packs two channels with v_ashr_pk_u8_i32 and ORs the others above them as if the upper half of that result were zero; on the
// MI355X the upper halves of the output dwords then came out wrong (the byte path, which the compiler clamps with v_med3_i32, was right).
__device__ inline uint32_t clip8_shr20(int v) { return (uint32_t)min(max(v, 0), (256 << 20) - 1) >> 20; }

// every product is a constant below 2^23 in magnitude (the largest is 2214593) times a value of -128..255: __mul24 is exact for them
// and issues at the full rate, a 32-bit multiply at a quarter of it.
// what the chroma of a 2 x 2 block adds to its four pixels
struct Chroma {
  int r, g, b;
};
__device__ inline Chroma chroma_terms(const FrameDesc& d, uint32_t U, uint32_t V) {
  const int u = (int)U - 128, v = (int)V - 128;
  return {__mul24(d.cvr, v), __mul24(d.cvg, v) + __mul24(d.cug, u), __mul24(d.cub, u)};
}
// one pixel: b | g << 8 | r << 16
__device__ inline uint32_t pixel(const FrameDesc& d, uint32_t Y, const Chroma& c) {
  const int yc = __mul24(max((int)Y - d.ybias, 0), d.cy) + (1 << 19);
  return clip8_shr20(yc + c.b) | clip8_shr20(yc + c.g) << 8 | clip8_shr20(yc + c.r) << 16;
}

__device__ inline uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// a whole strip of a wide frame: x0 is a multiple of 8 and x0 + 8 <= W
__device__ inline void strip_wide(const FrameDesc& d, int x0, int y0) {
  const bool two = y0 + 1 < d.H;
  const GBytes yrow = (GBytes)d.y + (size_t)y0 * d.y_pitch + x0, pu = (GBytes)d.u, pv = (GBytes)d.v;
  const Words2 l0 = load2(yrow);
  Words2 l1 = l0;
  if (two) l1 = load2(yrow + d.y_pitch);
  uint32_t cu[PX / 2], cv[PX / 2];
  const size_t crow = (size_t)(y0 >> 1) * d.c_pitch;
  if (d.flags & F_INTERLEAVED) {
    const Words2 c = load2(pu + crow + x0);
#pragma unroll
    for (int k = 0; k < PX / 2; ++k) {
      const uint32_t a = byte_of(c.w, 2 * k), b = byte_of(c.w, 2 * k + 1);
      cu[k] = (d.flags & F_SWAP) ? b : a;
      cv[k] = (d.flags & F_SWAP) ? a : b;
    }
  } else {
    const uint32_t wu = *(GWord)(pu + crow + (x0 >> 1)), wv = *(GWord)(pv + crow + (x0 >> 1));
#pragma unroll
    for (int k = 0; k < PX / 2; ++k) cu[k] = byte_of(&wu, k), cv[k] = byte_of(&wv, k);
  }
  Words6 o0, o1;
#pragma unroll
  for (int k = 0; k < 6; ++k) o0.w[k] = o1.w[k] = 0u;
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const Chroma c = chroma_terms(d, cu[p >> 1], cv[p >> 1]);
    const uint32_t a = pixel(d, byte_of(l0.w, p), c), b = pixel(d, byte_of(l1.w, p), c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int i = 3 * p + ch;
      o0.w[i >> 2] |= ((a >> (8 * ch)) & 0xffu) << (8 * (i & 3));
      o1.w[i >> 2] |= ((b >> (8 * ch)) & 0xffu) << (8 * (i & 3));
    }
  }
  const GOut orow = (GOut)d.dst + ((size_t)y0 * d.W + x0) * 3;
  store6(orow, o0);
  if (two) store6(orow + (size_t)d.W * 3, o1);
}

// any strip of any frame, byte by byte: the pixels [x0, min(x0 + 8, W)) of the rows y0 and, inside the frame, y0 + 1
__device__ inline void strip_bytes(const FrameDesc& d, int x0, int y0) {
  const GBytes py = (GBytes)d.y, pu = (GBytes)d.u, pv = (GBytes)d.v;
  const int rows = min(2, d.H - y0);
  const size_t crow = (size_t)(y0 >> 1) * d.c_pitch;
  for (int k = 0; k < PX / 2; ++k) {
    const int xb = x0 + 2 * k;
    if (xb >= d.W) break;
    uint32_t U, V;
    if (d.flags & F_INTERLEAVED) {
      const uint32_t a = pu[crow + xb], b = pu[crow + xb + 1];         // (xb is even: the pair of chroma sample xb / 2)
      U = (d.flags & F_SWAP) ? b : a;
      V = (d.flags & F_SWAP) ? a : b;
    } else {
      U = pu[crow + (xb >> 1)];
      V = pv[crow + (xb >> 1)];
    }
    const Chroma c = chroma_terms(d, U, V);
    const int cols = min(2, d.W - xb);
    for (int r = 0; r < rows; ++r)
      for (int j = 0; j < cols; ++j) {
        const uint32_t v = pixel(d, py[(size_t)(y0 + r) * d.y_pitch + xb + j], c);
        const GOut o = (GOut)d.dst + ((size_t)(y0 + r) * d.W + xb + j) * 3;
        o[0] = (uint8_t)v, o[1] = (uint8_t)(v >> 8), o[2] = (uint8_t)(v >> 16);
      }
  }
}

__global__ void __launch_bounds__(THREADS) ingest_kernel(const FrameDesc* __restrict__ descs, const TileRef* __restrict__ tiles) {
  const TileRef t = tiles[blockIdx.x];
  const FrameDesc d = descs[t.frame];
  const int tx = t.tile % d.tiles_x, ty = t.tile / d.tiles_x;
  const int x0 = tx * TILE_W + (int)(threadIdx.x % TX) * PX, y0 = ty * TILE_H + (int)(threadIdx.x / TX) * 2;
  if (x0 >= d.W || y0 >= d.H) return;
  if ((d.flags & F_WIDE) && x0 + PX <= d.W) strip_wide(d, x0, y0);
  else strip_bytes(d, x0, y0);
}

}  // namespace ingest

using namespace ingest;

struct rtd_ingest : bk::Base {
  bk::OwnStream q;
  bk::PinBuf pin;   // pinned: [descriptors | tiles | host frames]
  bk::DevBuf dev;   // its twin on the device
};

namespace ingest {

static void convert(rtd_ingest* g, int n, const rtd_yuv_frame* frames, bool on_device, uint8_t* const* out_dev) {
  hipStream_t s = g->q.stream;
  const Plan p = plan(n, frames, on_device);
  g->pin.reserve(p.total);
  g->dev.reserve(p.total);
  fill_tables(g->pin.p, p, n, frames, on_device, g->dev.p, out_dev);
  if (!on_device)
    for (int i = 0; i < n; ++i) pack_frame(g->pin.p + p.foff[i], frames[i]);
  HIP_CHECK(hipMemcpyAsync(g->dev.p, g->pin.p, p.total, hipMemcpyHostToDevice, s));       // tables and frames: one DMA
  rtd::rtd_launch(ingest_kernel, dim3((unsigned)p.tiles), dim3(THREADS), 0, s, (const FrameDesc*)g->dev.p, (const TileRef*)(g->dev.p + p.tile_off));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace ingest

extern "C" {

int rtd_ingest_create(int32_t device, rtd_ingest_handle* out) {
  return bk::create(out, rtd_ingest_destroy, [&](rtd_ingest* g) {
    bk::use_device(device);
    g->device = device;
    g->q.open();
  });
}

int rtd_ingest_convert(rtd_ingest_handle g, int32_t n, const rtd_yuv_frame* frames, int32_t frames_on_device, uint8_t* const* out_dev) {
  return guarded(g, [&] {
    validate(n, frames, out_dev);
    HIP_CHECK(hipSetDevice(g->device));
    try {
      convert(g, n, frames, frames_on_device != 0, out_dev);
    } catch (...) {
      g->q.drain();                                        // nothing of a failed call may still read the staging buffers
      throw;
    }
  });
}

int rtd_ingest_wait_stream(rtd_ingest_handle g, void* producer_stream) {
  return guarded(g, [&] {
    HIP_CHECK(hipSetDevice(g->device));
    g->q.wait_for(producer_stream);
  });
}

const char* rtd_ingest_last_error(rtd_ingest_handle g) { return bk::last_error(g); }

void rtd_ingest_destroy(rtd_ingest_handle g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  g->q.drain();
  g->dev.release();
  g->pin.release();
  g->q.close();
  delete g;
}

int rtd_debug_ingest_info(int32_t matrix, int32_t full_range, int32_t coeffs_out[5], int32_t* tile_h, int32_t* tile_w, int32_t n,
                          const rtd_yuv_frame* frames, int64_t* tiles) {
  static thread_local std::string err;
  return bk::caught(err, [&] {
    int32_t c[5];
    coeffs(matrix, full_range, c);
    if (coeffs_out) memcpy(coeffs_out, c, sizeof c);
    if (tile_h) *tile_h = TILE_H;
    if (tile_w) *tile_w = TILE_W;
    if (frames && tiles) {
      RTD_CHECK(n >= 0, RTD_E_INVALID, "n must be >= 0");
      *tiles = 0;
      for (int i = 0; i < n; ++i) {
        check_shape(i, frames[i]);
        *tiles += tiles_of(frames[i]);
      }
    }
  });
}

}  // extern "C"
