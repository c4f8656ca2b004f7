// ingest.hip - 4:2:0 camera frames (NV12, NV21, I420) to tight HWC BGR device frames: OpenCV's COLOR_YUV2BGR_* fixed-point path, all in
// integers.  The restatement the bytes must equal is tests/yuv_ref.py; the host side (constants, checks, staging layout) is
// ingest_host.h, and all three calls go through one path on it (run() below): a convert call is a resize call without resized outputs.
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
#include "global_bytes.h"
#include "ingest_host.h"

namespace ingest {

using rtd::Error;
namespace bk = rtd::backend;
using bk::guarded;
using namespace ingest_host;

struct Words2 { uint32_t w[2]; };
struct Words6 { uint32_t w[6]; };

// (the descriptors' pointers are read through global_bytes.h's address_space(1) types: global_* instead of flat_* instructions)
// dword-aligned rows are all a wide frame guarantees: adjacent dword accesses, which the compiler merges into dwordx2 / dwordx4 ones
__device__ inline Words2 load2(GBytes p) {
  const GWord q = (GWord)p;
  return {{q[0], q[1]}};
}
// four pixels (b | g << 8 | r << 16 each) as the three dwords of their 12 bytes
__device__ inline void pack4(const uint32_t px[4], uint32_t w[3]) {
  w[0] = px[0] | px[1] << 24;
  w[1] = px[1] >> 8 | px[2] << 16;
  w[2] = px[2] >> 16 | px[3] << 8;
}
__device__ inline void store3(GOut p, const uint32_t w[3]) {
  const GOutWord q = (GOutWord)p;
  q[0] = w[0], q[1] = w[1], q[2] = w[2];
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

// the chroma sample (cx, cy), byte by byte, as what it adds to its pixels
__device__ inline Chroma chroma_at(const FrameDesc& d, int cx, int cy) {
  const GBytes pu = (GBytes)d.u, pv = (GBytes)d.v;
  const size_t crow = (size_t)cy * d.c_pitch;
  uint32_t U, V;
  if (d.flags & F_INTERLEAVED) {
    const uint32_t a = pu[crow + 2 * cx], b = pu[crow + 2 * cx + 1];
    U = (d.flags & F_SWAP) ? b : a;
    V = (d.flags & F_SWAP) ? a : b;
  } else {
    U = pu[crow + cx];
    V = pv[crow + cx];
  }
  return chroma_terms(d, U, V);
}

// THE strip of a wide frame, as dwords: the 8 source pixels from x0 (a multiple of 8, x0 + 8 <= W) of the rows y0 (even) and y0 + 1, and
// their four chroma samples.  two: the row y0 + 1 exists (it is not loaded otherwise, and l1 is l0)
struct Strip {
  Words2 l0, l1;
  uint32_t cu[PX / 2], cv[PX / 2];
};
__device__ inline Strip load_strip(const FrameDesc& d, int x0, int y0, bool two) {
  Strip s;
  const GBytes yrow = (GBytes)d.y + (size_t)y0 * d.y_pitch + x0, pu = (GBytes)d.u, pv = (GBytes)d.v;
  s.l0 = load2(yrow);
  s.l1 = s.l0;
  if (two) s.l1 = load2(yrow + d.y_pitch);
  const size_t crow = (size_t)(y0 >> 1) * d.c_pitch;
  if (d.flags & F_INTERLEAVED) {
    const Words2 c = load2(pu + crow + x0);
#pragma unroll
    for (int k = 0; k < PX / 2; ++k) {
      const uint32_t a = byte_of(c.w, 2 * k), b = byte_of(c.w, 2 * k + 1);
      s.cu[k] = (d.flags & F_SWAP) ? b : a;
      s.cv[k] = (d.flags & F_SWAP) ? a : b;
    }
  } else {
    const uint32_t wu = *(GWord)(pu + crow + (x0 >> 1)), wv = *(GWord)(pv + crow + (x0 >> 1));
#pragma unroll
    for (int k = 0; k < PX / 2; ++k) s.cu[k] = byte_of(&wu, k), s.cv[k] = byte_of(&wv, k);
  }
  return s;
}

// a whole strip of a wide frame: x0 is a multiple of 8 and x0 + 8 <= W
__device__ inline void strip_wide(const FrameDesc& d, int x0, int y0) {
  const bool two = y0 + 1 < d.H;
  const Strip s = load_strip(d, x0, y0, two);
  Words6 o0, o1;
#pragma unroll
  for (int h = 0; h < PX / 4; ++h) {                              // four pixels of each row are three dwords
    uint32_t a[4], b[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const Chroma c = chroma_terms(d, s.cu[(4 * h + p) >> 1], s.cv[(4 * h + p) >> 1]);
      a[p] = pixel(d, byte_of(s.l0.w, 4 * h + p), c), b[p] = pixel(d, byte_of(s.l1.w, 4 * h + p), c);
    }
    pack4(a, o0.w + 3 * h), pack4(b, o1.w + 3 * h);
  }
  const GOut orow = (GOut)d.dst + ((size_t)y0 * d.W + x0) * 3;
  store6(orow, o0);
  if (two) store6(orow + (size_t)d.W * 3, o1);
}

// any strip of any frame, byte by byte: the pixels [x0, min(x0 + 8, W)) of the rows y0 and, inside the frame, y0 + 1
__device__ inline void strip_bytes(const FrameDesc& d, int x0, int y0) {
  const GBytes py = (GBytes)d.y;
  const int rows = min(2, d.H - y0);
  for (int k = 0; k < PX / 2; ++k) {
    const int xb = x0 + 2 * k;
    if (xb >= d.W) break;
    const Chroma c = chroma_at(d, xb >> 1, y0 >> 1);                  // (xb and y0 are even)
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
  const FrameDesc d = descs[t.owner];
  const int tx = t.tile % d.tiles_x, ty = t.tile / d.tiles_x;
  const int x0 = tx * TILE_W + (int)(threadIdx.x % TX) * PX, y0 = ty * TILE_H + (int)(threadIdx.x / TX) * 2;
  if (x0 >= d.W || y0 >= d.H) return;
  if ((d.flags & F_WIDE) && x0 + PX <= d.W) strip_wide(d, x0, y0);
  else strip_bytes(d, x0, y0);
}

// ---- the resize stage: OpenCV's resize(frame, (w, h)) with INTER_LINEAR on the converted (or BGR) frame, tests/resize_ref.py -----------
// One workgroup per listed 128 x 8 tile of OUTPUT pixels; a thread makes four output pixels of one row (12 bytes: three dwords where
// the output rows start on a dword, bytes otherwise and for a row's short tail; only ever its own bytes).  Two paths, chosen per frame
// on the host (resize_taps.h area2): the 2 x 2 mean, whose four output pixels are the convert kernel's strip of 8 source pixels in two
// rows, loaded the same way (dwords where the source rows allow it) with one chroma sample per block; and the linear path, which reads
// its four taps per output pixel from the per-frame column and row tables and converts every tap in registers (no LDS: the taps of a
// tile span a source region whose size depends on the scale, from a fraction of a pixel to 65535, and one code path serves them all).

enum { SRC_YUV = 0, SRC_BGR = 1 };

__device__ inline uint32_t luma_at(const FrameDesc& d, int x, int y) { return ((GBytes)d.y)[(size_t)y * d.y_pitch + x]; }
__device__ inline uint32_t bgr_at(const FrameDesc& d, int x, int y) {
  const GBytes p = (GBytes)d.y + (size_t)y * d.y_pitch + (size_t)x * 3;
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}

// the source pixels (x0, y0), (x1, y0), (x0, y1), (x1, y1) as b | g << 8 | r << 16; a chroma sample two taps share is read once
template <int SRC>
__device__ inline void taps4(const FrameDesc& s, int x0, int x1, int y0, int y1, uint32_t p[4]) {
  if (SRC == SRC_BGR) {
    p[0] = bgr_at(s, x0, y0), p[1] = bgr_at(s, x1, y0), p[2] = bgr_at(s, x0, y1), p[3] = bgr_at(s, x1, y1);
  } else {
    const int cx0 = x0 >> 1, cx1 = x1 >> 1, cy0 = y0 >> 1, cy1 = y1 >> 1;
    const Chroma c00 = chroma_at(s, cx0, cy0);
    Chroma c01 = c00, c10 = c00;
    if (cx1 != cx0) c01 = chroma_at(s, cx1, cy0);
    if (cy1 != cy0) c10 = chroma_at(s, cx0, cy1);
    Chroma c11 = cy1 == cy0 ? c01 : c10;
    if (cy1 != cy0 && cx1 != cx0) c11 = chroma_at(s, cx1, cy1);
    p[0] = pixel(s, luma_at(s, x0, y0), c00), p[1] = pixel(s, luma_at(s, x1, y0), c01);
    p[2] = pixel(s, luma_at(s, x0, y1), c10), p[3] = pixel(s, luma_at(s, x1, y1), c11);
  }
}

// one output pixel of the linear path from its four taps: resize_taps.h's linear8 on each channel
__device__ inline uint32_t blend(const uint32_t p[4], int w0, int w1, int b0, int b1) {
  uint32_t o = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    o |= (uint32_t)resize_taps::linear8(byte_of(&p[0], ch), byte_of(&p[1], ch), byte_of(&p[2], ch), byte_of(&p[3], ch), w0, w1, b0, b1) << (8 * ch);
  return o;
}

// resize_taps.h's area8 on each channel of four packed pixels, two channels at a time: blue and red in one sum (16 bits apart, and a
// sum of four bytes and 2 stays below 2^16), green in another.  An optimisation of area8 for packed pixels, not a second definition
__device__ inline uint32_t mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t m = 0x00ff00ffu;
  const uint32_t br = (((a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u) >> 2) & m;
  const uint32_t g = (((a >> 8) & 0xffu) + ((b >> 8) & 0xffu) + ((c >> 8) & 0xffu) + ((d >> 8) & 0xffu) + 2u) >> 2;
  return br | g << 8;
}

// the area path where the source rows start on dwords: the output pixels ox .. ox + 3 (ox a multiple of 4, all inside the row) of row oy
template <int SRC>
__device__ inline void area_wide(const FrameDesc& s, int ox, int oy, uint32_t px[RPX]) {
  const int x0 = 2 * ox, y0 = 2 * oy;
  if (SRC == SRC_BGR) {
    const GWord r0 = (GWord)((GBytes)s.y + (size_t)y0 * s.y_pitch + (size_t)x0 * 3), r1 = (GWord)((GBytes)r0 + s.y_pitch);
    uint32_t a[6], b[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = r0[k], b[k] = r1[k];
#pragma unroll
    for (int k = 0; k < RPX; ++k) {
      uint32_t q[4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int at = 3 * (2 * k + j);
        q[j] = byte_of(a, at) | byte_of(a, at + 1) << 8 | byte_of(a, at + 2) << 16;
        q[2 + j] = byte_of(b, at) | byte_of(b, at + 1) << 8 | byte_of(b, at + 2) << 16;
      }
      px[k] = mean4(q[0], q[1], q[2], q[3]);
    }
  } else {
    const Strip t = load_strip(s, x0, y0, true);                   // (both rows exist: 2 OH == H; RPX output pixels are PX source pixels)
#pragma unroll
    for (int k = 0; k < RPX; ++k) {
      const Chroma c = chroma_terms(s, t.cu[k], t.cv[k]);
      px[k] = mean4(pixel(s, byte_of(t.l0.w, 2 * k), c), pixel(s, byte_of(t.l0.w, 2 * k + 1), c), pixel(s, byte_of(t.l1.w, 2 * k), c),
                    pixel(s, byte_of(t.l1.w, 2 * k + 1), c));
    }
  }
}

// the area path of any frame, byte by byte: the first cnt of the four output pixels
template <int SRC>
__device__ inline void area_bytes(const FrameDesc& s, int ox, int oy, int cnt, uint32_t px[RPX]) {
#pragma unroll
  for (int k = 0; k < RPX; ++k) {
    if (k >= cnt) break;
    const int x = 2 * (ox + k), y = 2 * oy;
    if (SRC == SRC_BGR) {
      px[k] = mean4(bgr_at(s, x, y), bgr_at(s, x + 1, y), bgr_at(s, x, y + 1), bgr_at(s, x + 1, y + 1));
    } else {
      const Chroma c = chroma_at(s, ox + k, oy);
      px[k] = mean4(pixel(s, luma_at(s, x, y), c), pixel(s, luma_at(s, x + 1, y), c), pixel(s, luma_at(s, x, y + 1), c),
                    pixel(s, luma_at(s, x + 1, y + 1), c));
    }
  }
}

template <int SRC>
__global__ void __launch_bounds__(THREADS) resize_kernel(const ResizeDesc* __restrict__ descs, const TileRef* __restrict__ tiles) {
  const TileRef t = tiles[blockIdx.x];
  const ResizeDesc d = descs[t.owner];
  const int tx = t.tile % d.tiles_x, ty = t.tile / d.tiles_x;
  const int ox = tx * RTILE_W + (int)(threadIdx.x % TX) * RPX, oy = ty * RTILE_H + (int)(threadIdx.x / TX);
  if (ox >= d.OW || oy >= d.OH) return;
  const int cnt = min(RPX, d.OW - ox);
  uint32_t px[RPX] = {0u, 0u, 0u, 0u};
  if (d.rflags & R_AREA) {
    if ((d.rflags & R_SRC_WIDE) && cnt == RPX) area_wide<SRC>(d.src, ox, oy, px);
    else area_bytes<SRC>(d.src, ox, oy, cnt, px);
  } else {
    const GLin tab = (GLin)d.tab;
    const GLin r = tab + d.OW + oy;                        // (members one by one: a struct in the global address space is not copyable)
    const int j0 = r->i0, j1 = r->i1, b0 = r->w0, b1 = r->w1;
#pragma unroll
    for (int k = 0; k < RPX; ++k) {
      if (k >= cnt) break;
      const GLin e = tab + ox + k;
      uint32_t p[4];
      taps4<SRC>(d.src, e->i0, e->i1, j0, j1, p);
      px[k] = blend(p, e->w0, e->w1, b0, b1);
    }
  }
  const GOut o = (GOut)d.out + ((size_t)oy * d.OW + ox) * 3;
  if ((d.rflags & R_DST_WIDE) && cnt == RPX) {
    uint32_t w[3];
    pack4(px, w);
    store3(o, w);
  } else {
#pragma unroll
    for (int k = 0; k < RPX; ++k) {
      if (k >= cnt) break;
      o[3 * k] = (uint8_t)px[k], o[3 * k + 1] = (uint8_t)(px[k] >> 8), o[3 * k + 2] = (uint8_t)(px[k] >> 16);
    }
  }
}

}  // namespace ingest

using namespace ingest;

struct rtd_ingest : bk::Base {
  bk::OwnStream q;
  bk::PinBuf pin;   // pinned: [descriptors | tiles | host frames]
  bk::DevBuf dev;   // its twin on the device
};

namespace ingest {

// any of the three calls: up to three launches on the handle's stream after the one staging copy - the convert kernel for the frames
// whose native BGR frame is wanted (all frames of rtd_ingest_convert), the fused kernel for the other 4:2:0 frames, the BGR kernel for
// BGR sources and for the native frames the convert kernel has just written
static void run(rtd_ingest* g, const ResizeCall& c) {
  hipStream_t s = g->q.stream;
  const ResizePlan p = plan_resize(c);
  g->pin.reserve(p.total);
  g->dev.reserve(p.total);
  fill_resize(g->pin.p, p, c, g->dev.p);
  if (!c.on_device) pack_sources(g->pin.p, p, c);
  HIP_CHECK(hipMemcpyAsync(g->dev.p, g->pin.p, p.total, hipMemcpyHostToDevice, s));       // tables and frames: one DMA
  const ResizeDesc* descs = (const ResizeDesc*)g->dev.p;
  const TileRef* tiles = (const TileRef*)(g->dev.p + p.tile_off);
  if (p.conv_tiles) rtd::rtd_launch(ingest_kernel, dim3((unsigned)p.conv_tiles), dim3(THREADS), 0, s, (const FrameDesc*)(g->dev.p + p.fdesc_off), tiles);
  if (p.fused_tiles) rtd::rtd_launch(resize_kernel<SRC_YUV>, dim3((unsigned)p.fused_tiles), dim3(THREADS), 0, s, descs, tiles + p.conv_tiles);
  if (p.bgr_tiles) rtd::rtd_launch(resize_kernel<SRC_BGR>, dim3((unsigned)p.bgr_tiles), dim3(THREADS), 0, s, descs, tiles + p.conv_tiles + p.fused_tiles);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
}

// what every call does around run(): nothing is copied or launched before the whole call has passed its checks
static int call(rtd_ingest* g, const ResizeCall& c) {
  return guarded(g, [&] {
    validate_resize(c);
    HIP_CHECK(hipSetDevice(g->device));
    try {
      run(g, c);
    } catch (...) {
      g->q.drain();                                        // nothing of a failed call may still read the staging buffers
      throw;
    }
  });
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
  return call(g, ResizeCall::convert(n, frames, frames_on_device != 0, out_dev));
}

int rtd_ingest_convert_resize(rtd_ingest_handle g, int32_t n, const rtd_yuv_frame* frames, int32_t frames_on_device, const int32_t* out_hw,
                              uint8_t* const* out_dev, uint8_t* const* native_out_dev) {
  return call(g, ResizeCall{n, frames, nullptr, frames_on_device != 0, out_hw, out_dev, native_out_dev});
}

int rtd_ingest_resize(rtd_ingest_handle g, int32_t n, const rtd_bgr_frame* frames, int32_t frames_on_device, const int32_t* out_hw,
                      uint8_t* const* out_dev) {
  return call(g, ResizeCall{n, nullptr, frames, frames_on_device != 0, out_hw, out_dev, nullptr});
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

int rtd_debug_resize_table(int32_t ssize, int32_t dsize, int32_t columns, int32_t* out, int32_t ssize2, int32_t dsize2, int32_t* is_area2,
                           int32_t tile_hw[2]) {
  static thread_local std::string err;
  return bk::caught(err, [&] {
    if (out) {
      RTD_CHECK(sides_ok(ssize, dsize), RTD_E_INVALID, "bad size (1..65535)");
      std::vector<LinEntry> t((size_t)dsize);
      resize_taps::linear_table(ssize, dsize, columns != 0, t.data());
      for (int32_t d = 0; d < dsize; ++d) out[4 * d] = t[(size_t)d].i0, out[4 * d + 1] = t[(size_t)d].i1, out[4 * d + 2] = t[(size_t)d].w0, out[4 * d + 3] = t[(size_t)d].w1;
    }
    if (is_area2) {
      RTD_CHECK(sides_ok(ssize, dsize) && sides_ok(ssize2, dsize2), RTD_E_INVALID, "bad size (1..65535)");
      *is_area2 = resize_taps::area2(ssize, ssize2, dsize, dsize2) ? 1 : 0;
    }
    if (tile_hw) tile_hw[0] = RTILE_H, tile_hw[1] = RTILE_W;
  });
}

}  // extern "C"
