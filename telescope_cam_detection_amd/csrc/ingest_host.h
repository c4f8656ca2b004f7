// ingest_host.h - the pure host parts of the frame ingest (ingest.hip): the conversion constants, and ONE call path for its three
// calls (a convert call is a resize call whose frames have only a native output): the argument checks, the plan of the staging buffer,
// the descriptors, tile lists and tap tables (resize_taps.h) the kernels read, and where host frames lie.  No HIP here, so that
// tools/ingest_host_check.cpp can run all of it under the sanitizers on a CPU.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "call_parts.h"
#include "error.h"
#include "resize_taps.h"

namespace ingest_host {

using rtd::backend::TileRef;         // owner: the frame
using rtd::backend::align_up;
using rtd::backend::sides_ok;

// a thread converts PX pixels of two rows (PX / 2 chroma samples); a workgroup of TX x TY threads one tile
constexpr int PX = 8;
constexpr int TX = 32, TY = 8;
constexpr int THREADS = TX * TY;
constexpr int TILE_W = TX * PX, TILE_H = TY * 2;                 // 256 x 16 pixels

enum : int32_t { F_WIDE = 1, F_INTERLEAVED = 2, F_SWAP = 4 };   // FrameDesc::flags

struct FrameDesc {           // 80 bytes; what the kernel reads, the same for every thread of a workgroup
  const uint8_t* y;
  const uint8_t* u;          // F_INTERLEAVED: the pair plane
  const uint8_t* v;
  uint8_t* dst;
  int32_t W, H, y_pitch, c_pitch;
  int32_t tiles_x, flags, ybias;
  int32_t cy, cvr, cvg, cug, cub;
};

// THE constants: floor(c 2^20 + 0.5) of the decimal coefficients, order CY, CVR, CVG, CUG, CUB
inline void coeffs(int32_t matrix, int32_t full_range, int32_t out[5]) {
  RTD_CHECK(matrix == RTD_YUV_BT601 || matrix == RTD_YUV_BT709, RTD_E_INVALID, "unknown matrix");
  RTD_CHECK(full_range == 0 || full_range == 1, RTD_E_INVALID, "unknown range");
  static const double C[2][2][5] = {
      {{1.164, 1.596, -0.813, -0.391, 2.018}, {1.0, 1.402, -0.714, -0.344, 1.772}},     // BT.601 limited (OpenCV's own), full
      {{1.164, 1.793, -0.533, -0.213, 2.112}, {1.0, 1.575, -0.468, -0.187, 1.856}}};    // BT.709 limited, full
  for (int k = 0; k < 5; ++k) {
    const double s = C[matrix][full_range][k] * 1048576.0 + 0.5;
    int64_t f = (int64_t)s;                                      // (truncates towards zero)
    if ((double)f > s) --f;
    out[k] = (int32_t)f;
  }
}

inline int64_t chroma_w(int64_t W) { return (W + 1) / 2; }
inline int64_t chroma_h(int64_t H) { return (H + 1) / 2; }
inline bool interleaved(int32_t layout) { return layout != RTD_YUV_I420; }
// bytes of a chroma row
inline int64_t chroma_row(int32_t layout, int64_t W) { return interleaved(layout) ? 2 * chroma_w(W) : chroma_w(W); }
// bytes of a tightly packed frame: what ffmpeg's rawvideo writes
inline int64_t frame_bytes(int64_t H, int64_t W) { return H * W + 2 * chroma_w(W) * chroma_h(H); }

// everything about frame i but its pointers
inline void check_shape(int i, const rtd_yuv_frame& f) {
  const std::string fi = "frame " + std::to_string(i);
  RTD_CHECK(f.layout == RTD_YUV_NV12 || f.layout == RTD_YUV_NV21 || f.layout == RTD_YUV_I420, RTD_E_INVALID, fi + " has an unknown layout");
  RTD_CHECK(f.matrix == RTD_YUV_BT601 || f.matrix == RTD_YUV_BT709, RTD_E_INVALID, fi + " has an unknown matrix");
  RTD_CHECK(f.full_range == 0 || f.full_range == 1, RTD_E_INVALID, fi + " has an unknown range (0 limited, 1 full)");
  RTD_CHECK(sides_ok(f.width, f.height), RTD_E_INVALID, fi + " has a bad size (1..65535 per side)");
  RTD_CHECK(f.y_pitch >= f.width, RTD_E_INVALID, fi + ": y_pitch is less than a luma row");
  RTD_CHECK(f.c_pitch >= chroma_row(f.layout, f.width), RTD_E_INVALID, fi + ": c_pitch is less than a chroma row");
}

inline int64_t tiles_of(const rtd_yuv_frame& f) {
  return (int64_t)((f.width + TILE_W - 1) / TILE_W) * ((f.height + TILE_H - 1) / TILE_H);
}

// a host frame, row by row, into frame_bytes(H, W) bytes at dst: luma, then the chroma plane(s)
inline void pack_frame(uint8_t* dst, const rtd_yuv_frame& f) {
  const size_t W = (size_t)f.width, H = (size_t)f.height, ch = (size_t)chroma_h(f.height), crow = (size_t)chroma_row(f.layout, f.width);
  for (size_t r = 0; r < H; ++r) memcpy(dst + r * W, f.y + r * (size_t)f.y_pitch, W);
  dst += H * W;
  for (size_t r = 0; r < ch; ++r) memcpy(dst + r * crow, f.u + r * (size_t)f.c_pitch, crow);
  if (!interleaved(f.layout)) {
    dst += ch * crow;
    for (size_t r = 0; r < ch; ++r) memcpy(dst + r * crow, f.v + r * (size_t)f.c_pitch, crow);
  }
}

// the descriptor of frame i as the kernel reads it: `f` with the planes where the kernel finds them (a host frame: its packed copy
// on the device).  The dword-wide path needs every row of every plane and of the output on a 4-byte boundary.
inline FrameDesc describe(const rtd_yuv_frame& f, uint8_t* dst) {
  FrameDesc d;
  memset(&d, 0, sizeof d);
  d.y = f.y, d.u = f.u, d.v = interleaved(f.layout) ? f.u : f.v, d.dst = dst;
  d.W = f.width, d.H = f.height, d.y_pitch = f.y_pitch, d.c_pitch = f.c_pitch;
  d.tiles_x = (f.width + TILE_W - 1) / TILE_W;
  const uintptr_t bits = (uintptr_t)d.y | (uintptr_t)d.u | (uintptr_t)d.v | (uintptr_t)dst | (uintptr_t)f.y_pitch | (uintptr_t)f.c_pitch | (uintptr_t)f.width;
  d.flags = ((bits & 3) == 0 ? F_WIDE : 0) | (interleaved(f.layout) ? F_INTERLEAVED : 0) | (f.layout == RTD_YUV_NV21 ? F_SWAP : 0);
  d.ybias = f.full_range ? 0 : 16;
  int32_t c[5];
  coeffs(f.matrix, f.full_range, c);
  d.cy = c[0], d.cvr = c[1], d.cvg = c[2], d.cug = c[3], d.cub = c[4];
  return d;
}

// a packed frame at `base`: the tight frame description of `f`
inline rtd_yuv_frame packed_at(const rtd_yuv_frame& f, const uint8_t* base) {
  rtd_yuv_frame t = f;
  t.y = base;
  t.u = base + (size_t)f.height * (size_t)f.width;
  t.v = interleaved(f.layout) ? nullptr : t.u + (size_t)chroma_h(f.height) * (size_t)chroma_w(f.width);
  t.y_pitch = f.width;
  t.c_pitch = (int32_t)chroma_row(f.layout, f.width);
  return t;
}

// ---- a call: rtd_ingest_convert, rtd_ingest_convert_resize or rtd_ingest_resize ----------------------------------------------------------

using resize_taps::LinEntry;

// a thread makes RPX output pixels of one row; a workgroup of TX x TY threads one tile of RTILE_W x RTILE_H output pixels.  On the 2 x 2
// area path that is the convert kernel's source strip (8 pixels of two rows) and tile (256 x 16)
constexpr int RPX = 4;
constexpr int RTILE_W = TX * RPX, RTILE_H = TY;                 // 128 x 8 output pixels
constexpr int64_t MAX_RTILES = 1 << 24;                         // of all launches of a call together (the tile list is pinned memory)

enum : int32_t { R_AREA = 1, R_SRC_WIDE = 2, R_DST_WIDE = 4 };  // ResizeDesc::rflags

struct ResizeDesc {          // 112 bytes; what the resize kernel reads, the same for every thread of a workgroup
  FrameDesc src;             // the source: 4:2:0 planes as the convert kernel reads them, or BGR (y: first byte, y_pitch: bytes per row); dst unused
  uint8_t* out;
  const LinEntry* tab;       // the linear path: OW column entries, then OH row entries (null on the area path)
  int32_t OW, OH, tiles_x, rflags;
};

// the arguments of any of the three calls in one shape: exactly one of yuv / bgr is set.  rtd_ingest_convert is the call without
// resized outputs (`resizes` false, out_hw and out unused): its out_dev are the native outputs, and each frame must have one
struct ResizeCall {
  int n;
  const rtd_yuv_frame* yuv;
  const rtd_bgr_frame* bgr;
  bool on_device;
  const int32_t* out_hw;
  uint8_t* const* out;
  uint8_t* const* native;    // a resize call: may be null, and so may its entries
  bool resizes = true;
  static ResizeCall convert(int n, const rtd_yuv_frame* frames, bool on_device, uint8_t* const* out_dev) {
    return {n, frames, nullptr, on_device, nullptr, nullptr, out_dev, false};
  }
  int sw(int i) const { return yuv ? yuv[i].width : bgr[i].width; }
  int sh(int i) const { return yuv ? yuv[i].height : bgr[i].height; }
  int oh(int i) const { return out_hw[2 * i]; }
  int ow(int i) const { return out_hw[2 * i + 1]; }
  uint8_t* native_of(int i) const { return native ? native[i] : nullptr; }
  // the fused kernel reads frame i's planes; otherwise the BGR kernel reads the frame, or the native frame the convert kernel wrote
  bool fused(int i) const { return resizes && yuv && !native_of(i); }
  size_t host_bytes(int i) const { return yuv ? (size_t)frame_bytes(sh(i), sw(i)) : (size_t)sh(i) * (size_t)sw(i) * 3; }
};

inline int64_t rtiles_of(int oh, int ow) { return (int64_t)((ow + RTILE_W - 1) / RTILE_W) * ((oh + RTILE_H - 1) / RTILE_H); }

inline void check_bgr(int i, const rtd_bgr_frame& f) {
  const std::string fi = "frame " + std::to_string(i);
  RTD_CHECK(sides_ok(f.width, f.height), RTD_E_INVALID, fi + " has a bad size (1..65535 per side)");
  RTD_CHECK((int64_t)f.pitch >= 3 * (int64_t)f.width, RTD_E_INVALID, fi + ": pitch is less than a row of BGR pixels");
  RTD_CHECK(f.data, RTD_E_INVALID, fi + " has a null source");
}

// checks every argument of a call; nothing is copied or launched before the whole call has passed.  The limit of 2^24 tiles and the
// rule that no two outputs share a byte are the resize calls' alone: a convert call is accepted as it always was
inline void validate_resize(const ResizeCall& c) {
  RTD_CHECK(c.n >= 1 && c.n <= RTD_INGEST_MAX_FRAMES, RTD_E_INVALID, "1..RTD_INGEST_MAX_FRAMES frames per call");
  RTD_CHECK((c.yuv || c.bgr) && (c.resizes ? c.out_hw && c.out : c.native != nullptr), RTD_E_INVALID, "null argument");
  int64_t tiles = 0;
  struct Range { uintptr_t a, b; int frame; const char* what; };
  std::vector<Range> ranges;
  for (int i = 0; i < c.n; ++i) {
    const std::string fi = "frame " + std::to_string(i);
    if (c.yuv) {
      const rtd_yuv_frame& f = c.yuv[i];
      check_shape(i, f);
      RTD_CHECK(f.y && f.u && (interleaved(f.layout) || f.v), RTD_E_INVALID, fi + " has a null plane");
    } else {
      check_bgr(i, c.bgr[i]);
    }
    if (!c.resizes) {
      RTD_CHECK(c.native[i], RTD_E_INVALID, fi + " has a null output");
      continue;
    }
    RTD_CHECK(sides_ok(c.oh(i), c.ow(i)), RTD_E_INVALID, fi + " has a bad output size (1..65535 per side)");
    RTD_CHECK(c.out[i], RTD_E_INVALID, fi + " has a null output");
    tiles += rtiles_of(c.oh(i), c.ow(i));
    ranges.push_back({(uintptr_t)c.out[i], (uintptr_t)c.out[i] + (uintptr_t)c.oh(i) * (uintptr_t)c.ow(i) * 3, i, "output"});
    if (c.native_of(i)) {
      tiles += tiles_of(c.yuv[i]);
      ranges.push_back({(uintptr_t)c.native_of(i), (uintptr_t)c.native_of(i) + (uintptr_t)c.sh(i) * (uintptr_t)c.sw(i) * 3, i, "native output"});
    }
    RTD_CHECK(tiles <= MAX_RTILES, RTD_E_INVALID, fi + ": the call has more than 2^24 tiles");
  }
  for (size_t k = 1; k < ranges.size(); ++k)
    for (size_t j = 0; j < k; ++j)
      RTD_CHECK(ranges[k].b <= ranges[j].a || ranges[j].b <= ranges[k].a, RTD_E_INVALID,
                "frame " + std::to_string(ranges[k].frame) + ": its " + ranges[k].what + " shares memory with the " + ranges[j].what + " of frame " +
                    std::to_string(ranges[j].frame));
}

// the staging buffer of a call: [resize descriptors | convert descriptors (native outputs) | tiles: convert, fused, BGR | tap tables |
// host frames, tightly packed, each on a 256-byte boundary], each part on a 256-byte boundary.  A part nothing reads takes no room:
// a convert call is [convert descriptors | tiles | host frames]
struct ResizePlan {
  size_t fdesc_off = 0, tile_off = 0, table_off = 0, tables_end = 0, total = 0;
  int64_t conv_tiles = 0, fused_tiles = 0, bgr_tiles = 0;       // the three launches' slices of the tile list, in this order
  std::vector<uint8_t> area;                                    // per frame: the 2 x 2 mean
  std::vector<size_t> toff;                                     // per frame: where its tables lie (linear frames)
  std::vector<uint8_t> shared;                                  // per frame: its tables are those of an earlier frame of the same sizes
  std::vector<size_t> foff;                                     // host frames: where frame i goes
};

inline ResizePlan plan_resize(const ResizeCall& c) {
  ResizePlan p;
  const size_t n = (size_t)c.n;
  p.area.resize(n), p.toff.assign(n, 0), p.shared.assign(n, 0), p.foff.assign(n, 0);
  bool any_native = false;
  for (int i = 0; i < c.n; ++i) {
    if (c.native_of(i)) p.conv_tiles += tiles_of(c.yuv[i]), any_native = true;
    if (!c.resizes) continue;
    p.area[(size_t)i] = resize_taps::area2(c.sw(i), c.sh(i), c.ow(i), c.oh(i)) ? 1 : 0;
    const int64_t t = rtiles_of(c.oh(i), c.ow(i));
    if (c.fused(i)) p.fused_tiles += t;
    else p.bgr_tiles += t;
  }
  p.fdesc_off = align_up(c.resizes ? sizeof(ResizeDesc) * n : 0, 256);
  p.tile_off = align_up(p.fdesc_off + (any_native ? sizeof(FrameDesc) * n : 0), 256);
  p.table_off = align_up(p.tile_off + sizeof(TileRef) * (size_t)(p.conv_tiles + p.fused_tiles + p.bgr_tiles), 256);
  size_t at = p.table_off;
  for (int i = 0; i < c.n; ++i) {
    p.toff[(size_t)i] = at;
    if (!c.resizes || p.area[(size_t)i]) continue;
    for (int j = 0; j < i && !p.shared[(size_t)i]; ++j)         // the cameras of a site mostly share one size: one pair of tables for them
      if (!p.area[(size_t)j] && c.sw(j) == c.sw(i) && c.sh(j) == c.sh(i) && c.ow(j) == c.ow(i) && c.oh(j) == c.oh(i))
        p.toff[(size_t)i] = p.toff[(size_t)j], p.shared[(size_t)i] = 1;
    if (!p.shared[(size_t)i]) at = align_up(at + sizeof(LinEntry) * ((size_t)c.ow(i) + (size_t)c.oh(i)), 16);
  }
  p.tables_end = at = align_up(at, 256);
  for (int i = 0; i < c.n; ++i) {
    p.foff[(size_t)i] = at;
    if (!c.on_device) at = align_up(at + c.host_bytes(i), 256);
  }
  p.total = at;
  return p;
}

// a host BGR frame, row by row, into 3 H W bytes at dst
inline void pack_bgr(uint8_t* dst, const rtd_bgr_frame& f) {
  const size_t row = 3 * (size_t)f.width;
  for (size_t r = 0; r < (size_t)f.height; ++r) memcpy(dst + r * row, f.data + r * (size_t)f.pitch, row);
}

// the host frames of a call into stage + foff[i]
inline void pack_sources(uint8_t* stage, const ResizePlan& p, const ResizeCall& c) {
  for (int i = 0; i < c.n; ++i) {
    if (c.yuv) pack_frame(stage + p.foff[(size_t)i], c.yuv[i]);
    else pack_bgr(stage + p.foff[(size_t)i], c.bgr[i]);
  }
}

// writes the tables of a call into `stage` (p.tables_end bytes); the staging buffer's twin on the device starts at dev_base.  Frame i's
// planes are the caller's (device frames) or its packed copy at dev_base + foff[i] (host frames: pack_sources)
inline void fill_resize(uint8_t* stage, const ResizePlan& p, const ResizeCall& c, const uint8_t* dev_base) {
  ResizeDesc* descs = (ResizeDesc*)stage;
  FrameDesc* conv = (FrameDesc*)(stage + p.fdesc_off);
  TileRef* tiles = (TileRef*)(stage + p.tile_off);
  int64_t kc = 0, kf = p.conv_tiles, kb = p.conv_tiles + p.fused_tiles;
  for (int i = 0; i < c.n; ++i) {
    const size_t si = (size_t)i;
    ResizeDesc d;
    memset(&d, 0, sizeof d);
    uintptr_t bits = 0;                                         // every address and pitch the source rows start from
    if (c.yuv) {
      const rtd_yuv_frame f = c.on_device ? c.yuv[i] : packed_at(c.yuv[i], dev_base + p.foff[si]);
      if (c.native_of(i)) {
        conv[i] = describe(f, c.native_of(i));
        const int32_t cnt = (int32_t)tiles_of(f);
        for (int32_t t = 0; t < cnt; ++t) tiles[kc++] = {i, t};
      } else if (p.conv_tiles) {
        memset(&conv[i], 0, sizeof(FrameDesc));
      }
      if (!c.resizes) continue;
      d.src = describe(f, nullptr);
      bits = (uintptr_t)d.src.y | (uintptr_t)d.src.u | (uintptr_t)d.src.v | (uintptr_t)f.y_pitch | (uintptr_t)f.c_pitch;
    }
    if (!c.fused(i)) {                                          // a BGR source: the caller's frame, its packed copy, or the native output
      const uint8_t* data = c.yuv ? c.native_of(i) : c.on_device ? c.bgr[i].data : dev_base + p.foff[si];
      const int32_t pitch = c.yuv || !c.on_device ? 3 * c.sw(i) : c.bgr[i].pitch;
      memset(&d.src, 0, sizeof d.src);
      d.src.y = data, d.src.y_pitch = pitch, d.src.W = c.sw(i), d.src.H = c.sh(i);
      bits = (uintptr_t)data | (uintptr_t)pitch;
    }
    d.out = c.out[i];
    d.OW = c.ow(i), d.OH = c.oh(i);
    d.tiles_x = (d.OW + RTILE_W - 1) / RTILE_W;
    const bool dst_wide = (((uintptr_t)d.out | (uintptr_t)(3 * (int64_t)d.OW)) & 3) == 0;
    d.rflags = (p.area[si] ? R_AREA : 0) | ((bits & 3) == 0 ? R_SRC_WIDE : 0) | (dst_wide ? R_DST_WIDE : 0);
    if (!p.area[si]) {
      LinEntry* tab = (LinEntry*)(stage + p.toff[si]);
      if (!p.shared[si]) {
        resize_taps::linear_table(c.sw(i), d.OW, true, tab);
        resize_taps::linear_table(c.sh(i), d.OH, false, tab + d.OW);
      }
      d.tab = (const LinEntry*)(dev_base + p.toff[si]);
    }
    descs[i] = d;
    const int32_t cnt = (int32_t)rtiles_of(d.OH, d.OW);
    int64_t& k = c.fused(i) ? kf : kb;
    for (int32_t t = 0; t < cnt; ++t) tiles[k++] = {i, t};
  }
}

}  // namespace ingest_host
