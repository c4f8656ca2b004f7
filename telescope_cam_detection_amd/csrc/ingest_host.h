// ingest_host.h - the pure host parts of the frame ingest (ingest.hip): the conversion constants, the argument checks of a call, the
// descriptors and tile list the kernel reads, and where host frames lie in the staging buffer.  No HIP here, so that
// tools/ingest_host_check.cpp can run all of it under the sanitizers on a CPU.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "error.h"

namespace ingest_host {

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

struct TileRef {
  int32_t frame, tile;       // tile = ty * tiles_x + tx
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

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
  RTD_CHECK(f.width >= 1 && f.height >= 1 && f.width <= 65535 && f.height <= 65535, RTD_E_INVALID, fi + " has a bad size (1..65535 per side)");
  RTD_CHECK(f.y_pitch >= f.width, RTD_E_INVALID, fi + ": y_pitch is less than a luma row");
  RTD_CHECK(f.c_pitch >= chroma_row(f.layout, f.width), RTD_E_INVALID, fi + ": c_pitch is less than a chroma row");
}

// checks every argument of a call; nothing is copied or launched before the whole call has passed
inline void validate(int n, const rtd_yuv_frame* frames, uint8_t* const* out_dev) {
  RTD_CHECK(n >= 1 && n <= RTD_INGEST_MAX_FRAMES, RTD_E_INVALID, "1..RTD_INGEST_MAX_FRAMES frames per call");
  RTD_CHECK(frames && out_dev, RTD_E_INVALID, "null argument");
  for (int i = 0; i < n; ++i) {
    const rtd_yuv_frame& f = frames[i];
    const std::string fi = "frame " + std::to_string(i);
    check_shape(i, f);
    RTD_CHECK(f.y && f.u && (interleaved(f.layout) || f.v), RTD_E_INVALID, fi + " has a null plane");
    RTD_CHECK(out_dev[i], RTD_E_INVALID, fi + " has a null output");
  }
}

inline int64_t tiles_of(const rtd_yuv_frame& f) {
  return (int64_t)((f.width + TILE_W - 1) / TILE_W) * ((f.height + TILE_H - 1) / TILE_H);
}

// the staging buffer of a call: [descriptors | tiles | host frames, tightly packed, each on a 256-byte boundary]
struct Plan {
  size_t tile_off = 0, tables = 0, total = 0;   // tables: what the kernel's tables take; total: with the host frames
  int64_t tiles = 0;
  std::vector<size_t> foff;                     // host frames: where frame i's luma goes
};

inline Plan plan(int n, const rtd_yuv_frame* frames, bool on_device) {
  Plan p;
  for (int i = 0; i < n; ++i) p.tiles += tiles_of(frames[i]);
  p.tile_off = align_up(sizeof(FrameDesc) * (size_t)n, 256);
  p.tables = align_up(p.tile_off + sizeof(TileRef) * (size_t)p.tiles, 256);
  p.foff.resize((size_t)n);
  size_t at = p.tables;
  for (int i = 0; i < n; ++i) {
    p.foff[(size_t)i] = at;
    if (!on_device) at = align_up(at + (size_t)frame_bytes(frames[i].height, frames[i].width), 256);
  }
  p.total = at;
  return p;
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

// writes the tables of a call into `stage` (plan().tables bytes): frame i's planes are frames[i]'s (device frames) or its packed copy at
// dev_base + foff[i] (host frames, which are packed into stage + foff[i] by the caller)
inline void fill_tables(uint8_t* stage, const Plan& p, int n, const rtd_yuv_frame* frames, bool on_device, const uint8_t* dev_base,
                        uint8_t* const* out_dev) {
  FrameDesc* descs = (FrameDesc*)stage;
  TileRef* tiles = (TileRef*)(stage + p.tile_off);
  int64_t k = 0;
  for (int i = 0; i < n; ++i) {
    descs[i] = describe(on_device ? frames[i] : packed_at(frames[i], dev_base + p.foff[(size_t)i]), out_dev[i]);
    const int32_t cnt = (int32_t)tiles_of(frames[i]);
    for (int32_t t = 0; t < cnt; ++t) tiles[k++] = {i, t};
  }
}

}  // namespace ingest_host
