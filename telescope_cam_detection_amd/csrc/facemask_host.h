// facemask_host.h - the pure host parts of the face masks (facemask.hip): the argument checks of a call, the padded rectangle, the
// layers that keep the reference's face order, the descriptors, tile lists and tables the kernels read (blur taps; OpenCV's resize
// index and weight tables, made here in the same double / float arithmetic as cv2 makes them), and where everything lies in the
// staging buffer.  No HIP here, so that tools/facemask_host_check.cpp can run all of it under the sanitizers on a CPU.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "call_parts.h"
#include "error.h"
#include "gauss_taps.h"
#include "resize_taps.h"

namespace facemask_host {

using rtd::backend::TileRef;         // owner: the face, an index into the descriptors; tile: K_PIX_SMALL's is the SMALL_TILE chunk
using rtd::backend::align_up;
using rtd::backend::sides_ok;

// a workgroup of THREADS threads takes one TILE_W x TILE_H pixel tile of a face's region (blur, nearest, box), or SMALL_TILE bytes of
// a pixelate face's `small` image
constexpr int TILE_W = 64, TILE_H = 16;
constexpr int THREADS = 256;
constexpr int SMALL_TILE = 4 * THREADS;
constexpr int MAX_K = RTD_FACEMASK_MAX_K, MAX_R = MAX_K / 2;
constexpr int64_t MAX_TILES = 1 << 24;                  // of all launches of a call together (the tile list is host and pinned memory)

enum : int32_t { F_AREA2 = 1 };                         // FaceDesc::flags: `small` is the 2 x 2 area mean
enum Kind : int { K_BLUR_ROWS = 0, K_BLUR_COLS, K_PIX_SMALL, K_PIX_NEAREST, K_BOX, KINDS };

struct FaceDesc {            // 80 bytes; what the kernels read, the same for every thread of a workgroup
  uint8_t* frame;            // the frame's first byte on the device
  int64_t scratch_off;       // bytes into the scratch plane: BLUR rh x rw x 3 uint16 row sums; PIXELATE sh x sw x 3 bytes of `small`
  int64_t table_off;         // bytes into the tables: BLUR 2 r + 1 uint16 taps; PIXELATE LinEntry[sw], LinEntry[sh], int32 xmap[rw], ymap[rh]
  int32_t W, H;              // the frame
  int32_t x1, y1, rw, rh;    // the region (BLACK_BOX: the inclusive box as x1, y1 and its width and height)
  int32_t style, radius;
  int32_t sw, sh;            // PIXELATE: the size of `small`
  int32_t flags, tiles_x;    // tiles_x: region tiles per row
  int32_t frame_index, reserved0;
};

struct Rect {                // x2, y2 exclusive
  int64_t x1, y1, x2, y2;
  bool empty() const { return x2 <= x1 || y2 <= y1; }
  bool meets(const Rect& o) const { return x1 < o.x2 && o.x1 < x2 && y1 < o.y2 && o.y1 < y2; }
};

// the reference's padded rectangle: p = int(w * 0.2) in Python's arithmetic (a double product, truncated towards zero)
inline Rect padded(const rtd_face_rect& f, int64_t W, int64_t H) {
  const int64_t p = (int64_t)((double)f.w * 0.2);
  return {std::max<int64_t>(0, (int64_t)f.x - p), std::max<int64_t>(0, (int64_t)f.y - p), std::min<int64_t>(W, (int64_t)f.x + f.w + p),
          std::min<int64_t>(H, (int64_t)f.y + f.h + p)};
}

// the pixels a face writes (and reads): its padded rectangle; a black box one more row and column where the frame allows it
inline Rect touched(const rtd_face_rect& f, int64_t W, int64_t H) {
  Rect r = padded(f, W, H);
  if (!r.empty() && f.style == RTD_FACE_BLACK_BOX) r.x2 = std::min(r.x2 + 1, W), r.y2 = std::min(r.y2 + 1, H);
  return r;
}

// checks every argument of a call but the frame pointers; nothing is copied or launched before the whole call has passed
inline void validate(int64_t n, const int32_t* hw, int64_t n_faces, const rtd_face_rect* faces) {
  RTD_CHECK(n >= 1 && n <= RTD_FACEMASK_MAX_FRAMES, RTD_E_INVALID, "1..RTD_FACEMASK_MAX_FRAMES frames per call");
  RTD_CHECK(n_faces >= 0 && n_faces <= RTD_FACEMASK_MAX_FACES, RTD_E_INVALID, "0..RTD_FACEMASK_MAX_FACES faces per call");
  RTD_CHECK(hw && (faces || n_faces == 0), RTD_E_INVALID, "null argument");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t H = hw[2 * i], W = hw[2 * i + 1];
    RTD_CHECK(sides_ok(H, W), RTD_E_INVALID, "frame " + std::to_string(i) + " has a bad size (1..65535 per side)");
    RTD_CHECK(H * W * 3 < (1ll << 31), RTD_E_INVALID, "frame " + std::to_string(i) + " has 2 GiB or more");
  }
  for (int64_t k = 0; k < n_faces; ++k) {
    const rtd_face_rect& f = faces[k];
    const std::string fk = "face " + std::to_string(k);
    RTD_CHECK(f.frame >= 0 && f.frame < n, RTD_E_INVALID, fk + " names a frame outside the call");
    RTD_CHECK(f.style == RTD_FACE_BLUR || f.style == RTD_FACE_PIXELATE || f.style == RTD_FACE_BLACK_BOX, RTD_E_INVALID, fk + " has an unknown style");
    if (f.style == RTD_FACE_BLUR)
      RTD_CHECK(f.k_or_blocks >= 1 && f.k_or_blocks <= MAX_K && f.k_or_blocks % 2 == 1, RTD_E_INVALID, fk + ": k must be odd and in 1..99");
    if (f.style == RTD_FACE_PIXELATE) RTD_CHECK(f.k_or_blocks >= 1, RTD_E_INVALID, fk + ": blocks must be >= 1");
  }
}

inline void validate_frames(int64_t n, uint8_t* const* frames) {
  RTD_CHECK(frames, RTD_E_INVALID, "null argument");
  for (int64_t i = 0; i < n; ++i) RTD_CHECK(frames[i], RTD_E_INVALID, "frame " + std::to_string(i) + " is a null pointer");
}

// ---- OpenCV's resize tables (imgproc/src/resize.cpp): the INTER_LINEAR index and weight tables and the 2 x 2 area rule are resize_taps.h,
// shared with the frame ingest's resize stage ------------------------------------------------------------------------------------------

using resize_taps::LinEntry;
using resize_taps::area2;
using resize_taps::cv_round;
using resize_taps::linear_table;
using resize_taps::resize_scale;

// resizeNN from ssize samples up to dsize: x_ofs[x] = min(cvFloor(x * ifx), ssize - 1) with ifx = 1. / ((double)dsize / ssize)
inline void nearest_table(int ssize, int dsize, int32_t* out) {
  const double fx = (double)dsize / ssize, ifx = 1. / fx;
  for (int x = 0; x < dsize; ++x) out[x] = std::min((int)floor(x * ifx), ssize - 1);
}

// ---- the plan of a call ----------------------------------------------------------------------------------------------------------------

struct Launch {
  int layer, kind;
  size_t tile0, ntiles;      // its slice of the tile list
};

struct Plan {
  int layers = 0;
  std::vector<int32_t> layer_of;       // per face of the call: its layer, -1 skipped
  std::vector<Rect> rects;             // per face of the call: its padded rectangle
  std::vector<FaceDesc> descs;         // the kept faces, in call order (frame still null: the caller knows where the frames lie)
  std::vector<TileRef> tiles;
  std::vector<uint8_t> tables;
  std::vector<Launch> launches;        // in stream order
  std::vector<uint8_t> frame_used;     // per frame: some kept face masks it
  size_t scratch_bytes = 0;            // the largest layer's
  int64_t kind_tiles[KINDS] = {0, 0, 0, 0, 0};
  // the staging buffer: [descriptors | tiles | tables | host frames, each on a 256-byte boundary]
  size_t tile_off = 0, table_off = 0, tables_end = 0, total = 0;
  std::vector<size_t> foff;
};

inline int64_t region_tiles(const FaceDesc& d) { return (int64_t)d.tiles_x * ((d.rh + TILE_H - 1) / TILE_H); }

template <typename T>
inline size_t table_room(std::vector<uint8_t>& tables, size_t count) {      // `count` T's on an 8-byte boundary: their offset
  const size_t at = align_up(tables.size(), 8);
  tables.resize(at + count * sizeof(T), 0);
  return at;
}

inline Plan plan(int n, const int32_t* hw, int n_faces, const rtd_face_rect* faces, bool on_device) {
  Plan p;
  p.layer_of.assign((size_t)n_faces, -1);
  p.rects.resize((size_t)n_faces);
  p.frame_used.assign((size_t)n, 0);
  // ---- layers: a face goes into the first layer after every earlier face of its frame that it meets
  std::vector<Rect> touch((size_t)n_faces);
  std::vector<int> kept;
  for (int k = 0; k < n_faces; ++k) {
    const rtd_face_rect& f = faces[k];
    const int64_t H = hw[2 * f.frame], W = hw[2 * f.frame + 1];
    p.rects[(size_t)k] = padded(f, W, H);
    touch[(size_t)k] = touched(f, W, H);
    if (p.rects[(size_t)k].empty()) continue;
    int layer = 0;
    for (int j : kept)
      if (faces[j].frame == f.frame && touch[(size_t)j].meets(touch[(size_t)k])) layer = std::max(layer, p.layer_of[(size_t)j] + 1);
    p.layer_of[(size_t)k] = layer;
    p.layers = std::max(p.layers, layer + 1);
    p.frame_used[(size_t)f.frame] = 1;
    kept.push_back(k);
  }
  // ---- descriptors and tables of the kept faces
  std::vector<int> layer_of_desc;
  for (int k : kept) {
    const rtd_face_rect& f = faces[k];
    const Rect r = f.style == RTD_FACE_BLACK_BOX ? touch[(size_t)k] : p.rects[(size_t)k];
    FaceDesc d;
    memset(&d, 0, sizeof d);
    d.H = hw[2 * f.frame], d.W = hw[2 * f.frame + 1];
    d.x1 = (int32_t)r.x1, d.y1 = (int32_t)r.y1, d.rw = (int32_t)(r.x2 - r.x1), d.rh = (int32_t)(r.y2 - r.y1);
    d.style = f.style, d.frame_index = f.frame;
    d.tiles_x = (d.rw + TILE_W - 1) / TILE_W;
    if (f.style == RTD_FACE_BLUR) {
      d.radius = f.k_or_blocks / 2;
      d.table_off = (int64_t)table_room<uint16_t>(p.tables, (size_t)f.k_or_blocks);
      gauss8::tap_rule(f.k_or_blocks, (uint16_t*)(p.tables.data() + d.table_off));
    } else if (f.style == RTD_FACE_PIXELATE) {
      d.sw = std::max(1, d.rw / f.k_or_blocks), d.sh = std::max(1, d.rh / f.k_or_blocks);
      d.flags = area2(d.rw, d.rh, d.sw, d.sh) ? F_AREA2 : 0;
      // the two maps follow the entries directly (12 (sw + sh) is a multiple of 4)
      d.table_off = (int64_t)table_room<uint8_t>(p.tables, sizeof(LinEntry) * ((size_t)d.sw + d.sh) + sizeof(int32_t) * ((size_t)d.rw + d.rh));
      LinEntry* xs = (LinEntry*)(p.tables.data() + d.table_off);
      linear_table(d.rw, d.sw, true, xs);
      linear_table(d.rh, d.sh, false, xs + d.sw);
      int32_t* xmap = (int32_t*)(xs + d.sw + d.sh);
      nearest_table(d.sw, d.rw, xmap);
      nearest_table(d.sh, d.rh, xmap + d.rw);
    }
    p.descs.push_back(d);
    layer_of_desc.push_back(p.layer_of[(size_t)k]);
  }
  // ---- per layer: the scratch of its faces, and one tile list per launch
  for (int layer = 0; layer < p.layers; ++layer) {
    size_t scratch = 0;
    for (size_t i = 0; i < p.descs.size(); ++i) {
      FaceDesc& d = p.descs[i];
      if (layer_of_desc[i] != layer || d.style == RTD_FACE_BLACK_BOX) continue;
      d.scratch_off = (int64_t)scratch;
      const size_t bytes = d.style == RTD_FACE_BLUR ? (size_t)d.rh * d.rw * 3 * sizeof(uint16_t) : (size_t)d.sh * d.sw * 3;
      scratch = align_up(scratch + bytes, 256);
    }
    p.scratch_bytes = std::max(p.scratch_bytes, scratch);
    for (int kind = 0; kind < KINDS; ++kind) {
      const int style = kind <= K_BLUR_COLS ? RTD_FACE_BLUR : kind <= K_PIX_NEAREST ? RTD_FACE_PIXELATE : RTD_FACE_BLACK_BOX;
      const size_t tile0 = p.tiles.size();
      for (size_t i = 0; i < p.descs.size(); ++i) {
        const FaceDesc& d = p.descs[i];
        if (layer_of_desc[i] != layer || d.style != style) continue;
        const int64_t cnt = kind == K_PIX_SMALL ? ((int64_t)d.sh * d.sw * 3 + SMALL_TILE - 1) / SMALL_TILE : region_tiles(d);
        RTD_CHECK((int64_t)p.tiles.size() + cnt <= MAX_TILES, RTD_E_INVALID, "the call masks more than 2^24 tiles");
        for (int64_t t = 0; t < cnt; ++t) p.tiles.push_back({(int32_t)i, (int32_t)t});
      }
      if (p.tiles.size() > tile0) {
        p.launches.push_back({layer, kind, tile0, p.tiles.size() - tile0});
        p.kind_tiles[kind] += (int64_t)(p.tiles.size() - tile0);
      }
    }
  }
  // ---- the staging buffer
  p.tile_off = align_up(sizeof(FaceDesc) * p.descs.size(), 256);
  p.table_off = align_up(p.tile_off + sizeof(TileRef) * p.tiles.size(), 256);
  p.tables_end = align_up(p.table_off + p.tables.size(), 256);
  p.foff.assign((size_t)n, 0);
  size_t at = p.tables_end;
  for (int i = 0; i < n; ++i) {
    p.foff[(size_t)i] = at;
    if (!on_device && p.frame_used[(size_t)i]) at = align_up(at + (size_t)hw[2 * i] * hw[2 * i + 1] * 3, 256);
  }
  p.total = at;
  return p;
}

// writes the tables of a call into `stage` (p.tables_end bytes): frame_at[i] is where the kernels find frame i
inline void fill_tables(uint8_t* stage, const Plan& p, uint8_t* const* frame_at) {
  FaceDesc* descs = (FaceDesc*)stage;
  for (size_t i = 0; i < p.descs.size(); ++i) {
    descs[i] = p.descs[i];
    descs[i].frame = frame_at[p.descs[i].frame_index];
  }
  if (!p.tiles.empty()) memcpy(stage + p.tile_off, p.tiles.data(), sizeof(TileRef) * p.tiles.size());
  if (!p.tables.empty()) memcpy(stage + p.table_off, p.tables.data(), p.tables.size());
}

}  // namespace facemask_host
