// overlay.hip - detection overlays on a batch of HWC uint8 frames: filled rectangles, outlines and coverage masks (text), composited in
// list order (painter's algorithm), clipped to the frame, all in integers.  The restatement the bytes must equal is tests/overlay_ref.py.
// A frame is drawn where it lies in device memory, so an annotated frame can go on to the JPEG encoder without touching the host.
//
// One launch covers the whole call.  The host normalises the primitives (corners ordered, outer box and hole of an outline, clipped to
// the frame), drops those that miss their frame, and lists the 64 x 16 pixel tiles that some primitive paints; an outline counts as its
// four strips.  One workgroup per listed tile: it reads its frame's primitives in chunks of 256, keeps those that meet the tile (ballot
// compaction into LDS, order kept), and every thread walks the kept ones over its four pixels.  Only the bytes of painted pixels are
// stored, as bytes: with an odd W * C a dword can belong to two tiles, and a byte store of an owned byte needs no word of a neighbour.
#include <algorithm>
#include <mutex>
#include <new>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"

namespace overlay {

using rtd::Error;
namespace bk = rtd::backend;
using bk::TileRef;           // owner: the frame
using bk::align_up;
using bk::guarded;
using bk::sides_ok;

constexpr int TILE_W = 64, TILE_H = 16;
constexpr int THREADS = 256;
constexpr int ROWS_PER_THREAD = TILE_W * TILE_H / THREADS;      // 4: thread t owns column t % 64 of rows t / 64 + 4 k
constexpr int ROW_STEP = THREADS / TILE_W;
constexpr int CHUNK = THREADS;                                  // primitives examined per round: one per thread

struct DevPrim {             // 48 bytes; what the kernel reads (made on the host from rtd_overlay_prim)
  int x0, y0, x1, y1;        // FILL / OUTLINE: the painted box clipped to the frame, inclusive.  MASK: the mask's box, NOT clipped
  int hx0, hy0, hx1, hy1;    // OUTLINE: the hole (inclusive, clipped to the frame); empty (hx0 > hx1) otherwise
  uint32_t kind_bgr;         // kind << 24 | r << 16 | g << 8 | b
  int mask_w;
  int64_t mask_off;
};

struct FrameDesc {
  uint8_t* dst;
  int rows, cols, ch;
  int prim0, nprims;         // this frame's primitives in the flattened table
  int tiles_x;
};

__device__ inline bool meets_tile(const DevPrim& p, int X0, int Y0, int X1, int Y1) {
  if (p.x0 > X1 || p.x1 < X0 || p.y0 > Y1 || p.y1 < Y0) return false;
  return !(p.hx0 <= X0 && X1 <= p.hx1 && p.hy0 <= Y0 && Y1 <= p.hy1);       // a tile wholly inside an outline's hole stays as it is
}

template <int C>
__device__ inline void draw_tile(const FrameDesc& d, const DevPrim* __restrict__ prims, const uint8_t* __restrict__ masks, int tile, DevPrim* kept,
                                 int* wave_cnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tile % d.tiles_x, ty = tile / d.tiles_x;
  const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
  const int X1 = min(X0 + TILE_W, d.cols) - 1, Y1 = min(Y0 + TILE_H, d.rows) - 1;
  const int px = X0 + (tid & (TILE_W - 1)), py0 = Y0 + tid / TILE_W;

  uint32_t v[ROWS_PER_THREAD][C];                               // (words, and loops without early exits: everything stays in registers)
  uint32_t painted = 0;
  uint8_t* const col0 = d.dst + ((size_t)py0 * d.cols + px) * C;  // formed for every thread, used only for pixels inside the frame
  const size_t row_step = (size_t)ROW_STEP * d.cols * C;
#pragma unroll
  for (int k = 0; k < ROWS_PER_THREAD; ++k) {
    const bool in = px <= X1 && py0 + ROW_STEP * k <= Y1;
#pragma unroll
    for (int c = 0; c < C; ++c) v[k][c] = in ? (uint32_t)col0[k * row_step + c] : 0u;
  }

  for (int base = 0; base < d.nprims; base += CHUNK) {
    // ---- which primitives of this chunk meet the tile: kept in list order
    const int i = base + tid;
    const bool have = i < d.nprims;
    const DevPrim* pp = prims + d.prim0 + (have ? i : 0);
    const bool hit = have && meets_tile(*pp, X0, Y0, X1, Y1);
    const uint64_t m = __ballot(hit);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (hit) kept[before + __popcll(m & ((1ull << lane) - 1))] = *pp;
    __syncthreads();

    // ---- every thread walks them over its pixels
    for (int j = 0; j < total; ++j) {
      const DevPrim& q = kept[j];                               // the same address for the whole wave: an LDS broadcast
      const bool in_x = px >= q.x0 && px <= q.x1 && px <= X1;
      const uint32_t kb = q.kind_bgr;
      const bool is_mask = (kb >> 24) == RTD_OVL_MASK;
      const uint32_t col[3] = {kb & 0xffu, (kb >> 8) & 0xffu, (kb >> 16) & 0xffu};
      const bool in_hole_x = q.hx0 <= px && px <= q.hx1;
#pragma unroll
      for (int k = 0; k < ROWS_PER_THREAD; ++k) {
        const int py = py0 + ROW_STEP * k;
        if (in_x && py >= q.y0 && py <= q.y1 && py <= Y1) {
          uint32_t a = 255u;                                    // FILL / OUTLINE: full coverage outside the hole
          if (is_mask) a = masks[q.mask_off + (int64_t)(py - q.y0) * q.mask_w + (px - q.x0)];
          else if (in_hole_x && q.hy0 <= py && py <= q.hy1) a = 0u;
          if (a) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[k][c] = (v[k][c] * (255u - a) + col[c] * a + 127u) / 255u;   // a = 255: exactly col[c]
            painted |= 1u << k;
          }
        }
      }
    }
    __syncthreads();                                            // the next round overwrites kept[] and wave_cnt[]
  }

#pragma unroll
  for (int k = 0; k < ROWS_PER_THREAD; ++k) {
    if (painted & (1u << k)) {
#pragma unroll
      for (int c = 0; c < C; ++c) col0[k * row_step + c] = (uint8_t)v[k][c];
    }
  }
}

__global__ void __launch_bounds__(THREADS) overlay_kernel(const FrameDesc* __restrict__ descs, const DevPrim* __restrict__ prims,
                                                          const TileRef* __restrict__ tiles, const uint8_t* __restrict__ masks) {
  __shared__ DevPrim kept[CHUNK];
  __shared__ int wave_cnt[THREADS / 64];
  const TileRef t = tiles[blockIdx.x];
  const FrameDesc d = descs[t.owner];
  if (d.ch == 3) draw_tile<3>(d, prims, masks, t.tile, kept, wave_cnt);
  else draw_tile<1>(d, prims, masks, t.tile, kept, wave_cnt);
}

}  // namespace overlay

using namespace overlay;

struct rtd_overlay : bk::Base {
  bk::OwnStream q;
  bk::PinBuf pin;   // pinned: [descriptors | primitives | tiles | masks | host frames]
  bk::DevBuf dev;   // the same tables on the device (not the frames: they go straight to out_dev)
  std::vector<DevPrim> prims;            // host scratch, capacity kept between calls
  std::vector<TileRef> tiles;
  std::vector<uint8_t> marks;
  int64_t last_tiles = 0;
};

namespace overlay {

struct Box {                 // inclusive; empty when x0 > x1 or y0 > y1
  int64_t x0, y0, x1, y1;
  bool empty() const { return x0 > x1 || y0 > y1; }
  Box clip(int64_t W, int64_t H) const { return {std::max<int64_t>(x0, 0), std::max<int64_t>(y0, 0), std::min(x1, W - 1), std::min(y1, H - 1)}; }
};

static void mark(std::vector<uint8_t>& marks, int tiles_x, Box b, int W, int H) {
  b = b.clip(W, H);
  if (b.empty()) return;
  for (int64_t ty = b.y0 / TILE_H; ty <= b.y1 / TILE_H; ++ty)
    memset(&marks[(size_t)ty * tiles_x + b.x0 / TILE_W], 1, (size_t)(b.x1 / TILE_W - b.x0 / TILE_W + 1));
}

// checks every argument; nothing is copied or drawn before the whole call has passed
static void validate(int n, const uint8_t* const* frames, const int32_t* hwc, const int32_t* prim_counts, const rtd_overlay_prim* prims,
                     const uint8_t* masks, int64_t mask_bytes, uint8_t* const* out_dev) {
  RTD_CHECK(n <= RTD_OVERLAY_MAX_FRAMES, RTD_E_INVALID, "more than RTD_OVERLAY_MAX_FRAMES frames in one call");
  RTD_CHECK(frames && hwc && prim_counts && out_dev, RTD_E_INVALID, "null argument");
  RTD_CHECK(mask_bytes >= 0 && (masks || mask_bytes == 0), RTD_E_INVALID, "bad mask buffer");
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const std::string fi = "frame " + std::to_string(i);
    RTD_CHECK(frames[i] && out_dev[i], RTD_E_INVALID, fi + " has a null pointer");
    const int64_t H = hwc[3 * i], W = hwc[3 * i + 1], C = hwc[3 * i + 2];
    RTD_CHECK(sides_ok(H, W), RTD_E_INVALID, fi + " has a bad size (1..65535 per side)");
    RTD_CHECK(C == 1 || C == 3, RTD_E_INVALID, "frames must have 1 or 3 channels");
    RTD_CHECK(H * W * C < (1ll << 31), RTD_E_INVALID, fi + " has 2 GiB or more");
    RTD_CHECK(prim_counts[i] >= 0 && prim_counts[i] <= RTD_OVERLAY_MAX_PRIMS, RTD_E_INVALID,
              fi + " has " + std::to_string(prim_counts[i]) + " primitives (0..RTD_OVERLAY_MAX_PRIMS)");
    total += prim_counts[i];
  }
  RTD_CHECK(total == 0 || prims, RTD_E_INVALID, "null argument");
  for (int64_t k = 0; k < total; ++k) {
    const rtd_overlay_prim& p = prims[k];
    const std::string pk = "primitive " + std::to_string(k);
    RTD_CHECK(p.kind == RTD_OVL_FILL || p.kind == RTD_OVL_OUTLINE || p.kind == RTD_OVL_MASK, RTD_E_INVALID, pk + " has an unknown kind");
    if (p.kind == RTD_OVL_OUTLINE) RTD_CHECK(p.thickness >= 1 && p.thickness <= 65535, RTD_E_INVALID, pk + ": thickness must be in 1..65535");
    if (p.kind == RTD_OVL_MASK) {
      RTD_CHECK(p.x2 >= 0 && p.y2 >= 0 && p.x2 <= 65535 && p.y2 <= 65535, RTD_E_INVALID, pk + ": mask size must be in 0..65535 per side");
      RTD_CHECK(p.mask_offset >= 0 && p.mask_offset + (int64_t)p.x2 * p.y2 <= mask_bytes, RTD_E_INVALID, pk + ": its mask lies outside the mask buffer");
    }
  }
}

static void draw(rtd_overlay* o, int n, const uint8_t* const* frames, const int32_t* hwc, int on_device, const int32_t* prim_counts,
                 const rtd_overlay_prim* prims, const uint8_t* masks, int64_t mask_bytes, uint8_t* const* out_dev) {
  hipStream_t s = o->q.stream;
  // ---- the primitives the kernel will read, and the tiles they paint
  o->prims.clear();
  o->tiles.clear();
  std::vector<FrameDesc> descs(n);
  const rtd_overlay_prim* src = prims;
  for (int i = 0; i < n; ++i) {
    const int H = hwc[3 * i], W = hwc[3 * i + 1], C = hwc[3 * i + 2];
    FrameDesc& d = descs[i];
    d.dst = out_dev[i];
    d.rows = H;
    d.cols = W;
    d.ch = C;
    d.prim0 = (int)o->prims.size();
    d.tiles_x = (W + TILE_W - 1) / TILE_W;
    const int tiles_y = (H + TILE_H - 1) / TILE_H;
    o->marks.assign((size_t)d.tiles_x * tiles_y, 0);
    for (int k = 0; k < prim_counts[i]; ++k, ++src) {
      const rtd_overlay_prim& p = *src;
      DevPrim q;
      memset(&q, 0, sizeof q);
      q.hx0 = q.hy0 = 1;                                         // an empty hole
      q.hx1 = q.hy1 = 0;
      q.kind_bgr = ((uint32_t)p.kind << 24) | ((uint32_t)p.bgr[2] << 16) | ((uint32_t)p.bgr[1] << 8) | p.bgr[0];
      if (p.kind == RTD_OVL_MASK) {
        const Box b{p.x1, p.y1, (int64_t)p.x1 + p.x2 - 1, (int64_t)p.y1 + p.y2 - 1};
        if (b.clip(W, H).empty()) continue;                      // (so the box fits 32-bit integers: it reaches the frame and is < 65536 wide)
        q.x0 = (int)b.x0, q.y0 = (int)b.y0, q.x1 = (int)b.x1, q.y1 = (int)b.y1;
        q.mask_w = p.x2;
        q.mask_off = p.mask_offset;
        mark(o->marks, d.tiles_x, b, W, H);
      } else {
        const int64_t xl = std::min(p.x1, p.x2), xh = std::max(p.x1, p.x2), yl = std::min(p.y1, p.y2), yh = std::max(p.y1, p.y2);
        const int64_t out = p.kind == RTD_OVL_OUTLINE ? p.thickness / 2 : 0, in = p.kind == RTD_OVL_OUTLINE ? (p.thickness - 1) / 2 : 0;
        const Box outer{xl - out, yl - out, xh + out, yh + out};
        const Box oc = outer.clip(W, H);
        if (oc.empty()) continue;
        q.x0 = (int)oc.x0, q.y0 = (int)oc.y0, q.x1 = (int)oc.x1, q.y1 = (int)oc.y1;
        const Box hole{xl + in + 1, yl + in + 1, xh - in - 1, yh - in - 1};
        if (p.kind == RTD_OVL_FILL || hole.empty()) {
          mark(o->marks, d.tiles_x, outer, W, H);
        } else {
          const Box hc = hole.clip(W, H);
          if (!hc.empty()) q.hx0 = (int)hc.x0, q.hy0 = (int)hc.y0, q.hx1 = (int)hc.x1, q.hy1 = (int)hc.y1;
          mark(o->marks, d.tiles_x, {outer.x0, outer.y0, outer.x1, hole.y0 - 1}, W, H);      // top, bottom, left, right
          mark(o->marks, d.tiles_x, {outer.x0, hole.y1 + 1, outer.x1, outer.y1}, W, H);
          mark(o->marks, d.tiles_x, {outer.x0, hole.y0, hole.x0 - 1, hole.y1}, W, H);
          mark(o->marks, d.tiles_x, {hole.x1 + 1, hole.y0, outer.x1, hole.y1}, W, H);
        }
      }
      o->prims.push_back(q);
    }
    d.nprims = (int)o->prims.size() - d.prim0;
    for (size_t t = 0; t < o->marks.size(); ++t)
      if (o->marks[t]) o->tiles.push_back({i, (int)t});
  }
  RTD_CHECK(o->tiles.size() < (1ull << 31), RTD_E_INVALID, "the call paints 2^31 tiles or more");

  // ---- layout of the staging buffer
  const size_t prim_off = align_up(sizeof(FrameDesc) * n, 256);
  const size_t tile_off = align_up(prim_off + sizeof(DevPrim) * o->prims.size(), 256);
  const size_t mask_off = align_up(tile_off + sizeof(TileRef) * o->tiles.size(), 256);
  const size_t tables = align_up(mask_off + (size_t)mask_bytes, 256);
  std::vector<size_t> foff;
  const size_t total = bk::stage_offsets(n, hwc, on_device, tables, foff);
  o->pin.reserve(total);
  o->dev.reserve(tables);
  memcpy(o->pin.p, descs.data(), sizeof(FrameDesc) * n);
  if (!o->prims.empty()) memcpy(o->pin.p + prim_off, o->prims.data(), sizeof(DevPrim) * o->prims.size());
  if (!o->tiles.empty()) memcpy(o->pin.p + tile_off, o->tiles.data(), sizeof(TileRef) * o->tiles.size());
  if (mask_bytes) memcpy(o->pin.p + mask_off, masks, (size_t)mask_bytes);

  // ---- the frames arrive where they are drawn, then one launch
  for (int i = 0; i < n; ++i) {
    const size_t bytes = (size_t)hwc[3 * i] * hwc[3 * i + 1] * hwc[3 * i + 2];
    if (!on_device) {
      memcpy(o->pin.p + foff[i], frames[i], bytes);
      HIP_CHECK(hipMemcpyAsync(out_dev[i], o->pin.p + foff[i], bytes, hipMemcpyHostToDevice, s));
    } else if (frames[i] != out_dev[i]) {
      HIP_CHECK(hipMemcpyAsync(out_dev[i], frames[i], bytes, hipMemcpyDeviceToDevice, s));
    }
  }
  if (!o->tiles.empty()) {
    HIP_CHECK(hipMemcpyAsync(o->dev.p, o->pin.p, tables, hipMemcpyHostToDevice, s));
    rtd::rtd_launch(overlay_kernel, dim3((unsigned)o->tiles.size()), dim3(THREADS), 0, s, (const FrameDesc*)o->dev.p,
                    (const DevPrim*)(o->dev.p + prim_off), (const TileRef*)(o->dev.p + tile_off), (const uint8_t*)(o->dev.p + mask_off));
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipStreamSynchronize(s));
  o->last_tiles = (int64_t)o->tiles.size();
}

}  // namespace overlay

extern "C" {

int rtd_overlay_create(int32_t device, rtd_overlay_handle* out) {
  return bk::create(out, rtd_overlay_destroy, [&](rtd_overlay* o) {
    bk::use_device(device);
    o->device = device;
    o->q.open();
  });
}

int rtd_overlay_draw(rtd_overlay_handle o, int32_t n, const uint8_t* const* frames, const int32_t* hwc, int32_t frames_on_device,
                     const int32_t* prim_counts, const rtd_overlay_prim* prims, const uint8_t* masks, int64_t mask_bytes, uint8_t* const* out_dev) {
  return guarded(o, [&] {
    o->last_tiles = 0;
    RTD_CHECK(n >= 0, RTD_E_INVALID, "n must be >= 0");
    if (n == 0) return;
    validate(n, frames, hwc, prim_counts, prims, masks, mask_bytes, out_dev);
    HIP_CHECK(hipSetDevice(o->device));
    try {
      draw(o, n, frames, hwc, frames_on_device, prim_counts, prims, masks, mask_bytes, out_dev);
    } catch (...) {
      o->q.drain();                                        // nothing of a failed call may still read the staging buffers
      throw;
    }
  });
}

int rtd_overlay_wait_stream(rtd_overlay_handle o, void* producer_stream) {
  return guarded(o, [&] {
    HIP_CHECK(hipSetDevice(o->device));
    o->q.wait_for(producer_stream);
  });
}

const char* rtd_overlay_last_error(rtd_overlay_handle o) { return bk::last_error(o); }

void rtd_overlay_destroy(rtd_overlay_handle o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  o->q.drain();
  o->dev.release();
  o->pin.release();
  o->q.close();
  delete o;
}

int rtd_debug_overlay_tiles(rtd_overlay_handle o, int32_t* tile_h, int32_t* tile_w, int64_t* tiles) {
  return guarded(o, [&] {
    if (tile_h) *tile_h = TILE_H;
    if (tile_w) *tile_w = TILE_W;
    if (tiles) *tiles = o->last_tiles;
  });
}

}  // extern "C"
