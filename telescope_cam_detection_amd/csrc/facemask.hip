// facemask.hip - privacy face masks on HWC uint8 BGR frames where they lie in device memory: the reference's FaceMasker.apply_mask
// (cv2.GaussianBlur, cv2.resize, cv2.rectangle on the padded face rectangle), all in integers.  The restatement the bytes must equal is
// tests/face_ref.py; the host side (checks, padded rectangles, layers, tile lists, tables, staging layout) is facemask_host.h.
//
// A face is masked IN PLACE, so nothing a workgroup writes may be what another one still reads as its halo: every style that reads
// the frame is two launches with a scratch plane between them.  BLUR: the row pass reads the frame and writes 16-bit row sums to the
// scratch, the column pass reads the scratch and writes the frame.  PIXELATE: `small` goes to the scratch, the nearest pass writes the
// frame.  BLACK_BOX reads nothing and is one launch.  The host sorts the faces of a call into layers whose faces are disjoint (the
// reference applies them one after another); a layer is one launch (pair) per style present, over a flattened tile list of all its
// faces, one workgroup per tile, the face's descriptor the same for all its threads.  Layers follow each other on the handle's stream.
//
// Halos are staged through LDS: a row tile is 16 rows of 64 + 2 r pixels (7.6 KiB for r = 49), a column tile 16 + 2 r rows of 64 pixels
// of uint16 (42.75 KiB: three workgroups per CU).  The radius is a run-time value: the taps come from the face's table into LDS.
// A thread stores exactly the bytes of its own pixels, as bytes: with an odd 3 W a dword of the frame belongs to two rows, and a
// region starts at any byte.
#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "facemask_host.h"
#include "gauss8.h"
#include "global_bytes.h"

namespace facemask {

using rtd::Error;
namespace bk = rtd::backend;
using bk::guarded;
using namespace facemask_host;

// (the descriptors' pointers are read through global_bytes.h's address_space(1) types: global_* instead of flat_* instructions)
constexpr int ROW_LDS = (TILE_W + 2 * MAX_R) * 3;       // bytes of one staged row of the row pass
constexpr int COL_LDS = TILE_W * 3;                     // values of one staged row of the column pass

struct Tile {
  int x0, y0, tw, th;        // inside the region
};
__device__ inline Tile tile_of(const FaceDesc& d, int tile) {
  Tile t;
  t.x0 = (tile % d.tiles_x) * TILE_W, t.y0 = (tile / d.tiles_x) * TILE_H;
  t.tw = min(TILE_W, d.rw - t.x0), t.th = min(TILE_H, d.rh - t.y0);
  return t;
}
// byte (y, x, 0) of the region in its frame
__device__ inline size_t frame_at(const FaceDesc& d, int y, int x) { return ((size_t)(d.y1 + y) * d.W + (d.x1 + x)) * 3; }

// hlineSmooth: R[y][x][c] = sum_j taps[j] * region[y][reflect101(x - r + j)][c], exact in 16 bits
__global__ void __launch_bounds__(THREADS) facemask_blur_rows(const FaceDesc* __restrict__ descs, const TileRef* __restrict__ tiles,
                                                              const uint8_t* __restrict__ tables, uint8_t* __restrict__ scratch) {
  __shared__ uint8_t src[TILE_H * ROW_LDS];
  __shared__ uint16_t taps[MAX_K + 1];
  const TileRef tr = tiles[blockIdx.x];
  const FaceDesc d = descs[tr.owner];
  const Tile t = tile_of(d, tr.tile);
  const int tid = threadIdx.x, r = d.radius, k = 2 * r + 1;
  if (tid < k) taps[tid] = ((GHalf)(tables + d.table_off))[tid];
  const GBytes frame = (GBytes)d.frame;
  const int gw = t.tw + 2 * r;                                   // staged pixels per row: at most 64 + 98
  for (int i = tid; i < t.th * gw; i += THREADS) {
    const int row = i / gw, gx = i - row * gw;
    const GBytes p = frame + frame_at(d, t.y0 + row, gauss8::reflect101(t.x0 - r + gx, d.rw));
    uint8_t* s = src + row * ROW_LDS + gx * 3;
    s[0] = p[0], s[1] = p[1], s[2] = p[2];
  }
  __syncthreads();
  const int ew = t.tw * 3;                                       // bytes of a tile row: a value per byte, its taps 3 bytes apart
  const GOutHalf out = (GOutHalf)(scratch + d.scratch_off);
  for (int i = tid; i < t.th * ew; i += THREADS) {
    const int row = i / ew, e = i - row * ew;
    const uint8_t* s = src + row * ROW_LDS + e;
    uint32_t acc = 0;
    for (int j = 0; j < k; ++j) acc += (uint32_t)taps[j] * s[3 * j];
    out[((size_t)(t.y0 + row) * d.rw + t.x0) * 3 + e] = (uint16_t)acc;
  }
}

// vlineSmooth: out[y][x][c] = (sum_i taps[i] * R[reflect101(y - r + i)][x][c] + 32768) >> 16
__global__ void __launch_bounds__(THREADS) facemask_blur_cols(const FaceDesc* __restrict__ descs, const TileRef* __restrict__ tiles,
                                                              const uint8_t* __restrict__ tables, const uint8_t* __restrict__ scratch) {
  __shared__ uint16_t rows[(TILE_H + 2 * MAX_R) * COL_LDS];
  __shared__ uint16_t taps[MAX_K + 1];
  const TileRef tr = tiles[blockIdx.x];
  const FaceDesc d = descs[tr.owner];
  const Tile t = tile_of(d, tr.tile);
  const int tid = threadIdx.x, r = d.radius, k = 2 * r + 1;
  if (tid < k) taps[tid] = ((GHalf)(tables + d.table_off))[tid];
  const GHalf in = (GHalf)(scratch + d.scratch_off);
  const int ew = t.tw * 3, gh = t.th + 2 * r;                    // staged rows: at most 16 + 98
  for (int i = tid; i < gh * ew; i += THREADS) {
    const int gy = i / ew, e = i - gy * ew;
    rows[gy * COL_LDS + e] = in[((size_t)gauss8::reflect101(t.y0 - r + gy, d.rh) * d.rw + t.x0) * 3 + e];
  }
  __syncthreads();
  const GOut frame = (GOut)d.frame;
  for (int i = tid; i < t.th * ew; i += THREADS) {
    const int row = i / ew, e = i - row * ew;
    const uint16_t* s = rows + row * COL_LDS + e;
    uint32_t acc = 0;
    for (int j = 0; j < k; ++j) acc += (uint32_t)taps[j] * s[j * COL_LDS];
    frame[frame_at(d, t.y0 + row, t.x0) + e] = (uint8_t)((acc + 32768u) >> 16);
  }
}

// resize(region, (sw, sh), INTER_LINEAR) on 8-bit input, the tables from the host and the pixel rule resize_taps.h's (area8, linear8):
// a thread makes four bytes of `small`
__global__ void __launch_bounds__(THREADS) facemask_pix_small(const FaceDesc* __restrict__ descs, const TileRef* __restrict__ tiles,
                                                              const uint8_t* __restrict__ tables, uint8_t* __restrict__ scratch) {
  const TileRef tr = tiles[blockIdx.x];
  const FaceDesc d = descs[tr.owner];
  const GBytes frame = (GBytes)d.frame;
  const GLin xs = (GLin)(tables + d.table_off), ys = xs + d.sw;
  const GOut small = (GOut)(scratch + d.scratch_off);
  const int64_t total = (int64_t)d.sh * d.sw * 3;
  const size_t pitch = (size_t)d.W * 3;
  for (int q = 0; q < SMALL_TILE / THREADS; ++q) {
    const int64_t idx = (int64_t)tr.tile * SMALL_TILE + q * THREADS + (int)threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % 3), px = (int)(idx / 3), dx = px % d.sw, dy = px / d.sw;
    int v;
    if (d.flags & F_AREA2) {
      const GBytes p = frame + frame_at(d, 2 * dy, 2 * dx) + c;
      v = resize_taps::area8(p[0], p[3], p[pitch], p[pitch + 3]);
    } else {
      const int xi0 = xs[dx].i0, xi1 = xs[dx].i1, a0 = xs[dx].w0, a1 = xs[dx].w1;
      const int b0 = ys[dy].w0, b1 = ys[dy].w1;
      const GBytes r0 = frame + frame_at(d, ys[dy].i0, 0) + c, r1 = frame + frame_at(d, ys[dy].i1, 0) + c;
      v = resize_taps::linear8(r0[3 * xi0], r0[3 * xi1], r1[3 * xi0], r1[3 * xi1], a0, a1, b0, b1);
    }
    small[idx] = (uint8_t)v;
  }
}

// resize(small, (rw, rh), INTER_NEAREST): resizeNN's x_ofs and its row rule, both from the host
__global__ void __launch_bounds__(THREADS) facemask_pix_nearest(const FaceDesc* __restrict__ descs, const TileRef* __restrict__ tiles,
                                                                const uint8_t* __restrict__ tables, const uint8_t* __restrict__ scratch) {
  const TileRef tr = tiles[blockIdx.x];
  const FaceDesc d = descs[tr.owner];
  const Tile t = tile_of(d, tr.tile);
  const GInt xmap = (GInt)(tables + d.table_off + sizeof(LinEntry) * ((size_t)d.sw + d.sh)), ymap = xmap + d.rw;
  const GBytes small = (GBytes)(scratch + d.scratch_off);
  const GOut frame = (GOut)d.frame;
  const int ew = t.tw * 3;
  for (int i = threadIdx.x; i < t.th * ew; i += THREADS) {
    const int row = i / ew, e = i - row * ew, px = e / 3, c = e - 3 * px;
    frame[frame_at(d, t.y0 + row, t.x0) + e] = small[((size_t)ymap[t.y0 + row] * d.sw + xmap[t.x0 + px]) * 3 + c];
  }
}

// cv2.rectangle(frame, (x1, y1), (x2, y2), (0, 0, 0), -1): the host has made the inclusive box a region
__global__ void __launch_bounds__(THREADS) facemask_box(const FaceDesc* __restrict__ descs, const TileRef* __restrict__ tiles) {
  const TileRef tr = tiles[blockIdx.x];
  const FaceDesc d = descs[tr.owner];
  const Tile t = tile_of(d, tr.tile);
  const GOut frame = (GOut)d.frame;
  const int ew = t.tw * 3;
  for (int i = threadIdx.x; i < t.th * ew; i += THREADS) {
    const int row = i / ew, e = i - row * ew;
    frame[frame_at(d, t.y0 + row, t.x0) + e] = 0;
  }
}

// RGB2Gray<uchar> on BGR: (1868 B + 9617 G + 4899 R + 8192) >> 14.  A thread makes four pixels and stores them as one dword (the plane
// is pinned host memory: a store crosses the bus); the last, shorter group goes byte by byte.  `wide`: the frame starts on a dword.
__device__ inline uint32_t gray_of(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

__global__ void __launch_bounds__(THREADS) facemask_gray(const uint8_t* __restrict__ frame_, uint8_t* __restrict__ gray_, int64_t npix, int wide) {
  const GBytes frame = (GBytes)frame_;
  const GOut gray = (GOut)gray_;
  const int64_t p0 = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 4;
  if (p0 >= npix) return;
  if (p0 + 4 <= npix) {
    uint32_t w[3];
    if (wide) {
      const GWord q = (GWord)(frame + 3 * p0);                  // 12 bytes from a dword boundary
      w[0] = q[0], w[1] = q[1], w[2] = q[2];
    } else {
      const GBytes q = frame + 3 * p0;
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = (uint32_t)q[4 * k] | (uint32_t)q[4 * k + 1] << 8 | (uint32_t)q[4 * k + 2] << 16 | (uint32_t)q[4 * k + 3] << 24;
    }
    uint32_t out = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      uint32_t ch[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) ch[c] = byte_of(w, 3 * p + c);
      out |= gray_of(ch[0], ch[1], ch[2]) << (8 * p);
    }
    *(GOutWord)(gray + p0) = out;                               // (the plane starts on a dword and p0 is a multiple of 4)
  } else {
    for (int64_t p = p0; p < npix; ++p) gray[p] = (uint8_t)gray_of(frame[3 * p], frame[3 * p + 1], frame[3 * p + 2]);
  }
}

}  // namespace facemask

using namespace facemask;

struct rtd_facemask : bk::Base {
  bk::OwnStream q;
  bk::PinBuf pin;       // pinned: [descriptors | tiles | tables | host frames]
  bk::DevBuf dev;       // its twin on the device
  bk::DevBuf scratch;   // the plane between the two launches of a style: the largest layer's
  bk::PinBuf gray;      // the gray plane the kernel writes
};

namespace facemask {

static void apply(rtd_facemask* m, int n, uint8_t* const* frames, const int32_t* hw, bool on_device, int n_faces, const rtd_face_rect* faces) {
  hipStream_t s = m->q.stream;
  const Plan p = plan(n, hw, n_faces, faces, on_device);
  if (p.launches.empty()) return;                                // no face, or only empty rectangles: the frames stay as they are
  m->pin.reserve(p.total);
  m->dev.reserve(p.total);
  m->scratch.reserve(p.scratch_bytes);
  std::vector<uint8_t*> where((size_t)n);                        // a host frame is masked in its uploaded copy
  for (int i = 0; i < n; ++i) where[(size_t)i] = on_device ? frames[i] : m->dev.p + p.foff[(size_t)i];
  fill_tables(m->pin.p, p, where.data());
  if (!on_device)
    for (int i = 0; i < n; ++i)
      if (p.frame_used[(size_t)i]) memcpy(m->pin.p + p.foff[(size_t)i], frames[i], (size_t)hw[2 * i] * hw[2 * i + 1] * 3);
  HIP_CHECK(hipMemcpyAsync(m->dev.p, m->pin.p, p.total, hipMemcpyHostToDevice, s));         // tables and host frames: one DMA
  const FaceDesc* descs = (const FaceDesc*)m->dev.p;
  const uint8_t* tables = m->dev.p + p.table_off;
  for (const Launch& l : p.launches) {
    const TileRef* tiles = (const TileRef*)(m->dev.p + p.tile_off) + l.tile0;
    const dim3 grid((unsigned)l.ntiles), block(THREADS);
    switch (l.kind) {
      case K_BLUR_ROWS: rtd::rtd_launch(facemask_blur_rows, grid, block, 0, s, descs, tiles, tables, m->scratch.p); break;
      case K_BLUR_COLS: rtd::rtd_launch(facemask_blur_cols, grid, block, 0, s, descs, tiles, tables, (const uint8_t*)m->scratch.p); break;
      case K_PIX_SMALL: rtd::rtd_launch(facemask_pix_small, grid, block, 0, s, descs, tiles, tables, m->scratch.p); break;
      case K_PIX_NEAREST: rtd::rtd_launch(facemask_pix_nearest, grid, block, 0, s, descs, tiles, tables, (const uint8_t*)m->scratch.p); break;
      default: rtd::rtd_launch(facemask_box, grid, block, 0, s, descs, tiles); break;
    }
    HIP_CHECK(hipGetLastError());
  }
  if (!on_device && p.total > p.tables_end)
    HIP_CHECK(hipMemcpyAsync(m->pin.p + p.tables_end, m->dev.p + p.tables_end, p.total - p.tables_end, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (!on_device)
    for (int i = 0; i < n; ++i)
      if (p.frame_used[(size_t)i]) memcpy(frames[i], m->pin.p + p.foff[(size_t)i], (size_t)hw[2 * i] * hw[2 * i + 1] * 3);
}

static void gray_plane(rtd_facemask* m, const uint8_t* frame_dev, int rows, int cols, uint8_t* gray_out) {
  hipStream_t s = m->q.stream;
  const int64_t npix = (int64_t)rows * cols;
  m->gray.reserve((size_t)npix);
  const int64_t groups = (npix + 3) / 4;
  rtd::rtd_launch(facemask_gray, dim3((unsigned)((groups + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, frame_dev, m->gray.p, npix,
                  (int)(((uintptr_t)frame_dev & 3) == 0));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  memcpy(gray_out, m->gray.p, (size_t)npix);
}

}  // namespace facemask

extern "C" {

int rtd_facemask_create(int32_t device, rtd_facemask_handle* out) {
  return bk::create(out, rtd_facemask_destroy, [&](rtd_facemask* m) {
    bk::use_device(device);
    m->device = device;
    m->q.open();
  });
}

int rtd_facemask_apply(rtd_facemask_handle m, int32_t n, uint8_t* const* frames, const int32_t* hw, int32_t frames_on_device, int32_t n_faces,
                       const rtd_face_rect* faces) {
  return guarded(m, [&] {
    validate(n, hw, n_faces, faces);
    validate_frames(n, frames);
    HIP_CHECK(hipSetDevice(m->device));
    try {
      apply(m, n, frames, hw, frames_on_device != 0, n_faces, faces);
    } catch (...) {
      m->q.drain();                                        // nothing of a failed call may still read the staging buffers
      throw;
    }
  });
}

int rtd_facemask_gray(rtd_facemask_handle m, const uint8_t* frame_dev, int32_t rows, int32_t cols, uint8_t* gray_out) {
  return guarded(m, [&] {
    RTD_CHECK(frame_dev && gray_out, RTD_E_INVALID, "null argument");
    RTD_CHECK(sides_ok(rows, cols), RTD_E_INVALID, "the frame has a bad size (1..65535 per side)");
    HIP_CHECK(hipSetDevice(m->device));
    try {
      gray_plane(m, frame_dev, rows, cols, gray_out);
    } catch (...) {
      m->q.drain();
      throw;
    }
  });
}

int rtd_facemask_wait_stream(rtd_facemask_handle m, void* producer_stream) {
  return guarded(m, [&] {
    HIP_CHECK(hipSetDevice(m->device));
    m->q.wait_for(producer_stream);
  });
}

const char* rtd_facemask_last_error(rtd_facemask_handle m) { return bk::last_error(m); }

void rtd_facemask_destroy(rtd_facemask_handle m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  m->q.drain();
  m->scratch.release();
  m->gray.release();
  m->dev.release();
  m->pin.release();
  m->q.close();
  delete m;
}

int rtd_debug_facemask_plan(int32_t n, const int32_t* hw, int32_t n_faces, const rtd_face_rect* faces, int32_t* layers, int32_t* layer_of,
                            int32_t* rects, int32_t* tile_h, int32_t* tile_w, int64_t* tiles, int32_t taps_k, uint16_t* taps) {
  return bk::caught(bk::create_error<rtd_facemask>(), [&] {
    if (tile_h) *tile_h = TILE_H;
    if (tile_w) *tile_w = TILE_W;
    if (taps_k != 0 || taps) {
      RTD_CHECK(taps && taps_k >= 1 && taps_k <= MAX_K && taps_k % 2 == 1, RTD_E_INVALID, "taps: k must be odd and in 1..99");
      gauss8::tap_rule(taps_k, taps);
    }
    if (n == 0 && !hw && !faces) return;                   // the tile or the taps alone
    validate(n, hw, n_faces, faces);
    const Plan p = plan(n, hw, n_faces, faces, true);
    if (layers) *layers = p.layers;
    for (int k = 0; k < n_faces; ++k) {
      if (layer_of) layer_of[k] = p.layer_of[(size_t)k];
      const Rect& r = p.rects[(size_t)k];
      if (rects) rects[4 * k] = (int32_t)r.x1, rects[4 * k + 1] = (int32_t)r.y1, rects[4 * k + 2] = (int32_t)r.x2, rects[4 * k + 3] = (int32_t)r.y2;
    }
    if (tiles) memcpy(tiles, p.kind_tiles, sizeof p.kind_tiles);
  });
}

}  // extern "C"
