// Stand-alone check of the pure host parts of the frame ingest (csrc/ingest_host.h): the constants, the argument checks, the staging
// layout, the packing of host frames with padded pitches (exact-size heap copies: a read or write past a plane is a sanitizer report)
// and the descriptors and tile list the kernel reads.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/ingest_host_check.cpp -o ingest_host_check && ./ingest_host_check
#include <stdio.h>
#include <stdlib.h>

#include "../telescope_cam_detection_amd/csrc/ingest_host.h"

namespace ih = ingest_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

template <typename F>
static int code_of(F&& f) {
  try { f(); return RTD_OK; } catch (const rtd::Error& e) { return e.code; }
}

// a frame with padded pitches whose planes are separate exact-size heap blocks
struct HostFrame {
  rtd_yuv_frame f;
  uint8_t *y, *u, *v;
  HostFrame(int W, int H, int layout, int ypad, int cpad) {
    memset(&f, 0, sizeof f);
    const int crow = (int)ih::chroma_row(layout, W), ch = (int)ih::chroma_h(H);
    f.width = W, f.height = H, f.layout = layout, f.y_pitch = W + ypad, f.c_pitch = crow + cpad;
    // the last row of a plane ends with the row, not with the pitch
    const size_t ysz = (size_t)(H - 1) * f.y_pitch + W, csz = (size_t)(ch - 1) * f.c_pitch + crow;
    y = (uint8_t*)malloc(ysz), u = (uint8_t*)malloc(csz), v = ih::interleaved(layout) ? nullptr : (uint8_t*)malloc(csz);
    for (size_t i = 0; i < ysz; ++i) y[i] = (uint8_t)(i * 7 + 1);
    for (size_t i = 0; i < csz; ++i) u[i] = (uint8_t)(i * 5 + 2);
    if (v) for (size_t i = 0; i < csz; ++i) v[i] = (uint8_t)(i * 3 + 3);
    f.y = y, f.u = u, f.v = v;
  }
  ~HostFrame() { free(y), free(u), free(v); }
};

int main() {
  // ---- constants
  const int32_t want[2][2][5] = {{{1220542, 1673527, -852492, -409993, 2116026}, {1048576, 1470104, -748683, -360710, 1858077}},
                                 {{1220542, 1880097, -558891, -223347, 2214593}, {1048576, 1651507, -490734, -196084, 1946157}}};
  for (int m = 0; m < 2; ++m)
    for (int r = 0; r < 2; ++r) {
      int32_t c[5];
      ih::coeffs(m, r, c);
      CHECK(memcmp(c, want[m][r], sizeof c) == 0);
    }
  int32_t c5[5];
  CHECK(code_of([&] { ih::coeffs(2, 0, c5); }) == RTD_E_INVALID && code_of([&] { ih::coeffs(0, -1, c5); }) == RTD_E_INVALID);
  CHECK(ih::frame_bytes(2, 2) == 6 && ih::frame_bytes(1, 1) == 3 && ih::frame_bytes(3, 5) == 27 && ih::frame_bytes(1080, 1920) == 3110400);
  CHECK(sizeof(ih::FrameDesc) == 80 && sizeof(rtd_yuv_frame) == 56);

  // ---- argument checks
  {
    HostFrame a(5, 3, RTD_YUV_NV12, 13, 5), b(4, 8, RTD_YUV_I420, 0, 0);
    rtd_yuv_frame fr[2] = {a.f, b.f};
    uint8_t o0, o1;
    uint8_t* outs[2] = {&o0, &o1};
    CHECK(code_of([&] { ih::validate(2, fr, outs); }) == RTD_OK);
    CHECK(code_of([&] { ih::validate(0, fr, outs); }) == RTD_E_INVALID && code_of([&] { ih::validate(65, fr, outs); }) == RTD_E_INVALID);
    CHECK(code_of([&] { ih::validate(2, nullptr, outs); }) == RTD_E_INVALID && code_of([&] { ih::validate(2, fr, nullptr); }) == RTD_E_INVALID);
    auto bad = [&](auto edit) {
      rtd_yuv_frame g[2] = {a.f, b.f};
      uint8_t* po[2] = {&o0, &o1};
      edit(g, po);
      std::string msg;
      try { ih::validate(2, g, po); } catch (const rtd::Error& e) { CHECK(e.code == RTD_E_INVALID); msg = e.what(); }
      return msg;
    };
    CHECK(bad([](auto* g, auto** o) { g[1].width = 0; }).find("frame 1") == 0);
    CHECK(bad([](auto* g, auto** o) { g[0].height = 65536; }).find("frame 0") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].y_pitch = 3; }).find("frame 1") == 0);
    CHECK(bad([](auto* g, auto** o) { g[0].c_pitch = 5; }).find("frame 0") == 0);      // NV12, W = 5: a chroma row is 6 bytes
    CHECK(bad([](auto* g, auto** o) { g[1].c_pitch = 1; }).find("frame 1") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].v = nullptr; }).find("frame 1") == 0);      // I420 needs v
    CHECK(bad([](auto* g, auto** o) { g[0].v = nullptr; }).empty());                   // NV12 does not
    CHECK(bad([](auto* g, auto** o) { g[0].y = nullptr; }).find("frame 0") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].u = nullptr; }).find("frame 1") == 0);
    CHECK(bad([](auto* g, auto** o) { o[1] = nullptr; }).find("frame 1") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].layout = 3; }).find("frame 1") == 0);
    CHECK(bad([](auto* g, auto** o) { g[0].matrix = -1; }).find("frame 0") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].full_range = 2; }).find("frame 1") == 0);
  }

  // ---- plan, pack and tables over a sweep of sizes, layouts and paddings
  for (int H : {1, 2, 3, 5, 16, 17, 37})
    for (int W : {1, 2, 3, 5, 6, 8, 10, 53, 256, 257})
      for (int layout : {RTD_YUV_NV12, RTD_YUV_NV21, RTD_YUV_I420})
        for (int pad : {0, 1, 13}) {
          HostFrame a(W, H, layout, pad, pad), b(2, 2, RTD_YUV_I420, 0, 3);
          a.f.matrix = RTD_YUV_BT709, a.f.full_range = 1;
          rtd_yuv_frame fr[2] = {a.f, b.f};
          for (bool on_device : {false, true}) {
            const ih::Plan p = ih::plan(2, fr, on_device);
            const int64_t tiles = (int64_t)((W + ih::TILE_W - 1) / ih::TILE_W) * ((H + ih::TILE_H - 1) / ih::TILE_H) + 1;
            CHECK(p.tiles == tiles && p.tile_off % 256 == 0 && p.tables % 256 == 0 && p.tile_off >= 2 * sizeof(ih::FrameDesc));
            CHECK(p.tables >= p.tile_off + (size_t)tiles * sizeof(ih::TileRef));
            CHECK(p.foff[0] == p.tables && p.foff[0] % 256 == 0 && p.foff[1] % 256 == 0);
            CHECK(on_device ? p.total == p.tables : p.total >= p.foff[1] + 6 && p.foff[1] >= p.foff[0] + (size_t)ih::frame_bytes(H, W));
            uint8_t* stage = (uint8_t*)malloc(p.total);     // exact size
            memset(stage, 0xEE, p.total);
            uint8_t* const dev_base = (uint8_t*)0x10000000;   // never dereferenced
            uint8_t* outs[2] = {(uint8_t*)0x20000000, (uint8_t*)0x30000001};
            ih::fill_tables(stage, p, 2, fr, on_device, dev_base, outs);
            const ih::FrameDesc* d = (const ih::FrameDesc*)stage;
            const ih::TileRef* t = (const ih::TileRef*)(stage + p.tile_off);
            CHECK(d[0].W == W && d[0].H == H && d[0].dst == outs[0] && d[0].ybias == 0 && d[0].cy == 1048576 && d[0].cvr == 1651507 && d[1].ybias == 16);
            CHECK(t[0].frame == 0 && t[0].tile == 0 && t[tiles - 1].frame == 1 && t[tiles - 1].tile == 0 && t[tiles - 2].tile == (int32_t)tiles - 2);
            CHECK(!(d[1].flags & ih::F_WIDE));              // W = 2, and an odd output address
            CHECK(!!(d[0].flags & ih::F_INTERLEAVED) == (layout != RTD_YUV_I420) && !!(d[0].flags & ih::F_SWAP) == (layout == RTD_YUV_NV21));
            if (on_device) {
              CHECK(d[0].y == a.f.y && d[0].u == a.f.u && d[0].y_pitch == W + pad);
              CHECK(!!(d[0].flags & ih::F_WIDE) == ((((uintptr_t)a.f.y | (uintptr_t)a.f.u | (uintptr_t)d[0].v | W | (W + pad) | d[0].c_pitch) & 3) == 0));
            } else {
              CHECK(d[0].y == dev_base + p.foff[0] && d[0].u == d[0].y + (size_t)H * W && d[0].y_pitch == W);
              CHECK(d[0].c_pitch == (int32_t)ih::chroma_row(layout, W));
              const size_t ch = (size_t)ih::chroma_h(H), cw = (size_t)ih::chroma_w(W);
              if (layout == RTD_YUV_I420) CHECK(d[0].v == d[0].u + ch * cw);
              // wide exactly when every row starts on a dword: W % 4 == 0 and, for I420, a V plane that does too
              CHECK(!!(d[0].flags & ih::F_WIDE) == (W % 4 == 0 && (layout != RTD_YUV_I420 || (ch * cw) % 4 == 0)));
              ih::pack_frame(stage + p.foff[0], fr[0]);
              ih::pack_frame(stage + p.foff[1], fr[1]);
              const uint8_t* q = stage + p.foff[0];
              for (int r = 0; r < H; ++r) CHECK(memcmp(q + (size_t)r * W, a.y + (size_t)r * a.f.y_pitch, (size_t)W) == 0);
              const size_t crow = (size_t)ih::chroma_row(layout, W);
              for (size_t r = 0; r < ch; ++r) CHECK(memcmp(q + (size_t)H * W + r * crow, a.u + r * a.f.c_pitch, crow) == 0);
              if (layout == RTD_YUV_I420)
                for (size_t r = 0; r < ch; ++r) CHECK(memcmp(q + (size_t)H * W + (ch + r) * crow, a.v + r * a.f.c_pitch, crow) == 0);
              if (p.foff[1] > p.foff[0] + (size_t)ih::frame_bytes(H, W)) CHECK(stage[p.foff[0] + (size_t)ih::frame_bytes(H, W)] == 0xEE);   // nothing past the frame
            }
            free(stage);
          }
        }
  printf("ingest host check ok\n");
  return 0;
}
