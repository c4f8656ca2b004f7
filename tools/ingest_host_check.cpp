// Stand-alone check of the pure host parts of the frame ingest (csrc/ingest_host.h, csrc/resize_taps.h, csrc/call_parts.h): the
// constants, the cv2 pixel rule against hand-worked values, the tap tables, the argument checks of all three calls (limits, null
// pointers, outputs that share memory - a resize call's rule, not a convert call's), the staging layout, the descriptors and tile lists
// of the three launches, and the packing of host frames with padded pitches (planes and BGR frames are exact-size heap blocks: a read
// or write past one is a sanitizer report).
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/ingest_host_check.cpp -o ingest_host_check && ./ingest_host_check
#include <stdio.h>
#include <stdlib.h>

#include "../telescope_cam_detection_amd/csrc/ingest_host.h"

namespace ih = ingest_host;
namespace rt = resize_taps;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

// a 4:2:0 frame with padded pitches whose planes are separate exact-size heap blocks
struct HostFrame {
  rtd_yuv_frame f;
  uint8_t *y, *u, *v;
  HostFrame(int W, int H, int layout, int ypad, int cpad) {
    memset(&f, 0, sizeof f);
    const int crow = (int)ih::chroma_row(layout, W), ch = (int)ih::chroma_h(H);
    f.width = W, f.height = H, f.layout = layout, f.y_pitch = W + ypad, f.c_pitch = crow + cpad;
    const size_t ysz = (size_t)(H - 1) * f.y_pitch + W, csz = (size_t)(ch - 1) * f.c_pitch + crow;
    y = (uint8_t*)malloc(ysz), u = (uint8_t*)malloc(csz), v = ih::interleaved(layout) ? nullptr : (uint8_t*)malloc(csz);
    for (size_t i = 0; i < ysz; ++i) y[i] = (uint8_t)(i * 7 + 1);
    for (size_t i = 0; i < csz; ++i) u[i] = (uint8_t)(i * 5 + 2);
    if (v) for (size_t i = 0; i < csz; ++i) v[i] = (uint8_t)(i * 3 + 3);
    f.y = y, f.u = u, f.v = v;
  }
  ~HostFrame() { free(y), free(u), free(v); }
};

// a BGR frame with a padded pitch: the last row ends with the row, not with the pitch
struct HostBgr {
  rtd_bgr_frame f;
  uint8_t* p;
  HostBgr(int W, int H, int pad) {
    memset(&f, 0, sizeof f);
    f.width = W, f.height = H, f.pitch = 3 * W + pad;
    const size_t sz = (size_t)(H - 1) * f.pitch + 3 * (size_t)W;
    p = (uint8_t*)malloc(sz);
    for (size_t i = 0; i < sz; ++i) p[i] = (uint8_t)(i * 11 + 5);
    f.data = p;
  }
  ~HostBgr() { free(p); }
};

static std::string refusal(const ih::ResizeCall& c) {
  try { ih::validate_resize(c); } catch (const rtd::Error& e) { CHECK(e.code == RTD_E_INVALID); return e.what(); }
  return "";
}
static bool refused_with(const ih::ResizeCall& c, const char* starts, const char* holds = "") {
  const std::string m = refusal(c);
  return m.find(starts) == 0 && m.find(holds) != std::string::npos;
}
template <typename F>
static int code_of(F&& f) {
  try { f(); return RTD_OK; } catch (const rtd::Error& e) { return e.code; }
}

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

  CHECK(sizeof(ih::ResizeDesc) == 112 && sizeof(ih::LinEntry) == 12 && sizeof(rtd_bgr_frame) == 24 && ih::RTILE_W == 128 && ih::RTILE_H == 8);
  CHECK(sizeof(ih::TileRef) == 8 && ih::align_up(0, 256) == 0 && ih::align_up(1, 256) == 256 && ih::align_up(256, 256) == 256);
  CHECK(ih::sides_ok(1, 65535) && !ih::sides_ok(0, 1) && !ih::sides_ok(1, 0) && !ih::sides_ok(65536, 1) && !ih::sides_ok(1, 65536) && !ih::sides_ok(-1, 5));

  // ---- the pixel rule (resize_taps.h linear8, area8) against the values tests/test_resize_host.py and tests/test_face_masker_host.py
  // work by hand
  CHECK(rt::area8(10, 11, 12, 14) == 12 && rt::area8(20, 22, 24, 27) == 23 && rt::area8(30, 33, 36, 39) == 35);          // the 2 x 2 block: (47 + 2) >> 2 ...
  CHECK(rt::area8(1, 2, 5, 6) == 4 && rt::area8(3, 4, 7, 8) == 6 && rt::area8(9, 10, 13, 14) == 12 && rt::area8(11, 12, 15, 17) == 14);
  CHECK(rt::area8(0, 0, 0, 0) == 0 && rt::area8(255, 255, 255, 255) == 255 && rt::area8(0, 0, 0, 1) == 0 && rt::area8(0, 0, 1, 1) == 1);
  // the 3 x 1 row (0, 100, 255) (40, 100, 0) (200, 100, 255) to two pixels: column weights (1536, 512) on pixels 0, 1 and (512, 1536) on
  // pixels 1, 2; the one row blends with itself at (2048, 0).  Blue of output 0: H = 40 * 512 = 20480, (2048 * 1280) >> 16 = 40, 42 >> 2 = 10
  CHECK(rt::linear8(0, 40, 0, 40, 1536, 512, 2048, 0) == 10 && rt::linear8(100, 100, 100, 100, 1536, 512, 2048, 0) == 100);
  CHECK(rt::linear8(255, 0, 255, 0, 1536, 512, 2048, 0) == 191 && rt::linear8(40, 200, 40, 200, 512, 1536, 2048, 0) == 160);
  CHECK(rt::linear8(0, 255, 0, 255, 512, 1536, 2048, 0) == 191);
  // fractional weights along a row: 10 * 512 + 20 * 1536 = 35840, (2048 * 2240) >> 16 = 70, 72 >> 2 = 18; 40 * 1536 + 80 * 512 = 102400 -> 50
  CHECK(rt::linear8(10, 20, 10, 20, 512, 1536, 2048, 0) == 18 && rt::linear8(40, 80, 40, 80, 1536, 512, 2048, 0) == 50);
  // and down a column: ((512 * 1280) >> 16) + ((1536 * 2560) >> 16) + 2 = 72 -> 18, and 120 + 80 + 2 = 202 -> 50
  CHECK(rt::linear8(10, 10, 20, 20, 2048, 0, 512, 1536) == 18 && rt::linear8(40, 40, 80, 80, 2048, 0, 1536, 512) == 50);
  // fraction 0 is a copy: ((2048 * (2048 v >> 4)) >> 16) + 2) >> 2 = v
  for (int v = 0; v < 256; ++v) CHECK(rt::linear8(v, 99, 7, 3, 2048, 0, 2048, 0) == v);
  // the bound: the weights of a pair add up to 2049 at most, and then no value leaves a byte
  for (int w0 = 0; w0 <= 2049; ++w0)
    for (int b0 : {0, 1, 512, 1024, 1025, 2048, 2049}) {
      const int v = rt::linear8(255, 255, 255, 255, w0, 2049 - w0, b0, 2049 - b0);
      CHECK(v >= 0 && v <= 255);
    }

  // ---- the tables: the entries every kernel index comes from stay inside the source; the two weights are rounded one by one and add up
  // to 2048 give or take one (a 1 : 65535 up-scale reaches 2049), which keeps every output value at or below 255
  for (int s : {1, 2, 3, 7, 16, 33, 1080, 65535})
    for (int d : {1, 2, 3, 5, 16, 31, 720, 65535})
      for (bool columns : {true, false}) {
        ih::LinEntry* t = (ih::LinEntry*)malloc(sizeof(ih::LinEntry) * (size_t)d);      // exact size
        resize_taps::linear_table(s, d, columns, t);
        for (int k = 0; k < d; ++k)
          CHECK(t[k].i0 >= 0 && t[k].i0 <= t[k].i1 && t[k].i1 < s && t[k].w0 >= 0 && t[k].w1 >= 0 && t[k].w0 + t[k].w1 >= 2047 && t[k].w0 + t[k].w1 <= 2049);
        free(t);
      }
  CHECK(resize_taps::area2(2, 2, 1, 1) && resize_taps::area2(2560, 1440, 1280, 720) && !resize_taps::area2(6, 7, 3, 3) && !resize_taps::area2(3840, 2160, 1280, 720));

  // ---- argument checks of the convert call
  {
    HostFrame a(5, 3, RTD_YUV_NV12, 13, 5), b(4, 8, RTD_YUV_I420, 0, 0);
    rtd_yuv_frame fr[2] = {a.f, b.f};
    uint8_t o0, o1;
    uint8_t* outs[2] = {&o0, &o1};
    auto conv = [](int n, const rtd_yuv_frame* f, uint8_t* const* o) { return ih::ResizeCall::convert(n, f, false, o); };
    CHECK(refusal(conv(2, fr, outs)).empty());
    CHECK(refused_with(conv(0, fr, outs), "1..RTD_INGEST_MAX_FRAMES frames per call") && refused_with(conv(65, fr, outs), "1..RTD_INGEST_MAX_FRAMES frames per call"));
    CHECK(refused_with(conv(2, nullptr, outs), "null argument") && refused_with(conv(2, fr, nullptr), "null argument"));
    auto bad = [&](auto edit) {
      rtd_yuv_frame g[2] = {a.f, b.f};
      uint8_t* po[2] = {&o0, &o1};
      edit(g, po);
      return refusal(conv(2, g, po));
    };
    CHECK(bad([](auto* g, auto** o) { g[1].width = 0; }).find("frame 1 has a bad size (1..65535 per side)") == 0);
    CHECK(bad([](auto* g, auto** o) { g[0].height = 65536; }).find("frame 0 has a bad size (1..65535 per side)") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].y_pitch = 3; }).find("frame 1: y_pitch") == 0);
    CHECK(bad([](auto* g, auto** o) { g[0].c_pitch = 5; }).find("frame 0: c_pitch") == 0);      // NV12, W = 5: a chroma row is 6 bytes
    CHECK(bad([](auto* g, auto** o) { g[1].c_pitch = 1; }).find("frame 1: c_pitch") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].v = nullptr; }).find("frame 1 has a null plane") == 0);      // I420 needs v
    CHECK(bad([](auto* g, auto** o) { g[0].v = nullptr; }).empty());                   // NV12 does not
    CHECK(bad([](auto* g, auto** o) { g[0].y = nullptr; }).find("frame 0 has a null plane") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].u = nullptr; }).find("frame 1 has a null plane") == 0);
    CHECK(bad([](auto* g, auto** o) { o[1] = nullptr; }).find("frame 1 has a null output") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].layout = 3; }).find("frame 1 has an unknown layout") == 0);
    CHECK(bad([](auto* g, auto** o) { g[0].matrix = -1; }).find("frame 0 has an unknown matrix") == 0);
    CHECK(bad([](auto* g, auto** o) { g[1].full_range = 2; }).find("frame 1 has an unknown range") == 0);
    // two outputs of a convert call that share memory pass, as they always did; the same two addresses given to a resize call do not
    uint8_t* const base = (uint8_t*)0x10000000;               // never dereferenced
    uint8_t* same[2] = {base, base + 8};
    int32_t hw[4] = {2, 3, 4, 2};
    CHECK(refusal(conv(2, fr, same)).empty());
    CHECK(refused_with(ih::ResizeCall{2, fr, nullptr, false, hw, same, nullptr}, "frame 1: its output shares memory with the output of frame 0"));
    // nor has a convert call a tile limit: 64 frames of 65535 x 65535 are 2^26 tiles (the limit is the resize calls', below)
    rtd_yuv_frame big[64];
    uint8_t* bout[64];
    for (int i = 0; i < 64; ++i) big[i] = a.f, big[i].width = big[i].height = big[i].y_pitch = 65535, big[i].c_pitch = 65536, bout[i] = base;
    CHECK(refusal(ih::ResizeCall::convert(64, big, true, bout)).empty());
    // a resize call without its output arguments is not a convert call
    CHECK(refused_with(ih::ResizeCall{2, fr, nullptr, false, nullptr, nullptr, outs}, "null argument"));
  }

  // ---- argument checks of the two resize calls
  {
    HostFrame a(10, 6, RTD_YUV_NV12, 3, 1), b(7, 11, RTD_YUV_I420, 0, 2);
    HostBgr p(10, 6, 5), q(3, 3, 0);
    rtd_yuv_frame yf[2] = {a.f, b.f};
    rtd_bgr_frame bf[2] = {p.f, q.f};
    int32_t hw[4] = {3, 5, 6, 4};
    uint8_t* const base = (uint8_t*)0x10000000;               // never dereferenced
    uint8_t* outs[2] = {base, base + 45};                      // 3 x 5 x 3 = 45 bytes: back to back is allowed
    uint8_t* nat[2] = {base + 1000, nullptr};
    const ih::ResizeCall good{2, yf, nullptr, false, hw, outs, nat}, goodb{2, nullptr, bf, true, hw, outs, nullptr};
    CHECK(refusal(good).empty() && refusal(goodb).empty());
    auto with = [&](auto edit) {
      rtd_yuv_frame y2[2] = {a.f, b.f};
      rtd_bgr_frame b2[2] = {p.f, q.f};
      int32_t h2[4] = {3, 5, 6, 4};
      uint8_t* o2[2] = {outs[0], outs[1]};
      uint8_t* n2[2] = {nat[0], nat[1]};
      ih::ResizeCall cy{2, y2, nullptr, false, h2, o2, n2}, cb{2, nullptr, b2, true, h2, o2, nullptr};
      edit(cy, cb, y2, b2, h2, o2, n2);
      return std::make_pair(refusal(cy), refusal(cb));
    };
    auto both_name = [](const std::pair<std::string, std::string>& r, const char* frame) { return r.first.find(frame) == 0 && r.second.find(frame) == 0; };
    CHECK(both_name(with([](auto&, auto&, auto*, auto*, int32_t* h, auto**, auto**) { h[2] = 0; }), "frame 1"));
    CHECK(both_name(with([](auto&, auto&, auto*, auto*, int32_t* h, auto**, auto**) { h[1] = 65536; }), "frame 0"));
    CHECK(both_name(with([](auto&, auto&, auto*, auto*, int32_t*, auto** o, auto**) { o[1] = nullptr; }), "frame 1"));
    CHECK(both_name(with([](auto&, auto&, auto*, auto*, int32_t*, auto** o, auto**) { o[1] = o[0] + 44; }), "frame 1"));      // one shared byte
    CHECK(both_name(with([](auto&, auto&, auto*, auto*, int32_t*, auto** o, auto**) { o[1] = o[0]; }), "frame 1"));
    CHECK(both_name(with([](auto&, auto&, auto* y, auto* b, int32_t*, auto**, auto**) { y[1].width = 0, b[1].width = 65536; }), "frame 1"));
    CHECK(with([](auto&, auto&, auto*, auto* b, int32_t*, auto**, auto**) { b[0].pitch = 29; }).second.find("frame 0") == 0);
    CHECK(with([](auto&, auto&, auto*, auto* b, int32_t*, auto**, auto**) { b[1].data = nullptr; }).second.find("frame 1") == 0);
    CHECK(with([](auto&, auto&, auto* y, auto*, int32_t*, auto**, auto**) { y[1].v = nullptr; }).first.find("frame 1") == 0);
    CHECK(with([](auto&, auto&, auto* y, auto*, int32_t*, auto**, auto**) { y[0].c_pitch = 9; }).first.find("frame 0") == 0);
    // a native output that reaches into an output, and two native outputs on each other
    CHECK(with([](auto&, auto&, auto*, auto*, int32_t*, auto** o, auto** n) { n[0] = o[1] + 71; }).first.find("frame 1") == 0);     // output 1 is 6 x 4 x 3 = 72 bytes
    CHECK(with([](auto&, auto&, auto*, auto*, int32_t*, auto** o, auto** n) { n[0] = o[1] + 72; }).first.empty());
    CHECK(with([](auto&, auto&, auto*, auto*, int32_t*, auto**, auto** n) { n[1] = n[0] + 179; }).first.find("frame 1") == 0);
    CHECK(with([](auto& cy, auto& cb, auto*, auto*, int32_t*, auto**, auto**) { cy.n = 0, cb.n = 65; }) != std::make_pair(std::string(), std::string()));
    CHECK(!with([](auto& cy, auto& cb, auto*, auto*, int32_t*, auto**, auto**) { cy.yuv = nullptr, cb.bgr = nullptr; }).first.empty());
    CHECK(!with([](auto& cy, auto& cb, auto*, auto*, int32_t*, auto**, auto**) { cy.out_hw = nullptr, cb.out = nullptr; }).second.empty());
    // 65535 x 65535 is 512 x 8192 tiles: the fifth such output is past 2^24 (the outputs are 12 GiB apart: no overlap is reported first)
    rtd_bgr_frame five[5] = {p.f, p.f, p.f, p.f, p.f};
    int32_t huge[10];
    uint8_t* far[5];
    for (int i = 0; i < 5; ++i) huge[2 * i] = huge[2 * i + 1] = 65535, far[i] = (uint8_t*)(((uintptr_t)1 << 40) + ((uintptr_t)i << 34));
    CHECK(refusal(ih::ResizeCall{4, nullptr, five, true, huge, far, nullptr}).empty());
    CHECK(refusal(ih::ResizeCall{5, nullptr, five, true, huge, far, nullptr}).find("frame 4") == 0);
  }

  // ---- a convert call: plan, pack and tables over a sweep of sizes, layouts and paddings.  Nothing it does not read is staged: no resize
  // descriptors, no tap tables
  for (int H : {1, 2, 3, 5, 16, 17, 37})
    for (int W : {1, 2, 3, 5, 6, 8, 10, 53, 256, 257})
      for (int layout : {RTD_YUV_NV12, RTD_YUV_NV21, RTD_YUV_I420})
        for (int pad : {0, 1, 13}) {
          HostFrame a(W, H, layout, pad, pad), b(2, 2, RTD_YUV_I420, 0, 3);
          a.f.matrix = RTD_YUV_BT709, a.f.full_range = 1;
          rtd_yuv_frame fr[2] = {a.f, b.f};
          for (bool on_device : {false, true}) {
            uint8_t* const dev_base = (uint8_t*)0x10000000;   // never dereferenced
            uint8_t* outs[2] = {(uint8_t*)0x20000000, (uint8_t*)0x30000001};
            const ih::ResizeCall c = ih::ResizeCall::convert(2, fr, on_device, outs);
            ih::validate_resize(c);
            const ih::ResizePlan p = ih::plan_resize(c);
            const int64_t tiles = (int64_t)((W + ih::TILE_W - 1) / ih::TILE_W) * ((H + ih::TILE_H - 1) / ih::TILE_H) + 1;
            CHECK(p.conv_tiles == tiles && p.fused_tiles == 0 && p.bgr_tiles == 0);
            CHECK(p.fdesc_off == 0 && p.tile_off == ih::align_up(2 * sizeof(ih::FrameDesc), 256));                      // no resize descriptors
            CHECK(p.table_off == ih::align_up(p.tile_off + (size_t)tiles * sizeof(ih::TileRef), 256) && p.tables_end == p.table_off);   // no tables
            CHECK(p.foff[0] == p.tables_end && p.foff[0] % 256 == 0 && p.foff[1] % 256 == 0);
            CHECK(on_device ? p.total == p.tables_end : p.total >= p.foff[1] + 6 && p.foff[1] >= p.foff[0] + (size_t)ih::frame_bytes(H, W));
            uint8_t* stage = (uint8_t*)malloc(p.total);     // exact size
            memset(stage, 0xEE, p.total);
            ih::fill_resize(stage, p, c, dev_base);
            const ih::FrameDesc* d = (const ih::FrameDesc*)stage;
            const ih::TileRef* t = (const ih::TileRef*)(stage + p.tile_off);
            CHECK(d[0].W == W && d[0].H == H && d[0].dst == outs[0] && d[0].ybias == 0 && d[0].cy == 1048576 && d[0].cvr == 1651507 && d[1].ybias == 16);
            CHECK(d[1].dst == outs[1] && d[0].tiles_x == (W + ih::TILE_W - 1) / ih::TILE_W);
            CHECK(t[0].owner == 0 && t[0].tile == 0 && t[tiles - 1].owner == 1 && t[tiles - 1].tile == 0 && t[tiles - 2].tile == (int32_t)tiles - 2);
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
              ih::pack_sources(stage, p, c);
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

  // ---- the resize calls: plan, tables, descriptors, tiles and packing over a sweep of sizes, layouts and paddings
  uint8_t* const dev_base = (uint8_t*)0x40000000;              // never dereferenced
  for (int SH : {1, 2, 6, 9, 17, 36})
    for (int SW : {1, 2, 7, 10, 33, 520})
      for (int pad : {0, 1, 13})
        for (int mode = 0; mode < 3; ++mode) {                 // 0: half size where the source is even (the area rule), 1: two thirds, 2: the same size
          const int OH = mode == 0 ? (SH + 1) / 2 : mode == 1 ? (2 * SH + 2) / 3 : SH, OW = mode == 0 ? (SW + 1) / 2 : mode == 1 ? (2 * SW + 2) / 3 : SW;
          const bool area = mode == 0 && SH % 2 == 0 && SW % 2 == 0;
          for (int layout : {RTD_YUV_NV12, RTD_YUV_NV21, RTD_YUV_I420})
            for (bool on_device : {false, true})
              for (bool native : {false, true}) {
                HostFrame a(SW, SH, layout, pad, pad), b(4, 4, RTD_YUV_I420, 0, 3);
                rtd_yuv_frame fr[2] = {a.f, b.f};
                int32_t hw[4] = {OH, OW, 2, 2};
                uint8_t* outs[2] = {(uint8_t*)0x20000000, (uint8_t*)0x30000001};
                uint8_t* nat[2] = {native ? (uint8_t*)0x50000000 : nullptr, nullptr};
                const ih::ResizeCall c{2, fr, nullptr, on_device, hw, outs, nat};
                ih::validate_resize(c);
                const ih::ResizePlan p = ih::plan_resize(c);
                const int64_t rt = ih::rtiles_of(OH, OW);
                CHECK(p.area[0] == (area ? 1 : 0) && p.area[1] == 1);
                CHECK(p.conv_tiles == (native ? ih::tiles_of(a.f) : 0) && p.fused_tiles == (native ? 1 : rt + 1) && p.bgr_tiles == (native ? rt : 0));
                CHECK(p.fdesc_off % 256 == 0 && p.tile_off % 256 == 0 && p.table_off % 256 == 0 && p.tables_end % 256 == 0);
                CHECK(p.table_off >= p.tile_off + sizeof(ih::TileRef) * (size_t)(p.conv_tiles + p.fused_tiles + p.bgr_tiles));
                CHECK(p.tables_end >= p.toff[0] + (area ? 0 : sizeof(ih::LinEntry) * ((size_t)OW + OH)) && p.toff[0] % 4 == 0);
                CHECK(on_device ? p.total == p.tables_end : p.total >= p.foff[1] + 24 && p.foff[1] >= p.foff[0] + (size_t)ih::frame_bytes(SH, SW));
                uint8_t* stage = (uint8_t*)malloc(p.total);   // exact size
                memset(stage, 0xEE, p.total);
                ih::fill_resize(stage, p, c, dev_base);
                if (!on_device) ih::pack_sources(stage, p, c);
                const ih::ResizeDesc* d = (const ih::ResizeDesc*)stage;
                const ih::TileRef* t = (const ih::TileRef*)(stage + p.tile_off);
                CHECK(d[0].OW == OW && d[0].OH == OH && d[0].out == outs[0] && d[0].src.W == SW && d[0].src.H == SH && !!(d[0].rflags & ih::R_AREA) == area);
                CHECK(!(d[1].rflags & ih::R_DST_WIDE) && !!(d[0].rflags & ih::R_DST_WIDE) == (OW % 4 == 0));
                CHECK((d[0].tab == nullptr) == area && (area || (const uint8_t*)d[0].tab == dev_base + p.toff[0]));
                if (!area) {
                  const ih::LinEntry* tab = (const ih::LinEntry*)(stage + p.toff[0]);
                  for (int k = 0; k < OW; ++k) CHECK(tab[k].i1 < SW && tab[k].i0 >= 0);
                  for (int k = 0; k < OH; ++k) CHECK(tab[OW + k].i1 < SH && tab[OW + k].i0 >= 0);
                }
                if (native) {                                  // frame 0 goes through the convert kernel, then the BGR kernel reads what it wrote
                  const ih::FrameDesc* cd = (const ih::FrameDesc*)(stage + p.fdesc_off);
                  CHECK(cd[0].dst == nat[0] && cd[0].W == SW && cd[0].H == SH && cd[1].dst == nullptr);
                  CHECK(d[0].src.y == nat[0] && d[0].src.y_pitch == 3 * SW);
                  CHECK(t[0].owner == 0 && t[p.conv_tiles - 1].tile == (int32_t)p.conv_tiles - 1 && t[p.conv_tiles].owner == 1);
                  CHECK(t[p.conv_tiles + 1].owner == 0 && t[p.conv_tiles + rt].tile == (int32_t)rt - 1);
                } else {
                  CHECK(t[0].owner == 0 && t[rt - 1].tile == (int32_t)rt - 1 && t[rt].owner == 1 && t[rt].tile == 0);
                  if (on_device) CHECK(d[0].src.y == a.f.y && d[0].src.y_pitch == SW + pad);
                  else CHECK(d[0].src.y == dev_base + p.foff[0] && d[0].src.y_pitch == SW);
                }
                if (!on_device) {
                  const uint8_t* q = stage + p.foff[0];
                  for (int r = 0; r < SH; ++r) CHECK(memcmp(q + (size_t)r * SW, a.y + (size_t)r * a.f.y_pitch, (size_t)SW) == 0);
                  if (p.foff[1] > p.foff[0] + (size_t)ih::frame_bytes(SH, SW)) CHECK(stage[p.foff[0] + (size_t)ih::frame_bytes(SH, SW)] == 0xEE);
                }
                free(stage);
              }
          // the BGR call
          for (bool on_device : {false, true}) {
            HostBgr a(SW, SH, pad), b(2, 2, 1);
            rtd_bgr_frame fr[2] = {a.f, b.f};
            int32_t hw[4] = {OH, OW, 1, 1};
            uint8_t* outs[2] = {(uint8_t*)0x20000000, (uint8_t*)0x30000002};
            const ih::ResizeCall c{2, nullptr, fr, on_device, hw, outs, nullptr};
            ih::validate_resize(c);
            const ih::ResizePlan p = ih::plan_resize(c);
            CHECK(p.conv_tiles == 0 && p.fused_tiles == 0 && p.bgr_tiles == ih::rtiles_of(OH, OW) + 1 && p.fdesc_off == p.tile_off);
            uint8_t* stage = (uint8_t*)malloc(p.total);
            memset(stage, 0xEE, p.total);
            ih::fill_resize(stage, p, c, dev_base);
            if (!on_device) ih::pack_sources(stage, p, c);
            const ih::ResizeDesc* d = (const ih::ResizeDesc*)stage;
            CHECK(d[0].src.W == SW && d[0].src.H == SH && d[1].rflags == (ih::R_AREA | (on_device ? ((uintptr_t)b.f.data % 4 == 0 && b.f.pitch % 4 == 0 ? ih::R_SRC_WIDE : 0) : 0)));
            if (on_device) {
              CHECK(d[0].src.y == a.f.data && d[0].src.y_pitch == 3 * SW + pad);
            } else {
              CHECK(d[0].src.y == dev_base + p.foff[0] && d[0].src.y_pitch == 3 * SW && p.total >= p.foff[1] + 12);
              for (int r = 0; r < SH; ++r) CHECK(memcmp(stage + p.foff[0] + (size_t)r * 3 * SW, a.p + (size_t)r * a.f.pitch, 3 * (size_t)SW) == 0);
              if (p.foff[1] > p.foff[0] + 3 * (size_t)SH * SW) CHECK(stage[p.foff[0] + 3 * (size_t)SH * SW] == 0xEE);
            }
            free(stage);
          }
        }
  // ---- frames of the same sizes share one pair of tables; another size, and an area frame between them, do not disturb that
  {
    HostBgr a(9, 9, 0), b(4, 4, 0), c(9, 9, 3), d(9, 7, 0);
    rtd_bgr_frame fr[4] = {a.f, b.f, c.f, d.f};
    int32_t hw[8] = {3, 3, 2, 2, 3, 3, 3, 3};
    uint8_t* outs[4] = {(uint8_t*)0x20000000, (uint8_t*)0x20001000, (uint8_t*)0x20002000, (uint8_t*)0x20003000};
    const ih::ResizeCall call{4, nullptr, fr, true, hw, outs, nullptr};
    const ih::ResizePlan p = ih::plan_resize(call);
    CHECK(!p.shared[0] && p.area[1] && p.shared[2] && p.toff[2] == p.toff[0] && !p.shared[3] && p.toff[3] >= p.toff[0] + 6 * sizeof(ih::LinEntry));
    uint8_t* stage = (uint8_t*)malloc(p.total);
    memset(stage, 0xEE, p.total);
    ih::fill_resize(stage, p, call, dev_base);
    const ih::ResizeDesc* rd = (const ih::ResizeDesc*)stage;
    CHECK(rd[0].tab == rd[2].tab && rd[1].tab == nullptr && rd[3].tab != rd[0].tab && rd[3].tab != nullptr);
    const ih::LinEntry* t = (const ih::LinEntry*)(stage + p.toff[0]);
    CHECK(t[0].i0 == 1 && t[0].i1 == 1 + 1 && t[1].i0 == 4 && t[2].i0 == 7 && t[0].w0 == 2048 && t[0].w1 == 0);     // 9 -> 3: the middle of each three
    free(stage);
  }
  printf("ingest host check ok\n");
  return 0;
}
