// Stand-alone check of the pure host parts of the ingest's resize stage (csrc/ingest_host.h, csrc/resize_taps.h): the argument checks
// of both calls (limits, null pointers, outputs that share memory), the staging layout, the tap tables, the descriptors and tile lists
// of the three launches, and the packing of host frames with padded pitches (planes and BGR frames are exact-size heap blocks: a read
// or write past one is a sanitizer report).
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/resize_host_check.cpp -o resize_host_check && ./resize_host_check
#include <stdio.h>
#include <stdlib.h>

#include "../telescope_cam_detection_amd/csrc/ingest_host.h"

namespace ih = ingest_host;

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

int main() {
  CHECK(sizeof(ih::ResizeDesc) == 112 && sizeof(ih::LinEntry) == 12 && sizeof(rtd_bgr_frame) == 24 && ih::RTILE_W == 128 && ih::RTILE_H == 8);

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

  // ---- argument checks of both calls
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

  // ---- plan, tables, descriptors, tiles and packing over a sweep of sizes, layouts and paddings
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
                  CHECK(t[0].frame == 0 && t[p.conv_tiles - 1].tile == (int32_t)p.conv_tiles - 1 && t[p.conv_tiles].frame == 1);
                  CHECK(t[p.conv_tiles + 1].frame == 0 && t[p.conv_tiles + rt].tile == (int32_t)rt - 1);
                } else {
                  CHECK(t[0].frame == 0 && t[rt - 1].tile == (int32_t)rt - 1 && t[rt].frame == 1 && t[rt].tile == 0);
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
  printf("resize host check ok\n");
  return 0;
}
