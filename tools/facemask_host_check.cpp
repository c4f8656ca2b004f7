// Stand-alone check of the pure host parts of the face masks (csrc/facemask_host.h, csrc/gauss_taps.h): the limits, the padded
// rectangle, the layers, the tile lists, the blur taps, the resize tables and the staging layout, every table read back through exact-size
// heap copies (a read or write past one is a sanitizer report).
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/facemask_host_check.cpp -o facemask_host_check && ./facemask_host_check
#include <stdio.h>
#include <stdlib.h>

#include "../telescope_cam_detection_amd/csrc/facemask_host.h"

namespace fh = facemask_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

static rtd_face_rect face(int frame, int x, int y, int w, int h, int style, int k) { return {frame, x, y, w, h, style, k, 0}; }

static std::string refusal(int n, const int32_t* hw, int nf, const rtd_face_rect* f) {
  try { fh::validate(n, hw, nf, f); } catch (const rtd::Error& e) { CHECK(e.code == RTD_E_INVALID); return e.what(); }
  return "";
}

int main() {
  CHECK(sizeof(fh::FaceDesc) == 80 && sizeof(fh::TileRef) == 8 && sizeof(fh::LinEntry) == 12 && sizeof(rtd_face_rect) == 32);

  // ---- taps: every odd k, >= 0, symmetric, sum 256; the fixed tables
  for (int k = 1; k <= fh::MAX_K; k += 2) {
    uint16_t* c = (uint16_t*)malloc(sizeof(uint16_t) * k);       // exact size
    gauss8::tap_rule(k, c);
    int sum = 0;
    for (int i = 0; i < k; ++i) {
      sum += c[i];
      CHECK(c[i] <= 256 && c[i] == c[k - 1 - i]);
    }
    CHECK(sum == 256);
    free(c);
  }
  uint16_t c7[7];
  gauss8::tap_rule(7, c7);
  CHECK(c7[0] == 8 && c7[3] == 72);

  // ---- limits
  const int32_t hw2[4] = {48, 64, 5, 7};
  rtd_face_rect two[2] = {face(0, 10, 10, 20, 20, RTD_FACE_BLUR, 25), face(1, 0, 0, 3, 3, RTD_FACE_PIXELATE, 2)};
  CHECK(refusal(2, hw2, 2, two).empty());
  CHECK(!refusal(0, hw2, 2, two).empty() && !refusal(65, hw2, 0, two).empty() && !refusal(2, nullptr, 2, two).empty());
  CHECK(!refusal(2, hw2, 2, nullptr).empty() && !refusal(2, hw2, 1025, two).empty() && !refusal(2, hw2, -1, two).empty());
  CHECK(refusal(2, hw2, 0, nullptr).empty());
  auto bad = [&](auto edit) {
    rtd_face_rect g[2] = {two[0], two[1]};
    int32_t hw[4] = {48, 64, 5, 7};
    edit(g, hw);
    return refusal(2, hw, 2, g);
  };
  CHECK(bad([](auto* g, auto* hw) { g[1].frame = 2; }).find("face 1") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[0].frame = -1; }).find("face 0") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[1].style = 3; }).find("face 1") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[0].k_or_blocks = 24; }).find("face 0") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[0].k_or_blocks = 101; }).find("face 0") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[0].k_or_blocks = -1; }).find("face 0") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[1].k_or_blocks = 0; }).find("face 1") == 0);
  CHECK(bad([](auto* g, auto* hw) { g[0].style = RTD_FACE_BLACK_BOX, g[0].k_or_blocks = -7; }).empty());     // ignored there
  CHECK(bad([](auto* g, auto* hw) { hw[2] = 0; }).find("frame 1") == 0);
  CHECK(bad([](auto* g, auto* hw) { hw[1] = 65536; }).find("frame 0") == 0);
  CHECK(bad([](auto* g, auto* hw) { hw[0] = 65535, hw[1] = 65535; }).find("frame 0") == 0);                    // 2 GiB or more
  {
    uint8_t a;
    uint8_t* fr[2] = {&a, nullptr};
    int code = RTD_OK;
    try { fh::validate_frames(2, fr); } catch (const rtd::Error& e) { code = e.code; CHECK(std::string(e.what()).find("frame 1") == 0); }
    CHECK(code == RTD_E_INVALID);
  }

  // ---- padded rectangles at the four edges, extreme coordinates, the black box's extra row and column
  {
    const fh::Rect r = fh::padded(face(0, 10, 12, 20, 30, 0, 3), 64, 48);
    CHECK(r.x1 == 6 && r.y1 == 8 && r.x2 == 34 && r.y2 == 46);
    const fh::Rect l = fh::padded(face(0, 2, 1, 20, 30, 0, 3), 64, 48), q = fh::padded(face(0, 50, 30, 20, 30, 0, 3), 64, 48);
    CHECK(l.x1 == 0 && l.y1 == 0 && q.x2 == 64 && q.y2 == 48);
    CHECK(fh::padded(face(0, -100, 0, 20, 20, 0, 3), 64, 48).empty() && fh::padded(face(0, 70, 0, 20, 20, 0, 3), 64, 48).empty());
    CHECK(fh::padded(face(0, 0, 0, 0, 5, 0, 3), 64, 48).empty() && fh::padded(face(0, 5, 5, -20, 5, 0, 3), 64, 48).empty());
    CHECK(fh::padded(face(0, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, 0, 3), 64, 48).empty());
    CHECK(!fh::padded(face(0, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, 0, 3), 64, 48).empty());
    const fh::Rect b = fh::touched(face(0, 10, 12, 20, 30, RTD_FACE_BLACK_BOX, 0), 64, 48), e = fh::touched(face(0, 50, 30, 20, 30, RTD_FACE_BLACK_BOX, 0), 64, 48);
    CHECK(b.x2 == 35 && b.y2 == 47 && e.x2 == 64 && e.y2 == 48);
  }

  // ---- resize tables over a sweep of sizes and blocks: indices inside the source, weights that sum to 2048
  for (int rw : {1, 2, 3, 5, 6, 17, 64, 65, 168})
    for (int blocks : {1, 2, 3, 10, 500}) {
      const int sw = std::max(1, rw / blocks);
      fh::LinEntry* t = (fh::LinEntry*)malloc(sizeof(fh::LinEntry) * sw);
      int32_t* m = (int32_t*)malloc(sizeof(int32_t) * rw);
      for (bool columns : {true, false}) {
        fh::linear_table(rw, sw, columns, t);
        for (int d = 0; d < sw; ++d) CHECK(t[d].i0 >= 0 && t[d].i0 <= t[d].i1 && t[d].i1 < rw && t[d].w0 + t[d].w1 == 2048 && t[d].w0 >= 0 && t[d].w1 >= 0);
      }
      fh::nearest_table(sw, rw, m);
      for (int x = 0; x < rw; ++x) CHECK(m[x] >= 0 && m[x] < sw && (x == 0 || m[x] >= m[x - 1]));
      CHECK(m[0] == 0 && m[rw - 1] == sw - 1);
      if (blocks == 1)
        for (int x = 0; x < rw; ++x) CHECK(m[x] == x && t[x].i0 == x && t[x].w0 == 2048);
      free(t), free(m);
    }
  CHECK(fh::area2(4, 4, 2, 2) && fh::area2(168, 10, 84, 5) && !fh::area2(5, 4, 2, 2) && !fh::area2(6, 3, 2, 1) && !fh::area2(4, 4, 4, 4) && fh::area2(2, 2, 1, 1));

  // ---- plans: layers, tile lists, scratch, staging layout
  {
    // A and B overlap, C is disjoint: 2 layers; D on another frame never waits
    const int32_t hw[4] = {100, 200, 37, 223};
    rtd_face_rect f[5] = {face(0, 10, 10, 30, 30, RTD_FACE_BLUR, 25), face(0, 30, 30, 30, 30, RTD_FACE_PIXELATE, 10), face(0, 150, 10, 20, 20, RTD_FACE_BLACK_BOX, 0),
                          face(1, 10, 10, 30, 30, RTD_FACE_BLUR, 99), face(0, 500, 10, 20, 20, RTD_FACE_BLUR, 3)};
    for (bool on_device : {true, false}) {
      const fh::Plan p = fh::plan(2, hw, 5, f, on_device);
      CHECK(p.layers == 2 && p.layer_of[0] == 0 && p.layer_of[1] == 1 && p.layer_of[2] == 0 && p.layer_of[3] == 0 && p.layer_of[4] == -1);
      CHECK(p.descs.size() == 4 && p.frame_used[0] && p.frame_used[1]);
      CHECK(p.launches.size() == 5);                           // layer 0: blur rows, blur columns, box; layer 1: small, nearest
      CHECK(p.launches[0].kind == fh::K_BLUR_ROWS && p.launches[1].kind == fh::K_BLUR_COLS && p.launches[2].kind == fh::K_BOX);
      CHECK(p.launches[3].layer == 1 && p.launches[3].kind == fh::K_PIX_SMALL && p.launches[4].kind == fh::K_PIX_NEAREST);
      size_t tiles = 0;
      for (const fh::Launch& l : p.launches) {
        CHECK(l.tile0 == tiles && l.ntiles > 0);
        tiles += l.ntiles;
        for (size_t t = l.tile0; t < l.tile0 + l.ntiles; ++t) {
          const fh::FaceDesc& d = p.descs[(size_t)p.tiles[t].owner];
          const int64_t cnt = l.kind == fh::K_PIX_SMALL ? ((int64_t)d.sh * d.sw * 3 + fh::SMALL_TILE - 1) / fh::SMALL_TILE : fh::region_tiles(d);
          CHECK(p.tiles[t].tile >= 0 && p.tiles[t].tile < cnt);
        }
      }
      CHECK(tiles == p.tiles.size());
      // regions inside their frames; scratch of a layer's faces disjoint and inside scratch_bytes; tables inside the table block
      for (const fh::FaceDesc& d : p.descs) {
        CHECK(d.x1 >= 0 && d.y1 >= 0 && d.rw >= 1 && d.rh >= 1 && d.x1 + d.rw <= d.W && d.y1 + d.rh <= d.H);
        const size_t bytes = d.style == RTD_FACE_BLUR ? (size_t)d.rh * d.rw * 6 : d.style == RTD_FACE_PIXELATE ? (size_t)d.sh * d.sw * 3 : 0;
        CHECK((size_t)d.scratch_off + bytes <= p.scratch_bytes);
        const size_t tb = d.style == RTD_FACE_BLUR ? 2 * (size_t)(2 * d.radius + 1)
                          : d.style == RTD_FACE_PIXELATE ? sizeof(fh::LinEntry) * ((size_t)d.sw + d.sh) + 4 * ((size_t)d.rw + d.rh) : 0;
        CHECK((size_t)d.table_off + tb <= p.tables.size() && d.table_off % 8 == 0);
      }
      CHECK(p.tile_off % 256 == 0 && p.table_off % 256 == 0 && p.tables_end % 256 == 0 && p.tile_off >= sizeof(fh::FaceDesc) * 4);
      CHECK(p.table_off >= p.tile_off + sizeof(fh::TileRef) * p.tiles.size() && p.tables_end >= p.table_off + p.tables.size());
      CHECK(on_device ? p.total == p.tables_end : p.total >= p.foff[1] + 37 * 223 * 3 && p.foff[1] >= p.foff[0] + 100 * 200 * 3 && p.foff[0] == p.tables_end);
      uint8_t* stage = (uint8_t*)malloc(p.tables_end);         // exact size
      uint8_t* at[2] = {(uint8_t*)0x10000000, (uint8_t*)0x20000001};   // never dereferenced
      fh::fill_tables(stage, p, at);
      const fh::FaceDesc* d = (const fh::FaceDesc*)stage;
      CHECK(d[0].frame == at[0] && d[3].frame == at[1] && d[3].radius == 49 && d[0].x1 == 4 && d[0].rw == 42);
      const uint16_t* taps = (const uint16_t*)(stage + p.table_off + d[3].table_off);
      int sum = 0;
      for (int i = 0; i < 99; ++i) sum += taps[i];
      CHECK(sum == 256);
      free(stage);
    }
    // a chain of three: 3 layers; the same three on three frames: 1 layer
    rtd_face_rect chain[3] = {face(0, 10, 10, 30, 30, RTD_FACE_BLUR, 25), face(0, 40, 10, 30, 30, RTD_FACE_BLUR, 25), face(0, 70, 10, 30, 30, RTD_FACE_BLUR, 25)};
    const int32_t hw3[6] = {100, 200, 100, 200, 100, 200};
    CHECK(fh::plan(1, hw3, 3, chain, true).layers == 3);
    for (int i = 0; i < 3; ++i) chain[i].frame = i;
    CHECK(fh::plan(3, hw3, 3, chain, true).layers == 1);
    // no face at all, and only skipped ones: nothing to launch, no frame staged
    const fh::Plan none = fh::plan(2, hw, 0, nullptr, false), skipped = fh::plan(2, hw, 1, f + 4, false);
    CHECK(none.launches.empty() && skipped.launches.empty() && skipped.layers == 0 && skipped.total == skipped.tables_end);
    // 1024 faces of 1 x 1 on one frame: one layer, one tile each
    std::vector<rtd_face_rect> many;
    for (int i = 0; i < 1024; ++i) many.push_back(face(0, (i % 64) * 3, (i / 64) * 2, 1, 1, i % 3, i % 3 == 0 ? 3 : 1));
    const fh::Plan m = fh::plan(1, hw, 1024, many.data(), true);
    CHECK(m.layers == 1 && m.descs.size() == 1024 && m.kind_tiles[fh::K_BLUR_ROWS] == 342 && m.kind_tiles[fh::K_BOX] == 341);
    // a whole 4k frame as one face of every style
    const int32_t big[2] = {2160, 3840};
    rtd_face_rect whole[3] = {face(0, 0, 0, 3840, 2160, RTD_FACE_BLUR, 99), face(0, 0, 0, 3840, 2160, RTD_FACE_PIXELATE, 1), face(0, 0, 0, 3840, 2160, RTD_FACE_BLACK_BOX, 0)};
    const fh::Plan w = fh::plan(1, big, 3, whole, false);
    CHECK(w.layers == 3 && w.kind_tiles[fh::K_BLUR_COLS] == 60 * 135 && w.scratch_bytes >= (size_t)2160 * 3840 * 6);
  }
  printf("facemask host check ok\n");
  return 0;
}
