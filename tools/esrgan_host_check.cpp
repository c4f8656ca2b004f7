// Stand-alone check of the pure host parts of the ESRGAN upscaler (csrc/esrgan_host.h): config checks, the output layout, the tile
// rectangles, the conv table against a packed blob (present, shaped, in range) and the filter re-ordering.  The blob's parser itself
// (truncated, corrupted and crafted tables) is tools/weight_blob_host_check.cpp's.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/esrgan_host_check.cpp -o esrgan_host_check && ./esrgan_host_check
#include <stdio.h>
#include <stdlib.h>

#include "../telescope_cam_detection_amd/csrc/esrgan_host.h"

namespace eh = esrgan_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

template <typename F>
static int code_of(F&& f) {
  try { f(); return RTD_OK; } catch (const rtd::Error& e) { return e.code; }
}

// weights.pack_blob of {name: fp32 tensor}
static std::vector<char> pack(const std::vector<std::pair<std::string, std::vector<uint32_t>>>& ts) {
  std::vector<char> head{'R', 'T', 'D', 'W'};
  auto put = [&](const void* p, size_t n) { head.insert(head.end(), (const char*)p, (const char*)p + n); };
  const uint32_t ver = 1, count = (uint32_t)ts.size();
  put(&ver, 4); put(&count, 4);
  size_t table = 0;
  for (auto& t : ts) table += 2 + t.first.size() + 4 + 4 * t.second.size() + 16;
  uint64_t off = (head.size() + table + 63) / 64 * 64;
  std::vector<std::pair<uint64_t, uint64_t>> ext;
  for (auto& t : ts) {
    uint64_t n = 4;
    for (auto d : t.second) n *= d;
    ext.push_back({off, n});
    off = (off + n + 63) / 64 * 64;
  }
  for (size_t i = 0; i < ts.size(); ++i) {
    const uint16_t nl = (uint16_t)ts[i].first.size();
    put(&nl, 2); put(ts[i].first.data(), nl);
    const uint32_t nd = (uint32_t)ts[i].second.size();
    put(&nd, 4);
    for (auto d : ts[i].second) put(&d, 4);
    put(&ext[i].first, 8); put(&ext[i].second, 8);
  }
  std::vector<char> blob(off, 0);
  memcpy(blob.data(), head.data(), head.size());
  for (size_t i = 0; i < ts.size(); ++i) {
    float* f = (float*)(blob.data() + ext[i].first);
    for (uint64_t k = 0; k < ext[i].second / 4; ++k) f[k] = 0.001f * (float)((k * 7 + i) % 97) - 0.04f;
  }
  return blob;
}

int main() {
  // ---- config
  rtd_esrgan_config c{(int32_t)sizeof(rtd_esrgan_config), 0, RTD_PREC_F16X3, 64, 32, 23, 512, 10};
  CHECK(code_of([&] { eh::check_config(&c); }) == RTD_OK);
  auto bad = [&](auto edit) { rtd_esrgan_config d = c; edit(d); return code_of([&] { eh::check_config(&d); }); };
  CHECK(bad([](auto& d) { d.precision = RTD_PREC_BF16; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.tile = 8; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.tile = 513; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.tile = 0; }) == RTD_OK);
  CHECK(bad([](auto& d) { d.tile_pad = 33; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.num_block = 0; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.num_block = 33; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.num_feat = 32; }) == RTD_E_INVALID);
  CHECK(bad([](auto& d) { d.struct_size = 4; }) == RTD_E_INVALID);
  CHECK(code_of([&] { eh::check_config(nullptr); }) == RTD_E_INVALID);

  // ---- layout
  {
    const int32_t r[12] = {0, 0, 8, 8, 5, 7, 45, 40, 0, 0, 4096, 4096};
    int64_t off[4];
    eh::layout(3, r, off);
    CHECK(off[0] == 0 && off[1] == 3072 && off[2] == 3072 + (int64_t)(160 * 132 * 3 + 255) / 256 * 256);
    CHECK(off[3] - off[2] == 16384ll * 16384 * 3);
    eh::layout(0, nullptr, off);
    CHECK(off[0] == 0);
    const int32_t b1[4] = {0, 0, 7, 8}, b2[4] = {-1, 0, 20, 20}, b3[4] = {0, 0, 4097, 8}, b4[4] = {2147483647, 0, -2147483647 - 1, 9};
    for (const int32_t* b : {b1, b2, b3, b4}) CHECK(code_of([&] { eh::layout(1, b, off); }) == RTD_E_INVALID);
    CHECK(code_of([&] { eh::layout(-1, r, off); }) == RTD_E_INVALID);
    CHECK(code_of([&] { eh::layout(1, nullptr, off); }) == RTD_E_INVALID);
  }

  // ---- tiles: cores partition the crop, inputs stay inside it and hold their core, every (H, W, tile, pad) of a sweep
  for (int H : {8, 16, 33, 40, 97})
    for (int W : {8, 17, 33, 64})
      for (int tile : {0, 16, 17, 32, 512})
        for (int pad : {0, 4, 10, 32}) {
          const auto ts = eh::tile_rects(H, W, tile, pad);
          std::vector<int> cover((size_t)H * W, 0);
          for (const auto& t : ts) {
            CHECK(0 <= t.ix0 && t.ix0 <= t.cx0 && t.cx0 < t.cx1 && t.cx1 <= t.ix1 && t.ix1 <= W);
            CHECK(0 <= t.iy0 && t.iy0 <= t.cy0 && t.cy0 < t.cy1 && t.cy1 <= t.iy1 && t.iy1 <= H);
            CHECK(t.cx0 - t.ix0 <= pad && t.ix1 - t.cx1 <= pad && t.cy0 - t.iy0 <= pad && t.iy1 - t.cy1 <= pad);
            for (int y = t.cy0; y < t.cy1; ++y)
              for (int x = t.cx0; x < t.cx1; ++x) cover[(size_t)y * W + x]++;
          }
          for (int v : cover) CHECK(v == 1);
          if (tile == 0 || (tile >= H && tile >= W)) CHECK(ts.size() == 1 && ts[0].ix1 == W && ts[0].iy1 == H);
        }
  CHECK(eh::tile_rects(40, 33, 16, 4).size() == 9);

  // ---- blob: a one-block network
  std::vector<std::pair<std::string, std::vector<uint32_t>>> ts;
  const auto table = eh::conv_table(1);
  CHECK(table.size() == 21 && eh::conv_table(23).size() == 351);
  for (const auto& d : table) {
    ts.push_back({d.name + ".weight", {(uint32_t)d.cout, (uint32_t)d.cin, 3, 3}});
    ts.push_back({d.name + ".bias", {(uint32_t)d.cout}});
  }
  const std::vector<char> blob = pack(ts);
  {
    std::map<std::string, eh::HostTensor> host;
    eh::parse_blob(blob.data(), blob.size(), host);
    CHECK(host.size() == 42);
    for (const auto& d : table) eh::check_conv_tensors(host, d, true);
    // the re-ordering: OIHW -> [o][tap][channel], padded
    const auto& d = table[1];   // 64 -> 32
    const auto rows = eh::filter_rows(host.at(d.name + ".weight"), d.cout, d.cin, d.cin, 128, 9 * 64, 0.2f);
    CHECK(rows.size() == 128u * 576);
    const float* w = host.at(d.name + ".weight").data;
    CHECK(rows[(size_t)5 * 576 + 7 * 64 + 11] == w[((size_t)5 * 64 + 11) * 9 + 7] * 0.2f);
    CHECK(rows[(size_t)32 * 576] == 0.f);
    const auto first = eh::filter_rows(host.at("conv_first.weight"), 64, 3, 32, 128, 320, 1.f);
    CHECK(first[(size_t)2 * 320 + 8 * 32 + 2] == host.at("conv_first.weight").data[((size_t)2 * 3 + 2) * 9 + 8] && first[(size_t)2 * 320 + 8 * 32 + 3] == 0.f);
    // a missing tensor, a wrong shape, a NaN, a value beyond fp16
    auto h2 = host;
    h2.erase("conv_hr.bias");
    CHECK(code_of([&] { eh::check_conv_tensors(h2, table[19], true); }) == RTD_E_WEIGHTS);
    h2 = host;
    h2["conv_hr.weight"].shape = {64, 64, 3, 1};
    CHECK(code_of([&] { eh::check_conv_tensors(h2, table[19], true); }) == RTD_E_WEIGHTS);
  }
  {
    std::vector<char> b2 = blob;
    std::map<std::string, eh::HostTensor> host;
    eh::parse_blob(b2.data(), b2.size(), host);
    float* w = (float*)host.at("conv_body.weight").data;
    w[100] = 70000.f;
    CHECK(code_of([&] { eh::check_conv_tensors(host, table[16], true); }) == RTD_E_WEIGHTS);
    CHECK(code_of([&] { eh::check_conv_tensors(host, table[16], false); }) == RTD_OK);
    w[100] = NAN;
    CHECK(code_of([&] { eh::check_conv_tensors(host, table[16], false); }) == RTD_E_WEIGHTS);
  }
  printf("esrgan host check ok\n");
  return 0;
}
