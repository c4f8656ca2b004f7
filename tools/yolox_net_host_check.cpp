// Stand-alone check of the pure host parts of the YOLOX network (csrc/yolox_net_host.h): the variants served and refused, the conv table
// and its channel counts, the checks of a call (float input and uint8 frames), the front end's index and weight rule, the per-level anchor offsets, the blob's table (parsing, missing and mis-shaped tensors, NaN and range checks)
// and the SPP kernel's tiling.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/yolox_net_host_check.cpp -o yolox_net_host_check && ./yolox_net_host_check
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <set>

#include "../telescope_cam_detection_amd/csrc/yolox_net_host.h"

namespace yh = yolox_net_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

template <typename F>
static std::string refusal(F&& f, int code = RTD_E_INVALID) {
  try { f(); } catch (const rtd::Error& e) { CHECK(e.code == code); return e.what(); }
  return "";
}

static rtd_yolox_net_config config(int precision, int classes, int base, int depth, int batch) {
  return {(int32_t)sizeof(rtd_yolox_net_config), 0, precision, classes, base, depth, batch, 0};
}

// a blob as weights.pack_blob writes it: "RTDW", version 1, count; per tensor name, dims, offset, bytes; data on 64-byte boundaries
struct Blob {
  std::vector<std::string> names;
  std::vector<std::vector<uint32_t>> shapes;
  std::vector<std::vector<float>> data;
  void add(const std::string& n, std::vector<uint32_t> shape, float fill) {
    size_t numel = 1;
    for (uint32_t d : shape) numel *= d;
    names.push_back(n), shapes.push_back(shape), data.push_back(std::vector<float>(numel, fill));
  }
  std::vector<float> pack() const {       // (a float vector: 4-byte aligned, as parse_blob asks)
    std::vector<char> head;
    auto put = [&](const void* p, size_t n) { head.insert(head.end(), (const char*)p, (const char*)p + n); };
    const uint32_t ver = 1, count = (uint32_t)names.size();
    put("RTDW", 4), put(&ver, 4), put(&count, 4);
    size_t table = head.size();
    for (size_t i = 0; i < names.size(); ++i) table += 2 + names[i].size() + 4 + 4 * shapes[i].size() + 16;
    uint64_t off = (table + 63) / 64 * 64;
    std::vector<uint64_t> offs;
    for (size_t i = 0; i < names.size(); ++i) {
      offs.push_back(off);
      off = (off + data[i].size() * 4 + 63) / 64 * 64;
    }
    for (size_t i = 0; i < names.size(); ++i) {
      const uint16_t nl = (uint16_t)names[i].size();
      const uint32_t nd = (uint32_t)shapes[i].size();
      const uint64_t nb = data[i].size() * 4;
      put(&nl, 2), put(names[i].data(), nl), put(&nd, 4), put(shapes[i].data(), 4 * nd), put(&offs[i], 8), put(&nb, 8);
    }
    std::vector<float> out(off / 4, 0.f);
    memcpy(out.data(), head.data(), head.size());
    for (size_t i = 0; i < names.size(); ++i) memcpy((char*)out.data() + offs[i], data[i].data(), data[i].size() * 4);
    return out;
  }
};

static Blob blob_of(const std::vector<yh::ConvDesc>& table) {
  Blob b;
  for (const yh::ConvDesc& d : table) {
    b.add(d.name + ".weight", {(uint32_t)d.cout, (uint32_t)d.k, (uint32_t)d.k, (uint32_t)d.cin}, 0.01f);
    b.add(d.name + ".bias", {(uint32_t)d.cout}, 0.1f);
  }
  return b;
}

int main() {
  CHECK(sizeof(rtd_yolox_net_config) == 32);

  // ---- configs: yolox-s (32, 1) and yolox-l (64, 3) are served; m (48), x (80), tiny (24) and nano (16) are refused with the channel count
  auto cfg_refusal = [](rtd_yolox_net_config c) { return refusal([&] { yh::check_config(&c); }); };
  CHECK(cfg_refusal(config(RTD_PREC_F16X3, 80, 32, 1, 8)).empty() && cfg_refusal(config(RTD_PREC_FP32, 80, 64, 3, 64)).empty() && cfg_refusal(config(RTD_PREC_FP32, 1, 128, 8, 1)).empty());
  for (int base : {48, 80, 24, 16}) CHECK(cfg_refusal(config(RTD_PREC_F16X3, 80, base, 2, 8)).find("base_channels " + std::to_string(base)) == 0);
  CHECK(cfg_refusal(config(RTD_PREC_F16X3, 80, 4, 1, 8)).find("base_channels must") == 0 && cfg_refusal(config(RTD_PREC_F16X3, 80, 160, 1, 8)).find("base_channels must") == 0);
  CHECK(cfg_refusal(config(RTD_PREC_BF16, 80, 32, 1, 8)).find("precision") == 0);
  CHECK(cfg_refusal(config(RTD_PREC_F16X3, 0, 32, 1, 8)).find("num_classes") == 0 && cfg_refusal(config(RTD_PREC_F16X3, 1025, 32, 1, 8)).find("num_classes") == 0);
  CHECK(cfg_refusal(config(RTD_PREC_F16X3, 80, 32, 0, 8)).find("depth") == 0 && cfg_refusal(config(RTD_PREC_F16X3, 80, 32, 9, 8)).find("depth") == 0);
  CHECK(cfg_refusal(config(RTD_PREC_F16X3, 80, 32, 1, 0)).find("max_batch") == 0 && cfg_refusal(config(RTD_PREC_F16X3, 80, 32, 1, 65)).find("max_batch") == 0);
  rtd_yolox_net_config wrong = config(RTD_PREC_F16X3, 80, 32, 1, 8);
  wrong.struct_size = 28;
  CHECK(cfg_refusal(wrong).find("rtd_yolox_net_config") == 0 && !refusal([] { yh::check_config(nullptr); }).empty());
  wrong = config(RTD_PREC_F16X3, 80, 32, 1, 8);
  wrong.device = -1;
  CHECK(!cfg_refusal(wrong).empty());

  // ---- the checks of a call
  const rtd_yolox_net_config c = config(RTD_PREC_F16X3, 80, 32, 1, 8);
  alignas(16) float in[8];
  auto run_refusal = [&](int64_t n, const void* x, int64_t h, int64_t w, const void* pred) { return refusal([&] { yh::check_run(c, n, x, h, w, pred); }); };
  CHECK(run_refusal(8, in, 640, 640, in + 1).empty() && run_refusal(1, in + 4, 32, 64, in).empty());
  CHECK(run_refusal(0, in, 640, 640, in).find("1..max_batch") == 0 && run_refusal(9, in, 640, 640, in).find("1..max_batch") == 0);
  CHECK(run_refusal(1, nullptr, 640, 640, in).find("null") == 0 && run_refusal(1, in, 640, 640, nullptr).find("null") == 0);
  CHECK(run_refusal(1, in, 640, 650, in).find("the input size") == 0 && run_refusal(1, in, 0, 640, in).find("the input size") == 0 && !run_refusal(1, in, 16416, 64, in).empty());
  CHECK(run_refusal(1, in + 1, 640, 640, in).find("in_dev") == 0 && run_refusal(1, in, 640, 640, (const char*)in + 2).find("pred_dev") == 0);

  // ---- the checks of a call from frames: no alignment rule for a frame, null arrays and frames, sides 1..16384, then what check_run asks
  {
    const uint8_t bytes[16] = {0};
    const uint8_t* two[2] = {bytes + 1, bytes + 3};                       // (odd addresses are fine)
    const uint8_t* holed[2] = {bytes, nullptr};
    const int32_t hw[4] = {1080, 1920, 1, 16384};
    auto frames_refusal = [&](int64_t n, const uint8_t* const* f, const int32_t* s, int64_t h, int64_t w, const void* pred) {
      return refusal([&] { yh::check_run_frames(c, n, f, s, h, w, pred); });
    };
    CHECK(frames_refusal(2, two, hw, 640, 640, in).empty() && frames_refusal(1, two, hw, 32, 64, in + 1).empty());
    CHECK(frames_refusal(2, nullptr, hw, 640, 640, in).find("null") == 0 && frames_refusal(2, two, nullptr, 640, 640, in).find("null") == 0 &&
          frames_refusal(2, two, hw, 640, 640, nullptr).find("null") == 0);
    CHECK(frames_refusal(0, two, hw, 640, 640, in).find("1..max_batch") == 0 && frames_refusal(9, two, hw, 640, 640, in).find("1..max_batch") == 0);
    CHECK(frames_refusal(2, holed, hw, 640, 640, in).find("frame 1: null") == 0 && frames_refusal(1, holed, hw, 640, 640, in).empty());   // (only the n frames of the call are read)
    for (int32_t bad : {0, -1, 16385}) {
      const int32_t bh[4] = {1080, 1920, bad, 8}, bw[4] = {8, bad, 1080, 1920};
      CHECK(frames_refusal(2, two, bh, 640, 640, in).find("frame 1: sides") == 0 && frames_refusal(2, two, bw, 640, 640, in).find("frame 0: sides") == 0);
    }
    CHECK(frames_refusal(2, two, hw, 640, 650, in).find("the input size") == 0 && frames_refusal(2, two, hw, 640, 640, (const char*)in + 2).find("pred_dev") == 0);
    CHECK(refusal([&] { yh::check_frames(65, yh::MAX_BATCH, two, hw); }).find("1..max_batch") == 0);
  }

  // ---- the front end's index and weight rule: bilinear, align_corners = False, each operation one fp32 rounding
  {
    CHECK(yh::frame_scale(1080, 640) == 1.6875f && yh::frame_scale(1920, 640) == 3.f && yh::frame_scale(64, 64) == 1.f);
    // 2 -> 4: f = 0, 0.25, 0.75, 1.25
    const int want_i0[4] = {0, 0, 0, 1}, want_i1[4] = {1, 1, 1, 1};
    const float want_l1[4] = {0.f, 0.25f, 0.75f, 0.25f};
    for (int d = 0; d < 4; ++d) {
      const yh::FrameTap t = yh::frame_tap(yh::frame_scale(2, 4), d, 2);
      CHECK(t.i0 == want_i0[d] && t.i1 == want_i1[d] && t.l1 == want_l1[d] && t.l0 == 1.f - want_l1[d]);
    }
    // the identity size: every tap is the pixel itself with weight 1, and the blend returns the integer
    for (int d : {0, 1, 63, 16383}) {
      const yh::FrameTap t = yh::frame_tap(1.f, d, 16384);
      CHECK(t.i0 == d && t.l1 == 0.f && t.l0 == 1.f && t.i1 == (d < 16383 ? d + 1 : d));
      CHECK(yh::frame_blend(t, t, 255.f, 7.f, 9.f, 11.f) == 255.f);
    }
    // every tap of every size stays inside the frame, weights in [0, 1]; a 1-pixel side reads pixel 0 only
    for (int src : {1, 2, 3, 37, 1080, 2047, 16384})
      for (int dst : {2, 32, 96, 640, 16384})
        for (int d : {0, 1, dst / 2, dst - 2, dst - 1}) {
          const yh::FrameTap t = yh::frame_tap(yh::frame_scale(src, dst), d, src);
          CHECK(t.i0 >= 0 && t.i0 <= t.i1 && t.i1 <= src - 1 && t.i1 - t.i0 <= 1 && t.l1 >= 0.f && t.l1 <= 1.f && t.l0 >= 0.f && t.l0 <= 1.f);
          if (src == 1) CHECK(t.i0 == 0 && t.i1 == 0);
        }
    // 3 x downscale (1920 -> 640): f = 3 d + 1, exact; the blend of a 2 x 2 block with l1 = 0.5 on both axes is its mean
    const yh::FrameTap t3 = yh::frame_tap(3.f, 5, 1920), half = yh::frame_tap(2.f, 0, 4);
    CHECK(t3.i0 == 16 && t3.i1 == 17 && t3.l1 == 0.f && half.i0 == 0 && half.i1 == 1 && half.l1 == 0.5f);
    CHECK(yh::frame_blend(half, half, 0.f, 3.f, 12.f, 15.f) == 7.5f);
  }

  // ---- anchor offsets: levels in stride order, row-major within a level; the total is rtd_yolox_anchors
  for (auto hw : {std::pair<int, int>{640, 640}, {64, 96}, {160, 160}, {32, 32}, {416, 672}}) {
    int64_t off[yh::LEVELS + 1];
    int lh[yh::LEVELS], lw[yh::LEVELS];
    yh::level_offsets(hw.first, hw.second, off, lh, lw);
    CHECK(off[0] == 0 && off[yh::LEVELS] == yolox_post_host::anchors(hw.first, hw.second));
    for (int l = 0; l < yh::LEVELS; ++l) CHECK(lh[l] == hw.first / yh::STRIDES[l] && lw[l] == hw.second / yh::STRIDES[l] && off[l + 1] - off[l] == (int64_t)lh[l] * lw[l]);
  }
  {
    int64_t off[yh::LEVELS + 1];
    int lh[yh::LEVELS], lw[yh::LEVELS];
    yh::level_offsets(64, 96, off, lh, lw);
    CHECK(off[1] == 96 && off[2] == 120 && off[3] == 126);
  }

  // ---- the conv table: yolox-s has 80 convolutions (74 BaseConvs + 6 pred convs), yolox-l 128; names are unique; every channel count is a
  // multiple of 32 but a pred conv's outputs; a CSP's conv3 reads what its two halves write
  for (auto v : {std::tuple<int, int, size_t>{32, 1, 80}, {64, 3, 128}}) {
    const int base = std::get<0>(v), depth = std::get<1>(v);
    const std::vector<yh::ConvDesc> t = yh::conv_table(base, depth, 80);
    CHECK(t.size() == std::get<2>(v));
    std::set<std::string> names;
    for (const yh::ConvDesc& d : t) {
      CHECK(names.insert(d.name).second && (d.k == 1 || d.k == 3) && (d.stride == 1 || (d.stride == 2 && d.k == 3)) && d.cin % 32 == 0);
      const bool pred = d.name.find("_preds.") != std::string::npos;
      CHECK(pred ? (d.cout == 80 || d.cout == yh::PRED_REGOBJ) : d.cout % 32 == 0);
      if (d.name.size() > 6 && d.name.compare(d.name.size() - 6, 6, ".conv3") == 0) CHECK(d.cin == d.cout);
    }
    CHECK(t.front().name == "backbone.backbone.stem.conv" && t.front().cin == yh::FOCUS_C && t.front().cout == base);
    CHECK(t.back().name == "head.regobj_preds.2" && t.back().cin == 4 * base);
    CHECK(names.count("backbone.backbone.dark5.1.conv2") && names.count("backbone.C3_n4.m." + std::to_string(depth - 1) + ".conv2") &&
          names.count("backbone.backbone.dark3.1.m." + std::to_string(3 * depth - 1) + ".conv1") && !names.count("backbone.backbone.dark2.1.m." + std::to_string(depth) + ".conv1"));
  }
  CHECK(yh::pad32(80) == 96 && yh::pad32(3) == 32 && yh::pad32(5) == 32 && yh::pad32(32) == 32 && yh::pad32(1024) == 1024);

  // ---- the blob's table
  const std::vector<yh::ConvDesc> table = yh::conv_table(32, 1, 3);
  {
    const Blob b = blob_of(table);
    const std::vector<float> packed = b.pack();
    std::map<std::string, yh::HostTensor> host;
    yh::parse_blob((const char*)packed.data(), packed.size() * 4, host);
    CHECK(host.size() == 2 * table.size());
    for (const yh::ConvDesc& d : table)
      for (bool pair : {false, true}) yh::check_conv_tensors(host, d, pair);
    // another variant's table: the first conv that differs is named
    const std::vector<yh::ConvDesc> wide = yh::conv_table(64, 1, 3), deep = yh::conv_table(32, 2, 3), more = yh::conv_table(32, 1, 80);
    auto first_refusal = [&](const std::vector<yh::ConvDesc>& t) {
      return refusal([&] { for (const yh::ConvDesc& d : t) yh::check_conv_tensors(host, d, true); });
    };
    CHECK(first_refusal(wide).find("weight shape mismatch: backbone.backbone.stem.conv.weight") == 0);
    CHECK(first_refusal(deep).find("weight blob: missing tensor backbone.backbone.dark2.1.m.1.conv1.weight") == 0);
    CHECK(first_refusal(more).find("weight shape mismatch: head.cls_preds.0.weight") == 0);
    // every cut of the blob is refused, none reads past its end (the sanitizer watches)
    for (size_t cut : {(size_t)0, (size_t)8, (size_t)12, (size_t)40, packed.size() * 2, packed.size() * 4 - 64}) {      // (the last 64 bytes hold the last tensor)
      std::vector<float> part(packed.begin(), packed.begin() + cut / 4);
      std::map<std::string, yh::HostTensor> h2;
      CHECK(!refusal([&] { yh::parse_blob((const char*)part.data(), cut, h2); }, RTD_E_WEIGHTS).empty());
    }
  }
  {
    Blob b = blob_of(table);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    size_t at = 0;
    for (size_t i = 0; i < b.names.size(); ++i)
      if (b.names[i] == "backbone.C3_p3.conv2.weight") at = i;
    for (float bad : {nan, inf, -inf}) {
      b.data[at].back() = bad;
      const std::vector<float> packed = b.pack();
      std::map<std::string, yh::HostTensor> host;
      yh::parse_blob((const char*)packed.data(), packed.size() * 4, host);
      const std::string msg = refusal([&] { for (const yh::ConvDesc& d : table) yh::check_conv_tensors(host, d, false); }, RTD_E_WEIGHTS);
      CHECK(msg.find("backbone.C3_p3.conv2.weight holds a NaN or an infinity") != std::string::npos);
    }
    b.data[at].back() = 70000.f;
    const std::vector<float> packed = b.pack();
    std::map<std::string, yh::HostTensor> host;
    yh::parse_blob((const char*)packed.data(), packed.size() * 4, host);
    for (const yh::ConvDesc& d : table) yh::check_conv_tensors(host, d, false);            // fp32 engine: in range
    CHECK(refusal([&] { for (const yh::ConvDesc& d : table) yh::check_conv_tensors(host, d, true); }, RTD_E_WEIGHTS).find("backbone.C3_p3.conv2.weight reaches") != std::string::npos);
  }

  // ---- the SPP tiling: tiles cover the map once, the staged region is the tile and its halo, the blocks fit a launch
  CHECK(yh::SPP_REGION == yh::SPP_TILE + 2 * yh::SPP_HALO && yh::SPP_HALO == 3 * 2 && (size_t)2 * yh::SPP_REGION * yh::SPP_REGION * yh::SPP_CH * 4 <= 65536);
  for (int h : {1, 2, 5, 7, 19, 20, 21, 40, 41, 512})
    for (int w : {1, 3, 13, 20, 23, 60, 512}) {
      const yh::SppGrid g = yh::spp_grid(8, h, w, 256);
      CHECK(g.chunks == 256 / yh::SPP_CH && (g.tiles_x - 1) * yh::SPP_TILE < w && g.tiles_x * yh::SPP_TILE >= w && (g.tiles_y - 1) * yh::SPP_TILE < h && g.tiles_y * yh::SPP_TILE >= h);
      CHECK(g.blocks == (int64_t)8 * g.tiles_x * g.tiles_y * g.chunks);
    }
  CHECK(yh::spp_grid(1, 20, 20, 256).blocks == 32 && yh::spp_grid(8, 20, 20, 512).blocks == 512 && yh::spp_grid(64, 512, 512, 1024).blocks < ((int64_t)1 << 31));
  printf("yolox net host check ok\n");
  return 0;
}
