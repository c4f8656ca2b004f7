// Stand-alone check of the pure host parts of the YOLOX post-processing (csrc/yolox_post_host.h): the limits of a handle, the anchor
// count, the argument checks of a call, the class filter's words, the score pass's tiling and the scratch layout.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. tools/yolox_post_host_check.cpp -o yolox_post_host_check && ./yolox_post_host_check
#include <stdio.h>
#include <stdlib.h>

#include <limits>

#include "../telescope_cam_detection_amd/csrc/yolox_post_host.h"

namespace yh = yolox_post_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s at line %d\n", #c, __LINE__); exit(1); } } while (0)

template <typename F>
static std::string refusal(F&& f) {
  try { f(); } catch (const rtd::Error& e) { CHECK(e.code == RTD_E_INVALID); return e.what(); }
  return "";
}

static rtd_yolox_post_config config(int classes, int batch, int anchors, int cand) {
  return {(int32_t)sizeof(rtd_yolox_post_config), 0, classes, batch, anchors, cand};
}

int main() {
  CHECK(sizeof(rtd_yolox_post_config) == 24 && sizeof(rtd_yolox_post_params) == 32);

  // ---- the limits of a handle
  auto cfg_refusal = [](rtd_yolox_post_config c) { return refusal([&] { yh::check_config(&c); }); };
  CHECK(cfg_refusal(config(80, 8, 8400, 2048)).empty() && cfg_refusal(config(1, 1, 1, 64)).empty() && cfg_refusal(config(1024, 64, 1 << 20, 8192)).empty());
  CHECK(cfg_refusal(config(0, 8, 8400, 2048)).find("num_classes") == 0 && cfg_refusal(config(1025, 8, 8400, 2048)).find("num_classes") == 0);
  CHECK(cfg_refusal(config(80, 0, 8400, 2048)).find("max_batch") == 0 && cfg_refusal(config(80, 65, 8400, 2048)).find("max_batch") == 0);
  CHECK(cfg_refusal(config(80, 8, 0, 2048)).find("max_anchors") == 0 && cfg_refusal(config(80, 8, (1 << 20) + 1, 2048)).find("max_anchors") == 0);
  for (int bad : {0, 63, 100, 8256, -64}) CHECK(cfg_refusal(config(80, 8, 8400, bad)).find("max_candidates") == 0);
  rtd_yolox_post_config wrong = config(80, 8, 8400, 2048);
  wrong.struct_size = 20;
  CHECK(cfg_refusal(wrong).find("rtd_yolox_post_config") == 0 && !refusal([] { yh::check_config(nullptr); }).empty());

  // ---- anchors
  CHECK(yh::anchors(640, 640) == 8400 && yh::anchors(416, 416) == 3549 && yh::anchors(64, 96) == 126 && yh::anchors(160, 160) == 525 && yh::anchors(32, 32) == 21);
  CHECK(yh::anchors(16384, 16384) == 2048 * 2048 + 1024 * 1024 + 512 * 512);
  for (auto hw : {std::pair<int64_t, int64_t>{100, 96}, {96, 100}, {0, 64}, {64, -32}, {16416, 64}, {INT32_MAX, INT32_MAX}})
    CHECK(!refusal([&] { yh::anchors(hw.first, hw.second); }).empty());

  // ---- the checks of a call
  const rtd_yolox_post_config c = config(80, 8, 8400, 2048);
  float dummy[4];
  auto params = [](float conf, float nms, int decode = 0, int h = 0, int w = 0) {
    rtd_yolox_post_params p = {(int32_t)sizeof(rtd_yolox_post_params), conf, nms, decode, h, w, nullptr};
    return p;
  };
  auto run_refusal = [&](int64_t n, const void* pred, int64_t A, rtd_yolox_post_params p, const void* rows = (const void*)16, const void* counts = (const void*)16) {
    return refusal([&] { yh::check_run(c, n, pred, A, &p, rows, counts); });
  };
  CHECK(run_refusal(8, dummy, 8400, params(0.25f, 0.45f)).empty() && run_refusal(1, dummy + 1, 1, params(0.f, 1.f)).empty());
  CHECK(!run_refusal(0, dummy, 8400, params(0.25f, 0.45f)).empty() && !run_refusal(9, dummy, 8400, params(0.25f, 0.45f)).empty());
  CHECK(!run_refusal(8, dummy, 0, params(0.25f, 0.45f)).empty() && !run_refusal(8, dummy, 8401, params(0.25f, 0.45f)).empty());
  CHECK(run_refusal(8, nullptr, 8400, params(0.25f, 0.45f)).find("null") == 0 && run_refusal(8, dummy, 8400, params(0.25f, 0.45f), nullptr).find("null") == 0);
  CHECK(run_refusal(8, dummy, 8400, params(0.25f, 0.45f), (const void*)16, nullptr).find("null") == 0);
  CHECK(!run_refusal(8, (const char*)dummy + 2, 8400, params(0.25f, 0.45f)).empty());
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (float bad : {-0.01f, 1.5f, nan, inf, -inf}) {
    CHECK(run_refusal(8, dummy, 8400, params(bad, 0.45f)).find("conf_threshold") == 0);
    CHECK(run_refusal(8, dummy, 8400, params(0.25f, bad)).find("nms_threshold") == 0);
  }
  CHECK(run_refusal(8, dummy, 8400, params(0.25f, 0.45f, 1, 640, 640)).empty() && run_refusal(8, dummy, 3549, params(0.25f, 0.45f, 1, 416, 416)).empty());
  CHECK(run_refusal(8, dummy, 8400, params(0.25f, 0.45f, 1, 416, 416)).find("decode") == 0 && !run_refusal(8, dummy, 8400, params(0.25f, 0.45f, 1, 100, 96)).empty());
  CHECK(!run_refusal(8, dummy, 8400, params(0.25f, 0.45f, 2)).empty());
  rtd_yolox_post_params bad_size = params(0.25f, 0.45f);
  bad_size.struct_size = 28;
  CHECK(run_refusal(8, dummy, 8400, bad_size).find("rtd_yolox_post_params") == 0);
  CHECK(!refusal([&] { yh::check_run(c, 8, dummy, 8400, nullptr, dummy, dummy); }).empty());

  // ---- the class filter: exact-size input, no bit at or past num_classes
  for (int C : {1, 3, 31, 32, 33, 80, 1000, 1024}) {
    const int words = (C + 31) / 32;
    uint32_t* in = (uint32_t*)malloc(sizeof(uint32_t) * words);          // exact size
    for (int w = 0; w < words; ++w) in[w] = 0xffffffffu;
    uint32_t out[yh::KEEP_WORDS];
    for (const uint32_t* src : {(const uint32_t*)nullptr, (const uint32_t*)in}) {
      yh::keep_words(C, src, out);
      int bits = 0;
      for (int b = 0; b < yh::MAX_CLASSES; ++b) {
        const bool set = (out[b >> 5] >> (b & 31)) & 1u;
        CHECK(set == (b < C));
        bits += set;
      }
      CHECK(bits == C);
    }
    in[0] = 0;
    yh::keep_words(C, in, out);
    CHECK(out[0] == 0);
    free(in);
  }

  // ---- the score pass's tiling: whole rows inside the LDS array, an odd stride, no more lanes than the workgroup has
  for (int C = 1; C <= yh::MAX_CLASSES; ++C) {
    const yh::ScoreTile t = yh::score_tile(C);
    CHECK(t.floats == 5 + C && t.stride >= t.floats && t.stride % 2 == 1 && t.rows >= 1 && t.rows <= 64);
    CHECK(t.rows * t.stride <= yh::SCORE_LDS_WORDS && t.tpr_log2 >= 0 && t.tpr_log2 <= 6 && (t.rows << t.tpr_log2) <= yh::SCORE_THREADS);
    CHECK(t.tpr_log2 == 6 || (t.rows << (t.tpr_log2 + 1)) > yh::SCORE_THREADS);
  }
  CHECK(yh::score_tile(80).rows == 64 && yh::score_tile(80).stride == 85 && yh::score_tile(80).tpr_log2 == 2 && yh::score_tile(3).stride == 9);

  // ---- the scratch: five parts in order, on 256-byte boundaries, none inside another
  for (int64_t n : {1, 8, 64})
    for (int64_t A : {1, 126, 8400, 1 << 20})
      for (int64_t K : {64, 2048, 8192}) {
        const yh::Layout l = yh::layout(n, A, K);
        CHECK(l.words == K / 64 && l.passed == 0 && l.cand % 256 == 0 && l.meta % 256 == 0 && l.ranked % 256 == 0 && l.mask % 256 == 0 && l.total % 256 == 0);
        CHECK(l.cand >= (size_t)n * 4 && l.meta >= l.cand + (size_t)n * A * 8 && l.ranked >= l.meta + (size_t)n * A * 8 && l.mask >= l.ranked + (size_t)n * K * yh::ROW_RANKED * 4);
        CHECK(l.total >= l.mask + (size_t)n * K * (K / 64) * 8);
      }
  CHECK(yh::layout(64, 1 << 20, 8192).total < ((size_t)1 << 31));
  printf("yolox post host check ok\n");
  return 0;
}
