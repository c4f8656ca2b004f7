// yolox_post_host.h - the pure host parts of the YOLOX post-processing (yolox_post.hip): the limits of a handle, the anchor count of an
// input size, the argument checks of a call, how the score pass tiles its rows, and where everything lies in the handle's scratch.
// No HIP here, so that tools/yolox_post_host_check.cpp can run all of it under the sanitizers on a CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/rtdetr_mi355.h"
#include "call_parts.h"
#include "error.h"

namespace yolox_post_host {

using rtd::backend::align_up;

constexpr int MAX_CLASSES = 1024, MAX_BATCH = 64, MAX_ANCHORS = 1 << 20, MIN_CANDIDATES = 64, MAX_CANDIDATES = 8192;
constexpr int KEEP_WORDS = MAX_CLASSES / 32;
constexpr int MAX_INPUT_SIDE = 16384;
constexpr int ROW_OUT = 7;                // x1, y1, x2, y2, obj, class_conf, class_id
constexpr int ROW_RANKED = 8;             // the same seven and the box's area: two 16-byte loads
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_LDS_WORDS = 6144;     // 24 KiB: 64 rows of 85 floats with room to spare, five rows at 1024 classes

inline void check_config(const rtd_yolox_post_config* c) {
  RTD_CHECK(c && c->struct_size == (int32_t)sizeof(rtd_yolox_post_config), RTD_E_INVALID, "rtd_yolox_post_config: bad struct_size");
  RTD_CHECK(c->num_classes >= 1 && c->num_classes <= MAX_CLASSES, RTD_E_INVALID, "num_classes must be 1..1024");
  RTD_CHECK(c->max_batch >= 1 && c->max_batch <= MAX_BATCH, RTD_E_INVALID, "max_batch must be 1..64");
  RTD_CHECK(c->max_anchors >= 1 && c->max_anchors <= MAX_ANCHORS, RTD_E_INVALID, "max_anchors must be 1..2^20");
  RTD_CHECK(c->max_candidates >= MIN_CANDIDATES && c->max_candidates <= MAX_CANDIDATES && c->max_candidates % 64 == 0, RTD_E_INVALID,
            "max_candidates must be a multiple of 64 in 64..8192");
}

// the anchors of YOLOX's three levels (strides 8, 16, 32) on an in_h x in_w input
inline int32_t anchors(int64_t in_h, int64_t in_w) {
  RTD_CHECK(in_h >= 32 && in_w >= 32 && in_h <= MAX_INPUT_SIDE && in_w <= MAX_INPUT_SIDE && in_h % 32 == 0 && in_w % 32 == 0, RTD_E_INVALID,
            "the input size must be a multiple of 32 in 32..16384 per side");
  return (int32_t)((in_h / 8) * (in_w / 8) + (in_h / 16) * (in_w / 16) + (in_h / 32) * (in_w / 32));
}

// checks every argument of a call; nothing is allocated or launched before the whole call has passed
inline void check_run(const rtd_yolox_post_config& c, int64_t n, const void* pred, int64_t n_anchors, const rtd_yolox_post_params* p,
                      const void* rows, const void* counts) {
  RTD_CHECK(p && p->struct_size == (int32_t)sizeof(rtd_yolox_post_params), RTD_E_INVALID, "rtd_yolox_post_params: bad struct_size");
  RTD_CHECK(n >= 1 && n <= c.max_batch, RTD_E_INVALID, "1..max_batch (" + std::to_string(c.max_batch) + ") images per call, not " + std::to_string(n));
  RTD_CHECK(n_anchors >= 1 && n_anchors <= c.max_anchors, RTD_E_INVALID,
            "1..max_anchors (" + std::to_string(c.max_anchors) + ") anchors per image, not " + std::to_string(n_anchors));
  RTD_CHECK(pred && rows && counts, RTD_E_INVALID, "null argument");
  RTD_CHECK(((uintptr_t)pred & 3) == 0, RTD_E_INVALID, "pred_dev must lie on a 4-byte boundary");
  RTD_CHECK(isfinite(p->conf_threshold) && p->conf_threshold >= 0.f && p->conf_threshold <= 1.f, RTD_E_INVALID, "conf_threshold must be in [0, 1]");
  RTD_CHECK(isfinite(p->nms_threshold) && p->nms_threshold >= 0.f && p->nms_threshold <= 1.f, RTD_E_INVALID, "nms_threshold must be in [0, 1]");
  RTD_CHECK(p->decode == 0 || p->decode == 1, RTD_E_INVALID, "decode must be 0 or 1");
  if (p->decode == 1) {
    const int32_t want = anchors(p->in_h, p->in_w);
    RTD_CHECK(n_anchors == want, RTD_E_INVALID,
              "decode: a " + std::to_string(p->in_h) + " x " + std::to_string(p->in_w) + " input has " + std::to_string(want) + " anchors, not " +
                  std::to_string(n_anchors));
  }
}

// the class filter as the kernels take it: KEEP_WORDS words, every class set when the caller gave none, no bit at or past num_classes
inline void keep_words(int num_classes, const uint32_t* class_keep, uint32_t* out) {
  const int words = (num_classes + 31) / 32;
  for (int w = 0; w < KEEP_WORDS; ++w) {
    uint32_t v = w < words ? (class_keep ? class_keep[w] : 0xffffffffu) : 0u;
    const int first = w * 32;
    if (first + 32 > num_classes) v &= num_classes > first ? (0xffffffffu >> (32 - (num_classes - first))) : 0u;
    out[w] = v;
  }
}

// how the score pass tiles an image: a workgroup stages `rows` whole rows in LDS at a row stride of `stride` words (odd, so that lanes
// that walk different rows meet different banks), and 2^tpr_log2 neighbouring lanes share a row's class scores
struct ScoreTile {
  int floats, stride, rows, tpr_log2;
};
inline ScoreTile score_tile(int num_classes) {
  ScoreTile t;
  t.floats = 5 + num_classes;
  t.stride = t.floats | 1;
  t.rows = std::min(64, SCORE_LDS_WORDS / t.stride);
  t.tpr_log2 = 0;
  while ((2 << t.tpr_log2) * t.rows <= SCORE_THREADS && t.tpr_log2 < 6) ++t.tpr_log2;
  return t;
}

// the scratch of a call: [passed counts | candidate composites | class of a candidate | ranked rows | suppression bits], each on a
// 256-byte boundary
struct Layout {
  size_t passed = 0;       // int32 [n]
  size_t cand = 0;         // uint64 [n][n_anchors]
  size_t meta = 0;         // float2 [n][n_anchors]: class_conf, class_id of the anchors that passed
  size_t ranked = 0;       // float [n][max_candidates][ROW_RANKED]
  size_t mask = 0;         // uint64 [n][max_candidates][max_candidates / 64]
  size_t total = 0;
  int words = 0;           // max_candidates / 64
};
inline Layout layout(int64_t n, int64_t n_anchors, int64_t max_candidates) {
  Layout l;
  l.words = (int)(max_candidates / 64);
  l.passed = 0;
  l.cand = align_up((size_t)n * sizeof(int32_t), 256);
  l.meta = align_up(l.cand + (size_t)n * n_anchors * sizeof(uint64_t), 256);
  l.ranked = align_up(l.meta + (size_t)n * n_anchors * 2 * sizeof(float), 256);
  l.mask = align_up(l.ranked + (size_t)n * max_candidates * ROW_RANKED * sizeof(float), 256);
  l.total = align_up(l.mask + (size_t)n * max_candidates * l.words * sizeof(uint64_t), 256);
  return l;
}

}  // namespace yolox_post_host
