// yolox_net_host.h - the pure host parts of the YOLOX network (yolox_net.hip): the config checks and the variants served, the table of the
// network's convolutions (CSPDarknet, PAFPN, decoupled head) with the tensors the weight blob must hold for them, the per-level anchor
// offsets of the head rows, and how the SPP kernel tiles a map.  No HIP, no device: this header compiles on its own
// (tools/yolox_net_host_check.cpp runs it under -fsanitize=address,undefined).
#pragma once
#include <math.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "error.h"
#include "weight_blob.h"   // the packed blob: HostTensor, parse_blob, check_values
#include "yolox_post_host.h"   // anchors(): the input sizes served

namespace yolox_net_host {

using rtd::blob::HostTensor;
using rtd::blob::need;
using rtd::blob::parse_blob;

constexpr int MAX_BATCH = 64, MAX_CLASSES = 1024, MAX_DEPTH = 8, MAX_BASE = 128;
constexpr int FOCUS_C = 32;              // the Focus output: 12 channels in a whole 32-channel group, zeros above
constexpr int PRED_REGOBJ = 5;           // reg_pred (4) and obj_pred (1) stacked into one conv
constexpr int LEVELS = 3;
constexpr int STRIDES[LEVELS] = {8, 16, 32};
// the SPP kernel: a workgroup owns SPP_CH channels of an SPP_TILE x SPP_TILE tile and stages it with a halo of 6 (three 5-tap passes)
constexpr int SPP_TILE = 20, SPP_HALO = 6, SPP_REGION = SPP_TILE + 2 * SPP_HALO, SPP_CH = 8, SPP_THREADS = 1024;

inline int pad32(int c) { return (c + 31) / 32 * 32; }

// base = int(64 * width), depth = max(round(3 * depth_factor), 1): yolox-s is (32, 1), yolox-l (64, 3).  Every channel count of the
// network is a multiple of `base`, the narrowest (dark2's CSP halves, the Focus output) IS base: pair tensors need whole 32-channel groups.
inline void check_config(const rtd_yolox_net_config* c) {
  need(c && c->struct_size == (int32_t)sizeof(rtd_yolox_net_config), RTD_E_INVALID, "rtd_yolox_net_config: bad struct_size");
  need(c->precision == RTD_PREC_F16X3 || c->precision == RTD_PREC_FP32, RTD_E_INVALID, "precision must be RTD_PREC_F16X3 or RTD_PREC_FP32 (bf16 is refused)");
  need(c->base_channels >= 8 && c->base_channels <= MAX_BASE, RTD_E_INVALID, "base_channels must be 8..128");
  need(c->base_channels % 32 == 0, RTD_E_INVALID,
       "base_channels " + std::to_string(c->base_channels) + ": every channel count must be a multiple of 32 (yolox-s: 32, yolox-l: 64; m, x, tiny and nano are not served)");
  need(c->depth >= 1 && c->depth <= MAX_DEPTH, RTD_E_INVALID, "depth must be 1..8 bottlenecks per unit (yolox-s: 1, yolox-l: 3)");
  need(c->num_classes >= 1 && c->num_classes <= MAX_CLASSES, RTD_E_INVALID, "num_classes must be 1..1024");
  need(c->max_batch >= 1 && c->max_batch <= MAX_BATCH, RTD_E_INVALID, "max_batch must be 1..64");
  need(c->device >= 0, RTD_E_INVALID, "no such device");
}

inline void check_run(const rtd_yolox_net_config& c, int64_t n, const void* in, int64_t in_h, int64_t in_w, const void* pred) {
  need(in && pred, RTD_E_INVALID, "null argument");
  need(n >= 1 && n <= c.max_batch, RTD_E_INVALID, "1..max_batch (" + std::to_string(c.max_batch) + ") images per call, not " + std::to_string(n));
  (void)yolox_post_host::anchors(in_h, in_w);   // a multiple of 32 in 32..16384 per side
  need(((uintptr_t)in & 15) == 0, RTD_E_INVALID, "in_dev must lie on a 16-byte boundary");
  need(((uintptr_t)pred & 3) == 0, RTD_E_INVALID, "pred_dev must lie on a 4-byte boundary");
}

// ---- the uint8 front end (yolox_focus_u8): frames at their own sizes -> the resized image the Focus map is cut from.  The rule is
// F.interpolate(mode = "bilinear", align_corners = False) in fp32, every operation rounded on its own (no contraction into an FMA), so a
// numpy float32 restatement in the same order (tests/yolox_frames_ref.py) has the kernel's bits.  frame_scale runs on the host, frame_tap
// and frame_blend on both sides, as resize_taps.h shares cv2's rule.
constexpr int MAX_FRAME_SIDE = 16384;

#if defined(__HIPCC__)
#define YOLOX_FRAME_FN __host__ __device__ inline
#else
#define YOLOX_FRAME_FN inline
#endif

struct FrameTap {
  int i0, i1;        // the two source rows (or columns), clamped into the frame
  float l0, l1;      // their weights: l1 = the source coordinate's fraction, l0 = 1 - l1
};

inline float frame_scale(int src, int dst) { return (float)src / (float)dst; }

// area_pixel_compute_source_index(scale, d, align_corners = False, cubic = False) and the index / weight rule of upsample_bilinear2d
YOLOX_FRAME_FN FrameTap frame_tap(float scale, int d, int extent) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float centre = (float)d + 0.5f;
  const float scaled = scale * centre;
  float f = scaled - 0.5f;
  f = f < 0.f ? 0.f : f;
  FrameTap t;
  const int i = (int)f;
  t.i0 = i < extent - 1 ? i : extent - 1;
  t.i1 = t.i0 + 1 < extent - 1 ? t.i0 + 1 : extent - 1;
  t.l1 = f - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// one channel of one resized pixel from its four source values: nine operations, each one IEEE fp32
YOLOX_FRAME_FN float frame_blend(const FrameTap& ty, const FrameTap& tx, float p00, float p01, float p10, float p11) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = tx.l0 * p00, b = tx.l1 * p01, c = tx.l0 * p10, d = tx.l1 * p11;
  const float top = a + b, bot = c + d;
  const float u = ty.l0 * top, v = ty.l1 * bot;
  return u + v;
}

// rtd_yolox_net_run_frames: what rtd_yolox_net_run refuses but for the input's alignment (a frame lies at any byte address), a null
// array or frame, a side outside 1..16384.  check_frames alone is what rtd_op_yolox_focus_u8 shares.
inline void check_frames(int64_t n, int64_t max_batch, const uint8_t* const* frames, const int32_t* frame_hw) {
  need(frames && frame_hw, RTD_E_INVALID, "null argument");
  need(n >= 1 && n <= max_batch, RTD_E_INVALID, "1..max_batch (" + std::to_string(max_batch) + ") images per call, not " + std::to_string(n));
  for (int64_t i = 0; i < n; ++i) {
    need(frames[i], RTD_E_INVALID, "frame " + std::to_string(i) + ": null pointer");
    const int32_t h = frame_hw[2 * i], w = frame_hw[2 * i + 1];
    need(h >= 1 && h <= MAX_FRAME_SIDE && w >= 1 && w <= MAX_FRAME_SIDE, RTD_E_INVALID,
         "frame " + std::to_string(i) + ": sides must be 1..16384, not " + std::to_string(h) + " x " + std::to_string(w));
  }
}
inline void check_run_frames(const rtd_yolox_net_config& c, int64_t n, const uint8_t* const* frames, const int32_t* frame_hw, int64_t in_h, int64_t in_w,
                             const void* pred) {
  need(pred, RTD_E_INVALID, "null argument");
  check_frames(n, c.max_batch, frames, frame_hw);
  (void)yolox_post_host::anchors(in_h, in_w);   // a multiple of 32 in 32..16384 per side
  need(((uintptr_t)pred & 3) == 0, RTD_E_INVALID, "pred_dev must lie on a 4-byte boundary");
}

// first head row of each level (stride order, row-major over (y, x) within a level) and, in [LEVELS], the rows of an image
inline void level_offsets(int in_h, int in_w, int64_t off[LEVELS + 1], int lh[LEVELS], int lw[LEVELS]) {
  off[0] = 0;
  for (int l = 0; l < LEVELS; ++l) {
    lh[l] = in_h / STRIDES[l], lw[l] = in_w / STRIDES[l];
    off[l + 1] = off[l] + (int64_t)lh[l] * lw[l];
  }
}

// ---- the network's convolutions.  The blob (yolox_network.fold_state) holds per conv `name`.weight [cout][k][k][cin] fp32 - BatchNorm
// folded in, tap-major and channel-minor as launch_conv reads a filter row - and `name`.bias [cout].  The stem's cin is the Focus
// output's 32; head.regobj_preds.<l> is reg_preds.<l> stacked on obj_preds.<l>.
struct ConvDesc {
  std::string name;
  int cin, cout, k, stride;
};
inline void csp_table(std::vector<ConvDesc>& t, const std::string& p, int cin, int cout, int n) {
  const int h = cout / 2;
  t.push_back({p + ".conv1", cin, h, 1, 1});
  t.push_back({p + ".conv2", cin, h, 1, 1});
  for (int i = 0; i < n; ++i) {
    t.push_back({p + ".m." + std::to_string(i) + ".conv1", h, h, 1, 1});
    t.push_back({p + ".m." + std::to_string(i) + ".conv2", h, h, 3, 1});
  }
  t.push_back({p + ".conv3", 2 * h, cout, 1, 1});
}
inline std::vector<ConvDesc> conv_table(int base, int depth, int num_classes) {
  std::vector<ConvDesc> t;
  const std::string bb = "backbone.backbone.", fp = "backbone.";
  t.push_back({bb + "stem.conv", FOCUS_C, base, 3, 1});
  const int units[4] = {depth, 3 * depth, 3 * depth, depth};
  for (int s = 0; s < 4; ++s) {
    const std::string d = bb + "dark" + std::to_string(s + 2);
    const int cin = base << s, cout = base << (s + 1);
    t.push_back({d + ".0", cin, cout, 3, 2});
    if (s == 3) {
      t.push_back({d + ".1.conv1", cout, cout / 2, 1, 1});
      t.push_back({d + ".1.conv2", 2 * cout, cout, 1, 1});
      csp_table(t, d + ".2", cout, cout, units[s]);
    } else {
      csp_table(t, d + ".1", cout, cout, units[s]);
    }
  }
  const int c3 = 4 * base, c4 = 8 * base, c5 = 16 * base;
  t.push_back({fp + "lateral_conv0", c5, c4, 1, 1});
  csp_table(t, fp + "C3_p4", 2 * c4, c4, depth);
  t.push_back({fp + "reduce_conv1", c4, c3, 1, 1});
  csp_table(t, fp + "C3_p3", 2 * c3, c3, depth);
  t.push_back({fp + "bu_conv2", c3, c3, 3, 2});
  csp_table(t, fp + "C3_n3", 2 * c3, c4, depth);
  t.push_back({fp + "bu_conv1", c4, c4, 3, 2});
  csp_table(t, fp + "C3_n4", 2 * c4, c5, depth);
  const int hc = 4 * base, lc[LEVELS] = {c3, c4, c5};
  for (int l = 0; l < LEVELS; ++l) {
    const std::string s = std::to_string(l);
    t.push_back({"head.stems." + s, lc[l], hc, 1, 1});
    for (int j = 0; j < 2; ++j) t.push_back({"head.cls_convs." + s + "." + std::to_string(j), hc, hc, 3, 1});
    for (int j = 0; j < 2; ++j) t.push_back({"head.reg_convs." + s + "." + std::to_string(j), hc, hc, 3, 1});
    t.push_back({"head.cls_preds." + s, hc, num_classes, 1, 1});
    t.push_back({"head.regobj_preds." + s, hc, PRED_REGOBJ, 1, 1});
  }
  return t;
}

// `name`.weight / `name`.bias of the blob: present and of the conv's shape (else the blob is not this variant's: RTD_E_INVALID), finite
// and - pair engine - inside fp16's range (RTD_E_WEIGHTS, with the tensor's name)
inline void check_conv_tensors(const std::map<std::string, HostTensor>& host, const ConvDesc& d, bool pair) {
  const auto w = host.find(d.name + ".weight"), b = host.find(d.name + ".bias");
  need(w != host.end(), RTD_E_INVALID, "weight blob: missing tensor " + d.name + ".weight (not this variant's table)");
  need(b != host.end(), RTD_E_INVALID, "weight blob: missing tensor " + d.name + ".bias (not this variant's table)");
  const std::vector<int64_t> ws{d.cout, d.k, d.k, d.cin}, bs{d.cout};
  need(w->second.shape == ws, RTD_E_INVALID, "weight shape mismatch: " + d.name + ".weight (not this variant's table)");
  need(b->second.shape == bs, RTD_E_INVALID, "bias shape mismatch: " + d.name + ".bias (not this variant's table)");
  rtd::blob::check_values(d.name + ".weight", w->second, pair);
  rtd::blob::check_values(d.name + ".bias", b->second, pair);
}

// the SPP launch: one workgroup per (image, tile, chunk of SPP_CH channels)
struct SppGrid {
  int tiles_x, tiles_y, chunks;
  int64_t blocks;
};
inline SppGrid spp_grid(int64_t n, int h, int w, int c) {
  SppGrid g;
  g.tiles_x = (w + SPP_TILE - 1) / SPP_TILE, g.tiles_y = (h + SPP_TILE - 1) / SPP_TILE, g.chunks = c / SPP_CH;
  g.blocks = n * g.tiles_x * g.tiles_y * g.chunks;
  return g;
}

}  // namespace yolox_net_host
