// esrgan_host.h - the pure host parts of the Real-ESRGAN x4 crop upscaler (esrgan.hip): config checks, the output layout, the tile
// rectangles of RealESRGANer.tile_process and the list of RRDBNet's convolutions with the blob tensors they need (the blob itself:
// weight_blob.h).  No HIP, no device: this
// header compiles on its own (tools/esrgan_host_check.cpp runs it under -fsanitize=address,undefined).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "error.h"
#include "weight_blob.h"

namespace esrgan_host {

using rtd::blob::HostTensor;   // the packed blob (weight_blob.h)
using rtd::blob::need;
using rtd::blob::parse_blob;

constexpr int SCALE = 4;
constexpr int MIN_SIDE = 8, MAX_SIDE = 4096, MAX_ONE_PASS_SIDE = 576, MAX_CROPS = 64;
constexpr int64_t CROP_ALIGN = 256;

inline void check_config(const rtd_esrgan_config* c) {
  need(c && c->struct_size == (int32_t)sizeof(rtd_esrgan_config), RTD_E_INVALID, "rtd_esrgan_config: bad struct_size");
  need(c->precision == RTD_PREC_F16X3 || c->precision == RTD_PREC_FP32, RTD_E_INVALID,
       "precision must be RTD_PREC_F16X3 or RTD_PREC_FP32 (plain bf16 storage changes a third of the output bytes: refused)");
  need(c->num_feat == 64 && c->num_grow_ch == 32, RTD_E_INVALID, "num_feat must be 64 and num_grow_ch 32");
  need(c->num_block >= 1 && c->num_block <= 32, RTD_E_INVALID, "num_block must be 1..32");
  need(c->tile == 0 || (c->tile >= 16 && c->tile <= 512), RTD_E_INVALID, "tile must be 0 (one pass) or 16..512");
  need(c->tile_pad >= 0 && c->tile_pad <= 32, RTD_E_INVALID, "tile_pad must be 0..32");
  need(c->device >= 0, RTD_E_INVALID, "no such device");
}

// rects = [n][4] x1, y1, x2, y2 -> offsets[n + 1]: crop i is 4h x 4w x 3 (HWC, tight rows) at offsets[i], a multiple of 256
inline void layout(int32_t n, const int32_t* rects, int64_t* offsets) {
  need(n >= 0 && offsets && (rects || n == 0), RTD_E_INVALID, "layout: null argument or negative count");
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t x1 = rects[4 * i], y1 = rects[4 * i + 1], x2 = rects[4 * i + 2], y2 = rects[4 * i + 3];
    const std::string ci = "crop " + std::to_string(i);
    need(x1 >= 0 && y1 >= 0, RTD_E_INVALID, ci + " has a negative corner");
    const int64_t w = x2 - x1, h = y2 - y1;
    need(w >= MIN_SIDE && h >= MIN_SIDE && w <= MAX_SIDE && h <= MAX_SIDE, RTD_E_INVALID, ci + ": sides must be 8..4096 pixels");
    offsets[i] = at;
    at += (SCALE * h * SCALE * w * 3 + CROP_ALIGN - 1) / CROP_ALIGN * CROP_ALIGN;
  }
  offsets[n] = at;
}

// RealESRGANer.tile_process: the core of tile (ty, tx) is [tx * tile, min((tx + 1) * tile, W)), its input the core extended by `pad`
// and clamped to the crop.  tile == 0: the whole crop is one pass.  Coordinates are relative to the crop.
struct TileRect {
  int cx0, cy0, cx1, cy1;   // core
  int ix0, iy0, ix1, iy1;   // input
};
inline std::vector<TileRect> tile_rects(int H, int W, int tile, int pad) {
  std::vector<TileRect> out;
  if (tile <= 0) {
    out.push_back(TileRect{0, 0, W, H, 0, 0, W, H});
    return out;
  }
  const int nty = (H + tile - 1) / tile, ntx = (W + tile - 1) / tile;
  for (int ty = 0; ty < nty; ++ty)
    for (int tx = 0; tx < ntx; ++tx) {
      TileRect t;
      t.cx0 = tx * tile, t.cy0 = ty * tile;
      t.cx1 = t.cx0 + tile < W ? t.cx0 + tile : W;
      t.cy1 = t.cy0 + tile < H ? t.cy0 + tile : H;
      t.ix0 = t.cx0 - pad > 0 ? t.cx0 - pad : 0, t.iy0 = t.cy0 - pad > 0 ? t.cy0 - pad : 0;
      t.ix1 = t.cx1 + pad < W ? t.cx1 + pad : W, t.iy1 = t.cy1 + pad < H ? t.cy1 + pad : H;
      out.push_back(t);
    }
  return out;
}

// ---- RRDBNet(3, 3, 64, B, 32, scale 4): its convolutions in execution order (all 3x3, stride 1, pad 1, with bias)
struct ConvDesc {
  std::string name;   // state-dict prefix: `name`.weight [cout][cin][3][3], `name`.bias [cout]
  int cin, cout;
};
inline std::vector<ConvDesc> conv_table(int num_block) {
  std::vector<ConvDesc> t;
  t.push_back({"conv_first", 3, 64});
  for (int i = 0; i < num_block; ++i)
    for (int j = 1; j <= 3; ++j)
      for (int k = 1; k <= 5; ++k)
        t.push_back({"body." + std::to_string(i) + ".rdb" + std::to_string(j) + ".conv" + std::to_string(k), 64 + 32 * (k - 1), k == 5 ? 64 : 32});
  t.push_back({"conv_body", 64, 64});
  t.push_back({"conv_up1", 64, 64});
  t.push_back({"conv_up2", 64, 64});
  t.push_back({"conv_hr", 64, 64});
  t.push_back({"conv_last", 64, 3});
  return t;
}

// `name`.weight / `name`.bias of the blob: present, of the conv's shape, finite, and - pair engine - inside fp16's range
inline void check_conv_tensors(const std::map<std::string, HostTensor>& host, const ConvDesc& d, bool pair) {
  const auto w = host.find(d.name + ".weight"), b = host.find(d.name + ".bias");
  need(w != host.end(), RTD_E_WEIGHTS, "weight blob: missing tensor " + d.name + ".weight");
  need(b != host.end(), RTD_E_WEIGHTS, "weight blob: missing tensor " + d.name + ".bias");
  const std::vector<int64_t> ws{d.cout, d.cin, 3, 3}, bs{d.cout};
  need(w->second.shape == ws, RTD_E_WEIGHTS, "weight shape mismatch: " + d.name + ".weight");
  need(b->second.shape == bs, RTD_E_WEIGHTS, "bias shape mismatch: " + d.name + ".bias");
  rtd::blob::check_values(d.name + ".weight", w->second, pair);
  rtd::blob::check_values(d.name + ".bias", b->second, pair);
}

// OIHW fp32 -> the conv kernels' filter rows [npad][kcols]: k = tap * cin_pad + channel (tap-major, channel-minor), zero padded;
// every value times `scale` (a dense block's conv5 carries the block's 0.2)
inline std::vector<float> filter_rows(const HostTensor& w, int cout, int cin, int cin_pad, int npad, int kcols, float scale) {
  std::vector<float> pad((size_t)npad * kcols, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < 9; ++t) pad[(size_t)o * kcols + (size_t)t * cin_pad + c] = w.data[((size_t)o * cin + c) * 9 + t] * scale;
  return pad;
}

}  // namespace esrgan_host
