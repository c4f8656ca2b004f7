// classifier_host.h - the pure host parts of the EVA02 species classifier (classifier.hip): config checks, the derived extents, the weight
// blob's tensor table and the arena layout of one batch size.  No HIP, no device: this header compiles on its own
// (tools/eva_host_check.cpp runs it under -fsanitize=address,undefined).  The blob is the container of weight_blob.h (weights.pack_blob),
// holding the tensors eva_checkpoint.fold_state wrote: already folded and zero-padded, so the table below is a plain shape check.
#pragma once
#include <math.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/rtdetr_mi355.h"
#include "error.h"
#include "weight_blob.h"   // need(), HostTensor, parse_blob, check_values: one blob format for every back end that reads weights

namespace eva_host {

using rtd::blob::HostTensor;
using rtd::blob::need;
using rtd::blob::parse_blob;

constexpr int HEAD_DIM = 64, MAX_BATCH = 64, MAX_LN_C = 4096, MAX_IMG = 1024, MAX_DEPTH = 64;

inline int pad32(int v) { return (v + 31) / 32 * 32; }

struct Dims {
  int G = 0;    // patches per side
  int L = 0;    // tokens: G * G + 1 (the cls token first)
  int Kp = 0;   // 3 * patch * patch in whole 32-channel groups (ViT-L/14: 588 -> 608)
  int Hp = 0;   // SwiGLU hidden width in whole 32-channel groups (2730 -> 2752)
  int Cp = 0;   // classes in whole 32-channel groups (launch_conv's fp32 rows)
};
inline Dims dims(const rtd_eva_config& c) {
  Dims d;
  d.G = c.img / c.patch;
  d.L = d.G * d.G + 1;
  d.Kp = pad32(3 * c.patch * c.patch);
  d.Hp = pad32(c.hidden);
  d.Cp = pad32(c.classes);
  return d;
}

inline void check_config(const rtd_eva_config* c) {
  need(c && c->struct_size == (int32_t)sizeof(rtd_eva_config), RTD_E_INVALID, "rtd_eva_config: bad struct_size");
  need(c->precision == RTD_PREC_F16X3 || c->precision == RTD_PREC_FP32, RTD_E_INVALID, "precision must be RTD_PREC_F16X3 or RTD_PREC_FP32");
  need(c->max_batch >= 1 && c->max_batch <= MAX_BATCH, RTD_E_INVALID, "max_batch must be 1..64");
  need(c->patch >= 1 && c->patch <= 64 && c->img >= c->patch && c->img <= MAX_IMG && c->img % c->patch == 0, RTD_E_INVALID,
       "img must be a multiple of patch (patch 1..64, img up to 1024)");
  need(c->heads >= 1 && c->dim == c->heads * HEAD_DIM, RTD_E_INVALID, "head dim must be 64 (dim = 64 * heads)");
  need(c->dim <= MAX_LN_C, RTD_E_INVALID, "dim must be at most 4096");
  need(c->depth >= 1 && c->depth <= MAX_DEPTH, RTD_E_INVALID, "depth must be 1..64");
  need(c->hidden >= 1 && c->hidden <= MAX_LN_C, RTD_E_INVALID, "hidden must be 1..4096");
  need(c->classes >= 1 && c->classes <= 1 << 20, RTD_E_INVALID, "classes must be 1..1048576");
  need(c->pool == RTD_EVA_POOL_TOKEN || c->pool == RTD_EVA_POOL_AVG, RTD_E_INVALID, "pool must be RTD_EVA_POOL_TOKEN or RTD_EVA_POOL_AVG");
  need((c->scale_attn_inner | c->scale_mlp) >> 1 == 0, RTD_E_INVALID, "scale_attn_inner and scale_mlp are 0 or 1");
  need(c->device >= 0, RTD_E_INVALID, "no such device");
}

// ---- the tensors of the blob, in upload order
struct TensorDesc {
  std::string name;
  std::vector<int64_t> shape;
};
inline std::vector<TensorDesc> tensor_table(const rtd_eva_config& c) {
  const Dims d = dims(c);
  const int64_t D = c.dim;
  std::vector<TensorDesc> t;
  auto lin = [&](const std::string& n, int64_t out, int64_t in) { t.push_back({n + ".weight", {out, in}}); t.push_back({n + ".bias", {out}}); };
  auto ln = [&](const std::string& n, int64_t w) { t.push_back({n + ".weight", {w}}); t.push_back({n + ".bias", {w}}); };
  lin("patch_embed", D, d.Kp);
  t.push_back({"cls_token", {D}});
  t.push_back({"pos_embed", {d.L, D}});
  t.push_back({"rope_sin", {d.L - 1, HEAD_DIM}});
  t.push_back({"rope_cos", {d.L - 1, HEAD_DIM}});
  for (int i = 0; i < c.depth; ++i) {
    const std::string b = "blocks." + std::to_string(i);
    ln(b + ".norm1", D);
    lin(b + ".attn.qkv", 3 * D, D);
    if (c.scale_attn_inner) ln(b + ".attn.norm", D);
    lin(b + ".attn.proj", D, D);
    ln(b + ".norm2", D);
    lin(b + ".mlp.fc1", 2 * d.Hp, D);        // rows [0, Hp): the gate fc1_g, rows [Hp, 2 Hp): fc1_x
    if (c.scale_mlp) ln(b + ".mlp.norm", d.Hp);
    lin(b + ".mlp.fc2", D, d.Hp);
  }
  ln("final_norm", D);                       // `norm` (token pool) or `fc_norm` (avg pool)
  lin("head", d.Cp, D);
  return t;
}

// every tensor of the table: present, of its shape, finite, and - pair engine - inside fp16's range
inline void check_tensors(const std::map<std::string, HostTensor>& host, const std::vector<TensorDesc>& table, bool pair) {
  for (const TensorDesc& d : table) {
    const auto it = host.find(d.name);
    need(it != host.end(), RTD_E_WEIGHTS, "weight blob: missing tensor " + d.name);
    need(it->second.shape == d.shape, RTD_E_WEIGHTS, "weight shape mismatch: " + d.name);
    rtd::blob::check_values(d.name, it->second, pair);
  }
}

// ---- the arena of one batch size: byte offsets of the activation buffers (4 bytes per channel in both precisions), 256-byte aligned
struct Layout {
  size_t patches = 0;   // [n G G][Kp]
  size_t pe = 0;        // [n G G][D]     patch embed
  size_t xa = 0, xb = 0;   // [n L][D]    the residual stream, ping-pong (a conv never writes over its own residual)
  size_t y = 0;         // [n L][D]       LayerNorm outputs
  size_t qkv = 0;       // [n L][3 D]
  size_t ao = 0;        // [n L][D]       attention output
  size_t h1 = 0;        // [n L][2 Hp]    fc1_g | fc1_x
  size_t h2 = 0;        // [n L][Hp]
  size_t pool = 0, pooln = 0;   // [n][D]
  size_t logits = 0;    // [n][Cp] fp32
  size_t top = 0;       // bytes in all (the conv kernels' workspace goes behind it)
};
inline Layout layout(const rtd_eva_config& c, int n) {
  need(n >= 1 && n <= MAX_BATCH, RTD_E_INVALID, "1..64 images per call");
  const Dims d = dims(c);
  Layout a;
  size_t top = 256;   // (not 0: a plan holds its tensors as offsets, and the conv launcher's shape probe reads offset 0 as a null tensor)
  auto take = [&](size_t rows, size_t ch) {
    const size_t off = top;
    top += (rows * ch * 4 + 255) / 256 * 256;
    return off;
  };
  const size_t np = (size_t)n * d.G * d.G, nl = (size_t)n * d.L;
  a.patches = take(np, d.Kp);
  a.pe = take(np, c.dim);
  a.xa = take(nl, c.dim);
  a.xb = take(nl, c.dim);
  a.y = take(nl, c.dim);
  a.qkv = take(nl, 3 * (size_t)c.dim);
  a.ao = take(nl, c.dim);
  a.h1 = take(nl, 2 * (size_t)d.Hp);
  a.h2 = take(nl, d.Hp);
  a.pool = take(n, c.dim);
  a.pooln = take(n, c.dim);
  a.logits = take(n, d.Cp);
  a.top = top;
  return a;
}

}  // namespace eva_host
