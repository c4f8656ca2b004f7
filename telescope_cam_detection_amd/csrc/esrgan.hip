// esrgan.hip - Real-ESRGAN x4 upscaling of Stage-2 crops on device-resident frames: the reference's ImageEnhancer method "realesrgan"
// (src/image_enhancement.py), i.e. RealESRGANer.enhance(outscale 4) around RRDBNet(3, 3, 64, B, 32, scale 4).  The arithmetic is restated
// in tests/esrgan_ref.py.
//
// The network is 15 B + 6 3x3 convolutions and nothing else; all of them run through launch_conv (conv_igemm.hip) in the handle's
// precision, the fp16 hi + lo pair format (RTD_PREC_F16X3) or fp32.  Per padded-tile shape (h, w) the handle caches a plan: an op list
// over one arena.
//   in    [h, w, 32]     the tile's RGB / 255 in channels 0..2, zeros above (the pair format stores whole 32-channel groups; conv_first's
//                        filter is zero-padded to match)
//   feat  [h, w, 64]     conv_first's output, kept for `feat + conv_body(body(feat))`
//   d0..2 [h, w, 192]    dense-block buffers.  A block's input is channels 0..63 of one of them; convK (K = 1..4) reads the prefix view
//                        [0, 64 + 32 (K - 1)) and writes its 32 channels behind it (LeakyReLU epilogue); conv5 reads all 192 and writes
//                        channels 0..63 of the NEXT buffer with the block input as residual - its filter and bias carry the block's 0.2.
//                        An RRDB goes d0 -> d1 -> d2 -> d1, so its own input is still in d0 for the tail d0 = 0.2 * d1 + d0
//                        (launch_axpby, ops.hip).
//   u1, c1 [2h, 2w, 64]; u2, c2 [4h, 4w, 64]   launch_upsample2x, then the conv; conv_hr writes u2 again and conv_last (N padded to 32,
//                        fp32 rows out) writes over c2.
// esrgan_ingest fills `in` from the tile's rectangle of the uint8 BGR frame, esrgan_emit clamps, rounds and writes the tile's core (x4)
// into the crop's output image.  Everything is enqueued on the caller's stream; the handle owns no stream and never captures one.
#include <math.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <new>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "esrgan_host.h"
#include "net_plan.h"

namespace esrgan {

using namespace rtd;
namespace eh = esrgan_host;
namespace bk = rtd::backend;
namespace np = rtd::netplan;
using bk::guarded;
using np::at;
using np::based;

constexpr int IN_C = 32, FEAT = 64, GROW = 32, DENSE_C = 192, LAST_C = 32;

// ---------------------------------------------------------------------------------------------------------------- kernels
// one thread per pixel of the padded tile: BGR bytes -> RGB, float32(v) / 255 (a true fp32 division, as numpy's), channels 3..31 zero
template <bool PAIR>
__global__ void __launch_bounds__(256) esrgan_ingest(const uint8_t* __restrict__ src, int pitch, int h, int w, void* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const uint8_t* p = src + (size_t)y * pitch + (size_t)x * 3;
  const float rgb[3] = {(float)p[2] / 255.f, (float)p[1] / 255.f, (float)p[0] / 255.f};
  if (PAIR) {
    sp16* q = (sp16*)dst + (size_t)i * (2 * IN_C);
    sp16x8 hi = {0, 0, 0, 0, 0, 0, 0, 0}, lo = hi;
    const sp16x8 zero = hi;
#pragma unroll
    for (int c = 0; c < 3; ++c) { sp16 a, b; split2(rgb[c], a, b); hi[c] = a; lo[c] = b; }
    *(sp16x8*)q = hi;
    *(sp16x8*)(q + SPLIT_GROUP) = lo;
#pragma unroll
    for (int k = 1; k < 4; ++k) { *(sp16x8*)(q + 8 * k) = zero; *(sp16x8*)(q + SPLIT_GROUP + 8 * k) = zero; }
  } else {
    float* q = (float*)dst + (size_t)i * IN_C;
    *(f32x4*)q = f32x4{rgb[0], rgb[1], rgb[2], 0.f};
#pragma unroll
    for (int k = 1; k < IN_C / 4; ++k) *(f32x4*)(q + 4 * k) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// one thread per pixel of the core's x4 image: conv_last's fp32 rows (RGB in channels 0..2) -> clamp(0, 1), rint(x * 255) (half to
// even, as numpy rounds), RGB -> BGR, into the crop's output image
struct EmitArgs {
  const float* last;   // [4 th][4 tw][LAST_C]
  int tw4;             // 4 * tile input width
  int ox, oy;          // the core's first pixel inside the tile's x4 image
  int cw4, ch4;        // the core's x4 extent
  uint8_t* out;        // the crop's output image, at the core's first pixel
  int out_pitch;       // bytes per output row (4 W * 3)
};
__global__ void __launch_bounds__(256) esrgan_emit(EmitArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.cw4 * a.ch4) return;
  const int y = i / a.cw4, x = i - y * a.cw4;
  const f32x4 v = *(const f32x4*)(a.last + ((size_t)(a.oy + y) * a.tw4 + (a.ox + x)) * LAST_C);
  uint8_t* q = a.out + (size_t)y * a.out_pitch + (size_t)x * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) q[2 - c] = (uint8_t)rintf(fminf(fmaxf(v[c], 0.f), 1.f) * 255.f);
}

// ---------------------------------------------------------------------------------------------------------------- plan
enum OpKind { OP_CONV, OP_UPSAMPLE, OP_AXPBY, OP_COPY };
// (tensors of an op are arena offsets: net_plan.h)
struct Op {
  int kind = OP_CONV;
  ConvArgs conv;          // OP_CONV (x, y, res as offsets)
  Tensor a, b, y;         // OP_UPSAMPLE: a -> y; OP_AXPBY: y = 0.2 a + b; OP_COPY: a -> y
  std::string stage;      // the debug name of the tensor this op completes ("" = none)
  Tensor stage_t;
};
struct Plan : np::PlanBase {
  int h = 0, w = 0;
  Tensor in, last;
  std::vector<Op> ops;
};

}  // namespace esrgan

struct rtd_esrgan : rtd::netplan::NetBase {
  rtd_esrgan_config cfg;
  std::vector<char> blob;
  std::map<std::pair<int, int>, std::unique_ptr<esrgan::Plan>> plans;
  // the last tile of the last call (rtd_debug_esrgan_tensor re-runs it up to the stage asked for)
  const uint8_t* last_src = nullptr;
  int last_pitch = 0;
  esrgan::Plan* last_plan = nullptr;
};

namespace esrgan {

static std::unique_ptr<Plan> build_plan(rtd_esrgan* e, int h, int w) {
  auto p = std::make_unique<Plan>();
  p->h = h, p->w = w;
  const int P = e->P, B = e->cfg.num_block;
  np::Arena arena;
  auto alloc = [&](int hh, int ww, int c, int dt) { return arena.tensor(dt, 1, hh, ww, c); };
  const Tensor in = alloc(h, w, IN_C, P), feat = alloc(h, w, FEAT, P);
  const Tensor d[3] = {alloc(h, w, DENSE_C, P), alloc(h, w, DENSE_C, P), alloc(h, w, DENSE_C, P)};
  const Tensor u1 = alloc(2 * h, 2 * w, FEAT, P), c1 = alloc(2 * h, 2 * w, FEAT, P);
  const Tensor u2 = alloc(4 * h, 4 * w, FEAT, P), c2 = alloc(4 * h, 4 * w, FEAT, P);
  Tensor last = at((size_t)c2.p, F32, 1, 4 * h, 4 * w, LAST_C);
  p->in = in, p->last = last;

  size_t slab = 0;
  auto conv = [&](const std::string& name, const Tensor& x, const Tensor& y, int act, const Tensor* res, const std::string& stage) {
    Op op;
    op.kind = OP_CONV;
    ConvArgs& a = op.conv;
    a = conv_args(x, y, e->filters.at(name), 3, 1, 1, act);
    np::plan_conv(a, &e->conv_opts, res, RES_PRE, slab, name);
    op.stage = stage; op.stage_t = y;
    p->ops.push_back(op);
  };
  auto body = [](int i) { return "body." + std::to_string(i); };

  conv("conv_first", in, feat, ACT_NONE, nullptr, "");
  { Op op; op.kind = OP_COPY; op.a = feat; op.y = d[0].slice_c(0, FEAT); op.stage = "first"; op.stage_t = op.y; p->ops.push_back(op); }
  for (int i = 0; i < B; ++i) {
    const int order[4] = {0, 1, 2, 1};                         // the RRDB's blocks go d0 -> d1 -> d2 -> d1
    for (int j = 0; j < 3; ++j) {
      const Tensor& cur = d[order[j]];
      const Tensor& nxt = d[order[j + 1]];
      const std::string pfx = body(i) + ".rdb" + std::to_string(j + 1);
      for (int k = 1; k <= 4; ++k)
        conv(pfx + ".conv" + std::to_string(k), cur.slice_c(0, FEAT + GROW * (k - 1)), cur.slice_c(FEAT + GROW * (k - 1), GROW), ACT_LRELU, nullptr, "");
      const Tensor block_in = cur.slice_c(0, FEAT);
      conv(pfx + ".conv5", cur, nxt.slice_c(0, FEAT), ACT_NONE, &block_in, pfx);
    }
    Op op;
    op.kind = OP_AXPBY; op.a = d[1].slice_c(0, FEAT); op.b = d[0].slice_c(0, FEAT); op.y = op.b; op.stage = body(i); op.stage_t = op.y;
    p->ops.push_back(op);
  }
  const Tensor trunk = d[1].slice_c(0, FEAT);
  conv("conv_body", d[0].slice_c(0, FEAT), trunk, ACT_NONE, &feat, "trunk");
  { Op op; op.kind = OP_UPSAMPLE; op.a = trunk; op.y = u1; p->ops.push_back(op); }
  conv("conv_up1", u1, c1, ACT_LRELU, nullptr, "up1");
  { Op op; op.kind = OP_UPSAMPLE; op.a = c1; op.y = u2; p->ops.push_back(op); }
  conv("conv_up2", u2, c2, ACT_LRELU, nullptr, "up2");
  conv("conv_hr", c2, u2, ACT_LRELU, nullptr, "hr");
  conv("conv_last", u2, last, ACT_NONE, nullptr, "last");

  p->seal(arena.top, slab);
  return p;
}

static void run_op(rtd_esrgan* e, const Plan* p, const Op& op, hipStream_t s) {
  char* base = (char*)e->arena.p;
  switch (op.kind) {
    case OP_CONV: np::run_conv(op.conv, base, *p, s); break;
    case OP_UPSAMPLE: launch_upsample2x(based(op.a, base), based(op.y, base), s); break;
    case OP_AXPBY: launch_axpby(0.2f, based(op.a, base), based(op.b, base), based(op.y, base), s); break;
    default: {
      const Tensor a = based(op.a, base), y = based(op.y, base);
      HIP_CHECK(hipMemcpy2DAsync(y.p, (size_t)y.ld * 4, a.p, (size_t)a.ld * 4, (size_t)a.c * 4, (size_t)a.pixels(), hipMemcpyDeviceToDevice, s));
    }
  }
}

static void run_ingest(rtd_esrgan* e, const Plan* p, const uint8_t* src, int pitch, hipStream_t s) {
  const unsigned blocks = (unsigned)(((int64_t)p->h * p->w + 255) / 256);
  void* dst = e->arena.p + (size_t)p->in.p;
  if (e->P == F16X2) rtd_launch(esrgan_ingest<true>, dim3(blocks), dim3(256), 0, s, src, pitch, p->h, p->w, dst);
  else rtd_launch(esrgan_ingest<false>, dim3(blocks), dim3(256), 0, s, src, pitch, p->h, p->w, dst);
  HIP_CHECK(hipGetLastError());
}

static void run(rtd_esrgan* e, int n, const uint8_t* const* frames, const int32_t* frame_hw, const int32_t* rects, uint8_t* out, int64_t out_cap,
                hipStream_t s) {
  // ---- every argument is checked before anything is allocated or launched
  static_assert(eh::MAX_CROPS == bk::MAX_CROPS, "the shared argument check and the layout agree on the crops per call");
  bk::check_crop_call(n, frames, frame_hw, rects, out);
  int64_t offsets[eh::MAX_CROPS + 1];
  eh::layout(n, rects, offsets);
  const int tile = e->cfg.tile, pad = e->cfg.tile_pad;
  for (int i = 0; i < n; ++i) {
    bk::check_crop_frame(i, frames, frame_hw, rects);
    if (tile == 0)
      RTD_CHECK(rects[4 * i + 2] - rects[4 * i] <= eh::MAX_ONE_PASS_SIDE && rects[4 * i + 3] - rects[4 * i + 1] <= eh::MAX_ONE_PASS_SIDE, RTD_E_INVALID,
                "crop " + std::to_string(i) + ": without tiling (tile = 0) a crop side is at most 576 pixels");
  }
  RTD_CHECK(out_cap >= offsets[n], RTD_E_INVALID, "out_cap is smaller than rtd_esrgan_layout's total (" + std::to_string(offsets[n]) + " bytes)");

  HIP_CHECK(hipSetDevice(e->device));
  // ---- the plans of every tile shape of the call, and one arena that holds the largest
  struct Job { Plan* plan; eh::TileRect t; int crop; };
  std::vector<Job> jobs;
  size_t need = 0;
  e->last_plan = nullptr;
  // (the cache is trimmed here and not while the jobs are collected: they hold pointers to its plans)
  if (e->plans.size() > 256) e->plans.clear();
  for (int i = 0; i < n; ++i) {
    const int W = rects[4 * i + 2] - rects[4 * i], H = rects[4 * i + 3] - rects[4 * i + 1];
    for (const eh::TileRect& t : eh::tile_rects(H, W, tile, pad)) {
      const int h = t.iy1 - t.iy0, w = t.ix1 - t.ix0;
      Plan* p = np::get_or_build(e->plans, std::make_pair(h, w), (size_t)-1, [&] { return build_plan(e, h, w); });
      need = std::max(need, p->bytes);
      jobs.push_back(Job{p, t, i});
    }
  }
  e->arena.reserve(need);
  for (const Job& j : jobs) {
    const int i = j.crop;
    const int x1 = rects[4 * i], y1 = rects[4 * i + 1], W = rects[4 * i + 2] - x1, fw = frame_hw[2 * i + 1];
    const eh::TileRect& t = j.t;
    const int pitch = fw * 3;
    const uint8_t* src = frames[i] + ((size_t)(y1 + t.iy0) * fw + (x1 + t.ix0)) * 3;
    run_ingest(e, j.plan, src, pitch, s);
    for (const Op& op : j.plan->ops) run_op(e, j.plan, op, s);
    EmitArgs a;
    a.last = (const float*)(e->arena.p + (size_t)j.plan->last.p);
    a.tw4 = 4 * j.plan->w;
    a.ox = 4 * (t.cx0 - t.ix0), a.oy = 4 * (t.cy0 - t.iy0);
    a.cw4 = 4 * (t.cx1 - t.cx0), a.ch4 = 4 * (t.cy1 - t.cy0);
    a.out_pitch = 4 * W * 3;
    a.out = out + offsets[i] + (size_t)(4 * t.cy0) * a.out_pitch + (size_t)(4 * t.cx0) * 3;
    rtd_launch(esrgan_emit, dim3((unsigned)(((int64_t)a.cw4 * a.ch4 + 255) / 256)), dim3(256), 0, s, a);
    HIP_CHECK(hipGetLastError());
    e->last_src = src, e->last_pitch = pitch, e->last_plan = j.plan, e->last_stream = s;
  }
}

// The filters (net_plan.h: upload_filters): OIHW -> tap-major rows, conv_first's 3 input channels padded to the `in` tensor's 32 and
// conv_last's 3 outputs to 32 rows; `x5 * 0.2 + x`: the 0.2 lives in conv5's filter and bias
static void upload_weights(rtd_esrgan* e, const std::map<std::string, eh::HostTensor>& host, const std::vector<eh::ConvDesc>& table) {
  std::vector<np::FilterSpec> specs;
  for (const eh::ConvDesc& d : table) specs.push_back({d.name, conv_filter_extents(e->P, d.cout == 3 ? LAST_C : d.cout, 9 * (d.cin == 3 ? IN_C : d.cin))});
  np::upload_filters(*e, specs, [&](size_t i, std::vector<float>& rows, std::vector<float>& bias) {
    const eh::ConvDesc& d = table[i];
    const ConvFilter& f = specs[i].f;
    const bool conv5 = d.name.size() > 6 && d.name.compare(d.name.size() - 6, 6, ".conv5") == 0;
    const float scale = conv5 ? 0.2f : 1.f;
    rows = eh::filter_rows(host.at(d.name + ".weight"), d.cout, d.cin, d.cin == 3 ? IN_C : d.cin, f.Npad, f.kcols(), scale);
    const eh::HostTensor& b = host.at(d.name + ".bias");
    for (int o = 0; o < d.cout; ++o) bias[o] = b.data[o] * scale;
  });
}

}  // namespace esrgan

using namespace esrgan;

extern "C" {

int rtd_esrgan_create(const rtd_esrgan_config* cfg, const void* blob, size_t nbytes, rtd_esrgan_handle* out) {
  return bk::create(out, rtd_esrgan_destroy, [&](rtd_esrgan* e) {
    eh::check_config(cfg);
    e->cfg = *cfg;
    e->P = cfg->precision == RTD_PREC_FP32 ? F32 : F16X2;
    eh::need(blob && nbytes >= 12, RTD_E_WEIGHTS, "empty weight blob");
    e->blob.assign((const char*)blob, (const char*)blob + nbytes);
    std::map<std::string, eh::HostTensor> host;
    eh::parse_blob(e->blob.data(), e->blob.size(), host);
    const std::vector<eh::ConvDesc> table = eh::conv_table(cfg->num_block);
    for (const eh::ConvDesc& d : table) eh::check_conv_tensors(host, d, e->P == F16X2);   // the whole blob is checked before the device is touched
    bk::use_device(cfg->device);
    e->device = cfg->device;
    e->conv_opts = conv_opts_template();
    upload_weights(e, host, table);
    e->blob.clear();
    e->blob.shrink_to_fit();
  });
}

int rtd_esrgan_layout(int32_t n, const int32_t* rects, int64_t* offsets) {
  return bk::caught(bk::create_error<rtd_esrgan>(), [&] { eh::layout(n, rects, offsets); });
}

int rtd_esrgan_upscale(rtd_esrgan_handle e, int32_t n, const uint8_t* const* frames_dev, const int32_t* frame_hw, const int32_t* rects,
                       uint8_t* out_dev, int64_t out_cap, void* stream) {
  return guarded(e, [&] { run(e, n, frames_dev, frame_hw, rects, out_dev, out_cap, (hipStream_t)stream); });
}

int64_t rtd_esrgan_arena_bytes(rtd_esrgan_handle e) { return e ? e->arena_bytes() : 0; }

const char* rtd_esrgan_last_error(rtd_esrgan_handle e) { return bk::last_error(e); }

void rtd_esrgan_destroy(rtd_esrgan_handle e) {
  if (!e) return;
  e->release_device();
  delete e;
}

int rtd_debug_esrgan_tensor(rtd_esrgan_handle e, const char* name, float* out, int64_t capacity, int64_t shape[4]) {
  return guarded(e, [&] {
    RTD_CHECK(name && shape, RTD_E_INVALID, "null argument");
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_esrgan_upscale call yet");
    const Plan* p = e->last_plan;
    // the plan's buffers are reused along the network: the last tile is run again up to the stage asked for
    size_t upto = 0;
    Tensor t = p->in;
    if (strcmp(name, "ingest") != 0) {
      bool found = false;
      for (size_t i = 0; i < p->ops.size() && !found; ++i)
        if (p->ops[i].stage == name) { found = true; upto = i + 1; t = p->ops[i].stage_t; }
      RTD_CHECK(found, RTD_E_INVALID, std::string("unknown debug tensor ") + name);
    }
    shape[0] = 1, shape[1] = t.h, shape[2] = t.w, shape[3] = t.c;
    const int64_t numel = t.pixels() * t.c;
    if (!out) return;
    RTD_CHECK(capacity >= numel, RTD_E_INVALID, "debug tensor: output capacity too small");
    HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = e->last_stream;
    run_ingest(e, p, e->last_src, e->last_pitch, s);
    for (size_t i = 0; i < upto; ++i) run_op(e, p, p->ops[i], s);
    np::read_tensor(based(t, (char*)e->arena.p), t.pixels(), out, s);
  });
}

int rtd_debug_esrgan_plan_convs(rtd_esrgan_handle e, char* out, int64_t capacity, int64_t* needed) {
  return guarded(e, [&] {
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_esrgan_upscale call yet");
    std::vector<std::string> names;      // (build_plan's convs follow the table's order)
    for (const eh::ConvDesc& d : eh::conv_table(e->cfg.num_block)) names.push_back(d.name);
    np::text_out(np::plan_convs_text(*e->last_plan, OP_CONV, names), out, capacity, needed);
  });
}

}  // extern "C"
