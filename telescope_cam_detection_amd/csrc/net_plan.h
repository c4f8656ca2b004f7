// net_plan.h - what the back ends that run a whole network on launch_conv share (esrgan.hip, classifier.hip, yolox_net.hip): tensors held
// as byte offsets into one arena, the bump allocator that hands them out, a conv op's construction and launch, the handle's device
// memory, the filter upload and the read-back of a debug tensor.  A back end keeps its own Op struct and op kinds, its network walk, its
// `run` and its stage bookkeeping: nothing here interprets an op list.  Host only.
#pragma once
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "backend.h"

namespace rtd {
namespace netplan {

// ---- tensors of a plan hold their byte OFFSET inside the arena in `p`; a run adds the arena's base (the arena may be replaced by a
// larger one between calls, the plans stay)
inline Tensor at(size_t off, int dt, int n, int h, int w, int c) {
  Tensor t;
  t.p = (void*)off; t.dt = dt; t.n = n; t.h = h; t.w = w; t.c = c; t.ld = c; t.bstride = (int64_t)h * w * c;
  return t;
}
inline Tensor based(Tensor t, char* base) {
  t.p = base + (size_t)t.p;
  return t;
}
inline ConvArgs based(ConvArgs a, char* base) {
  a.x = based(a.x, base), a.y = based(a.y, base);
  if (a.res_mode != RES_NONE) a.res = based(a.res, base);
  return a;
}

// a bump allocator over arena offsets, every piece on a 256-byte boundary
struct Arena {
  size_t top = 0;
  static size_t room(int n, int h, int w, int c) { return backend::align_up((size_t)n * h * w * c * 4, 256); }   // (pair tensors take 4 bytes per channel too)
  size_t take(size_t bytes) {
    const size_t off = top;
    top += backend::align_up(bytes, 256);
    return off;
  }
  Tensor tensor(int dt, int n, int h, int w, int c) { return at(take(room(n, h, w, c)), dt, n, h, w, c); }
};

struct PlanBase {
  size_t bytes = 0;       // arena bytes, the split-K workspace included
  size_t slab_off = 0, slab_bytes = 0;
  void seal(size_t top, size_t slab) {   // the workspace goes behind the tensors
    slab_off = top;
    slab_bytes = slab;
    bytes = top + backend::align_up(slab, 256);
  }
};

// An OP_CONV while the plan is built: the handle's options and the residual, then the launcher's own checks and the workspace it would
// ask for - on addresses as aligned as the arena's (offset 0 would read as a null pointer).  A shape the launcher refuses is a refused
// call before anything is launched.
inline void plan_conv(ConvArgs& a, const ConvOpts* opts, const Tensor* res, int res_mode, size_t& slab, const std::string& label) {
  a.opts = opts;
  if (res) { a.res = *res; a.res_mode = res_mode; }
  const ConvArgs probe = based(a, (char*)(uintptr_t)4096);
  try {
    (void)conv_predict(probe, nullptr);
  } catch (const Error& er) {
    throw Error(RTD_E_INVALID, label + ": " + er.what());
  }
  slab = std::max(slab, conv_split_slab_bytes(probe));
}
inline void run_conv(const ConvArgs& planned, char* base, const PlanBase& p, hipStream_t s) {
  ConvArgs a = based(planned, base);
  if (p.slab_bytes) { a.ws.slab = (float*)(base + p.slab_off); a.ws.slab_bytes = p.slab_bytes; }
  launch_conv(a, s);
}

// the plan of `key`, built on its first use.  A plan is a host-side op list, cheap to rebuild: a cache that has grown past `cap` is
// emptied first, so the caller drops its pointers into the cache (last_plan) before it asks.  The cap bites for YOLOX alone (64 input
// shapes): EVA's key is a batch size of at most 64, and ESRGAN passes no cap and trims before a call collects its tiles, which hold
// plan pointers across lookups.
template <typename K, typename P, typename B>
P* get_or_build(std::map<K, std::unique_ptr<P>>& plans, const K& key, size_t cap, B&& build) {
  const auto it = plans.find(key);
  if (it != plans.end()) return it->second.get();
  if (plans.size() > cap) plans.clear();
  return (plans[key] = build()).get();
}

// ---- the handle: the device memory of a network back end
struct NetBase : backend::Base {
  int P = F16X2;
  std::map<std::string, ConvFilter> filters;
  std::vector<void*> allocs;
  backend::DevBuf arena;   // holds the largest plan seen (a repeated shape allocates nothing)
  ConvOpts conv_opts;
  hipStream_t last_stream = nullptr;

  char* dmalloc(size_t bytes) {
    void* q = nullptr;
    HIP_CHECK(hipMalloc(&q, bytes ? bytes : 256));
    allocs.push_back(q);
    return (char*)q;
  }
  void release_device() {
    (void)hipSetDevice(device);
    arena.release();                              // (hipFree waits for the device: nothing enqueued still uses the arena or the filters)
    for (void* q : allocs) (void)hipFree(q);
    allocs.clear();
    (void)hipGetLastError();
  }
  int64_t arena_bytes() {
    std::lock_guard<std::mutex> lk(mu);
    return (int64_t)arena.cap;
  }
};

// Filters and biases through the upload path of the handle's precision: fill(i, rows, bias) assigns filter i's zero-padded fp32 rows
// [Npad][kcols] (rows arrives empty) and writes its bias [Npad] (arrives zeroed), one filter at a time - the whole network's rows are never held at once - then
// host -> device and conv_filter_convert (common.h).  Two pools (filters, biases) and, on the pair engine, one staging pool that is
// freed when every conversion has run: three allocations and one wait for the whole network.
struct FilterSpec {
  std::string name;
  ConvFilter f;   // conv_filter_extents of it
};
template <typename Fill>
void upload_filters(NetBase& e, const std::vector<FilterSpec>& specs, Fill&& fill) {
  std::vector<size_t> w_off;
  size_t w_bytes = 0, b_bytes = 0;
  for (const FilterSpec& sp : specs) {
    w_off.push_back(w_bytes);
    w_bytes += backend::align_up(std::max(sp.f.bytes(), (size_t)sp.f.Npad * sp.f.kcols() * 4), 256);   // (the fp32 rows are staged at the same offsets)
    b_bytes += (size_t)sp.f.Npad * 4;
  }
  char* wpool = e.dmalloc(w_bytes);
  char* bpool = e.dmalloc(b_bytes);
  backend::OpScratch staging;
  char* stage = e.P == F16X2 ? staging.get<char>(w_bytes) : wpool;
  size_t b_off = 0;
  std::vector<float> rows, bias;
  for (size_t i = 0; i < specs.size(); ++i) {
    ConvFilter f = specs[i].f;
    rows.clear();
    bias.assign(f.Npad, 0.f);
    fill(i, rows, bias);
    RTD_CHECK(rows.size() == (size_t)f.Npad * f.kcols() && bias.size() == (size_t)f.Npad, RTD_E_STATE, "upload: filter rows of the wrong extent: " + specs[i].name);
    f.bias = (float*)(bpool + b_off);
    f.w = wpool + w_off[i];
    float* dev_rows = (float*)(stage + w_off[i]);
    HIP_CHECK(hipMemcpy(f.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dev_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    conv_filter_convert(f, dev_rows, nullptr);
    e.filters[specs[i].name] = f;
    b_off += (size_t)f.Npad * 4;
  }
  HIP_CHECK(hipDeviceSynchronize());
}

// the tail of a debug read: `rows` rows of t.c channels (t based, its pixel stride t.ld) -> dense fp32 on the host; returns when done
inline void read_tensor(const Tensor& t, int64_t rows, float* out, hipStream_t s) {
  const int64_t numel = rows * t.c;
  backend::OpScratch sc;
  float* f32 = sc.get<float>((size_t)numel);
  if (t.dt == F16X2) launch_split_to_f32(t.p, t.ld, f32, t.c, rows, t.c, s);
  else HIP_CHECK(hipMemcpy2DAsync(f32, (size_t)t.c * 4, t.p, (size_t)t.ld * 4, (size_t)t.c * 4, (size_t)rows, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(out, f32, (size_t)numel * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// ---- tests only (rtd_debug_yolox_plan_convs, rtd_debug_eva_plan_convs, rtd_debug_esrgan_plan_convs): the conv launches of a plan in
// execution order, one text line each -
//   name dtype B H W Cin Cout k stride pad act res_mode out_f32 ldx ldy ldres key S grid
// geometry, pixel strides and epilogue as the plan's ConvArgs hold them (H, W: the input's; out_f32: fp32 rows out of other operands;
// ldres 0 without a residual), key / S / grid from conv_predict on the probe addresses plan_conv used - the function
// rtd_debug_conv_choice_views answers from.  names: one per OP_CONV in order, or empty (the line's name is then the launch's index).
template <typename Plan>
std::string plan_convs_text(const Plan& p, int conv_kind, const std::vector<std::string>& names) {
  std::string out;
  size_t i = 0;
  for (const auto& op : p.ops) {
    if (op.kind != conv_kind) continue;
    const ConvArgs& a = op.conv;
    RTD_CHECK(names.empty() || i < names.size(), RTD_E_STATE, "plan convs: the plan has more convs than its table has names");
    const ConvChoiceReport r = conv_predict(based(a, (char*)(uintptr_t)4096), nullptr);
    const int v[15] = {a.x.dt, a.x.n, a.x.h, a.x.w, a.x.c, a.y.c, a.KH, a.stride, a.pad, a.act, a.res_mode, a.y.dt == F32 && a.x.dt != F32,
                       (int)a.x.ld, (int)a.y.ld, a.res_mode != RES_NONE ? (int)a.res.ld : 0};
    out += names.empty() ? std::to_string(i) : names[i];
    for (int k = 0; k < 15; ++k) out += " " + std::to_string(v[k]);
    out += std::string(" ") + r.key + " " + std::to_string(r.S) + " " + std::to_string(r.grid) + "\n";
    ++i;
  }
  RTD_CHECK(names.empty() || i == names.size(), RTD_E_STATE, "plan convs: the table has names the plan did not use");
  return out;
}
// the size-then-fill convention of rtd_debug_conv_instantiations
inline void text_out(const std::string& text, char* out, int64_t capacity, int64_t* needed) {
  if (needed) *needed = (int64_t)text.size() + 1;
  if (!out) return;
  RTD_CHECK(capacity > (int64_t)text.size(), RTD_E_INVALID, "text output: buffer too small");
  memcpy(out, text.c_str(), text.size() + 1);
}

// the kernel-level test entry points' guard: the message goes where rtd_X_last_error(NULL) of handle type H reads it, and the call
// returns when the device is done
template <typename H, typename F>
int op_guard(F&& f) {
  return backend::caught(backend::create_error<H>(), [&] { f(); HIP_CHECK(hipDeviceSynchronize()); });
}
inline int op_dtype(int dtype) {
  RTD_CHECK(dtype == F32 || dtype == F16X2, RTD_E_INVALID, "dtype must be 1 (fp32) or 4 (F16X2)");
  return dtype;
}

}  // namespace netplan
}  // namespace rtd
