// testapi.hip - kernel-level test, bench and debug entry points of libmi355rtdetr.so (include/rtdetr_mi355_test.h).
// Nothing here is on the detection path: tests/ , tools/ and bench.py's diagnostic legs are the only callers.
#include "engine_internal.h"

using namespace rtd;
using namespace rtd_eng;

using backend::OpScratch;   // device buffers, events and streams of one call here: released on every path, a throw included
static bool rows_fit_int(int a, int b) { return a >= 1 && b >= 1 && (int64_t)a * b <= 0x7fffffff; }
static Tensor rows_view(const void* p, int dt, int n, int rows, int c, int64_t ld) {
  Tensor t = mk(p, dt, n, rows, 1, c);
  t.ld = ld; t.bstride = (int64_t)rows * ld;
  return t;
}

extern "C" {

int rtd_debug_tensor(rtd_handle h, const char* name, float* out, int64_t capacity, int64_t shape[4]) {
  return guarded(h, [&] {
    RTD_CHECK(name && shape && h->last_n > 0, RTD_E_STATE, "no forward has run");
    Plan* p = h->plans[h->last_n].get();
    auto it = p->named.find(name);
    RTD_CHECK(it != p->named.end(), RTD_E_INVALID, std::string("unknown debug tensor ") + name);
    const Tensor& t = it->second;
    if (p->stem_fused && strcmp(name, "input") == 0 && out) {      // the fused stem never wrote it: run the stand-alone preprocess now
      HIP_CHECK(hipSetDevice(h->cfg.device));
      launch_preprocess_identity(h->last_fa, h->cfg.input_h, h->cfg.input_w, p->input, p->scale_wh, h->q.stream);
    }
    shape[0] = t.n; shape[1] = t.h; shape[2] = t.w; shape[3] = t.c;
    const int64_t numel = t.pixels() * t.c;
    if (!out) return;
    RTD_CHECK(capacity >= numel, RTD_E_INVALID, "debug tensor: output capacity too small");
    RTD_CHECK(t.bstride == (int64_t)t.h * t.w * t.ld, RTD_E_INVALID, "debug tensor: non-dense batch stride");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t es = dtype_size(t.dt);
    if (t.dt == I32) {                                             // index tensors: exact as fp32 (token ids < 2^24)
      std::vector<int32_t> tmp((size_t)numel);
      HIP_CHECK(hipStreamSynchronize(h->q.stream));
      HIP_CHECK(hipMemcpy(tmp.data(), t.p, (size_t)numel * 4, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < numel; ++i) out[i] = (float)tmp[(size_t)i];
      return;
    }
    if (t.dt == F16X2) RTD_CHECK(t.c % SPLIT_GROUP == 0, RTD_E_INVALID, "debug tensor: split tensor with a partial channel group");
    OpScratch sc;
    void* dense = sc.get<char>((size_t)numel * es);
    float* f32 = sc.get<float>((size_t)numel);
    HIP_CHECK(hipMemcpy2DAsync(dense, (size_t)t.c * es, t.p, (size_t)t.ld * es, (size_t)t.c * es, (size_t)t.pixels(), hipMemcpyDeviceToDevice, h->q.stream));
    if (t.dt == F16X2) launch_split_to_f32(dense, t.c, f32, t.c, t.pixels(), t.c, h->q.stream);
    else launch_to_f32(dense, t.dt, f32, numel, h->q.stream);
    HIP_CHECK(hipMemcpyAsync(out, f32, (size_t)numel * 4, hipMemcpyDeviceToHost, h->q.stream));
    HIP_CHECK(hipStreamSynchronize(h->q.stream));
  });
}

int rtd_debug_force_topk(rtd_handle h, const int32_t* idx, int32_t n) {
  return guarded(h, [&] {
    RTD_CHECK(h->loaded, RTD_E_STATE, "weights not loaded");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    if (idx && !h->force_used) {
      // first use on this handle: the override launch joins the plans; graphs built without it are rebuilt on their next run
      h->force_used = true;
      HIP_CHECK(hipStreamSynchronize(h->q.stream));
      for (auto& kv : h->plans) {
        if (kv.second->exec) { (void)hipGraphExecDestroy(kv.second->exec); kv.second->exec = nullptr; }
        if (kv.second->graph) { (void)hipGraphDestroy(kv.second->graph); kv.second->graph = nullptr; }
      }
    }
    int32_t flag = 0;
    if (idx) {
      RTD_CHECK(n >= 1 && n <= h->cfg.max_batch, RTD_E_INVALID, "batch size");
      for (int64_t i = 0; i < (int64_t)n * h->cfg.num_queries; ++i)
        RTD_CHECK(idx[i] >= 0 && idx[i] < h->S, RTD_E_INVALID, "forced token index out of range");
      HIP_CHECK(hipMemcpyAsync(h->forced_idx, idx, (size_t)n * h->cfg.num_queries * 4, hipMemcpyHostToDevice, h->q.stream));
      flag = 1;
    }
    HIP_CHECK(hipMemcpyAsync(h->force_flag, &flag, 4, hipMemcpyHostToDevice, h->q.stream));
    HIP_CHECK(hipStreamSynchronize(h->q.stream));
  });
}

static int g_profile_twice = 0;
int rtd_profile(rtd_handle h, int32_t n, int32_t reps, rtd_layer_time* out, int32_t capacity, int32_t* count) {
  return guarded(h, [&] {
    check_n(h, n);
    RTD_CHECK(count && reps >= 1, RTD_E_INVALID, "arguments");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    Plan* p = get_plan(h, n);
    std::vector<Op*> ops;                                     // what a forward of this handle launches
    for (auto& op : p->ops)
      if (op.kind == 0 && (!op.debug_only || h->force_used)) ops.push_back(&op);     // every launch, in plan order, on the main stream (no overlap while timing)
    const int nops = (int)ops.size();
    *count = nops;
    if (!out) return;
    // the fused stem reads its frames through the device table: without a preceding forward of this batch size point it at
    // zero-filled staging frames (timings do not depend on pixel values)
    if (p->stem_fused && (h->last_n != n || h->last_fa.n != n)) point_at_blank_frames(h, p, n);
    RTD_CHECK(capacity >= nops, RTD_E_INVALID, "profile: capacity too small");
    OpScratch sc;
    std::vector<hipEvent_t> ev((size_t)nops + 1);
    for (auto& x : ev) x = sc.event();
    std::vector<double> acc(nops, 0.0);
    for (Op* op : ops) op->run(h->q.stream);   // warm-up
    for (int r = 0; r < reps; ++r) {
      if (g_profile_twice) {
        // diagnostic: every op runs twice back to back and only the SECOND run is timed (operands, filter and TLB entries
        // warm from the first) - the gap to the normal profile is what the op pays for cold operands inside the network
        OpScratch sc2;
        std::vector<hipEvent_t> ev2((size_t)nops);
        for (auto& x : ev2) x = sc2.event();
        for (int i = 0; i < nops; ++i) {
          ops[i]->run(h->q.stream);
          HIP_CHECK(hipEventRecord(ev2[i], h->q.stream));
          ops[i]->run(h->q.stream);
          HIP_CHECK(hipEventRecord(ev[i + 1], h->q.stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->q.stream));
        for (int i = 0; i < nops; ++i) {
          float ms = 0.f;
          HIP_CHECK(hipEventElapsedTime(&ms, ev2[i], ev[i + 1]));
          acc[i] += ms;
        }
        continue;
      }
      HIP_CHECK(hipEventRecord(ev[0], h->q.stream));
      for (int i = 0; i < nops; ++i) {
        ops[i]->run(h->q.stream);
        HIP_CHECK(hipEventRecord(ev[i + 1], h->q.stream));
      }
      HIP_CHECK(hipStreamSynchronize(h->q.stream));
      for (int i = 0; i < nops; ++i) {
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        acc[i] += ms;
      }
    }
    for (int i = 0; i < nops; ++i) {
      rtd_layer_time& t = out[i];
      memset(&t, 0, sizeof t);
      strncpy(t.name, ops[i]->name.c_str(), sizeof(t.name) - 1);
      strncpy(t.kernel, ops[i]->kernel, sizeof(t.kernel) - 1);
      t.ms = (float)(acc[i] / reps);
      t.flops = ops[i]->flops;
      t.bytes = ops[i]->bytes;
    }
  });
}

// ---- kernel-level test entry points ---------------------------------------------------------------
// reads one dword per 128-byte line (bench only: does a READ bring lines into the Infinity Cache?)
__global__ void k_touch_read(const unsigned* p, size_t lines, unsigned* sink) {
  unsigned acc = 0;
  for (size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x; l < lines; l += (size_t)gridDim.x * blockDim.x) acc += p[l * 32];
  if (acc == 0x12345u) *sink = acc;
}
// bench only: finite fp16 values of mixed sign, exponents 2^-5 .. 2^2, random mantissas (matrix-core power depends on the operand bits:
// zero-filled operands let the chip hold a clock that real activations do not)
__global__ void k_fill_rand16(uint16_t* p, size_t n, unsigned seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = (uint16_t)((h & 0x8000u) | ((10u + ((h >> 16) & 7u)) << 10) | (h & 0x3ffu));
  }
}
// rtd_bench_mfma_rate: 16 independent accumulators per wave, 4 waves per CU (one per SIMD), operands in registers
__global__ __launch_bounds__(256) void k_mfma_rate(const unsigned* __restrict__ seed, int iters, long long* __restrict__ out, float* __restrict__ sink) {
  const int tid = threadIdx.x, lane = tid & 63;
  sp16x8 a[4], b[4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) {
      const unsigned h = seed[(lane * 8 + j + i * 512) & 4095];
      a[i][j] = __builtin_bit_cast(sp16, (unsigned short)h);
      b[i][j] = __builtin_bit_cast(sp16, (unsigned short)(h >> 16));
    }
  f32x4 acc[16];
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  // in-place accumulators pinned by inline asm: compiled from the builtin inside this translation unit, hipcc rotated the accumulators
  // through AGPR copies on the loop's back edge (27 instead of 17 cycles per MFMA)
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a[i & 3]), "v"(b[(i >> 2) & 3]));
  }
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");      // the last MFMAs' results are written before anything reads them
  __builtin_amdgcn_s_waitcnt(0);
  const long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
  for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][3];
  if (s == 123.456f) sink[0] = s;
  if (lane == 0) { const int w = blockIdx.x * 4 + (tid >> 6); out[2 * w] = c1 - c0; out[2 * w + 1] = r1 - r0; }
}
static int g_bench_rewarm = 0;   // "bench_rewarm": rtd_bench_conv rewrites 1 = activations, 2 = weights after its flush (back into the Infinity Cache)
int rtd_debug_option(const char* name, int value) {
  if (!name) return RTD_E_INVALID;
  if (strcmp(name, "reset") == 0) {                             // every switch back to its default (tests call this after each case)
    g_opts = PlanOpts();
    g_profile_twice = 0; g_bench_rewarm = 0;
    conv_opts_template() = ConvOpts();
    return RTD_OK;
  }
  // plan-build and conv-dispatch switches: process-wide TEMPLATES that rtd_create snapshots into the handle - a call here changes handles
  // created afterwards (and the kernel-level rtd_op_* / rtd_bench_* entry points), never a live handle
  const struct { const char* n; int* p; } plan_opts[] = {
      {"dec_fused", &g_opts.dec_fused}, {"side_stream", &g_opts.side_stream}, {"sel_fused", &g_opts.sel_fused},
      {"stem_fused_split", &g_opts.stem_fused_split}, {"stem_pool_fuse", &g_opts.stem_pool_fuse}, {"avg_fuse", &g_opts.avg_fuse}, {"dead_out", &g_opts.dead_out}, {"post_fused", &g_opts.post_fused}, {"aifi_pair", &g_opts.aifi_pair}, {"sc_fold", &g_opts.sc_fold}, {"arena_reuse", &g_opts.arena_reuse},
      {"up_fold", &g_opts.up_fold}, {"attn_split", &g_opts.attn_split}, {"c1_fuse", &g_opts.c1_fuse},
      {"profile_twice", &g_profile_twice}, {"bench_rewarm", &g_bench_rewarm},
  };
  for (const auto& t : plan_opts)
    if (strcmp(name, t.n) == 0) { *t.p = value; return RTD_OK; }
  if (conv_set_option(name, value)) return RTD_OK;
  return RTD_E_INVALID;
}

// a caller's filter [N][K] fp32 + bias [N] (device) as launch_conv wants them, staged in the call's scratch
static ConvFilter dev_filter(OpScratch& sc, int dtype, const void* w_f32, const float* bias, int N, int K) {
  ConvFilter f = conv_filter_extents(dtype, N, K);
  float* rows = sc.zeros<float>((size_t)f.Npad * f.kcols());
  HIP_CHECK(hipMemcpy2D(rows, (size_t)f.kcols() * 4, w_f32, (size_t)K * 4, (size_t)K * 4, N, hipMemcpyDeviceToDevice));
  f.bias = sc.zeros<float>(f.Npad);
  HIP_CHECK(hipMemcpy(f.bias, bias, (size_t)N * 4, hipMemcpyDeviceToDevice));
  f.w = f.converts() ? sc.get<char>(f.bytes()) : (void*)rows;
  conv_filter_convert(f, rows, nullptr);
  return f;
}
// the two-pass split-K workspace of a launch that owns none, from the call's scratch
static void give_slab(OpScratch& sc, ConvArgs& a) {
  a.ws.slab_bytes = conv_split_slab_bytes(a);
  if (a.ws.slab_bytes) a.ws.slab = sc.get<float>(a.ws.slab_bytes / 4);
}

static int op_conv_impl(int dtype, const void* x, const void* x2, int C2, const void* w_ohwi_f32, const float* bias, const void* res, void* y,
                        int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int act, int res_mode, int out_f32, int x_up2 = 0,
                        const void* w1_f32 = nullptr, const float* bias1 = nullptr, void* y1 = nullptr, int Cnext = 0, int next_act = 0) {
  return op_guard([&] {
    RTD_CHECK(KH == KW, RTD_E_INVALID, "square filters only");
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    OpScratch sc;
    const ConvFilter f = dev_filter(sc, dtype, w_ohwi_f32, bias, Cout, KH * KW * Cin + (x2 ? C2 : 0));
    // x_up2: H, W are the OUTPUT extents
    ConvArgs a = conv_args(x_up2 ? mk(x, dtype, B, H / 2, W / 2, Cin) : mk(x, dtype, B, H, W, Cin), mk(y, out_f32 ? F32 : dtype, B, OH, OW, Cout), f, KH, stride, pad, act);
    a.x_up2 = x_up2;
    a.res_mode = res ? res_mode : RES_NONE;
    if (res) a.res = mk(res, dtype, B, OH, OW, Cout);
    if (x2) a.x2 = mk(x2, dtype, B, OH, OW, C2);
    if (y1) {                                                    // a following 1x1 conv Cout -> Cnext fused into this launch (ConvArgs::next_*)
      RTD_CHECK(dtype == BF16 || dtype == F16X2, RTD_E_INVALID, "fused following conv: bf16 / f16x2 only");
      const ConvFilter f1 = dev_filter(sc, dtype, w1_f32, bias1, Cnext, Cout);
      a.next_w = f1.w; a.next_bias = f1.bias; a.next_y = mk(y1, dtype, B, OH, OW, Cnext); a.next_kpad = f1.Kpad; a.next_act = next_act;
      RTD_CHECK(conv_next_supported(a), RTD_E_INVALID, "fused following conv: shape not taken by the streaming kernels");
    }
    give_slab(sc, a);
    launch_conv(a, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int rtd_op_conv(int dtype, const void* x, const void* w_ohwi_f32, const float* bias, const void* res, void* y, int B, int H,
                int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int act, int res_mode, int out_f32) {
  return op_conv_impl(dtype, x, nullptr, 0, w_ohwi_f32, bias, res, y, B, H, W, Cin, Cout, KH, KW, stride, pad, act, res_mode, out_f32);
}

int rtd_op_conv_view(int dtype, const void* x, int ldx, const void* w_ohwi_f32, const float* bias, const void* res, int ldres, void* y, int ldy,
                     int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int act, int res_mode) {
  return op_guard([&] {
    RTD_CHECK(x && y && w_ohwi_f32 && bias && ldx >= Cin && ldy >= Cout && (!res || ldres >= Cout), RTD_E_INVALID, "conv view: arguments");
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    OpScratch sc;
    const ConvFilter f = dev_filter(sc, dtype, w_ohwi_f32, bias, Cout, KH * KH * Cin);
    auto view = [&](const void* p, int h, int w, int c, int ld) { Tensor t = mk(p, dtype, B, h, w, c); t.ld = ld; t.bstride = (int64_t)h * w * ld; return t; };
    ConvArgs a = conv_args(view(x, H, W, Cin, ldx), view(y, OH, OW, Cout, ldy), f, KH, stride, pad, act);
    a.res_mode = res ? res_mode : RES_NONE;
    if (res) a.res = view(res, OH, OW, Cout, ldres);
    give_slab(sc, a);
    launch_conv(a, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// the launch rtd_op_conv_views / rtd_debug_conv_choice_views describe: rtd_op_conv_dual's (x2 optional) on channel-slice views, images
// dense inside each buffer (bstride = h * w * ld) as Tensor::slice_c makes them; the filter's pointers are the caller's business
static ConvArgs views_args(int dtype, const void* x, int ldx, const void* x2, int C2, int ldx2, const ConvFilter& f, const void* res, int ldres, void* y,
                           int ldy, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int act, int res_mode, int out_f32, int x_up2) {
  RTD_CHECK(dtype == BF16 || dtype == F32 || dtype == F16X2, RTD_E_INVALID, "conv views: dtype");
  RTD_CHECK(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && KH >= 1 && stride >= 1 && pad >= 0, RTD_E_INVALID, "conv views: extents");
  RTD_CHECK(ldx >= Cin && ldy >= Cout && (!x2 || (C2 >= 1 && ldx2 >= C2)) && (!res || ldres >= Cout), RTD_E_INVALID, "conv views: pixel strides");
  RTD_CHECK(!x_up2 || (x2 && !((H | W) & 1)), RTD_E_INVALID, "conv views: x_up2 needs a second input and even output extents");
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
  auto view = [&](const void* p, int dt, int h, int w, int c, int ld) { Tensor t = mk(p, dt, B, h, w, c); t.ld = ld; t.bstride = (int64_t)h * w * ld; return t; };
  ConvArgs a = conv_args(x_up2 ? view(x, dtype, H / 2, W / 2, Cin, ldx) : view(x, dtype, H, W, Cin, ldx), view(y, out_f32 ? F32 : dtype, OH, OW, Cout, ldy), f, KH,
                         stride, pad, act);
  a.x_up2 = x_up2;
  a.res_mode = res ? res_mode : RES_NONE;
  if (res) a.res = view(res, dtype, OH, OW, Cout, ldres);
  if (x2) a.x2 = view(x2, dtype, OH, OW, C2, ldx2);
  return a;
}

int rtd_op_conv_views(int dtype, const void* x, int ldx, const void* x2, int C2, int ldx2, const void* w_f32, const float* bias, const void* res, int ldres,
                      void* y, int ldy, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int act, int res_mode, int out_f32, int x_up2) {
  if (!x || !y || !w_f32 || !bias) return RTD_E_INVALID;
  return op_guard([&] {
    RTD_CHECK((dtype == BF16 || dtype == F32 || dtype == F16X2) && Cin >= 1 && Cout >= 1 && KH >= 1 && (!x2 || C2 >= 1), RTD_E_INVALID, "conv views: arguments");
    OpScratch sc;
    const ConvFilter f = dev_filter(sc, dtype, w_f32, bias, Cout, KH * KH * Cin + (x2 ? C2 : 0));
    ConvArgs a = views_args(dtype, x, ldx, x2, C2, ldx2, f, res, ldres, y, ldy, B, H, W, Cin, Cout, KH, stride, pad, act, res_mode, out_f32, x_up2);
    give_slab(sc, a);
    launch_conv(a, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int rtd_op_conv_dual(int dtype, const void* x, const void* x2, const void* w_f32, const float* bias, const void* res, void* y, int B,
                     int H, int W, int Cin, int C2, int Cout, int KH, int stride, int pad, int act, int res_mode, int out_f32, int x_up2) {
  if (!x2 || (x_up2 && ((H | W) & 1))) return RTD_E_INVALID;
  return op_conv_impl(dtype, x, x2, C2, w_f32, bias, res, y, B, H, W, Cin, Cout, KH, KH, stride, pad, act, res_mode, out_f32, x_up2);
}

int rtd_op_conv_next(int dtype, const void* x, const void* x2, const void* w_f32, const float* bias, const void* res, void* y, const void* w1_f32,
                     const float* bias1, void* y1, int B, int H, int W, int Cin, int C2, int Cout, int Cnext, int act, int res_mode, int next_act) {
  if (!y1 || !w1_f32 || !bias1) return RTD_E_INVALID;
  return op_conv_impl(dtype, x, x2, x2 ? C2 : 0, w_f32, bias, res, y, B, H, W, Cin, Cout, 1, 1, 1, 0, act, res_mode, 0, 0, w1_f32, bias1, y1, Cnext, next_act);
}

// ... plus the fused 2 x 2 average of y (ConvArgs::avg_y) and, with y_dead, without the stores of y.  Cnext = 0: no follower.
int rtd_op_conv_avg(const void* x, const void* w_f32, const float* bias, const void* res, void* y, const void* w1_f32, const float* bias1, void* y1,
                    void* avg_y, int B, int H, int W, int Cin, int Cout, int Cnext, int act, int res_mode, int next_act, int y_dead) {
  if (!x || !w_f32 || !bias || !y || !avg_y || (Cnext != 0 && (!w1_f32 || !bias1 || !y1))) return RTD_E_INVALID;
  return op_guard([&] {
    RTD_CHECK(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && Cnext >= 0, RTD_E_INVALID, "conv + average: extents");
    OpScratch sc;
    const ConvFilter f = dev_filter(sc, F16X2, w_f32, bias, Cout, Cin);
    ConvArgs a = conv_args(mk(x, F16X2, B, H, W, Cin), mk(y, F16X2, B, H, W, Cout), f, 1, 1, 0, act);
    a.res_mode = res ? res_mode : RES_NONE;
    if (res) a.res = mk(res, F16X2, B, H, W, Cout);
    if (Cnext) {
      const ConvFilter f1 = dev_filter(sc, F16X2, w1_f32, bias1, Cnext, Cout);
      a.next_w = f1.w; a.next_bias = f1.bias; a.next_y = mk(y1, F16X2, B, H, W, Cnext); a.next_kpad = f1.Kpad; a.next_act = next_act;
    }
    a.avg_y = mk(avg_y, F16X2, B, H / 2, W / 2, Cout);
    a.y_dead = y_dead;
    RTD_CHECK(conv_avg_supported(a) && conv_sx_batch_fits(a), RTD_E_INVALID, "conv + average: shape not taken by the streaming kernel");
    give_slab(sc, a);
    launch_conv(a, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// stem.2 (3x3, 32 -> 64 channels, ReLU) and the 3x3 / stride-2 max-pool in one pass: x [B, H, W, 32] -> pooled [B, H / 2, W / 2, 64], pairs
int rtd_op_conv_pool(const void* x, const void* w_ohwi_f32, const float* bias, void* pooled, int B, int H, int W) {
  if (!x || !w_ohwi_f32 || !bias || !pooled) return RTD_E_INVALID;
  return op_guard([&] {
    RTD_CHECK(B >= 1 && H >= 1 && W >= 1, RTD_E_INVALID, "conv + max-pool: extents");
    OpScratch sc;
    const ConvFilter f = dev_filter(sc, F16X2, w_ohwi_f32, bias, 64, 9 * 32);
    const ConvArgs a = conv_args(mk(x, F16X2, B, H, W, 32), mk(nullptr, F16X2, B, H, W, 64), f, 3, 1, 1, ACT_RELU);   // y is never written
    const Tensor p = mk(pooled, F16X2, B, H / 2, W / 2, 64);
    RTD_CHECK(conv_pool_supported(a, p), RTD_E_INVALID, "conv + max-pool: shape not supported (even extents, >= 32 tiles of 8 x 32 per image, conv_reg)");
    launch_conv_pool(a, p, sc.get<char>(conv_pool_side_bytes(a)), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// backbone.stem.0 straight from the uint8 frames (launch_stem0_u8), the filter staged as the engine's get_weight({{"backbone.stem.0", 72}},
// F16X2, 32) packs it; frames_dev: a HOST array of n device pointers ([H][W][3] BGR bytes at any address), y [n, OH, OW, 32] pairs, dense
int rtd_op_stem0_u8(const uint8_t* const* frames_dev, int n, int H, int W, const void* w_ohwi_f32, const float* bias, void* y, int act) {
  if (!frames_dev || !w_ohwi_f32 || !bias || !y || n < 1 || n > RTD_MAX_BATCH || H < 1 || W < 1) return RTD_E_INVALID;
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_SILU) return RTD_E_INVALID;      // (what the launcher refuses, before any device work)
  for (int i = 0; i < n; ++i)
    if (!frames_dev[i]) return RTD_E_INVALID;
  return op_guard([&] {
    OpScratch sc;
    const ConvFilter f = dev_filter(sc, F16X2, w_ohwi_f32, bias, 32, 9 * 8);
    const uint8_t* const* table = sc.upload(frames_dev, (size_t)n);
    launch_stem0_u8(table, n, H, W, f.w, f.Kpad, f.bias, mk(y, F16X2, n, (H - 1) / 2 + 1, (W - 1) / 2 + 1, 32), act, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// ---- the conv choice, readable: host arithmetic only, no device call (they work on a machine without a GPU) ----
static void report_out(const ConvChoiceReport& r, char* key, int key_capacity, int32_t* info) {
  RTD_CHECK(key && info && key_capacity > (int)strlen(r.key), RTD_E_INVALID, "conv choice: key buffer too small");
  strcpy(key, r.key);
  const int v[12] = {r.family, r.stages, r.bn, r.mt, r.bm, r.smallc, r.wsq, r.sx, r.cog, r.S, r.grid, r.ntn};
  for (int i = 0; i < 12; ++i) info[i] = v[i];
}
int rtd_debug_conv_choice(int dtype, int B, int H, int W, int Cin, int C2, int Cout, int KH, int stride, int pad, int res_mode, int out_f32,
                          int x_up2, int Cnext, int avg, int pool, char* key, int key_capacity, int32_t* info) {
  return backend::caught(create_error(), [&] {
    RTD_CHECK(dtype == BF16 || dtype == F32 || dtype == F16X2, RTD_E_INVALID, "conv choice: dtype");
    RTD_CHECK(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && C2 >= 0 && Cout >= 1 && KH >= 1 && stride >= 1 && pad >= 0 && Cnext >= 0, RTD_E_INVALID, "conv choice: extents");
    RTD_CHECK(!x_up2 || !((H | W) & 1), RTD_E_INVALID, "conv choice: x_up2 needs even output extents");
    // the launch as op_conv_impl / rtd_op_conv_avg / rtd_op_conv_pool describe it: dense tensors behind a dummy 16-byte aligned address
    const void* const P = (const void*)(uintptr_t)4096;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    ConvFilter f = conv_filter_extents(dtype, Cout, KH * KH * Cin + C2);
    f.w = (void*)P; f.bias = (float*)P;
    ConvArgs a = conv_args(x_up2 ? mk(P, dtype, B, H / 2, W / 2, Cin) : mk(P, dtype, B, H, W, Cin), mk(P, out_f32 ? F32 : dtype, B, OH, OW, Cout), f, KH, stride, pad,
                           ACT_RELU);
    a.x_up2 = x_up2;
    a.res_mode = res_mode;
    if (res_mode != RES_NONE) a.res = mk(P, dtype, B, OH, OW, Cout);
    if (C2) a.x2 = mk(P, dtype, B, OH, OW, C2);
    if (Cnext) {
      a.next_w = P; a.next_bias = (const float*)P; a.next_y = mk(P, dtype, B, OH, OW, Cnext);
      a.next_kpad = conv_filter_extents(dtype, Cnext, Cout).Kpad; a.next_act = ACT_RELU;
    }
    if (avg) a.avg_y = mk(P, dtype, B, OH / 2, OW / 2, Cout);
    ConvChoiceReport r;
    if (pool) {
      const Tensor p = mk(P, dtype, B, OH / 2, OW / 2, Cout);
      r = conv_predict(a, &p);
    } else {
      r = conv_predict(a, nullptr);
    }
    report_out(r, key, key_capacity, info);
  });
}
// ... for the launch rtd_op_conv_views describes: the same views (pixel strides ld*, images dense inside each buffer) behind 16-byte aligned
// probe addresses, as yolox_net.hip's builder puts its launches to conv_predict
int rtd_debug_conv_choice_views(int dtype, int ldx, int C2, int ldx2, int ldres, int ldy, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad,
                                int res_mode, int out_f32, int x_up2, char* key, int key_capacity, int32_t* info) {
  return backend::caught(create_error(), [&] {
    RTD_CHECK((dtype == BF16 || dtype == F32 || dtype == F16X2) && Cin >= 1 && Cout >= 1 && KH >= 1 && C2 >= 0, RTD_E_INVALID, "conv choice (views): arguments");
    void* const P = (void*)(uintptr_t)4096;
    ConvFilter f = conv_filter_extents(dtype, Cout, KH * KH * Cin + C2);
    f.w = P; f.bias = (float*)P;
    const ConvArgs a = views_args(dtype, P, ldx, C2 ? P : nullptr, C2, ldx2, f, res_mode != RES_NONE ? P : nullptr, ldres, P, ldy, B, H, W, Cin, Cout, KH, stride,
                                  pad, ACT_RELU, res_mode, out_f32, x_up2);
    report_out(conv_predict(a, nullptr), key, key_capacity, info);
  });
}
int rtd_debug_last_conv(char* key, int key_capacity, int32_t* info) {
  return backend::caught(create_error(), [&] {
    ConvChoiceReport r;
    RTD_CHECK(conv_last_choice(&r), RTD_E_STATE, "no conv launch on this thread yet");
    report_out(r, key, key_capacity, info);
  });
}
int rtd_debug_conv_instantiations(char* out, int64_t capacity, int64_t* needed) {
  return backend::caught(create_error(), [&] {
    std::string all;
    for (const std::string& k : conv_instantiation_keys()) all += k + "\n";
    if (needed) *needed = (int64_t)all.size() + 1;
    if (!out) return;
    RTD_CHECK(capacity > (int64_t)all.size(), RTD_E_INVALID, "conv instantiations: buffer too small");
    memcpy(out, all.c_str(), all.size() + 1);
  });
}

// operands of one benchmarked conv in the call's scratch: zero-filled input, filter, bias and residual, the output, the split-K workspace
struct BenchConv {
  ConvArgs a;
  ConvFilter f;
  void *x = nullptr, *r = nullptr;
  size_t xb = 0, yb = 0;
};
static BenchConv bench_conv_make(OpScratch& sc, int dtype, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int with_res, int act) {
  BenchConv c;
  c.f = conv_filter_extents(dtype, Cout, KH * KH * Cin);
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
  const size_t es = dtype == BF16 ? 2 : 4;
  c.xb = (size_t)B * H * W * Cin * es; c.yb = (size_t)B * OH * OW * Cout * es;
  c.x = sc.zeros<char>(c.xb);
  void* y = sc.get<char>(c.yb);
  c.f.w = sc.zeros<char>(c.f.bytes());
  c.f.bias = sc.zeros<float>(c.f.Npad);
  c.a = conv_args(mk(c.x, dtype, B, H, W, Cin), mk(y, dtype, B, OH, OW, Cout), c.f, KH, stride, pad, act);
  if (with_res) {
    c.r = sc.zeros<char>(c.yb);
    c.a.res = mk(c.r, dtype, B, OH, OW, Cout);
    c.a.res_mode = RES_PRE;
  }
  give_slab(sc, c.a);                                            // two-pass split-K
  if (c.a.ws.slab) HIP_CHECK(hipMemset(c.a.ws.slab, 0, c.a.ws.slab_bytes));
  return c;
}

static int bench_conv_impl(int dtype, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int with_res, int act, int reps,
                           int flush_mb, float* us_out) {
  return op_guard([&] {
    OpScratch sc;
    const BenchConv c = bench_conv_make(sc, dtype, B, H, W, Cin, Cout, KH, stride, pad, with_res, act);
    const ConvArgs& a = c.a;
    void *x = c.x, *r = c.r, *w = c.f.w, *y = a.y.p; float* bias = c.f.bias;
    const size_t xb = c.xb, yb = c.yb, wb = c.f.bytes();
    const int OH = a.y.h, OW = a.y.w;
    if ((g_bench_rewarm & 32) && dtype != F32) {                 // "bench_rewarm" bit 5: random 16-bit operands instead of zeros
      rtd_launch(k_fill_rand16, dim3(1024), dim3(256), 0, nullptr, (uint16_t*)x, xb / 2, 1u);
      rtd_launch(k_fill_rand16, dim3(1024), dim3(256), 0, nullptr, (uint16_t*)w, wb / 2, 2u);
      if (r) rtd_launch(k_fill_rand16, dim3(1024), dim3(256), 0, nullptr, (uint16_t*)r, yb / 2, 3u);
      HIP_CHECK(hipDeviceSynchronize());
    }
    void* flush = flush_mb > 0 ? sc.get<char>((size_t)flush_mb << 20) : nullptr;
    const hipEvent_t e0 = sc.event(), e1 = sc.event();
    for (int i = 0; i < 3; ++i) launch_conv(a, nullptr);
    HIP_CHECK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < reps; ++i) launch_conv(a, nullptr);
    HIP_CHECK(hipEventRecord(e1, nullptr));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    us_out[0] = ms * 1e3f / reps;
    us_out[1] = 0.f;
    if (flush) {
      float tot = 0.f;
      for (int i = 0; i < reps; ++i) {
        HIP_CHECK(hipMemsetAsync(flush, i & 0xff, (size_t)flush_mb << 20, nullptr));
        if (g_bench_rewarm & 1) { HIP_CHECK(hipMemsetAsync(x, 0, xb, nullptr)); if (r) HIP_CHECK(hipMemsetAsync(r, 0, yb, nullptr)); }
        if (g_bench_rewarm & 2) HIP_CHECK(hipMemsetAsync(w, 0, wb, nullptr));
        if (g_bench_rewarm & 4) rtd_launch(k_touch_read, dim3(64), dim3(256), 0, nullptr, (const unsigned*)w, wb / 128, (unsigned*)bias);
        if (g_bench_rewarm & 16) {      // in-kernel prefetch path: a small unrelated conv launch carries pf = this filter
          ConvArgs d = a;
          d.x = mk(x, dtype, 1, H, W, Cin); d.y = mk(y, dtype, 1, OH, OW, Cout);
          if (with_res) d.res = mk(r, dtype, 1, OH, OW, Cout);
          d.pf = w; d.pf_bytes = wb;
          launch_conv(d, nullptr);
        }
        if (g_bench_rewarm & 8) rtd_launch(k_touch_read, dim3(64), dim3(256), 0, nullptr, (const unsigned*)x, xb / 128, (unsigned*)bias);
        HIP_CHECK(hipEventRecord(e0, nullptr));
        launch_conv(a, nullptr);
        HIP_CHECK(hipEventRecord(e1, nullptr));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        tot += ms;
      }
      us_out[1] = tot * 1e3f / reps;
    }
    HIP_CHECK(hipDeviceSynchronize());
  });
}
int rtd_bench_conv(int dtype, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int with_res, int reps,
                   int flush_mb, float* us_out) {
  return bench_conv_impl(dtype, B, H, W, Cin, Cout, KH, stride, pad, with_res, ACT_RELU, reps, flush_mb, us_out);
}
int rtd_bench_conv_act(int dtype, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int with_res, int act, int reps,
                       int flush_mb, float* us_out) {
  if (act < ACT_NONE || act > ACT_LRELU) return RTD_E_INVALID;
  return bench_conv_impl(dtype, B, H, W, Cin, Cout, KH, stride, pad, with_res, act, reps, flush_mb, us_out);
}

// Concurrency micro-benchmark (tools/pair_bench.py): conv A on one stream, conv B on another; us_out = {A alone, B alone,
// A and B issued together} per repetition (`reps` launches of each).  sh: B, HW, Cin, Cout, K, stride, pad
int rtd_bench_conv_pair(const int* shape_a, const int* shape_b, int reps, float* us_out) {
  return op_guard([&] {
    OpScratch sc;
    auto make = [&](const int* sh) { return bench_conv_make(sc, BF16, sh[0], sh[1], sh[1], sh[2], sh[3], sh[4], sh[5], sh[6], 0, ACT_RELU).a; };
    const ConvArgs A = make(shape_a), B = make(shape_b);
    const hipStream_t s1 = sc.stream(), s2 = sc.stream();
    auto run = [&](bool ra, bool rb) {
      for (int i = 0; i < 3; ++i) { if (ra) launch_conv(A, s1); if (rb) launch_conv(B, s2); }
      HIP_CHECK(hipDeviceSynchronize());
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < reps; ++i) { if (ra) launch_conv(A, s1); if (rb) launch_conv(B, s2); }
      HIP_CHECK(hipStreamSynchronize(s1));
      HIP_CHECK(hipStreamSynchronize(s2));
      return (float)(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps);
    };
    us_out[0] = run(true, false);
    us_out[1] = run(false, true);
    us_out[2] = run(true, true);
  });
}

int rtd_bench_mfma_rate(int random_operands, int ms_target, float* out) {
  return op_guard([&] {
    RTD_CHECK(out && ms_target >= 1 && ms_target <= 2000, RTD_E_INVALID, "arguments");
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));                              // the CURRENT device (a rank's own GPU), not device 0
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    const int cus = prop.multiProcessorCount;
    std::vector<unsigned> hs(4096, 0u);
    if (random_operands)
      for (int i = 0; i < 4096; ++i) {
        unsigned h = (unsigned)i * 2654435761u + 12345u; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        const unsigned lo = (h & 0x8000u) | ((10u + ((h >> 20) & 7u)) << 10) | (h & 0x3ffu);
        unsigned h2 = h * 2654435761u; h2 ^= h2 >> 16;
        const unsigned hi = (h2 & 0x8000u) | ((10u + ((h2 >> 20) & 7u)) << 10) | (h2 & 0x3ffu);
        hs[i] = lo | (hi << 16);
      }
    OpScratch sc;
    const unsigned* seed = sc.upload(hs.data(), hs.size());
    long long* stamps = sc.get<long long>((size_t)cus * 4 * 2);
    float* sink = sc.get<float>(4);
    // 16 MFMAs of 16 cycles per iteration at <= 2.4 GHz: 9400 iterations per millisecond
    const int iters = ms_target * 9400;
    const hipEvent_t e0 = sc.event(), e1 = sc.event();
    float ms = 0.f;
    for (int rep = 0; rep < 3; ++rep) {
      HIP_CHECK(hipEventRecord(e0, nullptr));
      rtd_launch(k_mfma_rate, dim3(cus), dim3(256), 0, nullptr, seed, iters, stamps, sink);
      HIP_CHECK(hipEventRecord(e1, nullptr));
      HIP_CHECK(hipEventSynchronize(e1));
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    }
    std::vector<long long> h((size_t)cus * 4 * 2);
    HIP_CHECK(hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost));
    double cyc = 0, rt = 0;
    for (int w = 0; w < cus * 4; ++w) { cyc += (double)h[2 * w]; rt += (double)h[2 * w + 1]; }
    out[0] = (float)((double)iters * 16.0 * cus * 4.0 * 16384.0 / (ms * 1e-3) / 1e12);
    out[1] = (float)(cyc / (rt * 10.0));
    out[2] = ms;
  });
}

int rtd_op_layernorm(int dtype, const void* x, const void* res, const float* g, const float* b, void* y, int rows, int dim, int out_f32) {
  return op_guard([&] {
    Tensor tx = mk(x, dtype, 1, rows, 1, dim), ty = mk(y, out_f32 ? F32 : dtype, 1, rows, 1, dim), tr = mk(res, dtype, 1, rows, 1, dim);
    launch_layernorm(tx, res ? &tr : nullptr, g, b, ty, 1e-5f, nullptr);
  });
}

int rtd_op_attention(int dtype, const void* qk, const void* v, void* o, int B, int L, int heads, int hd) {
  return op_guard([&] {
    const int D = heads * hd;
    launch_attention(mk(qk, dtype, B, L, 1, 2 * D), mk(v, dtype, B, L, 1, D), mk(o, dtype, B, L, 1, D), heads, nullptr);
  });
}

// the body both msdeform entry points share (each keeps its own argument checks): the level table [n_levels][3] h, w, start on the
// device, the reference boxes widened to 8-float rows, the launch
static void op_msdeform_body(int dtype, const void* value, int value_ld, int value_coff, const float* offaw, const float* ref, float* out, int B, int Q,
                             int heads, int hd, int n_levels, int n_points, const int32_t* level_hw, float offset_scale, int method) {
  int32_t lv[24]; int S = 0;
  for (int l = 0; l < n_levels; ++l) { lv[l * 3] = level_hw[2 * l]; lv[l * 3 + 1] = level_hw[2 * l + 1]; lv[l * 3 + 2] = S; S += level_hw[2 * l] * level_hw[2 * l + 1]; }
  OpScratch sc;
  const int32_t* lvd = sc.upload(lv, (size_t)3 * n_levels);
  float* ref8 = sc.zeros<float>((size_t)B * Q * 8);
  HIP_CHECK(hipMemcpy2D(ref8, 32, ref, 16, 16, (size_t)B * Q, hipMemcpyDeviceToDevice));
  launch_msdeform(rows_view(value, dtype, B, S, heads * hd, value_ld), value_coff, mk(offaw, F32, B, Q, 1, heads * n_levels * n_points * 3), ref8,
                  mk(out, F32, B, Q, 1, heads * hd), heads, hd, n_levels, n_points, lvd, offset_scale, method, nullptr);
  HIP_CHECK(hipDeviceSynchronize());
}

int rtd_op_msdeform(int dtype, const void* value, const float* offaw, const float* ref, float* out, int B, int Q, int heads, int hd,
                    int n_levels, int n_points, const int32_t* level_hw, int value_ld, float offset_scale) {
  return op_guard([&] {
    RTD_CHECK(n_levels >= 1 && n_levels <= 8, RTD_E_INVALID, "n_levels");
    op_msdeform_body(dtype, value, value_ld, 0, offaw, ref, out, B, Q, heads, hd, n_levels, n_points, level_hw, offset_scale, DEC_DEFAULT);
  });
}

// both view entry points: the argument checks, then the shared body with the sampler of `method`
static int op_msdeform_view(int method, int dtype, const void* value, int value_ld, int value_coff, const float* offaw, const float* ref, float* out,
                            int B, int Q, int heads, int hd, int n_levels, int n_points, const int32_t* level_hw, float offset_scale) {
  return op_guard([&] {
    RTD_CHECK(value && offaw && ref && out && level_hw && rows_fit_int(B, Q), RTD_E_INVALID, "msdeform view: arguments");
    RTD_CHECK(hd == 32 && heads >= 1, RTD_E_INVALID, "msdeform view: head dim must be 32");
    RTD_CHECK(n_levels >= 1 && n_levels <= 8 && n_points >= 1, RTD_E_INVALID, "msdeform view: 1..8 levels");
    RTD_CHECK(value_coff >= 0 && value_coff + heads * hd <= value_ld, RTD_E_INVALID, "msdeform view: the channel slice leaves the value row");
    for (int l = 0; l < n_levels; ++l) RTD_CHECK(level_hw[2 * l] >= 1 && level_hw[2 * l + 1] >= 1, RTD_E_INVALID, "msdeform view: level extents");
    op_msdeform_body(dtype, value, value_ld, value_coff, offaw, ref, out, B, Q, heads, hd, n_levels, n_points, level_hw, offset_scale, method);
  });
}

int rtd_op_msdeform_view(int dtype, const void* value, int value_ld, int value_coff, const float* offaw, const float* ref, float* out, int B, int Q,
                         int heads, int hd, int n_levels, int n_points, const int32_t* level_hw, float offset_scale) {
  return op_msdeform_view(DEC_DEFAULT, dtype, value, value_ld, value_coff, offaw, ref, out, B, Q, heads, hd, n_levels, n_points, level_hw, offset_scale);
}

int rtd_op_msdeform_discrete_view(int dtype, const void* value, int value_ld, int value_coff, const float* offaw, const float* ref, float* out, int B,
                                  int Q, int heads, int hd, int n_levels, int n_points, const int32_t* level_hw, float offset_scale) {
  return op_msdeform_view(DEC_DISCRETE, dtype, value, value_ld, value_coff, offaw, ref, out, B, Q, heads, hd, n_levels, n_points, level_hw, offset_scale);
}

int rtd_op_select_score(const float* x, int ldx, const float* w_f32, const float* bias, const float* g, const float* b, float* mx, int B, int S,
                        int C, int K) {
  return op_guard([&] {
    RTD_CHECK(x && w_f32 && bias && g && b && mx && rows_fit_int(B, S) && C >= 1, RTD_E_INVALID, "select_score: arguments");
    RTD_CHECK(K == 256 && ldx >= K && ldx % 4 == 0 && aligned16(x, g, b), RTD_E_INVALID, "select_score: 256-wide rows in 16-byte aligned storage");
    const int ntiles = packed_ntiles(C);                         // the engine's own packing (get_weight_packed): bias zero padded to Npad
    std::vector<float> hw((size_t)C * K), hb((size_t)ntiles * 16, 0.f);
    HIP_CHECK(hipMemcpy(hw.data(), w_f32, hw.size() * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hb.data(), bias, (size_t)C * 4, hipMemcpyDeviceToHost));
    const std::vector<float> pk = pack_fragments_f32_host(hw.data(), C, K, K, ntiles);
    OpScratch sc;
    SelArgs a{};
    a.score.w = sc.upload(pk.data(), pk.size()); a.score.b = sc.upload(hb.data(), hb.size()); a.score.ldw = K; a.score.N = C; a.score.K = K;
    a.ln.g = g; a.ln.b = b;
    a.x = x; a.ldx = ldx; a.rows = B * S; a.C = C; a.rows_per_image = S; a.mx = mx;
    launch_select_score(a, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int rtd_op_gather_ln(const float* x, int ldx, int S, const int32_t* idx, int B, int Q, const float* g, const float* b, float* dst, int ldd) {
  return op_guard([&] {
    RTD_CHECK(x && idx && g && b && dst && rows_fit_int(B, S) && rows_fit_int(B, Q), RTD_E_INVALID, "gather_ln: arguments");
    RTD_CHECK(ldx >= 256 && ldd >= 256 && ldx % 4 == 0 && ldd % 4 == 0 && aligned16(x, dst), RTD_E_INVALID, "gather_ln: 256-wide rows in 16-byte aligned storage");
    DecLN ln{g, b};
    launch_gather_ln(x, ldx, S, idx, B, Q, ln, dst, ldd, nullptr);
  });
}

int rtd_op_split_convert(int direction, const void* src, void* dst, int64_t rows, int C, int64_t lds, int64_t ldd) {
  return op_guard([&] {
    RTD_CHECK(src && dst && rows >= 1 && C >= 1 && lds >= C, RTD_E_INVALID, "split_convert: arguments");
    RTD_CHECK(C % SPLIT_GROUP == 0, RTD_E_INVALID, "split_convert: whole 32-channel groups");
    if (direction == 0) { RTD_CHECK(ldd >= C, RTD_E_INVALID, "split_convert: ldd"); launch_f32_to_split((const float*)src, lds, dst, ldd, rows, C, nullptr); }
    else if (direction == 1) { RTD_CHECK(ldd >= C, RTD_E_INVALID, "split_convert: ldd"); launch_split_to_f32(src, lds, (float*)dst, ldd, rows, C, nullptr); }
    else if (direction == 2) { RTD_CHECK(lds % SPLIT_GROUP == 0, RTD_E_INVALID, "split_convert: lds"); launch_count_saturated(src, rows * lds * 2, (unsigned long long*)dst, nullptr); }
    else RTD_CHECK(false, RTD_E_INVALID, "split_convert: direction 0 fp32 -> pair, 1 pair -> fp32, 2 count saturated");
  });
}

int rtd_op_set_rows(int dtype, void* y, int ld, int C, const int32_t* rows, int nrows, int rows_per_image, const float* vec, int B) {
  return op_guard([&] {
    RTD_CHECK(y && rows && vec && nrows >= 0 && nrows <= rows_per_image && C >= 1 && ld >= C && rows_fit_int(B, rows_per_image), RTD_E_INVALID, "set_rows: arguments");
    launch_set_rows(rows_view(y, dtype, B, rows_per_image, C, ld), rows, nrows, rows_per_image, vec, nullptr);
  });
}

int rtd_op_rowmax(const float* x, int ld, int C, int rows, float* out) {
  return op_guard([&] {
    RTD_CHECK(x && out && rows >= 1 && C >= 1 && ld >= C, RTD_E_INVALID, "rowmax: arguments");
    launch_rowmax(rows_view(x, F32, 1, rows, C, ld), out, nullptr);
  });
}

int rtd_op_gather_rows(int src_dtype, const void* src, int lds, int S, const int32_t* idx, int B, int Q, int C, float* dst, int ldd) {
  return op_guard([&] {
    RTD_CHECK(src && idx && dst && rows_fit_int(B, S) && rows_fit_int(B, Q) && C >= 1 && lds >= C && ldd >= C, RTD_E_INVALID, "gather_rows: arguments");
    launch_gather_rows(rows_view(src, src_dtype, B, S, C, lds), idx, S, rows_view(dst, F32, B, Q, C, ldd), nullptr);
  });
}

int rtd_op_boxes(const float* delta, int ldd, int rows, float* ref8, const float* anchors, const int32_t* idx, int S, float* ref_unact8) {
  return op_guard([&] {
    RTD_CHECK(delta && ref8 && rows >= 1 && ldd >= 4, RTD_E_INVALID, "boxes: arguments");
    const Tensor d = rows_view(delta, F32, 1, rows, 4, ldd);
    if (!anchors) { launch_box_refine(d, ref8, nullptr); return; }
    RTD_CHECK(idx && ref_unact8 && S >= 1, RTD_E_INVALID, "boxes: ref_init needs the token indices, S and the raw-box output");
    launch_ref_init(d, anchors, idx, S, ref_unact8, ref8, nullptr);
  });
}

int rtd_op_add(int dt_a, int dt_b, int dt_y, const void* a, const void* b, void* y, int B, int rows, int C, int b_broadcast) {
  return op_guard([&] {
    RTD_CHECK(a && b && y && rows_fit_int(B, rows) && C >= 1, RTD_E_INVALID, "add: arguments");
    launch_add(mk(a, dt_a, B, rows, 1, C), mk(b, dt_b, b_broadcast ? 1 : B, rows, 1, C), mk(y, dt_y, B, rows, 1, C), nullptr);
  });
}

int rtd_op_postprocess(const float* logits, const float* ref8, const float* scale_wh, int B, int Q, int C, int K, int fused, float* block6) {
  return op_guard([&] {
    RTD_CHECK(logits && ref8 && scale_wh && block6 && rows_fit_int(B, Q) && C >= 1 && (int64_t)Q * C <= 0x7fffffff, RTD_E_INVALID, "postprocess: arguments");
    RTD_CHECK(K == Q, RTD_E_INVALID, "postprocess: one output row per query (K == Q)");
    const Tensor lg = mk(logits, F32, B, Q, 1, C);
    if (fused) {
      RTD_CHECK(postprocess_fused_supported(lg, B, Q), RTD_E_INVALID, "postprocess: the one-launch form does not take this shape");
      launch_postprocess_fused(lg, ref8, scale_wh, B, Q, block6, nullptr);
      return;
    }
    RTD_CHECK(K <= 1024, RTD_E_INVALID, "postprocess: K <= 1024");
    OpScratch sc;
    float* scores = sc.get<float>((size_t)B * Q * C);
    float* topv = sc.get<float>((size_t)B * K);
    int32_t* topi = sc.get<int32_t>((size_t)B * K);
    launch_postprocess_scores(lg, scores, nullptr);
    launch_topk(scores, B, Q * C, K, topi, topv, nullptr);
    launch_postprocess_gather(topv, topi, ref8, scale_wh, B, Q, C, block6, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int rtd_op_pool(int kind, int dtype, const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy) {
  return op_guard([&] {
    RTD_CHECK(kind >= 0 && kind <= 2 && ldx >= C && ldy >= C, RTD_E_INVALID, "op_pool: kind 0 max-pool, 1 avg-pool, 2 upsample; ld >= C");
    const int OH = kind == 0 ? (H + 2 - 3) / 2 + 1 : (kind == 1 ? H / 2 : 2 * H), OW = kind == 0 ? (W + 2 - 3) / 2 + 1 : (kind == 1 ? W / 2 : 2 * W);
    Tensor tx = mk(x, dtype, B, H, W, C), ty = mk(y, dtype, B, OH, OW, C);
    tx.ld = ldx; tx.bstride = (int64_t)H * W * ldx;
    ty.ld = ldy; ty.bstride = (int64_t)OH * OW * ldy;
    if (kind == 0) launch_maxpool3x3s2(tx, ty, nullptr);
    else if (kind == 1) launch_avgpool2(tx, ty, nullptr);
    else launch_upsample2x(tx, ty, nullptr);
  });
}

int rtd_op_topk(const float* keys, int B, int N, int K, int32_t* idx_out, float* val_out) {
  return op_guard([&] { launch_topk(keys, B, N, K, idx_out, val_out, nullptr); });
}

int rtd_op_resize(const uint8_t* src, int sh, int sw, void* dst, int dh, int dw, int dtype) {
  return op_guard([&] {
    std::vector<int32_t> hb, hk, vb, vk;
    int hks, vks;
    pil_coeffs(sw, dw, hb, hk, hks);
    pil_coeffs(sh, dh, vb, vk, vks);
    OpScratch sc;
    auto up = [&](const std::vector<int32_t>& v) { return (const int32_t*)sc.upload(v.data(), v.size()); };
    ResizeCoef c;
    c.hb = up(hb); c.hk = up(hk); c.vb = up(vb); c.vk = up(vk); c.hks = hks; c.vks = vks;
    launch_resize_pil(src, sh, sw, sc.get<uint8_t>((size_t)sh * dw * 3), mk(dst, dtype, 1, dh, dw, 8), 0, c, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
  });
}

}  // extern "C"
