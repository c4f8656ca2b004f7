// yolox_net.hip - the YOLOX network on the conv engine: upstream's YOLOX(YOLOPAFPN(CSPDarknet), YOLOXHead) in eval mode, from the
// reference's `preprocess` output (fp32 BGR 0..255, [n][3][H][W]) to the head's undecoded rows [n][A][5 + C] that rtd_yolox_post_run
// reads with decode = 1.  The arithmetic is restated in tests/yolox_net_ref.py.
//
// Every convolution (conv + folded BatchNorm + SiLU; the pred convs plain with bias) runs through launch_conv (conv_igemm.hip) in the
// handle's precision, the fp16 hi + lo pair format (RTD_PREC_F16X3) or fp32.  Per (n, in_h, in_w) the handle caches a plan: an op list
// over one arena, tensors as byte offsets.
//   * a concatenation is never a copy: each producer writes its channel slice of the concat buffer (Tensor::slice_c) - a CSP layer's two
//     branches, SPP's four slices, the PAFPN's cat(up2(.), .) and cat(bu_conv(.), .);
//   * a Bottleneck's shortcut is the 3x3 conv's RES_POST residual;
//   * cls_pred is one conv, reg_pred and obj_pred (one input) are ONE conv of N = 5; both write fp32 rows at N padded to 32;
//   * every launch is put to conv_predict while the plan is built: a shape the launchers refuse is a refused call, never a launch.
// Four kernels are this file's own: yolox_focus (space to depth from the planar input into the trunk's storage), yolox_focus_u8 (the same
// map straight from uint8 HWC frames of any size, resized as the reference's F.interpolate does: rtd_yolox_net_run_frames), yolox_spp (the
// stride-1 max pools 5 / 9 / 13 of SPPBottleneck as three 5 x 5 passes in LDS, one launch) and yolox_head_emit (the three levels' pred
// rows -> [A][5 + C] rows with the sigmoids).  Everything is enqueued on the caller's stream; the handle owns no stream and captures nothing.
#include <math.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <tuple>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "net_plan.h"
#include "yolox_net_host.h"

namespace yolox_net {

using namespace rtd;
namespace yh = yolox_net_host;
namespace bk = rtd::backend;
namespace np = rtd::netplan;
using bk::guarded;
using np::at;
using np::based;
using np::op_dtype;

// ---------------------------------------------------------------------------------------------------------------- kernels
// the store of one Focus output pixel: v[0..11] and zeros above into its 32-channel group, fp32 or hi + lo pairs.  yolox_focus and
// yolox_focus_u8 both end here, so equal values are equal storage bits.
template <bool PAIR>
__device__ __forceinline__ void focus_store(void* __restrict__ y, int64_t i, const float (&v)[16]) {
  if (PAIR) {
    sp16* q = (sp16*)y + i * (2 * yh::FOCUS_C);
    const sp16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      sp16x8 hi, lo;
#pragma unroll
      for (int k = 0; k < 8; ++k) { sp16 a, c; split2(v[8 * g + k], a, c); hi[k] = a; lo[k] = c; }
      *(sp16x8*)(q + 8 * g) = hi;
      *(sp16x8*)(q + SPLIT_GROUP + 8 * g) = lo;
    }
#pragma unroll
    for (int g = 2; g < 4; ++g) { *(sp16x8*)(q + 8 * g) = zero; *(sp16x8*)(q + SPLIT_GROUP + 8 * g) = zero; }
  } else {
    float* q = (float*)y + i * yh::FOCUS_C;
#pragma unroll
    for (int g = 0; g < 4; ++g) *(f32x4*)(q + 4 * g) = f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
#pragma unroll
    for (int g = 4; g < 8; ++g) *(f32x4*)(q + 4 * g) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// Focus: one thread per OUTPUT pixel.  The two pixels (2 ox, 2 ox + 1) of an input row are one 8-byte load, so a wave reads 512
// consecutive bytes of each of the six rows (3 channels x 2 rows) it touches; the thread then writes its pixel's whole 128-byte channel
// group: channel 3 k + c from quadrant k (top-left, bottom-left, top-right, bottom-right), zeros in 12..31.
template <bool PAIR>
__global__ void __launch_bounds__(256) yolox_focus(const float* __restrict__ x, int n, int H, int W, void* __restrict__ y) {
  const int OH = H >> 1, OW = W >> 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * OH * OW) return;
  const int ox = (int)(i % OW);
  const int64_t t = i / OW;
  const int oy = (int)(t % OH), b = (int)(t / OH);
  float v[16];
#pragma unroll
  for (int k = 12; k < 16; ++k) v[k] = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = x + (((int64_t)b * 3 + c) * H + 2 * oy) * W + 2 * ox;
    const float2 top = *(const float2*)p, bot = *(const float2*)(p + W);
    v[c] = top.x; v[3 + c] = bot.x; v[6 + c] = top.y; v[9 + c] = bot.y;
  }
  focus_store<PAIR>(y, i, v);
}

// The uint8 front end: Focus of the resized frame, from the frames themselves.  One thread per OUTPUT pixel, as yolox_focus: it resamples the
// 2 x 2 block of resized pixels (2 oy + r, 2 ox + q) x 3 channels with the rule of yolox_net_host.h (frame_tap, frame_blend: bilinear,
// align_corners = False, each operation one fp32 rounding) and stores its whole 128-byte group.  Frames lie at any byte address and a
// pixel is 3 bytes, so no wider load is ever aligned: every tap is a byte load.  Neighbouring threads read neighbouring spans of the same
// source rows, which the vector L1 serves from the same lines; the kernel's traffic is the Focus map it writes (128 bytes per thread
// against at most 48 source bytes).  Per-frame descriptors travel as the kernel's argument, as CropBatch does.
struct FrameBatch {
  const uint8_t* p[yh::MAX_BATCH];   // contiguous HWC uint8 BGR frames on the device
  int h[yh::MAX_BATCH], w[yh::MAX_BATCH];
  float sy[yh::MAX_BATCH], sx[yh::MAX_BATCH];   // frame_scale(h, in_h), frame_scale(w, in_w)
};
template <bool PAIR>
__global__ void __launch_bounds__(256) yolox_focus_u8(const FrameBatch fb, int n, int H, int W, void* __restrict__ y) {
  const int OH = H >> 1, OW = W >> 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * OH * OW) return;
  const int ox = (int)(i % OW);
  const int64_t t = i / OW;
  const int oy = (int)(t % OH), b = (int)(t / OH);
  const uint8_t* __restrict__ f = fb.p[b];
  const int h = fb.h[b], w = fb.w[b];
  const float sy = fb.sy[b], sx = fb.sx[b];
  yh::FrameTap ty[2], tx[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) ty[r] = yh::frame_tap(sy, 2 * oy + r, h), tx[r] = yh::frame_tap(sx, 2 * ox + r, w);
  float v[16];
#pragma unroll
  for (int k = 12; k < 16; ++k) v[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                    // quadrant k: row 2 oy + (k & 1), column 2 ox + (k >> 1)
    const yh::FrameTap& ry = ty[k & 1];
    const yh::FrameTap& cx = tx[k >> 1];
    const uint8_t* r0 = f + (int64_t)ry.i0 * w * 3;
    const uint8_t* r1 = f + (int64_t)ry.i1 * w * 3;
    const int x0 = cx.i0 * 3, x1 = cx.i1 * 3;      // (at most 3 * 16383)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[3 * k + c] = yh::frame_blend(ry, cx, (float)r0[x0 + c], (float)r0[x1 + c], (float)r1[x0 + c], (float)r1[x1 + c]);
  }
  focus_store<PAIR>(y, i, v);
}

// SPP: MaxPool2d(k, stride 1, padding k / 2) for k = 5, 9, 13 of channel slice 0 of the [n][h][w][4 cs] concat buffer into slices 1, 2, 3.
// The padding never wins, so pool9 = pool5 o pool5 and pool13 = pool5 o pool5 o pool5 exactly.  A workgroup owns SPP_CH channels of one
// SPP_TILE^2 tile: it stages the tile with a halo of 6 as fp32 in LDS (pixels outside the map: -inf; a pair value hi + lo is exact in
// fp32, and re-splitting the winner reproduces its pair, as k_maxpool does), then runs the separable 5-tap row and column maxima three
// times over the whole staged region and stores the tile's core after each pass.  What a pass computes near the region's edge lacks
// taps from outside the region; that error moves inwards by 2 pixels per pass and reaches, after three, exactly the 6-pixel halo.
template <bool PAIR>
__global__ void __launch_bounds__(yh::SPP_THREADS) yolox_spp(void* __restrict__ buf, int h, int w, int cs, int64_t ld, int tiles_x, int tiles_y) {
  constexpr int R = yh::SPP_REGION, CH = yh::SPP_CH, T = yh::SPP_TILE, HALO = yh::SPP_HALO, NT = yh::SPP_THREADS;
  __shared__ float sa[R * R * CH], sb[R * R * CH];
  const int chunks = cs / CH;
  int64_t bi = blockIdx.x;
  const int chunk = (int)(bi % chunks); bi /= chunks;
  const int tx = (int)(bi % tiles_x); bi /= tiles_x;
  const int ty = (int)(bi % tiles_y);
  const int64_t img = bi / tiles_y;
  const int c0 = chunk * CH, x0 = tx * T - HALO, y0 = ty * T - HALO;
  const int64_t img_pix = img * h * (int64_t)w;

  for (int p = threadIdx.x; p < R * R; p += NT) {
    const int ry = p / R, rx = p - ry * R, gy = y0 + ry, gx = x0 + rx;
    float v[CH];
    if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) {
      const int64_t off = (img_pix + (int64_t)gy * w + gx) * ld;
      if (PAIR) {
        split_load8((const sp16*)buf, off, c0, v);
      } else {
        const float* q = (const float*)buf + off + c0;
        const f32x4 a = *(const f32x4*)q, b = *(const f32x4*)(q + 4);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
      }
    } else {
#pragma unroll
      for (int k = 0; k < CH; ++k) v[k] = -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) sa[p * CH + k] = v[k];
  }
  __syncthreads();

  for (int pass = 1; pass <= 3; ++pass) {
    for (int i = threadIdx.x; i < R * R * CH; i += NT) {          // rows: sb = max over x - 2 .. x + 2 of sa
      const int p = i / CH, rx = p % R;
      float m = sa[i];
#pragma unroll
      for (int d = 1; d <= 2; ++d) {
        if (rx - d >= 0) m = fmaxf(m, sa[i - d * CH]);
        if (rx + d < R) m = fmaxf(m, sa[i + d * CH]);
      }
      sb[i] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * R * CH; i += NT) {          // columns: sa = max over y - 2 .. y + 2 of sb
      const int p = i / CH, ry = p / R;
      float m = sb[i];
#pragma unroll
      for (int d = 1; d <= 2; ++d) {
        if (ry - d >= 0) m = fmaxf(m, sb[i - d * R * CH]);
        if (ry + d < R) m = fmaxf(m, sb[i + d * R * CH]);
      }
      sa[i] = m;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < T * T; p += NT) {               // the tile's core -> slice `pass`
      const int cy = p / T, cx = p - cy * T, gy = ty * T + cy, gx = tx * T + cx;
      if (gy >= h || gx >= w) continue;
      const float* s = sa + ((cy + HALO) * R + cx + HALO) * CH;
      float v[CH];
#pragma unroll
      for (int k = 0; k < CH; ++k) v[k] = s[k];
      const int64_t off = (img_pix + (int64_t)gy * w + gx) * ld;
      const int c = pass * cs + c0;
      if (PAIR) {
        split_store8((sp16*)buf, off, c, v);
      } else {
        float* q = (float*)buf + off + c;
        *(f32x4*)q = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)(q + 4) = f32x4{v[4], v[5], v[6], v[7]};
      }
    }
    // (the stores read sa, the next pass's row step only reads sa too: no barrier needed before it; its column step writes sa after
    // the barrier that follows the row step)
  }
}

// 1 / (1 + exp(-v)), every operation rounded on its own (see discrete_tap in common.h on `fp contract(off)`)
__device__ __forceinline__ float sigmoid_plain(float v) {
#pragma clang fp contract(off)
  const float e = expf(-v);
  const float d = 1.f + e;
  return 1.f / d;
}

// Head emit: one thread per float of pred [n][A][F], F = 5 + C: dword stores, consecutive lanes on consecutive addresses
struct EmitArgs {
  const float* cls[yh::LEVELS];      // [n][h_l w_l][cls_ld]
  const float* regobj[yh::LEVELS];   // [n][h_l w_l][regobj_ld]: 4 box terms, obj
  int64_t off[yh::LEVELS + 1];       // first row of each level; off[3] = A
  int cls_ld, regobj_ld, F;
  int64_t total;                     // n * A * F
  float* pred;
};
__global__ void __launch_bounds__(256) yolox_head_emit(EmitArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.total) return;
  const int j = (int)(i % a.F);
  const int64_t row = i / a.F, A = a.off[yh::LEVELS];
  const int64_t b = row / A, r = row - b * A;
  const int l = r >= a.off[2] ? 2 : (r >= a.off[1] ? 1 : 0);
  const int64_t pix = b * (a.off[l + 1] - a.off[l]) + (r - a.off[l]);
  float v;
  if (j < 4) v = a.regobj[l][pix * a.regobj_ld + j];
  else if (j == 4) v = sigmoid_plain(a.regobj[l][pix * a.regobj_ld + 4]);
  else v = sigmoid_plain(a.cls[l][pix * a.cls_ld + (j - 5)]);
  a.pred[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- launchers
static void launch_focus(int dt, const float* x, void* y, int n, int H, int W, hipStream_t s) {
  const int64_t total = (int64_t)n * (H / 2) * (W / 2);
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (dt == F16X2) rtd_launch(yolox_focus<true>, grid, blk, 0, s, x, n, H, W, y);
  else rtd_launch(yolox_focus<false>, grid, blk, 0, s, x, n, H, W, y);
  HIP_CHECK(hipGetLastError());
}
// frames / frame_hw: the caller's host arrays, already through yh::check_frames
static void launch_focus_u8(int dt, const uint8_t* const* frames, const int32_t* frame_hw, void* y, int n, int H, int W, hipStream_t s) {
  FrameBatch fb;
  memset(&fb, 0, sizeof fb);
  for (int i = 0; i < n; ++i) {
    fb.p[i] = frames[i], fb.h[i] = frame_hw[2 * i], fb.w[i] = frame_hw[2 * i + 1];
    fb.sy[i] = yh::frame_scale(fb.h[i], H), fb.sx[i] = yh::frame_scale(fb.w[i], W);
  }
  const int64_t total = (int64_t)n * (H / 2) * (W / 2);
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (dt == F16X2) rtd_launch(yolox_focus_u8<true>, grid, blk, 0, s, fb, n, H, W, y);
  else rtd_launch(yolox_focus_u8<false>, grid, blk, 0, s, fb, n, H, W, y);
  HIP_CHECK(hipGetLastError());
}
// t: the concat buffer's slice 0 view (c = the slice's channels, ld = 4 c)
static void launch_spp(const Tensor& t, hipStream_t s) {
  RTD_CHECK((t.dt == F32 || t.dt == F16X2) && t.n >= 1 && t.h >= 1 && t.w >= 1 && t.c >= yh::SPP_CH, RTD_E_INVALID, "spp: fp32 or pair tensors of at least 1 x 1");
  RTD_CHECK(t.c % (t.dt == F16X2 ? SPLIT_GROUP : yh::SPP_CH) == 0 && t.ld == 4 * (int64_t)t.c && aligned16(t.p), RTD_E_INVALID,
            "spp: slices of whole 8-channel chunks (pair tensors: 32-channel groups) in a 16-byte aligned 4-slice buffer");
  const yh::SppGrid g = yh::spp_grid(t.n, t.h, t.w, t.c);
  RTD_CHECK(g.blocks < ((int64_t)1 << 31), RTD_E_INVALID, "spp: too many tiles for one launch");
  const dim3 grid((unsigned)g.blocks), blk(yh::SPP_THREADS);
  if (t.dt == F16X2) rtd_launch(yolox_spp<true>, grid, blk, 0, s, t.p, t.h, t.w, t.c, t.ld, g.tiles_x, g.tiles_y);
  else rtd_launch(yolox_spp<false>, grid, blk, 0, s, t.p, t.h, t.w, t.c, t.ld, g.tiles_x, g.tiles_y);
  HIP_CHECK(hipGetLastError());
}
static void launch_emit(const EmitArgs& a, hipStream_t s) {
  RTD_CHECK((a.total + 255) / 256 < ((int64_t)1 << 31), RTD_E_INVALID, "head emit: too many rows for one launch");
  rtd_launch(yolox_head_emit, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------- plan
enum OpKind { OP_CONV, OP_UPSAMPLE, OP_SPP };
// (tensors of an op are arena offsets: net_plan.h)
struct Op {
  int kind = OP_CONV;
  ConvArgs conv;          // OP_CONV (x, y, res as offsets)
  Tensor a, y;            // OP_UPSAMPLE: a -> y; OP_SPP: a = slice 0 of the concat buffer
};
struct Plan : np::PlanBase {
  int n = 0, h = 0, w = 0;
  Tensor in;              // the Focus output
  Tensor cls_rows[yh::LEVELS], regobj_rows[yh::LEVELS];
  std::vector<Op> ops;
  std::map<std::string, Tensor> stages;
};

}  // namespace yolox_net

struct rtd_yolox_net : rtd::netplan::NetBase {
  rtd_yolox_net_config cfg;
  std::map<std::tuple<int, int, int>, std::unique_ptr<yolox_net::Plan>> plans;
  yolox_net::Plan* last_plan = nullptr;   // rtd_debug_yolox_tensor reads its stages
};

namespace yolox_net {

// One pass over the network.  Named stage outputs and everything a later layer reads live in the persistent part of the arena; a CSP
// layer's and a head branch's temporaries come from a scratch region at the arena's start that every such unit uses again.  The scratch
// region's size is known after a first pass (scratch = 0: nothing of it is kept), the plan is the second.
struct Builder {
  rtd_yolox_net* e;
  Plan* p;
  int n, P;
  np::Arena keep;            // the persistent part: it starts where the scratch region ends
  np::Arena scratch;         // reset by every unit that uses it
  size_t s_max = 0, slab = 0;

  Tensor alloc(int h, int w, int c, int dt) { return keep.tensor(dt, n, h, w, c); }
  Tensor salloc(int h, int w, int c) { const Tensor t = scratch.tensor(P, n, h, w, c); s_max = std::max(s_max, scratch.top); return t; }
  void stage(const std::string& name, const Tensor& t) { p->stages[name] = t; }

  void conv(const yh::ConvDesc& d, const Tensor& x, const Tensor& y, int act, const Tensor* res) {
    Op op;
    op.kind = OP_CONV;
    ConvArgs& a = op.conv;
    a = conv_args(x, y, e->filters.at(d.name), d.k, d.stride, (d.k - 1) / 2, act);
    np::plan_conv(a, &e->conv_opts, res, RES_POST, slab, d.name + " at " + std::to_string(n) + " x " + std::to_string(x.h) + " x " + std::to_string(x.w));
    p->ops.push_back(op);
  }
};

struct Net {
  Builder& b;
  const std::vector<yh::ConvDesc>& table;
  size_t next = 0;   // the table is in execution order: every conv() takes the next entry and checks its name's tail
  const yh::ConvDesc& take(const std::string& tail) {
    RTD_CHECK(next < table.size(), RTD_E_STATE, "plan: conv table exhausted at " + tail);
    const yh::ConvDesc& d = table[next++];
    RTD_CHECK(d.name.size() >= tail.size() && d.name.compare(d.name.size() - tail.size(), tail.size(), tail) == 0, RTD_E_STATE,
              "plan: expected " + tail + ", the table has " + d.name);
    return d;
  }
  void base_conv(const std::string& tail, const Tensor& x, const Tensor& y, const Tensor* res = nullptr) { b.conv(take(tail), x, y, ACT_SILU, res); }

  // CSPLayer: y = conv3(cat(m(conv1(x)), conv2(x))), m = n Bottlenecks (1x1, then 3x3 with the shortcut as its RES_POST residual)
  void csp(const std::string& tail, const Tensor& x, const Tensor& y, int n, bool shortcut) {
    const int h = y.c / 2;
    b.scratch.top = 0;
    const Tensor cat = b.salloc(x.h, x.w, 2 * h), A = b.salloc(x.h, x.w, h), B = b.salloc(x.h, x.w, h), T = b.salloc(x.h, x.w, h);
    base_conv(tail + ".conv1", x, A);
    base_conv(tail + ".conv2", x, cat.slice_c(h, h));
    Tensor cur = A;
    for (int i = 0; i < n; ++i) {
      const std::string m = tail + ".m." + std::to_string(i);
      const Tensor dst = i == n - 1 ? cat.slice_c(0, h) : (cur.p == A.p ? B : A);
      base_conv(m + ".conv1", cur, T);
      base_conv(m + ".conv2", T, dst, shortcut ? &cur : nullptr);
      cur = dst;
    }
    base_conv(tail + ".conv3", cat, y);
  }
  void upsample(const Tensor& a, const Tensor& y) { Op op; op.kind = OP_UPSAMPLE; op.a = a; op.y = y; b.p->ops.push_back(op); }

  void build(int H, int W) {
    const rtd_yolox_net_config& c = b.e->cfg;
    const int P = b.P, base = c.base_channels, d = c.depth;
    const int c3 = 4 * base, c4 = 8 * base, c5 = 16 * base, hc = 4 * base;
    int hh[6], ww[6];                                      // extents at stride 2^k
    for (int k = 0; k < 6; ++k) hh[k] = H >> k, ww[k] = W >> k;
    Plan* p = b.p;
    p->in = b.alloc(hh[1], ww[1], yh::FOCUS_C, P);
    b.stage("focus", p->in);
    // ---- CSPDarknet
    const Tensor stem = b.alloc(hh[1], ww[1], base, P);
    base_conv("stem.conv", p->in, stem);
    b.stage("stem", stem);
    const Tensor p3cat = b.alloc(hh[3], ww[3], 2 * c3, P), p4cat = b.alloc(hh[4], ww[4], 2 * c4, P);      // cat(up2(.), dark3 / dark4)
    const Tensor n3cat = b.alloc(hh[4], ww[4], 2 * c3, P), n4cat = b.alloc(hh[5], ww[5], 2 * c4, P);      // cat(bu_conv(.), fpn_out1 / fpn_out0)
    const Tensor dark2 = b.alloc(hh[2], ww[2], 2 * base, P), dark3 = p3cat.slice_c(c3, c3), dark4 = p4cat.slice_c(c4, c4);
    const Tensor dark5 = b.alloc(hh[5], ww[5], c5, P);
    Tensor x = stem;
    const Tensor outs[3] = {dark2, dark3, dark4};
    for (int s = 0; s < 3; ++s) {
      const std::string dn = "dark" + std::to_string(s + 2);
      const Tensor down = b.alloc(hh[s + 2], ww[s + 2], base << (s + 1), P);
      base_conv(dn + ".0", x, down);
      csp(dn + ".1", down, outs[s], s == 0 ? d : 3 * d, true);
      b.stage(dn, outs[s]);
      x = outs[s];
    }
    {
      const Tensor down = b.alloc(hh[5], ww[5], c5, P), sppcat = b.alloc(hh[5], ww[5], 2 * c5, P), spp = b.alloc(hh[5], ww[5], c5, P);
      base_conv("dark5.0", x, down);
      base_conv("dark5.1.conv1", down, sppcat.slice_c(0, c5 / 2));
      { Op op; op.kind = OP_SPP; op.a = sppcat.slice_c(0, c5 / 2); p->ops.push_back(op); }
      base_conv("dark5.1.conv2", sppcat, spp);
      b.stage("spp", spp);
      csp("dark5.2", spp, dark5, d, false);
      b.stage("dark5", dark5);
    }
    // ---- PAFPN
    const Tensor fpn_out0 = n4cat.slice_c(c4, c4), fpn_out1 = n3cat.slice_c(c3, c3);
    const Tensor f0 = b.alloc(hh[4], ww[4], c4, P), pan_out2 = b.alloc(hh[3], ww[3], c3, P), pan_out1 = b.alloc(hh[4], ww[4], c4, P);
    const Tensor pan_out0 = b.alloc(hh[5], ww[5], c5, P);
    base_conv("lateral_conv0", dark5, fpn_out0);
    upsample(fpn_out0, p4cat.slice_c(0, c4));
    csp("C3_p4", p4cat, f0, d, false);
    base_conv("reduce_conv1", f0, fpn_out1);
    upsample(fpn_out1, p3cat.slice_c(0, c3));
    csp("C3_p3", p3cat, pan_out2, d, false);
    base_conv("bu_conv2", pan_out2, n3cat.slice_c(0, c3));
    csp("C3_n3", n3cat, pan_out1, d, false);
    base_conv("bu_conv1", pan_out1, n4cat.slice_c(0, c4));
    csp("C3_n4", n4cat, pan_out0, d, false);
    b.stage("fpn_out0", fpn_out0); b.stage("fpn_out1", fpn_out1);
    b.stage("pan_out2", pan_out2); b.stage("pan_out1", pan_out1); b.stage("pan_out0", pan_out0);
    // ---- decoupled head
    const Tensor lv[yh::LEVELS] = {pan_out2, pan_out1, pan_out0};
    const int cls_c = yh::pad32(c.num_classes), ro_c = yh::pad32(yh::PRED_REGOBJ);
    for (int l = 0; l < yh::LEVELS; ++l) {
      const std::string s = std::to_string(l);
      const int lh = hh[l + 3], lw = ww[l + 3];
      const Tensor st = b.alloc(lh, lw, hc, P), cf = b.alloc(lh, lw, hc, P), rf = b.alloc(lh, lw, hc, P);
      p->cls_rows[l] = b.alloc(lh, lw, cls_c, F32);
      p->regobj_rows[l] = b.alloc(lh, lw, ro_c, F32);
      b.scratch.top = 0;
      const Tensor t = b.salloc(lh, lw, hc);
      base_conv("stems." + s, lv[l], st);
      base_conv("cls_convs." + s + ".0", st, t);
      base_conv("cls_convs." + s + ".1", t, cf);
      base_conv("reg_convs." + s + ".0", st, t);
      base_conv("reg_convs." + s + ".1", t, rf);
      b.conv(take("cls_preds." + s), cf, p->cls_rows[l], ACT_NONE, nullptr);
      b.conv(take("regobj_preds." + s), rf, p->regobj_rows[l], ACT_NONE, nullptr);
      b.stage("stem_" + s, st); b.stage("cls_feat_" + s, cf); b.stage("reg_feat_" + s, rf);
      b.stage("cls_rows_" + s, p->cls_rows[l]); b.stage("regobj_rows_" + s, p->regobj_rows[l]);
    }
    RTD_CHECK(next == table.size(), RTD_E_STATE, "plan: the conv table has entries the plan did not use");
  }
};

static std::unique_ptr<Plan> build_plan(rtd_yolox_net* e, int n, int h, int w) {
  const std::vector<yh::ConvDesc> table = yh::conv_table(e->cfg.base_channels, e->cfg.depth, e->cfg.num_classes);
  size_t scratch = 0;
  std::unique_ptr<Plan> p;
  for (int pass = 0; pass < 2; ++pass) {
    p = std::make_unique<Plan>();
    p->n = n, p->h = h, p->w = w;
    Builder b{e, p.get(), n, e->P, np::Arena{scratch}};
    Net net{b, table};
    net.build(h, w);
    scratch = b.s_max;
    p->seal(b.keep.top, b.slab);
  }
  return p;
}

static Plan* get_plan(rtd_yolox_net* e, int n, int h, int w) {
  return np::get_or_build(e->plans, std::make_tuple(n, h, w), 64, [&] { return build_plan(e, n, h, w); });
}

static void run_op(rtd_yolox_net* e, const Plan* p, const Op& op, hipStream_t s) {
  char* base = (char*)e->arena.p;
  switch (op.kind) {
    case OP_CONV: np::run_conv(op.conv, base, *p, s); break;
    case OP_UPSAMPLE: launch_upsample2x(based(op.a, base), based(op.y, base), s); break;
    default: launch_spp(based(op.a, base), s);
  }
}

static EmitArgs emit_args(const float* const cls[3], const float* const regobj[3], int cls_ld, int regobj_ld, int n, int in_h, int in_w, int num_classes,
                          float* pred) {
  EmitArgs a;
  int lh[yh::LEVELS], lw[yh::LEVELS];
  yh::level_offsets(in_h, in_w, a.off, lh, lw);
  for (int l = 0; l < yh::LEVELS; ++l) a.cls[l] = cls[l], a.regobj[l] = regobj[l];
  a.cls_ld = cls_ld, a.regobj_ld = regobj_ld, a.F = 5 + num_classes;
  a.total = (int64_t)n * a.off[yh::LEVELS] * a.F;
  a.pred = pred;
  return a;
}

// the checked call, whichever front end: `fill(focus)` launches the kernel that writes the plan's `in` tensor, the rest is the plan
template <typename Fill>
static void run_plan(rtd_yolox_net* e, int n, int in_h, int in_w, float* pred, hipStream_t s, Fill&& fill) {
  HIP_CHECK(hipSetDevice(e->device));
  e->last_plan = nullptr;                                          // (get_plan may empty the cache it points into)
  Plan* p = get_plan(e, n, in_h, in_w);                            // (a shape the conv launchers refuse throws here)
  e->arena.reserve(p->bytes);
  char* base = (char*)e->arena.p;
  fill((void*)(base + (size_t)p->in.p));
  for (const Op& op : p->ops) run_op(e, p, op, s);
  const float* cls[yh::LEVELS];
  const float* ro[yh::LEVELS];
  for (int l = 0; l < yh::LEVELS; ++l) cls[l] = (const float*)(base + (size_t)p->cls_rows[l].p), ro[l] = (const float*)(base + (size_t)p->regobj_rows[l].p);
  launch_emit(emit_args(cls, ro, (int)p->cls_rows[0].ld, (int)p->regobj_rows[0].ld, n, in_h, in_w, e->cfg.num_classes, pred), s);
  e->last_plan = p, e->last_stream = s;
}
// every argument is checked before anything is allocated or launched
static void run(rtd_yolox_net* e, int n, const float* in, int in_h, int in_w, float* pred, hipStream_t s) {
  yh::check_run(e->cfg, n, in, in_h, in_w, pred);
  run_plan(e, n, in_h, in_w, pred, s, [&](void* focus) { launch_focus(e->P, in, focus, n, in_h, in_w, s); });
}
static void run_frames(rtd_yolox_net* e, int n, const uint8_t* const* frames, const int32_t* frame_hw, int in_h, int in_w, float* pred, hipStream_t s) {
  yh::check_run_frames(e->cfg, n, frames, frame_hw, in_h, in_w, pred);
  run_plan(e, n, in_h, in_w, pred, s, [&](void* focus) { launch_focus_u8(e->P, frames, frame_hw, focus, n, in_h, in_w, s); });
}

// The filters (net_plan.h: upload_filters): the blob's rows [cout][k k cin] are launch_conv's filter rows as they are
static void upload_weights(rtd_yolox_net* e, const std::map<std::string, yh::HostTensor>& host, const std::vector<yh::ConvDesc>& table) {
  std::vector<np::FilterSpec> specs;
  for (const yh::ConvDesc& d : table) specs.push_back({d.name, conv_filter_extents(e->P, d.cout, d.k * d.k * d.cin)});
  np::upload_filters(*e, specs, [&](size_t i, std::vector<float>& rows, std::vector<float>& bias) {
    const ConvFilter& f = specs[i].f;
    rows = conv_filter_rows(f, {{host.at(table[i].name + ".weight").data, f.K}});
    memcpy(bias.data(), host.at(table[i].name + ".bias").data, (size_t)f.N * 4);
  });
}

template <typename F>
static int op_guard(F&& f) { return np::op_guard<rtd_yolox_net>(f); }

}  // namespace yolox_net

using namespace yolox_net;

extern "C" {

int rtd_yolox_net_create(const rtd_yolox_net_config* cfg, const void* blob, size_t nbytes, rtd_yolox_net_handle* out) {
  return bk::create(out, rtd_yolox_net_destroy, [&](rtd_yolox_net* e) {
    yh::check_config(cfg);
    e->cfg = *cfg;
    e->P = cfg->precision == RTD_PREC_FP32 ? F32 : F16X2;
    yh::need(blob && nbytes >= 12, RTD_E_INVALID, "empty weight blob");
    std::vector<char> copy((const char*)blob, (const char*)blob + nbytes);   // (4-byte aligned whatever the caller's pointer is)
    std::map<std::string, yh::HostTensor> host;
    yh::parse_blob(copy.data(), copy.size(), host);
    const std::vector<yh::ConvDesc> table = yh::conv_table(cfg->base_channels, cfg->depth, cfg->num_classes);
    for (const yh::ConvDesc& d : table) yh::check_conv_tensors(host, d, e->P == F16X2);   // the whole blob is checked before the device is touched
    bk::use_device(cfg->device);
    e->device = cfg->device;
    e->conv_opts = conv_opts_template();
    upload_weights(e, host, table);
  });
}

int rtd_yolox_net_run(rtd_yolox_net_handle e, int32_t n, const float* in_dev, int32_t in_h, int32_t in_w, float* pred_dev, void* stream) {
  return guarded(e, [&] { run(e, n, in_dev, in_h, in_w, pred_dev, (hipStream_t)stream); });
}

int rtd_yolox_net_run_frames(rtd_yolox_net_handle e, int32_t n, const uint8_t* const* frames_dev, const int32_t* frame_hw, int32_t in_h, int32_t in_w,
                             float* pred_dev, void* stream) {
  return guarded(e, [&] { run_frames(e, n, frames_dev, frame_hw, in_h, in_w, pred_dev, (hipStream_t)stream); });
}

int64_t rtd_yolox_net_arena_bytes(rtd_yolox_net_handle e) { return e ? e->arena_bytes() : 0; }

const char* rtd_yolox_net_last_error(rtd_yolox_net_handle e) { return bk::last_error(e); }

void rtd_yolox_net_destroy(rtd_yolox_net_handle e) {
  if (!e) return;
  e->release_device();
  delete e;
}

int rtd_debug_yolox_tensor(rtd_yolox_net_handle e, const char* name, float* out, int64_t capacity, int64_t shape[4]) {
  return guarded(e, [&] {
    RTD_CHECK(name && shape, RTD_E_INVALID, "null argument");
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_yolox_net_run call yet");
    const Plan* p = e->last_plan;
    const auto it = p->stages.find(name);
    RTD_CHECK(it != p->stages.end(), RTD_E_INVALID, std::string("unknown debug tensor ") + name);
    Tensor t = it->second;
    shape[0] = t.n, shape[1] = t.h, shape[2] = t.w, shape[3] = t.c;
    const int64_t numel = t.pixels() * t.c;
    if (!out) return;
    RTD_CHECK(capacity >= numel, RTD_E_INVALID, "debug tensor: output capacity too small");
    HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = e->last_stream;
    np::read_tensor(based(t, (char*)e->arena.p), t.pixels(), out, s);
  });
}

int rtd_debug_yolox_plan_convs(rtd_yolox_net_handle e, char* out, int64_t capacity, int64_t* needed) {
  return guarded(e, [&] {
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_yolox_net_run call yet");
    std::vector<std::string> names;      // (Net::take walks the same table: the i-th conv of a plan is its i-th entry)
    for (const yh::ConvDesc& d : yh::conv_table(e->cfg.base_channels, e->cfg.depth, e->cfg.num_classes)) names.push_back(d.name);
    np::text_out(np::plan_convs_text(*e->last_plan, OP_CONV, names), out, capacity, needed);
  });
}

int rtd_op_yolox_focus(int dtype, const float* x, void* y, int n, int h, int w) {
  return op_guard([&] {
    RTD_CHECK(x && y && n >= 1 && n <= yh::MAX_BATCH && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && h <= 16384 && w <= 16384, RTD_E_INVALID,
              "yolox_focus: arguments (even sides of 2..16384)");
    RTD_CHECK(aligned16(x, y), RTD_E_INVALID, "yolox_focus: alignment");
    launch_focus(op_dtype(dtype), x, y, n, h, w, nullptr);
  });
}

int rtd_op_yolox_focus_u8(int dtype, const uint8_t* const* frames, const int32_t* frame_hw, int n, int in_h, int in_w, void* y) {
  return op_guard([&] {
    yh::check_frames(n, yh::MAX_BATCH, frames, frame_hw);
    RTD_CHECK(y && in_h >= 2 && in_w >= 2 && in_h % 2 == 0 && in_w % 2 == 0 && in_h <= 16384 && in_w <= 16384, RTD_E_INVALID,
              "yolox_focus_u8: arguments (even output sides of 2..16384)");
    RTD_CHECK(aligned16(y), RTD_E_INVALID, "yolox_focus_u8: alignment");
    launch_focus_u8(op_dtype(dtype), frames, frame_hw, y, n, in_h, in_w, nullptr);
  });
}

int rtd_op_yolox_spp(int dtype, void* buf, int n, int h, int w, int c) {
  return op_guard([&] {
    RTD_CHECK(buf && n >= 1 && n <= yh::MAX_BATCH && h >= 1 && w >= 1 && h <= 4096 && w <= 4096 && c >= 8 && c <= 8192, RTD_E_INVALID, "yolox_spp: arguments");
    Tensor t = at(0, op_dtype(dtype), n, h, w, 4 * c);
    t.p = buf;
    launch_spp(t.slice_c(0, c), nullptr);
  });
}

int rtd_op_yolox_head_emit(const float* const cls[3], const float* const regobj[3], int cls_ld, int regobj_ld, int n, int in_h, int in_w,
                           int num_classes, float* pred) {
  return op_guard([&] {
    RTD_CHECK(cls && regobj && pred && cls[0] && cls[1] && cls[2] && regobj[0] && regobj[1] && regobj[2], RTD_E_INVALID, "yolox_head_emit: null argument");
    RTD_CHECK(n >= 1 && n <= yh::MAX_BATCH && num_classes >= 1 && num_classes <= yh::MAX_CLASSES && cls_ld >= num_classes && regobj_ld >= yh::PRED_REGOBJ,
              RTD_E_INVALID, "yolox_head_emit: arguments");
    (void)yolox_post_host::anchors(in_h, in_w);
    RTD_CHECK(((uintptr_t)pred & 3) == 0, RTD_E_INVALID, "yolox_head_emit: pred must lie on a 4-byte boundary");
    launch_emit(emit_args(cls, regobj, cls_ld, regobj_ld, n, in_h, in_w, num_classes, pred), nullptr);
  });
}

}  // extern "C"
