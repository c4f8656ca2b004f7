// enhance.hip - Stage-2 crop enhancement on device-resident frames: the reference's ImageEnhancer.enhance_clahe_bilateral
// (src/image_enhancement.py, method "clahe"): BGR -> Lab, CLAHE on L, Lab -> BGR, bilateral filter, for up to 64 crops per call.  The
// restatement the bytes must equal, stage by stage, is tests/enhance_ref.py: integers and host-built tables (enhance_tables.h)
// everywhere except the CLAHE interpolation and the bilateral sums, which are fp32 in the order written there, with contraction off.
//
// Three launches per call, each over a work list flattened across the crops (the descriptors travel as kernel arguments, so the call
// is asynchronous on the caller's stream without a staging copy that a later call could overwrite):
//   enhance_lab_hist   one workgroup per CLAHE tile: converts the tile of the (reflect-extended) crop, stores Lab for the real pixels,
//                      histograms L in LDS (one sub-histogram per wave), clips, redistributes, scans, writes the tile's 256-byte LUT.
//                      A pixel of the extension is recomputed from its mirrored source pixel: no launch waits for another.
//   enhance_apply      one thread per pixel: blends the four LUT values, Lab -> BGR by tables, into a second scratch plane.
//   enhance_bilateral  one workgroup per 64 x 16 output tile: tile + halo in LDS as one packed dword per pixel (the reflect arithmetic
//                      runs only in tiles that touch the crop's edge), colour weights in LDS, the L1 colour distance is v_sad_u8, the
//                      radius is a template parameter so the tap loop unrolls over the disc.
#include <mutex>
#include <new>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "enhance_tables.h"

#pragma clang fp contract(off)

namespace enhance {

using rtd::Error;
namespace bk = rtd::backend;
using bk::align_up;
using bk::guarded;

constexpr int THREADS = 256;
constexpr int MAX_CROPS = bk::MAX_CROPS, MAX_TILES = 16, MAX_RADIUS = 7, MIN_SIDE = 16;
constexpr int BIL_W = 64, BIL_H = 16;                         // output tile of the bilateral kernel
constexpr int BIL_ROWS = BIL_W * BIL_H / THREADS;             // 4: thread t owns column t % 64 of rows t / 64 + 4 k
constexpr int BIL_STEP = THREADS / BIL_W;
constexpr int64_t CROP_ALIGN = 256;                           // the packing rule of rtd_enhance_layout

struct CropDesc {            // 40 bytes
  const uint8_t* src;        // the crop's first pixel inside its frame
  int64_t off;               // byte offset of the crop in the output and in both scratch planes (rtd_enhance_layout)
  int pitch;                 // bytes per frame row
  int w, h;
  int tw, th;                // CLAHE tile (of the extended crop)
  int clip;                  // 0 = no clipping
};

struct EnhArgs {             // by value: 64 x 40 + 65 x 4 + 4 bytes of kernel arguments
  CropDesc c[MAX_CROPS];
  int first[MAX_CROPS + 1];  // first workgroup of every crop in this launch's flattened list
  int n;
};

struct LabConsts {
  int C[9], Ci[9];
  int fmin;
};

__device__ __forceinline__ int reflect101(int i, int n) {     // any i, n >= 2
  const int p = 2 * (n - 1);
  i %= p;
  i = i < 0 ? i + p : i;
  return i >= n ? p - i : i;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ int crop_of(const EnhArgs& a, int blk) {
  int c = 0;
  while (c + 1 < a.n && a.first[c + 1] <= blk) ++c;
  return c;
}

// ---------------------------------------------------------------------------------------------------------------- launch 1
__global__ void __launch_bounds__(THREADS) enhance_lab_hist(EnhArgs a, LabConsts k, const uint16_t* __restrict__ gtab, const uint16_t* __restrict__ ctab,
                                                            uint8_t* __restrict__ lab, uint8_t* __restrict__ luts, int tiles_x, int tiles) {
  __shared__ int hist[THREADS / 64][256];
  __shared__ int scan[256];
  __shared__ int clipped;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int crop = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const CropDesc d = a.c[crop];
  const int tx = tile % tiles_x, ty = tile / tiles_x;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) hist[w][tid] = 0;
  if (tid == 0) clipped = 0;
  __syncthreads();

  const int area = d.tw * d.th;
  uint8_t* const dst = lab + d.off;
  for (int i = tid; i < area; i += THREADS) {
    const int ey = ty * d.th + i / d.tw, ex = tx * d.tw + i % d.tw;
    const int sy = ey < d.h ? ey : reflect101(ey, d.h), sx = ex < d.w ? ex : reflect101(ex, d.w);
    const uint8_t* p = d.src + (size_t)sy * d.pitch + sx * 3;
    const int B = gtab[p[0]], G = gtab[p[1]], R = gtab[p[2]];
    const int fX = ctab[(R * k.C[0] + G * k.C[1] + B * k.C[2] + (1 << (LAB_SHIFT - 1))) >> LAB_SHIFT];
    const int fY = ctab[(R * k.C[3] + G * k.C[4] + B * k.C[5] + (1 << (LAB_SHIFT - 1))) >> LAB_SHIFT];
    const int fZ = ctab[(R * k.C[6] + G * k.C[7] + B * k.C[8] + (1 << (LAB_SHIFT - 1))) >> LAB_SHIFT];
    constexpr int RND = 1 << (LAB_SHIFT2 - 1);
    const int L = clamp255((296 * fY - (16 * 255 * (1 << LAB_SHIFT2) + 50) / 100 + RND) >> LAB_SHIFT2);
    const int A = clamp255((500 * (fX - fY) + 128 * (1 << LAB_SHIFT2) + RND) >> LAB_SHIFT2);
    const int Bb = clamp255((200 * (fY - fZ) + 128 * (1 << LAB_SHIFT2) + RND) >> LAB_SHIFT2);
    if (ex < d.w && ey < d.h) {
      uint8_t* q = dst + ((size_t)ey * d.w + ex) * 3;
      q[0] = (uint8_t)L, q[1] = (uint8_t)A, q[2] = (uint8_t)Bb;
    }
    atomicAdd(&hist[wave][L], 1);
  }
  __syncthreads();

  // ---- one thread per bin: clip, redistribute, scan, LUT
  int hv = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) hv += hist[w][tid];
  if (d.clip > 0 && hv > d.clip) {
    atomicAdd(&clipped, hv - d.clip);
    hv = d.clip;
  }
  __syncthreads();
  if (d.clip > 0) {
    const int total = clipped;
    hv += total / 256;
    const int residual = total % 256;
    if (residual != 0) {
      const int step = max(256 / residual, 1);
      if (tid % step == 0 && tid / step < residual) ++hv;
    }
  }
  scan[tid] = hv;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const float lut_scale = 255.0f / (float)area;
  luts[((size_t)crop * tiles + tile) * 256 + tid] = (uint8_t)clamp255((int)rintf((float)scan[tid] * lut_scale));
}

// ---------------------------------------------------------------------------------------------------------------- launch 2
__global__ void __launch_bounds__(THREADS) enhance_apply(EnhArgs a, LabConsts k, const int32_t* __restrict__ t_l, const int32_t* __restrict__ t_a,
                                                         const int32_t* __restrict__ t_b, const int32_t* __restrict__ finv, const uint8_t* __restrict__ gi,
                                                         const uint8_t* __restrict__ lab, const uint8_t* __restrict__ luts, uint8_t* __restrict__ bgr,
                                                         int tiles_x, int tiles_y) {
  const int crop = crop_of(a, blockIdx.x);
  const CropDesc d = a.c[crop];
  const int p = (blockIdx.x - a.first[crop]) * THREADS + threadIdx.x;
  if (p >= d.w * d.h) return;
  const int y = p / d.w, x = p % d.w;
  const uint8_t* q = lab + d.off + (size_t)p * 3;
  const int v = q[0];

  const float txf = (float)x * (1.0f / (float)d.tw) - 0.5f, tyf = (float)y * (1.0f / (float)d.th) - 0.5f;
  const float fx1 = floorf(txf), fy1 = floorf(tyf);
  const float xa = txf - fx1, ya = tyf - fy1;
  const float xa1 = 1.0f - xa, ya1 = 1.0f - ya;
  const int tx1 = min(max((int)fx1, 0), tiles_x - 1), tx2 = min((int)fx1 + 1, tiles_x - 1);      // (the upper clamp of tx1 never acts: x < extended width)
  const int ty1 = min(max((int)fy1, 0), tiles_y - 1), ty2 = min((int)fy1 + 1, tiles_y - 1);
  const uint8_t* lut = luts + (size_t)crop * tiles_x * tiles_y * 256 + v;
  const float l11 = (float)lut[(ty1 * tiles_x + tx1) * 256], l12 = (float)lut[(ty1 * tiles_x + tx2) * 256];
  const float l21 = (float)lut[(ty2 * tiles_x + tx1) * 256], l22 = (float)lut[(ty2 * tiles_x + tx2) * 256];
  const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
  const int L = clamp255((int)rintf(res));

  const int fy = t_l[L];
  const int fx = fy + t_a[q[1]], fz = fy - t_b[q[2]];
  const int X = finv[fx - k.fmin], Y = finv[fy - k.fmin], Z = finv[fz - k.fmin];
  uint8_t* o = bgr + d.off + (size_t)p * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int r = 2 - c;                                          // B from row 2, G from row 1, R from row 0
    const int lin = (k.Ci[3 * r] * X + k.Ci[3 * r + 1] * Y + k.Ci[3 * r + 2] * Z + (1 << (INV_Q - 1))) >> INV_Q;
    o[c] = gi[min(max(lin, 0), INV_S)];
  }
}

// ---------------------------------------------------------------------------------------------------------------- launch 3
template <int R>
__global__ void __launch_bounds__(THREADS) enhance_bilateral(EnhArgs a, const float* __restrict__ space_w, const float* __restrict__ color_w,
                                                             const uint8_t* __restrict__ bgr, uint8_t* __restrict__ out) {
  constexpr int LW = BIL_W + 2 * R, LH = BIL_H + 2 * R, D = 2 * R + 1;
  __shared__ uint32_t px[LH * LW];
  __shared__ float cw[COLOR_W];
  __shared__ float sw[D * D];
  const int tid = threadIdx.x;
  const int crop = crop_of(a, blockIdx.x);
  const CropDesc d = a.c[crop];
  const int t = blockIdx.x - a.first[crop];
  const int tiles_x = (d.w + BIL_W - 1) / BIL_W;
  const int X0 = (t % tiles_x) * BIL_W, Y0 = (t / tiles_x) * BIL_H;
  const uint8_t* src = bgr + d.off;
  const bool inner = X0 >= R && Y0 >= R && X0 + BIL_W + R <= d.w && Y0 + BIL_H + R <= d.h;     // no pixel of tile + halo leaves the crop
  for (int i = tid; i < LH * LW; i += THREADS) {
    int gy = Y0 - R + i / LW, gx = X0 - R + i % LW;
    if (!inner) gy = reflect101(gy, d.h), gx = reflect101(gx, d.w);
    const uint8_t* p = src + ((size_t)gy * d.w + gx) * 3;
    px[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
  for (int i = tid; i < COLOR_W; i += THREADS) cw[i] = color_w[i];
  if (tid < D * D) sw[tid] = space_w[tid];
  __syncthreads();

  const int lx = tid & (BIL_W - 1), ly0 = tid / BIL_W;
  const int gx = X0 + lx;
#pragma unroll 1
  for (int kk = 0; kk < BIL_ROWS; ++kk) {
    const int ly = ly0 + BIL_STEP * kk, gy = Y0 + ly;
    const uint32_t* win = px + ly * LW + lx;                      // the window's top-left pixel
    const uint32_t c0 = win[R * LW + R];
    float sb = 0.f, sg = 0.f, sr = 0.f, ws = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        if ((i - R) * (i - R) + (j - R) * (j - R) <= R * R) {
          const uint32_t nb = win[i * LW + j];
          const float wt = sw[i * D + j] * cw[__builtin_amdgcn_sad_u8(nb, c0, 0u)];
          sb = sb + (float)(nb & 255u) * wt;
          sg = sg + (float)((nb >> 8) & 255u) * wt;
          sr = sr + (float)((nb >> 16) & 255u) * wt;
          ws = ws + wt;
        }
      }
    }
    const float inv = 1.0f / ws;
    if (gx < d.w && gy < d.h) {
      uint8_t* o = out + d.off + ((size_t)gy * d.w + gx) * 3;
      o[0] = (uint8_t)clamp255((int)rintf(sb * inv));
      o[1] = (uint8_t)clamp255((int)rintf(sg * inv));
      o[2] = (uint8_t)clamp255((int)rintf(sr * inv));
    }
  }
}

// THE packing rule (rtd_enhance_layout): crop i is HWC with tightly packed rows and starts on a multiple of CROP_ALIGN bytes
static void layout(int n, const int32_t* rects, int64_t* offsets) {
  RTD_CHECK(n >= 0 && (n == 0 || rects) && offsets, RTD_E_INVALID, "null argument");
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t x1 = rects[4 * i], y1 = rects[4 * i + 1], x2 = rects[4 * i + 2], y2 = rects[4 * i + 3];
    const std::string ci = "crop " + std::to_string(i);
    RTD_CHECK(x1 >= 0 && y1 >= 0 && x2 - x1 >= MIN_SIDE && y2 - y1 >= MIN_SIDE, RTD_E_INVALID, ci + " is smaller than 16 pixels per side or has a negative corner");
    RTD_CHECK((x2 - x1) * (y2 - y1) * 3 < (1ll << 31), RTD_E_INVALID, ci + " has 2 GiB or more");
    offsets[i] = at;
    at += (int64_t)align_up((size_t)((x2 - x1) * (y2 - y1) * 3), CROP_ALIGN);
  }
  offsets[n] = at;
}

}  // namespace enhance

using namespace enhance;

struct rtd_enhance : bk::Base {
  double clip_limit = 0;
  int tiles_x = 0, tiles_y = 0, radius = 0;
  LabConsts consts;
  uint8_t* tables = nullptr;                 // one device allocation; the offsets below are into it
  size_t o_gtab = 0, o_ctab = 0, o_tl = 0, o_ta = 0, o_tb = 0, o_finv = 0, o_gi = 0, o_sw = 0, o_cw = 0;
  bk::DevBuf lab, bgr, luts;                 // scratch, grown on demand
  // what the last call left in the scratch (rtd_debug_enhance_stage)
  int last_n = 0;
  hipStream_t last_stream = nullptr;
  int64_t last_off[MAX_CROPS];
  int last_w[MAX_CROPS], last_h[MAX_CROPS];
};

namespace enhance {

static void upload_tables(rtd_enhance* e, const Tables& t) {
  size_t at = 0;
  auto place = [&](size_t bytes) {
    const size_t o = at;
    at = align_up(at + bytes, 256);
    return o;
  };
  e->o_gtab = place(t.gtab.size() * 2), e->o_ctab = place(t.ctab.size() * 2);
  e->o_tl = place(t.t_l.size() * 4), e->o_ta = place(t.t_a.size() * 4), e->o_tb = place(t.t_b.size() * 4);
  e->o_finv = place(t.finv.size() * 4), e->o_gi = place(t.gi.size());
  e->o_sw = place(t.space_w.size() * 4), e->o_cw = place(t.color_w.size() * 4);
  std::vector<uint8_t> host(at, 0);
  memcpy(&host[e->o_gtab], t.gtab.data(), t.gtab.size() * 2);
  memcpy(&host[e->o_ctab], t.ctab.data(), t.ctab.size() * 2);
  memcpy(&host[e->o_tl], t.t_l.data(), t.t_l.size() * 4);
  memcpy(&host[e->o_ta], t.t_a.data(), t.t_a.size() * 4);
  memcpy(&host[e->o_tb], t.t_b.data(), t.t_b.size() * 4);
  memcpy(&host[e->o_finv], t.finv.data(), t.finv.size() * 4);
  memcpy(&host[e->o_gi], t.gi.data(), t.gi.size());
  memcpy(&host[e->o_sw], t.space_w.data(), t.space_w.size() * 4);
  memcpy(&host[e->o_cw], t.color_w.data(), t.color_w.size() * 4);
  HIP_CHECK(hipMalloc((void**)&e->tables, at));
  HIP_CHECK(hipMemcpy(e->tables, host.data(), at, hipMemcpyHostToDevice));
}

template <int R>
static void launch_bilateral(const EnhArgs& a, int blocks, const float* sw, const float* cw, const uint8_t* bgr, uint8_t* out, hipStream_t s) {
  rtd::rtd_launch(enhance_bilateral<R>, dim3((unsigned)blocks), dim3(THREADS), 0, s, a, sw, cw, bgr, out);
}

static void run(rtd_enhance* e, int n, const uint8_t* const* frames, const int32_t* frame_hw, const int32_t* rects, uint8_t* out, int64_t out_cap,
                hipStream_t s) {
  // ---- every argument is checked before anything is allocated or launched
  bk::check_crop_call(n, frames, frame_hw, rects, out);
  int64_t offsets[MAX_CROPS + 1];
  layout(n, rects, offsets);
  for (int i = 0; i < n; ++i) bk::check_crop_frame(i, frames, frame_hw, rects);
  RTD_CHECK(out_cap >= offsets[n], RTD_E_INVALID, "out_cap is smaller than rtd_enhance_layout's total (" + std::to_string(offsets[n]) + " bytes)");

  const int tiles = e->tiles_x * e->tiles_y;
  EnhArgs lab_args, apply_args, bil_args;
  memset(&lab_args, 0, sizeof lab_args);
  lab_args.n = n;
  int64_t apply_blocks = 0, bil_blocks = 0;
  for (int i = 0; i < n; ++i) {
    CropDesc& d = lab_args.c[i];
    const int x1 = rects[4 * i], y1 = rects[4 * i + 1], fw = frame_hw[2 * i + 1];
    d.w = rects[4 * i + 2] - x1;
    d.h = rects[4 * i + 3] - y1;
    d.pitch = fw * 3;
    d.src = frames[i] + ((size_t)y1 * fw + x1) * 3;
    d.off = offsets[i];
    int ew = d.w, eh = d.h;
    if (d.w % e->tiles_x != 0 || d.h % e->tiles_y != 0) ew += e->tiles_x - d.w % e->tiles_x, eh += e->tiles_y - d.h % e->tiles_y;
    d.tw = ew / e->tiles_x;
    d.th = eh / e->tiles_y;
    d.clip = e->clip_limit > 0 ? std::max((int)std::min(e->clip_limit * (d.tw * d.th) / 256, 2147483647.0), 1) : 0;
    lab_args.first[i] = i * tiles;
  }
  lab_args.first[n] = n * tiles;
  apply_args = lab_args;
  bil_args = lab_args;
  for (int i = 0; i < n; ++i) {
    const CropDesc& d = lab_args.c[i];
    apply_args.first[i] = (int)apply_blocks;
    bil_args.first[i] = (int)bil_blocks;
    apply_blocks += ((int64_t)d.w * d.h + THREADS - 1) / THREADS;
    bil_blocks += (int64_t)((d.w + BIL_W - 1) / BIL_W) * ((d.h + BIL_H - 1) / BIL_H);
  }
  RTD_CHECK(apply_blocks < (1ll << 31), RTD_E_INVALID, "the call has 2^39 pixels or more");
  apply_args.first[n] = (int)apply_blocks;
  bil_args.first[n] = (int)bil_blocks;

  HIP_CHECK(hipSetDevice(e->device));
  e->last_n = 0;
  e->lab.reserve((size_t)offsets[n]);          // (hipFree waits for the device, so nothing enqueued earlier still reads a replaced buffer)
  e->bgr.reserve((size_t)offsets[n]);
  e->luts.reserve((size_t)n * tiles * 256);
  uint8_t *lab = e->lab.p, *bgr = e->bgr.p, *luts = e->luts.p;
  const uint8_t* T = e->tables;
  rtd::rtd_launch(enhance_lab_hist, dim3((unsigned)(n * tiles)), dim3(THREADS), 0, s, lab_args, e->consts, (const uint16_t*)(T + e->o_gtab),
                  (const uint16_t*)(T + e->o_ctab), lab, luts, e->tiles_x, tiles);
  HIP_CHECK(hipGetLastError());
  rtd::rtd_launch(enhance_apply, dim3((unsigned)apply_blocks), dim3(THREADS), 0, s, apply_args, e->consts, (const int32_t*)(T + e->o_tl),
                  (const int32_t*)(T + e->o_ta), (const int32_t*)(T + e->o_tb), (const int32_t*)(T + e->o_finv), T + e->o_gi, (const uint8_t*)lab,
                  (const uint8_t*)luts, bgr, e->tiles_x, e->tiles_y);
  HIP_CHECK(hipGetLastError());
  const float *sw = (const float*)(T + e->o_sw), *cw = (const float*)(T + e->o_cw);
  switch (e->radius) {
    case 1: launch_bilateral<1>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
    case 2: launch_bilateral<2>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
    case 3: launch_bilateral<3>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
    case 4: launch_bilateral<4>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
    case 5: launch_bilateral<5>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
    case 6: launch_bilateral<6>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
    default: launch_bilateral<7>(bil_args, (int)bil_blocks, sw, cw, bgr, out, s); break;
  }
  HIP_CHECK(hipGetLastError());
  e->last_n = n;
  e->last_stream = s;
  for (int i = 0; i < n; ++i) e->last_off[i] = offsets[i], e->last_w[i] = lab_args.c[i].w, e->last_h[i] = lab_args.c[i].h;
}

}  // namespace enhance

extern "C" {

int rtd_enhance_create(int32_t device, const rtd_enhance_params* p, rtd_enhance_handle* out) {
  return bk::create(out, rtd_enhance_destroy, [&](rtd_enhance* e) {
    RTD_CHECK(p && p->struct_size == (int32_t)sizeof(rtd_enhance_params), RTD_E_INVALID, "rtd_enhance_params: bad struct_size");
    RTD_CHECK(p->clip_limit == p->clip_limit && p->clip_limit <= 1e6f, RTD_E_INVALID, "clip_limit must be a number <= 1e6 (<= 0: no clipping)");
    RTD_CHECK(p->tiles_x >= 1 && p->tiles_x <= MAX_TILES && p->tiles_y >= 1 && p->tiles_y <= MAX_TILES, RTD_E_INVALID, "tile grid must be 1..16 per axis");
    RTD_CHECK(p->sigma_color == p->sigma_color && p->sigma_space == p->sigma_space && p->sigma_space <= 1e6f, RTD_E_INVALID, "bad sigma");
    const int radius = bilateral_radius(p->bilateral_d, (double)p->sigma_space);
    RTD_CHECK(radius >= 1 && radius <= MAX_RADIUS, RTD_E_INVALID, "the bilateral radius (d / 2, or rint(1.5 sigma_space) for d <= 0) must be 1..7");
    bk::use_device(device);
    e->device = device;
    e->clip_limit = (double)p->clip_limit;
    e->tiles_x = p->tiles_x, e->tiles_y = p->tiles_y, e->radius = radius;
    const Tables t = make_tables(p->bilateral_d, (double)p->sigma_color, (double)p->sigma_space);
    memcpy(e->consts.C, t.C, sizeof t.C);
    memcpy(e->consts.Ci, t.Ci, sizeof t.Ci);
    e->consts.fmin = t.fmin;
    upload_tables(e, t);
  });
}

int rtd_enhance_layout(int32_t n, const int32_t* rects, int64_t* offsets) {
  return bk::caught(bk::create_error<rtd_enhance>(), [&] { layout(n, rects, offsets); });
}

int rtd_enhance_crops(rtd_enhance_handle e, int32_t n, const uint8_t* const* frames_dev, const int32_t* frame_hw, const int32_t* rects,
                      uint8_t* out_dev, int64_t out_cap, void* stream) {
  return guarded(e, [&] { run(e, n, frames_dev, frame_hw, rects, out_dev, out_cap, (hipStream_t)stream); });
}

const char* rtd_enhance_last_error(rtd_enhance_handle e) { return bk::last_error(e); }

void rtd_enhance_destroy(rtd_enhance_handle e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  e->lab.release();                           // (hipFree waits for the device: nothing enqueued still uses the scratch)
  e->bgr.release();
  e->luts.release();
  if (e->tables) (void)hipFree(e->tables);
  (void)hipGetLastError();
  delete e;
}

int rtd_debug_enhance_stage(rtd_enhance_handle e, int32_t crop, int32_t stage, uint8_t* out, size_t nbytes) {
  return guarded(e, [&] {
    RTD_CHECK(out && stage >= 0 && stage <= 2, RTD_E_INVALID, "stage must be 0 (Lab), 1 (LUTs) or 2 (BGR before the bilateral filter)");
    RTD_CHECK(e->last_n > 0, RTD_E_STATE, "no successful rtd_enhance_crops call yet");
    RTD_CHECK(crop >= 0 && crop < e->last_n, RTD_E_INVALID, "no such crop in the last call");
    const size_t tiles = (size_t)e->tiles_x * e->tiles_y;
    const size_t want = stage == 1 ? tiles * 256 : (size_t)e->last_w[crop] * e->last_h[crop] * 3;
    RTD_CHECK(nbytes == want, RTD_E_INVALID, "nbytes must be " + std::to_string(want));
    HIP_CHECK(hipSetDevice(e->device));
    HIP_CHECK(hipStreamSynchronize(e->last_stream));
    const uint8_t* src = stage == 1 ? e->luts.p + (size_t)crop * tiles * 256 : (stage == 0 ? e->lab.p : e->bgr.p) + e->last_off[crop];
    HIP_CHECK(hipMemcpy(out, src, want, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
