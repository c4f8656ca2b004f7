// classifier.hip - the Stage-2 species classifier on the GPU: timm's `Eva` vision transformer (the reference's config names
// timm/eva02_large_patch14_clip_336.merged2b_ft_inat21; src/species_classifier.py calls `self.model(x)`).  The arithmetic is restated in
// tests/eva_ref.py.
//
// Every GEMM (patch embed, qkv, proj, fc1_g | fc1_x, fc2, head) is a 1x1 launch_conv (conv_igemm.hip) on token rows [1, 1, rows, C] in the
// handle's precision, the fp16 hi + lo pair format (RTD_PREC_F16X3) or fp32; the residual add is the conv's epilogue.  The kernels here are
// what a transformer needs beside them: eva_patchify, eva_tokens, eva_layernorm (rows of up to 4096 channels, a valid prefix, an optional
// SwiGLU front), eva_rope, eva_attention (MFMA attention on pair operands) and eva_pool.  Per batch size n the handle caches a plan: an op
// list over one arena (classifier_host.h: Layout).  The residual stream ping-pongs between xa and xb: proj reads xa and writes xb, fc2 reads
// xb and writes xa, so a conv never writes over the residual it reads.  Everything is enqueued on the caller's stream; the handle owns no
// stream and never captures one.
#include <math.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <new>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"
#include "classifier_host.h"
#include "net_plan.h"

namespace eva {

using namespace rtd;
namespace vh = eva_host;
namespace bk = rtd::backend;
namespace np = rtd::netplan;
using bk::guarded;
using np::op_dtype;

constexpr int HD = vh::HEAD_DIM;

// ---------------------------------------------------------------------------------------------------------------- kernels
// 8 consecutive channels (c % 8 == 0) of row `row` of a [rows][ld] tensor, pair storage or fp32
template <bool PAIR>
__device__ __forceinline__ void load8(const void* base, int64_t row, int64_t ld, int c, float (&v)[8]) {
  if (PAIR) {
    split_load8((const sp16*)base, row * ld, c, v);
  } else {
    const float* p = (const float*)base + row * ld + c;
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
  }
}
template <bool PAIR>
__device__ __forceinline__ void store8(void* base, int64_t row, int64_t ld, int c, const float (&v)[8]) {
  if (PAIR) {
    split_store8((sp16*)base, row * ld, c, v);
  } else {
    float* p = (float*)base + row * ld + c;
    *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
    *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
}

// one thread per 8 channels of a patch row: x [n][3][S][S] fp32 -> rows [n G G][Kp], k = (c p + i) p + j, zeros from 3 p p on
template <bool PAIR>
__global__ void __launch_bounds__(256) eva_patchify(const float* __restrict__ x, void* __restrict__ rows, int n, int S, int p, int G, int Kp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int chunks = Kp >> 3;
  if (i >= (int64_t)n * G * G * chunks) return;
  const int ch = (int)(i % chunks);
  const int64_t row = i / chunks;
  const int gx = (int)(row % G), gy = (int)((row / G) % G), img = (int)(row / ((int64_t)G * G));
  const int pp = p * p;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int kk = ch * 8 + k;
    float f = 0.f;
    if (kk < 3 * pp) {
      const int c = kk / pp, r = kk - c * pp, iy = r / p, jx = r - iy * p;
      f = x[(((int64_t)img * 3 + c) * S + (gy * p + iy)) * S + (gx * p + jx)];
    }
    v[k] = f;
  }
  store8<PAIR>(rows, row, Kp, ch * 8, v);
}

// one thread per 8 channels of a token row: x[n][0] = cls + pos[0], x[n][t] = pe[n][t - 1] + pos[t]
template <bool PAIR>
__global__ void __launch_bounds__(256) eva_tokens(const void* __restrict__ pe, const float* __restrict__ cls, const float* __restrict__ pos,
                                                  void* __restrict__ x, int n, int L, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int chunks = D >> 3;
  if (i >= (int64_t)n * L * chunks) return;
  const int c = (int)(i % chunks) * 8;
  const int64_t row = i / chunks;
  const int t = (int)(row % L);
  const int64_t img = row / L;
  float v[8];
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = cls[c + k];
  } else {
    load8<PAIR>(pe, img * (L - 1) + (t - 1), D, c, v);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] += pos[(int64_t)t * D + c + k];
  store8<PAIR>(x, row, D, c, v);
}

// LayerNorm of rows of up to 4096 channels over their first c_valid channels; one block per row, a thread holds up to two 8-channel
// chunks in registers (two passes: mean, then the variance of the centred values).  SWIGLU: the row is [g | x] (x at channel offset c)
// and the value is silu(g) * x (timm's SwiGLU followed by its sub-LN).  NORM = false: the value itself is written.
struct LnArgs {
  const void* x;       // SWIGLU: the gate g
  const void* x2;      // SWIGLU: x
  int64_t ld_in;
  void* y;
  int64_t ld_out;
  int c, c_valid;
  const float* gain;
  const float* bias;
  float eps;
};
__device__ __forceinline__ float block_sum256(float v, float* sh) {
  v = wave_sum64(v);
  __syncthreads();                                   // (sh may still be read from the previous reduction)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
template <bool PAIR, bool SWIGLU, bool NORM>
__global__ void __launch_bounds__(256) eva_layernorm(LnArgs a) {
  __shared__ float sh[4];
  const int64_t row = blockIdx.x;
  float v[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c0 = (threadIdx.x + 256 * i) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[i][k] = 0.f;
    if (c0 < a.c) {
      load8<PAIR>(SWIGLU ? a.x2 : a.x, row, a.ld_in, c0, v[i]);
      if (SWIGLU) {
        float g[8];
        load8<PAIR>(a.x, row, a.ld_in, c0, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[i][k] *= g[k] / (1.f + expf(-g[k]));
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k >= a.c_valid) v[i][k] = 0.f;
    }
  }
  if (NORM) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[i][k];
    const float mean = block_sum256(s, sh) / (float)a.c_valid;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = (threadIdx.x + 256 * i) * 8 + k;
        v[i][k] = c < a.c_valid ? v[i][k] - mean : 0.f;
        q += v[i][k] * v[i][k];
      }
    const float rstd = 1.f / sqrtf(block_sum256(q, sh) / (float)a.c_valid + a.eps);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = (threadIdx.x + 256 * i) * 8 + k;
        v[i][k] = c < a.c_valid ? v[i][k] * rstd * a.gain[c] + a.bias[c] : 0.f;
      }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c0 = (threadIdx.x + 256 * i) * 8;
    if (c0 < a.c) store8<PAIR>(a.y, row, a.ld_out, c0, v[i]);
  }
}

// one thread per 8 channels of q or k of one (token, head): the pair values are recombined to fp32, rotated and split again
template <bool PAIR>
__global__ void __launch_bounds__(256) eva_rope(void* __restrict__ qkv, const float* __restrict__ sin_t, const float* __restrict__ cos_t, int n, int L,
                                                int heads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int D = heads * HD, per_row = 2 * heads * (HD / 8);
  if (i >= (int64_t)n * L * per_row) return;
  const int u = (int)(i % per_row);
  const int64_t row = i / per_row;
  const int t = (int)(row % L);
  if (t == 0) return;                                            // the cls token is not rotated
  const int which = u / (heads * (HD / 8)), hu = u - which * heads * (HD / 8), head = hu / (HD / 8), d0 = (hu - head * (HD / 8)) * 8;
  const int c = which * D + head * HD + d0;
  float v[8], o[8];
  load8<PAIR>(qkv, row, 3 * (int64_t)D, c, v);
  const float* sn = sin_t + (int64_t)(t - 1) * HD + d0;
  const float* cs = cos_t + (int64_t)(t - 1) * HD + d0;
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    o[k] = v[k] * cs[k] - v[k + 1] * sn[k];
    o[k + 1] = v[k + 1] * cs[k + 1] + v[k] * sn[k + 1];
  }
  store8<PAIR>(qkv, row, 3 * (int64_t)D, c, o);
}

// MFMA attention on pair operands: o = softmax(q k^T) v per (image, head), head dim 64, q already scaled.  A block = 4 waves = 64 queries
// of one (image, head).  K and V come 64 keys at a time: the next tile's global loads are issued into registers before the current tile's
// MFMAs and written to LDS after them (register staging).  A head's 64 channels are two 32-channel groups [32 hi | 32 lo], i.e. 256
// consecutive bytes of a qkv row, and one group is one K-step of v_mfma_f32_16x16x32_f16.  Every wave runs the transposed scheme of
// k_attention_mfma_f32 (ops.hip) on its 16 queries:
//   S^T[key][query] = K Q^T per 16-key tile, three products hi hi + hi lo + lo hi per K-step; the lane holds 4 keys of its query column;
//   online softmax in fp32 over two such tiles (32 keys): the lane's 8 probabilities, split to hi + lo, ARE the B fragment of
//   O^T[d][query] += V^T P^T, whose 32 K-slots are (lane >> 4) * 8 + (tile * 4 + r);
//   V is stored in LDS transposed, keys in that slot order, so V^T's A fragment is one 16-byte read.
// Tail keys are loaded as zeros and masked to -inf; tail queries read the last row and are not stored.
__global__ void __launch_bounds__(256) eva_attention(const sp16* __restrict__ qkv, int64_t ld, sp16* __restrict__ o, int64_t ldo, int L, int D) {
  static_assert(HD == 64, "eva_attention: head dim 64 (two 32-channel groups per head, four 16-row output tiles)");
  constexpr int KT = 64, KROW = 2 * HD + 8, VROW = KT + 8;       // LDS row lengths in 16-bit elements (16-byte pads)
  __shared__ __attribute__((aligned(16))) sp16 Ks[KT * KROW];    // [key][group 0: 32 hi | 32 lo, group 1: 32 hi | 32 lo]
  __shared__ __attribute__((aligned(16))) sp16 Vt[2 * HD * VROW];   // [hi, lo][d][slot of key]
  const int b = blockIdx.z, head = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int qi = blockIdx.x * 64 + wave * 16 + r16;
  const int64_t row0 = (int64_t)b * L;

  sp16x8 qh[2], ql[2];
  {
    const sp16* qp = qkv + 2 * (row0 + min(qi, L - 1)) * ld + head * (2 * HD) + 8 * q4;
#pragma unroll
    for (int c = 0; c < 2; ++c) { qh[c] = *(const sp16x8*)(qp + 64 * c); ql[c] = *(const sp16x8*)(qp + 64 * c + SPLIT_GROUP); }
  }
  const sp16* kb = qkv + 2 * row0 * ld + 2 * (int64_t)D + head * (2 * HD);
  const sp16* vb = kb + 2 * (int64_t)D;
  // staging: a tile is 64 keys x 16 parts of 16 bytes for K and for V; thread -> part tid & 15, keys (tid >> 4) + 16 i
  const int part = tid & 15, key0 = tid >> 4;
  sp16x8 kreg[4], vreg[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kj = k0 + key0 + 16 * i;
      const sp16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kreg[i] = z; vreg[i] = z;
      if (kj < L) { kreg[i] = *(const sp16x8*)(kb + 2 * (int64_t)kj * ld + part * 8); vreg[i] = *(const sp16x8*)(vb + 2 * (int64_t)kj * ld + part * 8); }
    }
  };
  const int v_lo = (part >> 2) & 1, v_ch0 = (part >> 3) * SPLIT_GROUP + (part & 3) * 8;
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = key0 + 16 * i;
      *(sp16x8*)&Ks[key * KROW + part * 8] = kreg[i];
      const int kk = key & 31;
      const int slot = (key & 32) + 8 * ((kk & 15) >> 2) + 4 * (kk >> 4) + (kk & 3);
      sp16* vt = Vt + (v_lo * HD + v_ch0) * VROW + slot;
#pragma unroll
      for (int j = 0; j < 8; ++j) vt[j * VROW] = vreg[i][j];
    }
  };

  float m = -INFINITY, l = 0.f;
  f32x4 O[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) O[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  gload(0);
  for (int k0 = 0; k0 < L; k0 += KT) {
    __syncthreads();                                             // every wave is done with the previous tile
    lstore();
    __syncthreads();
    if (k0 + KT < L) gload(k0 + KT);                             // in flight while this tile is computed
    const int nchunk = (min(KT, L - k0) + 31) >> 5;
    for (int ch = 0; ch < nchunk; ++ch) {
      f32x4 S[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        S[sub] = f32x4{0.f, 0.f, 0.f, 0.f};                      // S^T[key 4 q4 + r][query r16] of the 16-key tile
        const sp16* kr = &Ks[(ch * 32 + sub * 16 + r16) * KROW + 8 * q4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const sp16x8 kh = *(const sp16x8*)(kr + 64 * c), kl = *(const sp16x8*)(kr + 64 * c + SPLIT_GROUP);
          S[sub] = mfma_pair16(kh, ql[c], S[sub]);
          S[sub] = mfma_pair16(kl, qh[c], S[sub]);
          S[sub] = mfma_pair16(kh, qh[c], S[sub]);
        }
      }
      float sv[8];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0 + ch * 32 + (j >> 2) * 16 + 4 * q4 + (j & 3);
        sv[j] = key < L ? S[j >> 2][j & 3] : -INFINITY;
        mx = fmaxf(mx, sv[j]);
      }
      mx = rows4_max(mx);
      const float mn = fmaxf(m, mx);                             // finite: key k0 + 32 ch of the chunk exists
      const float alpha = expf(m - mn);
      float rs = 0.f;
      sp16x8 ph, pl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = expf(sv[j] - mn);
        rs += p;
        sp16 a, c2;
        split2(p, a, c2);
        ph[j] = a; pl[j] = c2;
      }
      rs = rows4_sum(rs);
      l = l * alpha + rs;
      m = mn;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const sp16* vr = &Vt[(dt * 16 + r16) * VROW + ch * 32 + 8 * q4];
        const sp16x8 vh8 = *(const sp16x8*)vr, vl8 = *(const sp16x8*)(vr + HD * VROW);
#pragma unroll
        for (int r = 0; r < 4; ++r) O[dt][r] *= alpha;
        O[dt] = mfma_pair16(vl8, ph, O[dt]);                     // O^T[d 16 dt + 4 q4 + r][query r16]
        O[dt] = mfma_pair16(vh8, pl, O[dt]);
        O[dt] = mfma_pair16(vh8, ph, O[dt]);
      }
    }
  }
  if (qi < L) {
    const float inv = 1.f / l;
    sp16* op = o + 2 * (row0 + qi) * ldo + head * (2 * HD);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int c = dt * 16 + 4 * q4;
      sp16x4 h, w;
#pragma unroll
      for (int r = 0; r < 4; ++r) { sp16 a, c2; split2(O[dt][r] * inv, a, c2); h[r] = a; w[r] = c2; }
      sp16* q = op + ((c >> 5) << 6) + (c & 31);
      *(sp16x4*)q = h;
      *(sp16x4*)(q + SPLIT_GROUP) = w;
    }
  }
}

// one thread per 8 channels of an image: the cls row (avg = 0) or the mean of the patch tokens (avg = 1)
template <bool PAIR>
__global__ void __launch_bounds__(256) eva_pool(const void* __restrict__ x, void* __restrict__ y, int n, int L, int D, int avg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int chunks = D >> 3;
  if (i >= n * chunks) return;
  const int c = (i % chunks) * 8, img = i / chunks;
  float acc[8];
  if (!avg) {
    load8<PAIR>(x, (int64_t)img * L, D, c, acc);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int t = 1; t < L; ++t) {
      float v[8];
      load8<PAIR>(x, (int64_t)img * L + t, D, c, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += v[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] /= (float)(L - 1);
  }
  store8<PAIR>(y, img, D, c, acc);
}

// fp32 values at or beyond fp16's range, or not finite (rtd_eva_self_check on the logits, and on the fp32 engine's residual stream)
__global__ void __launch_bounds__(256) eva_count_big(const float* __restrict__ x, int64_t n, unsigned long long* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !(fabsf(x[i]) < 65504.f)) atomicAdd(count, 1ull);
}

// ---------------------------------------------------------------------------------------------------------------- launchers
static unsigned blocks_for(int64_t threads) { return (unsigned)((threads + 255) / 256); }

static void launch_patchify(int P, const float* x, void* rows, int n, int S, int p, hipStream_t s) {
  const int G = S / p, Kp = vh::pad32(3 * p * p);
  const unsigned g = blocks_for((int64_t)n * G * G * (Kp / 8));
  if (P == F16X2) rtd_launch(eva_patchify<true>, dim3(g), dim3(256), 0, s, x, rows, n, S, p, G, Kp);
  else rtd_launch(eva_patchify<false>, dim3(g), dim3(256), 0, s, x, rows, n, S, p, G, Kp);
  HIP_CHECK(hipGetLastError());
}
static void launch_tokens(int P, const void* pe, const float* cls, const float* pos, void* x, int n, int L, int D, hipStream_t s) {
  const unsigned g = blocks_for((int64_t)n * L * (D / 8));
  if (P == F16X2) rtd_launch(eva_tokens<true>, dim3(g), dim3(256), 0, s, pe, cls, pos, x, n, L, D);
  else rtd_launch(eva_tokens<false>, dim3(g), dim3(256), 0, s, pe, cls, pos, x, n, L, D);
  HIP_CHECK(hipGetLastError());
}
static void launch_eva_layernorm(int P, const LnArgs& a, int64_t rows, bool swiglu, bool norm, hipStream_t s) {
  RTD_CHECK(a.c >= 8 && a.c <= vh::MAX_LN_C && a.c % (P == F16X2 ? SPLIT_GROUP : 8) == 0, RTD_E_INVALID,
            "eva_layernorm: rows of at most 4096 channels, a multiple of 8 (pair storage: of 32)");
  RTD_CHECK(a.c_valid >= 1 && a.c_valid <= a.c, RTD_E_INVALID, "eva_layernorm: c_valid must be 1..c");
  RTD_CHECK(rows >= 1 && rows < (int64_t)1 << 31, RTD_E_INVALID, "eva_layernorm: rows");
  RTD_CHECK(a.ld_in % 8 == 0 && a.ld_out % 8 == 0 && aligned16(a.x, a.y) && (!swiglu || aligned16(a.x2)), RTD_E_INVALID, "eva_layernorm: alignment");
  RTD_CHECK(!norm || (a.gain && a.bias), RTD_E_INVALID, "eva_layernorm: null gain or bias");
  const dim3 g((unsigned)rows), blk(256);
  auto go = [&](auto pair, auto sw, auto nm) { rtd_launch((eva_layernorm<pair(), sw(), nm()>), g, blk, 0, s, a); };
  auto with_flags = [&](auto pair) {
    using T = std::true_type; using F = std::false_type;
    if (swiglu && norm) go(pair, T{}, T{});
    else if (swiglu) go(pair, T{}, F{});
    else if (norm) go(pair, F{}, T{});
    else go(pair, F{}, F{});
  };
  if (P == F16X2) with_flags(std::true_type{});
  else with_flags(std::false_type{});
  HIP_CHECK(hipGetLastError());
}
static void launch_rope(int P, void* qkv, const float* sin_t, const float* cos_t, int n, int L, int heads, hipStream_t s) {
  const unsigned g = blocks_for((int64_t)n * L * 2 * heads * (HD / 8));
  if (P == F16X2) rtd_launch(eva_rope<true>, dim3(g), dim3(256), 0, s, qkv, sin_t, cos_t, n, L, heads);
  else rtd_launch(eva_rope<false>, dim3(g), dim3(256), 0, s, qkv, sin_t, cos_t, n, L, heads);
  HIP_CHECK(hipGetLastError());
}
static Tensor rows_tensor(void* p, int dt, int n, int rows_per_image, int c, int64_t ld) {
  Tensor t;
  t.p = p; t.dt = dt; t.n = n; t.h = 1; t.w = rows_per_image; t.c = c; t.ld = ld; t.bstride = (int64_t)rows_per_image * ld;
  return t;
}
// qkv [n L][3 D] -> o [n L][D].  Pair storage: eva_attention, q as it is.  fp32: the library's launch_attention on the [q | k] view, which
// scales by 1 / 8 itself - the fp32 engine uploads the blob's folded q rows and q bias times 8, which undoes the fold exactly.
static void launch_eva_attention(int P, void* qkv, void* o, int n, int L, int heads, hipStream_t s) {
  const int D = heads * HD;
  RTD_CHECK(n >= 1 && n <= 65535 && heads >= 1 && heads <= 65535 && L >= 1, RTD_E_INVALID, "eva_attention: extents");
  RTD_CHECK(aligned16(qkv, o), RTD_E_INVALID, "eva_attention: alignment");
  if (P == F16X2) {
    rtd_launch(eva_attention, dim3((unsigned)((L + 63) / 64), (unsigned)heads, (unsigned)n), dim3(256), 0, s, (const sp16*)qkv, (int64_t)3 * D, (sp16*)o,
               (int64_t)D, L, D);
    HIP_CHECK(hipGetLastError());
  } else {
    const Tensor t = rows_tensor(qkv, F32, n, L, 3 * D, 3 * D);
    launch_attention(t.slice_c(0, 2 * D), t.slice_c(2 * D, D), rows_tensor(o, F32, n, L, D, D), heads, s);
  }
}
static void launch_pool(int P, const void* x, void* y, int n, int L, int D, int avg, hipStream_t s) {
  const unsigned g = blocks_for((int64_t)n * (D / 8));
  if (P == F16X2) rtd_launch(eva_pool<true>, dim3(g), dim3(256), 0, s, x, y, n, L, D, avg);
  else rtd_launch(eva_pool<false>, dim3(g), dim3(256), 0, s, x, y, n, L, D, avg);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------- plan
enum OpKind { OP_PATCHIFY, OP_CONV, OP_TOKENS, OP_LN, OP_ROPE, OP_ATTN, OP_POOL };
// (tensors of an op are arena offsets: net_plan.h)
struct Op {
  int kind = OP_CONV;
  ConvArgs conv;                       // OP_CONV (x, y, res as offsets)
  size_t a = 0, a2 = 0, y = 0;         // the other kinds: input(s) and output
  int c = 0, c_valid = 0;              // OP_LN
  int64_t rows = 0, ld_in = 0, ld_out = 0;
  bool swiglu = false, norm = true;
  const float* gain = nullptr;
  const float* bias = nullptr;
  std::string stage;                   // the debug name of the tensor this op completes ("" = none)
  size_t stage_off = 0;
  int stage_dt = F32, stage_rows = 0, stage_c = 0, stage_ld = 0;   // rows per image
};
struct Plan : np::PlanBase {
  int n = 0;
  vh::Layout lay;
  std::vector<Op> ops;
};

}  // namespace eva

struct rtd_eva : rtd::netplan::NetBase {
  rtd_eva_config cfg;
  eva_host::Dims dm;
  std::vector<char> blob;
  std::map<std::string, const float*> vecs;     // LayerNorm gains and biases, cls_token, pos_embed, the RoPE tables: fp32 on the device
  std::map<int, std::unique_ptr<eva::Plan>> plans;
  // the last call (rtd_debug_eva_tensor re-runs it up to the stage asked for; rtd_eva_self_check scans what it left)
  const float* last_x = nullptr;
  eva::Plan* last_plan = nullptr;
};

namespace eva {

static std::unique_ptr<Plan> build_plan(rtd_eva* e, int n) {
  auto p = std::make_unique<Plan>();
  p->n = n;
  p->lay = vh::layout(e->cfg, n);
  const vh::Layout& a = p->lay;
  const rtd_eva_config& c = e->cfg;
  const vh::Dims& d = e->dm;
  const int P = e->P, D = c.dim, L = d.L, np = n * d.G * d.G, nl = n * L;
  size_t slab = 0;
  auto rows_at = [&](size_t off, int dt, int rows, int ch, int ld) { return rows_tensor((void*)off, dt, 1, rows, ch, ld); };
  auto stage = [&](Op& op, const std::string& name, size_t off, int dt, int rows_per_image, int ch, int ld) {
    op.stage = name; op.stage_off = off; op.stage_dt = dt; op.stage_rows = rows_per_image; op.stage_c = ch; op.stage_ld = ld;
  };
  auto conv = [&](const std::string& name, const Tensor& x, const Tensor& y, const Tensor* res) -> Op& {
    Op op;
    op.kind = OP_CONV;
    ConvArgs& ca = op.conv;
    ca = conv_args(x, y, e->filters.at(name), 1, 1, 0, ACT_NONE);
    np::plan_conv(ca, &e->conv_opts, res, RES_PRE, slab, name);
    p->ops.push_back(op);
    return p->ops.back();
  };
  auto ln = [&](const std::string& name, size_t in, size_t in2, int64_t ld_in, size_t out, int64_t rows, int ch, int c_valid, bool swiglu, bool norm) -> Op& {
    Op op;
    op.kind = OP_LN;
    op.a = in; op.a2 = in2; op.y = out; op.rows = rows; op.c = ch; op.c_valid = c_valid; op.ld_in = ld_in; op.ld_out = ch; op.swiglu = swiglu; op.norm = norm;
    if (norm) { op.gain = e->vecs.at(name + ".weight"); op.bias = e->vecs.at(name + ".bias"); }
    p->ops.push_back(op);
    return p->ops.back();
  };

  { Op op; op.kind = OP_PATCHIFY; op.y = a.patches; p->ops.push_back(op); }
  stage(conv("patch_embed", rows_at(a.patches, P, np, d.Kp, d.Kp), rows_at(a.pe, P, np, D, D), nullptr), "patch_embed", a.pe, P, d.G * d.G, D, D);
  { Op op; op.kind = OP_TOKENS; op.a = a.pe; op.y = a.xa; stage(op, "tokens", a.xa, P, L, D, D); p->ops.push_back(op); }
  const Tensor xa = rows_at(a.xa, P, nl, D, D), xb = rows_at(a.xb, P, nl, D, D), y = rows_at(a.y, P, nl, D, D);
  const Tensor qkv = rows_at(a.qkv, P, nl, 3 * D, 3 * D), ao = rows_at(a.ao, P, nl, D, D);
  const Tensor h1 = rows_at(a.h1, P, nl, 2 * d.Hp, 2 * d.Hp), h2 = rows_at(a.h2, P, nl, d.Hp, d.Hp);
  for (int i = 0; i < c.depth; ++i) {
    const std::string b = "blocks." + std::to_string(i);
    ln(b + ".norm1", a.xa, 0, D, a.y, nl, D, D, false, true);
    conv(b + ".attn.qkv", y, qkv, nullptr);
    { Op op; op.kind = OP_ROPE; op.y = a.qkv; p->ops.push_back(op); }
    { Op op; op.kind = OP_ATTN; op.a = a.qkv; op.y = a.ao; p->ops.push_back(op); }
    if (c.scale_attn_inner) ln(b + ".attn.norm", a.ao, 0, D, a.y, nl, D, D, false, true);
    stage(conv(b + ".attn.proj", c.scale_attn_inner ? y : ao, xb, &xa), b + ".attn", a.xb, P, L, D, D);
    ln(b + ".norm2", a.xb, 0, D, a.y, nl, D, D, false, true);
    conv(b + ".mlp.fc1", y, h1, nullptr);
    // silu(g) * x, and the sub-LN over the hidden width's valid prefix when the checkpoint has one
    ln(b + ".mlp.norm", a.h1, a.h1 + (size_t)d.Hp * 4, 2 * d.Hp, a.h2, nl, d.Hp, c.hidden, true, c.scale_mlp != 0);
    stage(conv(b + ".mlp.fc2", h2, xa, &xb), b, a.xa, P, L, D, D);
  }
  { Op op; op.kind = OP_POOL; op.a = a.xa; op.y = a.pool; p->ops.push_back(op); }
  stage(ln("final_norm", a.pool, 0, D, a.pooln, n, D, D, false, true), "pool", a.pooln, P, 1, D, D);
  stage(conv("head", rows_at(a.pooln, P, n, D, D), rows_at(a.logits, F32, n, d.Cp, d.Cp), nullptr), "logits", a.logits, F32, 1, c.classes, d.Cp);

  p->seal(a.top, slab);
  return p;
}

static void run_op(rtd_eva* e, const Plan* p, const Op& op, const float* x, hipStream_t s) {
  char* base = (char*)e->arena.p;
  const rtd_eva_config& c = e->cfg;
  const vh::Dims& d = e->dm;
  switch (op.kind) {
    case OP_PATCHIFY: launch_patchify(e->P, x, base + op.y, p->n, c.img, c.patch, s); break;
    case OP_CONV: np::run_conv(op.conv, base, *p, s); break;
    case OP_TOKENS: launch_tokens(e->P, base + op.a, e->vecs.at("cls_token"), e->vecs.at("pos_embed"), base + op.y, p->n, d.L, c.dim, s); break;
    case OP_LN: {
      LnArgs a;
      a.x = base + op.a; a.x2 = base + op.a2; a.ld_in = op.ld_in; a.y = base + op.y; a.ld_out = op.ld_out; a.c = op.c; a.c_valid = op.c_valid;
      a.gain = op.gain; a.bias = op.bias; a.eps = 1e-6f;
      launch_eva_layernorm(e->P, a, op.rows, op.swiglu, op.norm, s);
      break;
    }
    case OP_ROPE: launch_rope(e->P, base + op.y, e->vecs.at("rope_sin"), e->vecs.at("rope_cos"), p->n, d.L, c.heads, s); break;
    case OP_ATTN: launch_eva_attention(e->P, base + op.a, base + op.y, p->n, d.L, c.heads, s); break;
    default: launch_pool(e->P, base + op.a, base + op.y, p->n, d.L, c.dim, c.pool == RTD_EVA_POOL_AVG, s);
  }
}

static void run(rtd_eva* e, const float* x, int n, float* logits, hipStream_t s) {
  // ---- every argument is checked before anything is allocated or launched
  RTD_CHECK(x && logits, RTD_E_INVALID, "null argument");
  RTD_CHECK(n >= 1 && n <= e->cfg.max_batch, RTD_E_INVALID, "1..max_batch (" + std::to_string(e->cfg.max_batch) + ") images per call");
  HIP_CHECK(hipSetDevice(e->device));
  e->last_plan = nullptr;
  Plan* p = np::get_or_build(e->plans, n, vh::MAX_BATCH, [&] { return build_plan(e, n); });   // (n <= 64: the cache never outgrows its cap)
  e->arena.reserve(p->bytes);
  for (const Op& op : p->ops) run_op(e, p, op, x, s);
  HIP_CHECK(hipMemcpy2DAsync(logits, (size_t)e->cfg.classes * 4, e->arena.p + p->lay.logits, (size_t)e->dm.Cp * 4, (size_t)e->cfg.classes * 4, (size_t)n,
                             hipMemcpyDeviceToDevice, s));
  e->last_x = x, e->last_plan = p, e->last_stream = s;
}

// Every 2-d `.weight` of the table is a filter, uploaded with its `.bias` (net_plan.h: upload_filters); every other tensor is an fp32
// vector in one pool.  The blob's q rows carry 1 / 8; the fp32 engine's attention (launch_attention) scales by 1 / 8 itself, so its q rows
// and q bias are uploaded times 8 - exact, a power of two.
static void upload_weights(rtd_eva* e, const std::map<std::string, vh::HostTensor>& host, const std::vector<vh::TensorDesc>& table) {
  std::vector<np::FilterSpec> specs;
  std::vector<std::pair<std::string, size_t>> vec_items;
  size_t v_bytes = 0;
  for (const vh::TensorDesc& d : table) {
    const bool is_w = d.shape.size() == 2 && d.name.size() > 7 && d.name.compare(d.name.size() - 7, 7, ".weight") == 0;
    if (is_w) {
      specs.push_back({d.name.substr(0, d.name.size() - 7), conv_filter_extents(e->P, (int)d.shape[0], (int)d.shape[1])});
    } else {
      const size_t dot = d.name.rfind('.');
      const bool is_filter_bias = dot != std::string::npos && d.name.substr(dot) == ".bias" && host.count(d.name.substr(0, dot) + ".weight") &&
                                  host.at(d.name.substr(0, dot) + ".weight").shape.size() == 2;
      if (is_filter_bias) continue;
      vec_items.push_back({d.name, v_bytes});
      v_bytes += bk::align_up((size_t)host.at(d.name).numel() * 4, 256);
    }
  }
  char* vpool = e->dmalloc(v_bytes);
  for (const auto& v : vec_items) {
    const vh::HostTensor& t = host.at(v.first);
    HIP_CHECK(hipMemcpy(vpool + v.second, t.data, (size_t)t.numel() * 4, hipMemcpyHostToDevice));
    e->vecs[v.first] = (const float*)(vpool + v.second);
  }
  const int D = e->cfg.dim;
  np::upload_filters(*e, specs, [&](size_t i, std::vector<float>& rows, std::vector<float>& bias) {
    const std::string& name = specs[i].name;
    const ConvFilter& f = specs[i].f;
    rows = conv_filter_rows(f, {{host.at(name + ".weight").data, f.K}});
    memcpy(bias.data(), host.at(name + ".bias").data, (size_t)f.N * 4);
    const bool qkv = name.size() > 9 && name.compare(name.size() - 9, 9, ".attn.qkv") == 0;
    if (qkv && e->P == F32) {
      const int kc = f.kcols();
      for (int o = 0; o < D; ++o) {
        bias[o] *= 8.f;
        for (int k = 0; k < f.K; ++k) rows[(size_t)o * kc + k] *= 8.f;
      }
    }
  });
}

// (the kernel-level entry points report where rtd_last_error(NULL) reads)
template <typename F>
static int op_guard(F&& f) { return np::op_guard<rtd_engine>(f); }

}  // namespace eva

using namespace eva;

extern "C" {

int rtd_eva_create(const rtd_eva_config* cfg, const void* blob, size_t nbytes, rtd_eva_handle* out) {
  return bk::create(out, rtd_eva_close, [&](rtd_eva* e) {
    vh::check_config(cfg);
    e->cfg = *cfg;
    e->dm = vh::dims(*cfg);
    e->P = cfg->precision == RTD_PREC_FP32 ? F32 : F16X2;
    vh::need(blob && nbytes >= 12, RTD_E_WEIGHTS, "empty weight blob");
    e->blob.assign((const char*)blob, (const char*)blob + nbytes);
    std::map<std::string, vh::HostTensor> host;
    vh::parse_blob(e->blob.data(), e->blob.size(), host);
    const std::vector<vh::TensorDesc> table = vh::tensor_table(*cfg);
    vh::check_tensors(host, table, e->P == F16X2);               // the whole blob is checked before the device is touched
    bk::use_device(cfg->device);
    e->device = cfg->device;
    e->conv_opts = conv_opts_template();
    upload_weights(e, host, table);
    e->blob.clear();
    e->blob.shrink_to_fit();
  });
}

int rtd_eva_forward(rtd_eva_handle e, const float* x_dev, int32_t n, float* logits_dev, void* stream) {
  return guarded(e, [&] { run(e, x_dev, n, logits_dev, (hipStream_t)stream); });
}

int rtd_eva_self_check(rtd_eva_handle e, int64_t* saturated) {
  return guarded(e, [&] {
    RTD_CHECK(saturated, RTD_E_INVALID, "null argument");
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_eva_forward call yet");
    HIP_CHECK(hipSetDevice(e->device));
    const Plan* p = e->last_plan;
    hipStream_t s = e->last_stream;
    bk::OpScratch sc;
    unsigned long long* cnt = sc.zeros<unsigned long long>(1);
    const int64_t nx = (int64_t)p->n * e->dm.L * e->cfg.dim, nlog = (int64_t)p->n * e->dm.Cp;
    if (e->P == F16X2) launch_count_saturated(e->arena.p + p->lay.xa, nx * 2, cnt, s);
    else rtd_launch(eva_count_big, dim3(blocks_for(nx)), dim3(256), 0, s, (const float*)(e->arena.p + p->lay.xa), nx, cnt);
    rtd_launch(eva_count_big, dim3(blocks_for(nlog)), dim3(256), 0, s, (const float*)(e->arena.p + p->lay.logits), nlog, cnt);
    HIP_CHECK(hipGetLastError());
    unsigned long long host = 0;
    HIP_CHECK(hipMemcpyAsync(&host, cnt, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    *saturated = (int64_t)host;
  });
}

int64_t rtd_eva_arena_bytes(rtd_eva_handle e) { return e ? e->arena_bytes() : 0; }

const char* rtd_eva_last_error(rtd_eva_handle e) { return bk::last_error(e); }

void rtd_eva_close(rtd_eva_handle e) {
  if (!e) return;
  e->release_device();
  delete e;
}

int rtd_debug_eva_tensor(rtd_eva_handle e, const char* name, float* out, int64_t capacity, int64_t shape[4]) {
  return guarded(e, [&] {
    RTD_CHECK(name && shape, RTD_E_INVALID, "null argument");
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_eva_forward call yet");
    const Plan* p = e->last_plan;
    size_t upto = 0;
    const Op* st = nullptr;
    for (size_t i = 0; i < p->ops.size() && !st; ++i)
      if (p->ops[i].stage == name) { st = &p->ops[i]; upto = i + 1; }
    RTD_CHECK(st, RTD_E_INVALID, std::string("unknown debug tensor ") + name);
    shape[0] = p->n, shape[1] = 1, shape[2] = st->stage_rows, shape[3] = st->stage_c;
    const int64_t rows = (int64_t)p->n * st->stage_rows, numel = rows * st->stage_c;
    if (!out) return;
    RTD_CHECK(capacity >= numel, RTD_E_INVALID, "debug tensor: output capacity too small");
    HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = e->last_stream;
    for (size_t i = 0; i < upto; ++i) run_op(e, p, p->ops[i], e->last_x, s);
    np::read_tensor(rows_tensor(e->arena.p + st->stage_off, st->stage_dt, p->n, st->stage_rows, st->stage_c, st->stage_ld), rows, out, s);
  });
}

int rtd_debug_eva_plan_convs(rtd_eva_handle e, char* out, int64_t capacity, int64_t* needed) {
  return guarded(e, [&] {
    RTD_CHECK(e->last_plan, RTD_E_STATE, "no successful rtd_eva_forward call yet");
    np::text_out(np::plan_convs_text(*e->last_plan, OP_CONV, {}), out, capacity, needed);
  });
}

// ---- kernel-level test entry points (include/rtdetr_mi355_test.h)
int rtd_op_eva_patchify(int dtype, const float* x, void* rows, int n, int img, int patch) {
  return op_guard([&] {
    RTD_CHECK(x && rows && n >= 1 && n <= vh::MAX_BATCH && patch >= 1 && patch <= 64 && img >= patch && img <= vh::MAX_IMG && img % patch == 0, RTD_E_INVALID,
              "eva_patchify: arguments");
    RTD_CHECK(aligned16(rows), RTD_E_INVALID, "eva_patchify: alignment");
    launch_patchify(op_dtype(dtype), x, rows, n, img, patch, nullptr);
  });
}

int rtd_op_eva_rope(int dtype, void* qkv, const float* sin_t, const float* cos_t, int n, int L, int heads) {
  return op_guard([&] {
    RTD_CHECK(qkv && sin_t && cos_t && n >= 1 && L >= 1 && heads >= 1 && (int64_t)n * L * heads < (int64_t)1 << 24, RTD_E_INVALID, "eva_rope: arguments");
    RTD_CHECK(aligned16(qkv), RTD_E_INVALID, "eva_rope: alignment");
    launch_rope(op_dtype(dtype), qkv, sin_t, cos_t, n, L, heads, nullptr);
  });
}

int rtd_op_eva_layernorm(int dtype, const void* x, void* y, const float* gain, const float* bias, int rows, int c, int c_valid, int swiglu, int norm,
                         float eps) {
  return op_guard([&] {
    RTD_CHECK(x && y && c >= 1, RTD_E_INVALID, "eva_layernorm: arguments");
    LnArgs a;
    a.x = x;
    a.x2 = (const char*)x + (size_t)c * 4;
    a.ld_in = swiglu ? 2 * (int64_t)c : c;
    a.y = y; a.ld_out = c; a.c = c; a.c_valid = c_valid; a.gain = gain; a.bias = bias; a.eps = eps;
    launch_eva_layernorm(op_dtype(dtype), a, rows, swiglu != 0, norm != 0, nullptr);
  });
}

int rtd_op_eva_attention(int dtype, const void* qkv, void* o, int n, int L, int heads) {
  return op_guard([&] {
    RTD_CHECK(qkv && o, RTD_E_INVALID, "eva_attention: null argument");
    launch_eva_attention(op_dtype(dtype), (void*)qkv, o, n, L, heads, nullptr);
  });
}

}  // extern "C"
