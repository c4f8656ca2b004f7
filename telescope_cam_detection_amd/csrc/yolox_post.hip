// yolox_post.hip - YOLOX post-processing on the device (rtd_yolox_post_* in include/rtdetr_mi355.h): upstream's
// yolox.utils.postprocess with torchvision's per-class batched_nms, and optionally the head's grid decode.  Restated in tests/yolox_ref.py.
//
// One memset and four launches per call, whatever n is; nothing crosses to the host between them.  Grids are sized from n_anchors and
// max_candidates, and a workgroup reads the image's device-side count and leaves when it has nothing to do.
//   yolox_score     the only pass over all n * A * (5 + C) floats: a workgroup streams whole rows as one flat dword range into LDS (rows
//                   are 4-byte aligned and no more), a few lanes share a row's class scores, and a passing row is appended to its image's
//                   candidate list as the composite (f2key(score) << 32 | ~anchor) - one ballot and one LDS add per wave, one global
//                   add per workgroup.
//   yolox_rank      one workgroup per image: when more rows passed than max_candidates, an 8-bit radix select of the max_candidates-th
//                   largest composite; a bitonic sort in LDS (score descending, anchor ascending: the composite's order); then the
//                   ranked rows - corners, obj, class_conf, class_id, area - from the prediction rows and the score pass's class record.
//   yolox_mask      the 64 x 64 bit-mask formulation: word (i, j / 64) has bit j % 64 set when j > i, same class and IoU > threshold.
//   yolox_scan      one wave per image walks the ranked rows in chunks of 64: a chunk is resolved from its diagonal word with scalar
//                   lane reads, its kept rows go to the output, and their words are ORed into the per-lane `removed` words of the later
//                   chunks - four rows' loads at a time, none depending on another.
// The score, corner, area and IoU expressions are single fp32 operations (__fmul_rn and friends are never contracted).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "../../include/rtdetr_mi355.h"
#include "backend.h"
#include "yolox_post_host.h"

namespace yolox_post {

namespace bk = rtd::backend;
using namespace yolox_post_host;
typedef unsigned long long u64;

constexpr int RANK_THREADS = 1024;

// ops.hip's top-k key: a larger key is a larger float; the composite orders by (score descending, index ascending)
__device__ __forceinline__ unsigned f2key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 entry_of(unsigned key, int i) { return ((u64)key << 32) | (unsigned)(0xffffffffu - (unsigned)i); }
__device__ __forceinline__ int entry_index(u64 e) { return (int)(0xffffffffu - (unsigned)(e & 0xffffffffu)); }

struct ScoreArgs {
  const float* pred;
  int A, C, F, stride, rows, tpr_log2;
  float conf;
  uint32_t keep[KEEP_WORDS];
};

__global__ __launch_bounds__(SCORE_THREADS) void yolox_score(ScoreArgs a, int* __restrict__ passed, u64* __restrict__ cand,
                                                              float2* __restrict__ meta) {
  __shared__ float tile[SCORE_LDS_WORDS];
  __shared__ int s_count, s_base;
  const int tid = threadIdx.x, img = blockIdx.y;
  if (tid == 0) s_count = 0;
  const int row0 = blockIdx.x * a.rows;
  const int rows = min(a.rows, a.A - row0);                       // >= 1: the grid is ceil(A / rows)
  const float* __restrict__ g = a.pred + ((int64_t)img * a.A + row0) * a.F;
  const int total = rows * a.F;
  if (a.stride == a.F) {
    for (int i = tid; i < total; i += SCORE_THREADS) tile[i] = g[i];
  } else {
    for (int i = tid; i < total; i += SCORE_THREADS) {
      const int r = i / a.F;
      tile[r * a.stride + (i - r * a.F)] = g[i];
    }
  }
  __syncthreads();
  const int tpr = 1 << a.tpr_log2;
  const int row = tid >> a.tpr_log2, part = tid & (tpr - 1);
  const bool valid = row < rows;
  const float* p = tile + min(row, rows - 1) * a.stride;
  // the largest class score and the lowest class that holds it; a NaN anywhere makes class_conf NaN, as torch.max does
  float best = part < a.C ? p[5 + part] : -INFINITY;
  int bc = part;
  bool nan = best != best;
  for (int c = part + tpr; c < a.C; c += tpr) {
    const float v = p[5 + c];
    nan |= v != v;
    if (v > best) best = v, bc = c;
  }
  for (int o = 1; o < tpr; o <<= 1) {                              // the lanes of a row are neighbours inside one wave
    const float ob = __shfl_xor(best, o);
    const int oc = __shfl_xor(bc, o);
    nan |= __shfl_xor((int)nan, o) != 0;
    if (ob > best || (ob == best && oc < bc)) best = ob, bc = oc;
  }
  float score = __fmul_rn(p[4], best);
  if (score == 0.f) score = 0.f;                                   // -0 and +0 are one score
  const bool kept_class = bc < a.C && ((a.keep[bc >> 5] >> (bc & 31)) & 1u);
  const bool pass = valid && part == 0 && !nan && kept_class && score >= a.conf;      // (NaN >= x is false)
  // one LDS add per wave, then one global add per workgroup: the images' counters are few addresses under many workgroups
  const u64 ballot = __ballot(pass);
  const int lane = tid & 63;
  const int leader = ballot ? __ffsll((long long)ballot) - 1 : 0;
  int wave_base = 0;
  if (ballot && lane == leader) wave_base = atomicAdd(&s_count, __popcll(ballot));
  wave_base = __shfl(wave_base, leader);
  __syncthreads();
  if (tid == 0 && s_count > 0) s_base = atomicAdd(&passed[img], s_count);
  __syncthreads();
  if (pass) {
    const int pos = s_base + wave_base + __popcll(ballot & ((1ull << lane) - 1ull));
    const int64_t anchor = (int64_t)img * a.A + row0 + row;
    if (pos < a.A) {
      cand[(int64_t)img * a.A + pos] = entry_of(f2key(score), row0 + row);
      meta[anchor] = make_float2(best, (float)bc);             // what the rank pass would otherwise work out again
    }
  }
}

struct RankArgs {
  const float* pred;
  int A, C, F, K;
  int decode, in_h, in_w;
};

__global__ __launch_bounds__(RANK_THREADS) void yolox_rank(RankArgs a, const int* __restrict__ passed, const u64* __restrict__ cand,
                                                           const float2* __restrict__ meta, float* __restrict__ ranked) {
  __shared__ u64 keys[MAX_CANDIDATES];
  __shared__ int hist[256];
  __shared__ int s_bin, s_need, s_pos;
  const int tid = threadIdx.x, img = blockIdx.x;
  const int np = min(passed[img], a.A);
  if (np <= 0) return;
  const u64* __restrict__ cd = cand + (int64_t)img * a.A;
  const int m = min(np, a.K);
  int P = 2;
  while (P < m) P <<= 1;
  if (np <= a.K) {
    for (int i = tid; i < P; i += RANK_THREADS) keys[i] = i < m ? cd[i] : 0ull;
  } else {
    // the K-th largest composite, a byte at a time from the top (composites are distinct: exactly K are >= it)
    u64 prefix = 0, mask = 0;
    int need = a.K;
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int i = tid; i < 256; i += RANK_THREADS) hist[i] = 0;
      __syncthreads();
      for (int i = tid; i < np; i += RANK_THREADS) {
        const u64 e = cd[i];
        if ((e & mask) == prefix) atomicAdd(&hist[(int)((e >> shift) & 255ull)], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int cum = 0, b = 255;
        for (; b > 0; --b) {
          if (cum + hist[b] >= need) break;
          cum += hist[b];
        }
        s_bin = b;
        s_need = need - cum;
      }
      __syncthreads();
      need = s_need;
      prefix |= (u64)s_bin << shift;
      mask |= 255ull << shift;
    }
    if (tid == 0) s_pos = 0;
    for (int i = tid; i < P; i += RANK_THREADS) keys[i] = 0ull;
    __syncthreads();
    for (int i = tid; i < np; i += RANK_THREADS) {
      const u64 e = cd[i];
      if (e >= prefix) {
        const int pos = atomicAdd(&s_pos, 1);
        if (pos < m) keys[pos] = e;
      }
    }
  }
  __syncthreads();
  // bitonic sort, descending; the zero padding (smaller than any composite) ends up last
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += RANK_THREADS) {
        const int x = i ^ j;
        if (x > i) {
          const u64 ka = keys[i], kb = keys[x];
          if ((i & k) == 0 ? ka < kb : ka > kb) keys[i] = kb, keys[x] = ka;
        }
      }
      __syncthreads();
    }
  }
  // the ranked rows
  const int n0 = a.decode ? (a.in_h / 8) * (a.in_w / 8) : 0, n1 = a.decode ? (a.in_h / 16) * (a.in_w / 16) : 0;
  for (int r = tid; r < m; r += RANK_THREADS) {
    const int idx = min(max(entry_index(keys[r]), 0), a.A - 1);
    const float* __restrict__ p = a.pred + ((int64_t)img * a.A + idx) * a.F;
    const float2 cls = meta[(int64_t)img * a.A + idx];             // class_conf, class_id: the score pass wrote them for every candidate
    float cx = p[0], cy = p[1], w = p[2], h = p[3];
    if (a.decode) {
      int loc = idx, s = 8;
      if (idx >= n0 + n1) loc = idx - n0 - n1, s = 32;
      else if (idx >= n0) loc = idx - n0, s = 16;
      const int wl = a.in_w / s;
      const int gy = loc / wl, gx = loc - gy * wl;
      const float fs = (float)s;
      cx = __fmul_rn(__fadd_rn(cx, (float)gx), fs);
      cy = __fmul_rn(__fadd_rn(cy, (float)gy), fs);
      w = __fmul_rn(expf(w), fs);
      h = __fmul_rn(expf(h), fs);
    }
    const float hw = __fmul_rn(w, 0.5f), hh = __fmul_rn(h, 0.5f);          // w / 2: exact
    const float x1 = __fsub_rn(cx, hw), y1 = __fsub_rn(cy, hh), x2 = __fadd_rn(cx, hw), y2 = __fadd_rn(cy, hh);
    float4* o = (float4*)(ranked + ((int64_t)img * a.K + r) * ROW_RANKED);
    o[0] = make_float4(x1, y1, x2, y2);
    o[1] = make_float4(p[4], cls.x, cls.y, __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1)));
  }
}

// grid (K / 64 column chunks, K / 256 groups of four row chunks, n), 256 threads: wave w of a workgroup holds the rows of chunk
// ri = 4 y + w, one per lane, against the 64 columns of chunk cj, which the workgroup stages once
constexpr int MASK_WAVES = 4;
__global__ __launch_bounds__(64 * MASK_WAVES) void yolox_mask(const int* __restrict__ passed, const float* __restrict__ ranked,
                                                              u64* __restrict__ mask, int K, float thr) {
  __shared__ float4 cbox[64];
  __shared__ float2 cmeta[64];      // class, area
  const int t = threadIdx.x & 63, cj = blockIdx.x, ri = blockIdx.y * MASK_WAVES + (threadIdx.x >> 6), img = blockIdx.z;
  const int m = min(passed[img], K);
  if ((int)blockIdx.y * MASK_WAVES > cj || cj * 64 >= m) return;           // (the same for the whole workgroup)
  const float4* __restrict__ R = (const float4*)(ranked + (int64_t)img * K * ROW_RANKED);
  const int col = cj * 64 + t;
  if (threadIdx.x < 64) {
    if (col < m) {
      const float4 b = R[2 * col], q = R[2 * col + 1];
      cbox[t] = b;
      cmeta[t] = make_float2(q.z, q.w);
    } else {
      cbox[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      cmeta[t] = make_float2(-1.f, 0.f);
    }
  }
  __syncthreads();
  const int row = ri * 64 + t;
  if (ri > cj || row >= m) return;
  const float4 a = R[2 * row], aq = R[2 * row + 1];
  u64 bits = 0;
  const int jn = min(64, m - cj * 64);
  for (int j = 0; j < jn; ++j) {
    const float4 b = cbox[j];
    const float2 bm = cmeta[j];
    const float iw = fmaxf(0.f, __fsub_rn(fminf(a.z, b.z), fmaxf(a.x, b.x)));
    const float ih = fmaxf(0.f, __fsub_rn(fminf(a.w, b.w), fmaxf(a.y, b.y)));
    const float inter = __fmul_rn(iw, ih);
    const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(aq.w, bm.y), inter));
    if (cj * 64 + j > row && bm.x == aq.z && iou > thr) bits |= 1ull << j;       // (NaN > thr is false)
  }
  const int words = K / 64;
  mask[((int64_t)img * K + row) * words + cj] = bits;
}

__device__ __forceinline__ u64 lane_read64(u64 v, int lane) {        // `lane` is the same in every lane
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}

// one wave per image
__global__ __launch_bounds__(64) void yolox_scan(const int* __restrict__ passed, const float* __restrict__ ranked, const u64* __restrict__ mask,
                                                 int K, float* __restrict__ rows_out, int* __restrict__ counts) {
  const int lane = threadIdx.x, img = blockIdx.x;
  const int np = passed[img];
  const int m = min(np, K);
  const int words = K / 64, chunks = (m + 63) / 64;
  const u64* __restrict__ M = mask + (int64_t)img * K * words;
  const float* __restrict__ R = ranked + (int64_t)img * K * ROW_RANKED;
  float* __restrict__ out = rows_out + (int64_t)img * K * ROW_OUT;
  u64 rem0 = 0, rem1 = 0;            // this lane's `removed` words: of chunk `lane` and of chunk `lane + 64`
  int nk = 0;
  u64 diag = lane < m ? M[(int64_t)lane * words] : 0ull;
  for (int c = 0; c < chunks; ++c) {
    const int nrow = (c + 1) * 64 + lane;
    const u64 diag_next = (c + 1 < chunks && nrow < m) ? M[(int64_t)nrow * words + c + 1] : 0ull;      // in flight while this chunk resolves
    const int nv = min(64, m - c * 64);
    u64 rem = lane_read64(c < 64 ? rem0 : rem1, c & 63);
    if (nv < 64) rem |= ~0ull << nv;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const u64 d = lane_read64(diag, i);
      if (!((rem >> i) & 1ull)) rem |= d;
    }
    const u64 kept = ~rem;
    if ((kept >> lane) & 1ull) {
      const int pos = nk + __popcll(kept & ((1ull << lane) - 1ull));
      const float* src = R + (int64_t)(c * 64 + lane) * ROW_RANKED;
      if (pos < K)
        for (int q = 0; q < ROW_OUT; ++q) out[(int64_t)pos * ROW_OUT + q] = src[q];
    }
    nk += __popcll(kept);
    if (c + 1 < chunks) {
      const bool use0 = lane > c && lane < chunks, use1 = lane + 64 > c && lane + 64 < chunks;
      u64 kb = kept;
      while (kb) {
        int r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          r[q] = kb ? __ffsll((long long)kb) - 1 : -1;
          if (kb) kb &= kb - 1ull;
        }
        u64 v0[4], v1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const u64* rowp = M + (int64_t)(c * 64 + max(r[q], 0)) * words;
          v0[q] = (r[q] >= 0 && use0) ? rowp[lane] : 0ull;
          v1[q] = (r[q] >= 0 && use1) ? rowp[lane + 64] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) rem0 |= v0[q], rem1 |= v1[q];
      }
    }
    diag = diag_next;
  }
  if (lane == 0) counts[2 * img] = nk, counts[2 * img + 1] = np;
}

}  // namespace yolox_post

using namespace yolox_post;

struct rtd_yolox_post : bk::Base {
  rtd_yolox_post_config cfg;
  bk::DevBuf scratch;                // grown on demand; belongs to the call in flight
};

namespace yolox_post {

static void run(rtd_yolox_post* y, int n, const float* pred, int n_anchors, const rtd_yolox_post_params* p, float* rows, int32_t* counts,
                hipStream_t s) {
  check_run(y->cfg, n, pred, n_anchors, p, rows, counts);
  const int C = y->cfg.num_classes, K = y->cfg.max_candidates;
  const Layout l = layout(n, n_anchors, K);
  const ScoreTile t = score_tile(C);

  HIP_CHECK(hipSetDevice(y->device));
  y->scratch.reserve(l.total);       // (hipFree waits for the device, so nothing enqueued earlier still uses a replaced buffer)
  uint8_t* S = y->scratch.p;
  int* passed = (int*)(S + l.passed);
  u64* cand = (u64*)(S + l.cand);
  float2* meta = (float2*)(S + l.meta);
  float* ranked = (float*)(S + l.ranked);
  u64* mask = (u64*)(S + l.mask);

  HIP_CHECK(hipMemsetAsync(passed, 0, (size_t)n * sizeof(int32_t), s));
  ScoreArgs sa;
  memset(&sa, 0, sizeof sa);
  sa.pred = pred, sa.A = n_anchors, sa.C = C, sa.F = t.floats, sa.stride = t.stride, sa.rows = t.rows, sa.tpr_log2 = t.tpr_log2;
  sa.conf = p->conf_threshold;
  keep_words(C, p->class_keep, sa.keep);
  rtd::rtd_launch(yolox_score, dim3((unsigned)((n_anchors + t.rows - 1) / t.rows), (unsigned)n), dim3(SCORE_THREADS), 0, s, sa, passed, cand, meta);
  HIP_CHECK(hipGetLastError());
  RankArgs ra;
  memset(&ra, 0, sizeof ra);
  ra.pred = pred, ra.A = n_anchors, ra.C = C, ra.F = t.floats, ra.K = K, ra.decode = p->decode, ra.in_h = p->in_h, ra.in_w = p->in_w;
  rtd::rtd_launch(yolox_rank, dim3((unsigned)n), dim3(RANK_THREADS), 0, s, ra, (const int*)passed, (const u64*)cand, (const float2*)meta, ranked);
  HIP_CHECK(hipGetLastError());
  rtd::rtd_launch(yolox_mask, dim3((unsigned)l.words, (unsigned)((l.words + MASK_WAVES - 1) / MASK_WAVES), (unsigned)n), dim3(64 * MASK_WAVES), 0, s, (const int*)passed, (const float*)ranked, mask, K,
                  p->nms_threshold);
  HIP_CHECK(hipGetLastError());
  rtd::rtd_launch(yolox_scan, dim3((unsigned)n), dim3(64), 0, s, (const int*)passed, (const float*)ranked, (const u64*)mask, K, rows, counts);
  HIP_CHECK(hipGetLastError());
}

}  // namespace yolox_post

extern "C" {

int rtd_yolox_anchors(int32_t in_h, int32_t in_w, int32_t* n_anchors) {
  return bk::caught(bk::create_error<rtd_yolox_post>(), [&] {
    RTD_CHECK(n_anchors, RTD_E_INVALID, "null argument");
    *n_anchors = anchors(in_h, in_w);
  });
}

int rtd_yolox_post_create(const rtd_yolox_post_config* cfg, rtd_yolox_post_handle* out) {
  return bk::create(out, rtd_yolox_post_destroy, [&](rtd_yolox_post* y) {
    check_config(cfg);
    bk::use_device(cfg->device);
    y->device = cfg->device;
    y->cfg = *cfg;
  });
}

int rtd_yolox_post_run(rtd_yolox_post_handle y, int32_t n, const float* pred_dev, int32_t n_anchors, const rtd_yolox_post_params* params,
                       float* rows_dev, int32_t* counts_dev, void* stream) {
  return guarded(y, [&] { run(y, n, pred_dev, n_anchors, params, rows_dev, counts_dev, (hipStream_t)stream); });
}

const char* rtd_yolox_post_last_error(rtd_yolox_post_handle y) { return bk::last_error(y); }

void rtd_yolox_post_destroy(rtd_yolox_post_handle y) {
  if (!y) return;
  (void)hipSetDevice(y->device);
  y->scratch.release();              // (hipFree waits for the device: nothing enqueued still uses the scratch)
  (void)hipGetLastError();
  delete y;
}

}  // extern "C"
