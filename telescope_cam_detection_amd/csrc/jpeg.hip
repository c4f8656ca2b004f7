// jpeg.hip - baseline JPEG (SOF0, one scan, 4:2:0 or gray) of a batch of HWC uint8 frames, byte-identical to libjpeg at its defaults
// (what cv2.imencode / Pillow write for a quality alone).  The restatement the bytes must equal is tests/jpeg_ref.py; it lists the
// arithmetic.  For device frames only the compressed bytes cross PCIe.
//
// Passes (every exchange between workgroups happens across a launch boundary; no workgroup waits for another inside a launch):
//   transform   one workgroup per 128 x 16 pixel tile (8 MCUs, or 2 x 16 gray blocks): aligned dword loads of the rows into LDS,
//               BGR -> YCbCr and the 2 x 2 chroma average in LDS, jfdctint rows then columns with 8 threads per block, exact quantisation
//               (host-made multipliers), zig-zag int16 blocks written in scan order as dwordx4, and per block one side word: the length
//               of its AC codes and its DC
//   size        one thread per block: the side word plus the DC code against the previous DC of its component, scanned inside
//               256-block chunks; then one workgroup scans the chunk totals of each frame
//   (host)      reads the bit count of every frame, places the frames in the unstuffed buffer
//   write       one workgroup per 128 blocks: code words assembled in LDS, whole dwords stored, the two boundary words OR-ed into the
//               zeroed buffer with one atomic each
//   stuff       0xFF -> 0xFF 0x00: count per 1 KB chunk, one workgroup scans the counts over all frames, scatter
// The host writes the markers around each frame's scan.
#include <algorithm>
#include <map>
#include <mutex>
#include <new>

#include "../../include/rtdetr_mi355.h"
#include "../../include/rtdetr_mi355_test.h"
#include "backend.h"

namespace jpeg_enc {

using rtd::Error;
namespace bk = rtd::backend;
using bk::align_up;
using bk::guarded;

constexpr int TILE_W = 128, TILE_H = 16;
constexpr int T_THREADS = 384;               // 48 blocks x 8 threads
constexpr int T_BLOCKS = 48;
constexpr int RAW_DW = 98;                   // dwords per staged row: 128 * 3 bytes + up to 3 of misalignment, rounded up
constexpr int CHUNK = 256;                   // blocks per sizing chunk
constexpr int W_BLOCKS = 128;                // blocks per bit-writing workgroup
constexpr int BLOCK_WORDS = 52;              // a block codes into at most 22 + 63 * 26 = 1660 bits
constexpr int S_CHUNK = 1024;                // unstuffed bytes per stuffing workgroup
constexpr int S_THREADS = 256;

struct Tables {
  uint32_t qm[2][64];        // floor(2^32 / d) + 1, d = 8 q: umulhi(n, qm) == n / d for n < 2^17 (n e < 2^32 with e = qm d - 2^32 <= d <= 2040)
  uint32_t qh[2][64];        // d >> 1
  uint32_t huff[2][16 + 256];   // (code << 5) | length: [0..15] DC by size, [16 + symbol] AC
  uint32_t zz[64];           // natural index -> zig-zag position
};

struct FrameDesc {
  const uint8_t* src;
  int rows, cols, ch;
  int bx, by;                // colour: MCUs per row / MCU rows; gray: 8 x 8 blocks per row / block rows
  int tiles_x, tile0;
  int block0, nblocks;       // this frame's blocks in the flattened scan-order list
  int chunk0, nchunks;       // its 256-block chunks in the flattened chunk list
  // filled after the sizing pass
  uint32_t ubase;            // byte offset of its unstuffed scan (a multiple of S_CHUNK)
  uint32_t ubytes;           // unstuffed scan bytes (padded to a whole byte)
  uint32_t bits;             // before padding
  int schunk0;               // its first stuffing chunk in the flattened list
};

__device__ inline int find_frame(const FrameDesc* d, int n, int v, int FrameDesc::*first) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].*first <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// exclusive scan of one value per thread over a workgroup of N threads (sh: N words); total = the sum
template <int N>
__device__ inline uint32_t wg_scan(uint32_t v, uint32_t* sh, int tid, uint32_t& total) {
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < N; o <<= 1) {
    const uint32_t t = tid >= o ? sh[tid - o] : 0u;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  total = sh[N - 1];
  const uint32_t r = sh[tid] - v;
  __syncthreads();
  return r;
}

#define DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

// libjpeg's jfdctint, one 8-point pass.  FIRST: outputs scaled up by 4 (PASS1_BITS); else the column pass, which removes that scale.
template <bool FIRST>
__device__ inline void fdct8(int* d) {
  constexpr int S = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) << 2;
    d[4] = (t10 - t11) << 2;
  } else {
    d[0] = DESCALE(t10 + t11, 2);
    d[4] = DESCALE(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = DESCALE(z1 + t13 * 6270, S);
  d[6] = DESCALE(z1 - t12 * 15137, S);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = DESCALE(a4 + z1 + z3, S);
  d[5] = DESCALE(a5 + z2 + z4, S);
  d[3] = DESCALE(a6 + z2 + z3, S);
  d[1] = DESCALE(a7 + z1 + z4, S);
}

__device__ inline void load_huff(uint32_t (*huff)[272], const Tables* tabs, int tid, int threads) {
  for (int i = tid; i < 2 * 272; i += threads) huff[i / 272][i % 272] = tabs->huff[i / 272][i % 272];
}

// side[block] = (bits of the block's AC codes << 16) | its DC as uint16: what the sizing pass and the DC prediction of the writing pass need
__global__ void __launch_bounds__(T_THREADS) transform_kernel(const FrameDesc* __restrict__ descs, int n_frames, const Tables* __restrict__ tabs,
                                                              uint4* __restrict__ coef, uint32_t* __restrict__ side) {
  __shared__ uint32_t huff[2][272];
  __shared__ uint32_t raw[TILE_H * RAW_DW];
  __shared__ uint8_t yp[TILE_H * TILE_W];
  __shared__ uint8_t cp[2][8 * 64];
  __shared__ int ws[T_BLOCKS * 64];
  __shared__ __attribute__((aligned(16))) short zq[T_BLOCKS * 64];
  __shared__ uint32_t qm[2][64], qh[2][64], zz[64];

  const int tid = threadIdx.x;
  const FrameDesc d = descs[find_frame(descs, n_frames, (int)blockIdx.x, &FrameDesc::tile0)];
  const int t = blockIdx.x - d.tile0;
  const int tx = t % d.tiles_x, ty = t / d.tiles_x;
  const int x0 = tx * TILE_W, y0 = ty * TILE_H;
  const bool colour = d.ch == 3;
  if (tid < 128) {
    qm[tid >> 6][tid & 63] = tabs->qm[tid >> 6][tid & 63];
    qh[tid >> 6][tid & 63] = tabs->qh[tid >> 6][tid & 63];
    if (tid < 64) zz[tid] = tabs->zz[tid];
  }
  load_huff(huff, tabs, tid, T_THREADS);

  // 1. the tile's rows -> LDS: aligned dwords; a dword that is not wholly inside the frame is put together from its bytes
  const int tw = min(TILE_W, d.cols - x0), th = min(TILE_H, d.rows - y0);
  const uintptr_t fb = (uintptr_t)d.src, fe = fb + (size_t)d.rows * d.cols * d.ch;
  for (int i = tid; i < TILE_H * RAW_DW; i += T_THREADS) {
    const int r = i / RAW_DW, k = i - r * RAW_DW;
    if (r >= th) continue;
    const uintptr_t a = fb + ((size_t)(y0 + r) * d.cols + x0) * d.ch;
    const uintptr_t p = (a & ~(uintptr_t)3) + 4 * (uintptr_t)k;
    if (p >= a + (size_t)tw * d.ch) continue;
    uint32_t v = 0;
    if (p >= fb && p + 4 <= fe) {
      v = *(const uint32_t*)p;
    } else {
      for (int b = 0; b < 4; ++b)
        if (p + b >= fb && p + b < fe) v |= (uint32_t) * (const uint8_t*)(p + b) << (8 * b);
    }
    raw[i] = v;
  }
  __syncthreads();

  // 2. luminance at every pixel of the tile (coordinates clamped to the frame: its last column / row replicated)
  const uint8_t* rb = (const uint8_t*)raw;
  for (int i = tid; i < TILE_H * TILE_W; i += T_THREADS) {
    const int ly = min(i / TILE_W, th - 1), lx = min(i % TILE_W, tw - 1);
    const int sh = (int)((fb + ((size_t)(y0 + ly) * d.cols + x0) * d.ch) & 3);
    const uint8_t* p = rb + ly * (RAW_DW * 4) + sh + lx * d.ch;
    yp[i] = colour ? (uint8_t)((19595 * p[2] + 38470 * p[1] + 7471 * p[0] + 32768) >> 16) : p[0];
  }
  // chroma: 2 x 2 boxes; the columns right of the frame repeat its last column, an odd last row is doubled, and the rows below the
  // frame repeat the last DOWNSAMPLED row (libjpeg pads after downsampling)
  if (colour) {
    const int qlast = ((d.rows - 1) >> 1) - (y0 >> 1);
    for (int i = tid; i < 8 * 64; i += T_THREADS) {
      const int qy = min(i >> 6, qlast), qx = i & 63;
      int cb = 0, cr = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ly = min(2 * qy + (k >> 1), th - 1), lx = min(2 * qx + (k & 1), tw - 1);
        const int sh = (int)((fb + ((size_t)(y0 + ly) * d.cols + x0) * d.ch) & 3);
        const uint8_t* p = rb + ly * (RAW_DW * 4) + sh + lx * 3;
        const int B = p[0], G = p[1], R = p[2];
        cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      }
      const int bias = 1 + (qx & 1);
      cp[0][i] = (uint8_t)((cb + bias) >> 2);
      cp[1][i] = (uint8_t)((cr + bias) >> 2);
    }
  }
  __syncthreads();

  // 3. DCT: 8 threads per block.  Local block b: colour MCU b / 6, member b % 6 (Y00 Y01 Y10 Y11 Cb Cr); gray column b % 16, row b / 16.
  const int b = tid >> 3, j = tid & 7;
  const int nloc = colour ? T_BLOCKS : 32;
  const int m = b / 6, k = b - 6 * m;
  const uint8_t* org;
  int stride, table = 0;
  if (!colour) {
    org = yp + (b >> 4) * 8 * TILE_W + (b & 15) * 8;
    stride = TILE_W;
  } else if (k < 4) {
    org = yp + (k >> 1) * 8 * TILE_W + m * 16 + (k & 1) * 8;
    stride = TILE_W;
  } else {
    org = cp[k - 4] + m * 8;
    stride = 64;
    table = 1;
  }
  int v[8];
  if (b < nloc) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (int)org[j * stride + i] - 128;
    fdct8<true>(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) ws[b * 64 + j * 8 + i] = v[i];
  }
  __syncthreads();
  // which blocks exist, and which are libjpeg's dummy blocks (luminance blocks past the frame's last real block column / row)
  bool exists, dummy = false;
  int gidx;
  if (colour) {
    const int mx = tx * 8 + m;
    exists = mx < d.bx;
    gidx = d.block0 + (ty * d.bx + mx) * 6 + k;
    if (k < 4) dummy = (2 * mx + (k & 1)) * 8 >= d.cols || (2 * ty + (k >> 1)) * 8 >= d.rows;
  } else {
    const int gx = tx * 16 + (b & 15), gy = ty * 2 + (b >> 4);
    exists = b < 32 && gx < d.bx && gy < d.by;
    gidx = d.block0 + gy * d.bx + gx;
  }
  if (b < nloc) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = ws[b * 64 + i * 8 + j];
    fdct8<false>(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int nat = i * 8 + j;
      const int c = v[i];
      const int q = (int)__umulhi((uint32_t)(abs(c) + (int)qh[table][nat]), qm[table][nat]);
      zq[b * 64 + zz[nat]] = dummy ? (short)0 : (short)(c < 0 ? -q : q);
    }
  }
  __syncthreads();
  // a dummy block carries the DC of the block before it in the MCU: right edge Y01 <- Y00, Y11 <- Y10; bottom edge Y10, Y11 <- Y01
  if (colour && tid < 8) {
    short* q = zq + tid * 6 * 64;
    const int mx = tx * 8 + tid;
    const bool right = (2 * mx + 1) * 8 >= d.cols, bottom = (2 * ty + 1) * 8 >= d.rows;
    if (right) q[64] = q[0];
    if (bottom) q[128] = q[192] = q[64];
    else if (right) q[192] = q[128];
  }
  __syncthreads();
  // 4. the block goes out, and with it the length of its AC codes: thread j holds zig-zag positions 8 j .. 8 j + 7, the block's 8
  // threads (neighbouring lanes of one wave) share a mask of the non-zero positions, and the run before a coefficient is its distance
  // to the next set bit below it (position 0 counts as set: runs start after the DC)
  const uint4 q4 = b < nloc ? ((const uint4*)zq)[b * 8 + j] : make_uint4(0, 0, 0, 0);
  const uint32_t w[4] = {q4.x, q4.y, q4.z, q4.w};
  int c8[8];
  uint32_t m8 = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c8[i] = (int)(short)(w[i >> 1] >> ((i & 1) * 16));
    m8 |= (uint32_t)(c8[i] != 0) << i;
  }
  uint64_t mask = 1;
#pragma unroll
  for (int t8 = 0; t8 < 8; ++t8) mask |= (uint64_t)__shfl(m8, t8, 8) << (8 * t8);
  const uint32_t* hl = huff[table] + 16;
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = 8 * j + i;
    if (c8[i] != 0 && p > 0) {
      const int run = p - 1 - (63 - __clzll((long long)(mask & ((1ull << p) - 1))));
      const int nb = 32 - __clz(abs(c8[i]));
      bits += (uint32_t)(run >> 4) * (hl[0xF0] & 31) + (hl[((run & 15) << 4) | nb] & 31) + nb;
    }
  }
  if (j == 0 && !(mask >> 63)) bits += hl[0] & 31;                    // trailing zeros: EOB
  bits += __shfl_xor(bits, 1, 8);
  bits += __shfl_xor(bits, 2, 8);
  bits += __shfl_xor(bits, 4, 8);
  if (b < nloc && exists) {
    coef[(size_t)gidx * 8 + j] = q4;
    if (j == 0) side[gidx] = (bits << 16) | (uint32_t)(uint16_t)c8[0];
  }
}

// ---- entropy coding ---------------------------------------------------------------------------------------------------------------
// MSB-first words in LDS; neighbouring blocks share words, so every flush is an LDS atomic OR into zeroed words
struct BitSink {
  uint32_t* words;
  uint64_t acc = 0;
  int n, w;
  __device__ BitSink(uint32_t* words_, uint32_t pos) : words(words_), n(pos & 31), w(pos >> 5) {}
  __device__ void put(uint32_t code, int len) {           // len <= 26
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      atomicOr(words + w++, (uint32_t)(acc >> n));
    }
  }
  __device__ void finish() {
    if (n) atomicOr(words + w, (uint32_t)(acc << (32 - n)));
  }
};

// the previous block of the same component in scan order (-1: none)
__device__ inline int pred_block(int lb, bool colour) {
  if (!colour) return lb - 1;
  const int k = lb % 6;
  if (k == 0) return lb >= 6 ? lb - 3 : -1;
  if (k < 4) return lb - 1;
  return lb >= 6 ? lb - 6 : -1;
}

__device__ inline void code_block(const uint4* __restrict__ blk, int pred, const uint32_t* huff, BitSink& s) {
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    const uint4 q = blk[g];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = (int)(short)(w[i >> 1] >> ((i & 1) * 16));
      if ((g | i) == 0) {
        const int diff = c - pred;
        const int nb = 32 - __clz(abs(diff));             // 0 for diff == 0
        const uint32_t e = huff[nb];
        s.put(((e >> 5) << nb) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1)), (int)(e & 31) + nb);
      } else if (c == 0) {
        ++run;
      } else {
        while (run > 15) {
          const uint32_t z = huff[16 + 0xF0];
          s.put(z >> 5, (int)(z & 31));
          run -= 16;
        }
        const int nb = 32 - __clz(abs(c));
        const uint32_t e = huff[16 + ((run << 4) | nb)];
        s.put(((e >> 5) << nb) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << nb) - 1)), (int)(e & 31) + nb);
        run = 0;
      }
    }
  }
  if (run) {
    const uint32_t z = huff[16];
    s.put(z >> 5, (int)(z & 31));
  }
}

__global__ void __launch_bounds__(CHUNK) size_kernel(const FrameDesc* __restrict__ descs, int n_frames, const Tables* __restrict__ tabs,
                                                     const uint32_t* __restrict__ side, uint32_t* __restrict__ blk_off,
                                                     uint32_t* __restrict__ chunk_bits) {
  __shared__ uint32_t dclen[2][16];
  __shared__ uint32_t sh[CHUNK];
  const int tid = threadIdx.x;
  if (tid < 32) dclen[tid >> 4][tid & 15] = tabs->huff[tid >> 4][tid & 15] & 31;
  __syncthreads();
  const FrameDesc& d = descs[find_frame(descs, n_frames, (int)blockIdx.x, &FrameDesc::chunk0)];
  const bool colour = d.ch == 3;
  const int lb = ((int)blockIdx.x - d.chunk0) * CHUNK + tid;
  uint32_t bits = 0;
  if (lb < d.nblocks) {
    const int pb = pred_block(lb, colour);
    const uint32_t sd = side[d.block0 + lb];
    const int diff = (int)(short)(sd & 0xffff) - (pb < 0 ? 0 : (int)(short)(side[d.block0 + pb] & 0xffff));
    const int nb = 32 - __clz(abs(diff));
    bits = (sd >> 16) + dclen[colour && lb % 6 >= 4][nb] + nb;
  }
  uint32_t total;
  const uint32_t off = wg_scan<CHUNK>(bits, sh, tid, total);
  if (lb < d.nblocks) blk_off[d.block0 + lb] = off;
  if (tid == 0) chunk_bits[blockIdx.x] = total;
}

// one workgroup: per frame, exclusive scan of its chunk totals (in place) and the frame's bit count
__global__ void __launch_bounds__(256) chunk_scan_kernel(const FrameDesc* __restrict__ descs, int n_frames, uint32_t* __restrict__ chunk_bits,
                                                         uint32_t* __restrict__ frame_bits) {
  __shared__ uint32_t sh[256];
  const int tid = threadIdx.x;
  for (int f = 0; f < n_frames; ++f) {
    const int c0 = descs[f].chunk0, nc = descs[f].nchunks;
    uint32_t carry = 0;
    for (int b = 0; b < nc; b += 256) {
      const int c = b + tid;
      const uint32_t v = c < nc ? chunk_bits[c0 + c] : 0u;
      uint32_t total;
      const uint32_t ex = wg_scan<256>(v, sh, tid, total);
      if (c < nc) chunk_bits[c0 + c] = carry + ex;
      carry += total;
    }
    if (tid == 0) frame_bits[f] = carry;
  }
}

__global__ void __launch_bounds__(W_BLOCKS) write_kernel(const FrameDesc* __restrict__ descs, int n_frames, const Tables* __restrict__ tabs,
                                                         const uint4* __restrict__ coef, const uint32_t* __restrict__ side,
                                                         const uint32_t* __restrict__ blk_off, const uint32_t* __restrict__ chunk_base,
                                                         uint32_t* __restrict__ ustream) {
  __shared__ uint32_t huff[2][272];
  __shared__ uint32_t words[W_BLOCKS * BLOCK_WORDS + 2];
  const int tid = threadIdx.x;
  load_huff(huff, tabs, tid, W_BLOCKS);
  const int chunk = blockIdx.x >> 1, half = blockIdx.x & 1;
  const FrameDesc& d = descs[find_frame(descs, n_frames, chunk, &FrameDesc::chunk0)];
  const bool colour = d.ch == 3;
  const int lb0 = (chunk - d.chunk0) * CHUNK + half * W_BLOCKS;     // the workgroup's first block in the frame
  if (lb0 >= d.nblocks) return;
  const uint32_t base = chunk_base[chunk];
  const uint32_t p0 = base + blk_off[d.block0 + lb0];
  const bool last = lb0 + W_BLOCKS >= d.nblocks;                     // the frame's last workgroup also writes the padding
  const uint32_t p1 = last ? d.ubytes * 8u : (half ? chunk_base[chunk + 1] : base + blk_off[d.block0 + lb0 + W_BLOCKS]);
  const uint32_t w0 = p0 >> 5;
  const int nwords = (int)(((p1 + 31) >> 5) - w0);
  for (int i = tid; i < nwords; i += W_BLOCKS) words[i] = 0;
  __syncthreads();
  const int lb = lb0 + tid;
  if (lb < d.nblocks) {
    const int pb = pred_block(lb, colour);
    const int pred = pb < 0 ? 0 : (int)(short)(side[d.block0 + pb] & 0xffff);
    BitSink s(words, base + blk_off[d.block0 + lb] - (w0 << 5));
    code_block(coef + (size_t)(d.block0 + lb) * 8, pred, huff[colour && lb % 6 >= 4], s);
    if (lb == d.nblocks - 1) {                                       // the final partial byte is filled with 1-bits
      const int pad = (int)(d.ubytes * 8u - d.bits);
      if (pad) s.put((1u << pad) - 1, pad);
    }
    s.finish();
  }
  __syncthreads();
  uint32_t* out = ustream + (d.ubase >> 2) + w0;
  for (int i = tid; i < nwords; i += W_BLOCKS) {
    const uint32_t w = __builtin_bswap32(words[i]);                  // the stream is big-endian
    if (i == 0 || i == nwords - 1) {
      if (w) atomicOr(out + i, w);                                   // a word shared with the neighbouring workgroup
    } else {
      out[i] = w;
    }
  }
}

// stuffing.  SCATTER = false: out bytes of each 1 KB chunk; true: write them at the chunk's scanned position
template <bool SCATTER>
__global__ void __launch_bounds__(S_THREADS) stuff_kernel(const FrameDesc* __restrict__ descs, int n_frames, const uint32_t* __restrict__ ustream,
                                                          uint32_t* __restrict__ cnt, uint8_t* __restrict__ out) {
  __shared__ uint32_t sh[S_THREADS];
  const int tid = threadIdx.x;
  const FrameDesc& d = descs[find_frame(descs, n_frames, (int)blockIdx.x, &FrameDesc::schunk0)];
  const uint32_t off = ((uint32_t)blockIdx.x - d.schunk0) * S_CHUNK + 4 * tid;        // byte in the frame's unstuffed scan
  const int nv = off >= d.ubytes ? 0 : (int)min(4u, d.ubytes - off);
  const uint32_t w = nv ? ustream[(d.ubase + off) >> 2] : 0u;
  int c = nv;
  for (int b = 0; b < nv; ++b) c += ((w >> (8 * b)) & 0xff) == 0xff;
  uint32_t total;
  const uint32_t ex = wg_scan<S_THREADS>((uint32_t)c, sh, tid, total);
  if (!SCATTER) {
    if (tid == 0) cnt[blockIdx.x] = total;
  } else {
    uint8_t* o = out + cnt[blockIdx.x] + ex;
    for (int b = 0; b < nv; ++b) {
      const uint8_t v = (uint8_t)(w >> (8 * b));
      *o++ = v;
      if (v == 0xff) *o++ = 0;
    }
  }
}

// one workgroup: exclusive scan of the chunk counts over all frames (in place); frame_out[f] = where frame f's stuffed scan starts,
// frame_out[n] = the total
__global__ void __launch_bounds__(256) stuff_scan_kernel(const FrameDesc* __restrict__ descs, int n_frames, int n_chunks, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ frame_out) {
  __shared__ uint32_t sh[256];
  const int tid = threadIdx.x;
  uint32_t carry = 0;
  for (int b = 0; b < n_chunks; b += 256) {
    const int c = b + tid;
    const uint32_t v = c < n_chunks ? cnt[c] : 0u;
    uint32_t total;
    const uint32_t ex = wg_scan<256>(v, sh, tid, total);
    if (c < n_chunks) cnt[c] = carry + ex;
    carry += total;
  }
  __syncthreads();
  for (int f = tid; f < n_frames; f += 256) frame_out[f] = cnt[descs[f].schunk0];
  if (tid == 0) frame_out[n_frames] = carry;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.1 / K.2 (natural order) and K.3 - K.6
static const uint8_t BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,  69,  56, 14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

static void quant_table(int quality, int t, uint8_t* q /* natural order */) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;      // the IJG quality scaling
  for (int i = 0; i < 64; ++i) q[i] = (uint8_t)std::min(std::max((BASE_Q[t][i] * scale + 50) / 100, 1), 255);
}

// canonical codes (T.81 Annex C) of a table into out[symbol] = (code << 5) | length
static void huff_table(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (code++ << 5) | (uint32_t)len;
    code <<= 1;
  }
}

static void make_tables(int quality, Tables& t) {
  memset(&t, 0, sizeof t);
  static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  for (int c = 0; c < 2; ++c) {
    uint8_t q[64];
    quant_table(quality, c, q);
    for (int i = 0; i < 64; ++i) {
      const uint32_t d = 8u * q[i];
      t.qm[c][i] = (uint32_t)((1ull << 32) / d) + 1;
      t.qh[c][i] = d >> 1;
    }
    huff_table(DC_BITS[c], dc_vals, t.huff[c]);
    huff_table(AC_BITS[c], AC_VALS[c], t.huff[c] + 16);
  }
  for (int i = 0; i < 64; ++i) t.zz[ZIGZAG[i]] = i;
}

static void put_marker(std::vector<uint8_t>& o, int tag, const std::vector<uint8_t>& payload) {
  const size_t len = payload.size() + 2;
  o.insert(o.end(), {0xFF, (uint8_t)tag, (uint8_t)(len >> 8), (uint8_t)len});
  o.insert(o.end(), payload.begin(), payload.end());
}

// everything before the scan, in libjpeg's order: SOI, APP0, DQT per table, SOF0, DHT per table, SOS
static std::vector<uint8_t> make_headers(int H, int W, int C, int quality) {
  std::vector<uint8_t> o = {0xFF, 0xD8};
  put_marker(o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  const int nt = C == 3 ? 2 : 1;
  for (int t = 0; t < nt; ++t) {
    uint8_t q[64];
    quant_table(quality, t, q);
    std::vector<uint8_t> p = {(uint8_t)t};
    for (int i = 0; i < 64; ++i) p.push_back(q[ZIGZAG[i]]);
    put_marker(o, 0xDB, p);
  }
  std::vector<uint8_t> sof = {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, (uint8_t)C};
  if (C == 3) sof.insert(sof.end(), {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  else sof.insert(sof.end(), {1, 0x11, 0});
  put_marker(o, 0xC0, sof);
  for (int t = 0; t < nt; ++t) {
    std::vector<uint8_t> p = {(uint8_t)t};
    p.insert(p.end(), DC_BITS[t], DC_BITS[t] + 16);
    for (int i = 0; i < 12; ++i) p.push_back((uint8_t)i);
    put_marker(o, 0xC4, p);
    p.assign(1, (uint8_t)(0x10 | t));
    p.insert(p.end(), AC_BITS[t], AC_BITS[t] + 16);
    p.insert(p.end(), AC_VALS[t], AC_VALS[t] + 162);
    put_marker(o, 0xC4, p);
  }
  if (C == 3) put_marker(o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  else put_marker(o, 0xDA, {1, 1, 0x00, 0, 63, 0});
  return o;
}

}  // namespace jpeg_enc

using namespace jpeg_enc;

struct rtd_jpeg : bk::Base {
  bk::OwnStream q;
  bk::PinBuf pin;            // pinned: [descriptors | tables | host frames] on the way in, the sizes and the stuffed scans on the way out
  bk::DevBuf in, coef, side, blk_off, chunks, sizes, ustream, scnt, out;
  std::map<std::tuple<int, int, int, int>, std::vector<uint8_t>> headers;   // the marker block per (H, W, C, quality), built once
  int64_t last_values = 0;   // int16 coefficients of the last call
};

namespace jpeg_enc {

static void encode(rtd_jpeg* j, int n, const uint8_t* const* frames, const int32_t* hwc, int on_device, int quality, uint8_t* out,
                   int64_t out_cap, int64_t* offsets) {
  hipStream_t s = j->q.stream;
  // ---- layout of the upload: descriptors, tables, host frames
  const size_t tab_off = align_up(sizeof(FrameDesc) * n, 256);
  const size_t frames_off = align_up(tab_off + sizeof(Tables), 256);
  std::vector<size_t> foff;
  const size_t total = bk::stage_offsets(n, hwc, on_device, frames_off, foff);
  j->pin.reserve(std::max(total, frames_off + (size_t)(n + 1) * 4));      // (the sizes come back through the frames' staging area)
  j->in.reserve(total);
  FrameDesc* descs = (FrameDesc*)j->pin.p;
  int tiles = 0, blocks = 0, chunks = 0;
  for (int i = 0; i < n; ++i) {
    const int H = hwc[3 * i], W = hwc[3 * i + 1], C = hwc[3 * i + 2];
    FrameDesc& d = descs[i];
    memset(&d, 0, sizeof d);
    d.src = on_device ? frames[i] : j->in.p + foff[i];
    d.rows = H;
    d.cols = W;
    d.ch = C;
    const int unit = C == 3 ? 16 : 8;
    d.bx = (W + unit - 1) / unit;
    d.by = (H + unit - 1) / unit;
    d.tiles_x = (W + TILE_W - 1) / TILE_W;
    d.tile0 = tiles;
    tiles += d.tiles_x * ((H + TILE_H - 1) / TILE_H);
    d.block0 = blocks;
    d.nblocks = d.bx * d.by * (C == 3 ? 6 : 1);
    blocks += d.nblocks;
    d.chunk0 = chunks;
    d.nchunks = (d.nblocks + CHUNK - 1) / CHUNK;
    chunks += d.nchunks;
    if (!on_device) memcpy(j->pin.p + foff[i], frames[i], (size_t)H * W * C);
  }
  make_tables(quality, *(Tables*)(j->pin.p + tab_off));
  j->coef.reserve((size_t)blocks * 128);
  j->side.reserve((size_t)blocks * 4);
  j->blk_off.reserve((size_t)blocks * 4);
  j->chunks.reserve((size_t)(chunks + 1) * 4);
  j->sizes.reserve((size_t)(n + 1) * 4);
  const FrameDesc* ddev = (const FrameDesc*)j->in.p;
  const Tables* tdev = (const Tables*)(j->in.p + tab_off);
  uint4* coef = (uint4*)j->coef.p;
  uint32_t* side = (uint32_t*)j->side.p;
  uint32_t* blk_off = (uint32_t*)j->blk_off.p;
  uint32_t* chunk_bits = (uint32_t*)j->chunks.p;
  uint32_t* sizes = (uint32_t*)j->sizes.p;
  j->last_values = 0;

  // ---- transform, size, scan: the bit count of every frame comes back
  HIP_CHECK(hipMemcpyAsync(j->in.p, j->pin.p, total, hipMemcpyHostToDevice, s));
  rtd::rtd_launch(transform_kernel, dim3(tiles), dim3(T_THREADS), 0, s, ddev, n, tdev, coef, side);
  rtd::rtd_launch(size_kernel, dim3(chunks), dim3(CHUNK), 0, s, ddev, n, tdev, (const uint32_t*)side, blk_off, chunk_bits);
  rtd::rtd_launch(chunk_scan_kernel, dim3(1), dim3(256), 0, s, ddev, n, chunk_bits, sizes);
  HIP_CHECK(hipGetLastError());
  uint32_t* got = (uint32_t*)(j->pin.p + frames_off);            // (the staged frames are on the device by then: stream order)
  HIP_CHECK(hipMemcpyAsync(got, sizes, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  j->last_values = (int64_t)blocks * 64;

  // ---- place the frames in the unstuffed buffer
  size_t ubytes = 0;
  int schunks = 0;
  for (int i = 0; i < n; ++i) {
    FrameDesc& d = descs[i];
    d.bits = got[i];
    d.ubytes = (d.bits + 7) / 8;
    d.ubase = (uint32_t)ubytes;
    d.schunk0 = schunks;
    schunks += (int)((d.ubytes + S_CHUNK - 1) / S_CHUNK);
    ubytes += align_up(d.ubytes, S_CHUNK);
    RTD_CHECK(ubytes < (1ull << 31), RTD_E_INVALID, "the batch codes into more than 2 GiB");
  }
  j->ustream.reserve(ubytes + 8);
  j->out.reserve(2 * ubytes + 8);                              // every byte could be 0xFF
  j->scnt.reserve((size_t)(schunks + 1) * 4);
  uint32_t* scnt = (uint32_t*)j->scnt.p;
  HIP_CHECK(hipMemcpyAsync(j->in.p, j->pin.p, sizeof(FrameDesc) * n, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(j->ustream.p, 0, ubytes + 8, s));
  rtd::rtd_launch(write_kernel, dim3(2 * chunks), dim3(W_BLOCKS), 0, s, ddev, n, tdev, (const uint4*)coef, (const uint32_t*)side,
                  (const uint32_t*)blk_off, (const uint32_t*)chunk_bits, (uint32_t*)j->ustream.p);
  rtd::rtd_launch(stuff_kernel<false>, dim3(schunks), dim3(S_THREADS), 0, s, ddev, n, (const uint32_t*)j->ustream.p, scnt, j->out.p);
  rtd::rtd_launch(stuff_scan_kernel, dim3(1), dim3(256), 0, s, ddev, n, schunks, scnt, sizes);
  rtd::rtd_launch(stuff_kernel<true>, dim3(schunks), dim3(S_THREADS), 0, s, ddev, n, (const uint32_t*)j->ustream.p, scnt, j->out.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(got, sizes, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));

  // ---- sizes are known: check the capacity, fetch the scans, write the files
  std::vector<uint32_t> start(got, got + n + 1);
  std::vector<const std::vector<uint8_t>*> hdr(n);
  int64_t need = 0;
  if (j->headers.size() >= 64) j->headers.clear();            // a caller that keeps changing sizes or qualities: start over
  for (int i = 0; i < n; ++i) {
    const auto key = std::make_tuple(hwc[3 * i], hwc[3 * i + 1], hwc[3 * i + 2], quality);
    auto it = j->headers.find(key);
    if (it == j->headers.end()) it = j->headers.emplace(key, make_headers(hwc[3 * i], hwc[3 * i + 1], hwc[3 * i + 2], quality)).first;
    hdr[i] = &it->second;
    offsets[i] = need;
    need += (int64_t)hdr[i]->size() + (start[i + 1] - start[i]) + 2;
  }
  offsets[n] = need;
  RTD_CHECK(out_cap >= need, RTD_E_INVALID, "out_cap is " + std::to_string(out_cap) + " bytes, " + std::to_string(need) + " are needed");
  j->pin.reserve(start[n]);
  if (start[n]) {
    HIP_CHECK(hipMemcpyAsync(j->pin.p, j->out.p, start[n], hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  for (int i = 0; i < n; ++i) {
    uint8_t* o = out + offsets[i];
    memcpy(o, hdr[i]->data(), hdr[i]->size());
    o += hdr[i]->size();
    memcpy(o, j->pin.p + start[i], start[i + 1] - start[i]);
    o += start[i + 1] - start[i];
    o[0] = 0xFF;
    o[1] = 0xD9;
  }
}

}  // namespace jpeg_enc

extern "C" {

int rtd_jpeg_create(int32_t device, rtd_jpeg_handle* out) {
  return bk::create(out, rtd_jpeg_destroy, [&](rtd_jpeg* j) {
    bk::use_device(device);
    j->device = device;
    j->q.open();
  });
}

int rtd_jpeg_encode(rtd_jpeg_handle j, int32_t n, const uint8_t* const* frames, const int32_t* hwc, int32_t frames_on_device, int32_t quality,
                    uint8_t* out, int64_t out_cap, int64_t* offsets) {
  return guarded(j, [&] {
    RTD_CHECK(n >= 0, RTD_E_INVALID, "n must be >= 0");
    RTD_CHECK(offsets, RTD_E_INVALID, "null argument");
    offsets[0] = 0;
    if (n == 0) return;
    RTD_CHECK(frames && hwc && (out || out_cap <= 0), RTD_E_INVALID, "null argument");
    RTD_CHECK(quality >= 1 && quality <= 100, RTD_E_INVALID, "quality must be in 1..100, got " + std::to_string(quality));
    for (int i = 0; i < n; ++i) {
      RTD_CHECK(frames[i], RTD_E_INVALID, "frame " + std::to_string(i) + " is null");
      RTD_CHECK(hwc[3 * i] >= 1 && hwc[3 * i + 1] >= 1 && hwc[3 * i] <= 65535 && hwc[3 * i + 1] <= 65535, RTD_E_INVALID,
                "frame " + std::to_string(i) + " has a bad size (1..65535 per side)");
      RTD_CHECK(hwc[3 * i + 2] == 1 || hwc[3 * i + 2] == 3, RTD_E_INVALID, "frames must have 1 or 3 channels");
      RTD_CHECK((int64_t)(hwc[3 * i] + 15) * (hwc[3 * i + 1] + 15) <= (1ll << 24), RTD_E_INVALID,
                "frame " + std::to_string(i) + " has more than 16 Mpixel (bit offsets inside a frame are 32-bit)");
    }
    HIP_CHECK(hipSetDevice(j->device));
    try {
      encode(j, n, frames, hwc, frames_on_device, quality, out, out_cap, offsets);
    } catch (...) {
      j->q.drain();                                        // nothing of a failed call may still read the staging buffers
      throw;
    }
  });
}

int rtd_jpeg_wait_stream(rtd_jpeg_handle j, void* producer_stream) {
  return guarded(j, [&] {
    HIP_CHECK(hipSetDevice(j->device));
    j->q.wait_for(producer_stream);
  });
}

const char* rtd_jpeg_last_error(rtd_jpeg_handle j) { return bk::last_error(j); }

void rtd_jpeg_destroy(rtd_jpeg_handle j) {
  if (!j) return;
  (void)hipSetDevice(j->device);
  j->q.drain();
  for (bk::DevBuf* b : {&j->in, &j->coef, &j->side, &j->blk_off, &j->chunks, &j->sizes, &j->ustream, &j->scnt, &j->out}) b->release();
  j->pin.release();
  j->q.close();
  delete j;
}

int rtd_debug_jpeg_coefficients(rtd_jpeg_handle j, int16_t* out, int64_t capacity, int64_t* count) {
  return guarded(j, [&] {
    RTD_CHECK(count, RTD_E_INVALID, "null argument");
    *count = j->last_values;
    if (!out) return;
    RTD_CHECK(capacity >= j->last_values, RTD_E_INVALID, "output buffer too small");
    if (!j->last_values) return;
    HIP_CHECK(hipSetDevice(j->device));
    HIP_CHECK(hipMemcpyAsync(out, j->coef.p, (size_t)j->last_values * 2, hipMemcpyDeviceToHost, j->q.stream));
    HIP_CHECK(hipStreamSynchronize(j->q.stream));
  });
}

}  // extern "C"
