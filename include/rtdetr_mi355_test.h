/* rtdetr_mi355_test.h - kernel-level TEST, BENCH and DEBUG entry points of libmi355rtdetr.so.
 *
 * Nothing in this header has a counterpart in the reference and nothing here is on the detection path: the product API
 * (what a reference-side binding uses) is rtdetr_mi355.h.  Callers: tests/, tools/ and the diagnostic legs of bench.py
 * (per-kernel timing for the roofline object, the sustained-MFMA probe).  Implemented in csrc/testapi.hip.
 */
#ifndef RTDETR_MI355_TEST_H
#define RTDETR_MI355_TEST_H

#include "rtdetr_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-kernel timing record filled by rtd_profile */
typedef struct rtd_layer_time {
  char name[48];
  char kernel[24];  /* kernel family: "conv_igemm", "layernorm", ... */
  float ms;         /* mean HIP-event time over `reps` launches on the handle's stream */
  double flops;     /* algorithmic flops of one launch (2 flop / MAC) */
  double bytes;     /* algorithmic bytes of one launch (in + out + weights, unfused) */
} rtd_layer_time;

/* ---- introspection used by tests / bench (no reference counterpart) -------------------------- */
/* copy a named intermediate tensor of the last forward to the host as fp32; shape = (n, h, w, c) */
int rtd_debug_tensor(rtd_handle h, const char* name, float* out, int64_t capacity, int64_t shape[4]);
/* force the encoder top-k selection of the next forwards (idx[n][Q] memory-token ids, NULL = off):
 * lets stage-level parity tests separate selection flips from decoder arithmetic */
int rtd_debug_force_topk(rtd_handle h, const int32_t* idx, int32_t n);
/* time every kernel of one forward of batch n with HIP events on the handle's stream */
int rtd_profile(rtd_handle h, int32_t n, int32_t reps, rtd_layer_time* out, int32_t capacity, int32_t* count);
/* A/B switches for tests and profiling (defaults in brackets; unknown names return RTD_E_INVALID).  Every switch edits a process-wide
 * TEMPLATE that rtd_create snapshots into the handle: a call changes handles created AFTERWARDS (and the kernel-level rtd_op_* /
 * rtd_bench_* entry points below, which read the template when called) - never a live handle, so two handles of one process cannot see
 * each other's settings and all plans of a handle (one per batch size, built lazily) agree with each other.
 * Conv dispatch, bf16 / fp32 operands (csrc/common.h ConvOpts; one tile family since round 5):
 *   conv_mode [0]   0 auto | 1 register-staged fallback kernel only | 3, 4 wave-specialised LDS-DMA tile with 4 / 2 stages everywhere |
 *                   10 128 x 64 tile everywhere
 *   ws2_min_blocks [257], ws64_max_blocks [160], glds_min_blocks [4], glds_min_n [128], reg_epilogue [1], prefetch [1]
 *   conv_reg [3] (pair operands too): bit 0 direct 3x3 kernels for the narrow stem / stage-0 layers, bit 1 the 64-channel pair kernel
 * Conv dispatch, pair operands (RTD_PREC_F16X3): split_ws2_min_blocks [257] | split_ws64_max_blocks [160] |
 *   split_flex [1: flexible tile heights on grids of <= split_flex_small_max [200] tiles], split_flex_min_nk [4] |
 *   split_k2 [1: two-pass split-K on >= 128 K-steps with <= 16 tiles per image] |
 *   split_wsq [1: 160..256-pixel tiles at one block per CU on grids of >= split_wsq_min_blocks [257] tiles with >= split_wsq_min_nk [24] K-steps] |
 *   split_sx [3: streaming 1x1 kernel 0 off, 1 stage-0 shapes, 2 + K = 128, 3 + K = 256 -> N >= 1024 (value projection), 4 + with residual (slower)]
 * Plan building:
 *   sc_fold [1] projection shortcut folded into the block's last conv | up_fold [1] FPN upsample folded into the CSP's first conv |
 *   c1_fuse [1] a block's reduce conv computed inside the previous block's expand conv (bf16: stage 0/1; f16x3: stage 0 and the first block
 *   of stage 1) | attn_split [3] self-attention on fp16-pair MFMAs (bit 0 the fused AIFI layer, bit 1 decoder) |
 *   arena_reuse [1] | stem_fused_split [1] (f16x3): stem.0 straight from the uint8 frames | stem_pool_fuse [1] (f16x3): stem.2 and the 3x3/s2
 *   max-pool in one pass | avg_fuse [1] (f16x3): a stage's last expand conv also writes the next stage's vd-shortcut average |
 *   post_fused [1] sigmoid + top-k + box decode of the post-processor in one launch |
 *   dead_out [1] (f16x3): the stage-0 output is not written when its only readers are that launch's fused follower conv and fused average |
 *   aifi_pair [1] (f16x3): the un-fused AIFI's linears on the pair kernels | side_stream [7: bit 0 query
 *   selection on a second stream beside the value projection, bit 1 decoder input projections beside the PAN path, bit 2 encoder input
 *   projections beside stages 2 / 3 and AIFI] | dec_fused [1] | sel_fused [1]
 * Tools: profile_twice [0], bench_rewarm [0: bit 5 = rtd_bench_conv fills its operands with random fp16 values instead of zeros].
 * "reset" (any value): every template back to the values in brackets. */
int rtd_debug_option(const char* name, int value);

/* ---- kernel-level test entry points (device pointers; dtype 0 = bf16, 1 = fp32, 4 = F16X2: hi/lo fp16 pairs in 32-channel groups
 * [32 hi | 32 lo], 4 bytes per channel - the storage of RTD_PREC_F16X3, rtd_op_conv / rtd_op_conv_dual only) --------------- */
int rtd_op_conv(int dtype, const void* x, const void* w_ohwi_f32, const float* bias, const void* res,
                void* y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                int act, int res_mode, int out_f32);
/* ... on channel-slice views: x, y and res are [B, H, W, .] with pixel strides ldx >= Cin, ldy >= Cout, ldres >= Cout (in channels),
 * images dense - how a dense block reads the prefix of a wider buffer and writes its channels behind it.  act: 0 none, 1 ReLU, 2 SiLU,
 * 3 GELU, 4 LeakyReLU(0.2) (rtd_op_conv too). */
int rtd_op_conv_view(int dtype, const void* x, int ldx, const void* w_ohwi_f32, const float* bias, const void* res, int ldres,
                     void* y, int ldy, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int act, int res_mode);
/* conv with a second input x2 [B,OH,OW,C2] read as an extra 1x1 tap at output resolution; w_f32 = [Cout][KH*KH*Cin + C2]
 * (how the plan folds a bottleneck's projection shortcut into its last conv).  x_up2 = 1 (1x1 only): x is [B,H/2,W/2,Cin] and is
 * read through a nearest 2x upsampling, H and W being the output extents (the FPN's conv over cat([upsample(lat), proj])). */
int rtd_op_conv_dual(int dtype, const void* x, const void* x2, const void* w_f32, const float* bias, const void* res,
                     void* y, int B, int H, int W, int Cin, int C2, int Cout, int KH, int stride, int pad,
                     int act, int res_mode, int out_f32, int x_up2);
/* rtd_op_conv_dual on channel-slice views: x, x2, res and y are [B, ., ., .] with pixel strides ldx >= Cin, ldx2 >= C2, ldres >= Cout,
 * ldy >= Cout (in channels), images dense inside each buffer (batch stride = h * w * ld) - how the networks write the halves of a concat
 * buffer and read a slice of one (Tensor::slice_c).  x2 may be NULL (C2, ldx2 ignored; x_up2 then refused), res may be NULL.  H and W are
 * the input extents (x_up2 = 1: the output extents), out_f32 = 1 writes fp32 rows (ldy in fp32 channels). */
int rtd_op_conv_views(int dtype, const void* x, int ldx, const void* x2, int C2, int ldx2, const void* w_f32, const float* bias,
                      const void* res, int ldres, void* y, int ldy, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad,
                      int act, int res_mode, int out_f32, int x_up2);
/* 1x1 conv (optionally with a second input, as rtd_op_conv_dual) with the FOLLOWING 1x1 conv Cout -> Cnext fused into the launch
 * (how the plan runs a bottleneck's reduce conv inside the previous block's expand conv): y = act(W [x | x2] + b (+ res)),
 * y1 = next_act(W1 y + b1), both written.  dtype 1 (bf16) / 4 (f16x2); RTD_E_INVALID for shapes the streaming kernels do not take. */
int rtd_op_conv_next(int dtype, const void* x, const void* x2, const void* w_f32, const float* bias, const void* res, void* y,
                     const void* w1_f32, const float* bias1, void* y1, int B, int H, int W, int Cin, int C2, int Cout, int Cnext,
                     int act, int res_mode, int next_act);
/* ... on F16X2 operands, with the 2 x 2 / stride-2 average of y written by the same launch: avg_y [B, H/2, W/2, Cout] (how the plan ends a
 * stage of a vd net: ConvArgs::avg_y).  Cnext = 0: no follower (w1_f32, bias1, y1 may be NULL).  y_dead = 1 (with a follower): the
 * launch drops the stores of y - the call still takes a y buffer and leaves it untouched.  RTD_E_INVALID before any launch, with
 * nothing written, for what conv_avg_supported() refuses (odd H, W % 16 != 0, no residual, other channel counts than 64 -> 256 + a
 * 128-channel follower or 128 -> N alone, maps below 80 x 80). */
int rtd_op_conv_avg(const void* x, const void* w_f32, const float* bias, const void* res, void* y, const void* w1_f32, const float* bias1,
                    void* y1, void* avg_y, int B, int H, int W, int Cin, int Cout, int Cnext, int act, int res_mode, int next_act,
                    int y_dead);
/* stem.2 and the max-pool in one pass (launch_conv_pool): x [B, H, W, 32] F16X2, w_ohwi_f32 [64][3][3][32], ReLU, then 3x3 / stride 2 /
 * pad 1 max -> pooled [B, H/2, W/2, 64] F16X2; the conv rows are never written.  RTD_E_INVALID before any launch for what
 * conv_pool_supported() refuses (odd extents, fewer than 32 tiles of 8 x 32 pixels per image, conv_reg 0). */
int rtd_op_conv_pool(const void* x, const void* w_ohwi_f32, const float* bias, void* pooled, int B, int H, int W);
/* backbone.stem.0 of the f16x3 engine straight from uint8 frames (stem0_u8_kernel: 3x3 / stride 2 / pad 1, BGR byte cb -> model channel
 * 2 - cb, pixel = (float)v / 255.0f as a hi / lo pair).  frames_dev: a HOST array of n device pointers, each an [H][W][3] BGR frame at ANY
 * byte address; w_ohwi_f32 [32][3][3][8] (device; channels = RGB + 5 pad the kernel never reads) and bias [32] (device) are staged as the
 * engine stages backbone.stem.0; y = F16X2 [n][OH][OW][32] dense, OH = (H - 1) / 2 + 1.  act: 0 none, 1 ReLU, 2 SiLU.  RTD_E_INVALID before
 * any launch, with nothing written, for n outside 1..64 (RTD_MAX_BATCH), a null pointer (a frame's included), extents < 1 or another act. */
int rtd_op_stem0_u8(const uint8_t* const* frames_dev, int n, int H, int W, const void* w_ohwi_f32, const float* bias, void* y, int act);

/* ---- which conv kernel: the choice behind launch_conv, readable.  Host arithmetic only: no device call, usable without a GPU.
 * A choice is a text key naming ONE instantiation plus info[12] = family, stages, bn, mt, bm, smallc, wsq, sx, cog, S, grid, ntn
 * (family: 0 tile, 1 ws, 2 sx, 3 reg3x3, 4 reg3x3_64, 5 wsf, 6 wsq, 7 wsx; S = slices of the two-pass split-K, > 1: k_splitk_reduce
 * follows; grid in blocks; fields a family does not use are 0, wsq / sx -1).  Keys:
 *   tile.<bf16|f32>.<BM>x<BN>.smallc<0|1>   conv_igemm_kernel          ws.<bf16|f32>.s<stages>.bn<BN>   conv_igemm_ws_kernel
 *   wsx.s<stages>.bn<BN>                    conv_igemm_wsx_kernel      wsf.s<stages>.bn<BN>.mt<MT>      conv_igemm_wsf_kernel
 *   wsq.<MTA>x<MTB>                         conv_igemm_wsq_kernel      reg3x3_64                        conv3x3_reg_split64_kernel
 *   reg3x3.cog<1|2>[.pool]                  conv3x3_reg_split_kernel (.pool: <2, true> + k_pool_fixup)
 *   sx.x<NGX>.x2_<NG2>.res<0|1>.next<N>.f32_<0|1>.avg<0|1>             conv1x1_sx_kernel
 * rtd_debug_conv_choice: what launch_conv would launch NOW (the rtd_debug_option template as it stands) for the launch rtd_op_conv /
 *   _dual / _next / _avg / _pool would describe: dense tensors, res and x2 in `dtype`, H and W the input extents (x_up2: the output
 *   extents), Cnext = 0 no follower, avg / pool 0 or 1 (pool: the launch_conv_pool form).  It runs the launchers' own checks and choice
 *   functions: a launch they refuse is refused here with the same error (rtd_last_error(NULL)).
 * rtd_debug_last_conv: what the calling thread's last launch_conv / launch_conv_pool did launch (RTD_E_STATE before the first).
 * rtd_debug_conv_instantiations: the keys of every instantiation the launchers can name, one per line, generated from the tables the
 *   launchers instantiate from; *needed = bytes including the final NUL (out may be NULL to ask). */
int rtd_debug_conv_choice(int dtype, int B, int H, int W, int Cin, int C2, int Cout, int KH, int stride, int pad, int res_mode, int out_f32,
                          int x_up2, int Cnext, int avg, int pool, char* key, int key_capacity, int32_t* info);
/* ... for the launch rtd_op_conv_views would describe: the same views (C2 = 0: no second input, res_mode = 0: no residual) behind 16-byte
 * aligned probe addresses; same outputs, same refusals. */
int rtd_debug_conv_choice_views(int dtype, int ldx, int C2, int ldx2, int ldres, int ldy, int B, int H, int W, int Cin, int Cout, int KH,
                                int stride, int pad, int res_mode, int out_f32, int x_up2, char* key, int key_capacity, int32_t* info);
int rtd_debug_last_conv(char* key, int key_capacity, int32_t* info);
int rtd_debug_conv_instantiations(char* out, int64_t capacity, int64_t* needed);
int rtd_op_layernorm(int dtype, const void* x, const void* res, const float* g, const float* b,
                     void* y, int rows, int dim, int out_f32);
int rtd_op_attention(int dtype, const void* qk, const void* v, void* o, int B, int L, int heads, int hd);
int rtd_op_msdeform(int dtype, const void* value, const float* offaw, const float* ref, float* out,
                    int B, int Q, int heads, int hd, int n_levels, int n_points, const int32_t* level_hw,
                    int value_ld, float offset_scale);
/* ... with the value rows as the engine holds them: [B, S, value_ld] with this layer's heads * hd channels at channel offset value_coff
 * (the decoder samples a 256-channel slice of the dec_layers * 256 wide projection of all layers); RTD_E_INVALID before any device work
 * when hd != 32 or the slice leaves the row */
int rtd_op_msdeform_view(int dtype, const void* value, int value_ld, int value_coff, const float* offaw, const float* ref, float* out,
                         int B, int Q, int heads, int hd, int n_levels, int n_points, const int32_t* level_hw, float offset_scale);
/* ... sampled as RTD_DEC_DISCRETE does: one nearest tap per point, clamped into the map (k_msdeform<DEC_DISCRETE, ...>); same arguments and checks */
int rtd_op_msdeform_discrete_view(int dtype, const void* value, int value_ld, int value_coff, const float* offaw, const float* ref, float* out,
                                  int B, int Q, int heads, int hd, int n_levels, int n_points, const int32_t* level_hw, float offset_scale);
/* ---- query selection (decoder.hip).  x = [B * S] fp32 rows of K = 256 channels with row stride ldx; w_f32 = [C][K] row-major and
 * bias = [C] (device, fp32: packed here exactly as the engine packs dec.enc_score); g, b = the LayerNorm's [256].
 * select_score: mx[B * S] = max over classes of (LayerNorm(x) W^T + bias).  gather_ln: dst[b][q][0:256] = LayerNorm(x[b][idx[b][q]]) with
 * row stride ldd; an index outside [0, S) is clamped to the nearest valid row. */
int rtd_op_select_score(const float* x, int ldx, const float* w_f32, const float* bias, const float* g, const float* b, float* mx,
                        int B, int S, int C, int K);
int rtd_op_gather_ln(const float* x, int ldx, int S, const int32_t* idx, int B, int Q, const float* g, const float* b, float* dst, int ldd);
/* fp32 rows <-> pair (F16X2) rows, C % 32 == 0, lds / ldd = row strides in channels: direction 0 = fp32 -> pair, 1 = pair -> fp32,
 * 2 = ADD the number of hi halves at +-65504 among the rows * lds * 2 16-bit words at src to the uint64 at dst (rtd_self_check's scan) */
int rtd_op_split_convert(int direction, const void* src, void* dst, int64_t rows, int C, int64_t lds, int64_t ldd);
/* the decoder's glue kernels (ops.hip), device pointers, strides in elements:
 * set_rows: y[b][rows[i]][0:C] = vec for every image b and i < nrows (y = [B][rows_per_image] rows of stride ld; rows[] in range)
 * rowmax: out[r] = max(x[r][0:C]), fp32
 * gather_rows: dst[b][q][0:C] (fp32, stride ldd) = src[b][clamp(idx[b][q], 0, S - 1)][0:C] (src_dtype 0 bf16 / 1 fp32, stride lds)
 * boxes: anchors != NULL: ref_unact8[t][0:4] = delta[t][0:4] + anchors[clamp(idx[t], 0, S - 1)], ref8 = sigmoid(.), lanes 4..7 of both zero;
 *        anchors == NULL: ref8[t][0:4] = sigmoid(delta[t][0:4] + inverse_sigmoid(ref8[t][0:4])) in place (delta rows of stride ldd)
 * add: y = a + b on [B][rows][C] dense tensors of the given dtypes; b_broadcast: b is [1][rows][C], read for every image */
int rtd_op_set_rows(int dtype, void* y, int ld, int C, const int32_t* rows, int nrows, int rows_per_image, const float* vec, int B);
int rtd_op_rowmax(const float* x, int ld, int C, int rows, float* out);
int rtd_op_gather_rows(int src_dtype, const void* src, int lds, int S, const int32_t* idx, int B, int Q, int C, float* dst, int ldd);
int rtd_op_boxes(const float* delta, int ldd, int rows, float* ref8, const float* anchors, const int32_t* idx, int S, float* ref_unact8);
int rtd_op_add(int dt_a, int dt_b, int dt_y, const void* a, const void* b, void* y, int B, int rows, int C, int b_broadcast);
/* the post-processor: logits [B * Q][C], ref8 [B * Q][8] cxcywh, scale_wh [B][2] -> block6 [B][K][6] = label, score, x1, y1, x2, y2 (K == Q).
 * fused 1 = the one-launch form (RTD_E_INVALID when it does not take the shape: never a fall-back), 0 = sigmoid + top-k + gather */
int rtd_op_postprocess(const float* logits, const float* ref8, const float* scale_wh, int B, int Q, int C, int K, int fused, float* block6);
/* the glue ops on an NHWC view x = [B, H, W, C] with pixel stride ldx (>= C: a channel slice), images dense: kind 0 = max-pool 3x3 / stride 2 /
 * pad 1, 1 = 2x2 average (even H, W), 2 = nearest 2x upsample; dtype 0 bf16, 1 fp32, 4 F16X2; y = [B, OH, OW, C] with pixel stride ldy */
int rtd_op_pool(int kind, int dtype, const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy);
int rtd_op_topk(const float* keys, int B, int N, int K, int32_t* idx_out, float* val_out);
int rtd_op_resize(const uint8_t* src, int sh, int sw, void* dst, int dh, int dw, int dtype);
/* kernel micro-benchmark (tools/conv_bench.py): one conv layer on zero-filled buffers, timed with HIP events.
 * us_out[0] = mean of `reps` back-to-back launches (operands warm in L2 / Infinity Cache),
 * us_out[1] = mean of `reps` launches each preceded by a `flush_mb` MiB memset (operands come from HBM). */
/* two convs on two streams: shape = {B, HW, Cin, Cout, K, stride, pad}; us_out = {A alone, B alone, A and B together} per repetition */
int rtd_bench_conv_pair(const int* shape_a, const int* shape_b, int reps, float* us_out);
int rtd_bench_conv(int dtype, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int with_res,
                   int reps, int flush_mb, float* us_out);
/* ... with the epilogue's activation as an argument (rtd_bench_conv runs ReLU) */
int rtd_bench_conv_act(int dtype, int B, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int with_res, int act,
                       int reps, int flush_mb, float* us_out);

/* What the matrix pipes of THIS device sustain (tools/mfma_rate_probe.hip inside the library; bench.py reports it beside `roofline`):
 * v_mfma_f32_16x16x32_f16 back to back on every CU, operands in registers, `random_operands` 0 = all-zero bits / 1 = random finite fp16
 * (the chip lowers its clock under matrix load on real data).  out[0] = TFLOP/s by HIP events, out[1] = in-kernel core clock in GHz
 * (s_memtime per s_memrealtime), out[2] = kernel milliseconds.  ~`ms_target` milliseconds of work per timed launch (3 launches). */
int rtd_bench_mfma_rate(int random_operands, int ms_target, float* out);

/* the blurred frame a motion slot holds (rows x cols uint8), copied to the host: what the bit-exactness tests compare with
 * tests/motion_ref.py.  RTD_E_STATE when the slot holds none (reset); implemented in csrc/motion.hip. */
int rtd_debug_motion_state(rtd_motion_handle m, int32_t slot, uint8_t* out, size_t nbytes);

/* the MOG2 model of a motion filter in a canonical layout: weight / variance [npix][5], mean [npix][5][C], modes_used [npix], with
 * hwc[3] and nframes (the updates since the model was initialised).  hwc and nframes are always written (zeros when the filter holds no
 * model); with all four arrays NULL nothing else is.  RTD_E_STATE when arrays are given but there is no model.  And the foreground
 * words of the last rtd_mog2_apply, [ceil(n / 32)][npix] (bit i of chunk c: update 32 c + i marked the pixel 255).  csrc/mog2.hip. */
int rtd_debug_mog2_model(rtd_mog2_handle g, int32_t* hwc, int64_t* nframes, float* weight, float* variance, float* mean,
                         uint8_t* modes_used, size_t npix);
int rtd_debug_mog2_fg_bits(rtd_mog2_handle g, uint32_t* out, size_t nwords);

/* the quantised coefficients of the last rtd_jpeg_encode: int16 [blocks][64] in zig-zag order, the blocks of all frames in scan order
 * (gray: raster order; BGR: per MCU Y00 Y01 Y10 Y11 Cb Cr) - locates a byte mismatch before the entropy coder (tests/jpeg_ref.py
 * coefficients).  *count receives the number of int16 values; out may be NULL to ask for it.  csrc/jpeg.hip. */
int rtd_debug_jpeg_coefficients(rtd_jpeg_handle j, int16_t* out, int64_t capacity, int64_t* count);

/* the tile of the overlay kernel (pixels) and the number of tiles the last rtd_overlay_draw launched (one workgroup each; 0 after a
 * failed call): what tests/overlay_ref.py tiles_touched predicts.  Any pointer may be NULL.  csrc/overlay.hip. */
int rtd_debug_overlay_tiles(rtd_overlay_handle o, int32_t* tile_h, int32_t* tile_w, int64_t* tiles);

/* a piece of the scratch the last rtd_enhance_crops left behind, copied to the host after synchronising with that call's stream:
 * stage 0 = the crop's Lab plane (h x w x 3), 1 = its tile LUTs (tiles_y x tiles_x x 256), 2 = its BGR plane before the bilateral
 * filter (h x w x 3): what tests/enhance_ref.py stages() returns.  nbytes must be the piece's size.  csrc/enhance.hip. */
int rtd_debug_enhance_stage(rtd_enhance_handle e, int32_t crop, int32_t stage, uint8_t* out, size_t nbytes);

/* a float stage output of the LAST TILE of the last rtd_esrgan_upscale, [1, h, w, c] fp32: `ingest` and `last` (32 channels: RGB in
 * 0..2, the padding above), `first`, `body.<i>.rdb<j>` (the 64-channel block output), `body.<i>`, `trunk`, `up1`, `up2`, `hr` (after
 * its LeakyReLU).  The plan reuses its buffers, so the tile is run again up to that stage on the call's stream (the frame must still
 * be alive).  out may be NULL to ask for the shape.  csrc/esrgan.hip. */
int rtd_debug_esrgan_tensor(rtd_esrgan_handle e, const char* name, float* out, int64_t capacity, int64_t shape[4]);

/* what the ingest kernel works with, pure host arithmetic (no GPU, no handle): the five constants CY, CVR, CVG, CUG, CUB of a matrix and
 * range as the one host function computes them, the tile of one workgroup (pixels), and the number of tiles a call on the n frames
 * would launch (the planes are not looked at).  Any pointer may be NULL (frames: n is then ignored).  RTD_E_INVALID for an unknown
 * matrix or range, or a frame rtd_ingest_convert would refuse for its size.  csrc/ingest.hip. */
int rtd_debug_ingest_info(int32_t matrix, int32_t full_range, int32_t coeffs[5], int32_t* tile_h, int32_t* tile_w, int32_t n,
                          const rtd_yuv_frame* frames, int64_t* tiles);

/* the tables of the ingest's resize stage, pure host arithmetic (no GPU, no handle): out receives the dsize entries i0, i1, w0, w1 of
 * the INTER_LINEAR pass from ssize to dsize samples (columns != 0: the column rule, else the row rule) as csrc/resize_taps.h builds
 * them; *is_area2 whether a resize of ssize x ssize2 (width x height) to dsize x dsize2 is the 2 x 2 mean instead; tile_hw the output
 * pixels (rows, columns) of one workgroup of the resize kernel.  out, is_area2 and tile_hw may be NULL.  RTD_E_INVALID for a size
 * outside 1..65535.  csrc/ingest.hip. */
int rtd_debug_resize_table(int32_t ssize, int32_t dsize, int32_t columns, int32_t* out /* [4 * dsize] */, int32_t ssize2, int32_t dsize2,
                           int32_t* is_area2, int32_t tile_hw[2]);

/* what rtd_facemask_apply would do with a call, pure host arithmetic (no GPU, no handle; the frames themselves are not looked at): the
 * number of layers, per face its layer (-1: skipped, its padded rectangle is empty) and its padded rectangle x1, y1, x2, y2 (the blur /
 * pixelate region, exclusive ends), the tile of one workgroup (pixels) and per launch kind the tiles of the whole call (tiles[5]: blur
 * rows, blur columns, pixelate small, pixelate nearest, black box).  With taps_k >= 1 the taps of a k-tap blur go to taps[taps_k]
 * (the shared rule of csrc/gauss_taps.h).  Any output pointer may be NULL.  RTD_E_INVALID for what rtd_facemask_apply would refuse
 * (the message: rtd_facemask_last_error(NULL)).  csrc/facemask.hip. */
int rtd_debug_facemask_plan(int32_t n, const int32_t* hw, int32_t n_faces, const rtd_face_rect* faces, int32_t* layers, int32_t* layer_of,
                            int32_t* rects, int32_t* tile_h, int32_t* tile_w, int64_t* tiles, int32_t taps_k, uint16_t* taps);

/* the classifier's own kernels (csrc/classifier.hip), device pointers, dense tensors, dtype 1 (fp32) or 4 (F16X2 pair storage):
 * patchify:  x [n][3][img][img] fp32 NCHW -> rows [n G G][pad32(3 patch^2)], k = (c patch + i) patch + j as the conv filter flattens, zeros above
 * rope:      in place on q and k of qkv [n L][3 * 64 heads] (q | k | v): out = x * cos + stack(-x[1::2], x[0::2]) * sin per head with the
 *            tables sin, cos [L - 1][64] fp32; token 0 of every image and v stay as they are
 * layernorm: y [rows][c] = LayerNorm over the first c_valid channels (gain, bias [c] fp32; channels from c_valid on are written as zero);
 *            swiglu = 1: the input is [rows][2 c] = g | x and the normalised value is silu(g) * x; norm = 0: no normalisation (gain, bias unused).
 *            c <= 4096, a multiple of 8 (pair storage: of 32)
 * attention: o [n L][64 heads] = softmax(q k^T) v per head from qkv [n L][3 * 64 heads].  Pair storage: eva_attention, NO scale (the handle
 *            folds 1 / 8 into q).  fp32: the library's launch_attention on the [q | k] view, which multiplies the scores by 1 / 8 itself
 *            (the fp32 handle uploads the blob's folded q rows and q bias times 8, which undoes the fold exactly): pass q times 8 for the
 *            same result */
int rtd_op_eva_patchify(int dtype, const float* x, void* rows, int n, int img, int patch);
int rtd_op_eva_rope(int dtype, void* qkv, const float* sin_t, const float* cos_t, int n, int L, int heads);
int rtd_op_eva_layernorm(int dtype, const void* x, void* y, const float* gain, const float* bias, int rows, int c, int c_valid, int swiglu,
                         int norm, float eps);
int rtd_op_eva_attention(int dtype, const void* qkv, void* o, int n, int L, int heads);
/* a float stage output of the last rtd_eva_forward, [n, 1, rows per image, c] fp32: `patch_embed`, `tokens`, `blocks.<k>.attn` (the
 * residual stream after the attention branch), `blocks.<k>`, `pool` (after its LayerNorm), `logits`.  The plan reuses its buffers, so
 * the call is run again up to that stage on its stream (the input must still be alive).  out may be NULL to ask for the shape. */
int rtd_debug_eva_tensor(rtd_eva_handle e, const char* name, float* out, int64_t capacity, int64_t shape[4]);

/* the YOLOX network's own kernels (csrc/yolox_net.hip), device pointers, dtype 1 (fp32) or 4 (F16X2 pair storage):
 * focus:     x [n][3][h][w] fp32 (16-byte aligned, h and w even) -> y [n][h/2][w/2][32]: channel 3 k + c = x[c][2 oy + (k & 1)][2 ox + (k >> 1)]
 *            (quadrants top-left, bottom-left, top-right, bottom-right), channels 12..31 zero
 * focus_u8:  frames: a host array of n (1..64) device pointers to contiguous uint8 HWC BGR frames of frame_hw[i] = (h, w), sides
 *            1..16384, at any byte address -> y [n][in_h/2][in_w/2][32] (16-byte aligned, in_h and in_w even): focus of the frames
 *            resized to in_h x in_w by rtd_yolox_net_run_frames' rule
 * spp:       buf [n][h][w][4 c]: reads channel slice 0 (c channels, a multiple of 8; pair storage: of 32) and writes the stride-1 max
 *            pools 5, 9, 13 (padding never wins) into slices 1, 2, 3
 * head_emit: the three levels' fp32 pred-conv rows - cls [n][h_l w_l][cls_ld], regobj [n][h_l w_l][regobj_ld] (4 box terms, obj) - ->
 *            pred [n][A][5 + num_classes] at any 4-byte address: box terms as they are, sigmoid(obj), sigmoid(cls) */
int rtd_op_yolox_focus(int dtype, const float* x, void* y, int n, int h, int w);
int rtd_op_yolox_focus_u8(int dtype, const uint8_t* const* frames, const int32_t* frame_hw, int n, int in_h, int in_w, void* y);
int rtd_op_yolox_spp(int dtype, void* buf, int n, int h, int w, int c);
int rtd_op_yolox_head_emit(const float* const cls[3], const float* const regobj[3], int cls_ld, int regobj_ld, int n, int in_h, int in_w,
                           int num_classes, float* pred);
/* a float stage output of the last rtd_yolox_net_run or rtd_yolox_net_run_frames, [n, h, w, c] fp32 (read after that call's stream has drained): `focus`, `stem`,
 * `dark2` .. `dark5`, `spp`, `fpn_out0`, `fpn_out1`, `pan_out2`, `pan_out1`, `pan_out0` and per level l = 0..2 `stem_<l>`,
 * `cls_feat_<l>`, `reg_feat_<l>`, `cls_rows_<l>`, `regobj_rows_<l>`.  out may be NULL to ask for the shape. */
int rtd_debug_yolox_tensor(rtd_yolox_net_handle y, const char* name, float* out, int64_t capacity, int64_t shape[4]);

/* the conv launches of a handle's LAST plan (the last successful run / forward / upscale: its last tile), in execution order, as text:
 * one line per launch, `name dtype B H W Cin Cout k stride pad act res_mode out_f32 ldx ldy ldres key S grid` - geometry (H, W: the
 * input's), pixel strides and epilogue as the plan holds them, key / S / grid from the function rtd_debug_conv_choice_views answers from,
 * under the handle's own options.  name: the conv table's (YOLOX, ESRGAN) or the launch's index (EVA).  Host arithmetic only.  out may
 * be NULL to ask for the size (*needed, with the terminating 0).  RTD_E_STATE before the first successful call. */
int rtd_debug_yolox_plan_convs(rtd_yolox_net_handle y, char* out, int64_t capacity, int64_t* needed);
int rtd_debug_eva_plan_convs(rtd_eva_handle e, char* out, int64_t capacity, int64_t* needed);
int rtd_debug_esrgan_plan_convs(rtd_esrgan_handle e, char* out, int64_t capacity, int64_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* RTDETR_MI355_TEST_H */
