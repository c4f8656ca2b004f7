/*
 * rtdetr_mi355.h - C ABI of libmi355rtdetr.so: RT-DETRv2 detection inference on MI355X (gfx950).
 *
 * Drop-in boundary.  The reference has no FFI or plugin registry; its boundary is the duck-typed
 * Python class `RTDETRDetector` constructed by name in the inference engine
 * (/root/reference/src/inference_engine_yolox.py:196-212, class body src/rtdetr_detector.py:26-425).
 * This library is what the replacement class (telescope_cam_detection_amd/rtdetr_detector.py) binds
 * with ctypes; every entry point below cites the reference interface it stands in for.
 * Plain pointers and sizes only - no torch types cross this boundary.
 *
 * Threading: handles are independent; calls on one handle are serialised internally; every entry
 * point selects the handle's device and uses the handle's own HIP stream (the reference runs one
 * detector instance per camera thread, src/inference_engine_yolox.py:320-381).
 */
#ifndef RTDETR_MI355_H
#define RTDETR_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtd_engine* rtd_handle;

/* return codes; RTD_E_OOM is distinct so the Python shim can re-raise torch.cuda.OutOfMemoryError,
 * which is the only exception the reference's degrade path reacts to
 * (src/inference_engine_yolox.py:607-623). */
enum {
  RTD_OK = 0,
  RTD_E_INVALID = 1, /* bad argument / unsupported shape */
  RTD_E_OOM = 2,     /* hipMalloc / arena exhaustion */
  RTD_E_HIP = 3,     /* any other HIP runtime error */
  RTD_E_WEIGHTS = 4, /* blob malformed or tensor missing / wrong shape */
  RTD_E_STATE = 5    /* call order (e.g. infer before load_weights) */
};

/* RTD_PREC_F16X3 (the default engine): every trunk activation and filter is a hi + lo pair of IEEE fp16 (x = hi + lo to 2^-22 relative,
 * 2^-25 absolute below 2^-3, saturating at +-65504) and every contraction runs as three fp16 MFMAs (hi*hi + hi*lo + lo*hi, fp32
 * accumulate): fp32-grade results at the 16-bit MFMA rate / 3.  It meets the reference tolerance (1e-3 on scores, 1e-2 px on boxes
 * against fp32 eager, src/rtdetr_detector.py:256-257) on 640-px AND 1280-px frames (tests/test_gpu_parity.py) at >= 1000 frames/s.
 * RTD_PREC_BF16: plain bf16 storage, one MFMA per product - faster, outside that tolerance (~1 px).  RTD_PREC_FP32: the reference
 * arithmetic on fp32 MFMAs. */
enum { RTD_PREC_BF16 = 0, RTD_PREC_FP32 = 1, RTD_PREC_F16X3 = 2 };
enum { RTD_LAYER_BASIC = 0, RTD_LAYER_BOTTLENECK = 1 };
/* The decoder's cross-attention sampler (upstream's `cross_attn_method`, HF's `decoder_method`).  RTD_DEC_DEFAULT: zero-padded bilinear
 * grid_sample.  RTD_DEC_DISCRETE (upstream's "dsp" checkpoints, e.g. rtdetrv2_r18vd_dsp_3x_coco.yml): per sampling point ONE tap at
 * int(loc * extent + 0.5), truncated toward zero and clamped into the map.  Same weight shapes; a checkpoint served with the other
 * sampler computes other logits (0.65 on the small test model) and no check can see it, so the configuration must say which.
 * RTD_PREC_BF16 is refused with RTD_DEC_DISCRETE: a bf16 offset carries 2^-9 relative, which moves the tap of a large share of points. */
enum { RTD_DEC_DEFAULT = 0, RTD_DEC_DISCRETE = 1 };

/* Constructor arguments of RTDETRDetector (src/rtdetr_detector.py:29-58) that matter to the device
 * side, plus the network description the reference obtains from upstream's YAML config
 * (src/rtdetr_detector.py:132).  Field order is ABI; struct_size guards it. */
enum { RTD_PROFILE_LATENCY = 0, RTD_PROFILE_THROUGHPUT = 1 };

typedef struct rtd_config {
  int32_t struct_size;      /* = sizeof(rtd_config) */
  int32_t device;           /* HIP ordinal  <- `device="cuda:N"` (:33) */
  int32_t precision;        /* RTD_PREC_* : storage/MFMA type of conv + large token GEMMs */
  int32_t max_batch;        /* largest n accepted by rtd_infer* */
  int32_t input_h, input_w; /* <- `input_size` (:35); must be multiples of 32 */
  int32_t use_graph;        /* 1: one hipGraph per batch size, built node by node from the plan (never stream-captured), replayed per call */
  /* architecture (HF:rt_detr/configuration_rt_detr_resnet.py, rt_detr_v2/configuration_rt_detr_v2.py) */
  int32_t layer_type;       /* RTD_LAYER_* */
  int32_t depths[4];
  int32_t hidden_sizes[4];
  int32_t embedding_size;
  int32_t enc_dim, enc_ffn, enc_heads, csp_hidden;
  int32_t d_model, dec_ffn, dec_heads, dec_layers;
  int32_t num_queries, num_classes, n_levels, n_points;
  float offset_scale;
  /* RTD_PROFILE_*: which way the kernel dispatch leans.  LATENCY (0): one batch in flight owns the GPU - tiles sized so that
   * every launch fills the CUs with the shortest critical path.  THROUGHPUT (1): several handles keep batches in flight on one
   * GPU (batching pipeline_depth > 1, bench.py --streams > 1) - other launches fill idle CUs anyway, so the convs take the
   * 256-pixel tile with the least LDS traffic per MFMA (+2.6 % frames/s with 3 handles, -6 % for a lone handle). */
  int32_t profile;
  int32_t dec_method;       /* RTD_DEC_* */
} rtd_config;

/* One detection row: what the per-row loop of src/rtdetr_detector.py:267-303 emits before it
 * becomes a Python dict (class_name / area are derived host-side from these). */
typedef struct rtd_det {
  int32_t class_id;
  float score;
  float x1, y1, x2, y2;
} rtd_det;

const char* rtd_version(void);

/* RTDETRDetector.__init__ (src/rtdetr_detector.py:29-58): allocates nothing on the device yet. */
int rtd_create(const rtd_config* cfg, rtd_handle* out);

/* RTDETRDetector.load_model (src/rtdetr_detector.py:132-173: load_state_dict + .deploy() + .to(device)).
 * `blob` is the flat container written by telescope_cam_detection_amd.weights.pack_blob (already
 * BN-folded / RepVGG-fused fp32 tensors); it is copied, converted to the handle's precision and laid
 * out for the kernels.  Builds the execution plan + activation arena for cfg.input_h x input_w. */
int rtd_load_weights(rtd_handle h, const void* blob, size_t nbytes);

/* RTDETRDetector.detect / detect_batch (src/rtdetr_detector.py:238-403) for n <= max_batch frames.
 * frames[i] : HWC uint8 BGR, hw[2*i] rows x hw[2*i+1] cols (the capture contract,
 *             src/stream_capture.py:228-239); host pointers, or device pointers if frames_on_device.
 * Frames whose size differs from input_h x input_w are stretch-resized exactly as PIL's antialiased
 * bilinear `T.Resize` does (src/rtdetr_detector.py:176-180).
 * out[i*num_queries ...] receives counts[i] rows in descending score order after the confidence
 * threshold (:271) and the wildlife filter {0,14,15,16,21} (:277, src/coco_constants.py:23-29).
 * Blocks until the results are on the host (the reference's three .cpu() syncs, :263-265). */
int rtd_infer(rtd_handle h, int32_t n, const uint8_t* const* frames_bgr_hwc, const int32_t* hw,
              int32_t frames_on_device, float conf_threshold, int32_t wildlife_only,
              rtd_det* out, int32_t* counts);

/* The raw tuple `labels, boxes, scores = self.model(img, orig_size)` (src/rtdetr_detector.py:257):
 * labels[n][Q] (int32), boxes[n][Q][4] xyxy in original-frame pixels, scores[n][Q], descending. */
int rtd_infer_raw(rtd_handle h, int32_t n, const uint8_t* const* frames_bgr_hwc, const int32_t* hw,
                  int32_t frames_on_device, int32_t* labels, float* boxes, float* scores);

/* RTDETRDetector.preprocess (src/rtdetr_detector.py:206-236) as a value: BGR -> RGB, PIL-exact antialiased stretch to input_h x input_w
 * when the frame has another size, / 255 - written as [3][input_h][input_w] fp32 to out_chw_dev (DEVICE memory of the caller, e.g. a torch
 * tensor).  Synchronous.  detect / detect_batch never call it (the network reads the uint8 frames directly); it exists so that a caller
 * of the reference's preprocess() gets the tensor without a forward pass or a host round trip. */
int rtd_preprocess(rtd_handle h, const uint8_t* frame_bgr_hwc, int32_t frame_h, int32_t frame_w, int32_t frame_on_device, float* out_chw_dev);

/* Pipelined form of detect_batch (src/rtdetr_detector.py:307-403 called by the batcher, src/shared_inference_coordinator.py:250),
 * also used by the multi-camera shard and the benchmark: rtd_infer_async enqueues upload + preprocess + network + post-process on the
 * handle's stream and returns; rtd_collect blocks for the LAST submitted batch and returns rtd_infer's rows for it.  A handle has ONE
 * result block: submit, then collect.  A second rtd_infer_async before rtd_collect is legal - batches run in submission order on the
 * handle's stream (the benchmark's back-to-back loop) - but it overwrites the block, so the earlier batch's rows can no longer be
 * collected; with host frames (frames_on_device = 0) it first waits for the previous batch, because the handle's pinned staging
 * buffer holds one batch.  Host frames are copied into that buffer before the call returns (the caller's buffers are free again)
 * and reach HBM by one asynchronous DMA; device frames must stay alive until rtd_collect / rtd_sync.  A failed rtd_infer_async
 * drains the handle's stream before it returns: nothing of the failed batch is still reading the staging buffers.  Everything is plain HIP inside the library: no torch stream, event or
 * allocator takes part.  The result block also stays on the device: [n][Q][6] fp32 rows (label, score, x1, y1, x2, y2) - the
 * fixed-size block each rank contributes to the all-gather - see rtd_result_block. */
int rtd_infer_async(rtd_handle h, int32_t n, const uint8_t* const* frames_bgr_hwc, const int32_t* hw, int32_t frames_on_device);
int rtd_collect(rtd_handle h, float conf_threshold, int32_t wildlife_only, rtd_det* out, int32_t* counts);
int rtd_result_block(rtd_handle h, float** dev_ptr, int64_t* n_floats);
int rtd_sync(rtd_handle h);
void* rtd_stream(rtd_handle h); /* hipStream_t of the handle: for profilers / HIP-event timing only - never wrap it in a torch stream */

/* Build everything a later rtd_infer* of batch size n needs - plan, activation arena, one eager pass on blank frames, the hipGraph -
 * so that the serving path only replays (RTDETRDetector.load_model prepares the sizes its caller declares; part of
 * src/rtdetr_detector.py:132-173's "model ready after load_model").  A size that was not prepared is still built on first use. */
int rtd_prepare(rtd_handle h, int32_t n);

/* Ordering against a stream the CALLER owns (torch's current stream that produced device-resident frames,
 * src/stream_capture_gpu_ffmpeg.py:253,277-278; the stream RCCL's all-gather runs on).  rtd_wait_stream: the handle's stream waits for
 * everything enqueued on `producer_stream` so far.  rtd_signal_stream: `consumer_stream` waits for everything enqueued on the handle's
 * stream so far.  Both use an event that belongs to the handle; streams are hipStream_t values (NULL = the legacy default stream). */
int rtd_wait_stream(rtd_handle h, void* producer_stream);
int rtd_signal_stream(rtd_handle h, void* consumer_stream);

/* What the handle did so far - carried into error reports so that a failure describes itself (batching.BatchCoordinator.get_stats). */
typedef struct rtd_stats {
  int32_t struct_size;           /* = sizeof(rtd_stats) */
  int32_t last_error_code;       /* RTD_E_* of the most recent failed call, 0 = none */
  int32_t stream_capture_status; /* hipStreamIsCapturing of the handle's stream now: 0 none (the only value this library produces) */
  int32_t in_flight;             /* 1: a submitted batch has not been collected */
  int64_t plans, graphs, graph_nodes, graph_launches, eager_passes, submits, collects, failed_calls;
  int64_t saturated_values;      /* F16X2 activations found AT the format's saturation value (+-65504) by the last rtd_self_check, -1 = never run */
  float max_abs_filter;          /* largest |folded filter value| of the loaded blob (> 65504 is refused by rtd_load_weights on the pair engine) */
  int32_t reserved;
} rtd_stats;
int rtd_get_stats(rtd_handle h, rtd_stats* out);

/* Real-weights guard (part of "the model is ready after load_model", src/rtdetr_detector.py:132-173).  Every parity claim of this library
 * was measured on seeded synthetic weights; the pair engine's fp16 halves SATURATE at +-65504 - silently, finitely.  Two things keep a
 * trained checkpoint honest:
 *  (1) rtd_load_weights returns RTD_E_WEIGHTS for a tensor that holds NaN / Inf and - RTD_PREC_F16X3 - for a folded filter value
 *      beyond 65504 (rtd_last_error names the tensor);
 *  (2) rtd_self_check runs ONE built-in frame of the handle's input size through the library's exact fp32 engine and through an engine of
 *      the handle's precision, both built from the blob the handle was loaded with, counts the activations that sit at the saturation value and
 *      matches the detection rows (same label, |dscore| <= score_tol = 1e-3, max |dbox| <= box_tol_px = 1e-2, the reference tolerance).
 *      The caller decides: RTDETRDetector.load_model(verify=True) logs the report and refuses a checkpoint whose rows do not match.
 *      Costs two temporary bs-1 engines (a second or two at load time); the handle itself is not touched. */
typedef struct rtd_check_report {
  int32_t struct_size;             /* in: = sizeof(rtd_check_report) */
  int32_t rows, rows_matched;      /* rows of the fp32 engine's answer / of them matched by the handle's precision within the tolerance */
  float worst_score_err, worst_box_err_px;   /* over the matched rows */
  float score_tol, box_tol_px;
  float max_abs_filter;
  int64_t saturated_values;        /* F16X2 activations at +-65504 after that forward (0 for the other precisions) */
  char max_abs_filter_name[64];
} rtd_check_report;
int rtd_self_check(rtd_handle h, const void* blob, size_t nbytes, rtd_check_report* out);   /* blob: the one given to rtd_load_weights (the handle keeps no host copy) */

/* mutable attribute `model.to(device)` / teardown (src/inference_engine_yolox.py:743-744) */
void rtd_destroy(rtd_handle h);
const char* rtd_last_error(rtd_handle h); /* h may be NULL: last error of a failed rtd_create */

/* device memory held by the handle's activation arenas (all prepared batch sizes), bytes */
int64_t rtd_arena_bytes(rtd_handle h);

/* ---- Stage 2: crop + classifier pre-processing for a whole batch of detections ------------------
 * For crop i: frame slice [y1:y2, x1:x2] (src/two_stage_pipeline_yolox.py:289) of a device-resident HWC uint8 BGR frame,
 * then SpeciesClassifier.preprocess (src/species_classifier.py:298-352): BGR->RGB, F.interpolate(bilinear,
 * align_corners=False) to out_size x out_size, /255, (x-mean)/std.  out_dev: [n][3][out_size][out_size] fp32 (what the
 * classifier network consumes).  rects = [n][4] (x1, y1, x2, y2), frame_hw = [n][2].  ASYNCHRONOUS: the launch is
 * enqueued on `stream` (a hipStream_t the caller owns, e.g. torch's current stream; NULL = the legacy default stream) and the call
 * returns at once - the batch is ready when that stream reaches it, so a consumer on the same stream (the classifier forward) needs no
 * synchronisation and the next detect batch overlaps with it.  Frames and out_dev must stay alive until then; the rectangles, sizes and
 * normalisation constants are copied into the launch before the call returns. */
int rtd_crop_resize_batch(int32_t n, const uint8_t* const* frames_dev, const int32_t* frame_hw, const int32_t* rects,
                          int32_t out_size, const float* mean3, const float* std3, float* out_dev, void* stream);

/* ---- Empty-frame filter: a motion gate ahead of detection (the reference's src/empty_frame_filter.py, config key
 * performance.empty_frame_filter) --------------------------------------------------------------------------------------------------
 * Per frame, exactly as EmptyFrameFilter.has_motion computes it with OpenCV on 8-bit frames (restated in tests/motion_ref.py):
 * BGR2GRAY, GaussianBlur(k x k, sigma 0) on OpenCV's bit-exact fixed-point path with BORDER_REFLECT_101,
 * area = #{ |blurred - stored| > threshold }, and the blurred frame replaces the camera's stored one.  One fused launch covers a whole
 * batch of frames from different cameras (csrc/motion.hip).  Independent of a detection engine: it has its own handle, which owns a
 * non-blocking stream, a pinned staging buffer for host frames (grown on demand, one upload per call) and one state buffer per slot
 * (allocated on the slot's first frame, reallocated on a size change; nothing is allocated on the steady path). */
typedef struct rtd_motion* rtd_motion_handle;
int rtd_motion_create(int32_t device, int32_t blur_size /* odd, 1..63 */, rtd_motion_handle* out);
/* n frames (HWC uint8, C = 1 or 3, host or device pointers), slots[i] = the camera's state slot (>= 0);
 * area[i] receives the count above, or -1 for a first frame (new slot, reset, size change).  threshold is the integer one (the caller
 * floors a fractional threshold; < 0 counts every pixel, >= 255 none).
 * Synchronous: returns when area[] is on the host.  Two frames with the same slot in one call are applied in order. */
int rtd_motion_check(rtd_motion_handle m, int32_t n, const uint8_t* const* frames, const int32_t* hwc /* [n][3] */,
                     int32_t frames_on_device, const int32_t* slots, int32_t threshold, int64_t* area);
int rtd_motion_reset(rtd_motion_handle m, int32_t slot /* -1 = all */);   /* the slot's next frame is a first frame */
int rtd_motion_wait_stream(rtd_motion_handle m, void* producer_stream);   /* as rtd_wait_stream */
const char* rtd_motion_last_error(rtd_motion_handle m);                  /* m may be NULL: last error of a failed rtd_motion_create */
void rtd_motion_destroy(rtd_motion_handle m);

/* ---- Motion filter: MOG2 background model and per-box motion after detection (the reference's src/motion_filter.py MotionFilter,
 * config key motion_filter) ------------------------------------------------------------------------------------------------------------
 * cv2.createBackgroundSubtractorMOG2(history, var_threshold, detect_shadows) with OpenCV's defaults otherwise (5 modes, background ratio
 * 0.9, generation threshold 9, variance 15 in [4, 75], complexity reduction 0.05, shadow tau 0.5), applied to 8-bit frames as OpenCV's
 * CPU path computes it (restated in tests/mog2_ref.py).  Per update i of a call: the model is updated with the frame and its
 * foreground mask (shadows dropped: mask == 255) is blurred with GaussianBlur(blur_size, sigma 0) on the bit-exact 8-bit path
 * (BORDER_REFLECT_101 at the frame edges); counts[i] = #{ blurred > 25 } inside box i.  One fused launch per chunk of 32 updates and
 * one launch for every box of the call (csrc/mog2.hip).  Own handle with a non-blocking stream and a pinned staging buffer for host
 * frames; the model (25 floats + 1 byte per pixel for BGR) is allocated on the first frame and reallocated on a size or channel change,
 * which re-initialises it as OpenCV does.  Nothing is allocated on the steady path. */
typedef struct rtd_mog2* rtd_mog2_handle;
int rtd_mog2_create(int32_t device, int32_t history /* >= 1 */, double var_threshold, int32_t detect_shadows, rtd_mog2_handle* out);
/* = a new subtractor with these parameters: the model is forgotten (the next update initialises it) */
int rtd_mog2_configure(rtd_mog2_handle g, int32_t history, double var_threshold, int32_t detect_shadows);
/* n updates of the model with one frame (HWC uint8, C = 1 or 3, host or device pointer), in order; rects = [n][4] boxes x1, y1, x2, y2
 * already clamped to the frame (an empty box is allowed: its update happens, its count is 0); blur_size odd, 1..63.
 * counts[i] receives the count of update i.  Synchronous: returns when counts[] is on the host.  n = 0: nothing happens. */
int rtd_mog2_apply(rtd_mog2_handle g, const uint8_t* frame, const int32_t* hwc /* [3] */, int32_t frame_on_device, int32_t n,
                   const int32_t* rects, int32_t blur_size, int64_t* counts);
int rtd_mog2_wait_stream(rtd_mog2_handle g, void* producer_stream);   /* as rtd_wait_stream */
const char* rtd_mog2_last_error(rtd_mog2_handle g);                  /* g may be NULL: last error of a failed rtd_mog2_create */
void rtd_mog2_destroy(rtd_mog2_handle g);

/* ---- JPEG encoder for device-resident frames (the reference's cv2.imencode('.jpg', ...) in src/snapshot_saver.py add_frame_to_buffer
 * and the MJPEG loop of src/web_server.py) -----------------------------------------------------------------------------------------------
 * Baseline sequential JPEG (SOF0, one scan, 8-bit; BGR frames as YCbCr 4:2:0, one-channel frames as gray), standard Huffman tables,
 * IJG quality scaling, JFIF APP0: byte for byte the file libjpeg writes at its defaults for a quality alone, which is what cv2.imencode
 * with IMWRITE_JPEG_QUALITY and Pillow's save(..., "JPEG", quality=q) produce (restated in tests/jpeg_ref.py).  The transform, the
 * Huffman coding and the byte stuffing run on the device (csrc/jpeg.hip); the host writes the markers.  Own handle with a non-blocking
 * stream, a pinned staging buffer and device buffers grown on demand: no device or pinned allocation on the steady path (a call makes
 * a few small host vectors; the marker block of a frame shape and quality is built once per handle).  Calls on one handle are
 * serialised by the handle.  Frames are at most 65535 pixels per side and 16 Mpixel each. */
typedef struct rtd_jpeg* rtd_jpeg_handle;
int rtd_jpeg_create(int32_t device, rtd_jpeg_handle* out);
/* n frames (HWC uint8, C = 1 or 3 = BGR; host or device pointers) -> n complete JPEG files, back to back in out (HOST memory,
 * capacity out_cap bytes); offsets[n+1] receives where each file starts and the total.  RTD_E_INVALID with the needed size in
 * offsets[n] when out_cap is too small (the call may be repeated; out may then be NULL).  The size is known only after the frames
 * have been coded, so such a call costs a whole encode except the copy of the bytes: size out for the largest batch once (a 1080p
 * frame at quality 90 takes about 0.5 MB) rather than asking every time.  quality 1..100.  Synchronous. */
int rtd_jpeg_encode(rtd_jpeg_handle j, int32_t n, const uint8_t* const* frames, const int32_t* hwc /* [n][3] */,
                    int32_t frames_on_device, int32_t quality, uint8_t* out, int64_t out_cap, int64_t* offsets);
int rtd_jpeg_wait_stream(rtd_jpeg_handle j, void* producer_stream);   /* as rtd_wait_stream */
const char* rtd_jpeg_last_error(rtd_jpeg_handle j);                  /* j may be NULL: last error of a failed rtd_jpeg_create */
void rtd_jpeg_destroy(rtd_jpeg_handle j);

/* ---- Detection overlays on device-resident frames (the reference's cv2.rectangle / cv2.putText in src/web_server.py _draw_detections
 * and src/visualization_utils.py draw_detections) ------------------------------------------------------------------------------------------
 * Filled rectangles, outlines and coverage masks (rasterised text) composited onto a batch of HWC uint8 frames in one launch
 * (csrc/overlay.hip), all in integers (restated in tests/overlay_ref.py).  The primitives of a frame apply in list order, clipped to the
 * frame:
 *   FILL     every pixel of the inclusive rectangle (cv2.rectangle with thickness -1)
 *   OUTLINE  with o = t / 2 and i = (t - 1) / 2: the pixels of [x1-o, x2+o] x [y1-o, y2+o] that are not strictly inside
 *            (x1+i, x2-i) x (y1+i, y2-i): a strip exactly t pixels wide with square corners (t = 1 is cv2's outline; for t >= 2 cv2 rounds
 *            the corners)
 *   MASK     coverage a per pixel: out = (bg * (255 - a) + colour * a + 127) / 255 per channel, integer division
 * One-channel frames take bgr[0].  Own handle with a non-blocking stream and a pinned staging buffer grown on demand: no device or pinned
 * allocation on the steady path.  Calls on one handle are serialised by the handle.
 * Limits: RTD_OVERLAY_MAX_FRAMES frames per call, RTD_OVERLAY_MAX_PRIMS primitives per frame, frames of 1..65535 pixels per side and
 * less than 2 GiB, OUTLINE thickness 1..65535, masks of 0..65535 pixels per side.  Beyond a limit: RTD_E_INVALID, and nothing is copied
 * or drawn. */
enum { RTD_OVL_FILL = 0, RTD_OVL_OUTLINE = 1, RTD_OVL_MASK = 2 };
enum { RTD_OVERLAY_MAX_FRAMES = 64, RTD_OVERLAY_MAX_PRIMS = 4096 };
typedef struct rtd_overlay_prim { /* 40 bytes */
  int32_t kind;
  int32_t x1, y1, x2, y2; /* FILL / OUTLINE: opposite corners, both INCLUSIVE, in any order, may lie outside the frame.
                             MASK: x1, y1 = where the mask's top-left pixel lands; x2, y2 = the mask's width and height */
  int32_t thickness;      /* OUTLINE: >= 1 */
  uint8_t bgr[3], reserved0;
  int64_t mask_offset;    /* MASK: byte offset into `masks`; rows tightly packed */
} rtd_overlay_prim;
typedef struct rtd_overlay* rtd_overlay_handle;
int rtd_overlay_create(int32_t device, rtd_overlay_handle* out);
/* n frames (HWC uint8, C = 1 or 3 = BGR; host or device pointers), prim_counts[i] primitives for frame i, back to back in prims;
 * masks = HOST memory of mask_bytes bytes (copied into the call).  out_dev[i] is device memory of the caller with room for the frame; it
 * may equal frames[i] for a device frame (drawn in place); otherwise the frame is first copied there (one device-to-device copy, or one
 * DMA from the staging buffer for a host frame).  Two frames of a call must not share out_dev memory.  Synchronous: returns when every
 * out_dev[i] holds its annotated frame. */
int rtd_overlay_draw(rtd_overlay_handle o, int32_t n, const uint8_t* const* frames, const int32_t* hwc /* [n][3] */,
                     int32_t frames_on_device, const int32_t* prim_counts /* [n] */, const rtd_overlay_prim* prims,
                     const uint8_t* masks, int64_t mask_bytes, uint8_t* const* out_dev /* [n] */);
int rtd_overlay_wait_stream(rtd_overlay_handle o, void* producer_stream);   /* as rtd_wait_stream */
const char* rtd_overlay_last_error(rtd_overlay_handle o);                  /* o may be NULL: last error of a failed rtd_overlay_create */
void rtd_overlay_destroy(rtd_overlay_handle o);

/* ---- Stage-2 crop enhancement on device-resident frames (the reference's ImageEnhancer.enhance_clahe_bilateral in
 * src/image_enhancement.py, enhancement method "clahe") -----------------------------------------------------------------------------------
 * Per crop (3-channel BGR): cv2.cvtColor(BGR2LAB) on OpenCV's 8-bit integer path, CLAHE(clip_limit, tiles_x x tiles_y) on L,
 * Lab -> BGR by this library's own integer tables, cv2.bilateralFilter(bilateral_d, sigma_color, sigma_space) with BORDER_REFLECT_101 of
 * the CROP (not of the frame around it).  The arithmetic is restated in tests/enhance_ref.py and matched bit for bit: tables from double
 * precision on the host, integers per pixel, fp32 in a fixed order for the CLAHE interpolation and the bilateral sums.  Three launches
 * per call, each over all crops (csrc/enhance.hip).
 * The handle owns the tables (built and uploaded at create) and the scratch (a Lab plane, the tile LUTs, a second BGR plane), which is
 * grown on demand: nothing is allocated on the steady path.  It owns NO stream: rtd_enhance_crops is ASYNCHRONOUS on the caller's
 * `stream`, exactly as rtd_crop_resize_batch, so a consumer on the same stream needs no synchronisation; frames and out_dev must stay
 * alive until the stream has passed the call (the rectangles and sizes are copied into the launches before it returns).  The scratch
 * belongs to the call in flight: calls on one handle must be enqueued on ONE stream, or be ordered by the caller.
 * Limits: tiles 1..16 per axis, bilateral radius (d / 2; for d <= 0 rint(1.5 sigma_space)) 1..7, 1..64 crops per call, every crop at
 * least 16 pixels per side and inside its frame.  Anything else: RTD_E_INVALID, nothing is launched and out_dev is left untouched.
 * clip_limit <= 0 disables clipping; sigmas <= 0 become 1. */
typedef struct rtd_enhance_params {
  int32_t struct_size; /* = sizeof(rtd_enhance_params) */
  float clip_limit;
  int32_t tiles_x, tiles_y;
  int32_t bilateral_d;
  float sigma_color, sigma_space;
} rtd_enhance_params;
typedef struct rtd_enhance* rtd_enhance_handle;
int rtd_enhance_create(int32_t device, const rtd_enhance_params* params, rtd_enhance_handle* out);
/* Where the crops of a call lie in its output: THE packing rule, pure host arithmetic (no GPU, no handle).  rects = [n][4] x1, y1, x2, y2;
 * offsets[n + 1]: crop i is h x w x 3 (HWC, rows tightly packed) at byte offsets[i], which is a multiple of 256; offsets[n] is the size
 * the output needs.  n >= 0 (no upper limit here: offsets[k] of a long list is where a call on rects k.. of it writes, relative to
 * offsets[k]).  RTD_E_INVALID for a rect with a negative corner or fewer than 16 pixels per side. */
int rtd_enhance_layout(int32_t n, const int32_t* rects, int64_t* offsets /* [n + 1] */);
/* crop i = frames_dev[i][y1:y2, x1:x2] of an HWC uint8 BGR frame of frame_hw[i] = (h, w); the enhanced crops go to out_dev (device
 * memory of out_cap >= offsets[n] bytes) where rtd_enhance_layout says. */
int rtd_enhance_crops(rtd_enhance_handle e, int32_t n, const uint8_t* const* frames_dev, const int32_t* frame_hw /* [n][2] */,
                      const int32_t* rects /* [n][4] */, uint8_t* out_dev, int64_t out_cap, void* stream);
const char* rtd_enhance_last_error(rtd_enhance_handle e);                  /* e may be NULL: last error of a failed create / layout */
void rtd_enhance_destroy(rtd_enhance_handle e);

/* ---- Real-ESRGAN x4 upscaling of Stage-2 crops on device-resident frames (the reference's ImageEnhancer method "realesrgan",
 * src/image_enhancement.py: RealESRGANer.enhance(outscale 4) around RRDBNet(3, 3, 64, num_block, 32, scale 4)) -------------------------
 * Per crop (3-channel BGR): float32(v) / 255, BGR -> RGB, the network on the whole crop (tile = 0) or tile by tile (the core of a tile
 * extended by tile_pad and clamped to the crop goes through the network, the core's x4 image is cut out), clamp(0, 1), RGB -> BGR,
 * round half to even of x * 255.  The arithmetic is restated in tests/esrgan_ref.py; the network's 15 num_block + 6 convolutions run on
 * the library's conv kernels in the handle's precision: RTD_PREC_F16X3 (fp16 hi + lo pairs) or RTD_PREC_FP32.  RTD_PREC_BF16 is refused
 * (it changes a third of the output bytes).  csrc/esrgan.hip.
 * blob = the container rtd_load_weights reads, holding the state dict's tensors under their own names (`conv_first.weight` [64][3][3][3],
 * `body.<i>.rdb<j>.conv<k>.weight`, ... `.bias`; OIHW fp32).  A missing or mis-shaped tensor, a NaN / Inf and - pair engine - a value
 * beyond 65504 return RTD_E_WEIGHTS with the tensor's name.
 * The handle owns the filters and one arena (the activations of the largest tile shape seen, and the conv kernels' split-K workspace);
 * a repeated shape allocates nothing.  It owns NO stream: rtd_esrgan_upscale is ASYNCHRONOUS on the caller's `stream`, exactly as
 * rtd_enhance_crops; crops are processed one after another, tile by tile; calls on one handle go on ONE stream.
 * Limits: 1..64 crops per call, every crop 8..4096 pixels per side and inside its frame; with tile = 0 a crop side is at most 576.
 * Anything else: RTD_E_INVALID before anything is launched, out_dev untouched.  Arena exhaustion: RTD_E_OOM. */
typedef struct rtd_esrgan_config {
  int32_t struct_size; /* = sizeof(rtd_esrgan_config) */
  int32_t device;
  int32_t precision;   /* RTD_PREC_F16X3 | RTD_PREC_FP32 */
  int32_t num_feat;    /* 64 */
  int32_t num_grow_ch; /* 32 */
  int32_t num_block;   /* 1..32 */
  int32_t tile;        /* 0 (one pass) or 16..512 */
  int32_t tile_pad;    /* 0..32 */
} rtd_esrgan_config;
typedef struct rtd_esrgan* rtd_esrgan_handle;
int rtd_esrgan_create(const rtd_esrgan_config* cfg, const void* blob, size_t nbytes, rtd_esrgan_handle* out);
/* pure host arithmetic: rects = [n][4] x1, y1, x2, y2; crop i is 4h x 4w x 3 (HWC, rows tightly packed) at byte offsets[i], a multiple
 * of 256; offsets[n] is the size the output needs.  RTD_E_INVALID for a negative corner or a side outside 8..4096. */
int rtd_esrgan_layout(int32_t n, const int32_t* rects, int64_t* offsets /* [n + 1] */);
int rtd_esrgan_upscale(rtd_esrgan_handle e, int32_t n, const uint8_t* const* frames_dev, const int32_t* frame_hw /* [n][2] */,
                       const int32_t* rects /* [n][4] */, uint8_t* out_dev, int64_t out_cap, void* stream);
int64_t rtd_esrgan_arena_bytes(rtd_esrgan_handle e);
const char* rtd_esrgan_last_error(rtd_esrgan_handle e);                    /* e may be NULL: last error of a failed create / layout */
void rtd_esrgan_destroy(rtd_esrgan_handle e);

/* ---- Frame ingest: 4:2:0 camera frames (NV12, NV21, I420) -> the BGR device frames every other entry point takes (in place of the
 * swscale conversion behind the reference's cv2.VideoCapture and behind `-pix_fmt bgr24` in src/stream_capture_gpu_ffmpeg.py) ----------
 * All frames of a call in one launch (csrc/ingest.hip).  The arithmetic is OpenCV's COLOR_YUV2BGR_NV12 / _NV21 / _I420 fixed-point
 * path, integers only (restated in tests/yuv_ref.py and matched bit for bit): the chroma plane has ceil(H/2) rows of ceil(W/2) samples,
 * pixel (y, x) takes sample (y >> 1, x >> 1) without interpolation, and with u = U - 128, v = V - 128, y' = max(Y - 16, 0) (limited
 * range) or Y (full range), in int32:
 *   B = clip8((y' CY + 2^19 + CUB u) >> 20),  G = clip8((y' CY + 2^19 + CVG v + CUG u) >> 20),  R = clip8((y' CY + 2^19 + CVR v) >> 20)
 * with the five constants floor(c 2^20 + 0.5) of the matrix's decimal coefficients (BT.601 limited: OpenCV's own 1220542, 1673527,
 * -852492, -409993, 2116026).  Odd widths and heights are accepted by the rule above (OpenCV refuses them; ffmpeg writes them so).
 * A plane is a pointer and a pitch in bytes, so a padded decoder surface is read where it lies; tightly packed rawvideo is
 * y_pitch = width, c_pitch = 2 ceil(W/2) (NV12 / NV21) or ceil(W/2) (I420), the planes back to back.  Frames of one call may differ in
 * size, layout, matrix and range.  Own handle with a non-blocking stream and a pinned staging buffer with its device twin, grown on
 * demand: no device or pinned allocation on the steady path.  Calls on one handle are serialised by the handle.
 * Limits: 1..RTD_INGEST_MAX_FRAMES frames per call, 1..65535 pixels per side, pitches of at least the row's bytes, known layout / matrix /
 * range values, no null plane or output.  Beyond a limit: RTD_E_INVALID with the frame's index in the message, and nothing is copied or
 * launched. */
enum { RTD_YUV_NV12 = 0, RTD_YUV_NV21 = 1, RTD_YUV_I420 = 2 };
enum { RTD_YUV_BT601 = 0, RTD_YUV_BT709 = 1 };
enum { RTD_INGEST_MAX_FRAMES = 64 };
typedef struct rtd_yuv_frame { /* 56 bytes */
  const uint8_t* y; /* luma: height rows of width bytes, y_pitch apart */
  const uint8_t* u; /* NV12: the interleaved U V plane; NV21: the interleaved V U plane; I420: the U plane.  ceil(H/2) rows, c_pitch apart */
  const uint8_t* v; /* I420: the V plane (c_pitch apart as well); unused for NV12 / NV21 */
  int32_t width, height;
  int32_t y_pitch, c_pitch;
  int32_t layout;     /* RTD_YUV_NV12 | _NV21 | _I420 */
  int32_t matrix;     /* RTD_YUV_BT601 | _BT709 */
  int32_t full_range; /* 0: limited (16..235 luma), 1: full */
  int32_t reserved0;
} rtd_yuv_frame;
typedef struct rtd_ingest* rtd_ingest_handle;
int rtd_ingest_create(int32_t device, rtd_ingest_handle* out);
/* n frames whose planes are all host memory (frames_on_device = 0: packed into the staging buffer and uploaded in ONE copy) or all
 * device memory; out_dev[i] is device memory of the caller with room for height x width x 3 bytes and receives the frame as tight HWC
 * BGR.  Two frames of a call must not share out_dev memory.  Synchronous: returns when every out_dev[i] is complete. */
int rtd_ingest_convert(rtd_ingest_handle g, int32_t n, const rtd_yuv_frame* frames, int32_t frames_on_device, uint8_t* const* out_dev /* [n] */);
/* The resize stage: camera frames at their native sizes in, BGR device frames of the requested sizes out, byte for byte OpenCV's
 * resize(frame, (w, h)) with INTER_LINEAR on 8-bit data (restated in tests/face_ref.py resize_linear, composed with the conversion in
 * tests/resize_ref.py): the 2 x 2 mean (a + b + c + d + 2) >> 2 where both scale factors are exactly 2, otherwise cv2's index and
 * weight tables (weights in 1/2048, built on the host by csrc/resize_taps.h) and
 *   out = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2,  H = p[i0] w0 + p[i1] w1.
 * A 4:2:0 frame is converted per source pixel first (the conversion clamps) and blended after.  Both calls are synchronous, use the
 * handle's stream and staging buffer (descriptors, tiles, tables and host frames go up in ONE copy) and check every limit before
 * anything is copied or launched: 1..RTD_INGEST_MAX_FRAMES frames, 1..65535 pixels per side for source and output, pitches of at
 * least a row, no null source or output, at most 2^24 tiles of 128 x 8 output pixels per call, and no two outputs of a call
 * (native ones included) sharing a byte.  Beyond a limit: RTD_E_INVALID with the frame's index in the message. */
typedef struct rtd_bgr_frame { /* 24 bytes */
  const uint8_t* data; /* height rows of width BGR pixels, pitch bytes apart */
  int32_t width, height, pitch, reserved0;
} rtd_bgr_frame;
/* as rtd_ingest_convert, but out_dev[i] (out_hw[2i] x out_hw[2i+1] x 3 bytes) receives the frame resized to out_hw[2i] rows of
 * out_hw[2i+1] pixels; native_out_dev may be NULL, and so may any of its entries: a non-null entry (height x width x 3 bytes) receives
 * the frame at its own size as rtd_ingest_convert would write it */
int rtd_ingest_convert_resize(rtd_ingest_handle g, int32_t n, const rtd_yuv_frame* frames, int32_t frames_on_device,
                              const int32_t* out_hw /* [n][2] */, uint8_t* const* out_dev /* [n] */, uint8_t* const* native_out_dev /* [n] or NULL */);
/* n BGR frames, all host memory (packed row by row into the staging buffer) or all device memory (read where they lie) */
int rtd_ingest_resize(rtd_ingest_handle g, int32_t n, const rtd_bgr_frame* frames, int32_t frames_on_device,
                      const int32_t* out_hw /* [n][2] */, uint8_t* const* out_dev /* [n] */);
int rtd_ingest_wait_stream(rtd_ingest_handle g, void* producer_stream);   /* as rtd_wait_stream */
const char* rtd_ingest_last_error(rtd_ingest_handle g);                  /* g may be NULL: last error of a failed rtd_ingest_create */
void rtd_ingest_destroy(rtd_ingest_handle g);

/* ---- Privacy face masks on device-resident frames (the reference's FaceMasker.apply_mask in src/face_masker.py: cv2.GaussianBlur,
 * cv2.resize and cv2.rectangle on the padded face rectangle) ---------------------------------------------------------------------------
 * Faces are masked where the frame lies (csrc/facemask.hip), all in integers, byte for byte what the reference does to the numpy frame
 * (restated in tests/face_ref.py).  With p = int(w * 0.2) the padded rectangle of a face (x, y, w, h) on an H x W frame is
 * x1 = max(0, x - p), y1 = max(0, y - p), x2 = min(W, x + w + p), y2 = min(H, y + h + p), and the region is frame[y1:y2, x1:x2]:
 *   BLUR       GaussianBlur(region, (k, k), 0) on OpenCV's fixed-point path: taps in 1/256 (getGaussianKernelBitExact), a row pass to
 *              16-bit sums, a column pass (sum + 32768) >> 16, BORDER_REFLECT_101 at the REGION's edges, each channel on its own.  The
 *              reference's adaptive_blur is BLUR with the k its caller works out per face.
 *   PIXELATE   small = resize(region, (max(1, rw / blocks), max(1, rh / blocks)), INTER_LINEAR), then resize(small, (rw, rh),
 *              INTER_NEAREST): OpenCV's portable 8-bit code, the index and weight tables made on the host.
 *   BLACK_BOX  zero over x1..min(x2, W - 1), y1..min(y2, H - 1) INCLUSIVE (cv2.rectangle fills both corners).
 * Faces apply in list order: where the rectangles of two faces of a frame overlap, the later one works on the earlier one's output.
 * The host sorts the faces of a call into layers (a face goes after every earlier face of its frame that it meets); a layer is one
 * launch pair per style present, over all its faces.  A face whose padded rectangle is empty is skipped (cv2 would raise).
 * Own handle with a non-blocking stream, a pinned staging buffer with its device twin and a scratch plane, all grown on demand: no
 * device or pinned allocation on the steady path.  Calls on one handle are serialised by the handle.
 * Limits: 1..RTD_FACEMASK_MAX_FRAMES frames per call, 1..65535 pixels per side and less than 2 GiB, at most RTD_FACEMASK_MAX_FACES faces, a frame index
 * inside the call, a known style, k odd in 1..99, blocks >= 1, no null pointer.  Beyond a limit: RTD_E_INVALID with the face's (or
 * frame's) index in the message, and nothing is copied or launched. */
enum { RTD_FACE_BLUR = 0, RTD_FACE_PIXELATE = 1, RTD_FACE_BLACK_BOX = 2 };
enum { RTD_FACEMASK_MAX_FRAMES = 64, RTD_FACEMASK_MAX_FACES = 1024, RTD_FACEMASK_MAX_K = 99 };
typedef struct rtd_face_rect { /* 32 bytes */
  int32_t frame;       /* which frame of the call */
  int32_t x, y, w, h;  /* the detector's box; may leave the frame */
  int32_t style;       /* RTD_FACE_* */
  int32_t k_or_blocks; /* BLUR: the kernel size k; PIXELATE: blocks; BLACK_BOX: ignored */
  int32_t reserved0;
} rtd_face_rect;
typedef struct rtd_facemask* rtd_facemask_handle;
int rtd_facemask_create(int32_t device, rtd_facemask_handle* out);
/* n frames (HWC uint8 BGR, tightly packed, hw = [n][2] rows, cols), all device memory (masked in place) or all host memory
 * (frames_on_device = 0: the frames that have a face are uploaded, masked and written back over the host frame).  Synchronous: returns
 * when every frame holds its masked pixels.  Bytes outside the padded rectangles are never written. */
int rtd_facemask_apply(rtd_facemask_handle m, int32_t n, uint8_t* const* frames, const int32_t* hw /* [n][2] */, int32_t frames_on_device,
                       int32_t n_faces, const rtd_face_rect* faces);
/* the gray plane a face detector takes, (1868 B + 9617 G + 4899 R + 8192) >> 14 (cv2.cvtColor BGR2GRAY) of one DEVICE frame, written by
 * the kernel into pinned host memory and copied to gray_out (HOST, rows x cols bytes): a third of the frame's bytes cross.  Synchronous. */
int rtd_facemask_gray(rtd_facemask_handle m, const uint8_t* frame_dev, int32_t rows, int32_t cols, uint8_t* gray_out);
int rtd_facemask_wait_stream(rtd_facemask_handle m, void* producer_stream);   /* as rtd_wait_stream */
const char* rtd_facemask_last_error(rtd_facemask_handle m);                  /* m may be NULL: last error of a failed rtd_facemask_create */
void rtd_facemask_destroy(rtd_facemask_handle m);

/* ---- Stage-2 species classifier: timm's `Eva` vision transformer (the reference's config names
 * timm/eva02_large_patch14_clip_336.merged2b_ft_inat21: ViT-L/14 at 336 px, 24 blocks, 1024 channels, 16 heads of 64, 577 tokens) ------
 * Patch embed (patch x patch conv, stride patch, bias), cls token, learned pos_embed; per block
 *   x += proj(attn_norm?(attention(rope(q), rope(k), v)));  x += fc2(mlp_norm?(silu(fc1_g y) * fc1_x y)), y = norm2(x)
 * with interleaved RoPE on the patch tokens of q and k (never the cls token), LayerNorm eps 1e-6, then norm -> cls row (RTD_EVA_POOL_TOKEN)
 * or mean of the patch tokens -> fc_norm (RTD_EVA_POOL_AVG), then the head.  Restated in tests/eva_ref.py.  csrc/classifier.hip.
 * blob = the container rtd_load_weights reads, holding what eva_checkpoint.fold_state writes (csrc/classifier_host.h lists names and
 * shapes): filters as [out][in] fp32 rows, 1 / 8 folded into the q rows, qkv as one [3 dim][dim] filter with a zero k bias, fc1_g | fc1_x
 * as one filter, hidden / 3 patch^2 / classes zero-padded to whole 32-channel groups, and the RoPE sin / cos tables [L - 1][64] as data
 * (the kernels hold no frequency rule).  A missing or mis-shaped tensor, a NaN / Inf and - pair engine - a value beyond 65504 return
 * RTD_E_WEIGHTS with the tensor's name, before the device is touched.
 * The GEMMs run on the library's conv kernels in the handle's precision, RTD_PREC_F16X3 (fp16 hi + lo pairs, attention on pair MFMAs
 * too) or RTD_PREC_FP32.  The handle owns the filters and one arena (one plan per batch size; a repeated batch size allocates nothing)
 * and NO stream: rtd_eva_forward is ASYNCHRONOUS on the caller's `stream`; calls on one handle go on ONE stream.
 * Limits: head dim 64, dim and hidden at most 4096, 1..max_batch images per call (max_batch at most 64).  Anything else: RTD_E_INVALID
 * before anything is launched, logits_dev untouched. */
enum { RTD_EVA_POOL_TOKEN = 0, RTD_EVA_POOL_AVG = 1 };
typedef struct rtd_eva_config {
  int32_t struct_size; /* = sizeof(rtd_eva_config) */
  int32_t device;
  int32_t precision;   /* RTD_PREC_F16X3 | RTD_PREC_FP32 */
  int32_t max_batch;   /* 1..64 */
  int32_t img, patch;  /* 336, 14 */
  int32_t dim, depth, heads; /* 1024, 24, 16 (dim = 64 heads) */
  int32_t hidden;      /* the SwiGLU width before padding: int(dim * 8 / 3) = 2730 */
  int32_t classes;     /* 10000 */
  int32_t ref_feat;    /* the RoPE table's ref_feat_shape (16): recorded only, the table arrives in the blob */
  int32_t scale_attn_inner; /* 1: LayerNorm between attention and proj (`attn.norm`) */
  int32_t scale_mlp;   /* 1: LayerNorm between SwiGLU and fc2 (`mlp.norm`) */
  int32_t pool;        /* RTD_EVA_POOL_* */
  int32_t reserved0;
} rtd_eva_config;
typedef struct rtd_eva* rtd_eva_handle;
int rtd_eva_create(const rtd_eva_config* cfg, const void* blob, size_t nbytes, rtd_eva_handle* out);
/* x_dev: [n][3][img][img] fp32 NCHW, normalised (what rtd_crop_resize_batch writes); logits_dev: [n][classes] fp32 */
int rtd_eva_forward(rtd_eva_handle e, const float* x_dev, int32_t n, float* logits_dev, void* stream);
/* the pair format's one hazard on ViT outlier channels is fp16's range: *saturated = the values of the last call's final residual stream
 * found AT +-65504, plus its logits at or beyond 65504 or not finite (0 = healthy).  Waits for the last call's stream.  RTD_E_STATE
 * before the first successful forward. */
int rtd_eva_self_check(rtd_eva_handle e, int64_t* saturated);
int64_t rtd_eva_arena_bytes(rtd_eva_handle e);
const char* rtd_eva_last_error(rtd_eva_handle e);                          /* e may be NULL: last error of a failed rtd_eva_create */
void rtd_eva_close(rtd_eva_handle e);

/* ---- YOLOX post-processing: upstream's yolox.utils.postprocess(prediction, num_classes, conf_thre, nms_thre, class_agnostic=False)
 * with torchvision's batched_nms in its per-class form (_batched_nms_vanilla), and optionally the head's grid decode ------------------
 * Per image, on prediction[A][5 + C] fp32 rows (cx, cy, w, h, obj, C class scores):
 *   corners      x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2
 *   class        class_conf = the largest class score, class_id = the LOWEST index that holds it (a NaN class score makes class_conf NaN)
 *   candidates   the rows with obj * class_conf >= conf_threshold (NaN never passes) whose class has its class_keep bit set
 *   order        score = obj * class_conf descending; equal scores by lower anchor index first
 *   suppression  greedy in that order: a row is dropped when an earlier KEPT row of the SAME class has
 *                inter / (area_a + area_b - inter) > nms_threshold, with inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)) and
 *                area = (x2 - x1) * (y2 - y1), every operation one fp32 operation in this order.  The comparison is strict, and 0 / 0 is
 *                NaN, which is not greater: the row stays.
 *   rows         x1, y1, x2, y2, obj, class_conf, class_id (as a float), score descending; rows past `kept` are not written.
 * decode = 1: the rows are the head's undecoded output (upstream's YOLOXHead with decode_in_inference = False: raw box terms, obj and class
 * scores already sigmoided), levels of stride 8, 16, 32 in that order, row-major over (y, x) within a level, and
 *   cx = (t0 + x) * s, cy = (t1 + y) * s, w = exp(t2) * s, h = exp(t3) * s                     before the steps above.
 * When more rows pass than max_candidates, the best max_candidates by (score descending, anchor ascending) enter the suppression;
 * counts[i][1] still reports every row that passed (upstream has no such cap).
 * The handle owns NO stream: rtd_yolox_post_run is ASYNCHRONOUS on the caller's `stream` (as rtd_enhance_crops), one memset and four
 * launches whatever n is, and nothing crosses to the host between them.  Its scratch (candidate lists, ranked rows, the suppression bit
 * matrix: n * max_candidates^2 / 8 bytes) is grown on demand and belongs to the call in flight: calls on one handle go on ONE stream.
 * Refused with RTD_E_INVALID before anything is launched, outputs untouched: n outside 1..max_batch, n_anchors outside 1..max_anchors,
 * decode = 1 with n_anchors != rtd_yolox_anchors(in_h, in_w), a null pointer, a threshold outside [0, 1] or not finite, a wrong
 * struct_size.  csrc/yolox_post.hip, csrc/yolox_post_host.h; restated in tests/yolox_ref.py. */
typedef struct rtd_yolox_post_config {
  int32_t struct_size; /* = sizeof(rtd_yolox_post_config) */
  int32_t device;
  int32_t num_classes;    /* 1..1024 */
  int32_t max_batch;      /* 1..64 */
  int32_t max_anchors;    /* 1..2^20 */
  int32_t max_candidates; /* 64..8192, a multiple of 64 */
} rtd_yolox_post_config;
typedef struct rtd_yolox_post_params {
  int32_t struct_size; /* = sizeof(rtd_yolox_post_params) */
  float conf_threshold, nms_threshold; /* each in [0, 1], finite */
  int32_t decode;      /* 0: rows are cx, cy, w, h; 1: the head's output, see above */
  int32_t in_h, in_w;  /* read when decode = 1: multiples of 32 */
  const uint32_t* class_keep; /* HOST, NULL (every class) or ceil(num_classes / 32) words: a class whose bit is 0 never passes */
} rtd_yolox_post_params;
typedef struct rtd_yolox_post* rtd_yolox_post_handle;
/* pure host: the anchors of an in_h x in_w input (multiples of 32, 32..16384), (h/8)(w/8) + (h/16)(w/16) + (h/32)(w/32); 640 x 640 -> 8400 */
int rtd_yolox_anchors(int32_t in_h, int32_t in_w, int32_t* n_anchors);
int rtd_yolox_post_create(const rtd_yolox_post_config* cfg, rtd_yolox_post_handle* out);
/* pred_dev: [n][n_anchors][5 + num_classes] fp32 at any 4-byte address; rows_dev: [n][max_candidates][7]; counts_dev: [n][2] kept, passed */
int rtd_yolox_post_run(rtd_yolox_post_handle y, int32_t n, const float* pred_dev, int32_t n_anchors, const rtd_yolox_post_params* params,
                       float* rows_dev, int32_t* counts_dev, void* stream);
const char* rtd_yolox_post_last_error(rtd_yolox_post_handle y);            /* y may be NULL: the last refused create / anchors call */
void rtd_yolox_post_destroy(rtd_yolox_post_handle y);

/* ---- The YOLOX network (upstream's YOLOX(YOLOPAFPN(CSPDarknet), YOLOXHead) in eval mode with decode_in_inference = False) on the
 * library's conv kernels: Focus, CSPDarknet with SPP, PAFPN and the decoupled head, every BaseConv as conv + folded BatchNorm (eps
 * 1e-3) + SiLU.  Input: the reference's `preprocess` output, fp32 [n][3][in_h][in_w] BGR in 0..255 (no mean, no std).  Output: the
 * head's undecoded rows fp32 [n][A][5 + num_classes] - 4 raw box terms, sigmoid(obj), sigmoid(class scores); levels of stride 8, 16, 32
 * in that order, row-major over (y, x) - which is what rtd_yolox_post_run reads with decode = 1.  Restated in tests/yolox_net_ref.py.
 * Variants: base_channels = int(64 * width) must be a multiple of 32 (yolox-s: 32 with depth 1, yolox-l: 64 with depth 3; m, x, tiny
 * and the depthwise nano are refused).  precision: RTD_PREC_F16X3 (fp16 hi + lo pairs, three MFMAs per product) or RTD_PREC_FP32.
 * blob: the packed container of yolox_network.fold_state - per convolution `name`.weight [cout][k][k][cin] with the BatchNorm folded in
 * and `name`.bias [cout]; a table that is not this variant's is RTD_E_INVALID, a NaN, an infinity or (pair engine) |w| > 65504 is
 * RTD_E_WEIGHTS with the tensor's name.
 * The handle owns the filters, one cached plan per (n, in_h, in_w) and ONE arena that holds the largest plan seen (a repeated shape
 * allocates nothing).  It owns NO stream and captures nothing: rtd_yolox_net_run is ASYNCHRONOUS on the caller's `stream`, and the arena
 * belongs to the call in flight: calls on one handle go on ONE stream.  Refused with RTD_E_INVALID before anything is launched: a null
 * pointer, a wrong struct_size, n outside 1..max_batch, a side that is no multiple of 32, in_dev off a 16-byte boundary, pred_dev off a
 * 4-byte boundary, and any shape the conv launchers refuse (with their message).  csrc/yolox_net.hip, csrc/yolox_net_host.h. */
typedef struct rtd_yolox_net_config {
  int32_t struct_size;   /* = sizeof(rtd_yolox_net_config) */
  int32_t device;
  int32_t precision;     /* RTD_PREC_F16X3 | RTD_PREC_FP32 */
  int32_t num_classes;   /* 1..1024 */
  int32_t base_channels; /* int(64 * width): 32 (yolox-s) or 64 (yolox-l) */
  int32_t depth;         /* max(round(3 * depth), 1): 1 (yolox-s), 3 (yolox-l) */
  int32_t max_batch;     /* 1..64 */
  int32_t reserved0;
} rtd_yolox_net_config;
typedef struct rtd_yolox_net* rtd_yolox_net_handle;
int rtd_yolox_net_create(const rtd_yolox_net_config* cfg, const void* blob, size_t nbytes, rtd_yolox_net_handle* out);
int rtd_yolox_net_run(rtd_yolox_net_handle y, int32_t n, const float* in_dev /* [n][3][in_h][in_w] */, int32_t in_h, int32_t in_w,
                      float* pred_dev /* [n][rtd_yolox_anchors(in_h, in_w)][5 + num_classes] */, void* stream);
/* The same call from the camera frames themselves (in place of src/yolox_detector.py:186-220 `preprocess` + the call above): frame i is a
 * contiguous uint8 HWC BGR device buffer of frame_hw[i] = (h, w), sides 1..16384, at ANY byte address; frames of one call may differ in
 * size.  One kernel resizes them as F.interpolate(mode = "bilinear", align_corners = False) does on the float frame - fp32, source
 * coordinate max(scale * (d + 0.5) - 0.5, 0) with scale = (float)src / (float)dst, every operation rounded on its own - and writes the
 * Focus map; no float frame and no resized image exists.  A frame already in_h x in_w passes as its integers.  Same plan cache, arena,
 * stream rule and refusals as rtd_yolox_net_run but for the input's alignment; also refused before anything is allocated or launched: a
 * null array, a null frame pointer, a side outside 1..16384.  frames_dev and frame_hw are HOST arrays, read before the call returns.
 * Restated in tests/yolox_frames_ref.py. */
int rtd_yolox_net_run_frames(rtd_yolox_net_handle y, int32_t n, const uint8_t* const* frames_dev /* host array of n device pointers */,
                             const int32_t* frame_hw /* host [n][2]: h, w */, int32_t in_h, int32_t in_w, float* pred_dev, void* stream);
int64_t rtd_yolox_net_arena_bytes(rtd_yolox_net_handle y);
const char* rtd_yolox_net_last_error(rtd_yolox_net_handle y);              /* y may be NULL: the last refused create / rtd_op_yolox_* call */
void rtd_yolox_net_destroy(rtd_yolox_net_handle y);

#ifdef __cplusplus
}
#endif
#endif /* RTDETR_MI355_H */
