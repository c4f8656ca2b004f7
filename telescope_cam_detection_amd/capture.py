"""Camera capture that runs on an AMD host: the reference's `RTSPStreamCaptureGPU` (src/stream_capture_gpu_ffmpeg.py) without its
NVIDIA-only decoder flags, and without the CPU colour conversion in front of the pipe.

ffmpeg is asked for its decoder's own 4:2:0 output (`-pix_fmt nv12`, 1.5 bytes per pixel; the reference asks for bgr24, 3 bytes per
pixel made by swscale on a CPU core), the capture thread reads `frame_bytes(H, W)` bytes per frame and the frame ingest (ingest.py,
csrc/ingest.hip) turns them into the [H, W, 3] uint8 BGR device tensor every later stage takes.  Constructor, attributes, methods,
loop semantics and the queue item are the reference class's; what differs:

* `decoder_args` (default none) goes in front of `-i`: a site names its hardware decoder there, e.g. ("-hwaccel", "vaapi").
* `matrix` / `full_range` choose the conversion (BT.601 limited by default: swscale's own choice for a stream without colour tags).
* `source_size=(w, h)` states the stream's native size: ffmpeg is then asked for no `-s` (no swscale resize on a CPU core), the thread
  reads native frames and the ingest resizes them to the target size on the GPU (`cv2.resize`'s bytes, not swscale's); with
  `keep_native` the native BGR frame stays on the device beside it (`latest_native_frame`, the queue item's `native_frame`) for Stage 2.
* `popen` and `ingest` are seams for tests: a stand-in for subprocess.Popen, and an object with `to_bgr` as FrameIngest.

`install(main_module)` lets the reference's main.py build this class in place of its `RTSPStreamCapture` without editing it.
"""
from __future__ import annotations

import logging
import subprocess
import time
from queue import Full, Queue
from threading import Event, Lock, Thread
from typing import Optional, Sequence, Tuple

from .ingest import frame_bytes

logger = logging.getLogger(__name__)

ITEM_KEYS = ("frame", "timestamp", "frame_id", "camera_id", "camera_name", "is_gpu_tensor")


class RTSPStreamCaptureGPU:
    """One camera: an ffmpeg child that writes raw NV12 frames to a pipe, a thread that reads them, converts them on the GPU and feeds
    `frame_queue`."""

    # seconds: ffmpeg's start-up check, the pause before a reconnect, the pause after an exception in the loop (the reference's values)
    settle_delay = 0.5
    reconnect_delay = 2.0
    error_delay = 1.0

    def __init__(self, rtsp_url: str, frame_queue: Queue, target_width: int = 1280, target_height: int = 720, camera_id: str = "default",
                 camera_name: str = "Default Camera", use_tcp: bool = False, buffer_size: Optional[int] = None, max_failures: int = 30,
                 retry_delay: float = 5.0, keep_frames_on_gpu: bool = True, device="cuda:0", decoder_args: Sequence[str] = (),
                 matrix: str = "bt601", full_range: bool = False, popen=subprocess.Popen, ingest=None,
                 source_size: Optional[Tuple[int, int]] = None, keep_native: bool = False):
        import torch

        self.rtsp_url = rtsp_url
        self.frame_queue = frame_queue
        self.target_width = int(target_width)
        self.target_height = int(target_height)
        self.camera_id = camera_id
        self.camera_name = camera_name
        self.use_tcp = use_tcp
        self.buffer_size = buffer_size
        self.max_failures = max_failures
        self.retry_delay = retry_delay
        self.keep_frames_on_gpu = keep_frames_on_gpu
        self.device = torch.device(device) if isinstance(device, str) else device
        self.decoder_args = tuple(str(a) for a in decoder_args)
        self.matrix = matrix
        self.full_range = bool(full_range)
        self._popen = popen
        self._ingest = ingest
        # (w, h) of the stream as the camera sends it: the operator's statement, nothing probes it
        self.source_size = None if source_size is None else (int(source_size[0]), int(source_size[1]))
        self.keep_native = bool(keep_native)
        if self.keep_native and self.source_size is None:
            raise ValueError("keep_native needs source_size")
        if buffer_size is not None:
            logger.warning(f"[{camera_id}] buffer_size={buffer_size} is ignored: ffmpeg buffers the stream itself")

        self.ffmpeg_process = None
        self.stop_event = Event()
        self.capture_thread: Optional[Thread] = None
        self.is_connected = False
        self.latest_frame = None              # a device tensor, or a numpy array with keep_frames_on_gpu = False
        self.latest_native_frame = None       # with keep_native: the same frame at the source size
        self.frame_lock = Lock()

        self.frame_count = 0                  # frames since the last FPS reading
        self.frame_id_counter = 0             # never reset
        self.dropped_frames = 0
        self.reconnects = 0
        self.last_fps_check = time.time()
        self.fps = 0.0

    # ---- the ffmpeg child ---------------------------------------------------------------------------------------------------------------
    def _build_ffmpeg_command(self) -> list:
        cmd = ["ffmpeg", *self.decoder_args]
        if self.use_tcp:
            cmd += ["-rtsp_transport", "tcp"]
        if self.source_size is not None:      # native frames over the pipe: the resize is the ingest's
            return cmd + ["-i", self.rtsp_url, "-f", "rawvideo", "-pix_fmt", "nv12", "pipe:1"]
        cmd += ["-i", self.rtsp_url, "-f", "rawvideo", "-pix_fmt", "nv12", "-s", f"{self.target_width}x{self.target_height}", "pipe:1"]
        return cmd

    def connect(self) -> bool:
        logger.info(f"[{self.camera_id}] Connecting to {self.rtsp_url} (ffmpeg, NV12 over a pipe)")
        try:
            if self._ingest is None:
                from .ingest import FrameIngest
                self._ingest = FrameIngest(self.device)
            self.ffmpeg_process = self._popen(self._build_ffmpeg_command(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, bufsize=10 ** 8)
            if self.settle_delay:
                time.sleep(self.settle_delay)
            if self.ffmpeg_process.poll() is not None:
                stderr = self.ffmpeg_process.stderr.read().decode("utf-8", errors="ignore")
                logger.error(f"[{self.camera_id}] ffmpeg did not start: {stderr[:500]}")
                return False
            self.is_connected = True
            return True
        except Exception as e:
            logger.error(f"[{self.camera_id}] Connection error: {e}")
            return False

    def _end_process(self, wait_s: float) -> bool:
        """terminate, then kill; True when the child is gone (its reference is then dropped), False when it could not be ended"""
        proc = self.ffmpeg_process
        if proc is None:
            return True
        try:
            proc.terminate()
            try:
                proc.wait(timeout=wait_s)
            except subprocess.TimeoutExpired:
                logger.warning(f"[{self.camera_id}] ffmpeg ignored terminate(), killing it")
                proc.kill()
                proc.wait(timeout=2.0)
        except Exception as e:                # (a second TimeoutExpired included: the reference is kept, so the zombie stays visible)
            logger.error(f"[{self.camera_id}] could not end ffmpeg: {e!r}")
            return False
        self.ffmpeg_process = None
        return True

    def start(self) -> bool:
        """starts the capture thread; the connection is made by the thread"""
        self.stop_event.clear()
        self.capture_thread = Thread(target=self._capture_loop, daemon=True)
        self.capture_thread.start()
        return True

    def stop(self) -> None:
        self.stop_event.set()
        if self.capture_thread is not None:
            self.capture_thread.join(timeout=5.0)
            if self.capture_thread.is_alive():
                logger.error(f"[{self.camera_id}] the capture thread did not stop within 5 s")
        if not self._end_process(5.0):
            return
        self.is_connected = False

    def _reconnect(self) -> bool:
        self.reconnects += 1
        gone = self._end_process(2.0)
        self.is_connected = False
        if not gone:
            return False
        if self.reconnect_delay:
            time.sleep(self.reconnect_delay)
        return self.connect()

    # ---- the loop -----------------------------------------------------------------------------------------------------------------------
    def _convert_native(self, raw: bytes):
        """one native NV12 frame off the pipe -> (the target-size BGR frame, the native BGR frame or None)"""
        sw, sh = self.source_size
        kw = dict(layout="nv12", matrix=self.matrix, full_range=self.full_range, out_sizes=(self.target_height, self.target_width))
        if self.keep_native:
            imgs, natives = self._ingest.to_bgr([raw], [(sh, sw)], native_out=True, **kw)
            img, native = imgs[0], natives[0]
        else:
            img, native = self._ingest.to_bgr([raw], [(sh, sw)], **kw)[0], None
        if not self.keep_frames_on_gpu:
            img, native = img.cpu().numpy(), None if native is None else native.cpu().numpy()
        return img, native

    def _convert(self, raw: bytes):
        """one NV12 frame off the pipe -> a BGR device tensor, or its numpy copy"""
        size = (self.target_height, self.target_width)
        img = self._ingest.to_bgr([raw], [size], layout="nv12", matrix=self.matrix, full_range=self.full_range)[0]
        return img if self.keep_frames_on_gpu else img.cpu().numpy()

    def _failed(self, failures: int) -> int:
        """a failure has been counted: reconnect at max_failures; returns the new count"""
        if failures < self.max_failures:
            return failures
        logger.error(f"[{self.camera_id}] {failures} failures in a row, reconnecting")
        self._reconnect()
        return 0

    def _capture_loop(self) -> None:
        failures = 0
        need = frame_bytes(self.target_height, self.target_width) if self.source_size is None else frame_bytes(self.source_size[1], self.source_size[0])
        while not self.stop_event.is_set():
            try:
                if not self.is_connected or self.ffmpeg_process is None:
                    if not self.connect():
                        logger.warning(f"[{self.camera_id}] not connected, next attempt in {self.retry_delay} s")
                        if self.stop_event.wait(self.retry_delay):
                            break
                        continue
                    failures = 0
                raw = self.ffmpeg_process.stdout.read(need)
                if len(raw) != need:
                    failures += 1
                    logger.warning(f"[{self.camera_id}] short read: {len(raw)} of {need} bytes ({failures}/{self.max_failures})")
                    failures = self._failed(failures)
                    continue
                native = None
                if self.source_size is None:
                    img = self._convert(raw)
                else:
                    img, native = self._convert_native(raw)
                with self.frame_lock:
                    self.latest_frame = img
                    if self.keep_native:
                        self.latest_native_frame = native
                # the queue gets a tensor of its own: its consumer and the readers of latest_frame never share memory
                own = (lambda t: t.clone()) if self.keep_frames_on_gpu else (lambda a: a.copy())
                item = {"frame": own(img), "timestamp": time.time(), "frame_id": self.frame_id_counter, "camera_id": self.camera_id,
                        "camera_name": self.camera_name, "is_gpu_tensor": self.keep_frames_on_gpu}
                if self.keep_native:
                    item["native_frame"] = own(native)
                try:
                    self.frame_queue.put_nowait(item)
                    self.frame_count += 1
                    self.frame_id_counter += 1
                except Full:
                    self.dropped_frames += 1
                self._update_fps()
                failures = 0
            except Exception as e:
                failures += 1
                logger.warning(f"[{self.camera_id}] stream error ({failures}/{self.max_failures}): {e!r}")
                failures = self._failed(failures)
                if self.error_delay:
                    time.sleep(self.error_delay)

    def _update_fps(self) -> None:
        now = time.time()
        if now - self.last_fps_check < 1.0:
            return
        self.fps = self.frame_count / (now - self.last_fps_check)
        self.last_fps_check = now
        self.frame_count = 0
        if self.dropped_frames:
            logger.debug(f"[{self.camera_id}] {self.fps:.1f} fps, {self.dropped_frames} dropped")
            self.dropped_frames = 0           # (as the reference: the count of the last second)

    # ---- readers ------------------------------------------------------------------------------------------------------------------------
    def get_latest_frame(self):
        with self.frame_lock:
            return self.latest_frame

    def get_latest_native_frame(self):
        with self.frame_lock:
            return self.latest_native_frame

    def get_latest_frame_as_numpy(self):
        frame = self.get_latest_frame()
        if frame is not None and hasattr(frame, "cpu"):
            frame = frame.cpu().numpy()
        return frame

    def get_stats(self) -> dict:
        return {"is_connected": self.is_connected, "fps": self.fps, "total_frames": self.frame_count, "dropped_frames": self.dropped_frames,
                "queue_size": self.frame_queue.qsize()}


def install(main_module, source_size=None, **defaults) -> None:
    """Let the reference's main.py capture through this class without editing it:

        import main, telescope_cam_detection_amd.capture as cap
        cap.install(main, decoder_args=("-hwaccel", "vaapi"))

    `main._create_stream_capture` builds `RTSPStreamCapture(rtsp_url=..., frame_queue=..., target_width=..., target_height=...,
    camera_id=..., camera_name=..., use_tcp=..., buffer_size=..., max_failures=..., retry_delay=...)`; the name is rebound to a subclass of
    RTSPStreamCaptureGPU that takes those keywords and adds `defaults` (decoder_args, device, keep_frames_on_gpu, matrix, full_range,
    keep_native).  `source_size` is one (w, h) for all cameras, or a dict keyed by camera_id: a camera that is absent from it keeps the
    `-s` command (and gets no keep_native)."""
    class RTSPStreamCapture(RTSPStreamCaptureGPU):
        def __init__(self, *args, **kwargs):
            kw = {**defaults, **kwargs}
            if source_size is not None and "source_size" not in kwargs:
                cam = kw.get("camera_id", "default")
                kw["source_size"] = source_size.get(cam) if isinstance(source_size, dict) else source_size
                if kw["source_size"] is None:
                    kw.pop("keep_native", None)
            super().__init__(*args, **kw)

    if not hasattr(main_module, "_rtd_original_RTSPStreamCapture"):
        main_module._rtd_original_RTSPStreamCapture = getattr(main_module, "RTSPStreamCapture", None)
    main_module.RTSPStreamCapture = RTSPStreamCapture
