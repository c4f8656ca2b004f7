"""The JPEG encoder without a GPU: the numpy restatement (tests/jpeg_ref.py) against the Pillow fixtures (tests/golden/jpeg_small.npz,
jpeg_large.json; tools/make_jpeg_golden.py) and against Pillow / cv2 live where they are importable, and the Python wrapper
(JpegEncoder, imencode, install) over the restatement backend."""
import collections
import hashlib
import io
import json
import os
import threading
import types

import numpy as np
import pytest

from tests import jpeg_ref as ref
from telescope_cam_detection_amd import jpeg
from telescope_cam_detection_amd.synth import make_frame, noise_frame, scene_frame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUALITIES = [1, 25, 50, 75, 90, 95, 100]


def small_cases():
    z = np.load(os.path.join(GOLDEN, "jpeg_small.npz"))
    names = sorted(k[3:] for k in z.files if k.startswith("in_"))
    assert len(names) >= 12
    return z, names


def large_entries():
    with open(os.path.join(GOLDEN, "jpeg_large.json")) as f:
        return json.load(f)["entries"]


def test_restatement_reproduces_every_small_fixture_byte_for_byte():
    z, names = small_cases()
    for name in names:
        a = z["in_" + name]
        for q in QUALITIES:
            want = z[f"jpg_{name}_q{q}"].tobytes()
            got = ref.encode(a, q)
            assert got == want, (name, q, len(got), len(want))


def test_restatement_reproduces_the_large_fixtures():
    entries = large_entries()
    assert {(e["h"], e["w"]) for e in entries} == {(1080, 1920), (720, 1280), (487, 641)}
    for e in entries:
        got = ref.encode(make_frame(e["kind"], e["seed"], e["h"], e["w"]), e["quality"])
        assert (len(got), hashlib.sha256(got).hexdigest()) == (e["length"], e["sha256"]), e


def _pillow(a, q):
    from PIL import Image
    a = a[:, :, 0] if a.shape[2] == 1 else np.ascontiguousarray(a[:, :, ::-1])
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q)
    return buf.getvalue()


def _fresh():
    return [(noise_frame(101, 37, 91), 80), (scene_frame(102, 122, 66), 35), (noise_frame(103, 64, 200)[:, :, :1].copy(), 99),
            (scene_frame(104, 90, 161)[:, :, 2:].copy(), 10), (scene_frame(105, 240, 320), 90)]


def test_restatement_equals_pillow_live_and_pillow_decodes_it():
    pytest.importorskip("PIL", reason="Pillow is not installed: the live comparison needs it (the fixtures hold its bytes)")
    from PIL import Image
    for a, q in _fresh():
        got = ref.encode(a, q)
        assert got == _pillow(a, q), (a.shape, q)
        im = Image.open(io.BytesIO(got))
        im.load()
        assert im.size == (a.shape[1], a.shape[0]) and im.mode == ("L" if a.shape[2] == 1 else "RGB")


def test_restatement_equals_cv2_imencode():
    cv2 = pytest.importorskip("cv2", reason="cv2 is not installed: its bytes are compared only where it is")
    for a, q in _fresh():
        ok, enc = cv2.imencode(".jpg", a, [cv2.IMWRITE_JPEG_QUALITY, q])
        assert ok and enc.tobytes() == ref.encode(a, q), (a.shape, q)


# ---- the wrapper over the restatement backend -----------------------------------------------------------------------------------------
def test_encoder_types_batches_and_parameter_handling():
    be = ref.RefBackend()
    enc = jpeg.JpegEncoder(device=0, backend=be)
    a, g = scene_frame(1, 40, 56), noise_frame(2, 24, 31)[:, :, 0].copy()
    one = enc.encode(a)
    assert isinstance(one, bytes) and one == ref.encode(a, 95) and be.calls[-1] == (1, False, 95)
    assert enc.encode(g, quality=50) == ref.encode(g, 50)                   # HxW is a gray frame
    assert enc.encode(a[:, ::2], 75) == ref.encode(np.ascontiguousarray(a[:, ::2]), 75)      # non-contiguous input
    import torch
    assert enc.encode(torch.from_numpy(a), 90) == ref.encode(a, 90)         # a host tensor
    many = enc.encode_batch([a, g, a], quality=25)
    assert many == [ref.encode(a, 25), ref.encode(g, 25), ref.encode(a, 25)] and be.calls[-1] == (3, False, 25)
    assert enc.encode_batch([]) == [] and be.waits == 0
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            enc.encode(a, bad)
    with pytest.raises(ValueError):
        enc.encode(a.astype(np.float32))
    with pytest.raises(ValueError):
        enc.encode(np.zeros((4, 4, 2), np.uint8))


def test_imencode_has_the_cv2_call_shape():
    enc = jpeg.JpegEncoder(device=0, backend=ref.RefBackend())
    a = scene_frame(3, 33, 47)
    ok, buf = jpeg.imencode(".jpg", a, encoder=enc)
    assert ok is True and isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.ndim == 1
    assert buf.tobytes() == ref.encode(a, 95)                               # OpenCV's default quality
    ok, buf = jpeg.imencode(".JPEG", a, [jpeg.IMWRITE_JPEG_QUALITY, 60], encoder=enc)
    assert ok and buf.tobytes() == ref.encode(a, 60)
    ok, buf = jpeg.imencode(".jpg", a, [jpeg.IMWRITE_JPEG_QUALITY, 0], encoder=enc)      # libjpeg turns quality 0 into 1
    assert ok and buf.tobytes() == ref.encode(a, 1)
    try:
        import cv2  # noqa: F401
        have_cv2 = True
    except ImportError:
        have_cv2 = False
    if have_cv2:
        ok, buf = jpeg.imencode(".png", a, encoder=enc)
        assert ok and bytes(buf[:4]) == b"\x89PNG"
    else:
        with pytest.raises(ValueError):
            jpeg.imencode(".png", a, encoder=enc)
        with pytest.raises(ValueError):
            jpeg.imencode(".jpg", a, [2, 1], encoder=enc)                  # IMWRITE_JPEG_PROGRESSIVE: not encoded here


class StandInSaver:
    """the attributes and the bookkeeping of the reference's SnapshotSaver that add_frame_to_buffer touches (src/snapshot_saver.py)"""

    def __init__(self, maxlen=4, use_compressed_buffer=True):
        self.frame_buffer = collections.deque(maxlen=maxlen)
        self.buffer_lock = threading.Lock()
        self.use_compressed_buffer = use_compressed_buffer
        self.buffer_memory_bytes = 0
        self.estimated_buffer_memory_mb = 0.0
        self.original_calls = []

    def _estimate_frame_size(self, frame_data):
        if "frame_compressed" in frame_data:
            return frame_data["frame_compressed"].nbytes
        if "frame" in frame_data and frame_data["frame"] is not None:
            return frame_data["frame"].nbytes
        return 0

    def add_frame_to_buffer(self, frame, timestamp):
        self.original_calls.append(timestamp)


class FakeDeviceFrame:
    """what the wrapper asks of a device tensor, over a numpy array (the CPU test has no device)"""

    is_cuda = True
    device = 0

    def __init__(self, a):
        import torch
        self._a = a
        self.dtype = torch.uint8
        self.shape = a.shape

    def dim(self):
        return self._a.ndim

    def contiguous(self):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return self._a

    def data_ptr(self):
        return self._a.ctypes.data


def stand_in_module():
    return types.SimpleNamespace(SnapshotSaver=type("SnapshotSaver", (StandInSaver,), {}), MAX_BUFFER_MEMORY_MB=500)


def reference_bookkeeping(sizes, maxlen):
    """buffer_memory_bytes after each append, as snapshot_saver.py:162-179 computes it"""
    buf, total, out = collections.deque(maxlen=maxlen), 0, []
    for s in sizes:
        if len(buf) == buf.maxlen:
            total -= buf[0]
        buf.append(s)
        total += s
        out.append(total)
    return out


def test_installed_add_frame_to_buffer_bookkeeping_and_fall_through(monkeypatch):
    mod = stand_in_module()
    be = ref.RefBackend()
    jpeg.install(mod, encoder=jpeg.JpegEncoder(device=0, backend=be))
    monkeypatch.setattr("torch.cuda.current_stream", lambda *_a, **_k: types.SimpleNamespace(cuda_stream=0))
    saver = mod.SnapshotSaver(maxlen=4)
    frames = [scene_frame(20 + i, 48 + 8 * i, 64) for i in range(7)]
    want = [ref.encode(f, 90) for f in frames]
    track = reference_bookkeeping([len(w) for w in want], 4)
    for i, f in enumerate(frames):
        saver.add_frame_to_buffer(FakeDeviceFrame(f), 100.0 + i)
        assert saver.buffer_memory_bytes == track[i]
        assert saver.estimated_buffer_memory_mb == track[i] / (1024 * 1024)
    assert be.waits == 7 and saver.original_calls == []
    assert len(saver.frame_buffer) == 4
    for entry, w, i in zip(saver.frame_buffer, want[3:], range(3, 7)):
        assert set(entry) == {"frame_compressed", "timestamp"} and entry["timestamp"] == 100.0 + i
        c = entry["frame_compressed"]
        assert isinstance(c, np.ndarray) and c.dtype == np.uint8 and c.ndim == 1 and c.tobytes() == w
    assert saver.buffer_memory_bytes == sum(len(w) for w in want[3:])
    # numpy frames, None and an uncompressed buffer keep the reference's own path
    saver.add_frame_to_buffer(frames[0], 1.0)
    saver.add_frame_to_buffer(None, 2.0)
    assert saver.original_calls == [1.0] and len(be.calls) == 7
    plain = mod.SnapshotSaver(maxlen=2, use_compressed_buffer=False)
    plain.add_frame_to_buffer(FakeDeviceFrame(frames[0]), 3.0)
    assert plain.original_calls == [3.0] and len(plain.frame_buffer) == 0
    jpeg.install(mod)                                                       # a second install wraps the original once
    assert mod.SnapshotSaver._rtd_original_add_frame_to_buffer is StandInSaver.add_frame_to_buffer


class SharedBufferBackend(jpeg.DeviceBackend):
    """DeviceBackend's own encode (lock, retry with a larger array, copy-out) over a stand-in for the library call: the files are written
    into the caller's array by the restatement and the call then yields, as a ctypes call does when it gives the GIL back, so that
    another thread's call lands in the shared array before this thread copies its bytes out."""

    def __init__(self):                       # no library, no handle
        from telescope_cam_detection_amd import _capi
        self._capi = _capi
        self._h = None
        self._out = np.empty(256, np.uint8)   # small: the first calls also take the grow-and-repeat path
        self._lock = threading.Lock()
        self.in_call = 0
        self.overlapped = False

    def encode_raw(self, ptrs, shapes, on_device, quality, out):
        import ctypes
        import time
        self.in_call += 1
        self.overlapped |= self.in_call > 1
        files = []
        for p, s in zip(ptrs, shapes):
            n = int(np.prod(s))
            a = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(p)).reshape(s)
            files.append(ref.encode(a, quality))
        offs = [0]
        for f in files:
            offs.append(offs[-1] + len(f))
        rc = self._capi.RTD_OK
        if out is None or out.nbytes < offs[-1]:
            rc = self._capi.RTD_E_INVALID
        else:
            out[:offs[-1]] = np.frombuffer(b"".join(files), np.uint8)
        time.sleep(0.002)                     # the other threads run here
        self.in_call -= 1
        return rc, offs

    def _raise(self, rc):
        raise RuntimeError(f"the stand-in call returned {rc}")

    def wait_stream(self, producer_stream):
        pass

    def close(self):
        pass


def test_one_saver_and_one_encoder_shared_by_several_camera_threads(monkeypatch):
    """the reference's layout: ONE SnapshotSaver for all cameras, add_frame_to_buffer called from every camera's thread; each thread
    must get its own frame's file although all calls share the backend's output array"""
    mod = stand_in_module()
    be = SharedBufferBackend()
    jpeg.install(mod, encoder=jpeg.JpegEncoder(device=0, backend=be))
    monkeypatch.setattr("torch.cuda.current_stream", lambda *_a, **_k: types.SimpleNamespace(cuda_stream=0))
    cams, per_cam = 6, 8
    saver = mod.SnapshotSaver(maxlen=cams * per_cam)
    frames = {(c, i): scene_frame(100 * c + i, 24 + 8 * c, 40 + 8 * (i % 3)) for c in range(cams) for i in range(per_cam)}
    want = {k: ref.encode(f, 90) for k, f in frames.items()}
    errors = []
    start = threading.Barrier(cams)

    def camera(c):
        try:
            start.wait()
            for i in range(per_cam):
                saver.add_frame_to_buffer(FakeDeviceFrame(frames[(c, i)]), float(1000 * c + i))
        except Exception as e:                # noqa: BLE001 - reported below
            errors.append(repr(e))

    threads = [threading.Thread(target=camera, args=(c,)) for c in range(cams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not be.overlapped                  # a call and its copy-out are one critical section
    assert len(saver.frame_buffer) == cams * per_cam
    for entry in saver.frame_buffer:
        c, i = divmod(int(entry["timestamp"]), 1000)
        assert entry["frame_compressed"].tobytes() == want[(c, i)], (c, i)
    assert saver.buffer_memory_bytes == sum(len(w) for w in want.values())


def test_default_encoder_builds_one_encoder_per_device_under_concurrent_first_use(monkeypatch):
    import time
    built = []

    class SlowEncoder:
        def __init__(self, device=None, backend=None):
            time.sleep(0.01)
            built.append(device)

    monkeypatch.setattr(jpeg, "JpegEncoder", SlowEncoder)
    monkeypatch.setattr(jpeg, "_encoders", {})
    got = []
    threads = [threading.Thread(target=lambda: got.append(jpeg.default_encoder(0))) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert built == [0] and len(got) == 8 and all(g is got[0] for g in got)
