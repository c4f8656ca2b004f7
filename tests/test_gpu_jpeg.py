"""The JPEG encoder on the MI355X (csrc/jpeg.hip): files byte-identical to Pillow's (tests/golden/jpeg_small.npz, jpeg_large.json) for host
and device frames, alone and batched, device frames also as views at odd byte offsets of a shared buffer; the bench layout of 8 x 1080p; capacity and argument handling of rtd_jpeg_encode; stream ordering
of device frames; the installed snapshot-saver path.  On a mismatch the first differing coefficient block is reported
(rtd_debug_jpeg_coefficients against tests/jpeg_ref.py)."""
import hashlib

import numpy as np
import pytest
import torch

from tests import jpeg_ref as ref
from tests.frontend_ref import Placed
from tests.test_jpeg_host import QUALITIES, large_entries, reference_bookkeeping, small_cases, stand_in_module
from telescope_cam_detection_amd import _capi, jpeg
from telescope_cam_detection_amd.synth import make_frame, scene_frame

pytestmark = pytest.mark.gpu


@pytest.fixture()
def be():
    b = jpeg.DeviceBackend(0)
    yield b
    b.close()


def explain(be, frames, quality):
    """where the coefficients of the last call first differ from the restatement's"""
    got = be.coefficients()
    want = np.concatenate([ref.coefficients(f, quality) for f in frames])
    if got.shape != want.shape:
        return f"coefficient blocks: got {got.shape}, want {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    if not len(bad):
        return "coefficients equal the restatement's: the entropy coder or the stuffing differs"
    b = int(bad[0])
    return f"{len(bad)} of {len(want)} blocks differ; first block {b}: got {got[b].tolist()} want {want[b].tolist()}"


def check(be, frames, quality, want, on_device):
    args = [torch.from_numpy(f).cuda() for f in frames] if on_device else frames
    torch.cuda.synchronize()
    got = be.encode(args, on_device, quality)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, frames[i].shape, quality, on_device, len(g), len(w), explain(be, frames, quality))
    assert len(got) == len(want)


def test_every_small_fixture_is_byte_identical_alone(be):
    z, names = small_cases()
    for name in names:
        a = z["in_" + name]
        for q in QUALITIES:
            for dev in (False, True):
                check(be, [a], q, [z[f"jpg_{name}_q{q}"].tobytes()], dev)


def test_every_small_fixture_is_byte_identical_in_one_batch_per_quality(be):
    z, names = small_cases()
    frames = [z["in_" + n] for n in names]
    for q in QUALITIES:
        want = [z[f"jpg_{n}_q{q}"].tobytes() for n in names]
        for dev in (False, True):
            check(be, frames, q, want, dev)


def test_device_frames_at_any_byte_address_are_byte_identical(be):
    """transform_kernel stages a tile's rows as aligned dwords and puts a dword that leaves the frame together from bytes: every small
    fixture at every quality from device frames that are views 1, 2, 3 and 0 bytes past a 16-byte boundary of one 0xFF-filled buffer
    (>= 4 KiB of filler around each: a stray read neither faults nor goes unseen), alone and then all in one batch at mixed offsets."""
    z, names = small_cases()
    frames = [z["in_" + n] for n in names]
    same = [Placed(frames, [off] * len(frames), 0xFF) for off in (1, 2, 3, 0)]
    mixed = Placed(frames, [(1, 2, 3, 0)[i % 4] for i in range(len(frames))], 0xFF)
    assert {p % 16 for p in mixed.ptrs} == {0, 1, 2, 3}
    for q in QUALITIES:
        want = [z[f"jpg_{n}_q{q}"].tobytes() for n in names]
        for placed in same:
            for i, f in enumerate(frames):
                got = be.encode([placed.views[i]], True, q)
                assert got == [want[i]], (names[i], q, placed.ptrs[i] % 16, len(got[0]), len(want[i]), explain(be, [f], q))
        got = be.encode(mixed.views, True, q)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (names[i], q, mixed.ptrs[i] % 16, len(g), len(w), explain(be, frames, q))
        assert len(got) == len(want)


def test_large_fixtures_match_length_and_sha256(be):
    for e in large_entries():
        a = make_frame(e["kind"], e["seed"], e["h"], e["w"])
        for dev in (False, True):
            arg = torch.from_numpy(a).cuda() if dev else a
            torch.cuda.synchronize()
            got = be.encode([arg], dev, e["quality"])[0]
            ok = (len(got), hashlib.sha256(got).hexdigest()) == (e["length"], e["sha256"])
            assert ok, (e, dev, len(got), explain(be, [a], e["quality"]))


def test_batch_equals_singles_and_eight_1080p_device_frames(be):
    frames = [scene_frame(40 + i, 1080, 1920) for i in range(8)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    batch = be.encode(dev, True, 90)
    singles = [be.encode([d], True, 90)[0] for d in dev]
    assert batch == singles
    e = [x for x in large_entries() if (x["kind"], x["h"], x["quality"]) == ("scene", 1080, 90)][0]
    first = be.encode([torch.from_numpy(make_frame("scene", e["seed"], 1080, 1920)).cuda()] + dev[1:], True, 90)
    assert hashlib.sha256(first[0]).hexdigest() == e["sha256"] and first[1:] == batch[1:]
    for b, f in zip(batch[:2], frames[:2]):                                 # (the restatement takes seconds per 1080p frame)
        assert b == ref.encode(f, 90)


def test_two_calls_with_different_sizes_and_qualities_on_one_handle(be):
    a, b, c = scene_frame(1, 250, 130), scene_frame(2, 33, 47)[:, :, :1].copy(), scene_frame(3, 487, 641)
    assert be.encode([a, b], False, 30) == [ref.encode(a, 30), ref.encode(b, 30)]
    assert be.encode([c], False, 95) == [ref.encode(c, 95)]
    assert be.encode([b, a], False, 75) == [ref.encode(b, 75), ref.encode(a, 75)]


def test_capacity_too_small_reports_the_size_and_the_repeat_succeeds(be):
    a, b = scene_frame(4, 120, 200), scene_frame(5, 64, 64)
    want = [ref.encode(a, 80), ref.encode(b, 80)]
    ptrs, shapes = [a.ctypes.data, b.ctypes.data], [a.shape, b.shape]
    small = np.empty(100, np.uint8)
    rc, offs = be.encode_raw(ptrs, shapes, False, 80, small)
    assert rc == _capi.RTD_E_INVALID and offs[-1] == len(want[0]) + len(want[1])
    rc, offs = be.encode_raw(ptrs, shapes, False, 80, None)                 # a size query
    assert rc == _capi.RTD_E_INVALID and offs[-1] == len(want[0]) + len(want[1])
    out = np.empty(offs[-1], np.uint8)
    rc, offs = be.encode_raw(ptrs, shapes, False, 80, out)
    assert rc == _capi.RTD_OK and offs == [0, len(want[0]), len(want[0]) + len(want[1])]
    assert out[:offs[1]].tobytes() == want[0] and out[offs[1]:].tobytes() == want[1]


def test_bad_arguments_are_refused(be):
    a = scene_frame(6, 16, 16)
    out = np.empty(1 << 16, np.uint8)
    for ptrs, shapes, q in (([a.ctypes.data], [(16, 16, 2)], 90), ([a.ctypes.data], [(16, 16, 3)], 0), ([a.ctypes.data], [(16, 16, 3)], 101),
                            ([None], [(16, 16, 3)], 90), ([a.ctypes.data], [(0, 16, 3)], 90)):
        rc, _ = be.encode_raw(ptrs, shapes, False, q, out)
        assert rc == _capi.RTD_E_INVALID, (shapes, q)
    assert be.encode([a], False, 90) == [ref.encode(a, 90)]                 # the handle is still good


def test_a_frame_written_on_a_side_stream_just_before_encode_is_the_one_encoded():
    enc = jpeg.JpegEncoder(device=0)
    a, b = scene_frame(7, 720, 1280), scene_frame(8, 720, 1280)
    want = ref.encode(b, 90)
    frame = torch.from_numpy(a).cuda()
    src = torch.from_numpy(b).cuda()
    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            big.fill_(1)                                                    # keeps the side stream busy ahead of the write
        frame.copy_(src)
        got = enc.encode(frame, 90)
    assert got == want
    enc.close()


def test_installed_snapshot_saver_keeps_device_frames_on_the_device():
    mod = stand_in_module()
    jpeg.install(mod)
    saver = mod.SnapshotSaver(maxlen=3)
    z, _ = small_cases()
    names = ["c3_64x48_scene", "c3_250x130_scene", "c3_17x23_noise", "c3_16x16_scene", "c3_7x5_noise"]
    want = [z[f"jpg_{n}_q90"].tobytes() for n in names]
    track = reference_bookkeeping([len(w) for w in want], 3)
    for i, n in enumerate(names):
        saver.add_frame_to_buffer(torch.from_numpy(z["in_" + n]).cuda(), float(i))
        assert saver.buffer_memory_bytes == track[i]
        assert saver.estimated_buffer_memory_mb == track[i] / (1024 * 1024)
    assert [e["frame_compressed"].tobytes() for e in saver.frame_buffer] == want[2:]
    assert [e["timestamp"] for e in saver.frame_buffer] == [2.0, 3.0, 4.0]
    assert saver.original_calls == []
    saver.add_frame_to_buffer(z["in_" + names[0]], 9.0)                     # a numpy frame takes the reference's own path
    assert saver.original_calls == [9.0]


def test_camera_threads_and_an_mjpeg_thread_share_the_process_wide_encoder():
    """one saver for all cameras (the reference's layout) plus imencode from another thread, all through default_encoder: every caller
    gets the file of its own frame"""
    import threading
    mod = stand_in_module()
    jpeg.install(mod)
    cams, per_cam = 6, 10
    saver = mod.SnapshotSaver(maxlen=cams * per_cam)
    frames = {(c, i): scene_frame(300 + 20 * c + i, 120 + 16 * c, 200 + 8 * i) for c in range(cams) for i in range(per_cam)}
    want = {k: ref.encode(f, 90) for k, f in frames.items()}
    big = scene_frame(9, 720, 1280)                                         # larger than the shared output array's first size
    want_big = ref.encode(big, 80)
    dev = {k: torch.from_numpy(f).cuda() for k, f in frames.items()}
    dev_big = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    errors = []
    start = threading.Barrier(cams + 1)

    def camera(c):
        try:
            start.wait()
            for i in range(per_cam):
                saver.add_frame_to_buffer(dev[(c, i)], float(1000 * c + i))
        except Exception as e:                                              # noqa: BLE001 - reported below
            errors.append(repr(e))

    def mjpeg():
        try:
            start.wait()
            for _ in range(per_cam):
                ok, buf = jpeg.imencode(".jpg", dev_big, [jpeg.IMWRITE_JPEG_QUALITY, 80])
                if not ok or buf.tobytes() != want_big:
                    errors.append("imencode returned another frame's bytes")
        except Exception as e:                                              # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=camera, args=(c,)) for c in range(cams)] + [threading.Thread(target=mjpeg)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    assert len(saver.frame_buffer) == cams * per_cam
    for entry in saver.frame_buffer:
        c, i = divmod(int(entry["timestamp"]), 1000)
        assert entry["frame_compressed"].tobytes() == want[(c, i)], (c, i)
