"""GPU: the fused uint8 stem (csrc/ops.hip stem0_u8_kernel) at kernel level through rtd_op_stem0_u8, and device frames at any byte
address.  The kernel loads aligned dwords from a byte-granular patch origin that can be negative, falls back to bytes when the frame
base is not 4-byte aligned or a dword leaves the frame, zero-pads by coordinate while the dword holds the neighbouring row's bytes, and
gathers a permuted K (k = 10 kh + 3 kw + byte, BGR -> RGB folded into the filter index).  Held to tests/frontend_ref.py: fp64 on the
values the kernel sees (A), bits independent of address and surroundings (B), a 0 / 1 filter whose output words are known exactly (C),
refusals (D), and the two engines' device-frame paths on views into a shared buffer (E).

Every frame lives in ONE uint8 device buffer with >= 4 KiB of filler before and after it and starts `off` bytes past a 16-byte boundary:
a stray read neither faults nor goes unseen (B compares filler 0x00 with 0xFF).  Outputs are tests/test_gpu_conv_instances.py Guarded
buffers: NaN prefill, sentinel guard bands."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from telescope_cam_detection_amd import _capi
from tests import frontend_ref as ref
from tests.frontend_ref import SHAPES, Placed, operands
from tests.test_gpu_conv_instances import Guarded, assert_pair_bound

pytestmark = pytest.mark.gpu

ACT = _capi.ACT
ids = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _capi.lib()


def mixed(off, n):
    """frame i of a call at offset (off + i) % 4: different offsets in one call"""
    return [(off + i) % 4 for i in range(n)]


@functools.lru_cache(maxsize=None)
def case(shape):
    frames, w, bias = operands(*shape)
    return frames, w, bias, torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda()


@functools.lru_cache(maxsize=None)
def reference(shape, act):
    frames, w, bias = operands(*shape)
    want = torch.from_numpy(ref.stem0_ref(frames, w, bias, ACT[act]))
    assert want.abs().max().item() > 0.1
    return want


def stem0(L, ptrs, n, H, W, wd, bd, out, act):
    table = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    return L.rtd_op_stem0_u8(table, n, H, W, wd.data_ptr(), bd.data_ptr(), out.ptr(), act)


def run(L, shape, offs, fill, act, wd=None, bd=None):
    """one launch on freshly placed frames -> the Guarded output (status checked)"""
    n, H, W = shape
    frames, _, _, wd0, bd0 = case(shape)
    placed = Placed(frames, offs, fill)
    out = Guarded("pair", n, ref.out_extent(H), ref.out_extent(W), 32)
    rc = stem0(L, placed.ptrs, n, H, W, wd if wd is not None else wd0, bd if bd is not None else bd0, out, act)
    assert rc == 0, (rc, L.rtd_last_error(None))
    return out


@pytest.mark.parametrize("shape,act", [(s, a) for s in SHAPES for a in ("none", "relu")] + [((2, 17, 67), "silu")],
                         ids=lambda v: v if isinstance(v, str) else ids(v))
def test_stem0_u8_against_fp64_at_every_alignment(L, shape, act):
    """A. random filter (1e3 in the pad channels 3..7: they must never reach the result), every frame offset 0..3 (mixed within a call for
    n > 1), against fp64 at the project's pair bound; every element written, no guard touched, ragged tiles included."""
    want = reference(shape, act)
    for off in range(4):
        out = run(L, shape, mixed(off, shape[0]), 0xFF, ACT[act])
        assert_pair_bound(out.values(), want, f"stem0_u8 {ids(shape)} {act} off {off}")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_stem0_u8_bits_do_not_depend_on_address_or_surroundings(L, shape):
    """B. eight launches per shape - offsets 0..3 x filler 0x00 / 0xFF - give the same output bits."""
    first = None
    for fill in (0x00, 0xFF):
        for off in range(4):
            out = run(L, shape, mixed(off, shape[0]), fill, ACT["relu"])
            out.values()
            if first is None:
                first = out.bits()
            np.testing.assert_array_equal(out.bits(), first, err_msg=f"{ids(shape)} off {off} filler {fill:#x}")


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("shape", [(1, 16, 64), (2, 17, 67), (1, 3, 5)], ids=ids)
def test_stem0_u8_tap_map_bit_for_bit(L, shape, off):
    """C. the 0 / 1 filter that copies tap c // 3, RGB channel c % 3 into output channel c: the words are tests/frontend_ref.py
    tap_map_words exactly (tap order, channel swap, zero padding and the byte each lane gathers), channels 27..31 zero words."""
    w, bias = ref.tap_map_filter()
    out = run(L, shape, mixed(off, shape[0]), 0xFF, ACT["none"], torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda())
    out.values()
    got = out.bits().view(np.uint16)
    np.testing.assert_array_equal(got, ref.tap_map_words(case(shape)[0]))
    assert (got[..., 27:32] == 0).all() and (got[..., 59:64] == 0).all()


@pytest.mark.parametrize("why,n,act", [("act = 3", 1, 3), ("n = 0", 0, 1), ("n = 65", 65, 1)])
def test_stem0_u8_refusals_write_nothing(L, why, n, act):
    """D. RTD_E_INVALID before any launch; the output keeps its prefill and its guards."""
    shape = (1, 16, 64)
    _, _, _, wd, bd = case(shape)
    placed = Placed(case(shape)[0], [0], 0xFF)
    out = Guarded("pair", max(n, 1), 8, 32, 32)
    rc = stem0(L, placed.ptrs * max(n, 1), n, 16, 64, wd, bd, out, act)
    assert rc == _capi.RTD_E_INVALID, (why, rc, L.rtd_last_error(None))
    torch.cuda.synchronize()
    assert out.untouched(), why


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_engine_reads_device_frames_at_any_byte_address(precision):
    """E. tinyc at (160, 224), batch 2, hipGraph: infer_raw on device frames that are allocations of their own, then contiguous views at
    byte offsets (1, 3) and (2, 0) past 16-byte boundaries of one 0xFF-filled buffer: final rows and the first stage tensor bit for bit.
    f16x3 takes the fused uint8 stem (asserted from the plan: backbone.stem.0 moves n H W 3 bytes in + its output), bf16 the identity
    pre-process kernel."""
    from telescope_cam_detection_amd.arch import ARCHS
    from telescope_cam_detection_amd.synth import scene_frame
    from telescope_cam_detection_amd.weights import fold_weights, pack_blob, synth_weights

    arch, (H, W), n = ARCHS["tinyc"], (160, 224), 2
    assert arch.embedding_size == 64
    blob = pack_blob(fold_weights(arch, synth_weights(arch, 3)))
    frames = [scene_frame(80 + i, H, W) for i in range(n)]
    stage = "stem" if precision == "f16x3" else "input"
    eng = _capi.Engine(arch, blob, 0, _capi.precision_code(precision), n, (H, W), True)
    try:
        own = [torch.from_numpy(f).cuda() for f in frames]
        torch.cuda.synchronize()
        want = eng.infer_raw(own, on_device=True)
        want_stage = eng.debug_tensor(stage)
        assert np.isfinite(want_stage).all() and np.abs(want_stage).max() > 0.1
        for offs in ((1, 3), (2, 0)):
            placed = Placed(frames, offs, 0xFF)
            assert [p % 16 for p in placed.ptrs] == list(offs)
            got = eng.infer_raw(placed.views, on_device=True)
            np.testing.assert_array_equal(eng.debug_tensor(stage), want_stage, err_msg=f"{precision} {stage} at offsets {offs}")
            for g, w_, what in zip(got, want, ("labels", "boxes", "scores")):
                np.testing.assert_array_equal(g, w_, err_msg=f"{precision} {what} at offsets {offs}")
        stem = [p for p in eng.profile(n, 1) if p["name"] == "backbone.stem.0"]
        assert len(stem) == 1
        fused_bytes = n * H * W * 3 + n * (H // 2) * (W // 2) * 32 * 4
        assert (stem[0]["bytes"] == fused_bytes) == (precision == "f16x3"), (stem[0], fused_bytes)
    finally:
        eng.close()
