"""tests/frontend_ref.py held to torch before a kernel is held to it (no GPU): stem0_ref against F.conv2d in fp64, and the tap-map words
against stem0_ref with the tap-map filter - channel order, tap order and padding of both references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from telescope_cam_detection_amd import _capi
from tests import frontend_ref as ref
from tests.frontend_ref import SHAPES, operands


@pytest.mark.parametrize("n,H,W", SHAPES)
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_stem0_ref_agrees_with_conv2d_on_the_unrounded_operands(n, H, W, act):
    """stem0_ref rounds pixels and filter to pairs; conv2d(stride 2, padding 1) in fp64 takes float32(v) / float32(255) and the fp32 filter
    as they are, channels swapped BGR -> RGB by hand.  Elementwise bound 2^-20 sum |x| |w| on the pre-activation sum: the pair rounding of
    an operand is <= 2^-22 relative (+ 2^-25 absolute where lo is an fp16 subnormal: operands below 1/8, which the slack of the other
    taps of a uniform random frame covers), <= 2^-21 per product, 2 x margin; ReLU and SiLU have slope <= 1.1, inside that margin.  The
    1e3 in the filter's pad channels would show at once."""
    frames, w, bias = operands(n, H, W)
    got = ref.stem0_ref(frames, w, bias, _capi.ACT[act])
    x = torch.from_numpy(np.stack(frames).astype(np.float32) / np.float32(255.0)).double()      # [n, H, W, bgr]
    x = x.flip(-1).permute(0, 3, 1, 2)                                                           # [n, rgb, H, W]
    wt = torch.from_numpy(w[:, :, :, :3]).double().permute(0, 3, 1, 2)                           # [32, rgb, kh, kw]
    pre = F.conv2d(x, wt, torch.from_numpy(bias).double(), stride=2, padding=1)
    want = {"none": lambda t: t, "relu": F.relu, "silu": F.silu}[act](pre).permute(0, 2, 3, 1).numpy()
    bound = 2.0 ** -20 * F.conv2d(x.abs(), wt.abs(), None, stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    assert got.shape == want.shape == (n, ref.out_extent(H), ref.out_extent(W), 32)
    err = np.abs(got - want)
    print(f"stem0_ref vs conv2d {n}x{H}x{W} {act}: worst err / bound {np.max(err / bound):.3f}, max |y| {np.abs(want).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_tap_map_words_are_the_values_of_stem0_ref_with_the_tap_map_filter(n, H, W):
    """two independent walks over taps and channels (a shifted copy; a strided-window product with a 0 / 1 filter) give equal values"""
    frames, _, _ = operands(n, H, W)
    w, bias = ref.tap_map_filter()
    assert w.sum() == 27 and (w[27:] == 0).all() and (w[:, :, :, 3:] == 0).all() and (bias == 0).all()
    words = ref.tap_map_words(frames)
    assert words.dtype == np.uint16 and words.shape == (n, ref.out_extent(H), ref.out_extent(W), 64)
    want = ref.stem0_ref(frames, w, bias, _capi.ACT["none"])
    np.testing.assert_array_equal(_capi.from_split(words).astype(np.float64), want)
    assert (words[..., 27:32] == 0).all() and (words[..., 59:64] == 0).all()
    # and the map is not trivially empty: the centre tap of output (0, 0) is pixel (0, 0), RGB
    px = ref.pixels_seen(frames[0])[0, 0]
    np.testing.assert_array_equal(_capi.from_split(words)[0, 0, 0, 12:15], px)
    assert (_capi.from_split(words)[0, 0, 0, 0:9] == 0).all()                                  # taps of row -1: padding
