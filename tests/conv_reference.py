"""The conv tests' references on the CPU (torch only, no GPU): the convolution as unfold + matmul on the values the kernel sees, the
epilogue and the 3x3 / stride-2 max-pool - in fp64, or in the dtype asked for."""
import torch
import torch.nn.functional as F

ACT_FN = {"none": lambda t: t, "relu": F.relu, "silu": F.silu, "gelu": F.gelu, "lrelu": lambda t: F.leaky_relu(t, 0.2)}


def conv_ref(xv, wmat, bias, k, pad, x2v=None, stride=1, x_up2=0, dtype=torch.float64):
    """fp64 [B, OH, OW, N]: unfold + matmul.  xv [B, H, W, Cin], wmat [N, k*k*Cin (+ C2)] with tap-major / channel-minor columns.
    x_up2: xv is read through a nearest 2x upsampling (the seen values, repeated).  dtype: the arithmetic (torch.float32: the yardstick
    of tests/conv_range_cases.py)."""
    if x_up2:
        xv = xv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, H, W, Cin = xv.shape
    N = wmat.shape[0]
    if k == 1 and stride == 1:
        cols = xv.reshape(B, H * W, Cin).to(dtype)
        OH, OW = H, W
    else:
        OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        u = F.unfold(xv.permute(0, 3, 1, 2).to(dtype), k, padding=pad, stride=stride)          # [B, Cin * k * k, L], channel-major
        cols = u.reshape(B, Cin, k * k, OH * OW).permute(0, 3, 2, 1).reshape(B, OH * OW, k * k * Cin)
    if x2v is not None:
        cols = torch.cat([cols, x2v.reshape(B, OH * OW, -1).to(dtype)], dim=-1)
    return (cols @ wmat.to(dtype).t() + bias.to(dtype)).reshape(B, OH, OW, N)


def epilogue_ref(y, act, res_mode, rv):
    if res_mode == 1:
        y = y + rv.to(y.dtype)
    y = ACT_FN[act](y)
    if res_mode == 2:
        y = y + rv.to(y.dtype)
    return y


def pooled_ref(y):
    """3x3 / stride 2 / pad 1 max of fp64 [B, H, W, C]."""
    return F.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
