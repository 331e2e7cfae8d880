"""Shared by test_conv3x3_dilated_cpu.py and test_conv3x3_dilated_gpu.py: the dilated flavour of alo_conv3x3_nhwc (ALO_CONV_DILATION_2
in ``stride``: 3x3, stride 1, dilation 2, zero padding 2; aloception-oss_amd/csrc/conv.hip and conv_f32.hip), its fp64 references and
the per-element bounds the kernels and the numpy restatement are held to.

Only the window changes against the undilated kernels: the nine taps sit at offsets {-2, 0, 2}^2, K = 9 Cin products as before, so both
bounds are the undilated ones over that window.

  bf16 (test_backbone_kernels_gpu.py, module docstring):   |y - ref| <= 2^-8 |ref| + c_acc(9 Cin) A
  fp32 (conv_f32_ref.py, module docstring):                |y - ref| <= c_acc(9 Cin) S + 2^-20 S + 2^-38 (amax_image sum|w| + wmax_row sum|x|) + 2^-24 |ref|

A = S = the same convolution of |x|, |w| and |b| (non-finite inputs as 0), the sums over the taps that lie inside the image.  The
reference is F.conv2d(x.double(), w.double(), b.double(), 1, 2, 2) on the kernel's own operands.
"""
import numpy as np
import torch
import torch.nn.functional as F

from kernel_bounds import _finite_abs, c_acc
from split_f16_ref import finite_amax, split_exponent, split_terms

OFFSETS = (-2, 0, 2)    # a tap's row / column offset, in the order of the weight's ky / kx


def windows(x):
    """(N, H, W, C) -> (N, H, W, 9 C): the 3x3 / dilation 2 / padding 2 windows, zero outside, k = (ky * 3 + kx) * C + c."""
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 4, w + 4, c), dtype=x.dtype)
    xp[:, 2:2 + h, 2:2 + w] = x
    return np.concatenate([xp[:, 2 * ky:2 * ky + h, 2 * kx:2 * kx + w] for ky in range(3) for kx in range(3)], axis=-1)


def conv3x3_dilated_split(x, w, b, relu):
    """The fp32 kernel's arithmetic (conv_f32_ref.conv3x3_split over the dilated window).  x (N, H, W, Cin), w (Cout, 3, 3, Cin),
    b (Cout,) or None, all fp32 -> (N, H, W, Cout) fp32."""
    cout = w.shape[0]
    rows = w.reshape(cout, -1)
    kc = np.array([split_exponent(finite_amax(r)) for r in rows], dtype=np.int32)
    w_hi, w_lo = split_terms(rows, kc[:, None])
    out = []
    for img in x:
        k = split_exponent(finite_amax(img))
        x_hi, x_lo = (windows(t[None])[0] for t in split_terms(img, k))
        acc = (x_hi @ w_lo.T + x_lo @ w_hi.T) + x_hi @ w_hi.T          # small terms first, fp32 throughout
        y = np.ldexp(acc, k + kc).astype(np.float32)
        if b is not None:
            y = y + b
        out.append(np.where(y > 0, y, np.where(np.isnan(y), y, np.float32(0))) if relu else y)
    return np.stack(out).astype(np.float32)


def reference_parts(x, w):
    """What the references and bounds need of x (N, Cin, H, W) and w (Cout, Cin, 3, 3) (any float dtype, any device, any memory format),
    without bias or activation, to be shared among cases: (conv(x, w), conv(|x|, |w|), sum |w| and sum |x| over the taps that exist,
    amax per image, wmax per channel), fp64."""
    x64, w64 = x.double(), w.double()
    xa, wa = _finite_abs(x), _finite_abs(w)
    sum_w = F.conv2d(torch.ones_like(xa[:1]), wa, None, 1, 2, 2)
    sum_x = F.conv2d(xa, torch.ones_like(wa[:1]), None, 1, 2, 2)
    amax = xa.flatten(1).amax(1).view(-1, 1, 1, 1)
    wmax = wa.flatten(1).amax(1).view(1, -1, 1, 1)
    return F.conv2d(x64, w64, None, 1, 2, 2), F.conv2d(xa, wa, None, 1, 2, 2), sum_w, sum_x, amax, wmax


def reference_and_bound(x, w, b, relu, parts=None):
    """-> (ref, bound), fp64 (N, Cout, H, W), for the dtype of ``x``: torch.bfloat16 or torch.float32 (module docstring).
    ``parts``: :func:`reference_parts` of the same x and w."""
    ref, s, sum_w, sum_x, amax, wmax = reference_parts(x, w) if parts is None else parts
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1)
        s = s + b.double().abs().view(1, -1, 1, 1)
    if relu:
        ref = torch.relu(ref)
    mag = torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0)
    c = c_acc(9 * x.shape[1])
    if x.dtype == torch.bfloat16:
        return ref, 2.0 ** -8 * mag + c * s
    assert x.dtype == torch.float32, x.dtype
    return ref, (c + 2.0 ** -20) * s + 2.0 ** -38 * (amax * sum_w + wmax * sum_x) + 2.0 ** -24 * mag
