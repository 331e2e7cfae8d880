"""Shared by test_conv_taps_f32_cpu.py and test_conv_taps_f32_gpu.py: the five-tap flavours of aloception-oss_amd/csrc/conv_f32.hip
(1x5 with zero padding (0, 2), 5x1 with zero padding (2, 0), stride 1) restated in numpy, and the fp64 reference with the per-element
bound that both the restatement (CPU) and the kernel (GPU) are held to.

The arithmetic is conv3x3_f32_kernel's (conv_f32_ref.py) over another window: one power of two per image and per output channel, the
two-term split of both operands, w_lo x_hi + w_hi x_lo first and w_hi x_hi last into fp32, the scales undone by ldexp, + bias, ReLU.
The bound is that module's, derived there, with the K = 5 Cin products of a five-tap window in place of the 9 Cin of a 3x3 one:

  |y - ref| <= c_acc(5 Cin) S + 2^-20 S + 2^-38 (amax_image sum|w| + wmax_row sum|x|) + 2^-24 |ref|

S = sum |x_k| |w_k| + |b| over the window, the sums over the taps that lie inside the image.
"""
import numpy as np
import torch
import torch.nn.functional as F

from kernel_bounds import c_acc
from split_f16_ref import finite_amax, split_exponent, split_terms

PADDING = {False: (0, 2), True: (2, 0)}     # vertical -> F.conv2d's padding


def windows(x, vertical):
    """(N, H, W, C) -> (N, H, W, 5 C): the five-tap windows along x (1x5) or along y (5x1), zero outside, k = t * C + c."""
    n, h, w, c = x.shape
    py, px = PADDING[vertical]
    xp = np.zeros((n, h + 2 * py, w + 2 * px, c), dtype=x.dtype)
    xp[:, py:py + h, px:px + w] = x
    taps = [xp[:, t:t + h, :] if vertical else xp[:, :, t:t + w] for t in range(5)]
    return np.concatenate(taps, axis=-1)


def conv_taps_split(x, w, b, vertical, relu):
    """The kernel's arithmetic.  x (N, H, W, Cin), w (Cout, 5, Cin) tap-major, b (Cout,) or None, all fp32 -> (N, H, W, Cout) fp32."""
    cout = w.shape[0]
    rows = w.reshape(cout, -1)
    kc = np.array([split_exponent(finite_amax(r)) for r in rows], dtype=np.int32)
    w_hi, w_lo = split_terms(rows, kc[:, None])
    out = []
    for img in x:
        k = split_exponent(finite_amax(img))
        x_hi, x_lo = (windows(t[None], vertical)[0] for t in split_terms(img, k))
        acc = (x_hi @ w_lo.T + x_lo @ w_hi.T) + x_hi @ w_hi.T          # small terms first, fp32 throughout
        y = np.ldexp(acc, k + kc).astype(np.float32)
        if b is not None:
            y = y + b
        out.append(np.where(y > 0, y, np.where(np.isnan(y), y, np.float32(0))) if relu else y)
    return np.stack(out).astype(np.float32)


def weight_4d(w, vertical):
    """(Cout, 5, Cin) tap-major -> the (Cout, Cin, 5, 1) or (Cout, Cin, 1, 5) weight of F.conv2d."""
    w = torch.as_tensor(w).permute(0, 2, 1)
    return (w[:, :, :, None] if vertical else w[:, :, None, :]).contiguous()


def reference_parts(x, w):
    """The convolutions of :func:`reference_and_bound` that do not depend on the bias or the activation, for tests that share them
    among cases: (conv(x, w), conv(|x|, |w|), sum |w| and sum |x| over the taps that exist, amax per image, wmax per channel), fp64."""
    pad = PADDING[w.shape[2] == 5]
    assert tuple(w.shape[2:]) in ((1, 5), (5, 1))
    x64, w64 = x.double(), w.double()
    xa = torch.nan_to_num(x64.abs(), nan=0.0, posinf=0.0)
    wa = torch.nan_to_num(w64.abs(), nan=0.0, posinf=0.0)
    sum_w = F.conv2d(torch.ones_like(xa[:1]), wa, None, 1, pad)
    sum_x = F.conv2d(xa, torch.ones_like(wa[:1]), None, 1, pad)
    amax = xa.flatten(1).amax(1).view(-1, 1, 1, 1)
    wmax = wa.flatten(1).amax(1).view(1, -1, 1, 1)
    return F.conv2d(x64, w64, None, 1, pad), F.conv2d(xa, wa, None, 1, pad), sum_w, sum_x, amax, wmax


def reference_and_bound(x, w, b, relu, parts=None):
    """x (N, Cin, H, W), w (Cout, Cin, 1, 5) or (Cout, Cin, 5, 1), b (Cout,) or None: fp32 CPU tensors (any memory format).
    -> (ref, bound), fp64 (N, Cout, H, W): F.conv2d in fp64 on the same operands, and the bound of the module docstring.
    ``parts``: :func:`reference_parts` of the same x and w."""
    ref, s, sum_w, sum_x, amax, wmax = reference_parts(x, w) if parts is None else parts
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1)
        s = s + b.double().abs().view(1, -1, 1, 1)
    if relu:
        ref = torch.relu(ref)
    bound = (c_acc(5 * x.shape[1]) + 2.0 ** -20) * s + 2.0 ** -38 * (amax * sum_w + wmax * sum_x) + 2.0 ** -24 * torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0)
    return ref, bound
