"""Shared by test_conv3x3_f32_cpu.py and test_conv3x3_f32_gpu.py: the arithmetic of aloception-oss_amd/csrc/conv_f32.hip restated in
numpy, and the fp64 reference with the per-element bound that both the restatement (CPU) and the kernel (GPU) are held to.

The bound.  y = act(sum_k x_k w_k + b) over the K = 9 Cin products of a window; S = sum |x_k| |w_k| + |b|.
  * The kernel divides an image by 2^k (its largest finite magnitude amax lands in [2^14, 2^15)) and output channel o's weights by
    2^k_o (wmax_o likewise): exact.  Each scaled operand u is split into hi = fp16(u), lo = fp16(u - hi), both round to nearest:
    |u - hi| <= 2^-11 |u| (exact in fp32), and lo keeps 11 bits of that unless it is subnormal in fp16, where it is stored to within
    half a subnormal step, 2^-25: |u - hi - lo| <= 2^-22 |u| + 2^-25, and 2^-25 <= 2^-39 of the largest scaled magnitude (>= 2^14).
  * The three products hi hi + hi lo + lo hi are exact in fp32 (11 x 11 bits); the dropped lo lo is <= 2^-22 |x w|.  Per product the
    result is off by  2^-22 |x w| (x's split) + 2^-22 |x w| (w's) + 2^-22 |x w| (lo lo) <= 2^-20 |x w|  plus the subnormal floors
    2^-39 amax |w| + 2^-39 wmax_o |x| (+ second-order terms): summed over the window, 2^-20 S + 2^-38 (amax sum |w| + wmax_o sum |x|)
    with a factor 2 of room on the floor.
  * Accumulation in fp32.  c_acc(K) S = (K + 1) 2^-23 S (kernel_bounds.c_acc) is what a K-term fp32 dot product plus its bias is
    allowed anywhere in this suite: twice the worst case (K 2^-24 S) of K roundings of partial sums.  Here the partial sums are
    rounded once per MFMA, each of which adds 16 products: 3 K / 16 instructions (three per 16 channels of a tap), of which two
    thirds add terms 2^-11 as large; the numpy restatement adds three BLAS products.  Both stay inside c_acc(9 Cin) S, the bias
    addition included.  Undoing the scales is exact (ldexp); the result is rounded once more: 2^-24 |ref|.

  |y - ref| <= c_acc(9 Cin) S + 2^-20 S + 2^-38 (amax_image sum|w| + wmax_row sum|x|) + 2^-24 |ref|

ReLU is 1-Lipschitz, so the bound carries over.  Non-finite inputs take no part in amax or in the sums; the outputs whose window holds
one are compared for kind (kernel_bounds.compare), not for value.
"""
import numpy as np
import torch
import torch.nn.functional as F

from kernel_bounds import c_acc
from split_f16_ref import finite_amax, split_exponent, split_terms  # noqa: F401  (re-exported)


def windows(x, stride):
    """(N, H, W, C) -> (N, Ho, Wo, 9 C): the 3x3 / padding 1 windows, k = (ky * 3 + kx) * C + c."""
    n, h, w, c = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    xp = np.zeros((n, h + 2, w + 2, c), dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    taps = [xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]
    return np.concatenate(taps, axis=-1)


def conv3x3_split(x, w, b, stride, relu):
    """The kernel's arithmetic.  x (N, H, W, Cin), w (Cout, 3, 3, Cin), b (Cout,) or None, all fp32 -> (N, Ho, Wo, Cout) fp32."""
    cout = w.shape[0]
    rows = w.reshape(cout, -1)
    kc = np.array([split_exponent(finite_amax(r)) for r in rows], dtype=np.int32)
    w_hi, w_lo = split_terms(rows, kc[:, None])
    out = []
    for img in x:
        k = split_exponent(finite_amax(img))
        x_hi, x_lo = (windows(t[None], stride)[0] for t in split_terms(img, k))
        acc = (x_hi @ w_lo.T + x_lo @ w_hi.T) + x_hi @ w_hi.T          # small terms first, fp32 throughout
        y = np.ldexp(acc, k + kc).astype(np.float32)
        if b is not None:
            y = y + b
        out.append(np.where(y > 0, y, np.where(np.isnan(y), y, np.float32(0))) if relu else y)
    return np.stack(out).astype(np.float32)


def reference_and_bound(x, w, b, stride, relu):
    """x (N, Cin, H, W), w (Cout, Cin, 3, 3), b (Cout,) or None: fp32 CPU tensors (any memory format).
    -> (ref, bound), fp64 (N, Cout, Ho, Wo): F.conv2d in fp64 on the same operands, and the bound of the module docstring."""
    x64, w64 = x.double(), w.double()
    b64 = None if b is None else b.double()
    ref = F.conv2d(x64, w64, b64, stride, 1)
    xa = torch.nan_to_num(x64.abs(), nan=0.0, posinf=0.0)
    wa = torch.nan_to_num(w64.abs(), nan=0.0, posinf=0.0)
    s = F.conv2d(xa, wa, None if b is None else b64.abs(), stride, 1)
    sum_w = F.conv2d(torch.ones_like(xa[:1]), wa, None, stride, 1)                   # over the taps that exist
    sum_x = F.conv2d(xa, torch.ones_like(wa[:1]), None, stride, 1)
    amax = xa.flatten(1).amax(1).view(-1, 1, 1, 1)
    wmax = wa.flatten(1).amax(1).view(1, -1, 1, 1)
    cin = x.shape[1]
    if relu:
        ref = torch.relu(ref)
    bound = (c_acc(9 * cin) + 2.0 ** -20) * s + 2.0 ** -38 * (amax * sum_w + wmax * sum_x) + 2.0 ** -24 * torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0)
    return ref, bound
