"""Shared by test_linear_f32_cpu.py and test_linear_f32_gpu.py: the arithmetic of aloception-oss_amd/csrc/gemm_f32.hip restated in
numpy, and the fp64 reference with the per-element bound that both the restatement (CPU) and the kernel (GPU) are held to.

The bound is conv_f32_ref.py's (read its derivation first) with K for 9 Cin and the ROW's largest finite magnitude for the image's:
y = act(sum_k x_k w_k + b [+ res]);  S = sum_k |x_k| |w_k| + |b|,  pre = sum_k x_k w_k + b,  ref = act(pre [+ res]).

  |y - ref| <= (c_acc(K) + 2^-20) S + 2^-38 (amax_row sum_k |w_ok| + wmax_o sum_k |x_k|) + 2^-24 |pre| [+ 2^-24 |pre + res|]

  * c_acc(K) S: the fp32 accumulation (3 K / 16 MFMAs of 16 products each, the K-split's one extra addition at N = 64) and the bias.
  * 2^-20 S and the 2^-38 floor: the two-term splits of a row (one power of two per row of x) and of a channel's weights, and the
    dropped lo lo product.
  * 2^-24 |pre|: undoing the scales is exact, adding the bias rounds once.  With a residual the sum pre + res is formed in fp32 from
    the rounded pre: one more rounding, 2^-24 |pre + res|.
ReLU is 1-Lipschitz, so the bound carries over.  Non-finite inputs take no part in amax or in the sums; the outputs of a row that
holds one are compared for kind (kernel_bounds.compare), not for value.
"""
import numpy as np
import torch

from kernel_bounds import c_acc
from split_f16_ref import row_exponents, split_terms, split_weight


def linear_split(x, w, b=None, res=None, relu=False):
    """The kernel's arithmetic.  x (M, K), w (N, K), b (N,) or None, res (M, N) or None, all fp32 -> (M, N) fp32."""
    w_hi, w_lo, kc = split_weight(w)
    kr = row_exponents(x)
    x_hi, x_lo = split_terms(x, kr[:, None])
    with np.errstate(over="ignore", invalid="ignore"):
        acc = (x_hi @ w_lo.T + x_lo @ w_hi.T) + x_hi @ w_hi.T           # small terms first, fp32 throughout
        y = np.ldexp(acc, kr[:, None] + kc[None, :]).astype(np.float32)
        if b is not None:
            y = y + b
        if res is not None:
            y = (y + res).astype(np.float32)
    return (np.where(y > 0, y, np.where(np.isnan(y), y, np.float32(0))) if relu else y).astype(np.float32)


def reference_and_bound(x, w, b=None, res=None, relu=False):
    """x (M, K), w (N, K), b (N,) or None, res (M, N) or None: fp32 CPU tensors.  -> (ref, bound), fp64 (M, N)."""
    fin = lambda a: torch.nan_to_num(a.abs(), nan=0.0, posinf=0.0)  # noqa: E731
    x64, w64 = x.double(), w.double()
    pre = x64 @ w64.t()
    xa, wa = fin(x64), fin(w64)
    s = xa @ wa.t()
    if b is not None:
        pre = pre + b.double()
        s = s + b.double().abs()
    k = x.shape[1]
    bound = ((c_acc(k) + 2.0 ** -20) * s
             + 2.0 ** -38 * (xa.amax(1, keepdim=True) * wa.sum(1)[None, :] + wa.amax(1)[None, :] * xa.sum(1, keepdim=True))
             + 2.0 ** -24 * fin(pre))
    ref = pre
    if res is not None:
        ref = pre + res.double()
        bound = bound + 2.0 ** -24 * fin(ref)
    return (torch.relu(ref) if relu else ref), bound


# (M, K, N): where the kernel can go wrong
SHAPES = [
    (1, 64, 64),            # one row; N = 64: the two waves split K
    (63, 64, 128),          # ragged tiles either side of 64
    (65, 128, 64),
    (130, 192, 192),        # odd multiples of 64; a column block whose second wave is idle
    (200, 256, 320),
    (77, 2048, 256),        # long K
    (300, 1024, 2048),      # many column blocks
    (66000, 64, 64),        # a workgroup walks a second tile
    (70001, 128, 192),
]
SCALES = [1e-20, 1.0, 3e4, 5e18]


def operands(shape, scale=1.0):
    """x (M, K) at ``scale``, w (N, K) at 1 / sqrt(K), b (N,) and res (M, N) at ``scale``: fp32 CPU tensors from a seed of the shape."""
    m, k, n = shape
    g = torch.Generator().manual_seed(m * 7 + k * 3 + n)
    x = torch.randn(m, k, generator=g) * scale
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g) * scale
    res = torch.randn(m, n, generator=g) * scale
    return x, w, b, res
