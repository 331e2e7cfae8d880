"""Shared by test_stem_f32_cpu.py and test_stem_f32_gpu.py: the arithmetic of aloception-oss_amd/csrc/stem_f32.hip restated in numpy,
and the fp64 reference with the per-element bound that both the restatement (CPU) and the kernel (GPU) are held to.

The frame.  A workgroup makes 8 x 7 pooled pixels (tile (ty, tx) of an image: pooled rows 8 ty .., columns 7 tx ..) from the 17 x 15
convolution outputs behind them, which read a WINDOW of 39 rows x 35 pixels x 3 channels of the image: rows 32 ty - 5 .. + 38, columns
28 tx - 5 .. + 34, zero outside the image.  The window is divided by one power of two 2^k, from its largest finite magnitude; a pooled
pixel belongs to one tile, so everything behind it was computed at that tile's scale — neighbouring tiles compute the convolution
outputs they share twice, each at its own scale.

The bound, in the manner of conv_f32_ref.py (whose derivation of the split's error is not repeated here).  A convolution output is
c = relu(sum_k x_k w_k + b) over K = 147 products; S = sum |x_k| |w_k| + |b|; amax = the largest finite magnitude of the window,
wmax_o = the largest of output channel o's weights.
  * scales: exact.  The split of both operands and the dropped lo lo product: 2^-20 S, plus the floor of low terms that are subnormal
    in fp16, 2^-38 (amax sum |w| + wmax_o sum |x|) with conv_f32_ref.py's factor 2 of room; sum |w| <= 147 wmax_o and
    sum |x| <= 147 amax, so the floor is at most 2^-37 * 147 amax wmax_o.  This is the term that knows the window: a pixel 10^6
    times dimmer than the brightest one of its window keeps an ABSOLUTE error of that size.
  * accumulation in fp32: c_acc(147) S (kernel_bounds.c_acc), 11 k-steps of three MFMAs; the 29 zero columns of the (64, 176)
    matrix add nothing.  The undo is exact (ldexp), the bias is added in fp32: one more rounding, 2^-24 |c|.
  * ReLU and the max over the 3 x 3 pooling window are 1-Lipschitz in every argument and exact in fp32: the pooled pixel's bound is the
    largest bound of the convolution outputs it reads.

  |c - ref_c| <= (c_acc(147) + 2^-20) S + 2^-37 * 147 amax_window wmax_o + 2^-24 |ref_c|;   |y - ref| <= max over the 3 x 3 of that

Non-finite pixels take no part in amax or in the sums; the outputs that hold one are compared for kind (kernel_bounds.compare).
"""
import numpy as np
import torch
import torch.nn.functional as F

from kernel_bounds import c_acc
from split_f16_ref import finite_amax, split_exponent, split_terms, split_weight

POOL_ROWS, POOL_COLS = 8, 7            # pooled pixels per tile
CONV_ROWS, CONV_COLS = 17, 15          # convolution outputs behind them
WIN_ROWS, WIN_COLS = 39, 35            # input pixels behind those
K = 147


def out_sizes(h, w):
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return hc, wc, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1


def tiles(h, w):
    _, _, hp, wp = out_sizes(h, w)
    return -(-hp // POOL_ROWS), -(-wp // POOL_COLS)


def stem_matrix(w):
    """(64, 3, 7, 7) -> the (64, 176) matrix of alo_stem_conv_pool: m[o][ky * 24 + kx * 3 + c] = w[o][c][ky][kx], zero elsewhere."""
    m = np.zeros((64, 8, 24), dtype=w.dtype)
    m[:, :7, :21] = w.transpose(0, 2, 3, 1).reshape(64, 7, 21)
    return np.ascontiguousarray(m.reshape(64, 192)[:, :176])


def windows(img):
    """(3, H, W) -> (tiles_y, tiles_x, 39, 35, 3): every tile's window, zero outside the image."""
    _, h, w = img.shape
    ty, tx = tiles(h, w)
    padded = np.zeros((32 * ty + WIN_ROWS, 28 * tx + WIN_COLS, 3), dtype=img.dtype)     # pixel (0, 0) at (5, 5)
    padded[5:5 + h, 5:5 + w] = img.transpose(1, 2, 0)
    return np.stack([np.stack([padded[32 * i:32 * i + WIN_ROWS, 28 * j:28 * j + WIN_COLS] for j in range(tx)]) for i in range(ty)])


def window_amax(x):
    """(N, 3, H, W) fp32 -> (N, Hp, Wp) fp64: the largest finite magnitude of the window behind each pooled pixel."""
    _, _, hp, wp = out_sizes(*x.shape[2:])
    out = []
    for img in x:
        win = windows(img)
        mag = np.where(np.isfinite(win), np.abs(win), 0).max(axis=(2, 3, 4)).astype(np.float64)
        out.append(np.repeat(np.repeat(mag, POOL_ROWS, 0), POOL_COLS, 1)[:hp, :wp])
    return np.stack(out)


def _relu_keep_nan(y):
    return np.where(y > 0, y, np.where(np.isnan(y), y, np.float32(0)))


def stem_split(x, w, b):
    """The kernel's arithmetic.  x (N, 3, H, W), w (64, 3, 7, 7), b (64,) or None, all fp32 numpy -> (N, 64, Hp, Wp) fp32."""
    n, _, h, wd = x.shape
    hc, wc, hp, wp = out_sizes(h, wd)
    rows = w.transpose(0, 2, 3, 1).reshape(64, K)                         # k = (ky * 7 + kx) * 3 + c
    w_hi, w_lo, kc = split_weight(rows)
    out = np.zeros((n, hp, wp, 64), dtype=np.float32)
    for i, img in enumerate(x):
        win = windows(img)
        for ty in range(win.shape[0]):
            for tx in range(win.shape[1]):
                k = split_exponent(np.float32(finite_amax(win[ty, tx])))
                hi, lo = split_terms(win[ty, tx], k)
                # convolution output (r, c) of the tile reads window rows 2 r .. + 6, columns 2 c .. + 6
                cols = [np.concatenate([t[ky:ky + 2 * CONV_ROWS - 1:2, kx:kx + 2 * CONV_COLS - 1:2] for ky in range(7) for kx in range(7)],
                                       axis=-1).reshape(-1, K) for t in (hi, lo)]
                with np.errstate(over="ignore", invalid="ignore"):
                    acc = (cols[0] @ w_lo.T + cols[1] @ w_hi.T) + cols[0] @ w_hi.T      # small terms first, fp32 throughout
                    y = np.ldexp(acc, k + kc).astype(np.float32)
                    if b is not None:
                        y = y + b
                y = _relu_keep_nan(y).reshape(CONV_ROWS, CONV_COLS, 64)
                # convolution outputs outside the map are the pool's padding
                cy = 2 * POOL_ROWS * ty - 1 + np.arange(CONV_ROWS)
                cx = 2 * POOL_COLS * tx - 1 + np.arange(CONV_COLS)
                inside = ((cy >= 0) & (cy < hc))[:, None] & ((cx >= 0) & (cx < wc))[None, :]
                y = np.where(inside[..., None], y, np.float32(0))
                pooled = np.zeros((POOL_ROWS, POOL_COLS, 64), dtype=np.float32)
                for dy in range(3):
                    for dx in range(3):
                        pooled = np.maximum(pooled, y[dy:dy + 2 * POOL_ROWS - 1:2, dx:dx + 2 * POOL_COLS - 1:2])   # a NaN stays
                py, px = POOL_ROWS * ty, POOL_COLS * tx
                out[i, py:py + POOL_ROWS, px:px + POOL_COLS] = pooled[:hp - py, :wp - px]
    return out.transpose(0, 3, 1, 2)


def reference_and_bound(x, w, b):
    """x (N, 3, H, W), w (64, 3, 7, 7), b (64,) or None: fp32 CPU tensors (any strides).
    -> (ref, bound), fp64 (N, 64, Hp, Wp): max_pool2d(relu(conv2d)) in fp64 on the same operands, and the bound of the module docstring."""
    x64, w64 = x.double(), w.double()
    b64 = None if b is None else b.double()
    conv = torch.relu(F.conv2d(x64, w64, b64, 2, 3))
    ref = F.max_pool2d(conv, 3, 2, 1)
    xa = torch.nan_to_num(x64.abs(), nan=0.0, posinf=0.0)
    wa = torch.nan_to_num(w64.abs(), nan=0.0, posinf=0.0)
    s = F.conv2d(xa, wa, None if b is None else b64.abs(), 2, 3)
    local = (c_acc(K) + 2.0 ** -20) * s + 2.0 ** -24 * torch.nan_to_num(conv.abs(), nan=0.0, posinf=0.0)
    amax = torch.from_numpy(window_amax(x.contiguous().numpy()))[:, None]
    wmax = wa.flatten(1).amax(1).view(1, -1, 1, 1)
    return ref, F.max_pool2d(local, 3, 2, 1) + 2.0 ** -37 * K * amax * wmax


def stock_fp32(x, w, b):
    """What the default route computes: the same ops in fp32."""
    return F.max_pool2d(torch.relu(F.conv2d(x, w, b, 2, 3)), 3, 2, 1)
