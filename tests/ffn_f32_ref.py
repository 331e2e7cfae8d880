"""Shared by test_ffn_f32_cpu.py and test_ffn_f32_gpu.py: the arithmetic of aloception-oss_amd/csrc/ffn_f32.hip restated in numpy, and
the fp64 reference with the per-element bound that both the restatement (CPU) and the kernel (GPU) are held to.

y = relu(x W1^T + b1) W2^T + b2 with x (M, 256), W1 (F, 256), W2 (256, F).  The first product is linear_f32_ref.linear_split with the
ReLU (one power of two per row of x and per hidden unit); the second one consumes the fp32 hidden activation h' 256 units at a time:
each (row, chunk) has its own power of two, a chunk's three products go into a fresh accumulator, and the chunks are added in fp32 in
ascending order, then b2.

The bound (read linear_f32_ref.py's and conv_f32_ref.py's derivations first).  h = relu(x W1^T + b1) exactly, h' what the kernel holds.
  * |h' - h| <= bound1, linear_f32_ref.reference_and_bound(x, W1, b1, relu=True)'s bound.  The second product is linear in h, so this
    reaches output o as  sum_u bound1_u |W2_ou| = (bound1 @ |W2|^T)_o.
  * The second product's own error, on the operand it really has: |h'| <= |h| + bound1 =: H, S2 = H @ |W2|^T + |b2|.
      - accumulation: within a chunk 3 x 256 / 16 MFMAs round partial sums of that chunk's products, over the F / 256 chunks that is
        what c_acc(F) S2 allows an F-term fp32 dot product plus its bias (kernel_bounds.c_acc: twice the worst case of F roundings);
        the F / 256 additions  y_acc += chunk  round a partial sum of magnitude <= S2 each: (F / 256) 2^-23 S2 at the same factor 2.
      - 2^-20 S2: the two-term splits of a chunk of a row (|u - hi - lo| <= 2^-22 |u| + floor) and of a column's weights, and the
        dropped lo lo product, as in conv_f32_ref.py.
      - the floors, 2^-38 (amax sum |w| + wmax sum |h|) there, with the CHUNK's amax because the power of two is the chunk's:
        2^-38 (sum_chunks amax_row,chunk sum_{u in chunk} |W2_ou|  +  wmax_o sum_u H_u).
      - undoing the scales is exact (ldexp); adding b2 rounds once: 2^-24 |ref|.

  |y - ref| <= bound1 @ |W2|^T + (c_acc(F) + (F / 256) 2^-23 + 2^-20) S2
               + 2^-38 (sum_chunks amax_chunk(H) sum_chunk |W2_o| + wmax_o sum H) + 2^-24 |ref|

Non-finite inputs take no part in any amax or sum; the outputs of a row that holds one, or whose hidden row does, are compared for kind
(kernel_bounds.compare), not for value.
"""
import numpy as np
import torch

import linear_f32_ref
from kernel_bounds import c_acc
from linear_f32_ref import linear_split
from split_f16_ref import row_exponents, split_terms, split_weight

CHUNK = 256


def ffn_split(x, w1, b1, w2, b2):
    """The kernel's arithmetic.  x (M, 256), w1 (F, 256), b1 (F,) or None, w2 (256, F), b2 (256,) or None, fp32 numpy -> (M, 256) fp32."""
    h = linear_split(x, w1, b1, None, True)
    w_hi, w_lo, kc = split_weight(w2)
    y = np.zeros((x.shape[0], w2.shape[0]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, h.shape[1], CHUNK):
            hc = h[:, c0:c0 + CHUNK]
            kr = row_exponents(hc)                                           # the (row, chunk)'s own power of two
            h_hi, h_lo = split_terms(hc, kr[:, None])
            wh, wl = w_hi[:, c0:c0 + CHUNK], w_lo[:, c0:c0 + CHUNK]
            acc = (h_hi @ wl.T + h_lo @ wh.T) + h_hi @ wh.T                  # a fresh accumulator, small terms first
            y = (y + np.ldexp(acc, kr[:, None] + kc[None, :]).astype(np.float32)).astype(np.float32)
        if b2 is not None:
            y = (y + b2).astype(np.float32)
    return y


def reference_and_bound(x, w1, b1, w2, b2):
    """x (M, 256), w1 (F, 256), b1 (F,) or None, w2 (256, F), b2 (256,) or None: fp32 CPU tensors.  -> (ref, bound), fp64 (M, 256)."""
    fin = lambda a: torch.nan_to_num(a.abs(), nan=0.0, posinf=0.0)  # noqa: E731
    h, bound1 = linear_f32_ref.reference_and_bound(x, w1, b1, None, True)
    w64 = w2.double()
    wa = fin(w64)
    ref = h @ w64.t()
    hub = fin(h) + bound1
    s2 = hub @ wa.t()
    if b2 is not None:
        ref = ref + b2.double()
        s2 = s2 + b2.double().abs()
    f = w1.shape[0]
    floor = wa.amax(1)[None, :] * hub.sum(1, keepdim=True)
    for c0 in range(0, f, CHUNK):
        floor = floor + hub[:, c0:c0 + CHUNK].amax(1, keepdim=True) * wa[:, c0:c0 + CHUNK].sum(1)[None, :]
    bound = (bound1 @ wa.t() + (c_acc(f) + (f // CHUNK) * 2.0 ** -23 + 2.0 ** -20) * s2 + 2.0 ** -38 * floor + 2.0 ** -24 * fin(ref))
    return ref, bound


MANY_TILES = 17000      # 266 tiles of 64 rows on at most 256 workgroups (one per CU): ten workgroups walk a second tile, the last holds 40 rows
# (M, F): the smallest at which each mechanism can fail
SHAPES = [
    (1, 256),               # one row, one chunk
    (63, 512),              # ragged either side of a tile; a second chunk
    (65, 256),
    (130, 1024),            # three tiles, four chunks (the detector's width)
    (77, 2048),             # eight chunks
    (MANY_TILES, 256),
]
SCALES = linear_f32_ref.SCALES


def operands(shape, scale=1.0):
    """x (M, 256), b1 (F,), b2 (256,) at ``scale``, w1 (F, 256) at 1 / 16, w2 (256, F) at 1 / sqrt(F): fp32 CPU tensors from a seed of the
    shape."""
    m, f = shape
    g = torch.Generator().manual_seed(m * 11 + f)
    x = torch.randn(m, 256, generator=g) * scale
    w1 = torch.randn(f, 256, generator=g) / 16
    b1 = torch.randn(f, generator=g) * scale
    w2 = torch.randn(256, f, generator=g) / f ** 0.5
    b2 = torch.randn(256, generator=g) * scale
    return x, w1, b1, w2, b2


def dim_rows(shape=(130, 1024)):
    """Operands with row 70 of x 10^6 dimmer than its neighbours, and W1's second chunk of hidden units 10^6 dimmer than its first (every
    row's second hidden chunk is then that much dimmer: row 3 is the one the tests run alone), b1 likewise."""
    x, w1, b1, w2, b2 = (t.clone() for t in operands(shape))
    x[70] *= 1e-6
    w1[CHUNK:2 * CHUNK] *= 1e-6
    b1[CHUNK:2 * CHUNK] *= 1e-6
    return x, w1, b1, w2, b2
