"""fp64 yardstick of ``alo_hip.attention`` (ALO_BLOCK_ATTENTION of include/alo_encoder_block.h) on torch ops, from the kernel's own
operands: a bf16 / fp16 / fp32 element widens to fp64 exactly, so the only error in the comparison is the kernel's.  Runs on whatever
device its arguments live on; tests/test_attention_cpu.py pins it to ``nn.MultiheadAttention``.
"""
import torch

from kernel_bounds import c_acc

HEADS, HEAD_DIM = 8, 32
SCALE = float(torch.tensor(HEAD_DIM ** -0.5, dtype=torch.float32))   # the fp32 scale the wrapper passes, exact in fp64
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}


def _heads(t):
    b, l, _ = t.shape
    return t.double().view(b, l, HEADS, HEAD_DIM).transpose(1, 2)   # (B, H, L, 32)


def attention_ref(q, k, v, key_padding_mask=None):
    """q (B, Lq, 256), k and v (B, Lk, 256), mask (B, Lk) bool / uint8 (non-zero = ignored) or None -> (B, Lq, 256) fp64.  A query
    all of whose keys are masked is NaN in its 256 outputs (softmax over an all -inf row), as ``nn.MultiheadAttention`` gives."""
    scores = _heads(q) @ _heads(k).transpose(-1, -2) * SCALE            # (B, H, Lq, Lk)
    if key_padding_mask is not None:
        scores = scores.masked_fill(key_padding_mask.bool()[:, None, None, :], float("-inf"))
    out = torch.softmax(scores, dim=-1) @ _heads(v)                     # all -inf -> NaN
    return out.transpose(1, 2).reshape(q.shape[0], q.shape[1], HEADS * HEAD_DIM)


def attention_bound(q, k, v, key_padding_mask, dtype):
    """(B, Lq, 256) fp64: ``2 A (u_out + u_P + 2 ds + c_acc(Lk) 2^-24)`` per output, derived in tests/test_attention_gpu.py.
    A = max |v| over the image's unmasked keys (all 256 channels), ds = c_acc(32) 2^-24 scale max_k sum_d |q_d k_d| of the
    query's head."""
    u = UNIT_ROUNDOFF[dtype]
    u_out, u_p = (2.0 ** -24, 0.0) if dtype == torch.float32 else (u, u)
    qh, kh = _heads(q), _heads(k)
    mag = qh.abs() @ kh.abs().transpose(-1, -2)                          # (B, H, Lq, Lk): sum_d |q_d k_d|
    vmax = v.double().abs().amax(-1)                                     # (B, Lk): max |v| of a key
    if key_padding_mask is not None:
        dead = key_padding_mask.bool()
        mag = mag.masked_fill(dead[:, None, None, :], 0.0)
        vmax = vmax.masked_fill(dead, 0.0)
    ds = c_acc(HEAD_DIM) * 2.0 ** -24 * SCALE * mag.amax(-1)             # (B, H, Lq)
    a = vmax.amax(-1)[:, None, None]                                     # (B, 1, 1)
    bound = 2 * a * (u_out + u_p + 2 * ds + c_acc(k.shape[1]) * 2.0 ** -24)   # (B, H, Lq)
    b, lq = q.shape[:2]
    return bound.transpose(1, 2)[..., None].expand(b, lq, HEADS, HEAD_DIM).reshape(b, lq, HEADS * HEAD_DIM).contiguous()
