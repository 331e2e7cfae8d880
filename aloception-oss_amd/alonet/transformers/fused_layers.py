"""The inference-time layer helpers the two transformers share (Deformable-DETR's and DETR's): the gate of the fused routes, the
residual + LayerNorm epilogue, ``nn.MultiheadAttention``'s projections as GEMMs of this library, dense attention, the feed-forward
ladder.  Everything here runs on batch-first (B, L, E) tensors and only behind :func:`_fused_ok`.
"""
import torch.nn.functional as F

import alo_hip


def _fused_ok(module, kwargs, *operands):
    """The one-pass HIP epilogues (alo_add_layernorm) stand in for ``norm(x + dropout(y))`` when nothing is lost: eval mode
    (dropout is the identity), no autograd graph, CUDA, fp32 / bf16 / fp16, and not the pure-torch export branch.  ``operands``:
    the activation first, then every tensor and module the fast path behind this gate reads (alo_hip.fusable) — the kernels detach
    their result, so a trainable parameter or an upstream tensor that requires grad sends the whole route to the stock ops."""
    return (not module.training and "is_tracing" not in kwargs and alo_hip.fusable(*operands, f16=True)
            and alo_hip.add_layernorm_supported(operands[0]))


def _add_norm(norm, x, residual, pos=None):
    return alo_hip.add_layernorm(x, residual, norm.weight, norm.bias, norm.eps, pos=pos)


def _self_attention(mha, qk_in, v_in, key_padding_mask=None):
    """Inference form of ``nn.MultiheadAttention(q = k = qk_in, v = v_in)`` on batch-first (B, L, E) tensors: the packed
    input projection as two GEMMs (q and k share their input), ``scaled_dot_product_attention`` over the heads, the output
    projection — no sequence-first transposes, projections on the short-K MFMA kernel when the shape allows.  A
    ``key_padding_mask`` (B, L) is for callers behind :func:`_attention_ok` only: it goes to ``alo_hip.attention``."""
    (w_qk, b_qk), (w_v, b_v) = _in_proj_rows(mha)
    qk = alo_hip.linear_auto(qk_in, w_qk, b_qk)
    v = alo_hip.linear_auto(v_in, w_v, b_v)
    return alo_hip.linear_auto(_attend(mha, qk, v, key_padding_mask), mha.out_proj.weight, mha.out_proj.bias)


def _cross_attention(mha, q_in, k_in, v_in, key_padding_mask=None):
    """Inference form of ``nn.MultiheadAttention(q_in, k_in, v_in)`` on batch-first tensors behind :func:`_attention_ok`: three
    projections, ``alo_hip.attention`` with the keys' padding mask, the output projection."""
    E = mha.embed_dim
    w, b = mha.in_proj_weight, mha.in_proj_bias
    rows = alo_hip.derived(mha, "in_proj_thirds", (w,), lambda: (w[:E], w[E: 2 * E], w[2 * E:]))
    q, k, v = (alo_hip.linear_auto(x, rows[i], None if b is None else b[i * E: (i + 1) * E]) for i, x in enumerate((q_in, k_in, v_in)))
    return alo_hip.linear_auto(alo_hip.attention(q, k, v, key_padding_mask), mha.out_proj.weight, mha.out_proj.bias)


def _attention_ok(mha, x):
    """Whether ``mha`` over the batch-first activation ``x`` can run on ``alo_hip.attention``: the ``ALO_ATTENTION=fused`` switch and
    the kernel's geometry (8 heads, d_model 256, one packed input projection, no extra key / value rows); the caller's
    :func:`_fused_ok` answers for autograd, device and dtype."""
    return (alo_hip.attention_routed() and mha.num_heads == alo_hip.ATTENTION_HEADS and mha.embed_dim == 256 and x.shape[-1] == 256
            and mha.in_proj_weight is not None and mha.bias_k is None and mha.bias_v is None and not mha.add_zero_attn
            and not mha.batch_first)


def _in_proj_rows(mha):
    """((w_qk (2E, E), b_qk), (w_v (E, E), b_v)) of ``mha``'s packed input projection."""
    E = mha.embed_dim
    w, b = mha.in_proj_weight, mha.in_proj_bias
    # the SAME row slices every call (inference only: _fused_ok): what linear_auto derives from a weight rides on the tensor object
    w_qk, w_v = alo_hip.derived(mha, "in_proj_rows", (w,), lambda: (w[: 2 * E], w[2 * E:]))
    return (w_qk, None if b is None else b[: 2 * E]), (w_v, None if b is None else b[2 * E:])


def _attend(mha, qk, v, key_padding_mask=None):
    """Attention over ``mha``'s heads on the projected (B, L, 2E) [q; k] and (B, L, E) v -> (B, L, E), before the output
    projection: ``alo_hip.attention`` on the tensors as they stand under ``ALO_ATTENTION=fused`` (8 heads, E = 256), else
    ``scaled_dot_product_attention`` between two head-major transposes (no mask there)."""
    B, L, E = v.shape
    H = mha.num_heads
    q, k = qk[..., :E], qk[..., E:]
    if alo_hip.attention_routed() and H == alo_hip.ATTENTION_HEADS and alo_hip.attention_supported(q, k, v, key_padding_mask):
        return alo_hip.attention(q, k, v, key_padding_mask)
    if key_padding_mask is not None:
        raise RuntimeError("_attend: a key_padding_mask needs the alo_hip.attention route (ALO_ATTENTION=fused)")
    heads = lambda t: t.reshape(B, L, H, E // H).transpose(1, 2)  # (B, H, L, E/H)
    out = F.scaled_dot_product_attention(heads(q), heads(k), heads(v))
    return out.transpose(1, 2).reshape(B, L, E)


def _ffn(linear1, activation, linear2, x):
    """``linear2(act(linear1(x)))``; for ReLU the activation rides in the first GEMM's epilogue (alo_linear_shortk when
    d_model is 64 / 128 / 256 and the tensors are bf16 / fp16, else hipBLASLt's RELU_BIAS via ``torch._addmm_activation``) instead
    of a separate pass over the (rows, d_ffn) intermediate.  d_model = 256: one kernel for both layers in bf16 / fp16, and in fp32
    under ``ALO_F32_LAYERS=split`` at the shapes ``alo_hip.ffn_f32_routed`` admits."""
    if activation is F.relu and alo_hip.ffn256_supported(x, linear1.weight, linear2.weight, f16=True):
        # d_model = 256, bf16 / fp16: both layers in one kernel, the hidden activation never leaves the chip
        return alo_hip.ffn256(x, linear1.weight, linear1.bias, linear2.weight, linear2.bias)
    if activation is F.relu and alo_hip.ffn_f32_routed(x, linear1.weight, linear2.weight):
        # d_model = 256, fp32 under ALO_F32_LAYERS=split, at the shapes it was measured to win: the same block on the fp16 matrix cores
        return alo_hip.ffn_f32(x, linear1.weight, linear1.bias, linear2.weight, linear2.bias)
    if activation is F.relu and linear1.bias is not None:
        h = alo_hip.linear_auto(x, linear1.weight, linear1.bias, relu=True)
        return alo_hip.linear_auto(h, linear2.weight, linear2.bias)
    return linear2(activation(linear1(x)))
