"""Deformable transformer (encoder over all pyramid pixels, decoder over object queries) on the gfx950 MSDA op.

Module tree, parameter names and arithmetic follow alonet/deformable_detr/deformable_transformer.py:22-633 so that a
reference checkpoint's ``transformer.*`` keys load unchanged; every attention gather goes through
``MSDeformAttn`` -> ``MSDeformAttnFunction`` -> HIP.  The two-stage variant (``two_stage=True``: the encoder's tokens propose
the decoder's queries, reference :108-112, :130-177, :248-263) is restated at the end of this file's helpers; at inference its
element-wise passes run on the kernels of csrc/two_stage.hip.
"""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, normal_, xavier_uniform_

import alo_hip
from alonet.transformers.fused_layers import _add_norm, _attend, _ffn, _fused_ok, _in_proj_rows, _self_attention  # noqa: F401 (re-exported)

from .ops.modules import MSDeformAttn
from .utils import inverse_sigmoid


_GEOMETRY = {}


def _level_geometry(shapes, device):
    """int32 ``spatial_shapes`` (L,2) / ``level_start_index`` (L,) on the device — what this fork of the op reads
    (ms_deform_attn_cuda.cu:67-68) — built once per (pyramid, device): a host->device copy per forward would also make the
    forward impossible to capture in a HIP graph.  The host-side copies ride along as attributes so that shape checks
    and loops downstream need no device synchronisation."""
    key = (shapes, str(device))
    if key not in _GEOMETRY:
        sizes = [h * w for h, w in shapes]
        # built outside inference mode whatever the caller's mode: an inference tensor cached here would later fail in
        # MSDeformAttnFunction's save_for_backward when a training step reuses the same pyramid shape
        with torch.inference_mode(False):
            spatial_shapes = torch.tensor(shapes, dtype=torch.int32, device=device)
            level_start_index = torch.tensor([sum(sizes[:i]) for i in range(len(sizes))], dtype=torch.int32, device=device)
        spatial_shapes._alo_total = sum(sizes)
        spatial_shapes._alo_shapes = list(shapes)
        _GEOMETRY[key] = (spatial_shapes, level_start_index)
    return _GEOMETRY[key]


PROPOSAL_EMBED_DIM = 512   # 4 box components x 128 sine features: fixed by the reference (:131), hence d_model = 256 for two-stage


def encoder_output_proposals(mask_flatten, shapes, dtype=torch.float32):
    """One box proposal per encoder token, from the padding mask alone (reference :145-171).

    mask_flatten (B, S) bool, True on padding; shapes [(h_l, w_l)] as Python ints.  Returns ``(proposals, keep)``:
    ``proposals`` (B, S, 4) ``dtype`` holds ``log(p / (1 - p))`` of ``p = ((x + 0.5) / valid_W, (y + 0.5) / valid_H, wh, wh)``
    with ``wh = 0.05 * 2^level``, where ``valid_W`` / ``valid_H`` count the un-padded tokens of the level's first row / first
    column per image; ``keep`` (B, S) bool is True where the token is not padding and ``0.01 < p < 0.99`` holds in all four
    components.  Tokens outside ``keep`` get ``+inf`` in all four components.

    The model calls it in float32 whatever its own dtype, as the reference does (its grid is float32 and its counts are
    integers): nothing here depends on a parameter, so there is nothing to differentiate.  ``dtype=torch.float64`` is the
    yardstick the float32 kernel (``alo_hip.encoder_proposals``) is measured against.

    Two properties of the reference are kept on purpose:
      * a dropped token is only marked by ``+inf`` coordinates and a zeroed memory row.  Its class logit, computed from the
        zeroed row, is finite (the heads' biases), so ``topk`` can still select it;
      * a level whose first row (or column) is entirely padding has ``valid_W = 0``: ``p = inf`` fails the window test, so the
        whole level is dropped for that image — no NaN appears.
    """
    device = mask_flatten.device
    B = mask_flatten.shape[0]
    per_level, start = [], 0
    for lvl, (h, w) in enumerate(shapes):
        free = ~mask_flatten[:, start:start + h * w].view(B, h, w)
        valid_h = free[:, :, 0].sum(1).to(dtype).view(B, 1, 1)
        valid_w = free[:, 0, :].sum(1).to(dtype).view(B, 1, 1)
        cy = ((torch.arange(h, dtype=dtype, device=device) + 0.5).view(1, h, 1) / valid_h).expand(B, h, w)
        cx = ((torch.arange(w, dtype=dtype, device=device) + 0.5).view(1, 1, w) / valid_w).expand(B, h, w)
        side = torch.full((B, h, w), 0.05 * 2.0 ** lvl, dtype=dtype, device=device)
        per_level.append(torch.stack((cx, cy, side, side), -1).view(B, h * w, 4))
        start += h * w
    p = torch.cat(per_level, 1)
    keep = ((p > 0.01) & (p < 0.99)).all(-1) & ~mask_flatten
    proposals = torch.log(p / (1 - p)).masked_fill(~keep.unsqueeze(-1), float("inf"))
    return proposals, keep


def proposal_pos_embed(coords_unact):
    """Sine embedding of un-activated boxes (reference :130-143): (..., 4) -> (..., 512) in the input's dtype, component-major;
    within a component ``sin(a_i)`` at even and ``cos(a_i)`` at odd positions, ``a_i = sigmoid(c) * 2 pi / 10000^(2 floor(i / 2) / 128)``.
    The frequencies are float32 whatever the input's dtype, as in the reference.  ``+-inf`` gives sigmoid 1 / 0: finite output."""
    dim_t = 10000 ** (torch.arange(64, dtype=torch.float32, device=coords_unact.device) / 64)   # one per (sin, cos) pair; 2 k / 128 = k / 64 exactly
    angle = (coords_unact.sigmoid() * (2 * math.pi)).unsqueeze(-1) / dim_t     # (..., 4, 64)
    return torch.stack((angle.sin(), angle.cos()), -1).flatten(-3)


def _get_clones(module, n):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


def _get_activation_fn(activation):
    fns = {"relu": F.relu, "gelu": F.gelu, "glu": F.glu}
    if activation not in fns:
        raise RuntimeError(f"activation should be relu/gelu, not {activation}.")
    return fns[activation]


class DeformableTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self.dropout2 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout3 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, src):
        src2 = self.linear2(self.dropout2(self.activation(self.linear1(src))))
        return self.norm2(src + self.dropout3(src2))

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None, **kwargs):
        src2 = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index,
                              padding_mask, **kwargs)
        src = self.norm1(src + self.dropout1(src2))
        return self.forward_ffn(src)

    def forward_fused(self, src, query, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None,
                      next_query=True, **kwargs):
        """Inference form of ``forward``: ``query = src + pos`` comes in ready-made, both residual + LayerNorm pairs are
        one HIP pass each, and the second one also emits the next layer's query.  -> (src', src' + pos | None)"""
        src2 = self.self_attn(query, reference_points, src, spatial_shapes, level_start_index, padding_mask, **kwargs)
        src = _add_norm(self.norm1, src2, src)
        src2 = _ffn(self.linear1, self.activation, self.linear2, src)
        if next_query and pos is not None:
            return _add_norm(self.norm2, src2, src, pos=pos)
        return _add_norm(self.norm2, src2, src), None

    def block_supported(self, src, query):
        """Whether this layer's row-local chain fits the fused kernel (alo_hip.encoder_block): the conjunction of what the
        separate launches of ``forward_fused`` and of the head-major attention path ask for."""
        attn = self.self_attn
        return (self.activation is F.relu and attn.head_major_supported(query, src)
                and alo_hip.encoder_block_supported(
                    src, self.linear1.weight, self.linear2.weight, self.linear1.bias, self.linear2.bias, self.norm1.weight,
                    self.norm1.bias, self.norm2.weight, self.norm2.bias, attn.output_proj.bias, heads=attn.n_heads,
                    levels=attn.n_levels, points=attn.n_points, value_weight=attn.value_proj.weight))

    def forward_block(self, src, value, both, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None,
                      next_layer=None):
        """``forward_fused`` in two launches: the attention kernel on ready-made inputs (value, offsets + logits), then everything
        up to the next attention kernel in one (alo_hip.encoder_block): output projection, both residual + LayerNorm pairs, the
        FFN and ``next_layer``'s three projections.  -> (src', next value | None, next offsets + logits | None)"""
        attn = self.self_attn
        out = attn.forward_head_major(value, both, reference_points, spatial_shapes, level_start_index, project=False)
        tail = (out, attn.output_proj.weight, attn.output_proj.bias, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        nxt = None
        if next_layer is not None:
            n_attn = next_layer.self_attn
            w_cat, b_cat = n_attn._merged_query_projection()
            nxt = (pos, padding_mask, n_attn.value_proj.weight, n_attn.value_proj.bias, w_cat, b_cat)
        return alo_hip.encoder_block(
            src, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias,
            (self.norm2.weight, self.norm2.bias, self.norm2.eps),
            tail=tail, nxt=nxt)


class DeformableTransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers):
        super().__init__()
        self.layers = _get_clones(encoder_layer, num_layers)
        self.num_layers = num_layers

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device, **kwargs):
        """Every pixel centre of every level, normalised by the valid (un-padded) extent: (B, S, L, 2)."""
        per_level = []
        host_shapes = getattr(spatial_shapes, "_alo_shapes", None)  # python copy set by DeformableTransformer: no device sync
        if (host_shapes is not None and valid_ratios.is_cuda and valid_ratios.dtype == torch.float32
                and not alo_hip.needs_autograd(valid_ratios) and "is_tracing" not in kwargs):
            return alo_hip.encoder_reference_points(valid_ratios, host_shapes)   # one kernel instead of ~10 per level
        for lvl in range(spatial_shapes.shape[0]):
            h, w = host_shapes[lvl] if host_shapes is not None else (int(spatial_shapes[lvl, 0]), int(spatial_shapes[lvl, 1]))
            ys = torch.arange(h, dtype=torch.float32, device=device) + 0.5
            xs = torch.arange(w, dtype=torch.float32, device=device) + 0.5
            ref_y, ref_x = torch.meshgrid(ys, xs, indexing="ij")
            ref_y = ref_y.reshape(1, -1) / (valid_ratios[:, None, lvl, 1] * h)
            ref_x = ref_x.reshape(1, -1) / (valid_ratios[:, None, lvl, 0] * w)
            per_level.append(torch.stack((ref_x, ref_y), -1))
        reference_points = torch.cat(per_level, 1)
        return reference_points[:, :, None] * valid_ratios[:, None]

    def forward(self, src, spatial_shapes, level_start_index, valid_ratios, pos=None, padding_mask=None, **kwargs):
        output = src
        reference_points = self.get_reference_points(spatial_shapes, valid_ratios, device=src.device, **kwargs)
        if _fused_ok(self, kwargs, output, pos, self) and all(hasattr(layer, "forward_fused") for layer in self.layers):
            query = output if pos is None else output + pos
            if (pos is not None and alo_hip.encoder_block_enabled()
                    and all(hasattr(layer, "forward_block") and layer.block_supported(output, query) for layer in self.layers)):
                # between two attention kernels ONE launch: layer 0's projections with the separate kernels, then per layer the
                # attention kernel and the block, which also makes the next layer's projections
                value, both = self.layers[0].self_attn.head_major_inputs(query, output, padding_mask)
                for i, layer in enumerate(self.layers):
                    nxt = self.layers[i + 1] if i + 1 < len(self.layers) else None
                    output, value, both = layer.forward_block(output, value, both, pos, reference_points, spatial_shapes,
                                                              level_start_index, padding_mask, next_layer=nxt)
                return output
            for i, layer in enumerate(self.layers):
                output, query = layer.forward_fused(output, query, pos, reference_points, spatial_shapes, level_start_index,
                                                    padding_mask, next_query=i + 1 < len(self.layers), **kwargs)
                if query is None:
                    query = output
            return output
        for layer in self.layers:
            output = layer(output, pos, reference_points, spatial_shapes, level_start_index, padding_mask, **kwargs)
        return output


class DeformableTransformerDecoderLayer(nn.Module):
    def __init__(self, d_model=256, dim_feedforward=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8,
                 n_points=4):
        super().__init__()
        self.cross_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.activation = _get_activation_fn(activation)
        self.dropout3 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.dropout4 = nn.Dropout(dropout)
        self.norm3 = nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, tgt):
        tgt2 = self.linear2(self.dropout3(self.activation(self.linear1(tgt))))
        return self.norm3(tgt + self.dropout4(tgt2))

    def pre_process_tgt(self, tgt, query_pos, tgt_key_padding_mask, **kwargs):
        return tgt, query_pos, tgt_key_padding_mask

    def decoder_layer_forward(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index,
                              tgt_key_padding_mask=None, src_padding_mask=None, **kwargs):
        carried = tgt.__dict__.get("_alo_with_pos")  # (query_pos, tgt + query_pos) left by the previous layer's last LayerNorm kernel
        if carried is not None and carried[0] is query_pos:
            q = k = carried[1]
        else:
            q = k = self.with_pos_embed(tgt, query_pos)  # self-attention among the queries (sequence-first API)
        # the fused route reads every parameter of this layer, and its LayerNorm kernels detach what the cross-attention made of
        # ``src`` / ``reference_points``: all of them are asked
        if (_fused_ok(self, kwargs, tgt, query_pos, src, reference_points, self) and tgt_key_padding_mask is None
                and self.self_attn._qkv_same_embed_dim):
            tgt2 = _self_attention(self.self_attn, q, tgt)
        else:
            tgt2 = self.self_attn(q.transpose(0, 1), k.transpose(0, 1), tgt.transpose(0, 1),
                                  key_padding_mask=tgt_key_padding_mask)[0].transpose(0, 1)
        # inference: residual + LayerNorm (+ query_pos) in one pass each
        if _fused_ok(self, kwargs, tgt, tgt2, query_pos, src, reference_points, self):
            if query_pos is None:
                tgt = query = _add_norm(self.norm2, tgt2, tgt)
            else:
                tgt, query = _add_norm(self.norm2, tgt2, tgt, pos=query_pos.expand_as(tgt))
            tgt2 = self.cross_attn(query, reference_points, src, src_spatial_shapes, level_start_index,
                                   src_padding_mask, **kwargs)
            tgt = _add_norm(self.norm1, tgt2, tgt)
            if query_pos is None or not query_pos.is_contiguous():
                return _add_norm(self.norm3, _ffn(self.linear1, self.activation, self.linear2, tgt), tgt)
            # the layer's output and (output + query_pos), the next layer's self-attention input, from the same pass
            out, out_pos = _add_norm(self.norm3, _ffn(self.linear1, self.activation, self.linear2, tgt), tgt, pos=query_pos)
            out._alo_with_pos = (query_pos, out_pos)
            return out
        tgt = self.norm2(tgt + self.dropout2(tgt2))
        tgt2 = self.cross_attn(self.with_pos_embed(tgt, query_pos), reference_points, src, src_spatial_shapes,
                               level_start_index, src_padding_mask, **kwargs)
        tgt = self.norm1(tgt + self.dropout1(tgt2))
        return self.forward_ffn(tgt)

    def block_supported(self, tgt, query_pos, src):
        """Whether this layer's two row-local chains fit the fused kernels (alo_hip.decoder_block_a / _b): stock forward methods,
        bf16 with d_model = 256, 8 heads, L = P = 4, ReLU, every bias, a hidden width whose LDS frame fits, and what the separate
        launches of ``decoder_layer_forward`` and of the head-major attention path ask for."""
        mha, attn, cls = self.self_attn, self.cross_attn, DeformableTransformerDecoderLayer
        stock = all(getattr(type(self), name) is getattr(cls, name) for name in ("forward", "pre_process_tgt", "decoder_layer_forward"))
        return (stock and self.activation is F.relu and mha._qkv_same_embed_dim and mha.embed_dim == 256 and mha.num_heads == 8
                and attn.n_heads == 8 and attn.head_major_supported(tgt, src)
                and alo_hip.ffn256_supported(tgt, self.linear1.weight, self.linear2.weight)
                and alo_hip.decoder_block_supported(
                    tgt, query_pos, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                    attn.output_proj.weight, attn.output_proj.bias, self.linear1.weight, self.linear1.bias, self.linear2.weight,
                    self.linear2.bias, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias, self.norm3.weight,
                    self.norm3.bias, hidden=self.linear1.out_features))

    def forward_block(self, tgt, qk, v, query_pos, reference_points, src, src_spatial_shapes, level_start_index,
                      src_padding_mask=None, next_layer=None):
        """``decoder_layer_forward`` at inference with ONE launch between two attention kernels: self-attention on the ready-made
        projections ``qk`` (B, L, 512) and ``v`` (B, L, 256), chain A (alo_hip.decoder_block_a: output projection, norm2, the
        merged offsets + logits projection of ``tgt + query_pos``), the MSDA kernel, chain B (alo_hip.decoder_block_b: output
        projection, norm1, the FFN, norm3 and ``next_layer``'s two input projections).  The last layer has no next projections
        and keeps its separate launches after the MSDA kernel.  -> (out, next qk | None, next v | None)"""
        mha, attn = self.self_attn, self.cross_attn
        w_cat, b_cat = attn._merged_query_projection()
        tgt, both = alo_hip.decoder_block_a(_attend(mha, qk, v), tgt, query_pos, mha.out_proj.weight, mha.out_proj.bias,
                                            (self.norm2.weight, self.norm2.bias, self.norm2.eps), w_cat, b_cat)
        value = alo_hip.value_proj_head_major(src, attn.value_proj.weight, attn.value_proj.bias, src_padding_mask, attn.n_heads)
        out = attn.forward_head_major(value, both, reference_points, src_spatial_shapes, level_start_index, project=False)
        if next_layer is None:
            tgt = _add_norm(self.norm1, alo_hip.linear_auto(out, attn.output_proj.weight, attn.output_proj.bias), tgt)
            return _add_norm(self.norm3, _ffn(self.linear1, self.activation, self.linear2, tgt), tgt), None, None
        (w_qk, b_qk), (w_v, b_v) = _in_proj_rows(next_layer.self_attn)
        out, v, qk = alo_hip.decoder_block_b(
            out, tgt, query_pos, attn.output_proj.weight, attn.output_proj.bias, (self.norm1.weight, self.norm1.bias, self.norm1.eps),
            self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias,
            (self.norm3.weight, self.norm3.bias, self.norm3.eps), w_v, b_v, w_qk, b_qk)
        return out, qk, v

    def forward(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index,
                tgt_key_padding_mask=None, src_padding_mask=None, **kwargs):
        tgt, query_pos, tgt_key_padding_mask = self.pre_process_tgt(tgt, query_pos, tgt_key_padding_mask, **kwargs)
        return self.decoder_layer_forward(tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index,
                                          tgt_key_padding_mask, src_padding_mask, **kwargs)


class DeformableTransformerDecoder(nn.Module):
    def __init__(self, decoder_layer, num_layers, return_intermediate=False):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.return_intermediate = return_intermediate
        self.bbox_embed = None  # set by DeformableDETR for iterative box refinement
        self.class_embed = None
        self.two_stage = False  # set by DeformableTransformer: two-stage queries keep the layers' separate launches

    def pre_process_tgt(self, tgt, query_pos, tgt_key_padding_mask, reference_points, **kwargs):
        return tgt, query_pos, tgt_key_padding_mask, reference_points

    def decoder_forward(self, tgt, reference_points, src, src_spatial_shapes, src_level_start_index, src_valid_ratios,
                        query_pos=None, src_padding_mask=None, tgt_key_padding_mask=None, **kwargs):
        output = tgt
        intermediate, intermediate_refs = [], []
        ref_input = None
        # one launch between two attention kernels (forward_block): inference in bf16 on stock layers, one-stage, queries with a dense
        # query_pos and no padding; layer 0's two input projections with the separate kernels, every later layer gets them from
        # the block before it.  Intermediate outputs and box refinement read ``output`` as on the separate launches.
        block = (alo_hip.decoder_block_routed(tgt) and not self.two_stage and query_pos is not None and tgt_key_padding_mask is None
                 and query_pos.shape == tgt.shape and query_pos.is_contiguous()
                 and all(hasattr(layer, "forward_block") and _fused_ok(layer, kwargs, tgt, query_pos, src, reference_points, layer)
                         and layer.block_supported(tgt, query_pos, src) for layer in self.layers))
        qk = v = None
        if block:
            (w_qk, b_qk), (w_v, b_v) = _in_proj_rows(self.layers[0].self_attn)
            qk, v = alo_hip.linear_auto(tgt + query_pos, w_qk, b_qk), alo_hip.linear_auto(tgt, w_v, b_v)
        for lid, layer in enumerate(self.layers):
            if ref_input is None or self.bbox_embed is not None:  # without box refinement the reference points never change
                if reference_points.shape[-1] == 4:
                    ratios = torch.cat([src_valid_ratios, src_valid_ratios], -1)
                    ref_input = reference_points[:, :, None] * ratios[:, None]
                else:
                    assert reference_points.shape[-1] == 2
                    ref_input = reference_points[:, :, None] * src_valid_ratios[:, None]
            if block:
                nxt = self.layers[lid + 1] if lid + 1 < len(self.layers) else None
                output, qk, v = layer.forward_block(output, qk, v, query_pos, ref_input, src, src_spatial_shapes,
                                                    src_level_start_index, src_padding_mask, next_layer=nxt)
            else:
                output = layer(tgt=output, query_pos=query_pos, reference_points=ref_input, src=src,
                               src_spatial_shapes=src_spatial_shapes, level_start_index=src_level_start_index,
                               src_padding_mask=src_padding_mask, tgt_key_padding_mask=tgt_key_padding_mask, **kwargs)
            if self.bbox_embed is not None:  # iterative bounding-box refinement
                tmp = self.bbox_embed[lid](output)
                if reference_points.shape[-1] == 4:
                    new_ref = (tmp + inverse_sigmoid(reference_points)).sigmoid()
                else:
                    tmp = torch.cat([tmp[..., :2] + inverse_sigmoid(reference_points), tmp[..., 2:]], -1)
                    new_ref = tmp.sigmoid()
                reference_points = new_ref.detach()
            if self.return_intermediate:
                intermediate.append(output)
                intermediate_refs.append(reference_points)
        if self.return_intermediate:
            return torch.stack(intermediate), torch.stack(intermediate_refs)
        return output, reference_points

    def forward(self, tgt, reference_points, src, src_spatial_shapes, src_level_start_index, src_valid_ratios,
                query_pos=None, src_padding_mask=None, tgt_key_padding_mask=None, decoder_outputs=None, **kwargs):
        decoder_outputs = {} if decoder_outputs is None else decoder_outputs
        tgt, query_pos, tgt_key_padding_mask, reference_points = self.pre_process_tgt(
            tgt, query_pos, tgt_key_padding_mask=tgt_key_padding_mask, reference_points=reference_points, **kwargs)
        output, inter_refs = self.decoder_forward(
            tgt=tgt, reference_points=reference_points, src=src, src_spatial_shapes=src_spatial_shapes,
            src_level_start_index=src_level_start_index, src_valid_ratios=src_valid_ratios, query_pos=query_pos,
            src_padding_mask=src_padding_mask, tgt_key_padding_mask=tgt_key_padding_mask, **kwargs)
        decoder_outputs["init_reference_out"] = reference_points
        decoder_outputs.update({"hs": output, "inter_references_out": inter_refs})
        return decoder_outputs


class DeformableTransformer(nn.Module):
    """Transformer with multi-scale deformable attention.  GPU only (the MSDA op has no CPU implementation)."""

    def __init__(self, d_model=256, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=1024,
                 encoder=None, decoder=None, decoder_layer=None, encoder_layer=None, dropout=0.1, activation="relu",
                 return_intermediate_dec=False, num_feature_levels=4, dec_n_points=4, enc_n_points=4,
                 two_stage=False, two_stage_num_proposals=300):
        super().__init__()
        if two_stage and 2 * d_model != PROPOSAL_EMBED_DIM:
            raise ValueError(f"two-stage Deformable-DETR needs d_model = {PROPOSAL_EMBED_DIM // 2}: the proposals' sine embedding is "
                             f"fixed at 4 x 128 = {PROPOSAL_EMBED_DIM} = 2 * d_model channels (got d_model = {d_model})")
        self.d_model, self.nhead = d_model, nhead
        self.two_stage, self.two_stage_num_proposals = two_stage, two_stage_num_proposals
        if encoder is None:
            encoder_layer = encoder_layer or DeformableTransformerEncoderLayer(
                d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead, enc_n_points)
            encoder = DeformableTransformerEncoder(encoder_layer, num_encoder_layers)
        self.encoder = encoder
        if decoder is None:
            decoder_layer = decoder_layer or DeformableTransformerDecoderLayer(
                d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead, dec_n_points)
            decoder = DeformableTransformerDecoder(decoder_layer, num_decoder_layers, return_intermediate_dec)
        self.decoder = decoder
        self.decoder.two_stage = two_stage
        self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model))
        if two_stage:   # the queries come from the encoder's proposals: no learned reference points (reference :108-114)
            self.enc_output = nn.Linear(d_model, d_model)
            self.enc_output_norm = nn.LayerNorm(d_model)
            self.pos_trans = nn.Linear(d_model * 2, d_model * 2)
            self.pos_trans_norm = nn.LayerNorm(d_model * 2)
        else:
            self.reference_points = nn.Linear(d_model, 2)
        self._reset_parameters()

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        if not self.two_stage:
            xavier_uniform_(self.reference_points.weight.data, gain=1.0)
            constant_(self.reference_points.bias.data, 0.0)
        normal_(self.level_embed)

    def get_proposal_pos_embed(self, proposals):
        return proposal_pos_embed(proposals)

    def gen_encoder_output_proposals(self, memory, memory_padding_mask, shapes, fused=False):
        """(``enc_output_norm(enc_output(memory with dropped rows zeroed))``, proposals (B, S, 4) float32): see
        :func:`encoder_output_proposals` for the semantics.  ``shapes``: [(h, w)] as Python ints.  ``fused``: inference, the
        element-wise part on alo_encoder_proposals_masked (or, where that does not apply, alo_encoder_proposals / alo_mask_rows)."""
        if fused and alo_hip.encoder_proposals_masked_supported(memory_padding_mask, shapes, memory, f16=True):
            proposals, keep, output_memory = alo_hip.encoder_proposals_masked(memory_padding_mask, shapes, memory)   # both in one launch
        else:
            if fused and alo_hip.encoder_proposals_supported(memory_padding_mask, shapes):
                proposals, keep = alo_hip.encoder_proposals(memory_padding_mask, shapes)
            else:
                proposals, keep = encoder_output_proposals(memory_padding_mask, shapes)
            if fused and alo_hip.mask_rows_supported(memory, keep, f16=True):
                output_memory = alo_hip.mask_rows(memory, keep)
            else:
                output_memory = memory.masked_fill(~keep.unsqueeze(-1), 0.0)
        if fused and alo_hip.add_layernorm_supported(output_memory):
            output_memory = _add_norm(self.enc_output_norm,
                                      alo_hip.linear_auto(output_memory, self.enc_output.weight, self.enc_output.bias), None)
        else:
            output_memory = self.enc_output_norm(self.enc_output(output_memory))
        return output_memory, proposals

    def _proposal_heads(self):
        """The detection heads the proposals are scored with: entry ``decoder.num_layers`` of ``decoder.class_embed`` /
        ``decoder.bbox_embed`` (the model attaches them; reference :252-254)."""
        n = self.decoder.num_layers
        for name in ("class_embed", "bbox_embed"):
            heads = getattr(self.decoder, name, None)
            if heads is None:
                raise RuntimeError(f"two-stage DeformableTransformer: decoder.{name} is missing — attach the detection heads "
                                   f"({n + 1} of them: one per decoder layer and one for the encoder's proposals) before the forward")
            if len(heads) <= n:
                raise RuntimeError(f"two-stage DeformableTransformer: decoder.{name} holds {len(heads)} heads, the proposals "
                                   f"are scored by entry {n} (one per decoder layer and one more)")
        return self.decoder.class_embed[n], self.decoder.bbox_embed[n]

    def _two_stage_queries(self, memory, mask_flatten, shapes, kwargs):
        """Reference :248-263: score every encoder token as a box proposal, keep the ``two_stage_num_proposals`` best by class
        channel 0 and derive the decoder's inputs from their (detached) boxes.
        -> (query_pos, tgt, reference_points (B, K, 4), enc_outputs_class, enc_outputs_coord_unact)"""
        class_head, box_head = self._proposal_heads()
        fused = _fused_ok(self, kwargs, memory, self.enc_output, self.enc_output_norm, self.pos_trans, self.pos_trans_norm)
        output_memory, output_proposals = self.gen_encoder_output_proposals(memory, mask_flatten, shapes, fused=fused)
        enc_outputs_class = class_head(output_memory)
        enc_outputs_coord_unact = box_head(output_memory) + output_proposals
        topk = torch.topk(enc_outputs_class[..., 0], self.two_stage_num_proposals, dim=1)[1]
        if fused and alo_hip.proposal_queries_supported(enc_outputs_coord_unact, topk, memory.dtype, f16=True):
            # detached as in the stock branch below (reference :258): the proposals are the decoder's inputs, not a route for gradients
            reference_points, embed = alo_hip.proposal_queries(enc_outputs_coord_unact.detach(), topk, memory.dtype,
                                                               owner=self.pos_trans.weight)
        else:
            coords = torch.gather(enc_outputs_coord_unact, 1, topk.unsqueeze(-1).expand(-1, -1, 4)).detach()
            reference_points = coords.sigmoid()
            embed = proposal_pos_embed(coords).to(memory.dtype)
        if fused and alo_hip.add_layernorm_supported(embed):
            pos_trans_out = _add_norm(self.pos_trans_norm, alo_hip.linear_auto(embed, self.pos_trans.weight, self.pos_trans.bias), None)
        else:
            pos_trans_out = self.pos_trans_norm(self.pos_trans(embed))
        query_pos, tgt = torch.split(pos_trans_out, memory.shape[-1], dim=2)
        if fused:   # the decoder layers' one-pass kernels want dense operands
            query_pos, tgt = query_pos.contiguous(), tgt.contiguous()
        return query_pos, tgt, reference_points, enc_outputs_class, enc_outputs_coord_unact

    @staticmethod
    def get_valid_ratio(mask):
        """mask (B,H,W) -> (B,2): fraction (w, h) of the map that is not padding."""
        _, H, W = mask.shape
        valid_h = torch.sum((~mask).float()[:, :, 0], 1, keepdim=True)
        valid_w = torch.sum((~mask).float()[:, 0, :], 1, keepdim=True)
        return torch.cat([valid_w / W, valid_h / H], 1)

    def forward(self, srcs, masks, pos_embeds, query_embed=None, **kwargs):
        assert self.two_stage or query_embed is not None
        device = srcs[0].device
        src_flatten, mask_flatten, pos_flatten, shapes = [], [], [], []
        pos_encoder = kwargs.pop("pos_encoder", None)  # set by DeformableDETR when it left the encodings to this module
        ready = kwargs.pop("src_flatten", None)        # (B, S, C): the levels of ``srcs`` are already views into it
        ready_mask = kwargs.pop("mask_flatten", None)  # (B, S) bool and (B, L, 2) float32 from alo_mask_pyramid
        ready_ratios = kwargs.pop("valid_ratios", None)
        for lvl, (src, mask, pos_embed) in enumerate(zip(srcs, masks, pos_embeds)):
            _, _, h, w = src.shape
            shapes.append((h, w))
            if ready is None:
                src_flatten.append(src.flatten(2).transpose(1, 2))
            if ready_mask is None:
                mask_flatten.append(mask.flatten(1))
            if pos_embed is not None:
                pos_flatten.append(pos_embed.flatten(2).transpose(1, 2) + self.level_embed[lvl].view(1, 1, -1))
        src_flatten = torch.cat(src_flatten, 1) if ready is None else ready
        mask_flatten = torch.cat(mask_flatten, 1) if ready_mask is None else ready_mask
        spatial_shapes, level_start_index = _level_geometry(tuple(shapes), device)
        sizes = [h * w for h, w in shapes]
        if pos_flatten:
            pos_flatten = torch.cat(pos_flatten, 1).to(src_flatten.dtype)
        else:
            # inference: sine encoding of all levels + level embedding in one HIP pass, straight into the flattened layout
            pos_flatten = alo_hip.pos_sine_flat(mask_flatten, spatial_shapes, level_start_index, pos_encoder.dim_t(device),
                                                self.level_embed, pos_encoder.normalize, pos_encoder.center,
                                                pos_encoder.scale, src_flatten.dtype)
        valid_ratios = torch.stack([self.get_valid_ratio(m) for m in masks], 1) if ready_ratios is None else ready_ratios

        memory = self.encoder(src_flatten, spatial_shapes, level_start_index, valid_ratios, pos_flatten, mask_flatten,
                              **kwargs)

        bs, _, c = memory.shape
        enc_outputs_class = enc_outputs_coord_unact = None
        if self.two_stage:
            query_pos, tgt, reference_points, enc_outputs_class, enc_outputs_coord_unact = self._two_stage_queries(
                memory, mask_flatten, shapes, kwargs)
        else:
            query_pos, tgt = torch.split(query_embed, c, dim=1)
            query_pos = query_pos.unsqueeze(0).expand(bs, -1, -1)
            tgt = tgt.unsqueeze(0).expand(bs, -1, -1)
            if _fused_ok(self, kwargs, memory, query_embed):
                # the one-pass kernels of the decoder layers want dense operands: materialise the two broadcasts once per forward
                # instead of once per layer
                query_pos, tgt = query_pos.contiguous(), tgt.contiguous()
            reference_points = self.reference_points(query_pos).sigmoid()

        out = {}
        out.update(self.decoder(tgt, reference_points, memory, spatial_shapes, level_start_index, valid_ratios,
                                query_pos=query_pos, src_padding_mask=mask_flatten, **kwargs))
        memory_t = memory.transpose(1, 2)
        splits, start = [], 0
        for (h, w), n in zip(shapes, sizes):
            splits.append(memory_t[..., start:start + n].reshape(bs, c, h, w))
            start += n
        out["memory"] = splits
        out["enc_outputs_class"] = enc_outputs_class
        out["enc_outputs_coord_unact"] = enc_outputs_coord_unact
        return out
