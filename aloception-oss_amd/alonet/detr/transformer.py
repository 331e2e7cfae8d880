"""DETR transformer: post-/pre-norm encoder-decoder on ``nn.MultiheadAttention`` with positional encodings added to
queries and keys at every layer; the decoder returns the (normalised) activations of every layer.

Module tree and parameter names follow alonet/detr/transformer.py:22-440 (``encoder.layers.N.{self_attn, linear1,
linear2, norm1, norm2}``, ``decoder.layers.N.{self_attn, multihead_attn, linear1, linear2, norm1..3}``, ``decoder.norm``)
so reference checkpoints load unchanged.  On stock ops this is the CPU-runnable plumbing model (BASELINE configs[0]).  Under
``ALO_ATTENTION=fused`` a post-norm model at d_model 256 with 8 heads runs its inference forward on the library instead
(``Transformer._forward_fused``): batch-first activations from the flatten to the outputs, every projection a GEMM of
``alo_hip.linear_auto``, attention with the key padding mask in ``alo_hip.attention``, each residual + LayerNorm in
``alo_hip.add_layernorm``, the feed-forward block on the ``ffn256`` / ``ffn_f32`` ladder.  Everything outside that gate
(pre-norm, ``attn_mask``, other widths, training, CPU, overridden hooks) takes the stock ops below unchanged.
"""
import copy

import torch
import torch.nn.functional as F
from torch import nn

import alo_hip
from alonet.transformers.fused_layers import _add_norm, _attention_ok, _cross_attention, _ffn, _fused_ok, _self_attention


def _get_clones(module, n):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


def _get_activation_fn(activation):
    fns = {"relu": F.relu, "gelu": F.gelu, "glu": F.glu}
    if activation not in fns:
        raise RuntimeError(f"activation should be relu/gelu, not {activation}.")
    return fns[activation]


def _with_pos(tensor, pos):
    return tensor if pos is None else tensor + pos


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", normalize_before=False):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.activation = _get_activation_fn(activation)
        self.normalize_before = normalize_before

    def with_pos_embed(self, tensor, pos):
        return _with_pos(tensor, pos)

    def _ffn(self, x):
        return self.linear2(self.dropout(self.activation(self.linear1(x))))

    def forward(self, src, src_mask=None, src_key_padding_mask=None, pos=None, **kwargs):
        if self.normalize_before:
            src2 = self.norm1(src)
            q = k = _with_pos(src2, pos)
            src = src + self.dropout1(self.self_attn(q, k, value=src2, attn_mask=src_mask,
                                                     key_padding_mask=src_key_padding_mask)[0])
            return src + self.dropout2(self._ffn(self.norm2(src)))
        q = k = _with_pos(src, pos)
        src = self.norm1(src + self.dropout1(self.self_attn(q, k, value=src, attn_mask=src_mask,
                                                            key_padding_mask=src_key_padding_mask)[0]))
        return self.norm2(src + self.dropout2(self._ffn(src)))


class TransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = _get_clones(encoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm

    def forward(self, src, mask=None, src_key_padding_mask=None, pos=None, **kwargs):
        out = src
        for layer in self.layers:
            out = layer(out, src_mask=mask, src_key_padding_mask=src_key_padding_mask, pos=pos, **kwargs)
        return out if self.norm is None else self.norm(out)


class TransformerDecoderLayer(nn.Module):
    def __init__(self, d_model, n_heads=8, dim_feedforward=2048, dropout=0.1, activation="relu",
                 normalize_before=False):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)
        self.activation = _get_activation_fn(activation)
        self.normalize_before = normalize_before

    def with_pos_embed(self, tensor, pos):
        return _with_pos(tensor, pos)

    def pre_process_tgt(self, tgt, query_pos, tgt_key_padding_mask, **kwargs):
        return tgt, query_pos, tgt_key_padding_mask

    def _ffn(self, x):
        return self.linear2(self.dropout(self.activation(self.linear1(x))))

    def decoder_layer_forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                              memory_key_padding_mask=None, pos=None, query_pos=None, **kwargs):
        def self_block(x):
            q = k = _with_pos(x, query_pos)
            return self.self_attn(q, k, value=x, attn_mask=tgt_mask, key_padding_mask=tgt_key_padding_mask)[0]

        def cross_block(x):
            return self.multihead_attn(query=_with_pos(x, query_pos), key=_with_pos(memory, pos), value=memory,
                                       attn_mask=memory_mask, key_padding_mask=memory_key_padding_mask)[0]

        if self.normalize_before:
            tgt = tgt + self.dropout1(self_block(self.norm1(tgt)))
            tgt = tgt + self.dropout2(cross_block(self.norm2(tgt)))
            return tgt + self.dropout3(self._ffn(self.norm3(tgt)))
        tgt = self.norm1(tgt + self.dropout1(self_block(tgt)))
        tgt = self.norm2(tgt + self.dropout2(cross_block(tgt)))
        return self.norm3(tgt + self.dropout3(self._ffn(tgt)))

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos=None, query_pos=None, **kwargs):
        tgt, query_pos, tgt_key_padding_mask = self.pre_process_tgt(tgt, query_pos, tgt_key_padding_mask, **kwargs)
        return self.decoder_layer_forward(tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask,
                                          memory_key_padding_mask, pos, query_pos, **kwargs)


class TransformerDecoder(nn.Module):
    def __init__(self, decoder_layer, num_layers, norm=None, return_intermediate=False):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm
        self.return_intermediate = return_intermediate

    def pre_process_tgt(self, tgt, query_pos, tgt_key_padding_mask, **kwargs):
        return tgt, query_pos, tgt_key_padding_mask

    def decoder_forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                        memory_key_padding_mask=None, pos=None, query_pos=None, **kwargs):
        out = tgt
        intermediate = []
        for layer in self.layers:
            out = layer(out, memory, tgt_mask=tgt_mask, memory_mask=memory_mask,
                        tgt_key_padding_mask=tgt_key_padding_mask, memory_key_padding_mask=memory_key_padding_mask,
                        pos=pos, query_pos=query_pos, **kwargs)
            if self.return_intermediate:
                intermediate.append(self.norm(out))
        if self.norm is not None:
            out = self.norm(out)
        if self.return_intermediate:
            return torch.stack(intermediate)
        return out.unsqueeze(0)

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos=None, query_pos=None, decoder_outputs=None, **kwargs):
        decoder_outputs = {} if decoder_outputs is None else decoder_outputs
        tgt, query_pos, tgt_key_padding_mask = self.pre_process_tgt(tgt, query_pos, tgt_key_padding_mask=None, **kwargs)
        decoder_outputs["hs"] = self.decoder_forward(
            tgt, memory, tgt_mask=tgt_mask, memory_mask=memory_mask, tgt_key_padding_mask=tgt_key_padding_mask,
            memory_key_padding_mask=memory_key_padding_mask, pos=pos, query_pos=query_pos, **kwargs)
        return decoder_outputs


class Transformer(nn.Module):
    def __init__(self, d_model=512, nhead=8, encoder=None, decoder=None, decoder_layer=None, encoder_layer=None,
                 num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=2048, dropout=0.1, activation="relu",
                 normalize_before=False, return_intermediate_dec=False):
        super().__init__()
        if encoder is None:
            encoder_layer = encoder_layer or TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout,
                                                                     activation, normalize_before)
            encoder = TransformerEncoder(encoder_layer, num_encoder_layers,
                                         nn.LayerNorm(d_model) if normalize_before else None)
        self.encoder = encoder
        if decoder is None:
            decoder_layer = decoder_layer or TransformerDecoderLayer(d_model, nhead, dim_feedforward, dropout,
                                                                     activation, normalize_before)
            decoder = TransformerDecoder(decoder_layer, num_decoder_layers, nn.LayerNorm(d_model),
                                         return_intermediate=return_intermediate_dec)
        self.decoder = decoder
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.d_model = d_model
        self.nhead = nhead

    def _fused_route_ok(self, x, mask, query_embed, pos_embed, kwargs):
        """The gate of :meth:`_forward_fused` on the flattened batch-first activation ``x`` (B, HW, C): the switch, inference
        outside autograd over the activation and every module the route reads, post-norm layers with the stock forwards and
        hooks (a subclass that overrides one keeps the stock ops), the attention kernel's geometry, one dtype throughout."""
        if not alo_hip.attention_routed() or "decoder_outputs" in kwargs:
            return False
        if any((k == "mask" or k.endswith("_mask")) and v is not None for k, v in kwargs.items()):
            return False    # an attn_mask for the encoder (mask), the decoder (tgt_mask) or the cross-attention (memory_mask)
        enc, dec = self.encoder, self.decoder
        stock = (type(enc).forward is TransformerEncoder.forward and type(dec).forward is TransformerDecoder.forward
                 and type(dec).decoder_forward is TransformerDecoder.decoder_forward
                 and type(dec).pre_process_tgt is TransformerDecoder.pre_process_tgt
                 and all(type(l).forward is TransformerEncoderLayer.forward and not l.normalize_before for l in enc.layers)
                 and all(type(l).forward is TransformerDecoderLayer.forward and not l.normalize_before
                         and type(l).decoder_layer_forward is TransformerDecoderLayer.decoder_layer_forward
                         and type(l).pre_process_tgt is TransformerDecoderLayer.pre_process_tgt for l in dec.layers))
        if not stock or len(enc.layers) == 0 or len(dec.layers) == 0 or (dec.return_intermediate and dec.norm is None):
            return False
        if mask.dtype != torch.bool or not _fused_ok(self, kwargs, x, mask, query_embed, pos_embed, self):
            return False
        mhas = [l.self_attn for l in enc.layers] + [m for l in dec.layers for m in (l.self_attn, l.multihead_attn)]
        return (all(_attention_ok(m, x) for m in mhas) and query_embed.dtype == x.dtype and pos_embed.dtype == x.dtype
                and all(p.dtype == x.dtype and p.device == x.device for p in self.parameters()))

    def _forward_fused(self, x, mask, query_embed, pos, shape):
        """The inference forward on the library: x, pos (B, HW, C) contiguous, mask (B, HW) bool -> the dict of :meth:`forward`,
        with the shapes and strides the sequence-first stock route gives its outputs."""
        bs, c, h, w = shape
        enc, dec = self.encoder, self.decoder
        qk_in = x + pos
        for layer in enc.layers:
            x = _add_norm(layer.norm1, _self_attention(layer.self_attn, qk_in, x, mask), x)
            x, qk_in = _add_norm(layer.norm2, _ffn(layer.linear1, layer.activation, layer.linear2, x), x, pos=pos)
        memory, key_in = x, qk_in           # the cross-attention's keys are memory + pos in every decoder layer
        if enc.norm is not None:
            memory = _add_norm(enc.norm, memory, None)
            key_in = memory + pos
        query_pos = query_embed.unsqueeze(0).expand(bs, -1, -1).contiguous()
        tgt, tgt_q, hs = torch.zeros_like(query_pos), query_pos, []
        for layer in dec.layers:
            tgt, tgt_q = _add_norm(layer.norm1, _self_attention(layer.self_attn, tgt_q, tgt), tgt, pos=query_pos)
            cross = _cross_attention(layer.multihead_attn, tgt_q, key_in, memory, mask)
            tgt = _add_norm(layer.norm2, cross, tgt)
            tgt, tgt_q = _add_norm(layer.norm3, _ffn(layer.linear1, layer.activation, layer.linear2, tgt), tgt, pos=query_pos)
            if dec.return_intermediate:
                hs.append(_add_norm(dec.norm, tgt, None))
        if not dec.return_intermediate:
            hs = [tgt if dec.norm is None else _add_norm(dec.norm, tgt, None)]
        # (layers, B, Q, C) and (B, C, H, W) as views of sequence-first storage: what the stock route hands on
        return {"hs": torch.stack(hs).transpose(1, 2).contiguous().transpose(1, 2),
                "memory": memory.transpose(0, 1).contiguous().permute(1, 2, 0).view(bs, c, h, w)}

    def forward(self, src, mask, query_embed, pos_embed, **kwargs):
        """src (B,C,H,W), mask (B,H,W) bool, query_embed (Q,C), pos_embed (B,C,H,W) -> dict(hs (layers,B,Q,C), memory)."""
        bs, c, h, w = src.shape
        if alo_hip.attention_routed() and src.is_cuda:
            x = src.flatten(2).transpose(1, 2)
            if self._fused_route_ok(x, mask, query_embed, pos_embed, kwargs):
                return self._forward_fused(x.contiguous(), mask.flatten(1).contiguous(), query_embed,
                                           pos_embed.flatten(2).transpose(1, 2).contiguous(), (bs, c, h, w))
        src = src.flatten(2).permute(2, 0, 1)
        pos_embed = pos_embed.flatten(2).permute(2, 0, 1)
        query_embed = query_embed.unsqueeze(1).repeat(1, bs, 1)
        mask = mask.flatten(1)
        memory = self.encoder(src, src_key_padding_mask=mask, pos=pos_embed, **kwargs)
        out = {}
        out.update(self.decoder(torch.zeros_like(query_embed), memory, memory_key_padding_mask=mask, pos=pos_embed,
                                query_pos=query_embed, **kwargs))
        out["memory"] = memory.permute(1, 2, 0).view(bs, c, h, w)
        out["hs"] = out["hs"].transpose(1, 2)
        return out
