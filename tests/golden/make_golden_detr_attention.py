#!/usr/bin/env python
"""G22 — the reference's DETR transformer at the width the attention kernel serves (build container only).

  g22_detr_transformer_d256.npz   alonet/detr/transformer.py of the reference: Transformer(d_model 256, 8 heads, 2 + 2 post-norm
                                  layers, dim_feedforward 512, dropout 0, return_intermediate_dec) in fp64 with
                                  helpers.formula_state_dict weights (as G10), run on the float64 copies of fp32 inputs:
                                    src    (2, 256, 7, 10) fp32, randn            70 tokens: more than one key tile of the kernel
                                    pos    (2, 256, 7, 10) fp32, 0.5 * randn
                                    mask   (2, 7, 10) bool; image 0 unpadded, image 1 valid on its top-left 5 x 6 pixels
                                    query  (37, 256) fp32, randn
                                    hs     (2, 2, 37, 256) fp64, memory (2, 256, 7, 10) fp64

Arrays only.  The fixture pins the packed in_proj row order, the key padding mask in the encoder's self-attention and the decoder's
cross-attention, the per-layer decoder.norm of return_intermediate and the sequence-first plumbing to the reference.

Usage:  python tests/golden/make_golden_detr_attention.py        (from the repo root)
"""
import importlib
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as G  # noqa: E402

CFG = dict(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=512, dropout=0.0, return_intermediate_dec=True)
QUERIES, H, W, VALID = 37, 7, 10, (5, 6)


def main():
    if not os.path.isdir(G.REF):
        sys.exit("make_golden_detr_attention.py needs the reference checkout (build container only)")
    G.load_reference()
    sys.path.insert(0, os.path.dirname(OUT))
    from helpers import formula_state_dict

    G._shell("alonet.detr", G.REF + "/alonet/detr")
    TR = importlib.import_module("alonet.detr.transformer")
    torch.manual_seed(2200)
    tr = TR.Transformer(**CFG).double().eval()
    tr.load_state_dict(formula_state_dict(tr.state_dict()))
    src = torch.randn(2, CFG["d_model"], H, W).float()
    pos = (0.5 * torch.randn(2, CFG["d_model"], H, W)).float()
    query = torch.randn(QUERIES, CFG["d_model"]).float()
    mask = torch.zeros(2, H, W, dtype=torch.bool)
    mask[1, VALID[0]:, :] = True
    mask[1, :, VALID[1]:] = True
    with torch.no_grad():
        out = tr(src.double(), mask, query.double(), pos.double())
    hs, memory = out["hs"], out["memory"]
    assert hs.dtype == torch.float64 and tuple(hs.shape) == (2, 2, QUERIES, CFG["d_model"]) and torch.isfinite(hs).all()
    assert tuple(memory.shape) == (2, CFG["d_model"], H, W) and torch.isfinite(memory).all()
    path = os.path.join(OUT, "g22_detr_transformer_d256.npz")
    np.savez_compressed(path, src=G._np(src), pos=G._np(pos), mask=G._np(mask), query=G._np(query), hs=G._np(hs), memory=G._np(memory))
    print("wrote g22, bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
