#!/usr/bin/env python
"""G19 — the reference's two-stage DeformableTransformer (build container only).

  g19_two_stage_transformer.npz   alonet/deformable_detr/deformable_transformer.py:108-112 (enc_output / pos_trans layers),
                                  :130-143 (get_proposal_pos_embed), :145-177 (gen_encoder_output_proposals), :248-263 (top-k
                                  proposals -> decoder inputs), :296-298 (enc_outputs_* keys), run in fp64 through the
                                  ``is_tracing`` branch: d_model 256, 8 heads, 1 + 1 layers, ffn 1024, 4 levels, 4 points,
                                  ``two_stage_num_proposals`` 12, levels (12,10) (6,5) (3,3) (2,2) (S = 163), B = 2 with image 1
                                  padded on its right and bottom (padded and window-invalid proposals at every level).

The reference never attaches ``decoder.class_embed`` / ``decoder.bbox_embed`` itself (its DeformableDETR predates the two-stage
wiring); the generator attaches 2 x Linear(256, 5) and 2 x the reference's MLP(256, 256, 4, 3), as the published model does.
Weights: ``helpers.formula_state_dict`` (derived from tensor names), so no checkpoint is stored.  Inputs are float16-representable
and stored as float16; outputs are the reference's fp64 values, except the per-level memory (float32, as in G12).

The twelve selected class logits and the thirteenth must be pairwise at least 1e-3 apart in fp64, so that an fp32 run selects
the same tokens in the same order; the seed below is the first for which they are (a condition on the fixture, not a tolerance).

Usage:  python tests/golden/make_golden_two_stage.py        (from the repo root)
"""
import importlib
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import make_golden as G  # noqa: E402

SIZES = [(12, 10), (6, 5), (3, 3), (2, 2)]
TOPK, MIN_GAP = 12, 1e-3


def run(ref_mods, seed):
    from helpers import formula_state_dict

    DT = importlib.import_module("alonet.deformable_detr.deformable_transformer")
    MLP = importlib.import_module("alonet.transformers.mlp").MLP
    torch.manual_seed(seed)
    d_model, nhead, L = 256, 8, 4
    tr = DT.DeformableTransformer(d_model=d_model, nhead=nhead, num_encoder_layers=1, num_decoder_layers=1,
                                  dim_feedforward=1024, dropout=0.0, return_intermediate_dec=True, num_feature_levels=L,
                                  dec_n_points=4, enc_n_points=4, two_stage=True, two_stage_num_proposals=TOPK)
    tr.decoder.class_embed = torch.nn.ModuleList([torch.nn.Linear(d_model, 5) for _ in range(2)])
    tr.decoder.bbox_embed = torch.nn.ModuleList([MLP(d_model, d_model, 4, 3) for _ in range(2)])
    tr = tr.double().eval()
    tr.load_state_dict(formula_state_dict(tr.state_dict()))
    B = 2
    srcs = [torch.randn(B, d_model, h, w).half().double() for h, w in SIZES]
    poss = [(torch.randn(B, d_model, h, w) * 0.5).half().double() for h, w in SIZES]
    masks = []
    for h, w in SIZES:  # image 1 is padded on its right / bottom quarter (at least one column / row)
        m = torch.zeros(B, h, w, dtype=torch.bool)
        m[1, :, w - max(1, w // 4):] = True
        m[1, h - max(1, h // 4):, :] = True
        masks.append(m)
    with torch.no_grad():
        out = tr(srcs, masks, poss, None, is_tracing=None)
        logits = out["enc_outputs_class"][..., 0]
        order = torch.argsort(logits, dim=1, descending=True, stable=True)
        top = torch.gather(logits, 1, order[:, :TOPK + 1])
        gap = (top[:, :, None] - top[:, None, :]).abs() + torch.eye(TOPK + 1, dtype=torch.float64) * 1e9
        topk = torch.topk(logits, TOPK, dim=1)[1]
        if gap.min().item() < MIN_GAP or not torch.equal(topk, order[:, :TOPK]):
            return None
        # the two restated functions on their own, called on the reference object
        memory = torch.cat([m.flatten(2).transpose(1, 2) for m in out["memory"]], 1)
        mask_flatten = torch.cat([m.flatten(1) for m in masks], 1)
        shapes = torch.as_tensor(SIZES, dtype=torch.int32)
        _, proposals = tr.gen_encoder_output_proposals(memory, mask_flatten, shapes)
        picked = torch.gather(out["enc_outputs_coord_unact"], 1, topk.unsqueeze(-1).repeat(1, 1, 4))
        embed = tr.get_proposal_pos_embed(picked)
    _np = G._np
    save = dict(cfg=np.array([d_model, nhead, 1, 1, 1024, L, 4, 4, TOPK, 5]), seed=np.array(seed), keys=np.array(sorted(tr.state_dict())),
                enc_outputs_class=_np(out["enc_outputs_class"]), enc_outputs_coord_unact=_np(out["enc_outputs_coord_unact"]),
                topk=_np(topk), topk_gap=np.array(gap.min().item()), output_proposals=_np(proposals), proposal_pos_embed=_np(embed),
                init_reference_out=_np(out["init_reference_out"]), hs=_np(out["hs"]),
                inter_references_out=_np(out["inter_references_out"]))
    for i in range(L):
        save[f"src{i}"], save[f"pos{i}"] = _np(srcs[i]).astype(np.float16), _np(poss[i]).astype(np.float16)
        save[f"mask{i}"] = _np(masks[i])
        save[f"memory{i}"] = _np(out["memory"][i]).astype(np.float32)
    return save


def main():
    if not os.path.isdir(G.REF):
        sys.exit("make_golden_two_stage.py needs the reference checkout (build container only)")
    torch.set_num_threads(4)
    ref_mods = G.load_reference()
    for seed in range(1900, 1964):
        save = run(ref_mods, seed)
        if save is not None:
            break
        print(f"seed {seed}: selected logits closer than {MIN_GAP}, next")
    else:
        sys.exit("no seed separates the selected logits")
    coord = save["enc_outputs_coord_unact"]
    assert np.isinf(coord).any() and not np.isnan(coord).any() and float(save["topk_gap"]) >= MIN_GAP
    path = os.path.join(OUT, "g19_two_stage_transformer.npz")
    np.savez_compressed(path, **save)
    print("wrote g19 with seed", int(save["seed"]), "gap", float(save["topk_gap"]), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
