"""Two-stage Deformable-DETR on the CPU: module wiring, parameter names and the torch restatements of the proposal arithmetic
against the reference's own outputs (G19, tests/golden/make_golden_two_stage.py), plus the C ABI of include/alo_two_stage.h.

As in test_models_cpu.py the deformable attention runs through the reference's ``is_tracing`` escape hatch (pure-torch op)."""
import numpy as np
import pytest
import torch
from torch import nn

import alo_hip
from alonet.deformable_detr import DeformableDETR, DeformableTransformer
from alonet.deformable_detr.deformable_transformer import encoder_output_proposals, proposal_pos_embed
from alonet.transformers import MLP
from helpers import declared_functions, formula_state_dict

t = torch.from_numpy


def build_g19_transformer(g, attach_heads=True):
    """The fixture's configuration with this repository's classes, in fp64, weights from the tensor names."""
    d_model, nhead, enc, dec, ffn, L, dec_p, enc_p, topk, classes = (int(x) for x in g["cfg"])
    tr = DeformableTransformer(d_model=d_model, nhead=nhead, num_encoder_layers=enc, num_decoder_layers=dec, dim_feedforward=ffn,
                               dropout=0.0, return_intermediate_dec=True, num_feature_levels=L, dec_n_points=dec_p,
                               enc_n_points=enc_p, two_stage=True, two_stage_num_proposals=topk)
    if attach_heads:
        tr.decoder.class_embed = nn.ModuleList([nn.Linear(d_model, classes) for _ in range(dec + 1)])
        tr.decoder.bbox_embed = nn.ModuleList([MLP(d_model, d_model, 4, 3) for _ in range(dec + 1)])
    tr = tr.double().eval()
    res = tr.load_state_dict(formula_state_dict(tr.state_dict()))
    assert not res.missing_keys and not res.unexpected_keys
    return tr, L


def g19_inputs(g, L, device="cpu", dtype=torch.float64):
    srcs = [t(g[f"src{i}"]).to(device, dtype) for i in range(L)]
    poss = [t(g[f"pos{i}"]).to(device, dtype) for i in range(L)]
    masks = [t(g[f"mask{i}"]).to(device) for i in range(L)]
    return srcs, masks, poss


def assert_same_inf_pattern_and_close(got, want, atol):
    """+inf exactly where the reference has it (no NaN, no -inf anywhere), finite entries within ``atol``."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any() and not np.isneginf(got).any()
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    finite = np.isfinite(want)
    assert finite.any() and (~finite).any()
    assert np.abs(got[finite] - want[finite]).max() <= atol


def test_two_stage_constructor_builds_the_reference_parameter_set(golden):
    g = golden("g19_two_stage_transformer.npz")
    tr, _ = build_g19_transformer(g)
    keys = sorted(tr.state_dict())
    assert keys == [str(k) for k in g["keys"]]
    assert not any(k.startswith("reference_points.") for k in keys)
    assert {"enc_output.weight", "enc_output_norm.bias", "pos_trans.weight", "pos_trans_norm.weight"} <= set(keys)
    assert tr.pos_trans.weight.shape == (512, 512) and tr.enc_output.weight.shape == (256, 256)
    one_stage = DeformableTransformer(d_model=32, nhead=2, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=32)
    assert "reference_points.weight" in one_stage.state_dict() and "enc_output.weight" not in one_stage.state_dict()


def test_proposals_restatement_matches_reference_fp64(golden):
    g = golden("g19_two_stage_transformer.npz")
    shapes = [tuple(g[f"mask{i}"].shape[1:]) for i in range(4)]
    mask_flatten = torch.cat([t(g[f"mask{i}"]).flatten(1) for i in range(4)], 1)
    proposals, keep = encoder_output_proposals(mask_flatten, shapes)   # the model's call: float32 grid, as the reference
    assert proposals.dtype == torch.float32
    # The reference's grid is float32 whatever the memory's dtype, so G19 holds float32 values and the float32 call is the one held
    # to the fp64 bar of 1e-10: same divisions, same log.  That leans on torch's CPU float32 log giving the same bits here as where
    # the fixture was made (its vectorised paths are chosen by instruction set); a build that differs there misses by about one
    # float32 ulp of a logit, <= 5e-7, and the float64 call below, free of that dependency, still pins the arithmetic to 2e-6.
    assert_same_inf_pattern_and_close(proposals.numpy(), g["output_proposals"], 1e-10)
    assert np.array_equal(keep.numpy(), np.isfinite(g["output_proposals"]).all(-1))
    assert not keep[mask_flatten].any()                                     # padding is never kept
    for lvl, start in enumerate(np.cumsum([0] + [h * w for h, w in shapes])[:-1]):   # both kinds of token at every level
        sl = keep[:, start:start + shapes[lvl][0] * shapes[lvl][1]]
        assert sl.any() and not sl.all()
    p64, keep64 = encoder_output_proposals(mask_flatten, shapes, dtype=torch.float64)
    assert torch.equal(keep64, keep) and p64.dtype == torch.float64
    assert_same_inf_pattern_and_close(p64.numpy(), g["output_proposals"], 2e-6)   # float32 rounding of the stored grid


def test_proposal_pos_embed_restatement_matches_reference_fp64(golden):
    g = golden("g19_two_stage_transformer.npz")
    coords = t(g["enc_outputs_coord_unact"])
    picked = torch.gather(coords, 1, t(g["topk"]).unsqueeze(-1).expand(-1, -1, 4))
    embed = proposal_pos_embed(picked)
    assert embed.dtype == torch.float64 and embed.shape == (2, 12, 512)
    assert np.abs(embed.numpy() - g["proposal_pos_embed"]).max() <= 1e-10
    edge = proposal_pos_embed(torch.tensor([[float("inf"), float("-inf"), 0.0, 1.0]], dtype=torch.float64))
    assert torch.isfinite(edge).all()
    assert edge[0, 128] == 0.0 and edge[0, 129] == 1.0                      # sigmoid(-inf) = 0: sin 0, cos 0


def test_two_stage_transformer_graph_matches_reference_fp64(golden):
    g = golden("g19_two_stage_transformer.npz")
    tr, L = build_g19_transformer(g)
    srcs, masks, poss = g19_inputs(g, L)
    with torch.no_grad():
        out = tr(srcs, masks, poss, None, is_tracing=None)
    assert_same_inf_pattern_and_close(out["enc_outputs_coord_unact"].numpy(), g["enc_outputs_coord_unact"], 1e-10)
    np.testing.assert_allclose(out["enc_outputs_class"].numpy(), g["enc_outputs_class"], rtol=0, atol=1e-10)
    topk = torch.topk(out["enc_outputs_class"][..., 0], 12, dim=1)[1]
    assert np.array_equal(topk.numpy(), g["topk"])
    assert out["init_reference_out"].shape == (2, 12, 4)
    for key in ("init_reference_out", "hs", "inter_references_out"):
        np.testing.assert_allclose(out[key].numpy(), g[key], rtol=1e-9, atol=1e-10)
    for i in range(L):   # stored as float32, as G12's
        np.testing.assert_allclose(out["memory"][i].numpy(), g[f"memory{i}"], rtol=0, atol=2e-6)
    with pytest.raises(AssertionError):   # one-stage still insists on its query embedding
        DeformableTransformer(d_model=32, nhead=2, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=32)(
            [s[:, :32] for s in srcs], masks, [p[:, :32] for p in poss], None, is_tracing=None)


def test_two_stage_needs_d_model_256():
    with pytest.raises(ValueError, match="d_model = 256"):
        DeformableTransformer(d_model=64, nhead=4, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=64, two_stage=True)


def test_missing_or_short_heads_raise_runtime_error(golden):
    g = golden("g19_two_stage_transformer.npz")
    tr, L = build_g19_transformer(g, attach_heads=False)
    srcs, masks, poss = g19_inputs(g, L)
    with torch.no_grad(), pytest.raises(RuntimeError, match="decoder.class_embed is missing"):
        tr(srcs, masks, poss, None, is_tracing=None)
    tr.decoder.class_embed = nn.ModuleList([nn.Linear(256, 5) for _ in range(2)]).double()
    with torch.no_grad(), pytest.raises(RuntimeError, match="decoder.bbox_embed is missing"):
        tr(srcs, masks, poss, None, is_tracing=None)
    tr.decoder.bbox_embed = nn.ModuleList([MLP(256, 256, 4, 3)]).double()
    with torch.no_grad(), pytest.raises(RuntimeError, match="decoder.bbox_embed holds 1 heads"):
        tr(srcs, masks, poss, None, is_tracing=None)
    tr.decoder.bbox_embed = nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(2)]).double()
    tr.two_stage_num_proposals = 164   # S = 163
    with torch.no_grad(), pytest.raises(RuntimeError, match="out of range"):
        tr(srcs, masks, poss, None, is_tracing=None)


def build_two_stage_detr(device=None, num_queries=7, with_box_refine=True, **kwargs):
    """DeformableDETR over the seeded stub pyramid (helpers.stub_pyramid) with a two-stage transformer of 1 + 2 layers."""
    from test_models_golden_cpu import deformable_joiner

    backbone = deformable_joiner((8, 12, 16, 24), 256)
    transformer = DeformableDETR.build_transformer(DeformableDETR.__new__(DeformableDETR), hidden_dim=256, dropout=0.0, nheads=8, dim_feedforward=64, enc_layers=1,
                                                   dec_layers=2, num_feature_levels=4, two_stage=True, num_queries=num_queries)
    return DeformableDETR(backbone, transformer, num_classes=5, num_queries=num_queries, aux_loss=True,
                          with_box_refine=with_box_refine, device=device, **kwargs)


def test_two_stage_model_wiring():
    model = build_two_stage_detr()
    keys = set(model.state_dict())
    assert model.transformer.two_stage and model.transformer.two_stage_num_proposals == 7
    for i in range(3):   # 2 decoder layers + the proposal heads
        assert f"class_embed.{i}.weight" in keys and f"bbox_embed.{i}.layers.2.bias" in keys
    assert "class_embed.3.weight" not in keys and "bbox_embed.3.layers.0.weight" not in keys
    assert "transformer.enc_output.weight" in keys and "transformer.pos_trans_norm.bias" in keys
    assert not any(k.startswith("query_embed.") for k in keys) and not any("reference_points" in k for k in keys)
    assert model.transformer.decoder.class_embed is model.class_embed and model.transformer.decoder.bbox_embed is model.bbox_embed
    assert model.num_decoder_layers == 2
    assert all(float(b.layers[-1].bias.detach().abs().max()) == 0.0 for b in model.bbox_embed)
    with pytest.raises(ValueError, match="with_box_refine"):
        build_two_stage_detr(with_box_refine=False)
    one_stage = DeformableDETR.build_transformer(DeformableDETR.__new__(DeformableDETR), hidden_dim=32, nheads=2, dim_feedforward=32, enc_layers=1, dec_layers=1)
    assert not one_stage.two_stage and "reference_points.weight" in one_stage.state_dict()


def test_two_stage_model_forward_on_the_torch_branch():
    """The whole model on the CPU through ``is_tracing``: the extra output keys, their shapes, and gradients into the new layers."""
    import aloscene

    torch.manual_seed(0)
    model = build_two_stage_detr().eval()
    model.load_state_dict(formula_state_dict(model.state_dict()))
    gen = torch.Generator().manual_seed(3)
    frames = aloscene.Frame.batch_list([aloscene.Frame(torch.rand(3, h, w, generator=gen) * 255, normalization="255").norm_resnet()
                                        for h, w in ((64, 96), (48, 80))])
    out = model(frames, is_tracing=None)
    S = sum(-(-64 // s) * -(-96 // s) for s in (8, 16, 32, 64))
    assert out["pred_logits"].shape == (2, 7, 5) and out["pred_boxes"].shape == (2, 7, 4) and len(out["aux_outputs"]) == 1
    assert out["enc_outputs_class"].shape == (2, S, 5) and out["enc_outputs_coord"].shape == (2, S, 4)
    assert "enc_outputs" not in out   # that key is the panoptic head's encoder memory
    coord = out["enc_outputs_coord"]
    assert torch.isfinite(coord).all() and coord.min() >= 0 and coord.max() <= 1 and bool((coord == 1).any())   # sigmoid(+inf) at dropped tokens
    (out["pred_logits"].sum() + out["pred_boxes"].sum() + out["enc_outputs_class"].sum()).backward()
    for p in (model.transformer.enc_output.weight, model.transformer.pos_trans.weight, model.class_embed[2].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


# ---- C ABI of include/alo_two_stage.h (the library's whole export set is held to its headers in test_cabi.py) ------------------
def test_header_declares_the_three_kernels():   # and the first two as one launch
    assert declared_functions("alo_two_stage.h") == ["alo_encoder_proposals", "alo_encoder_proposals_masked", "alo_mask_rows", "alo_proposal_queries"]


def test_argument_errors_are_reported_before_any_launch():
    import ctypes

    lib = hot = alo_hip.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    shapes = (ctypes.c_int * 18)(*([2, 2] * 9))
    assert lib.alo_encoder_proposals(None, None, None, 1, 1, shapes, None) == 1 and b"null pointer" in hot.alo_last_error()
    assert lib.alo_encoder_proposals(one, one, one, 1, 9, shapes, None) == 1 and b"L <= 8" in hot.alo_last_error()
    empty = (ctypes.c_int * 2)(3, 0)
    assert lib.alo_encoder_proposals(one, one, one, 1, 1, empty, None) == 1 and b"empty shape" in hot.alo_last_error()
    assert lib.alo_mask_rows(one, one, ctypes.c_void_p(32), 4, 12, alo_hip.ALO_BF16, None) != 0 and b"16 bytes" in hot.alo_last_error()
    assert lib.alo_mask_rows(one, one, ctypes.c_void_p(32), 4, 8, alo_hip.ALO_F64, None) != 0 and b"dtype" in hot.alo_last_error()
    assert lib.alo_mask_rows(one, one, one, 4, 8, alo_hip.ALO_F32, None) == 1 and b"alias" in hot.alo_last_error()
    assert lib.alo_proposal_queries(one, one, one, one, one, 1, 0, 1, alo_hip.ALO_F32, None) == 1 and b"K >= 1" in hot.alo_last_error()
    assert lib.alo_proposal_queries(one, one, one, ctypes.c_void_p(20), one, 1, 4, 1, alo_hip.ALO_F32, None) == 1 and b"aligned" in hot.alo_last_error()
    cpu = torch.zeros(2, 4, dtype=torch.bool)
    assert not alo_hip.encoder_proposals_supported(cpu, [(2, 2)])
    with pytest.raises(RuntimeError, match="encoder_proposals"):
        alo_hip.encoder_proposals(cpu, [(2, 2)])
    with pytest.raises(RuntimeError, match="mask_rows"):
        alo_hip.mask_rows(torch.zeros(2, 4, 8), cpu)
    with pytest.raises(RuntimeError, match="proposal_queries"):
        alo_hip.proposal_queries(torch.zeros(2, 4, 4), torch.zeros(2, 1, dtype=torch.long), torch.float32)
