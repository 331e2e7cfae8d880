"""Two-stage Deformable-DETR on the GPU: the kernels of csrc/two_stage.hip against the torch formulation, the transformer
against the reference's outputs (G19), fast path vs torch path, HIP-graph replay and one training step."""
import numpy as np
import pytest
import torch

import alo_hip
from alonet.deformable_detr.deformable_transformer import encoder_output_proposals, proposal_pos_embed
from test_two_stage_cpu import assert_same_inf_pattern_and_close, build_g19_transformer, build_two_stage_detr, g19_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = torch.from_numpy

# fp32 transformer outputs vs the reference's fp64 ones: the fp32 bar of tests/test_models_gpu.py
# (test_deformable_transformer_on_hip_matches_reference), which lies inside the 0.1 its G12 test allows the bf16 path
FP32_TOL = 1e-3
G19_SHAPES = [(12, 10), (6, 5), (3, 3), (2, 2)]
KERNEL_TAGS = ("encoder_proposals", "mask_rows", "encoder_proposals_masked", "proposal_queries")
# the forward's launches: proposals and row masking go out as one kernel (alo_encoder_proposals_masked), the queries as another
FORWARD_TAGS = ("encoder_proposals_masked", "proposal_queries")


def _ran(timer, which=FORWARD_TAGS):
    tags = [tag.split("/")[0] for tag in timer.summary()]
    return {k: k in tags for k in which}


def _any_kernel_ran(timer):
    return _ran(timer, KERNEL_TAGS)


def _g19_on_gpu(golden, dtype=torch.float32):
    g = golden("g19_two_stage_transformer.npz")
    tr, L = build_g19_transformer(g)
    return g, tr.to(DEV, dtype), g19_inputs(g, L, DEV, dtype), L


def _check_against_g19(out, g, L, tol):
    topk = torch.topk(out["enc_outputs_class"][..., 0], int(g["cfg"][8]), dim=1)[1]
    assert np.array_equal(topk.cpu().numpy(), g["topk"])                          # same tokens, same order
    assert_same_inf_pattern_and_close(out["enc_outputs_coord_unact"].double().cpu().numpy(), g["enc_outputs_coord_unact"], tol)
    errs = {k: np.abs(out[k].double().cpu().numpy() - g[k]).max()
            for k in ("enc_outputs_class", "init_reference_out", "hs", "inter_references_out")}
    for i in range(L):
        errs[f"memory{i}"] = np.abs(out["memory"][i].double().cpu().numpy() - g[f"memory{i}"]).max()
    print("two-stage fp32 vs G19, max-abs:", {k: float(v) for k, v in errs.items()})
    assert max(errs.values()) <= tol, errs


def test_two_stage_transformer_on_hip_matches_reference(golden):
    g, tr, (srcs, masks, poss), L = _g19_on_gpu(golden)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = tr(srcs, masks, poss, None)
    assert all(_ran(timer).values()), _ran(timer)
    assert out["init_reference_out"].shape == (2, 12, 4)
    _check_against_g19(out, g, L, FP32_TOL)


def test_two_stage_transformer_bf16_on_hip_matches_reference(golden, monkeypatch):
    """The headline dtype: bf16 tgt / query_pos beside the float32 reference points and proposals that only the two-stage branch
    hands the decoder.  bf16 rounding of the class logits (about 0.02) exceeds the smallest gap between G19's ranked logits
    (0.0018), so the ranking is not comparable in this dtype: the fixture's selection is imposed on ``torch.topk`` and everything
    else is held to the bf16 bar of tests/test_models_gpu.py (BF16_TRANSFORMER_TOL), the +inf pattern exactly."""
    from test_models_gpu import BF16_TRANSFORMER_TOL

    g, tr, (srcs, masks, poss), L = _g19_on_gpu(golden, torch.bfloat16)
    real_topk = torch.topk

    def fixture_topk(scores, k, dim=-1):
        assert k == 12 and dim == 1 and scores.shape == (2, 163)
        idx = t(g["topk"]).to(scores.device)
        return torch.gather(scores, 1, idx), idx

    monkeypatch.setattr(torch, "topk", fixture_topk)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = tr(srcs, masks, poss, None)
    monkeypatch.setattr(torch, "topk", real_topk)
    assert all(_ran(timer).values()), _ran(timer)
    assert out["hs"].dtype == torch.bfloat16 and out["enc_outputs_class"].dtype == torch.bfloat16
    assert out["init_reference_out"].dtype == torch.float32 and out["enc_outputs_coord_unact"].dtype == torch.float32
    assert_same_inf_pattern_and_close(out["enc_outputs_coord_unact"].double().cpu().numpy(), g["enc_outputs_coord_unact"], BF16_TRANSFORMER_TOL)
    errs = {k: np.abs(out[k].double().cpu().numpy() - g[k]).max()
            for k in ("enc_outputs_class", "init_reference_out", "hs", "inter_references_out")}
    for i in range(L):
        errs[f"memory{i}"] = np.abs(out["memory"][i].double().cpu().numpy() - g[f"memory{i}"]).max()
    print("two-stage bf16 vs G19, max-abs:", {k: float(v) for k, v in errs.items()})
    assert max(errs.values()) <= BF16_TRANSFORMER_TOL, errs


def _mask(shapes, B, seed, edit=None):
    """(B, S) bool: image 0 unpadded, the others padded on the right / bottom by a random amount; ``edit(levels)`` then changes the
    per-level (B, h, w) arrays in place."""
    rng = np.random.default_rng(seed)
    levels = []
    for h, w in shapes:
        m = np.zeros((B, h, w), bool)
        for b in range(1, B):
            m[b, int(rng.integers(1, h + 1)):, :] = True
            m[b, :, int(rng.integers(1, w + 1)):] = True
        levels.append(m)
    if edit is not None:
        edit(levels)
    return torch.from_numpy(np.concatenate([m.reshape(B, -1) for m in levels], 1))


def _first_row_padded(levels):      # image 1, level 0: only the first row is padding, so valid_W = 0 while valid_H = h - 1
    levels[0][1] = False
    levels[0][1, 0, :] = True


def _level_padded(levels):          # image 2, level 1: nothing but padding
    levels[1][2] = True


def _unpadded(levels):
    for m in levels:
        m[:] = False


PROPOSAL_CASES = {
    "g19_pyramid": (G19_SHAPES, 2, None),
    "one_pixel": ([(1, 1)], 2, None),
    "valid_w_zero": ([(5, 7), (3, 4)], 3, _first_row_padded),
    "eight_levels": ([(9, 11), (7, 5), (5, 6), (4, 4), (3, 5), (2, 3), (2, 2), (1, 3)], 2, None),
    "level_fully_padded": ([(6, 6), (3, 3), (2, 2)], 3, _level_padded),
    "ragged_S": ([(13, 7), (5, 3)], 3, None),                 # S = 106, not a multiple of 64
    "several_blocks": ([(40, 33), (50, 3)], 2, _unpadded),    # 1320 tokens: 3 blocks; 0.5 / 50 = 0.01 sits on the window's edge
}


@pytest.mark.parametrize("case", sorted(PROPOSAL_CASES))
def test_encoder_proposals_kernel_vs_torch(case):
    """``keep`` and the +inf pattern bit-equal to the float32 torch formulation on the same device; finite logits within 2e-5 of
    the float64 formulation (inputs in (0.01, 0.99), |logit| <= 4.6, worst term 1 - p near 0.99: relative error 6e-6)."""
    shapes, B, edit = PROPOSAL_CASES[case]
    mask = _mask(shapes, B, seed=len(case), edit=edit).to(DEV)
    got, keep = alo_hip.encoder_proposals(mask, shapes)
    want32, keep32 = encoder_output_proposals(mask, shapes)
    want64, keep64 = encoder_output_proposals(mask, shapes, dtype=torch.float64)
    assert got.dtype == torch.float32 and keep.dtype == torch.bool and got.shape == (B, mask.shape[1], 4)
    assert torch.equal(keep, keep32)
    assert not torch.isnan(got).any()
    assert torch.equal(torch.isposinf(got), torch.isposinf(want32)) and not torch.isneginf(got).any()
    assert torch.equal(torch.isposinf(got).all(-1), ~keep) and torch.equal(torch.isposinf(got).any(-1), ~keep)
    finite = keep64 & keep
    if finite.any():
        assert (got.double() - want64)[finite].abs().max().item() <= 2e-5
    if case == "valid_w_zero":
        assert bool(mask[1, 0]) and not bool(mask[1, 7]) and not keep[1, :35].any() and keep[0, :35].any()
        assert torch.isposinf(got[1, :35]).all()
    if case == "level_fully_padded":
        assert not keep[2, 36:45].any()
    if case == "eight_levels":   # wh = 0.05 * 2^l leaves the window from level 5 on
        start5 = sum(h * w for h, w in shapes[:5])
        assert not keep[:, start5:].any() and keep[0, :start5].any()
    if case == "several_blocks":
        assert not keep[0, 1320:1323].any() and keep[0, 1323:1326].all()   # row 0 of the 50-row level: p_y = float32(0.01) is not > 0.01
    if case == "one_pixel":
        assert keep[0, 0] and got[0, 0, 0] == 0.0   # p = 0.5


@pytest.mark.parametrize("dtype,C", [(torch.float32, 256), (torch.bfloat16, 256), (torch.float32, 8), (torch.bfloat16, 8), (torch.float32, 1032)])
@pytest.mark.parametrize("case", ["g19_pyramid", "one_pixel", "valid_w_zero", "level_fully_padded", "several_blocks"])
def test_encoder_proposals_masked_kernel_equals_the_two_kernels(case, dtype, C):
    """One launch, the same bits as alo_encoder_proposals + alo_mask_rows, and as masked_fill on the float32 formulation's keep;
    C = 1032 floats: more vectors per row (258) than the block has threads."""
    shapes, B, edit = PROPOSAL_CASES[case]
    mask = _mask(shapes, B, seed=len(case), edit=edit).to(DEV)
    memory = torch.randn(B, mask.shape[1], C, generator=torch.Generator().manual_seed(C)).to(DEV, dtype)
    memory[-1, -1, 0], memory[0, 0, -1] = float("nan"), float("inf")
    proposals, keep = alo_hip.encoder_proposals(mask, shapes)
    got_p, got_k, got_m = alo_hip.encoder_proposals_masked(mask, shapes, memory)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got_k, keep) and torch.equal(got_k, encoder_output_proposals(mask, shapes)[1])
    assert torch.equal(got_p.view(torch.int32), proposals.view(torch.int32))
    assert torch.equal(got_m.view(bits), alo_hip.mask_rows(memory, keep).view(bits))
    assert torch.equal(got_m.view(bits), memory.masked_fill(~keep.unsqueeze(-1), 0.0).view(bits))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [8, 256])
@pytest.mark.parametrize("S", [1, 163])
def test_mask_rows_kernel_is_masked_fill(dtype, C, S):
    gen = torch.Generator().manual_seed(S * 1000 + C)
    memory = torch.randn(2, S, C, generator=gen).to(DEV, dtype)
    keep = (torch.rand(2, S, generator=gen) < 0.6).to(DEV)
    keep[0, 0], keep[1, -1] = True, False
    memory[1, -1, 0], memory[1, -1, -1] = float("nan"), float("inf")     # in a dropped row: become 0
    memory[0, 0, C // 2] = float("nan")                                  # in a kept row: preserved
    got = alo_hip.mask_rows(memory, keep)
    want = memory.masked_fill(~keep.unsqueeze(-1), 0.0)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(bits), want.view(bits))
    assert not got[1, -1].any() and torch.isnan(got[0, 0, C // 2])


@pytest.fixture(scope="module")
def query_case():
    """Coordinates with +-inf rows, a float64 reference of everything the kernel produces."""
    gen = torch.Generator().manual_seed(19)
    S = 163
    coords = torch.randn(2, S, 4, generator=gen) * 3
    coords[0, 5] = float("inf")
    coords[1, 7] = float("-inf")
    coords[1, 9, 1], coords[1, 9, 2] = float("inf"), float("-inf")
    return coords


@pytest.mark.parametrize("K", [1, 12, 300])
def test_proposal_queries_kernel_vs_torch_fp64(query_case, K):
    """Reference points within 1e-6, fp32 embedding within 2e-5 (arguments <= 2 pi: fp32 rounding of the argument dominates),
    bf16 embedding within one bf16 ulp of the rounded fp64 value."""
    coords = query_case.to(DEV)
    S = coords.shape[1]
    gen = torch.Generator().manual_seed(K)
    topk = torch.randint(0, S, (2, K), generator=gen)
    topk[:, 0] = torch.tensor([0, S - 1])                                 # first and last token
    if K > 1:
        topk[0, 1:4], topk[1, 1:4] = torch.tensor([5, 5, S - 1])[:K - 1], torch.tensor([7, 9, 7])[:K - 1]   # +-inf rows, duplicates
    topk = topk.to(DEV)
    picked = torch.gather(coords.double(), 1, topk.unsqueeze(-1).expand(-1, -1, 4))
    want_ref, want_embed = picked.sigmoid(), proposal_pos_embed(picked)
    ref, embed = alo_hip.proposal_queries(coords, topk, torch.float32)
    assert ref.shape == (2, K, 4) and embed.shape == (2, K, 512) and embed.dtype == torch.float32
    assert torch.isfinite(ref).all() and torch.isfinite(embed).all()
    assert (ref.double() - want_ref).abs().max().item() <= 1e-6
    assert (embed.double() - want_embed).abs().max().item() <= 2e-5
    ref16, embed16 = alo_hip.proposal_queries(coords, topk, torch.bfloat16)
    assert torch.equal(ref16, ref) and embed16.dtype == torch.bfloat16 and torch.isfinite(embed16.float()).all()
    rounded = want_embed.to(torch.bfloat16).double()
    ulp = 2.0 ** (torch.floor(torch.log2(rounded.abs().clamp_min(2.0 ** -126))) - 7)
    assert ((embed16.double() - rounded).abs() <= ulp).all()
    if K > 1:
        assert torch.equal(ref[0, 1], torch.ones(4, device=DEV)) and torch.equal(ref[1, 1], torch.zeros(4, device=DEV))
        assert torch.equal(embed[0, 1], embed[0, 2]) and torch.equal(ref[1, 1], ref[1, 3])   # duplicates give identical rows


def test_proposal_queries_guards_indices_topk_cannot_produce(query_case):
    coords = query_case.to(DEV)
    topk = torch.tensor([[-1, 163, 2 ** 40], [3, -2 ** 40, 162]], device=DEV)
    ref, embed = alo_hip.proposal_queries(coords, topk, torch.float32)
    torch.cuda.synchronize()
    bad = torch.tensor([[True, True, True], [False, True, False]], device=DEV)
    assert torch.equal(ref[bad], torch.full((4, 4), 0.5, device=DEV))        # read as a row of zeros
    assert (ref[~bad] - coords[1, [3, 162]].sigmoid()).abs().max().item() <= 1e-6
    assert torch.isfinite(embed).all()


def test_fast_path_equals_torch_path(golden, monkeypatch):
    """Under no_grad the kernels run; with them switched off the same module selects the same tokens and agrees within the
    fp32 bar."""
    g, tr, (srcs, masks, poss), L = _g19_on_gpu(golden)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        fast = tr(srcs, masks, poss, None)
    assert all(_ran(timer).values()), _ran(timer)
    for name in KERNEL_TAGS:
        monkeypatch.setattr(alo_hip, name + "_supported", lambda *a, **k: False)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        slow = tr(srcs, masks, poss, None)
    assert not any(_any_kernel_ran(timer).values()), _any_kernel_ran(timer)
    _check_against_g19(slow, g, L, FP32_TOL)
    assert torch.equal(torch.topk(fast["enc_outputs_class"][..., 0], 12, dim=1)[1], torch.topk(slow["enc_outputs_class"][..., 0], 12, dim=1)[1])
    assert torch.equal(torch.isposinf(fast["enc_outputs_coord_unact"]), torch.isposinf(slow["enc_outputs_coord_unact"]))
    for key in ("enc_outputs_class", "init_reference_out", "hs", "inter_references_out"):
        assert (fast[key] - slow[key]).abs().max().item() <= FP32_TOL, key
    finite = torch.isfinite(slow["enc_outputs_coord_unact"])
    assert (fast["enc_outputs_coord_unact"][finite] - slow["enc_outputs_coord_unact"][finite]).abs().max().item() <= FP32_TOL


def test_two_stage_model_graph_capture_replays_the_eager_forward():
    """GraphedForward captures the two-stage forward (nothing in it synchronises with the host) and replays it on fresh inputs."""
    import aloscene
    from alonet.common import GraphedForward
    from helpers import formula_state_dict

    model = build_two_stage_detr(device=torch.device(DEV)).eval()
    model.load_state_dict(formula_state_dict(model.state_dict()))
    gen = torch.Generator().manual_seed(5)

    def batch(pad):
        fr = [aloscene.Frame(torch.rand(3, 64 - pad * i, 96, generator=gen) * 255, normalization="255").norm_resnet() for i in range(2)]
        return aloscene.Frame.batch_list(fr).to(DEV)

    first, second = batch(0), batch(16)
    assert first.shape == second.shape and bool(second.mask.as_tensor().any()) and not bool(first.mask.as_tensor().any())
    graphed = GraphedForward(model)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        want = model(first)
    assert all(_ran(timer).values()), _ran(timer)
    with torch.no_grad():
        for frames in (first, second, first):
            want = model(frames)
            got = graphed(frames)
            assert want["enc_outputs_class"].shape == (2, 128, 5) and want["enc_outputs_coord"].shape == (2, 128, 4)
            for key in ("pred_logits", "pred_boxes", "enc_outputs_class", "enc_outputs_coord"):
                assert torch.equal(got[key], want[key]), key
    assert len(graphed._graphs) == 1


def test_two_stage_training_step_runs_on_the_torch_formulation(golden):
    g, tr, (srcs, masks, poss), L = _g19_on_gpu(golden)
    tr.train()
    srcs = [s.requires_grad_(True) for s in srcs]
    with alo_hip.LaunchTimer() as timer:
        out = tr(srcs, masks, poss, None)
        assert not out["init_reference_out"].requires_grad and out["init_reference_out"].grad_fn is None   # detached proposals
        assert not out["inter_references_out"].requires_grad
        finite = torch.isfinite(out["enc_outputs_coord_unact"])
        loss = out["hs"].square().mean() + out["enc_outputs_class"].square().mean() + out["enc_outputs_coord_unact"][finite].square().mean()
        loss.backward()
    assert not any(_any_kernel_ran(timer).values()), _any_kernel_ran(timer)
    for p in (tr.enc_output.weight, tr.pos_trans.weight, tr.enc_output_norm.weight, tr.pos_trans_norm.bias, tr.level_embed, srcs[0]):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    assert all(torch.isfinite(p.grad).all() for p in tr.parameters() if p.grad is not None)
