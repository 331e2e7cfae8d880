"""The fp64 references and bounds of test_glue_kernels_gpu.py (tests/kernel_bounds.py), checked without a GPU: every
re-implementation is pinned to the stock module it stands for, and the stock fp32 op alone stays inside the bound the HIP kernel is
held to (a bound the stock op missed would be a statement about the bound, not about the kernel)."""
import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb
from kernel_bounds import compare


@pytest.mark.parametrize("normalize,center", [(True, True), (True, False), (False, False)])
def test_pos_sine_ref_is_the_module_plus_level_embed(normalize, center):
    """PositionEmbeddingSine (fp32) per level -> flatten -> + level_embed -> cat against pos_sine_ref, inside the fp32 bound: a
    reference with the blocks, the sin / cos interleave or the centre / normalise arithmetic wrong misses it by O(1)."""
    from alonet.transformers import PositionEmbeddingSine

    shapes = [(13, 70), (7, 11), (4, 6), (2, 3)]
    b, nf = 8, 32
    enc = PositionEmbeddingSine(nf, normalize=normalize, center=center)
    level_embed = torch.randn(len(shapes), 2 * nf, generator=torch.Generator().manual_seed(0))
    kinds = ["none", "right", "bottom", "corner", "scatter", "all", "cross", "scatter+right"]
    mask_flat = kb.pyramid_masks(b, shapes, kinds, "cpu", seed=1)
    want, s0 = [], 0
    for lvl, (h, w) in enumerate(shapes):
        m = mask_flat[:, s0:s0 + h * w].view(b, 1, h, w)
        s0 += h * w
        want.append(enc((torch.empty(b, 1, h, w), m)).flatten(2).transpose(1, 2) + level_embed[lvl].view(1, 1, -1))
    want = torch.cat(want, 1)
    ref, p = kb.pos_sine_ref(mask_flat, shapes, enc.dim_t(torch.device("cpu")), level_embed, normalize, center, enc.scale)
    assert ref.shape == want.shape == (b, sum(h * w for h, w in shapes), 2 * nf)
    assert mask_flat[5].all() and not mask_flat[0].any() and torch.isfinite(ref).all()
    assert p.abs().max().item() > (60 if not normalize else 6)     # the arguments the bound scales with are really there
    ratio = compare(want, ref, kb.pos_sine_bound(ref, p), "PositionEmbeddingSine (fp32, CPU)")
    print(f"stock fp32 chain on the CPU: worst error / bound = {ratio:.3g}")


def test_pyramid_masks_hold_the_cases_they_name():
    m = kb.pyramid_masks(7, [(6, 9)], ["none", "right", "bottom", "corner", "scatter", "all", "cross"], "cpu", seed=3).view(7, 6, 9)
    assert not m[0].any() and m[1, :, 6:].all() and not m[1, :, :6].any() and m[2, 3:].all() and not m[2, :3].any()
    assert m[3, 3:].all() and m[3, :, 6:].all() and not m[3, :3, :6].any() and m[5].all()
    assert m[6, 3].all() and m[6, :, 4].all() and int(m[6].sum()) == 9 + 6 - 1
    rows = (~m[4]).cumsum(1)
    assert 0 < int(m[4].sum()) < 54 and not torch.equal(rows, torch.arange(1, 10).expand(6, 9))   # not a rectangle


def test_gru_refs_are_the_gru_step_of_the_update_block():
    """gru_gate_ref -> gru_update_ref against alonet.raft.update._gru_step in fp64, with the three convolutions replaced by fixed
    maps of their input (the q map reads the r * h channels, so a reference that gated the wrong operand would differ)."""
    from alonet.raft.update import _gru_step

    g = torch.Generator().manual_seed(2)
    b, c, cx, hh, ww = 2, 6, 5, 3, 4
    h = torch.randn(b, c, hh, ww, generator=g, dtype=torch.float64)
    x = torch.randn(b, cx, hh, ww, generator=g, dtype=torch.float64)
    wz, wr, wq = (torch.randn(c, c + cx, 1, 1, generator=g, dtype=torch.float64) for _ in range(3))
    bz, br, bq = (torch.randn(c, generator=g, dtype=torch.float64) for _ in range(3))
    want = _gru_step(h, x, lambda t: F.conv2d(t, wz, bz), lambda t: F.conv2d(t, wr, br), lambda t: F.conv2d(t, wq, bq))
    hx = torch.cat([h, x], 1)
    zr = torch.cat([F.conv2d(hx, wz), F.conv2d(hx, wr)], 1)            # bias-free pre-activations, as the fused path has them
    z, rh = kb.gru_gate_ref(zr, torch.cat([bz, br]), h)
    got = kb.gru_update_ref(F.conv2d(torch.cat([rh, x], 1), wq), bq, z, h)
    assert (got - want).abs().max().item() <= 1e-14


@pytest.mark.parametrize("c", [256, 260, 1024])
def test_stock_layer_norm_fp32_stays_inside_the_layernorm_bound(c):
    """F.layer_norm in fp32 against fp64 on the rows the GPU test draws (mean = 1000 x std and constant rows included)."""
    x, res, gamma, beta, kind = kb.layernorm_inputs(4099, c, "cpu", seed=c, ill=True)
    v = x + res
    stats = v.double()
    ratio_ms = (stats.mean(-1).abs() / stats.std(-1).clamp_min(1e-30))
    well = kind == 0
    assert (ratio_ms[kind == 1] > 800).all() and (stats[kind == 2].var(-1, unbiased=False) == 0).all() and (ratio_ms[well] <= 1).all()
    assert int((kind == 1).sum()) > 400 and int((kind == 2).sum()) > 300
    ref, bound = kb.layernorm_ref_and_bound(v, gamma, beta, 1e-5)
    assert (ref[kind == 2] == beta.double()).all()                    # a constant row normalises to beta exactly
    got = F.layer_norm(v, (c,), gamma, beta, 1e-5)
    ratio = compare(got, ref, bound, f"F.layer_norm fp32 C={c}")
    assert (got[well].double() - ref[well]).abs().max().item() <= 2e-5   # the absolute figure of test_fused_gpu.py
    print(f"F.layer_norm fp32 (CPU), C = {c}: worst error / bound = {ratio:.3g}, "
          f"bound on the mean = 1000 x std rows up to {bound[kind == 1].max().item():.3g}")


def test_layernorm_ref_gives_nan_rows_for_non_finite_inputs():
    x, res, gamma, beta, _ = kb.layernorm_inputs(9, 256, "cpu", seed=1)
    x[2, 5], x[4, 0], x[7, 255] = kb.NAN, kb.INF, -kb.INF
    ref, _ = kb.layernorm_ref_and_bound(x + res, gamma, beta, 1e-5)
    stock = F.layer_norm(x + res, (256,), gamma, beta, 1e-5)
    bad = torch.tensor([False, False, True, False, True, False, False, True, False])
    assert torch.equal(torch.isnan(ref).all(-1), bad) and torch.equal(torch.isnan(ref).any(-1), bad)
    assert torch.equal(torch.isnan(stock), torch.isnan(ref))


@pytest.mark.parametrize("n,c,hw,groups", [(2, 256, 2049, 32), (3, 16, 700, 8), (2, 32, 513, 8), (2, 64, 300, 8)])
def test_stock_group_norm_fp32_stays_inside_the_groupnorm_bound(n, c, hw, groups):
    """F.group_norm in fp32 against fp64 on bf16 groups with mean / std in {0.25, 16, 100} and a constant group."""
    x = kb.groupnorm_ill_inputs(n, c, hw, groups, "cpu", seed=c + hw)
    per = x.double().view(n, groups, -1)
    r = per.mean(-1).abs() / per.std(-1).clamp_min(1e-30)
    assert (r[:, 1::4] > 12).all() and (r[:, 2::4] > 60).all() and (per[:, 3::4].var(-1, unbiased=False) == 0).all()
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.randn(c, generator=g).bfloat16(), torch.randn(c, generator=g).bfloat16()
    for relu in (False, True):
        ref, bound = kb.groupnorm_ref_and_bound(x, groups, gamma, beta, 1e-5, relu)
        got = F.group_norm(x.float(), groups, gamma.float(), beta.float(), 1e-5)
        ratio = compare(torch.relu(got) if relu else got, ref, bound, f"F.group_norm fp32 relu={relu}")
        assert ratio < 0.5    # the stock fp32 op never needs the bf16 half-ulp the bound carries for the kernel's rounding
    const = ref.view(n, groups, c // groups, hw)[:, 3::4]
    assert torch.equal(const, torch.relu(beta.double()).view(1, groups, -1, 1)[:, 3::4].expand_as(const))


def test_groupnorm_ref_spreads_a_non_finite_value_over_its_group_only():
    x = kb.groupnorm_ill_inputs(2, 32, 50, 8, "cpu", seed=1)
    gamma, beta = torch.ones(32).bfloat16(), torch.zeros(32).bfloat16()
    for v in (kb.NAN, kb.INF):
        y = x.clone()
        y[1, 9, 7] = v                                                # group 2 of image 1
        for relu in (False, True):
            ref, _ = kb.groupnorm_ref_and_bound(y, 8, gamma, beta, 1e-5, relu)
            nan = torch.isnan(ref).view(2, 8, -1)
            want = torch.zeros(2, 8, dtype=torch.bool)
            want[1, 2] = True
            assert torch.equal(nan.all(-1), want) and torch.equal(nan.any(-1), want)
            stock = F.group_norm(y.float(), 8, gamma.float(), beta.float(), 1e-5)
            assert torch.equal(torch.isnan(torch.relu(stock) if relu else stock), torch.isnan(ref))


def test_panoptic_chain_helpers_are_the_stock_chain_and_differ_from_fp64_only_at_near_ties():
    """panoptic_probabilities + panoptic_onehot_from in fp32 is the chain of detr_panoptic.py (test_fused_gpu.py spells it out);
    against the same chain in fp64 it may decide differently only where panoptic_near_tie says so.  F.threshold keeps NaN and
    argmax takes the first NaN for the maximum: a NaN probability selects its query."""
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(2, 7, 20, 33, generator=g) * 3
    logits[:, :, :6] -= 6.0
    size = (80, 131)
    m = F.threshold(F.interpolate(logits, size=size, mode="bilinear", align_corners=False).sigmoid(), 0.5, 0.0)
    for b in range(2):
        nothing = (~m[b].bool()).all(dim=0, keepdim=True)
        onehot = torch.zeros_like(m[b])
        onehot.scatter_(0, m[b].argmax(dim=0, keepdim=True), 1)
        want = onehot.long() * (~nothing)
        got = kb.panoptic_onehot_from(kb.panoptic_probabilities(logits[b], size, 0.5))
        assert torch.equal(got, want) and bool((want.sum(0) == 0).any()) and bool((want.sum(0) == 1).any())
        got64 = kb.panoptic_onehot_from(kb.panoptic_probabilities(logits[b].double(), size, 0.5))
        differ = (got != got64).any(0)
        assert not (differ & ~kb.panoptic_near_tie(logits[b], size, 0.5)).any()
        assert (got != got64).float().mean().item() <= 1e-5
    masks = torch.tensor([[[0.7]], [[kb.NAN]], [[kb.NAN]], [[0.9]]])
    assert torch.isnan(F.threshold(torch.tensor([kb.NAN]), 0.5, 0.0)).all()
    assert kb.panoptic_onehot_from(masks).flatten().tolist() == [0, 1, 0, 0]


def test_compare_rejects_what_it_is_there_to_reject():
    ref = torch.tensor([1.0, kb.NAN, kb.INF, 2.0], dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    assert compare(torch.tensor([1.0005, kb.NAN, kb.INF, 2.0]), ref, bound, "ok") == pytest.approx(0.5, rel=1e-3)
    for bad in ([1.002, kb.NAN, kb.INF, 2.0], [1.0, 0.0, kb.INF, 2.0], [1.0, kb.NAN, -kb.INF, 2.0], [1.0, kb.NAN, kb.NAN, 2.0],
                [1.0, kb.NAN, kb.INF, kb.NAN]):
        with pytest.raises(AssertionError):
            compare(torch.tensor(bad), ref, bound, "bad")
