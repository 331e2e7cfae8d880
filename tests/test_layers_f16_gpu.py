"""The transformer's layer kernels in fp16 (storage fp16, arithmetic fp32, one rounding to nearest even per stored result).

Every kernel-level reference is computed in fp64 from the kernel's own fp16 operands (fp16 -> fp64 is exact), and every output
element is held to the bound of tests/test_backbone_kernels_gpu.py with the rounding term swapped:

    |got - ref| <= 2^-11 |ref| + 2^-24 + c(K) * A,        c(K) = (K + 1) * 2^-23  (kernel_bounds.c_acc),

A being the same operation on |x|, |w|, |b| in fp64.  2^-11 |ref| is half an ulp of the fp16 result (11 significant bits), 2^-24 one
subnormal spacing of it (a result below 2^-14 is rounded to a multiple of 2^-24).  c(K) * A covers the fp32 accumulation in any order:
products of two fp16 values carry 22 significant bits and an exponent >= 2^-48, so they are exact in fp32.  A residual epilogue rounds
x W^T + b to fp16 before it adds the identity, which adds 2^-11 |x W^T + b|.  Operands are drawn without fp16 subnormals (magnitudes
below 2^-14 are zeroed): whether the fp16 MFMA honours subnormal operands is outside this bound.

The model-level tests check which launches an fp16 model makes: the layer kernels, no separate head-major pass, no bf16-only kernel.
"""
import numpy as np
import pytest
import torch

import alo_hip
import kernel_bounds as kb
from kernel_bounds import _finite_abs, c_acc, compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
NAN = float("nan")
RND, TINY = 2.0 ** -11, 2.0 ** -24     # half an ulp of an fp16 result (relative); one fp16 subnormal spacing


def h16(t):
    """``t`` as fp16 with no subnormal: magnitudes below 2^-14 become zero."""
    t = t.to(F16)
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randh(g, *shape, scale=1.0):
    return h16(torch.randn(*shape, device=DEV, generator=g) * scale)


def linear_ref_and_bound(x2, w, b, relu, residual):
    """act(x2 @ w^T + b [+ residual]) in fp64 and the bound of the module docstring.  x2 (M, K), w (N, K), residual (M, N)."""
    k = x2.shape[1]
    w64 = w.double()
    b64 = b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=x2.device)
    pre = x2.double() @ w64.t() + b64
    amag = _finite_abs(x2) @ w64.abs().t() + b64.abs()
    ref = pre if residual is None else pre + residual.double()
    if relu:
        ref = torch.relu(ref)
    bound = RND * ref.abs() + TINY + c_acc(k) * amag
    if residual is not None:
        bound = bound + RND * torch.nan_to_num(pre.abs(), nan=0.0, posinf=0.0)
    return ref, bound


def tags_of(timer):
    return set(tag.split("/")[0] for tag in timer.summary())


# ---- linear_shortk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(64, 64), (320, 128), (768, 256)])
@pytest.mark.parametrize("rows", [1, 65, 129, 300])
def test_linear_shortk_fp16(rows, n, k):
    g = gen(rows * 1000 + n + k)
    x, w, b = randh(g, rows, k), randh(g, n, k, scale=k ** -0.5), randh(g, n, scale=0.5)
    res = randh(g, rows, n)
    assert alo_hip.linear_shortk_supported(x, w, f16=True) and not alo_hip.linear_shortk_supported(x, w.bfloat16(), f16=True)
    assert not alo_hip.linear_shortk_supported(x, w)     # fp16 is opt-in: a caller that does not ask keeps its bf16 answer
    worst = 0.0
    for bias in (b, None):
        for relu in (False, True):
            for r in (None, res):
                got = alo_hip.linear_shortk(x, w, bias, relu, residual=r)
                assert got.shape == (rows, n) and got.dtype == F16
                ref, bound = linear_ref_and_bound(x, w, bias, relu, r)
                worst = max(worst, compare(got, ref, bound, f"linear_shortk fp16 {rows, n, k} bias={bias is not None} relu={relu} res={r is not None}"))
    print(f"linear_shortk fp16 rows={rows} N={n} K={k}: worst error / bound = {worst:.3g}")
    # linear_auto picks the same kernel, leading dimensions are kept
    with alo_hip.LaunchTimer() as timer:
        auto = alo_hip.linear_auto(x, w, b, True, residual=res)
    assert tags_of(timer) == {"linear_shortk"}
    assert torch.equal(auto, alo_hip.linear_shortk(x, w, b, True, residual=res))
    if rows % 3 == 0:
        got3 = alo_hip.linear_auto(x.view(3, rows // 3, k), w, b)
        assert got3.shape == (3, rows // 3, n) and torch.equal(got3.reshape(rows, n), alo_hip.linear_shortk(x, w, b))


def test_linear_shortk_fp16_range_and_nan():
    """Results beyond the fp16 range become the infinity of their sign (as ``.half()`` of the fp64 result gives: no clamp), results
    inside it stay within the bound; NaN in gives NaN out under the ReLU."""
    g = gen(7)
    rows, n, k = 130, 64, 64
    x, w, b = randh(g, rows, k), randh(g, n, k, scale=0.5), randh(g, n, scale=0.5)
    w[:, 0] = 4.0
    beyond = {3: 60000.0, 64: -60000.0, 129: 60000.0}       # 4 x 60000 = 2.4e5, the other 63 products sum to a few units
    inside = {5: 7000.0, 65: -7000.0, 128: 7000.0}          # 2.8e4
    for r, v in {**beyond, **inside}.items():
        x[r, 0] = v
    got = alo_hip.linear_shortk(x, w, b, False)
    ref, bound = linear_ref_and_bound(x, w, b, False, None)
    far, near = sorted(beyond), sorted(inside)
    assert (ref[far].abs() >= 1e5).all() and (ref[near].abs() <= 3e4).all() and (ref[near].abs() >= 2e4).all()
    assert torch.isinf(got[far]).all() and torch.equal(got[far], ref[far].to(F16))          # the reference's infinity, with its sign
    assert torch.equal(torch.sign(got[far][:, 0]).cpu(), torch.tensor([1.0, -1.0, 1.0], dtype=F16))
    finite = torch.ones(rows, dtype=torch.bool, device=DEV)
    finite[far] = False
    assert torch.isfinite(got[finite]).all()
    compare(got[finite], ref[finite], bound[finite], "linear_shortk fp16 inside the range")
    x[7, 9] = NAN
    got = alo_hip.linear_shortk(x, w, b, True)
    assert torch.isnan(got[7]).all() and not torch.isnan(got[8]).any()
    assert (got[64] == 0).all() and torch.isposinf(got[3]).all()                           # relu(-inf) = 0, relu(+inf) = +inf


# ---- linear_packed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(512, 128), (1024, 384)])
@pytest.mark.parametrize("rows", [1, 77, 130])
def test_linear_packed_fp16(rows, k, n):
    g = gen(rows * 1000 + n + k)
    x, w, b = randh(g, rows, k), randh(g, n, k, scale=k ** -0.5), randh(g, n, scale=0.5)
    res = randh(g, rows, n)
    worst = 0.0
    with torch.no_grad():
        assert alo_hip.linear_packed_supported(x, w, f16=True) and not alo_hip.linear_packed_supported(x, w.bfloat16(), f16=True)
        assert not alo_hip.linear_packed_supported(x, w)
        for relu in (False, True):
            for r in (None, res):
                got = alo_hip.linear_packed(x, w, b, relu, residual=r)
                assert got.shape == (rows, n) and got.dtype == F16
                ref, bound = linear_ref_and_bound(x, w, b, relu, r)
                worst = max(worst, compare(got, ref, bound, f"linear_packed fp16 {rows, k, n} relu={relu} res={r is not None}"))
    print(f"linear_packed fp16 rows={rows} K={k} N={n}: worst error / bound = {worst:.3g}")


# ---- ffn256 ------------------------------------------------------------------------------------------------------------------
def ulp16_at(v):
    """Spacing of the fp16 values at magnitude ``v`` (fp64 tensor): 2^(floor(log2 v) - 10), at least the subnormal spacing 2^-24."""
    return torch.maximum(2.0 ** (torch.floor(torch.log2(v.clamp_min(2.0 ** -30))) - 10), torch.full_like(v, TINY))


def ffn_ref_and_bound(x, w1, b1, w2, b2):
    """The two-step reference, the hidden activation rounded to fp16 in between as the two-launch path stores it, and its bound:

      * the kernel's hidden value before rounding, h', is within e = c(256) * A1 of the exact h (fp32 accumulation);
      * rounding is monotone, so fp16(h') lies between fp16(h - e) and fp16(h + e): it differs from fp16(h) by at most
        d = e + ulp(|fp16(h)| + e), i.e. the hidden elements that round the other way move by one fp16 ulp (plus e where e exceeds it);
      * that moves the output by at most sum_j |w2[., j]| d_j; the second product's own fp32 accumulation adds c(F) * A2 over the
        operands it really sees (|fp16(h)| + d), and the result is rounded once: 2^-11 |ref| + 2^-24."""
    x64, w1d, w2d = x.double(), w1.double(), w2.double()
    b1d = b1.double() if b1 is not None else torch.zeros(w1.shape[0], dtype=torch.float64, device=x.device)
    b2d = b2.double() if b2 is not None else torch.zeros(256, dtype=torch.float64, device=x.device)
    hid = torch.relu(x64 @ w1d.t() + b1d).to(F16).double()
    e = c_acc(256) * (x64.abs() @ w1d.abs().t() + b1d.abs())
    d = e + ulp16_at(hid + e)
    ref = hid @ w2d.t() + b2d
    amag = (hid + d) @ w2d.abs().t() + b2d.abs()
    return ref, RND * ref.abs() + TINY + c_acc(w1.shape[0]) * amag + d @ w2d.abs().t()


@pytest.mark.parametrize("fh", [256, 1024])
@pytest.mark.parametrize("rows", [1, 65, 130])
def test_ffn256_fp16(rows, fh):
    g = gen(rows + fh)
    x = randh(g, rows, 256)
    w1, w2 = randh(g, fh, 256, scale=0.06), randh(g, 256, fh, scale=0.03)
    b1, b2 = randh(g, fh), randh(g, 256)
    assert alo_hip.ffn256_supported(x, w1, w2, f16=True) and not alo_hip.ffn256_supported(x, w1.bfloat16(), w2, f16=True)
    assert not alo_hip.ffn256_supported(x, w1, w2)
    first = alo_hip.ffn256(x, w1, b1, w2, b2).clone()
    for bias1, bias2 in ((b1, b2), (None, None)):
        got = alo_hip.ffn256(x, w1, bias1, w2, bias2)
        assert got.shape == x.shape and got.dtype == F16
        ref, bound = ffn_ref_and_bound(x, w1, bias1, w2, bias2)
        worst = compare(got, ref, bound, f"ffn256 fp16 rows={rows} F={fh} bias={bias1 is not None}")
        print(f"ffn256 fp16 rows={rows} F={fh} bias={bias1 is not None}: worst error / bound = {worst:.3g}, "
              f"median bound {bound.median().item():.3g}")
    # the packed copy follows an in-place weight update
    with torch.no_grad():
        w1.copy_(h16(w1.float() * 0.5))
    again = alo_hip.ffn256(x, w1, b1, w2, b2)
    ref2, bound2 = ffn_ref_and_bound(x, w1, b1, w2, b2)
    compare(again, ref2, bound2, "ffn256 fp16 after an in-place weight update")
    assert not torch.equal(again, first)


# ---- value_proj_head_major ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,heads,K", [(3, 301, 4, 128), (1, 64, 2, 64)])
def test_value_proj_head_major_fp16_equals_linear_then_relayout(N, S, heads, K):
    g = gen(N + S + K)
    x, w, b = randh(g, N, S, K), randh(g, heads * 32, K, scale=0.1), randh(g, heads * 32)
    mask = torch.rand(N, S, device=DEV, generator=g) < 0.25
    mask[0, 0], mask[-1, -1] = True, False
    assert alo_hip.value_proj_head_major_supported(x, w, heads, f16=True) and not alo_hip.value_proj_head_major_supported(x, w, heads)
    for m in (mask, None):
        got = alo_hip.value_proj_head_major(x, w, b, m, heads)
        two_step = alo_hip.value_head_major(alo_hip.linear_shortk(x, w, b).view(N, S, heads, 32), m)
        assert got.shape == (N, heads, S, 32) and got.dtype == F16 and torch.equal(got, two_step)
    got = alo_hip.value_proj_head_major(x, w, b, mask, heads)
    assert float(got.permute(0, 2, 1, 3)[mask].abs().max()) == 0.0
    assert float(got.permute(0, 2, 1, 3)[~mask].abs().max()) > 0.0


# ---- add_layernorm -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 256, 264, 1024])
@pytest.mark.parametrize("rows", [1, 7, 33])
def test_add_layernorm_fp16(rows, c):
    """Well- and ill-conditioned rows (mean = 1000 x std, constant rows): the fp32 bound of kernel_bounds.layernorm_ref_and_bound on
    v = x + res as the kernel forms it (fp32), plus the one rounding of the result to fp16."""
    x, res, gamma, beta, _ = kb.layernorm_inputs(rows, c, DEV, seed=rows * 7 + c, ill=True)
    x, res, gamma, beta = h16(x), h16(res), h16(gamma), h16(beta)
    pos = randh(gen(rows + c), rows, c)
    assert alo_hip.add_layernorm_supported(x) and alo_hip.fusable(x, f16=True) and not alo_hip.fusable(x)
    for with_res in (True, False):
        for with_pos in (True, False):
            r = res if with_res else None
            got = alo_hip.add_layernorm(x, r, gamma, beta, 1e-5, pos=pos if with_pos else None)
            if with_pos:
                assert torch.equal(got[1], got[0] + pos)     # computed from the rounded `out`, as the unfused `out + pos`
                got = got[0]
            assert got.dtype == F16 and got.shape == x.shape
            v = x.float() + r.float() if with_res else x.float()
            ref, bound = kb.layernorm_ref_and_bound(v, gamma.float(), beta.float(), 1e-5, bf16=False)
            compare(got, ref, bound + RND * ref.abs() + TINY, f"add_layernorm fp16 rows={rows} C={c} res={with_res} pos={with_pos}")


# ---- bias_act ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu,with_res", [(True, False), (True, True), (False, False), (False, True)])
def test_bias_act_fp16(relu, with_res):
    """x + bias (+ residual) in fp32 (at most two additions: 2^-22 of the magnitudes), one rounding to fp16; NaN kept by the ReLU."""
    g = gen(31 + 2 * relu + with_res)
    x = randh(g, 2, 64, 9, 11).contiguous(memory_format=torch.channels_last)
    bias = randh(g, 64)
    r = randh(g, 2, 64, 9, 11).contiguous(memory_format=torch.channels_last) if with_res else None
    x[1, 3, 2, 5] = NAN
    want = x.double() + bias.double().view(1, -1, 1, 1) + (r.double() if with_res else 0)
    want = torch.relu(want) if relu else want
    amag = _finite_abs(x) + bias.double().abs().view(1, -1, 1, 1) + (_finite_abs(r) if with_res else 0)
    got = alo_hip.bias_act_(x.clone(memory_format=torch.preserve_format), bias, r, relu)
    assert got.dtype == F16 and torch.isnan(got[1, 3, 2, 5])
    compare(got, want, RND * want.abs() + TINY + 2.0 ** -22 * amag, f"bias_act fp16 relu={relu} res={with_res}")
    rows = randh(g, 33, 64)
    got2 = alo_hip.bias_act_(rows.clone(), bias, None, relu)
    want2 = rows.double() + bias.double()
    compare(got2, torch.relu(want2) if relu else want2, RND * want2.abs() + TINY + 2.0 ** -22 * (rows.double().abs() + bias.double().abs()),
            "bias_act fp16 matrix")


# ---- pos_sine_flat -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize,center", [(True, True), (True, False), (False, False)])
def test_pos_sine_flat_fp16(normalize, center):
    from alonet.transformers import PositionEmbeddingSine

    shapes, b, nf = [(12, 17), (6, 9), (3, 5), (2, 3)], 3, 128
    enc = PositionEmbeddingSine(nf, normalize=normalize, center=center)
    level_embed = randh(gen(5), len(shapes), 2 * nf)
    mask_flat = kb.pyramid_masks(b, shapes, ["none", "corner", "scatter"], DEV, seed=5)
    sh = torch.tensor(shapes, dtype=torch.int32, device=DEV)
    sizes = [h * w for h, w in shapes]
    start = torch.tensor([sum(sizes[:i]) for i in range(len(sizes))], dtype=torch.int32, device=DEV)
    dim_t = enc.dim_t(torch.device(DEV))
    got = alo_hip.pos_sine_flat(mask_flat, sh, start, dim_t, level_embed, normalize, center, enc.scale, F16)
    assert got.shape == (b, sum(sizes), 2 * nf) and got.dtype == F16
    ref, p = kb.pos_sine_ref(mask_flat, shapes, dim_t, level_embed, normalize, center, enc.scale)
    worst = compare(got, ref, kb.pos_sine_bound(ref, p) + RND * ref.abs() + TINY, "pos_sine_flat fp16")
    print(f"pos_sine_flat fp16 norm={normalize} center={center}: worst error / bound = {worst:.3g}")


# ---- two-stage glue ----------------------------------------------------------------------------------------------------------
def _pyramid_mask(shapes, b, seed):
    rng = np.random.default_rng(seed)
    levels = []
    for hh, ww in shapes:
        m = np.zeros((b, hh, ww), bool)
        for i in range(1, b):
            m[i, int(rng.integers(1, hh + 1)):, :] = True
            m[i, :, int(rng.integers(1, ww + 1)):] = True
        levels.append(m.reshape(b, -1))
    return torch.from_numpy(np.concatenate(levels, 1)).to(DEV)


@pytest.mark.parametrize("C", [8, 256])
def test_two_stage_row_copies_fp16_are_bit_exact(C):
    from alonet.deformable_detr.deformable_transformer import encoder_output_proposals

    shapes = [(12, 10), (6, 5), (3, 3), (2, 2)]
    mask = _pyramid_mask(shapes, 3, seed=C)
    memory = torch.randn(3, mask.shape[1], C, generator=torch.Generator().manual_seed(C)).to(DEV, F16)
    memory[-1, -1, 0], memory[0, 0, -1], memory[0, 1, 0] = NAN, float("inf"), 2.0 ** -20      # a subnormal is copied like any bits
    keep = torch.rand(3, mask.shape[1], device=DEV, generator=gen(C)) < 0.6
    assert alo_hip.mask_rows_supported(memory, keep, f16=True) and not alo_hip.mask_rows_supported(memory, keep)
    got = alo_hip.mask_rows(memory, keep)
    assert got.dtype == F16 and torch.equal(got.view(torch.int16), memory.masked_fill(~keep.unsqueeze(-1), 0.0).view(torch.int16))
    assert alo_hip.encoder_proposals_masked_supported(mask, shapes, memory, f16=True)
    proposals, pkeep = alo_hip.encoder_proposals(mask, shapes)
    got_p, got_k, got_m = alo_hip.encoder_proposals_masked(mask, shapes, memory)
    assert torch.equal(got_k, pkeep) and torch.equal(got_k, encoder_output_proposals(mask, shapes)[1])
    assert torch.equal(got_p.view(torch.int32), proposals.view(torch.int32))
    assert got_m.dtype == F16 and torch.equal(got_m.view(torch.int16), memory.masked_fill(~got_k.unsqueeze(-1), 0.0).view(torch.int16))


@pytest.mark.parametrize("K", [1, 12, 300])
def test_proposal_queries_fp16_vs_the_double_evaluation(K):
    from alonet.deformable_detr.deformable_transformer import proposal_pos_embed

    S = 163
    coords = torch.randn(2, S, 4, generator=torch.Generator().manual_seed(19)) * 3
    coords[0, 5], coords[1, 7] = float("inf"), float("-inf")
    coords = coords.to(DEV)
    topk = torch.randint(0, S, (2, K), generator=torch.Generator().manual_seed(K))
    topk[:, 0] = torch.tensor([5, 7])
    topk = topk.to(DEV)
    assert alo_hip.proposal_queries_supported(coords, topk, F16, f16=True) and not alo_hip.proposal_queries_supported(coords, topk, F16)
    picked = torch.gather(coords.double(), 1, topk.unsqueeze(-1).expand(-1, -1, 4))
    want = proposal_pos_embed(picked)
    ref32, _ = alo_hip.proposal_queries(coords, topk, torch.float32)
    ref, embed = alo_hip.proposal_queries(coords, topk, F16)
    assert torch.equal(ref, ref32) and embed.dtype == F16 and embed.shape == (2, K, 512)
    compare(embed, want, RND * want.abs() + TINY, f"proposal_queries fp16 K={K}")
    torch_f16 = proposal_pos_embed(picked.float()).to(F16)          # the torch formulation in fp16: its fp32 angle costs more than the rounding
    assert (embed.double() - torch_f16.double()).abs().max().item() <= 2e-5 + 2 * RND   # two roundings of values <= 1, either way


# ---- models ------------------------------------------------------------------------------------------------------------------
def test_g12_transformer_fp16_runs_on_the_layer_kernels(golden):
    """d_model 256, 8 heads x 32, L = P = 4 in fp16: the route of the bf16 model (merged query projection + value_proj_head_major,
    the head-major attention kernel, output projection; FFN and residual + LayerNorm in one kernel each), no separate head-major
    pass, and not the bf16-only encoder block.  Outputs at the bf16 bar of tests/test_models_gpu.py."""
    from test_models_f16_gpu import _transformer_errors
    from test_models_gpu import BF16_TRANSFORMER_TOL

    errs, tags = _transformer_errors(golden("g12_deformable_transformer_d256.npz"), F16)
    print("G12 fp16 max-abs vs the reference:", errs, "launches:", sorted(tags))
    assert {"linear_shortk", "ffn256", "add_layernorm", "value_proj_hm", "msda_fwd_fused"} <= tags, tags
    assert "value_head_major" not in tags and not any(tag.startswith("encoder_block") for tag in tags), tags
    assert max(errs.values()) <= BF16_TRANSFORMER_TOL, errs


def test_g19_two_stage_transformer_fp16_runs_on_the_glue_kernels(golden, monkeypatch):
    """The two-stage transformer in fp16: proposals + row masking and the decoder queries on the two-stage kernels.  As in the bf16
    test of tests/test_two_stage_gpu.py the fixture's selection is imposed on ``torch.topk`` (the smallest gap between G19's ranked
    logits, 0.0018, is below what 11 significant bits keep through the encoder) and the rest is held to the bf16 bar."""
    from test_models_gpu import BF16_TRANSFORMER_TOL
    from test_two_stage_cpu import assert_same_inf_pattern_and_close, build_g19_transformer, g19_inputs

    g = golden("g19_two_stage_transformer.npz")
    tr, L = build_g19_transformer(g)
    tr = tr.to(DEV, F16)
    srcs, masks, poss = g19_inputs(g, L, DEV, F16)
    real_topk = torch.topk

    def fixture_topk(scores, k, dim=-1):
        idx = torch.from_numpy(g["topk"]).to(scores.device)
        return torch.gather(scores, 1, idx), idx

    monkeypatch.setattr(torch, "topk", fixture_topk)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = tr(srcs, masks, poss, None)
    monkeypatch.setattr(torch, "topk", real_topk)
    tags = tags_of(timer)
    assert {"proposal_queries", "encoder_proposals_masked", "add_layernorm", "linear_shortk", "ffn256"} <= tags, tags
    assert out["hs"].dtype == F16 and out["init_reference_out"].dtype == torch.float32
    assert_same_inf_pattern_and_close(out["enc_outputs_coord_unact"].double().cpu().numpy(), g["enc_outputs_coord_unact"], BF16_TRANSFORMER_TOL)
    errs = {k: float(np.abs(out[k].double().cpu().numpy() - g[k]).max()) for k in ("enc_outputs_class", "init_reference_out", "hs", "inter_references_out")}
    print("two-stage fp16 vs G19, max-abs:", errs)
    assert max(errs.values()) <= BF16_TRANSFORMER_TOL, errs


# what an fp16 model may launch: the kernels that take ALO_F16 and the ones whose operands are not the model's dtype (masks, fp32 geometry)
FP16_OR_DTYPE_FREE = {"linear_shortk", "linear_packed", "ffn256", "add_layernorm", "bias_act", "pos_sine_flat", "value_proj_hm", "value_head_major",
                      "msda_fwd", "msda_fwd_fused", "mask_pyramid", "encoder_reference_points", "panoptic_onehot", "encoder_proposals",
                      "encoder_proposals_masked", "mask_rows", "proposal_queries"}


def test_raft_update_block_in_fp16_stays_off_the_fp32_kernels():
    """RAFT's update block gates its fused passes on fp32 itself (alonet/raft/update.py): a ``.half()`` block keeps the stock ops."""
    from alonet.raft.update import BasicUpdateBlock

    torch.manual_seed(4)
    blk = BasicUpdateBlock(corr_levels=4, corr_radius=4).to(DEV).half().eval()
    net, inp = torch.randn(1, 128, 12, 16, device=DEV).half().tanh(), torch.randn(1, 128, 12, 16, device=DEV).half().relu()
    corr, flow = torch.randn(1, 324, 12, 16, device=DEV).half(), torch.randn(1, 2, 12, 16, device=DEV).half()
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        net2, up_mask, delta = blk(net, inp, corr, flow)
    assert not timer.summary(), timer.summary()
    assert net2.dtype == F16 and torch.isfinite(net2.float()).all() and torch.isfinite(delta.float()).all() and up_mask.shape == (1, 576, 12, 16)


def test_panoptic_head_in_fp16_reaches_no_bf16_only_kernel():
    """PanopticHead over Deformable-DETR R50, ``.half()``, channels-last: the backbone, the input projections and the mask head have
    bf16-only kernels behind their gates and must keep the stock ops; the transformer runs on the fp16 layer kernels."""
    import aloscene
    from alonet.deformable_detr_panoptic import DeformableDetrR50PanopticFinetune

    torch.manual_seed(3)
    frames = aloscene.Frame.batch_list([aloscene.Frame(torch.rand(3, 128, 160) * 255, normalization="255").norm_resnet()
                                        for _ in range(2)]).to(DEV)
    p = DeformableDetrR50PanopticFinetune(num_classes=4, base_weights=None, device=torch.device(DEV)).eval()
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = p.half().to(memory_format=torch.channels_last)(frames.to(F16))
    tags = tags_of(timer)
    print("panoptic fp16 launches:", sorted(tags))
    assert tags <= FP16_OR_DTYPE_FREE, tags - FP16_OR_DTYPE_FREE
    assert {"linear_shortk", "ffn256", "add_layernorm", "msda_fwd_fused"} <= tags, tags
    assert out["pred_logits"].dtype == F16 and out["pred_logits"].shape[:2] == (2, 300)
    assert out["pred_masks"].shape[0] == 2
