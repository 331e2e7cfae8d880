"""The "glue" kernels between the backbone and the attention op (fused.hip, groupnorm.hip, conv_small.hip, geometry.hip and the
head-major epilogue of gemm.hip) at the launch sizes the headline models run, against fp64 references, element by element.

Each kernel has a path that only a large launch takes (a grid-stride loop past the grid cap, a second 64-column item, a second round
of chunk stripes); the helpers below mirror the launch arithmetic so that a case can ASSERT that it takes the path it is here for.
References are fp64 on the GPU from the kernel's own fp32 / bf16 operands (both convert exactly); the ones that are not a stock op
in ``.double()`` live in kernel_bounds.py and are pinned to the stock modules in test_glue_references_cpu.py.  Non-finite inputs
are values only (every index is in bounds); ``compare`` checks the non-finite set, then the bound on the rest.

Bounds (u = 2^-24, the fp32 unit roundoff; every bf16 result adds 2^-8 |ref|, half a bf16 ulp for the one final rounding):

pos_sine_flat      2^-22 + 6 u |p| + u |ref|, p = embed / dim_t the fp64 argument.  The embed takes three roundings (+ eps, the
                   division, * scale; counts and count - 0.5 are exact) and the division by dim_t one: the fp32 argument is off by
                   <= 5 u |p| (6 with the second-order terms), sin / cos are 1-Lipschitz; u |ref| is the rounding of the add of
                   level_embed; 2^-22 (four ulps of 1) is for the sine itself.  Checked against the stock fp32 chain
                   (PositionEmbeddingSine on the same device, arguments up to 240): it is held to the same bound on every case
                   below (measured: at most 0.54 of the bound on an MI355X, the kernel the same; so the 2^-22 stands), and
                   test_glue_references_cpu.py holds the CPU chain to it (worst 0.55 of the bound there).
add_layernorm      |gamma_c| 2 u ((sqrt(C) + 8) (1 + |xhat|) + 4 (|v| + |mean|) / sigma) + u |ref|, v = x + res in fp32, mean /
                   sigma / xhat from the fp64 reference, sigma = sqrt(var + eps).  Two-pass mean / variance in wave-tree order:
                   sqrt(C)-like growth of the two reductions, a handful of roundings on the normalise / scale / shift path; the last
                   bracket is the rounding of v - mean itself, which no fp32 evaluation avoids (it dominates on the mean = 1000 x std
                   rows).  F.layer_norm in fp32 stays inside it (CPU: worst 0.77 of the bound; the GPU op is held to it below, measured
                   0.62).  Rows with
                   |mean| <= sigma additionally keep the absolute 2e-5 of test_fused_gpu.py.
groupnorm_*        2^-8 |ref| + 2^-10 |gamma_c| (1 + |xhat|).  The statistics pass forms ss - s * mean per thread in fp32 (256 bf16
                   values), merged with Chan's formula; emulating exactly that arithmetic in numpy gives a variance off by <= 2.7e-4
                   relative and a normalised value off by <= 5.3e-4 absolute at mean / std = 100; 2^-10 is twice that.  The constant
                   group is 1.5: s, ss and s * mean are exact for a bf16 constant, the variance is exactly 0, rstd = eps^-1/2 = 316
                   and the one rounding of beta - mean * gamma * rstd is u * 1.5 * 316 |gamma| = 2.8e-5 |gamma|.  F.group_norm in
                   fp32 stays inside the same bound (held to it below on the GPU, measured at most 0.03 of it, and in the CPU file).
conv3x3_small,     2^-8 |ref| + c(K) A, c(K) = (K + 1) 2^-23, A the same product of absolute values: derivation in
value_proj_hm      test_backbone_kernels_gpu.py (K = 9 Cin, resp. the projection's K).
upsample_add       bit-for-bit the stock expression (one fp32 add, one rounding: nothing to bound).
panoptic_onehot    integer output.  At most 1e-5 of the outputs may differ from the stock fp32 chain, and every pixel that differs must
                   be a near-tie of the fp64 chain (top two probabilities, or the top one and the threshold, closer than 1e-5): those
                   are the only pixels where two correct fp32 evaluations can decide differently.  The stock fp32 chain against its
                   fp64 self is held to the same two conditions, which ties the 1e-5 to the inputs.
gru_gate_ / _update_  2^-21 (1 + |h|): at most 8 fp32 roundings of values <= 1 + |h| around one expf / tanhf (8 u (1 + |h|)).  The
                   stock torch fp32 ops (sigmoid, tanh, the same formulas) are held to the same bound on the same inputs below
                   (measured: at most 0.27 of it, so the device expf / tanhf need no extra term).
bias_act_nchw_     u |ref|: one add.
"""
import pytest
import torch
import torch.nn.functional as F

import alo_hip
import kernel_bounds as kb
from kernel_bounds import INF, NAN, _finite_abs, c_acc, compare
from test_backbone_kernels_gpu import check_conv3x3

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- launch arithmetic, mirrored from the kernels ----------------------------------------------------------------------------
def pos_paths(b, shapes, nf):
    """fused.hip pos_prefix_kernel / alo_pos_sine_flat: per level col_items = per = ceil(W / 64), items = col_items + H walked by
    32 x 4 waves; pos_generate_kernel: n4 = B * S * 2F / 4 float4s on at most 16384 x 256 threads."""
    s = sum(h * w for h, w in shapes)
    return {"col_items": max(-(-w // 64) for _, w in shapes), "per": max(-(-w // 64) for _, w in shapes),
            "items": max(-(-w // 64) + h for h, w in shapes), "n4": b * s * 2 * nf // 4}


GRID_CAP = 16384 * 256   # stream_blocks(): 256 * 64 workgroups of 256 threads


def ln_second_pass(rows):
    """fused.hip add_layernorm_t: blocks = min(ceil(rows / 4), 8192), one wave per row: a wave takes a 2nd row iff rows > 4 blocks."""
    return rows > 4 * min(-(-rows // 4), 8192)


def gn_chunks(hw, groups):
    """groupnorm.hip: nchunks = ceil(HW / 256) chunk triples, merged in nstripes = 256 / groups stripes."""
    return -(-hw // 256), 256 // groups


def upadd_total(bq, c, h, w):
    """groupnorm.hip alo_upsample_add_nhwc: total 16-byte vectors; the grid is capped at 8192 x 256 threads."""
    return bq * h * w * c // 8


def small_conv_tiles(h, w):
    return -(-h // 8), -(-w // 16)


# ---- pos_sine_flat -----------------------------------------------------------------------------------------------------------
HEADLINE_PYRAMID = [(100, 167), (50, 84), (25, 42), (13, 21)]
TALL_PYRAMID = [(136, 240), (68, 120), (34, 60), (17, 30)]
WIDTHS = [(5, 63), (5, 64), (5, 65), (5, 128), (5, 129)]
ALL_MASKS = ["none", "right", "bottom", "corner", "scatter", "all", "cross", "scatter+right"]


def _check_pos(b, shapes, nf, dtype, normalize, center, kinds, seed):
    from alonet.transformers import PositionEmbeddingSine

    enc = PositionEmbeddingSine(nf, normalize=normalize, center=center)
    g = torch.Generator(device=DEV).manual_seed(seed)
    level_embed = torch.randn(len(shapes), 2 * nf, device=DEV, generator=g).to(dtype).float()   # a parameter of the model's dtype
    mask_flat = kb.pyramid_masks(b, shapes, kinds, DEV, seed)
    sh = torch.tensor(shapes, dtype=torch.int32, device=DEV)
    sizes = [h * w for h, w in shapes]
    start = torch.tensor([sum(sizes[:i]) for i in range(len(sizes))], dtype=torch.int32, device=DEV)
    dim_t = enc.dim_t(torch.device(DEV))
    got = alo_hip.pos_sine_flat(mask_flat, sh, start, dim_t, level_embed, normalize, center, enc.scale, dtype)
    assert got.shape == (b, sum(sizes), 2 * nf) and got.dtype == dtype
    ref, p = kb.pos_sine_ref(mask_flat, shapes, dim_t, level_embed, normalize, center, enc.scale)
    worst = compare(got, ref, kb.pos_sine_bound(ref, p, dtype == torch.bfloat16), f"pos_sine_flat {shapes[0]} {dtype}")
    # the stock fp32 chain on this device is held to the fp32 bound on the same case (what the 2^-22 term rests on)
    stock, s0 = [], 0
    for lvl, (h, w) in enumerate(shapes):
        m = mask_flat[:, s0:s0 + h * w].view(b, 1, h, w)
        s0 += h * w
        stock.append(enc((torch.empty(b, 1, h, w, device=DEV), m)).flatten(2).transpose(1, 2) + level_embed[lvl].view(1, 1, -1))
    stock_ratio = compare(torch.cat(stock, 1), ref, kb.pos_sine_bound(ref, p), "PositionEmbeddingSine fp32 (stock)")
    print(f"pos_sine_flat {shapes[0]} B={b} F={nf} {dtype} norm={normalize} center={center}: kernel {worst:.3g}, "
          f"stock fp32 chain {stock_ratio:.3g} of the bound, max |p| = {p.abs().max().item():.4g}")


@pytest.mark.parametrize("dtype,normalize,center", [(torch.float32, True, True), (torch.float32, True, False),
                                                     (torch.float32, False, False), (torch.bfloat16, True, True)])
def test_pos_sine_flat_headline_pyramid(dtype, normalize, center):
    paths = pos_paths(8, HEADLINE_PYRAMID, 128)
    assert paths["col_items"] > 1 and paths["per"] > 1 and paths["n4"] > GRID_CAP, paths
    _check_pos(8, HEADLINE_PYRAMID, 128, dtype, normalize, center, ALL_MASKS, seed=11)


@pytest.mark.parametrize("dtype,normalize,center", [(torch.float32, True, True), (torch.float32, True, False),
                                                     (torch.float32, False, False), (torch.bfloat16, True, True)])
def test_pos_sine_flat_tall_pyramid_strides_over_items(dtype, normalize, center):
    paths = pos_paths(2, TALL_PYRAMID, 128)
    assert paths["items"] > 128 and paths["col_items"] > 1, paths
    _check_pos(2, TALL_PYRAMID, 128, dtype, normalize, center, ["scatter", "cross"], seed=12)
    _check_pos(2, TALL_PYRAMID, 128, dtype, normalize, center, ["none", "corner"], seed=13)


@pytest.mark.parametrize("dtype,normalize,center", [(torch.float32, True, True), (torch.float32, False, False),
                                                     (torch.bfloat16, True, True)])
def test_pos_sine_flat_widths_on_the_item_boundaries(dtype, normalize, center):
    assert {-(-w // 64) for _, w in WIDTHS} == {1, 2, 3}
    _check_pos(8, WIDTHS, 128, dtype, normalize, center, ALL_MASKS, seed=14)


def test_pos_sine_flat_d_model_128():
    _check_pos(3, HEADLINE_PYRAMID, 64, torch.float32, True, True, ["scatter", "right", "cross"], seed=15)
    _check_pos(3, HEADLINE_PYRAMID, 64, torch.bfloat16, True, True, ["scatter", "right", "cross"], seed=15)


# ---- add_layernorm -----------------------------------------------------------------------------------------------------------
def _ln_call(x, res, gamma, beta, pos):
    got = alo_hip.add_layernorm(x, res, gamma, beta, 1e-5, pos=pos)
    if pos is None:
        return got
    assert torch.equal(got[1], got[0] + pos)     # bit-exact: computed from the rounded `out`, as the unfused `out + pos`
    return got[0]


def _ln_check(out, x, res, gamma, beta, dtype, well, what):
    """In row blocks, to bound the fp64 working set."""
    worst = 0.0
    for r0 in range(0, x.shape[0], 1 << 16):
        sl = slice(r0, r0 + (1 << 16))
        v = x[sl].float() + res[sl].float() if res is not None else x[sl].float()
        ref, bound = kb.layernorm_ref_and_bound(v, gamma.float(), beta.float(), 1e-5, dtype == torch.bfloat16)
        worst = max(worst, compare(out[sl], ref, bound, f"{what} rows {r0}.."))
        if dtype == torch.float32 and well is not None:
            w = well[sl]
            assert (out[sl][w].double() - ref[w]).abs().max().item() <= 2e-5, what
    return worst


@pytest.mark.parametrize("rows", [177784, 32768 + 5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_res,with_pos", [(True, False), (True, True), (False, False), (False, True)])
def test_add_layernorm_second_row_pass(rows, dtype, with_res, with_pos):
    assert ln_second_pass(rows) and not ln_second_pass(32768)
    x, res, gamma, beta, kind = kb.layernorm_inputs(rows, 256, DEV, seed=rows + 2 * with_res + with_pos)
    x, res, gamma, beta = x.to(dtype), res.to(dtype) if with_res else None, gamma.to(dtype), beta.to(dtype)
    pos = torch.randn(rows, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(dtype) if with_pos else None
    out = _ln_call(x, res, gamma, beta, pos)
    worst = _ln_check(out, x, res, gamma, beta, dtype, kind == 0, f"add_layernorm {rows} {dtype}")
    print(f"add_layernorm rows={rows} {dtype} res={with_res} pos={with_pos}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("c", [256, 260, 1024])
def test_add_layernorm_ill_conditioned_rows_and_wide_rows(c):
    """fp32 rows with mean = 1000 x std, constant rows (variance 0, rstd = eps^-1/2), C = 260 / 1024, all past 32768 rows; the stock
    fp32 op on the same device is held to the same bound."""
    rows = 32768 + 5
    assert ln_second_pass(rows)
    x, res, gamma, beta, kind = kb.layernorm_inputs(rows, c, DEV, seed=c, ill=True)
    pos = torch.randn(rows, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    for r, p in ((res, pos), (None, None)):
        v = x + r if r is not None else x
        assert (v[kind == 2].double().var(-1, unbiased=False) == 0).all()
        out = _ln_call(x, r, gamma, beta, p)
        worst = _ln_check(out, x, r, gamma, beta, torch.float32, kind == 0, f"add_layernorm ill C={c}")
        stock = _ln_check(F.layer_norm(v, (c,), gamma, beta, 1e-5), x, r, gamma, beta, torch.float32, kind == 0, f"F.layer_norm C={c}")
        print(f"add_layernorm ill-conditioned C={c}: kernel {worst:.3g}, stock fp32 op {stock:.3g} of the bound")


def test_add_layernorm_bf16_aliasing_at_encoder_size():
    """`out` aliasing `x` through the raw ABI at 8 x 22223 rows (each row is read completely before it is written)."""
    rows = 177784
    assert ln_second_pass(rows)
    x, res, gamma, beta, _ = kb.layernorm_inputs(rows, 256, DEV, seed=3)
    x, res, gamma, beta = x.bfloat16(), res.bfloat16(), gamma.bfloat16(), beta.bfloat16()
    out = alo_hip.add_layernorm(x, res, gamma, beta, 1e-5)
    x2 = x.clone()
    rc = alo_hip.lib().alo_add_layernorm(alo_hip._ptr(x2), alo_hip._ptr(res), alo_hip._ptr(gamma), alo_hip._ptr(beta), alo_hip._ptr(x2),
                                         None, None, rows, 256, 1e-5, alo_hip.ALO_BF16, alo_hip._stream(x.device))
    assert rc == 0 and torch.equal(x2, out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_add_layernorm_non_finite_rows(dtype):
    """NaN / +Inf / -Inf in three rows (first pass, second pass, last row): exactly those rows are all-NaN, as F.layer_norm makes
    them; every other row is bit-identical to the run without them."""
    rows = 32768 + 5
    x, res, gamma, beta, _ = kb.layernorm_inputs(rows, 256, DEV, seed=9)
    x, res, gamma, beta = x.to(dtype), res.to(dtype), gamma.to(dtype), beta.to(dtype)
    pos = torch.randn(rows, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(dtype)
    clean, clean_pos = alo_hip.add_layernorm(x, res, gamma, beta, 1e-5, pos=pos)
    assert torch.isfinite(clean.float()).all()
    spots = {5: (17, NAN), 32768 + 1: (0, INF), rows - 1: (255, -INF)}
    xp, rp = x.clone(), res.clone()
    for i, (r, (c, v)) in enumerate(spots.items()):
        (xp if i != 1 else rp)[r, c] = v           # the +Inf arrives through the residual
    out, out_pos = alo_hip.add_layernorm(xp, rp, gamma, beta, 1e-5, pos=pos)
    bad = torch.zeros(rows, dtype=torch.bool, device=DEV)
    bad[list(spots)] = True
    stock = F.layer_norm(xp.float() + rp.float(), (256,), gamma.float(), beta.float(), 1e-5)
    assert torch.equal(torch.isnan(stock).all(-1), bad) and torch.equal(torch.isnan(stock).any(-1), bad)
    for t in (out, out_pos):
        assert torch.equal(torch.isnan(t.float()).all(-1), bad) and torch.equal(torch.isnan(t.float()).any(-1), bad)
    assert torch.equal(bits(out[~bad]), bits(clean[~bad])) and torch.equal(bits(out_pos[~bad]), bits(clean_pos[~bad]))


# ---- groupnorm_rows / groupnorm_nhwc -----------------------------------------------------------------------------------------
def _gn_params(c, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(c, device=DEV, generator=g).bfloat16(), torch.randn(c, device=DEV, generator=g).bfloat16()


def _gn_rows_check(out, x, groups, gamma, beta, what):
    """x, out (B, HW, C): one image at a time."""
    worst = 0.0
    for i in range(x.shape[0]):
        ref, bound = kb.groupnorm_ref_and_bound(x[i:i + 1].transpose(1, 2), groups, gamma, beta, 1e-5)
        worst = max(worst, compare(out[i:i + 1].transpose(1, 2), ref, bound, f"{what} image {i}"))
    return worst


def test_groupnorm_rows_headline_levels_into_one_flat_buffer():
    """The four levels of the headline (B = 8, C = 256, 32 groups), each written with out=flat[:, start:start + HW] into one
    (8, 8 + 22223 + 8, 256) buffer as deformable_detr.py does; the whole buffer is checked afterwards."""
    b, c, groups, pad = 8, 256, 32, 8
    sizes = [h * w for h, w in HEADLINE_PYRAMID]
    assert sum(sizes) == 22223
    nchunks, nstripes = gn_chunks(sizes[0], groups)
    assert nchunks == 66 and nchunks > nstripes == 8
    flat = torch.full((b, sum(sizes) + 2 * pad, c), 7.0, device=DEV, dtype=torch.bfloat16)
    gamma, beta = _gn_params(c, 1)
    g = torch.Generator(device=DEV).manual_seed(2)
    xs, start = [], pad
    with torch.no_grad():
        for hw in sizes:
            x = (torch.randn(b, hw, c, device=DEV, generator=g) * 3 + 0.7).bfloat16()
            out = alo_hip.groupnorm_rows(x, gamma, beta, groups, 1e-5, out=flat[:, start:start + hw])
            assert out.data_ptr() == flat[:, start:].data_ptr()
            xs.append(x)
            start += hw
    start = pad
    for x, hw in zip(xs, sizes):
        worst = _gn_rows_check(flat[:, start:start + hw], x, groups, gamma, beta, f"groupnorm_rows HW={hw}")
        print(f"groupnorm_rows level HW={hw}: worst error / bound = {worst:.3g}")
        start += hw
    assert (flat[:, :pad] == 7.0).all() and (flat[:, start:] == 7.0).all() and start == pad + 22223


@pytest.mark.parametrize("hw", [2048, 2049, 2304])
def test_groupnorm_rows_stripe_boundary(hw):
    """Exactly 8 chunks, 8 chunks + 1 row, 9 chunks with 8 stripes: the second round of the stripe loop starts at chunk 8."""
    nchunks, nstripes = gn_chunks(hw, 32)
    assert nstripes == 8 and (nchunks > nstripes) == (hw > 2048)
    gamma, beta = _gn_params(256, hw)
    g = torch.Generator(device=DEV).manual_seed(hw)
    x = (torch.randn(3, hw, 256, device=DEV, generator=g) * 3 + 0.7).bfloat16()
    x[:, 2048:] += 4.0            # the rows of the 9th chunk weigh on the statistics: dropping them moves every output
    with torch.no_grad():
        out = alo_hip.groupnorm_rows(x, gamma, beta, 32, 1e-5)
    _gn_rows_check(out, x, 32, gamma, beta, f"groupnorm_rows HW={hw}")


@pytest.mark.parametrize("n,c,h,w,groups", [(128, 16, 200, 334, 8), (128, 32, 100, 167, 8), (128, 64, 50, 84, 8), (128, 128, 25, 42, 8)])
@pytest.mark.parametrize("relu", [False, True])
def test_groupnorm_nhwc_at_128_maps(n, c, h, w, groups, relu):
    nchunks, nstripes = gn_chunks(h * w, groups)
    assert nstripes == 32 and (nchunks > nstripes) == (h * w > 8192)
    g = torch.Generator(device=DEV).manual_seed(c + h)
    x = (torch.randn(n, c, h, w, device=DEV, generator=g) * 2 + 0.3).bfloat16().contiguous(memory_format=torch.channels_last)
    norm = torch.nn.GroupNorm(groups, c).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(c, device=DEV, generator=g))
        norm.bias.copy_(torch.randn(c, device=DEV, generator=g))
        out = alo_hip.groupnorm_nhwc(x, norm, relu=relu)
    assert out.shape == x.shape and out.is_contiguous(memory_format=torch.channels_last)
    worst = 0.0
    for i0 in range(0, n, 16):
        ref, bound = kb.groupnorm_ref_and_bound(x[i0:i0 + 16], groups, norm.weight.detach(), norm.bias.detach(), norm.eps, relu)
        worst = max(worst, compare(out[i0:i0 + 16], ref, bound, f"groupnorm_nhwc C={c} images {i0}.."))
    print(f"groupnorm_nhwc {n} x {c} x {h} x {w} relu={relu}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("c,groups,hw", [(256, 32, 2304), (16, 8, 9000), (32, 8, 700), (64, 8, 513)])
def test_groupnorm_ill_conditioned_groups(c, groups, hw):
    """Groups with mean / std in {0.25, 16, 100} and a constant group, through groupnorm_rows (C = 256) or groupnorm_nhwc with and
    without ReLU; F.group_norm in fp32 on the same device is held to the same bound."""
    n = 3
    x = kb.groupnorm_ill_inputs(n, c, hw, groups, DEV, seed=c + hw)          # (N, C, HW)
    gamma, beta = _gn_params(c, c)
    rows = x.transpose(1, 2).contiguous()                                    # (N, HW, C): channels-last
    for relu in (False, True):
        ref, bound = kb.groupnorm_ref_and_bound(x, groups, gamma, beta, 1e-5, relu)
        with torch.no_grad():
            if c == 256:
                if relu:
                    continue
                out = alo_hip.groupnorm_rows(rows, gamma, beta, groups, 1e-5).transpose(1, 2)
            else:
                norm = torch.nn.GroupNorm(groups, c).to(DEV).to(torch.bfloat16)
                norm.weight.copy_(gamma)
                norm.bias.copy_(beta)
                x4 = rows.transpose(1, 2).unsqueeze(-1)                      # (N, C, HW, 1) with channels-last strides
                assert x4.is_contiguous(memory_format=torch.channels_last)
                out = alo_hip.groupnorm_nhwc(x4, norm, relu=relu)[..., 0]
            stock = F.group_norm(x.float(), groups, gamma.float(), beta.float(), 1e-5)
        worst = compare(out, ref, bound, f"groupnorm ill C={c} relu={relu}")
        stock_ratio = compare(torch.relu(stock) if relu else stock, ref, bound, "F.group_norm fp32 (stock)")
        print(f"groupnorm ill-conditioned C={c} relu={relu}: kernel {worst:.3g}, stock fp32 op {stock_ratio:.3g} of the bound")


@pytest.mark.parametrize("c,groups,hw", [(256, 32, 2304), (16, 8, 714), (32, 8, 221), (64, 8, 1230)])
@pytest.mark.parametrize("value", [NAN, INF])
def test_groupnorm_non_finite_value_fills_its_group_only(c, groups, hw, value):
    """NaN / +Inf in one (image, group): every output of that image's group is NaN, as the stock op gives (ReLU keeps them); every
    other (image, group) is bit-identical to the clean run."""
    n, cpg = 3, c // groups
    g = torch.Generator(device=DEV).manual_seed(c)
    rows = (torch.randn(n, hw, c, device=DEV, generator=g) * 2 + 0.3).bfloat16()
    gamma, beta = _gn_params(c, 7)
    spots = [(1, hw // 3, 5 * cpg + 1), (2, hw - 1, c - 1)]                  # groups 5 and groups - 1
    planted = rows.clone()
    for i, r, ch in spots:
        planted[i, r, ch] = value
    want = torch.zeros(n, groups, dtype=torch.bool, device=DEV)
    want[1, 5] = want[2, groups - 1] = True

    def run(t, relu):
        with torch.no_grad():
            if c == 256:
                return alo_hip.groupnorm_rows(t, gamma, beta, groups, 1e-5)
            norm = torch.nn.GroupNorm(groups, c).to(DEV).to(torch.bfloat16)
            norm.weight.copy_(gamma)
            norm.bias.copy_(beta)
            return alo_hip.groupnorm_nhwc(t.transpose(1, 2).unsqueeze(-1), norm, relu=relu)[..., 0].transpose(1, 2)

    for relu in ((False,) if c == 256 else (False, True)):
        clean, out = run(rows, relu), run(planted, relu)
        stock = F.group_norm(planted.float().transpose(1, 2), groups, gamma.float(), beta.float(), 1e-5)
        stock = torch.relu(stock) if relu else stock
        for t in (stock.transpose(1, 2), out):
            nan = torch.isnan(t.float()).reshape(n, hw, groups, cpg).permute(0, 2, 1, 3).flatten(2)
            assert torch.equal(nan.all(-1), want) and torch.equal(nan.any(-1), want), (relu, value)
        keep = ~want[:, None, :, None].expand(n, hw, groups, cpg).reshape(n, hw, c)
        assert torch.equal(bits(out)[keep], bits(clean)[keep])


# ---- conv3x3_small -----------------------------------------------------------------------------------------------------------
def _small_conv(cin, cout, bias, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=bias).to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / (9 * cin) ** 0.5)
        if bias:
            conv.bias.copy_(0.5 * torch.randn(cout, device=DEV, generator=g))
    return conv, g


def _small_conv_check(x, conv, what):
    with torch.no_grad():
        assert alo_hip.conv3x3_small_supported(x, conv)
        got = alo_hip.conv3x3_small(x, conv)
    assert got.is_contiguous(memory_format=torch.channels_last)
    b = None if conv.bias is None else conv.bias.detach()
    return got, check_conv3x3(x, conv.weight.detach(), b, False, 1, got, what)


@pytest.mark.parametrize("n,cin,cout,h,w", [(128, 64, 32, 100, 167), (128, 32, 16, 200, 334), (128, 16, 1, 200, 334)])
@pytest.mark.parametrize("bias", [True, False])
def test_conv3x3_small_at_128_maps(n, cin, cout, h, w, bias):
    conv, g = _small_conv(cin, cout, bias, cin + cout)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    _, worst = _small_conv_check(x, conv, f"conv3x3_small {cin}->{cout}")
    print(f"conv3x3_small {n} x {cin}->{cout} x {h} x {w} bias={bias}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("h,w", [(7, 15), (8, 16), (9, 17), (15, 31), (16, 32), (17, 33), (8, 33), (17, 16)])
@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 16), (16, 1), (16, 4)])
def test_conv3x3_small_around_the_tile_size(h, w, cin, cout):
    ty, tx = small_conv_tiles(h, w)
    assert (ty, tx) == ((h + 7) // 8, (w + 15) // 16)
    conv, g = _small_conv(cin, cout, True, h * w + cin)
    x = torch.randn(3, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    _small_conv_check(x, conv, f"conv3x3_small {h} x {w}")


@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 16), (16, 1)])
def test_conv3x3_small_non_finite_pixels_stay_in_their_neighbourhood(cin, cout):
    """NaN / Inf at a map corner, a tile corner and the last pixel of a map: exactly the 3 x 3 neighbourhood inside that map is
    non-finite in every output channel (compare() checks the set against the fp64 op), the next map's first pixels are clean."""
    n, h, w = 4, 37, 50
    conv, g = _small_conv(cin, cout, True, cin)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    x[0, 3, 0, 0] = NAN                    # map corner
    x[0, 5, 8, 16] = INF                   # first pixel of tile (1, 1)
    x[0, 6, 15, 31] = NAN                  # last pixel of tile (1, 1)
    x[1, cin - 1, h - 1, w - 1] = NAN      # the last pixel of map 1
    x[2, 0, h - 1, w - 1] = -INF
    got, _ = _small_conv_check(x, conv, "conv3x3_small non-finite")
    bad = ~torch.isfinite(got.float())
    want = torch.zeros(n, 1, h, w, dtype=torch.bool, device=DEV)
    for i, yy, xx in ((0, 0, 0), (0, 8, 16), (0, 15, 31), (1, h - 1, w - 1), (2, h - 1, w - 1)):
        want[i, 0, max(yy - 1, 0):yy + 2, max(xx - 1, 0):xx + 2] = True
    assert torch.equal(bad, want.expand(n, cout, h, w))
    assert not bad[2, :, 0, :8].any() and not bad[3].any()


# ---- upsample_add ------------------------------------------------------------------------------------------------------------
def _upadd_stock(x, fpn, q, i):
    h, w = fpn.shape[-2:]
    return fpn[i:i + 1].unsqueeze(1).repeat(1, q, 1, 1, 1).flatten(0, 1) + F.interpolate(x[i * q:(i + 1) * q], size=(h, w), mode="nearest")


@pytest.mark.parametrize("b,q,c,h,w,hh,ww", [(8, 16, 32, 100, 167, 200, 334), (8, 16, 64, 50, 84, 100, 167), (8, 16, 128, 25, 42, 50, 84)])
def test_upsample_add_past_the_grid_cap(b, q, c, h, w, hh, ww):
    assert upadd_total(b * q, c, hh, ww) > 8192 * 256
    g = torch.Generator(device=DEV).manual_seed(c + hh)
    x = torch.randn(b * q, c, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    fpn = torch.randn(b, c, hh, ww, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        got = alo_hip.upsample_add(x, fpn)
        assert got.is_contiguous(memory_format=torch.channels_last)
        for i in range(b):
            assert torch.equal(got[i * q:(i + 1) * q], _upadd_stock(x, fpn, q, i)), i


def test_upsample_add_non_finite_and_signed_zero_bits():
    """NaN / +-Inf / -0.0 in both operands: the raw bits of the stock result wherever it is not NaN, NaN where it is."""
    b, q, c, h, w, hh, ww = 2, 3, 16, 9, 11, 18, 23
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(b * q, c, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    fpn = torch.randn(b, c, hh, ww, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    x[0, 0, 0, 0], x[1, 3, 4, 5], x[2, 7, 8, 10], x[3, 1, 2, 2], x[5, 15, 8, 10] = NAN, INF, -INF, -0.0, INF
    x[4] = -0.0
    fpn[0, 3, 8:11, 10:13] = -INF            # meets the +Inf of x[1]: Inf - Inf
    fpn[1, :, :9] = -0.0                     # -0.0 + -0.0 = -0.0 over a region of x[4]
    fpn[1, :, 9:] = 0.0
    fpn[1, 15, hh - 1, ww - 1] = NAN
    with torch.no_grad():
        got = alo_hip.upsample_add(x, fpn)
        want = torch.cat([_upadd_stock(x, fpn, q, i) for i in range(b)])
    nan = torch.isnan(want.float())
    assert nan.any() and torch.isinf(want.float()).any() and (bits(want) == -32768).any()
    assert torch.equal(torch.isnan(got.float()), nan)
    assert torch.equal(bits(got)[~nan], bits(want)[~nan])


# ---- panoptic_onehot ---------------------------------------------------------------------------------------------------------
def _onehot_check(logits, size, got, what):
    """Per image: got and the stock fp32 chain against each other and against the fp64 chain."""
    differ = differ_stock = 0
    saw_nothing = False
    for i in range(logits.shape[0]):
        want = kb.panoptic_onehot_from(kb.panoptic_probabilities(logits[i], size, 0.5))
        want64 = kb.panoptic_onehot_from(kb.panoptic_probabilities(logits[i].double(), size, 0.5))
        tie = kb.panoptic_near_tie(logits[i], size, 0.5)
        d = got[i] != want
        assert not (d.any(0) & ~tie).any(), f"{what}: image {i} differs from the stock chain away from any near-tie"
        d64 = want != want64
        assert not (d64.any(0) & ~tie).any(), f"{what}: the stock fp32 chain differs from fp64 away from any near-tie"
        differ += int(d.sum())
        differ_stock += int(d64.sum())
        saw_nothing |= bool((want.sum(0) == 0).any())
    total = got.numel()
    print(f"{what}: {differ} of {total} outputs differ from the stock fp32 chain, the stock chain from fp64 in {differ_stock}")
    assert int(got.sum(1).max()) <= 1 and saw_nothing
    assert differ_stock / total <= 1e-5 and differ / total <= 1e-5


@pytest.mark.parametrize("b,q,h,w,hh,ww", [(8, 16, 200, 334, 800, 1333), (2, 5, 97, 160, 40, 64), (2, 1, 30, 40, 64, 90)])
def test_panoptic_onehot_at_frame_size(b, q, h, w, hh, ww):
    g = torch.Generator(device=DEV).manual_seed(b * 100 + q)
    logits = torch.randn(b, q, h, w, device=DEV, generator=g) * 3
    logits[:, :, : h // 3] -= 6.0     # a region where no query passes the threshold
    got = alo_hip.panoptic_onehot(logits, (hh, ww), 0.5)
    assert got.shape == (b, q, hh, ww) and got.dtype == torch.long
    _onehot_check(logits, (hh, ww), got, f"panoptic_onehot {h} x {w} -> {hh} x {ww}")


def test_panoptic_onehot_nan_logits_select_their_query_as_the_stock_chain_does():
    """F.threshold keeps NaN (NaN <= thr is false) and torch.argmax takes the first NaN for the maximum, so in the stock chain a
    NaN probability selects its query; the kernel does the same on every pixel a NaN logit reaches."""
    b, q, h, w, size = 2, 5, 20, 33, (80, 131)
    g = torch.Generator(device=DEV).manual_seed(8)
    logits = torch.randn(b, q, h, w, device=DEV, generator=g) * 3
    logits[:, :, :6] -= 6.0
    logits[0, 3, 10, 12] = NAN
    logits[0, 1, 3, 20] = NAN             # in the region where nothing passes the threshold
    logits[1, 2, 8, 8] = logits[1, 4, 8, 8] = NAN   # two NaN queries on one pixel: the first one wins
    logits[1, 0, 15, 25] = NAN
    got = alo_hip.panoptic_onehot(logits, size, 0.5)
    for i in range(b):
        probs = kb.panoptic_probabilities(logits[i], size, 0.5)
        want = kb.panoptic_onehot_from(probs)
        reached = torch.isnan(probs).any(0)
        assert int(reached.sum()) >= 2 * 36
        assert torch.equal(got[i][:, reached], want[:, reached])
        first_nan = torch.isnan(probs).float().argmax(0)[reached]
        assert torch.equal(got[i][:, reached].argmax(0), first_nan) and (got[i][:, reached].sum(0) == 1).all()
        clean = torch.nan_to_num(logits[i], nan=0.0)
        tie = kb.panoptic_near_tie(clean, size, 0.5)
        assert not ((got[i] != want).any(0) & ~reached & ~tie).any()


# ---- gru_gate_ / gru_update_ / bias_act_nchw_ --------------------------------------------------------------------------------
def _gru_buffers(b, c, cx, h, w, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    zr = torch.randn(b, 2 * c, h, w, device=DEV, generator=g) * 2
    hx = torch.randn(b, c + cx, h, w, device=DEV, generator=g)
    hx[:, :c] = torch.tanh(hx[:, :c])
    rhx = torch.randn(b, c + cx, h, w, device=DEV, generator=g)
    q = torch.randn(b, c, h, w, device=DEV, generator=g) * 2
    bzr, bq = torch.randn(2 * c, device=DEV, generator=g), torch.randn(c, device=DEV, generator=g)
    return zr, hx, rhx, q, bzr, bq


def _gru_round_trip(zr, hx, rhx, q, bzr, bq, c, what):
    """gru_gate_ then gru_update_, each against the fp64 formulas of its own operands; the stock fp32 ops are held to the same bound."""
    zr0, hx0, rhx0 = zr.clone(), hx.clone(), rhx.clone()
    h0 = hx0[:, :c]
    alo_hip.gru_gate_(zr, bzr, hx, rhx, c)
    z_ref, rh_ref = kb.gru_gate_ref(zr0, bzr, h0)
    bound = kb.gru_bound(h0)
    worst = max(compare(zr[:, :c], z_ref, bound, f"{what}: z"), compare(rhx[:, :c], rh_ref, bound, f"{what}: r * h"))
    assert torch.equal(bits(zr[:, c:]), bits(zr0[:, c:])), "the r half of zr changed"
    assert torch.equal(bits(rhx[:, c:]), bits(rhx0[:, c:])) and torch.equal(bits(hx), bits(hx0)), "channels >= C / hx changed"
    pre = zr0 + bzr.view(1, -1, 1, 1)
    stock = max(compare(torch.sigmoid(pre[:, :c]), z_ref, bound, "torch fp32 sigmoid"),
                compare(torch.sigmoid(pre[:, c:]) * h0, rh_ref, bound, "torch fp32 sigmoid * h"))
    # update: z is what the gate left in zr (the kernel's operand)
    z = zr[:, :c].clone()
    zr1 = zr.clone()
    net = torch.full_like(q, 3.0)
    alo_hip.gru_update_(q, bq, zr, hx, c, net)
    new_ref = kb.gru_update_ref(q, bq, z, h0)
    worst = max(worst, compare(hx[:, :c], new_ref, bound, f"{what}: update"))
    assert torch.equal(bits(net), bits(hx[:, :c])) and torch.equal(bits(hx[:, c:]), bits(hx0[:, c:])) and torch.equal(bits(zr), bits(zr1))
    stock = max(stock, compare((1 - z) * h0 + z * torch.tanh(q + bq.view(1, -1, 1, 1)), new_ref, bound, "torch fp32 update"))
    print(f"{what}: kernels {worst:.3g}, stock torch fp32 ops {stock:.3g} of the bound")
    return zr, hx, rhx


@pytest.mark.parametrize("b,c,cx", [(4, 128, 256), (12, 128, 256), (4, 96, 146)])
def test_gru_gate_and_update_at_raft_size(b, c, cx):
    h, w = 90, 160
    n4 = b * c * h * w // 4
    assert (n4 > GRID_CAP) == (b == 12)
    zr, hx, rhx, q, bzr, bq = _gru_buffers(b, c, cx, h, w, seed=b + c)
    assert hx.stride(0) != c * h * w
    _gru_round_trip(zr, hx, rhx, q, bzr, bq, c, f"gru B={b} C={c}")


def test_gru_saturated_and_non_finite_pre_activations():
    """Pre-activations in {-inf, -100, -20, 0, 20, 100, +inf}: z and r are exactly 0 / 1 at the ends, tanh exactly -1 / +1, and no
    NaN appears; a NaN planted in one element of zr, q or hx reaches that element only."""
    b, c, cx, h, w = 2, 128, 256, 12, 20
    zr, hx, rhx, q, bzr, bq = _gru_buffers(b, c, cx, h, w, seed=5)
    bzr.zero_()
    bq.zero_()
    vals = torch.tensor([-INF, -100.0, -20.0, 0.0, 20.0, 100.0, INF], device=DEV)
    idx = torch.arange(zr.numel(), device=DEV).view_as(zr)
    zr.copy_(vals[idx % 7])
    q.copy_(vals[(torch.arange(q.numel(), device=DEV).view_as(q) // 7) % 7])    # every (z, q) pair of the set occurs
    pre_z, pre_r, pre_q, h0 = zr[:, :c].clone(), zr[:, c:].clone(), q.clone(), hx[:, :c].clone()
    zr, hx, rhx = _gru_round_trip(zr, hx, rhx, q, bzr, bq, c, "gru saturated")
    z, rh, new = zr[:, :c], rhx[:, :c], hx[:, :c]
    assert (z[pre_z <= -100] == 0).all() and (z[pre_z >= 100] == 1).all() and (z[pre_z == 0] == 0.5).all()
    assert (rh[pre_r <= -100] == 0).all() and torch.equal(rh[pre_r >= 100], h0[pre_r >= 100])
    assert torch.isfinite(new).all() and torch.isfinite(z).all() and torch.isfinite(rh).all()
    assert (new[(z == 1) & (pre_q >= 100)] == 1).all() and (new[(z == 1) & (pre_q <= -100)] == -1).all()
    assert torch.equal(new[z == 0], h0[z == 0])
    # NaN in one element of each operand
    zr, hx, rhx, q, bzr, bq = _gru_buffers(b, c, cx, h, w, seed=6)
    zr[0, 3, 4, 5] = NAN            # z
    zr[1, c + 7, 0, 0] = NAN        # r
    hx[1, 9, 11, 19] = NAN          # h
    q[0, 100, 6, 6] = NAN
    zr, hx, rhx = _gru_round_trip(zr, hx, rhx, q, bzr, bq, c, "gru NaN")
    nan_new = torch.isnan(hx[:, :c]).nonzero().tolist()
    assert sorted(nan_new) == sorted([[0, 3, 4, 5], [1, 9, 11, 19], [0, 100, 6, 6]])
    assert sorted(torch.isnan(rhx[:, :c]).nonzero().tolist()) == [[1, 7, 0, 0], [1, 9, 11, 19]]     # r * h: the NaN r and the NaN h
    assert torch.isnan(zr[:, :c]).nonzero().tolist() == [[0, 3, 4, 5]]


@pytest.mark.parametrize("b,c", [(4, 128), (12, 128), (4, 96)])
@pytest.mark.parametrize("relu", [True, False])
def test_bias_act_nchw_at_raft_size(b, c, relu):
    h, w = 90, 160
    assert (b * c * h * w // 4 > GRID_CAP) == (b == 12)
    g = torch.Generator(device=DEV).manual_seed(b + c)
    x = torch.randn(b, c, h, w, device=DEV, generator=g)
    bias = torch.randn(c, device=DEV, generator=g)
    x[0, 0, 0, 0], x[b - 1, c - 1, h - 1, w - 1], x[1, 5, 7, 9], x[2, 1, 1, 1] = NAN, INF, -INF, NAN
    ref = x.double() + bias.double().view(1, -1, 1, 1)
    ref = torch.relu(ref) if relu else ref
    got = alo_hip.bias_act_nchw_(x.clone(), bias, relu)
    compare(got, ref, 2.0 ** -24 * ref.abs(), f"bias_act_nchw B={b} C={c} relu={relu}")
    assert torch.isnan(got[0, 0, 0, 0]) and torch.isnan(got[2, 1, 1, 1])       # the ReLU keeps NaN


# ---- value_proj_head_major ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s,heads,k", [(8, 22223, 8, 256), (2, 22223, 8, 128)])
def test_value_proj_head_major_against_fp64_linear(n, s, heads, k):
    """F.linear in fp64 -> masked_fill -> head-major permute.  A NaN input row under the padding mask comes out exactly 0 (what
    masked_fill gives); a NaN row not under the mask is NaN in all heads * 32 outputs of that pixel and nowhere else."""
    g = torch.Generator(device=DEV).manual_seed(n + s + k)
    x = torch.randn(n, s, k, device=DEV, generator=g).bfloat16()
    w = (torch.randn(heads * 32, k, device=DEV, generator=g) / k ** 0.5).bfloat16()
    bias = (0.5 * torch.randn(heads * 32, device=DEV, generator=g)).bfloat16()
    mask = torch.rand(n, s, device=DEV, generator=g) < 0.25
    hidden, shown = (0, 100), (1, 63)
    mask[hidden], mask[shown], mask[n - 1, s - 1], mask[0, 64] = True, False, False, True
    x[hidden[0], hidden[1], 3] = NAN
    x[shown[0], shown[1], k - 1] = NAN
    x[n - 1, s - 1, 0] = NAN
    x[0, 64, 5] = INF
    got = alo_hip.value_proj_head_major(x, w, bias, mask, heads)
    assert got.shape == (n, heads, s, 32)
    w64, b64 = w.double(), bias.double()
    for i in range(n):
        ref = (x[i].double() @ w64.t() + b64).masked_fill(mask[i][:, None], 0.0)
        amag = (_finite_abs(x[i]) @ w64.abs().t() + b64.abs()).masked_fill(mask[i][:, None], 0.0)
        ref, amag = (t.view(s, heads, 32).permute(1, 0, 2) for t in (ref, amag))
        compare(got[i], ref, 2.0 ** -8 * ref.abs() + c_acc(k) * amag, f"value_proj_head_major image {i}")
        assert (bits(got[i].permute(1, 0, 2)[mask[i]]) == 0).all()             # +0.0 exactly under the mask
    nan = torch.isnan(got.float())
    want = torch.zeros(n, s, dtype=torch.bool, device=DEV)
    want[shown] = want[n - 1, s - 1] = True
    assert torch.equal(nan.all(3).all(1), want) and torch.equal(nan.any(3).any(1), want)
    nomask = alo_hip.value_proj_head_major(x, w, bias, None, heads)
    keep = ~mask[:, None, :, None].expand_as(got)
    assert torch.equal(bits(nomask)[keep], bits(got)[keep]) and torch.isnan(nomask[hidden[0], :, hidden[1]].float()).all()
