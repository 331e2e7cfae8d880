"""alo_hip.linear_f32 and alo_hip.conv1x1_strided_f32 (alo_linear_packed / alo_conv1x1_nhwc with dtype = ALO_F32,
aloception-oss_amd/csrc/gemm_f32.hip) against the fp64 product of the same fp32 operands, per output element, within the bound derived
in linear_f32_ref.py — which test_linear_f32_cpu.py holds the numpy restatement of the kernel's arithmetic to, so what is asked of the
kernel here has been checked without a GPU."""
import functools
import itertools

import pytest
import torch

import alo_hip
import guarded
from kernel_bounds import INF, NAN, compare
from linear_f32_ref import SCALES, SHAPES, operands, reference_and_bound
from test_linear_f32_cpu import numpy_split_packed

pytestmark = pytest.mark.gpu
FLAGS = list(itertools.product([True, False], repeat=3))     # bias, ReLU, residual
FLAG_IDS = ["".join(c if on else "-" for c, on in zip("bias+relu+res".split("+"), f)) for f in FLAGS]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(shape, scale, bias, relu, residual):
    """Operands, fp64 reference and bound of one case, on the CPU: made once, never written to."""
    x, w, b, res = operands(shape, scale)
    b, res = (b if bias else None), (res if residual else None)
    return (x, w, b, res) + reference_and_bound(x, w, b, res, relu)


def _run(x, w, b, res, relu):
    dev = lambda a: None if a is None else a.cuda()  # noqa: E731
    with torch.no_grad():
        y = alo_hip.linear_f32(dev(x), dev(w), dev(b), relu=relu, residual=dev(res))
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == (*x.shape[:-1], w.shape[0])
    return y.cpu()


def _hold(shape, scale, bias, relu, residual):
    x, w, b, res, ref, bound = _case(shape, scale, bias, relu, residual)
    got = _run(x, w, b, res, relu)
    ratio = compare(got, ref, bound, f"linear_f32 {shape} scale={scale} bias={bias} relu={relu} residual={residual}")
    print(f"linear_f32 {shape} scale={scale} bias={bias} relu={relu} residual={residual}: worst |err| / bound = {ratio:.4f}, "
          f"max |err| / max |ref| = {((got.double() - ref).abs().max() / ref.abs().max()).item():.3g}")


@pytest.mark.parametrize("bias,relu,residual", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("shape", SHAPES[:5], ids=ids)
def test_kernel_meets_the_bound_with_every_epilogue(shape, bias, relu, residual):
    _hold(shape, 1.0, bias, relu, residual)


def _grid(m):
    """The launch arithmetic of gemm_f32.hip (xcd_tile_range / xcd_grid of common.hpp): 64-row tiles, one contiguous eighth per XCD,
    at most 128 workgroups per XCD and column block -> (tiles, tiles per XCD, workgroups per XCD)."""
    tiles = (m + 63) // 64
    per_xcd = (tiles + 7) // 8
    return tiles, per_xcd, min(per_xcd, 128)


@pytest.mark.parametrize("bias,relu,residual", [(True, True, True), (False, False, False)], ids=["all", "plain"])
@pytest.mark.parametrize("shape", SHAPES[5:], ids=ids)
def test_kernel_meets_the_bound_at_long_k_many_columns_and_second_tiles(shape, bias, relu, residual):
    tiles, per_xcd, groups = _grid(shape[0])
    if shape[0] >= 66000:
        # 66000 rows: 1032 tiles, 129 per XCD on 128 workgroups: one workgroup per XCD walks tiles t and t + 128;
        # 70001 rows: 1094 tiles, 137 per XCD: nine do, and the last tile holds 49 rows
        assert (tiles, per_xcd, groups) in ((1032, 129, 128), (1094, 137, 128)) and per_xcd > groups
    else:
        assert per_xcd == groups           # every workgroup has one tile
    _hold(shape, 1.0, bias, relu, residual)


@pytest.mark.parametrize("scale", SCALES)
def test_kernel_meets_the_bound_at_any_input_magnitude(scale):
    _hold((130, 192, 192), scale, True, True, True)
    _hold((65, 128, 64), scale, True, False, False)


# (N, Cin, Cout, H, W), stride 2
STRIDED = [(2, 64, 64, 5, 7), (3, 128, 256, 37, 51), (1, 64, 128, 1, 9), (2, 256, 64, 9, 1)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", STRIDED, ids=ids)
def test_strided_1x1_convolution_reads_the_kept_pixels_itself(shape, relu):
    n, cin, cout, h, w_ = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, cin, h, w_, generator=g).contiguous(memory_format=torch.channels_last)
    wt, b = torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    with torch.no_grad():
        y = alo_hip.conv1x1_strided_f32(x.cuda().contiguous(memory_format=torch.channels_last), wt.cuda(), b.cuda(), 2, relu=relu)
    ho, wo = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
    assert y.shape == (n, cout, ho, wo) and y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    rows = x[:, :, ::2, ::2].permute(0, 2, 3, 1).reshape(-1, cin)
    ref, bound = reference_and_bound(rows, wt, b, None, relu)
    compare(y.cpu().permute(0, 2, 3, 1).reshape(-1, cout), ref, bound, f"conv1x1_strided_f32 {shape} relu={relu}")


def test_a_dim_row_next_to_bright_ones_keeps_its_accuracy_and_its_bits():
    x, w, b, res = operands((130, 192, 192))
    x, b, res = x.clone(), b * 1e-6, res.clone()
    x[70] *= 1e-6
    res[70] *= 1e-6
    ref, bound = reference_and_bound(x, w, b, res, False)
    got = _run(x, w, b, res, False)
    compare(got, ref, bound, "linear_f32 rows 10^6 apart")
    alone = _run(x[70:71], w, b, res[70:71], False)
    assert torch.equal(alone[0], got[70]), "the dim row's result depends on its neighbours"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(65, 128, 64), (130, 192, 192)], ids=ids)
def test_non_finite_inputs_spoil_exactly_their_rows(shape, relu):
    x, w, b, res = operands(shape)
    x = x.clone()
    x[2, 5], x[40, 77], x[11] = INF, -INF, NAN      # single elements, and a whole row
    ref, bound = reference_and_bound(x, w, b, res, relu)
    assert torch.isinf(ref).any() and torch.isnan(ref).any() and torch.isfinite(ref).any()
    got = _run(x, w, b, res, relu)
    compare(got, ref, bound, f"linear_f32 with Inf / NaN inputs, relu={relu}")
    spoiled = torch.zeros(shape[0], dtype=torch.bool)
    spoiled[[2, 40, 11]] = True
    assert torch.isfinite(got[~spoiled]).all() and torch.isnan(got[11]).all()
    if not relu:
        assert not torch.isfinite(got[spoiled]).any()


def test_split_weights_are_cached_on_the_weight_and_follow_it():
    x, w, b, res = operands((63, 64, 128))
    xg, wg = x.cuda(), w.cuda()
    with torch.no_grad():
        y0 = alo_hip.linear_f32(xg, wg)
        pack = wg.__dict__["_alo_derived"]["linear_f32_b"][1]
        assert torch.equal(pack.cpu(), numpy_split_packed(w))                              # the pack kernel's order, too
        assert alo_hip.linear_f32(xg, wg) is not None and wg.__dict__["_alo_derived"]["linear_f32_b"][1] is pack
        wg.mul_(2.0)                                                                       # a new version: re-derived
        y1 = alo_hip.linear_f32(xg, wg)
    assert wg.__dict__["_alo_derived"]["linear_f32_b"][1] is not pack
    assert torch.equal(y1, 2.0 * y0)                                                       # a power of two moves the exponents only


def test_launches_stay_in_their_buffers_and_ignore_stale_bytes():
    """One small and one multi-tile shape, every epilogue, and a strided convolution inside guarded buffers with the existing role
    table: y is OUT for both entry points."""
    assert guarded.ROLES["alo_linear_packed"] == {4: guarded.OUT} and guarded.ROLES["alo_conv1x1_nhwc"] == {5: guarded.OUT}
    with guarded.GuardedLaunches() as g:
        for bias, relu, residual in FLAGS:
            _hold((63, 64, 128), 1.0, bias, relu, residual)
        for bias, relu, residual in ((True, True, True), (False, False, False)):
            _hold((66000, 64, 64), 1.0, bias, relu, residual)
        x = torch.randn(2, 128, 9, 7, device="cuda").contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            alo_hip.conv1x1_strided_f32(x, torch.randn(192, 128, device="cuda"), torch.randn(192, device="cuda"), 2, relu=True)
    tags = [tag for _, tag in g.seen if tag is not None]
    assert tags.count("linear_f32/K=64/N=128") == 8 and tags.count("linear_f32/K=64/N=64") == 2
    assert tags.count("conv1x1_strided_f32/K=128/N=192") == 1
    assert {s for s, _ in g.seen} == {"alo_linear_packed", "alo_conv1x1_nhwc", "alo_pack_mfma_b"}
