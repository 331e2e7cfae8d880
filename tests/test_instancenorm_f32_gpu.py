"""alo_hip.instancenorm_nhwc_f32 (alo_groupnorm_rows_act with dtype = ALO_F32, groups == C, no affine;
aloception-oss_amd/csrc/instancenorm_f32.hip) against fp64 ``F.instance_norm`` on the same fp32 values.  The bar is the split
family's (tests/test_split_numerics.py): 4 x the max-abs error of the stock fp32 op on the same input, on the same device, + 3e-7 max|ref|.
test_instancenorm_f32_cpu.py holds the torch restatement of the kernel's arithmetic to the same bar; here the kernel is also held to
the restatement bit for bit (the kernel is compiled without contraction, and each of its operations is correctly rounded)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import alo_hip
import guarded
import kernel_bounds as kb
from instancenorm_f32_ref import instancenorm_rows, reference_and_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last

# (B, HW, C) -> (H, W): one row; less than a chunk; either side of the 256-row chunk; several chunks, ragged; C = 256 (4 batches a thread)
SHAPES = {(3, 1, 64): (1, 1), (2, 63, 64): (7, 9), (2, 255, 128): (15, 17), (2, 257, 128): (257, 1), (3, 37 * 29, 64): (37, 29),
          (1, 4 * 256 + 5, 256): (3, 343)}
SHAPE_IDS = [f"B{b}-HW{hw}-C{c}" for b, hw, c in SHAPES]
RELU = pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])


@functools.lru_cache(maxsize=None)
def _inputs(shape, ill):
    """(B, C, H, W) fp32 on the CPU, never written to: ordinary values whose channel scales run from 1e-3 to 1e3 around channel means
    of order 1, or (``ill``) kernel_bounds.groupnorm_ill_inputs with groups = C — mean / std in {0.25, 16, 100} and a constant channel."""
    b, hw, c = shape
    h, w = SHAPES[shape]
    if ill:
        x = kb.groupnorm_ill_inputs(b, c, hw, c, "cpu", seed=c + hw).float()
    else:
        g = torch.Generator().manual_seed(1000 * b + hw + c)
        x = torch.randn(b, c, hw, generator=g) * torch.logspace(-3, 3, c).view(1, -1, 1) + torch.randn(b, c, 1, generator=g)
    return x.view(b, c, h, w)


def _on_gpu(x):
    return x.to(DEV).contiguous(memory_format=CL)


def _run(x, relu=False, out=None):
    with torch.no_grad():
        y = alo_hip.instancenorm_nhwc_f32(x, 1e-5, relu, out=out)
    assert y.dtype == torch.float32 and y.shape == x.shape and (out is None or y is out)
    return y


def _check(got, x_gpu, relu, what):
    """The bar, with the stock op's error measured on the device the kernel ran on.  One spatial element: exactly 0 (torch refuses it)."""
    ref, bar, e_stock = reference_and_bar(x_gpu, relu=relu)
    err = (got.double() - ref).abs().max().item()
    print(f"{what}: kernel {err:.3g}  stock fp32 {e_stock:.3g}  bar {bar:.3g}")
    assert torch.isfinite(got).all() and err <= bar, (what, err, bar)


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
@pytest.mark.parametrize("ill", [False, True], ids=["ordinary", "ill-conditioned"])
@RELU
def test_matches_fp64_instance_norm_in_place_and_out_of_place(shape, ill, relu):
    x = _on_gpu(_inputs(shape, ill))
    keep = x.clone()
    got = _run(x, relu)
    assert got.is_contiguous(memory_format=CL) and torch.equal(x, keep)             # out of place: the input is left alone
    _check(got, x, relu, f"{shape} ill={ill} relu={relu}")
    if ill and shape[1] > 1:
        assert (got[:, 3::4] == 0).all()                                            # a constant channel: exactly 0
    if relu:
        assert (got >= 0).all()
    inplace = _run(keep, relu, out=keep)
    assert torch.equal(inplace, got)                                                # in place: the same bits
    b, hw, c = shape
    want = instancenorm_rows(x.permute(0, 2, 3, 1).reshape(b, hw, c).cpu(), 1e-5, relu)
    assert torch.equal(got.permute(0, 2, 3, 1).reshape(b, hw, c).cpu(), want)       # the restated arithmetic, bit for bit


@pytest.mark.parametrize("shape", [(2, 63, 64), (2, 257, 128), (3, 37 * 29, 64)], ids=lambda s: "x".join(map(str, s)))
def test_images_further_apart_than_their_rows_keep_the_gap(shape):
    """``y_batch_stride > HW * C``: the images of ``out`` lie inside a larger buffer; under the guarded launch a changed gap byte, a
    store outside the buffers or a result that depends on the workspace's old contents is an error."""
    b, hw, c = shape
    h, w = SHAPES[shape]
    x = _on_gpu(_inputs(shape, False))
    big = torch.full((b, hw + 3, c), 7.0, device=DEV)
    out = big[:, 2:2 + hw].view(b, h, w, c).permute(0, 3, 1, 2)
    assert out.stride(0) == (hw + 3) * c
    with guarded.GuardedLaunches() as g:
        got = _run(x, True, out=out)
    assert g.seen == [("alo_groupnorm_rows_act", f"instancenorm_f32/C={c}")], g.seen
    assert torch.equal(got, _run(x, True))
    assert (big[:, :2] == 7).all() and (big[:, 2 + hw:] == 7).all()
    with guarded.GuardedLaunches():
        assert torch.equal(_run(x.clone(), True, out=None), got)
        y = x.clone()
        assert torch.equal(_run(y, True, out=y), got)                               # in place under the guard as well


@pytest.mark.parametrize("bad", [kb.NAN, kb.INF, -kb.INF], ids=["nan", "+inf", "-inf"])
@RELU
def test_non_finite_element_spoils_exactly_its_own_image_and_channel(bad, relu):
    shape = (3, 37 * 29, 64)
    x = _on_gpu(_inputs(shape, False))
    clean = _run(x, relu)
    y = x.clone()
    y[1, 5, 20, 11] = bad                                                           # chunk 2 of image 1
    got = _run(y, relu)
    stock = F.instance_norm(y)
    assert not torch.isfinite(stock[1, 5]).any() and not torch.isfinite(got[1, 5]).any()      # as torch makes it
    keep = torch.ones(3, 64, dtype=torch.bool, device=DEV)
    keep[1, 5] = False
    assert torch.equal(got[keep], clean[keep])                                      # every other (image, channel): the clean run's bits


def test_two_runs_are_bit_for_bit_equal():
    for shape in ((3, 37 * 29, 64), (1, 4 * 256 + 5, 256)):
        x = _on_gpu(_inputs(shape, True))
        assert torch.equal(_run(x, True), _run(x, True))


def test_launch_tag_and_one_launch_per_call():
    x = _on_gpu(_inputs((2, 255, 128), False))
    with alo_hip.LaunchTimer() as t:
        _run(x, True)
    assert {k: v["calls"] for k, v in t.summary().items()} == {"instancenorm_f32/C=128": 1}


def test_bf16_groupnorm_is_untouched_by_fp32_calls():
    g = torch.Generator(device=DEV).manual_seed(3)
    norm = torch.nn.GroupNorm(8, 64).to(DEV).bfloat16()
    with torch.no_grad():
        norm.weight.copy_(torch.randn(64, device=DEV, generator=g))
        norm.bias.copy_(torch.randn(64, device=DEV, generator=g))
        xb = torch.randn(2, 64, 19, 23, device=DEV, generator=g).bfloat16().contiguous(memory_format=CL)
        before = alo_hip.groupnorm_nhwc(xb, norm, relu=True)
        _run(_on_gpu(_inputs((2, 257, 128), False)), True)
        after = alo_hip.groupnorm_nhwc(xb, norm, relu=True)
    assert torch.equal(before, after)
    ref, bound = kb.groupnorm_ref_and_bound(xb, 8, norm.weight, norm.bias, norm.eps, relu=True)
    kb.compare(after, ref, bound, "groupnorm_nhwc after an fp32 InstanceNorm")


def test_wrapper_refuses_what_the_kernel_does_not_serve():
    x = torch.randn(1, 64, 5, 6, device=DEV)
    assert not alo_hip.instancenorm_nhwc_f32_supported(x)                           # NCHW
    assert alo_hip.instancenorm_nhwc_f32_supported(x.contiguous(memory_format=CL))
    assert not alo_hip.instancenorm_nhwc_f32_supported(torch.randn(1, 96, 5, 6, device=DEV).contiguous(memory_format=CL))
    assert not alo_hip.instancenorm_nhwc_f32_supported(x.contiguous(memory_format=CL).bfloat16())
    with pytest.raises(RuntimeError, match="instancenorm_nhwc_f32: needs"):
        alo_hip.instancenorm_nhwc_f32(x)
    with pytest.raises(RuntimeError, match="out must be"):
        alo_hip.instancenorm_nhwc_f32(x.contiguous(memory_format=CL), out=torch.empty_like(x))           # an NCHW out
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.instancenorm_nhwc_f32(x.contiguous(memory_format=CL).requires_grad_())
