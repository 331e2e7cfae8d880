"""alo_hip.conv_taps_f32 (alo_conv3x3_nhwc with ALO_CONV_TAPS_1X5 / ALO_CONV_TAPS_5X1 and dtype = ALO_F32; conv_taps_f32_kernel of
aloception-oss_amd/csrc/conv_f32.hip) against F.conv2d in fp64 on the same fp32 operands, per output element, within the bound of
conv_taps_f32_ref.py — which test_conv_taps_f32_cpu.py holds the numpy restatement of the kernel's arithmetic to."""
import functools

import pytest
import torch

import alo_hip
import guarded
from conv_taps_f32_ref import PADDING, reference_and_bound, reference_parts
from kernel_bounds import INF, NAN, compare

pytestmark = pytest.mark.gpu
GEOMETRIES = pytest.mark.parametrize("vertical", [False, True], ids=["1x5", "5x1"])

# (N, Cin, Cout, H, W): where the kernel can go wrong
SHAPES = [
    (1, 64, 64, 1, 1),          # every tap but the centre is outside; Cout = 64: the two waves split K
    (1, 64, 64, 1, 5),          # a window as wide as the image / a column of one-pixel rows
    (1, 64, 64, 5, 1),
    (2, 64, 128, 3, 4),         # both sides shorter than the window
    (1, 64, 64, 7, 11),         # 77 pixels: rows cross the tile boundary, the second tile is ragged, K-split
    (2, 128, 256, 9, 13),       # tiles straddle the image boundary, two column blocks
    (1, 384, 256, 12, 16),      # SepConvGRU's [z | r] convolution
    (1, 384, 128, 12, 16),      # SepConvGRU's q convolution
    (1, 64, 64, 130, 520),      # 1057 tiles (the last one ragged) on the launch's 1024 persistent workgroups
]


@functools.lru_cache(maxsize=None)
def _operands(shape, vertical, scale=1.0):
    """x (channels-last), w, b on the CPU: drawn once per shape and geometry, never written to."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + cin + cout + 7 * h + w + vertical)
    x = (torch.randn(n, cin, h, w, generator=g) * scale).contiguous(memory_format=torch.channels_last)
    wt = torch.randn(cout, cin, *((5, 1) if vertical else (1, 5)), generator=g) / (5 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * scale
    return x, wt, b


@functools.lru_cache(maxsize=None)
def _parts(shape, vertical):
    """The fp64 convolutions behind reference and bound: once per shape and geometry, shared by the bias / ReLU cases."""
    x, wt, _ = _operands(shape, vertical)
    return reference_parts(x, wt)


def _reference(shape, vertical, bias, relu):
    x, wt, b = _operands(shape, vertical)
    return reference_and_bound(x, wt, b if bias else None, relu, _parts(shape, vertical))


def _run(x, wt, b, relu):
    with torch.no_grad():
        y = alo_hip.conv_taps_f32(x.cuda().contiguous(memory_format=torch.channels_last), wt.cuda(), None if b is None else b.cuda(), relu=relu)
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last) and y.shape == (x.shape[0], wt.shape[0], *x.shape[2:])
    return y.cpu()


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@GEOMETRIES
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_meets_the_bound(shape, vertical, bias, relu):
    x, wt, b = _operands(shape, vertical)
    ref, bound = _reference(shape, vertical, bias, relu)
    got = _run(x, wt, b if bias else None, relu)
    ratio = compare(got, ref, bound, f"conv_taps_f32 {shape} vertical={vertical}")
    print(f"conv_taps_f32 {shape} vertical={vertical} bias={bias} relu={relu}: worst |err| / bound = {ratio:.4f}, "
          f"max |err| / max |ref| = {((got.double() - ref).abs().max() / ref.abs().max()).item():.3g}")


MAG_SHAPE = (2, 128, 64, 5, 7)


@GEOMETRIES
@pytest.mark.parametrize("scale", [1e-20, 1.0, 3e4, 5e18])
def test_kernel_meets_the_bound_at_any_input_magnitude(scale, vertical):
    x, wt, b = _operands(MAG_SHAPE, vertical, scale)
    ref, bound = reference_and_bound(x, wt, b, True)
    ratio = compare(_run(x, wt, b, True), ref, bound, f"conv_taps_f32 inputs at {scale} vertical={vertical}")
    print(f"inputs at {scale}, vertical={vertical}: worst |err| / bound = {ratio:.4f}")


@GEOMETRIES
def test_a_dim_image_next_to_a_bright_one_keeps_its_accuracy_and_its_bits(vertical):
    x, wt, b = _operands(MAG_SHAPE, vertical)
    x = x.clone()
    x[1] *= 1e-6
    b = b * 1e-6
    ref, bound = reference_and_bound(x, wt, b, False)
    got = _run(x, wt, b, False)
    compare(got, ref, bound, f"conv_taps_f32 items 10^6 apart, vertical={vertical}")
    for i in range(2):
        alone = _run(x[i:i + 1], wt, b, False)
        assert torch.equal(alone[0].view(torch.int32), got[i].view(torch.int32)), f"image {i}'s result depends on its batch neighbour"


@pytest.mark.parametrize("relu", [False, True])
@GEOMETRIES
def test_non_finite_inputs_spoil_exactly_their_windows(vertical, relu):
    x, wt, b = _operands(MAG_SHAPE, vertical)
    clean = _run(x, wt, b, relu)
    x = x.clone()
    x[0, 5, 2, 3] = INF          # one element: the outputs around it are infinities of the weight's sign
    x[0, 77, 4, 6] = -INF        # the image's last pixel
    x[1, :, 1, 5] = NAN          # a whole pixel
    holds = torch.zeros(x.shape[0], 1, *x.shape[2:])
    holds[0, 0, 2, 3] = holds[0, 0, 4, 6] = holds[1, 0, 1, 5] = 1
    window = torch.nn.functional.conv2d(holds, torch.ones(1, 1, *wt.shape[2:]), None, 1, PADDING[vertical]) > 0   # (N, 1, H, W)
    ref, bound = reference_and_bound(x, wt, b, relu)
    assert torch.isinf(ref).any() and torch.isnan(ref).any() and torch.isfinite(ref).any()
    got = _run(x, wt, b, relu)
    compare(got, ref, bound, f"conv_taps_f32 with Inf / NaN inputs, vertical={vertical}")       # fp64's kind where it is not finite
    assert not (~torch.isfinite(ref) & ~window).any() and (relu or (~torch.isfinite(ref) | ~window).all())   # (ReLU turns -inf into 0)
    assert (torch.isfinite(got) == torch.isfinite(ref)).all()
    keep = ~window.expand_as(got)
    assert torch.equal(got.view(torch.int32)[keep], clean.view(torch.int32)[keep]), "an output outside every spoiled window changed"


@GEOMETRIES
def test_two_calls_give_equal_bits(vertical):
    x, wt, b = _operands((2, 128, 256, 9, 13), vertical)
    first, second = _run(x, wt, b, True), _run(x, wt, b, True)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))


@GEOMETRIES
@pytest.mark.parametrize("shape", [(1, 64, 64, 7, 11), (1, 384, 256, 12, 16)], ids=lambda s: "x".join(map(str, s)))
def test_launch_stays_in_its_buffers_and_ignores_stale_bytes(shape, vertical):
    x, wt, b = _operands(shape, vertical)
    ref, bound = _reference(shape, vertical, True, True)
    with guarded.GuardedLaunches() as g:
        got = _run(x, wt, b, True)
    name = "5x1" if vertical else "1x5"      # (the split weight's two alo_pack_mfma_b launches run under the guard as well)
    assert [tag for s, tag in g.seen if s == "alo_conv3x3_nhwc"] == [f"conv{name}_f32/C={shape[1]}"], g.seen
    compare(got, ref, bound, f"guarded conv_taps_f32 {shape} vertical={vertical}")


def test_supported_gate():
    x = torch.randn(1, 128, 6, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    w15, w51 = torch.randn(64, 128, 1, 5, device="cuda"), torch.randn(64, 128, 5, 1, device="cuda")
    with torch.no_grad():
        assert alo_hip.conv_taps_f32_supported(x, w15, (0, 2)) and alo_hip.conv_taps_f32_supported(x, w51, (2, 0))
        assert not alo_hip.conv_taps_f32_supported(x, w15, (2, 0)) and not alo_hip.conv_taps_f32_supported(x, w51, (0, 2))
        assert not alo_hip.conv_taps_f32_supported(x, w15, (0, 0))
        assert not alo_hip.conv_taps_f32_supported(x, torch.randn(64, 128, 3, 3, device="cuda"), (1, 1))
        assert not alo_hip.conv_taps_f32_supported(x[:, :96].contiguous(memory_format=torch.channels_last), w15[:, :96].contiguous(), (0, 2))
        assert not alo_hip.conv_taps_f32_supported(x, w15[:40].contiguous(), (0, 2))
        assert not alo_hip.conv_taps_f32_supported(x.contiguous(), w15, (0, 2))                 # NCHW
        assert not alo_hip.conv_taps_f32_supported(x.bfloat16(), w15.bfloat16(), (0, 2))
        with pytest.raises(RuntimeError, match="conv_taps_f32: needs"):
            alo_hip.conv_taps_f32(x.contiguous(), w15)
    assert not alo_hip.conv_taps_f32_supported(x, w15, (0, 2))                                  # grad mode on: no backward
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.conv_taps_f32(x, w15.requires_grad_())


def test_split_weights_are_cached_on_the_weight_and_follow_it():
    x, wt, b = _operands(MAG_SHAPE, True)
    xg, wg = x.cuda().contiguous(memory_format=torch.channels_last), wt.cuda()
    with torch.no_grad():
        y0 = alo_hip.conv_taps_f32(xg, wg)
        pack = wg.__dict__["_alo_derived"]["conv_taps_f32_b"][1]
        assert alo_hip.conv_taps_f32(xg, wg) is not None and wg.__dict__["_alo_derived"]["conv_taps_f32_b"][1] is pack
        wg.mul_(2.0)                                                                       # a new version: re-derived
        y1 = alo_hip.conv_taps_f32(xg, wg)
    assert wg.__dict__["_alo_derived"]["conv_taps_f32_b"][1] is not pack
    assert torch.equal(y1, 2.0 * y0)                                                       # a power of two moves the exponents only
