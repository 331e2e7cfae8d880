"""alo_hip.conv3x3_f32 (alo_conv3x3_nhwc with dtype = ALO_F32, aloception-oss_amd/csrc/conv_f32.hip) against F.conv2d in fp64 on the
same fp32 operands, per output element, within the bound derived in conv_f32_ref.py — which test_conv3x3_f32_cpu.py holds the
numpy restatement of the kernel's arithmetic to, so what is asked of the kernel here has been checked without a GPU."""
import functools

import pytest
import torch

import alo_hip
from conv_f32_ref import reference_and_bound
from kernel_bounds import INF, NAN, compare

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, H, W): where the kernel can go wrong
SHAPES = [
    (1, 64, 64, 1, 1),          # one pixel: every tap but the centre is padding; Cout = 64: the two waves split K
    (1, 64, 128, 2, 2),
    (2, 128, 64, 5, 7),         # rows shorter than a tile, a tile crossing row ends
    (2, 192, 128, 9, 66),       # a tile boundary inside a row; 192 = RAFT's odd multiple of 64
    (3, 256, 192, 13, 11),      # a column block whose second wave has no channels
    (1, 128, 256, 64, 3),       # two column blocks, narrow rows
    (2, 256, 64, 12, 20),       # flow_head.conv2 padded to 64 output channels
    (2, 1024, 512, 13, 11),     # few tiles, 64 channel chunks
]


@functools.lru_cache(maxsize=None)
def _operands(shape, scale=1.0):
    """x (channels-last), w, b on the CPU: drawn once per shape, never written to."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + cin + cout + 7 * h + w)
    x = (torch.randn(n, cin, h, w, generator=g) * scale).contiguous(memory_format=torch.channels_last)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * scale
    return x, wt, b


def _run(x, wt, b, stride, relu):
    with torch.no_grad():
        y = alo_hip.conv3x3_f32(x.cuda().contiguous(memory_format=torch.channels_last), wt.cuda(), None if b is None else b.cuda(),
                                relu=relu, stride=stride)
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    return y.cpu()


@pytest.mark.parametrize("relu_bias", [True, False], ids=["relu+bias", "plain"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_meets_the_bound(shape, stride, relu_bias):
    x, wt, b = _operands(shape)
    b = b if relu_bias else None
    ref, bound = reference_and_bound(x, wt, b, stride, relu_bias)
    got = _run(x, wt, b, stride, relu_bias)
    ratio = compare(got, ref, bound, f"conv3x3_f32 {shape} stride {stride}")
    print(f"conv3x3_f32 {shape} s={stride} relu+bias={relu_bias}: worst |err| / bound = {ratio:.4f}, "
          f"max |err| / max |ref| = {((got.double() - ref).abs().max() / ref.abs().max()).item():.3g}")


MAG_SHAPE = (2, 128, 64, 5, 7)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("scale", [1e-20, 1.0, 3e4, 5e18])
def test_kernel_meets_the_bound_at_any_input_magnitude(scale, stride):
    x, wt, b = _operands(MAG_SHAPE, scale)
    ref, bound = reference_and_bound(x, wt, b, stride, True)
    ratio = compare(_run(x, wt, b, stride, True), ref, bound, f"conv3x3_f32 inputs at {scale} stride {stride}")
    print(f"inputs at {scale}, stride {stride}: worst |err| / bound = {ratio:.4f}")


@pytest.mark.parametrize("stride", [1, 2])
def test_a_dim_image_next_to_a_bright_one_keeps_its_accuracy_and_its_bits(stride):
    x, wt, b = _operands(MAG_SHAPE)
    x = x.clone()
    x[1] *= 1e-6
    b = b * 1e-6
    ref, bound = reference_and_bound(x, wt, b, stride, False)
    got = _run(x, wt, b, stride, False)
    compare(got, ref, bound, f"conv3x3_f32 items 10^6 apart, stride {stride}")
    alone = _run(x[1:], wt, b, stride, False)
    assert torch.equal(alone[0], got[1]), "the dim image's result depends on its batch neighbour"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
def test_non_finite_inputs_spoil_exactly_their_windows(stride, relu):
    x, wt, b = _operands(MAG_SHAPE)
    x = x.clone()
    x[0, 5, 2, 3] = INF          # one element: the outputs around it are infinities of the weight's sign
    x[0, 77, 4, 6] = -INF
    x[1, :, 1, 5] = NAN          # a whole pixel
    ref, bound = reference_and_bound(x, wt, b, stride, relu)
    assert (~torch.isfinite(ref)).any() and torch.isinf(ref).any() and torch.isnan(ref).any() and torch.isfinite(ref).any()
    compare(_run(x, wt, b, stride, relu), ref, bound, f"conv3x3_f32 with Inf / NaN inputs, stride {stride}")


def test_supported_gate():
    x = torch.randn(1, 128, 6, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    w = torch.randn(64, 128, 3, 3, device="cuda")
    with torch.no_grad():
        assert alo_hip.conv3x3_f32_supported(x, w) and alo_hip.conv3x3_f32_supported(x, w, stride=(2, 2))
        assert not alo_hip.conv3x3_supported(x, w)                                         # the bf16 gate answers as before
        assert not alo_hip.conv3x3_f32_supported(x[:, :96].contiguous(memory_format=torch.channels_last), w[:, :96].contiguous())
        assert not alo_hip.conv3x3_f32_supported(x, w[:40].contiguous())
        assert not alo_hip.conv3x3_f32_supported(x.contiguous(), w)                        # NCHW
        assert not alo_hip.conv3x3_f32_supported(x, w, stride=(3, 3))
        assert not alo_hip.conv3x3_f32_supported(x, w, dilation=(2, 2))
        assert not alo_hip.conv3x3_f32_supported(x, w.bfloat16())
        assert not alo_hip.conv3x3_f32_supported(x.bfloat16(), w.bfloat16())
        with pytest.raises(RuntimeError, match="conv3x3_f32: needs"):
            alo_hip.conv3x3_f32(x.contiguous(), w)
    assert not alo_hip.conv3x3_f32_supported(x, w)                                         # grad mode on: no backward
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.conv3x3_f32(x, w.requires_grad_())


def test_split_weights_are_cached_on_the_weight_and_follow_it():
    x, wt, b = _operands(MAG_SHAPE)
    xg, wg = x.cuda().contiguous(memory_format=torch.channels_last), wt.cuda()
    with torch.no_grad():
        y0 = alo_hip.conv3x3_f32(xg, wg)
        pack = wg.__dict__["_alo_derived"]["conv3x3_f32_b"][1]
        assert alo_hip.conv3x3_f32(xg, wg) is not None and wg.__dict__["_alo_derived"]["conv3x3_f32_b"][1] is pack
        wg.mul_(2.0)                                                                       # a new version: re-derived
        y1 = alo_hip.conv3x3_f32(xg, wg)
    assert wg.__dict__["_alo_derived"]["conv3x3_f32_b"][1] is not pack
    assert torch.equal(y1, 2.0 * y0)                                                       # a power of two moves the exponents only
