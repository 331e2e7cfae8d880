"""conv3x3_c64_kernel (conv.hip): the 64 -> 64 stride-1 convolution with its weights resident in registers.

It replaces conv3x3_kernel<PlanS1<1>, true> for that one shape class and keeps its summation: the same K split over two halves, each half
accumulated in the same order, half 0 + half 1, + bias, ReLU, one rounding.  So the outputs must be the streaming kernel's bit for
bit; ALO_CONV3X3_C64=stream (read on every call) routes the shape back to the streaming kernel for the comparison.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import alo_hip
from test_backbone_kernels_gpu import check_conv3x3

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, H, W).  Tiles are 64 flattened pixels of one image; the grid is 8 XCDs x min(ceil(tiles / 8), 64) workgroups.
SHAPES = [(1, 1, 1), (1, 3, 3),
          (1, 1, 70),       # one row wider than a tile
          (1, 9, 7),        # 63 pixels, a ragged single tile
          (1, 8, 8),        # exactly one tile
          (1, 5, 13),       # one pixel in the second tile
          (1, 17, 23),      # tiles that start mid-row, halo rows shared across tiles
          (3, 10, 10),      # image boundaries inside the persistent loop
          (2, 70, 130),     # 286 tiles: every XCD's range is walked by 36 workgroups
          (3, 120, 150)]    # 846 tiles, 106 per XCD on 64 workgroups: the tile loop wraps, across image boundaries too
FLAGS = [(True, True), (True, False), (False, True), (False, False)]   # (with_bias, relu)


@functools.lru_cache(maxsize=None)
def operands(shape, cin=64, cout=64):
    n, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(n * 1000 + h * 31 + w + cin + 7 * cout)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / 24).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(cout, device=DEV, generator=g).to(torch.bfloat16)
    return x, wt, b


@functools.lru_cache(maxsize=None)
def routed_by_default(shape, with_bias, relu):
    """The output as alo_conv3x3_nhwc routes it with no knob set; shared by the tests, never written to."""
    x, wt, b = operands(shape)
    with torch.no_grad():
        return alo_hip.conv3x3(x, wt, b if with_bias else None, relu=relu, stride=1)


def bits(t):
    return t.contiguous(memory_format=torch.channels_last).view(torch.int16)


@pytest.fixture(autouse=True)
def no_knob(monkeypatch):
    monkeypatch.delenv("ALO_CONV3X3_C64", raising=False)


@pytest.mark.parametrize("with_bias,relu", FLAGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_same_bits_as_the_streaming_kernel(shape, with_bias, relu, monkeypatch):
    x, wt, b = operands(shape)
    got = routed_by_default(shape, with_bias, relu)
    monkeypatch.setenv("ALO_CONV3X3_C64", "stream")
    with torch.no_grad():
        stream = alo_hip.conv3x3(x, wt, b if with_bias else None, relu=relu, stride=1)
    assert got.shape == stream.shape == (shape[0], 64, shape[1], shape[2])
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(bits(got), bits(stream))


@pytest.mark.parametrize("with_bias,relu", FLAGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_fp32_convolution(shape, with_bias, relu):
    """The bar of test_fused_gpu.py::test_conv3x3_matches_fp32_convolution: half a bf16 ulp of the largest value against F.conv2d in
    fp32 on the same bf16 operands, then element by element against fp64 (test_backbone_kernels_gpu.check_conv3x3)."""
    x, wt, b = operands(shape)
    b = b if with_bias else None
    got = routed_by_default(shape, with_bias, relu)
    with torch.no_grad():
        ref = F.conv2d(x.float(), wt.float(), None if b is None else b.float(), 1, 1)
        if relu:
            ref = F.relu(ref)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert (got.float() - ref).abs().max().item() <= 2.0 ** -8 * max(1.0, ref.abs().max().item())
    check_conv3x3(x, wt, b, relu, 1, got)


@pytest.mark.parametrize("cin,cout,stride", [(128, 64, 1), (64, 128, 1), (64, 64, 2)])
def test_other_shapes_do_not_see_the_knob(cin, cout, stride, monkeypatch):
    """Only stride 1, Cin = Cout = 64 reaches the new kernel: everything else gives the same bits whatever the knob says."""
    x, wt, b = operands((2, 17, 23), cin, cout)
    with torch.no_grad():
        default = alo_hip.conv3x3(x, wt, b, relu=True, stride=stride)
        monkeypatch.setenv("ALO_CONV3X3_C64", "stream")
        stream = alo_hip.conv3x3(x, wt, b, relu=True, stride=stride)
    assert torch.equal(bits(default), bits(stream))
    check_conv3x3(x, wt, b, True, stride, default)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("py,px", [(5, 22), (8, 0), (0, 0), (16, 11)])   # right edge, left edge, corner, last row
def test_nan_pixel_reaches_only_its_window(py, px, relu):
    """Out-of-image taps are zeroed by selection, not by multiplication, and a flattened halo run wraps into the neighbouring rows:
    a NaN pixel must reach the outputs whose 3x3 window contains it and no other."""
    shape = (1, 17, 23)
    x, wt, b = operands(shape)
    clean = routed_by_default(shape, True, relu)
    xn = x.clone(memory_format=torch.preserve_format)
    xn[0, :, py, px] = float("nan")
    with torch.no_grad():
        got = alo_hip.conv3x3(xn, wt, b, relu=relu, stride=1)
    inside = torch.zeros(shape[1], shape[2], dtype=torch.bool, device=DEV)
    inside[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    assert torch.isnan(got[0][:, inside]).all()
    assert torch.equal(bits(got)[0][:, ~inside], bits(clean)[0][:, ~inside])
