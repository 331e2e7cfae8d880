"""conv3x3_pipe_kernel<PipeS2<..>> (conv.hip): the stride-2 3x3 convolution of 128 and more output channels on the pipelined loop.

It replaces conv3x3_kernel<PlanS2, false> for bf16, stride 2, no dilation, Cout >= 128, no split-K, and keeps that kernel's arithmetic and
its halo (per tap row a run of odd-column and a run of even-column input pixels, clamped into the image, out-of-image taps zeroed by
selection), so the outputs must be the streaming kernel's bit for bit.  ALO_CONV3X3_PIPE=stride1 (read on every call) keeps stride 2 on
the streaming kernel and stride 1 on the pipelined one, "off" sends both back.  Cout >= 256 runs tiles of 96 output pixels x 256
channels, Cout = 128 / 192 tiles of 128 x 128: the maps below have every parity of H and W and output pixel counts on both sides of
64, 96 and 128, and the long walks give persistent workgroups more than one tile across an image boundary.

As in test_conv3x3_pipe_gpu.py the `one_pass` fixture passes every launch of the route's shapes WITHOUT a workspace (no workspace, no
split-K) and records them; each test asserts that what it compared met the gate of alo_conv3x3_nhwc (bf16, stride 2, no dilation,
Cout >= 128, no workspace).  Which kernel a launch then runs rests on the gate as written in conv.hip.
"""
import pytest
import torch
import torch.nn.functional as F

import alo_hip
from guarded import GuardedLaunches
from test_backbone_kernels_gpu import check_conv3x3
from test_conv3x3_pipe_gpu import backbone, bits, operands

pytestmark = pytest.mark.gpu
DEV = "cuda"

CHANNELS = [(64, 128),     # one body of two chunks: the pipeline's prologue and epilogue meet
            (128, 128),
            (192, 192),    # three bodies; the last column block's second half has no columns
            (256, 256),    # two column blocks of the streaming kernel, one of the 256-wide tile
            (512, 512),
            (128, 256)]
# input maps: every parity of H and W; 1-4, 63, 64, 64, 65, 96, 97, 128, 128 and 129 output pixels
MAPS = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (13, 17), (15, 16), (16, 16), (9, 25), (15, 24), (1, 193), (16, 31), (15, 32), (5, 85)]
BATCHES = [1, 3]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]   # (with_bias, relu)
# Outputs of 181 x 183 and 161 x 163: more tiles than the 512 resident workgroups, a ragged last tile, a walk across the image boundary
# (518 tiles of 128 / 548 tiles of 96; the workgroups step 64 tiles inside their XCD's contiguous eighth)
LONG_WALKS = [(2, 128, 128, 361, 365), (2, 256, 256, 321, 325)]


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def conv(x, wt, b, relu):
    with torch.no_grad():
        return alo_hip.conv3x3(x, wt, b, relu=relu, stride=2)


@pytest.fixture(autouse=True)
def no_knob(monkeypatch):
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)


@pytest.fixture
def one_pass(monkeypatch):
    """Stride-2 launches of the route's shapes go without a workspace; -> the list of (Cin, Cout, input pixels per image) so launched."""
    real, routed = alo_hip._launch, []

    def launch(symbol, device, tag, nbytes, flops, *args, **kw):
        # alo_conv3x3_nhwc(x, w_packed, bias, y, workspace, N, H, W, Cin, Cout, stride, relu, dtype)
        if symbol == "alo_conv3x3_nhwc" and args[10] == 2 and args[9] >= 128 and args[12] == alo_hip.ALO_BF16:
            args = args[:4] + (None,) + args[5:]
            routed.append((args[8], args[9], args[6] * args[7]))
        return real(symbol, device, tag, nbytes, flops, *args, **kw)

    monkeypatch.setattr(alo_hip, "_launch", launch)
    return routed


def both(x, wt, b, relu, monkeypatch):
    """(the default route, the streaming kernel) on the same operands"""
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    got = conv(x, wt, b, relu)
    monkeypatch.setenv("ALO_CONV3X3_PIPE", "stride1")
    stream = conv(x, wt, b, relu)
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    return got, stream


def check_fp32(x, wt, b, relu, got):
    """The bar of test_fused_gpu.py::test_conv3x3_matches_fp32_convolution, then the fp64 one."""
    with torch.no_grad():
        ref = F.conv2d(x.float(), wt.float(), None if b is None else b.float(), 2, 1)
        if relu:
            ref = F.relu(ref)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert (got.float() - ref).abs().max().item() <= 2.0 ** -8 * max(1.0, ref.abs().max().item())
    check_conv3x3(x, wt, b, relu, 2, got)


def test_the_maps_cover_every_parity_and_both_tile_sizes():
    assert {(h % 2, w % 2) for h, w in MAPS if h > 2 and w > 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    pixels = {ho * wo for ho, wo in (out_hw(h, w) for h, w in MAPS)}
    assert {1, 4, 63, 64, 65, 96, 97, 128, 129} <= pixels


@pytest.mark.parametrize("with_bias,relu", FLAGS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_same_bits_as_the_streaming_kernel_and_the_fp32_bar(cin, cout, with_bias, relu, monkeypatch, one_pass):
    for n in BATCHES:
        for h, w in MAPS:
            x, wt, b = operands(n, cin, cout, h, w)
            b = b if with_bias else None
            got, stream = both(x, wt, b, relu, monkeypatch)
            assert got.shape == stream.shape == (n, cout) + out_hw(h, w), (n, h, w)
            assert torch.equal(bits(got), bits(stream)), (n, h, w)
            check_fp32(x, wt, b, relu, got)
    assert one_pass == [(cin, cout, h * w) for n in BATCHES for h, w in MAPS for _ in range(2)]


@pytest.mark.parametrize("with_bias,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("shape", LONG_WALKS, ids=str)
def test_long_walk_across_the_image_boundary(shape, with_bias, relu, monkeypatch, one_pass):
    x, wt, b = operands(*shape)
    b = b if with_bias else None
    got, stream = both(x, wt, b, relu, monkeypatch)
    assert torch.equal(bits(got), bits(stream))
    check_fp32(x, wt, b, relu, got)
    assert one_pass == [(shape[1], shape[2], shape[3] * shape[4])] * 2


def reach(h, w, pixels):
    """The outputs whose 3x3 stride-2 window holds one of the input pixels."""
    ho, wo = out_hw(h, w)
    inside = torch.zeros(ho, wo, dtype=torch.bool, device=DEV)
    for py, px in pixels:
        for yo in range(ho):
            for xo in range(wo):
                if abs(py - 2 * yo) <= 1 and abs(px - 2 * xo) <= 1:
                    inside[yo, xo] = True
    return inside


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("cin,cout", [(128, 128), (256, 256), (512, 512)])
@pytest.mark.parametrize("h,w", [(16, 18), (17, 23), (16, 23), (17, 18)])
def test_nan_in_border_pixels_reaches_exactly_its_windows(h, w, cin, cout, relu, monkeypatch, one_pass):
    """The halo's loads are clamped into the image and out-of-image taps are zeroed by selection.  At even H the last outputs' bottom
    tap is the real row H - 1; at odd H it is row H, outside the image, and its load is clamped onto row H - 1 (columns alike).  A NaN
    in the last row or column therefore reaches the outputs whose window holds it and never leaks through a masked tap; ReLU keeps it
    there, and no other output changes."""
    x, wt, b = operands(1, cin, cout, h, w)
    clean = conv(x, wt, b, relu)
    for pixels in ([(0, 0)], [(h - 1, w - 1)], [(h - 1, 3), (4, w - 1)], [(0, w - 1), (h - 1, 0)]):
        xn = x.clone(memory_format=torch.preserve_format)
        for py, px in pixels:
            xn[0, :, py, px] = float("nan")
        got, stream = both(xn, wt, b, relu, monkeypatch)
        inside = reach(h, w, pixels)
        assert bool(inside.any())
        assert torch.isnan(got[0][:, inside]).all(), pixels
        assert torch.equal(bits(got)[0][:, ~inside], bits(clean)[0][:, ~inside]), pixels
        assert torch.equal(bits(got), bits(stream)), pixels
    assert one_pass == [(cin, cout, h * w)] * 9


@pytest.mark.parametrize("shape,pix", [(LONG_WALKS[0], 128), (LONG_WALKS[1], 96)], ids=str)
def test_nan_and_inf_in_every_tile_of_one_walk(shape, pix, monkeypatch, one_pass):
    """Workgroup 0 takes tiles 0 and 64 of image 0 (518 / 548 tiles, 65 / 69 per XCD, 64 workgroups per XCD): NaN, +Inf and -Inf sit
    under the first, a middle and the last output pixel of both, and in the image's last row and column."""
    n, cin, cout, h, w = shape
    ho, wo = out_hw(h, w)
    assert -(-ho * wo // pix) * n > 512 and 64 * pix + pix <= ho * wo
    x, wt, b = operands(*shape)
    xn = x.clone(memory_format=torch.preserve_format)
    for tile in (0, 64):
        for p, v in ((tile * pix, "nan"), (tile * pix + pix // 2, "inf"), (tile * pix + pix - 1, "-inf")):
            xn[0, : cin // 2, 2 * (p // wo), 2 * (p % wo)] = float(v)
    xn[0, 0, h - 1, :] = float("inf")
    xn[1, 1, :, w - 1] = float("nan")
    got, stream = both(xn, wt, b, True, monkeypatch)
    assert not bool(torch.isfinite(got[0, :, 0, 0].float()).any()) and bool(torch.isnan(got[1, :, :, wo - 1]).all())
    assert bool(torch.isfinite(got[1, :, :, : wo - 1].float()).all())
    assert torch.equal(bits(got), bits(stream))
    assert one_pass == [(cin, cout, h * w)] * 2


@pytest.mark.parametrize("shape", [(3, 128, 128, 9, 25), (1, 192, 192, 16, 31), (3, 256, 256, 13, 17), (1, 512, 512, 15, 24)], ids=str)
def test_launches_stay_in_their_buffers_and_ignore_stale_bytes(shape, one_pass):
    """tests/guarded.py: the launch runs twice between guard zones, y pre-filled with 0xFF and with 0x3C bytes; no byte outside y may
    change and y must have the same bits under both fills.  (The guarded launches go through `one_pass`: it is the launch function
    GuardedLaunches finds on entry.)"""
    x, wt, b = operands(*shape)
    plain = conv(x, wt, b, True)
    with GuardedLaunches() as g:
        got = conv(x, wt, b, True)
    assert "alo_conv3x3_nhwc" in {symbol for symbol, _ in g.seen}
    assert torch.equal(bits(got), bits(plain))
    assert one_pass == [(shape[1], shape[2], shape[3] * shape[4])] * 3     # plain, and one per fill


# ---- the bf16 backbone ------------------------------------------------------------------------------------------------------------------
# the three stride-2 convolutions on a 72 x 104 input, conv2 of layer2.0 / layer3.0 / layer4.0: (Cin, Cout, input pixels per image)
BODY_ROUTED = [(128, 128, 18 * 26), (256, 256, 9 * 13), (512, 512, 5 * 7)]
KNOBS = [None, "stride1", "off"]


def set_knob(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    else:
        monkeypatch.setenv("ALO_CONV3X3_PIPE", value)


@pytest.fixture(params=["as the wrapper launches", "one pass"])
def body_launches(request):
    """The backbone as alo_hip.conv3x3 launches it (a launch that is handed a workspace may split K and stay on the streaming kernel)
    and with every stride-2 launch in one pass (all three reach the gate); -> the record of the latter, else None."""
    return request.getfixturevalue("one_pass") if request.param == "one pass" else None


def test_resnet_body_eager(monkeypatch, body_launches):
    body, x = backbone()
    stages = []
    for knob in KNOBS:
        set_knob(monkeypatch, knob)
        with alo_hip.LaunchTimer() as t, torch.no_grad():
            stages.append({k: v.clone() for k, v in body(x).items()})
        assert {"conv3x3/C=128/s=2", "conv3x3/C=256/s=2", "conv3x3/C=512/s=2"} <= set(t.summary())
    if body_launches is not None:
        assert body_launches == BODY_ROUTED * 3
    default, stride1, off = stages
    assert default.keys() == stride1.keys() == off.keys() and len(default) == 4
    for k in default:
        assert bool(torch.isfinite(default[k].float()).all())
        assert torch.equal(bits(default[k]), bits(stride1[k])) and torch.equal(bits(default[k]), bits(off[k])), k


def _captured(body, x, knob, monkeypatch):
    """The stages of two replays of one captured forward: on a zeroed input, then on x."""
    set_knob(monkeypatch, knob)
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        body(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = body(static_x)
    static_x.zero_()
    graph.replay()
    zeroed = {k: v.clone() for k, v in out.items()}
    static_x.copy_(x)
    graph.replay()
    real = {k: v.clone() for k, v in out.items()}
    torch.cuda.synchronize()
    return zeroed, real


def test_resnet_body_under_graph_capture(monkeypatch, body_launches):
    body, x = backbone()
    zero, real = zip(*[_captured(body, x, knob, monkeypatch) for knob in KNOBS])
    if body_launches is not None:
        assert body_launches == BODY_ROUTED * 6     # per knob the warm-up forward and the captured one
    with torch.no_grad():
        eager_off = body(x)   # the knob is still "off"
    for k in real[0]:
        for other in (1, 2):
            assert torch.equal(bits(real[0][k]), bits(real[other][k])), (k, KNOBS[other])
            assert torch.equal(bits(zero[0][k]), bits(zero[other][k])), (k, KNOBS[other])
        assert torch.equal(bits(real[0][k]), bits(eager_off[k])), k
        assert not torch.equal(bits(zero[0][k]), bits(real[0][k])), k
