"""conv3x3_pipe_kernel<PipeS1<..>> (conv.hip): the stride-1 3x3 convolution of 128 and more output channels with its LDS reads and weight requests
issued ahead of the MFMAs that use them.

It replaces conv3x3_kernel<PlanS1<1>, false> for bf16, stride 1, no dilation, Cout >= 128, no split-K, and keeps that kernel's arithmetic: every
accumulator starts at zero and takes one v_mfma_f32_32x32x16_bf16 per k-step in the order chunk, tap, channel; out-of-image taps are
zeroed by selection; bias after the sum, ReLU that keeps NaN, one rounding.  So the outputs must be the streaming kernel's bit for bit;
ALO_CONV3X3_PIPE=off (read on every call) routes the shapes back to the streaming kernel for the comparison.  Cout >= 256 runs tiles of
96 pixels x 256 channels (three row tiles per wave), Cout = 128 / 192 tiles of 128 pixels x 128 channels: the maps below are ragged in
both, and the long walk gives persistent workgroups more than one tile across an image boundary.

alo_hip.conv3x3 hands alo_conv3x3_nhwc a split-K workspace whenever alo_conv3x3_workspace_bytes reports one, which it does for 256 and
more input channels on small maps, and a call that splits K is not the route's: with the knob either way it would run the streaming
kernel.  The `one_pass` fixture therefore passes every routed-shape launch WITHOUT a workspace (the header: no workspace, no split-K), so
both kernels make the whole sum in one pass at every size below, and records the launches: each test asserts that what it compared met
the gate of alo_conv3x3_nhwc (bf16, stride 1, no dilation, Cout >= 128, no workspace).  Which kernel a launch then runs is not observable
from outside the library (same tag, same bits, no entry point may be added): that rests on the gate as written in conv.hip.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import alo_hip
from guarded import GuardedLaunches
from test_backbone_kernels_gpu import check_conv3x3

pytestmark = pytest.mark.gpu
DEV = "cuda"

CHANNELS = [(64, 128),     # one chunk: the pipeline's prologue and epilogue meet
            (128, 128),
            (192, 192),    # three chunks; the last column block's second half has no columns
            (256, 256),    # two column blocks of the streaming kernel, one of the 256-wide tile
            (512, 512),
            (128, 256)]
MAPS = [(1, 1), (1, 3), (3, 3), (7, 9), (8, 8), (5, 13), (10, 20)]   # 63, 64 and 65 pixels among them
BATCHES = [1, 3]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]   # (with_bias, relu)
# More tiles than the 512 resident workgroups, so that some take two and the walk crosses the image boundary:
#   181 x 183 = 33123 pixels per image: 518 tiles of 64 (the last one 35 pixels) for the streaming kernel, 259 of 128 (99 pixels): 518;
#   161 x 163 = 26243 pixels per image at 256 channels: 274 tiles of 96 (the last one 35 pixels), 548 in all.
LONG_WALKS = [(2, 128, 128, 181, 183), (2, 256, 256, 161, 163)]


@functools.lru_cache(maxsize=None)
def operands(n, cin, cout, h, w):
    g = torch.Generator(device=DEV).manual_seed(n * 1000 + h * 31 + w + cin + 7 * cout)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / (9 * cin) ** 0.5).to(torch.bfloat16)
    wt = wt.contiguous(memory_format=torch.channels_last)
    b = torch.randn(cout, device=DEV, generator=g).to(torch.bfloat16)
    return x, wt, b


def conv(x, wt, b, relu, stride=1, dilation=1):
    with torch.no_grad():
        return alo_hip.conv3x3(x, wt, b, relu=relu, stride=stride, dilation=dilation)


def bits(t):
    return t.contiguous(memory_format=torch.channels_last).view(torch.int16)


@pytest.fixture(autouse=True)
def no_knob(monkeypatch):
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)


@pytest.fixture
def one_pass(monkeypatch):
    """Launches of the route's shapes go without a workspace; -> the list of (Cin, Cout, pixels per image) so launched."""
    real, routed = alo_hip._launch, []

    def launch(symbol, device, tag, nbytes, flops, *args, **kw):
        # alo_conv3x3_nhwc(x, w_packed, bias, y, workspace, N, H, W, Cin, Cout, stride, relu, dtype)
        if symbol == "alo_conv3x3_nhwc" and args[10] == 1 and args[9] >= 128 and args[12] == alo_hip.ALO_BF16:
            args = args[:4] + (None,) + args[5:]
            routed.append((args[8], args[9], args[6] * args[7]))
        return real(symbol, device, tag, nbytes, flops, *args, **kw)

    monkeypatch.setattr(alo_hip, "_launch", launch)
    return routed


def both(x, wt, b, relu, monkeypatch, **kw):
    """(the default route, the streaming kernel) on the same operands"""
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    got = conv(x, wt, b, relu, **kw)
    monkeypatch.setenv("ALO_CONV3X3_PIPE", "off")
    stream = conv(x, wt, b, relu, **kw)
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    return got, stream


def check_fp32(x, wt, b, relu, got):
    """The bar of test_fused_gpu.py::test_conv3x3_matches_fp32_convolution."""
    with torch.no_grad():
        ref = F.conv2d(x.float(), wt.float(), None if b is None else b.float(), 1, 1)
        if relu:
            ref = F.relu(ref)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert (got.float() - ref).abs().max().item() <= 2.0 ** -8 * max(1.0, ref.abs().max().item())
    check_conv3x3(x, wt, b, relu, 1, got)


@pytest.mark.parametrize("with_bias,relu", FLAGS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_same_bits_as_the_streaming_kernel_and_the_fp32_bar(cin, cout, with_bias, relu, monkeypatch, one_pass):
    for n in BATCHES:
        for h, w in MAPS:
            x, wt, b = operands(n, cin, cout, h, w)
            b = b if with_bias else None
            got, stream = both(x, wt, b, relu, monkeypatch)
            assert got.shape == stream.shape == (n, cout, h, w), (n, h, w)
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


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("cin,cout", [(128, 128), (256, 256), (512, 512)])
@pytest.mark.parametrize("py,px", [(5, 22), (0, 0), (8, 11)])   # right edge, corner, interior
def test_nan_pixel_reaches_exactly_its_window(py, px, cin, cout, relu, monkeypatch, one_pass):
    """Out-of-image taps are zeroed by selection and a flattened halo run wraps into the neighbouring rows: a NaN pixel reaches the
    outputs whose 3x3 window contains it, ReLU keeps it there, and no other output changes."""
    x, wt, b = operands(1, cin, cout, 17, 23)
    clean = conv(x, wt, b, relu)
    xn = x.clone(memory_format=torch.preserve_format)
    xn[0, :, py, px] = float("nan")
    got, stream = both(xn, wt, b, relu, monkeypatch)
    inside = torch.zeros(17, 23, dtype=torch.bool, device=DEV)
    inside[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    assert torch.isnan(got[0][:, inside]).all()
    assert torch.equal(bits(got)[0][:, ~inside], bits(clean)[0][:, ~inside])
    assert torch.equal(bits(got), bits(stream))
    assert one_pass == [(cin, cout, 17 * 23)] * 3


@pytest.mark.parametrize("cin,cout", [(128, 128), (256, 256), (512, 512)])
def test_infinite_weights_stay_in_their_column(cin, cout, monkeypatch, one_pass):
    x, wt, b = operands(3, cin, cout, 5, 13)
    clean = conv(x, wt, b, False)
    wi = wt.clone(memory_format=torch.preserve_format)
    wi[5, 3, 1, 1] = float("inf")
    wi[cout - 2, cin - 1, 0, 2] = float("-inf")
    got, stream = both(x, wi, b, False, monkeypatch)
    assert torch.equal(bits(got), bits(stream))
    touched = torch.zeros(cout, dtype=torch.bool, device=DEV)
    touched[[5, cout - 2]] = True
    assert not torch.isfinite(got[:, touched].float()).any()     # every window holds the tap or its zero padding (0 x Inf)
    assert torch.equal(bits(got)[:, ~touched], bits(clean)[:, ~touched])
    assert one_pass == [(cin, cout, 5 * 13)] * 3


@pytest.mark.parametrize("shape", [(3, 128, 128, 5, 13), (1, 192, 192, 10, 20), (3, 256, 256, 7, 9), (1, 512, 512, 10, 20)], ids=str)
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


@pytest.mark.parametrize("case", [(2, 64, 64, 17, 23, 1, 1),       # conv3x3_c64_kernel
                                  (2, 128, 128, 17, 23, 2, 1),     # stride 2
                                  (2, 128, 64, 17, 23, 1, 1),      # the K-split form
                                  (2, 512, 512, 9, 13, 1, 2),      # dilated
                                  (1, 512, 512, 13, 21, 1, 1)],    # 5 tiles x 4 column blocks: split-K over four channel ranges
                         ids=["c64", "stride2", "cout64", "dilated", "zsplit"])
def test_other_calls_do_not_see_the_knob(case, monkeypatch):
    n, cin, cout, h, w, stride, dilation = case
    if case[-2:] == (1, 1) and cout >= 128:
        assert alo_hip.lib().alo_conv3x3_workspace_bytes(n, h, w, cin, cout, 1) > 0
    x, wt, b = operands(n, cin, cout, h, w)
    default, off = both(x, wt, b, True, monkeypatch, stride=stride, dilation=dilation)
    assert torch.equal(bits(default), bits(off))
    if dilation == 1:
        check_conv3x3(x, wt, b, True, stride, default)


# ---- the bf16 backbone ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backbone():
    from alonet.detr.backbone import ResNetBody

    torch.manual_seed(0)
    body = ResNetBody("resnet50", return_layers={"layer1": "0", "layer2": "1", "layer3": "2", "layer4": "3"}).to(DEV).eval()
    for m in body.modules():  # non-trivial frozen statistics
        if hasattr(m, "running_var"):
            m.running_var.uniform_(0.5, 2.0); m.running_mean.normal_(0, 0.2); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    body = body.to(torch.bfloat16)
    x = torch.randn(2, 3, 72, 104, device=DEV).to(torch.bfloat16)
    return body, x


# the ten stride-1 convolutions of layer2 .. layer4 on a 72 x 104 input: (Cin, Cout, pixels per image), in order
BODY_ROUTED = [(128, 128, 9 * 13)] * 3 + [(256, 256, 5 * 7)] * 5 + [(512, 512, 3 * 4)] * 2


@pytest.fixture(params=["as the wrapper launches", "one pass"])
def body_launches(request):
    """The backbone as alo_hip.conv3x3 launches it (layer3 and layer4 split K at this size and stay on the streaming kernel) and with
    every routed-shape launch in one pass (all ten reach the gate); -> the record of the latter, else None."""
    return request.getfixturevalue("one_pass") if request.param == "one pass" else None


def test_resnet_body_eager(monkeypatch, body_launches):
    body, x = backbone()
    with alo_hip.LaunchTimer() as t, torch.no_grad():
        on = {k: v.clone() for k, v in body(x).items()}
    assert {"conv3x3/C=128/s=1", "conv3x3/C=256/s=1", "conv3x3/C=512/s=1"} <= set(t.summary())
    if body_launches is not None:
        assert body_launches == BODY_ROUTED
    monkeypatch.setenv("ALO_CONV3X3_PIPE", "off")
    with torch.no_grad():
        off = body(x)
    assert on.keys() == off.keys() and len(on) == 4
    for k in on:
        assert bool(torch.isfinite(on[k].float()).all()) and torch.equal(bits(on[k]), bits(off[k])), k


def _captured(body, x, knob, monkeypatch):
    """The stages of two replays of one captured forward: on a zeroed input, then on x."""
    if knob:
        monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    else:
        monkeypatch.setenv("ALO_CONV3X3_PIPE", "off")
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
    zero_on, real_on = _captured(body, x, True, monkeypatch)
    if body_launches is not None:
        assert body_launches == BODY_ROUTED * 2     # the warm-up forward and the captured one
    zero_off, real_off = _captured(body, x, False, monkeypatch)
    with torch.no_grad():
        eager_off = body(x)   # the knob is still "off"
    for k in real_on:
        assert torch.equal(bits(real_on[k]), bits(real_off[k])), k
        assert torch.equal(bits(real_on[k]), bits(eager_off[k])), k
        assert torch.equal(bits(zero_on[k]), bits(zero_off[k])), k
        assert not torch.equal(bits(zero_on[k]), bits(real_on[k])), k
