"""What the layer2 bottleneck chain (alo_conv1x1_nhwc with a chain buffer at Cin = 128, Cout = 512; csrc/conv1x1_chain_l2.hip) promises
without a GPU: the entry point's refusals for the new values, the routing table behind the three values of ``ALO_BOTTLENECK_CHAIN``, and
the hand-off loop of ResNetBody under each of them."""
import ctypes

import pytest
import torch

import alo_hip

CHAIN, DOWN = alo_hip.CONV1X1_CHAIN, alo_hip.CONV1X1_CHAIN_DOWN


def test_argument_errors_are_reported_before_any_launch():
    lib = alo_hip.lib()
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731  (never dereferenced: validation fails first)
    x, w, r, y = p(1 << 20), p(2 << 20), p(3 << 20), p(8 << 20)
    bf16, f32 = alo_hip.ALO_BF16, alo_hip.ALO_F32

    def call(x=x, w=w, flags=CHAIN | 128, bias=None, res=r, y=y, n=1, h=4, w_=8, cin=128, cout=512, stride=1, relu=1, dtype=bf16):
        rc = lib.alo_conv1x1_nhwc(x, w, flags, bias, res, y, n, h, w_, cin, cout, stride, relu, dtype, None)
        return rc, lib.alo_last_error()

    # wrong Cin or Cout (also: one family's Cin with the other's Cout), a next width that is not 0 or 128, stride 2 without _DOWN, a
    # stride the loader does not address, no ReLU, fp32
    for kwargs in (dict(cin=256), dict(cout=256), dict(cout=1024), dict(cin=64), dict(flags=CHAIN | 64), dict(flags=CHAIN | DOWN | 64),
                   dict(flags=CHAIN | 32), dict(flags=CHAIN | 256), dict(flags=CHAIN | 1), dict(stride=2), dict(stride=2, flags=CHAIN),
                   dict(stride=3, flags=CHAIN | DOWN), dict(stride=4, flags=CHAIN | DOWN | 128), dict(relu=0), dict(dtype=f32)):
        rc, msg = call(**kwargs)
        assert rc == 2 and b"chain buffer" in msg, (kwargs, msg)
    rc, msg = call(res=None)
    assert rc == 1 and b"residual" in msg
    rc, msg = call(bias=p(4 << 20))
    assert rc == 1 and b"bias must be NULL" in msg
    for kwargs in (dict(y=p((8 << 20) + 8)), dict(x=p((1 << 20) + 2)), dict(res=p((3 << 20) + 4)), dict(w=p((2 << 20) + 8))):
        rc, msg = call(**kwargs)
        assert rc == 1 and b"16-byte aligned" in msg, kwargs
    rows = 32
    # y-then-z is rows * (512 + 128) * 2 bytes from y: it may end where an input begins, not one row later
    rc, msg = call(x=p((8 << 20) + rows * 1280 - 256))
    assert rc == 1 and b"overlaps" in msg
    rc, msg = call(y=p((3 << 20) + rows * 1024 - 16 * 4), flags=CHAIN)            # inside the (rows, 512) identity
    assert rc == 1 and b"overlaps" in msg
    # _DOWN at stride 2: residual is x0's whole (1, 4, 8, 256) map, 16 KB, of which the launch makes 2 x 4 = 8 rows
    rc, msg = call(y=p((3 << 20) + 32 * 512 - 16), flags=CHAIN | DOWN, stride=2)
    assert rc == 1 and b"overlaps" in msg


def test_the_three_knob_values_route_as_documented(monkeypatch):
    routed = alo_hip.bottleneck_chain_routed
    monkeypatch.delenv("ALO_BOTTLENECK_CHAIN", raising=False)
    assert routed(64, True, 64) and routed(64, False, 64) and routed(64, True, 0)
    for form in [(True, 128), (False, 128), (True, 0), (False, 0)]:
        assert routed(128, *form) == (form in alo_hip.CHAIN_LAYER2_ROUTED)
    assert not routed(256, False, 256) and not routed(512, True, 512)
    monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", "layer1")
    assert alo_hip.bottleneck_chain_enabled() and routed(64, True, 64) and routed(64, False, 64)
    assert not any(routed(128, d, n2) for d in (True, False) for n2 in (0, 128))
    for off in ("off", "0", "OFF"):
        monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", off)
        assert not alo_hip.bottleneck_chain_enabled() and not routed(64, True, 64) and not routed(128, True, 128)


def test_the_gate_refuses_cpu_tensors_and_the_bottleneck_keeps_its_path():
    from alonet.detr.backbone import Bottleneck, FrozenBatchNorm2d

    mid = torch.zeros(1, 128, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    idn = torch.zeros(1, 512, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w3, b3 = torch.zeros(512, 128, dtype=torch.bfloat16), torch.zeros(512, dtype=torch.bfloat16)
    with torch.no_grad():
        assert not alo_hip.conv1x1_chain_supported(mid, (w3, b3), identity=idn)
    ds = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, stride=2, bias=False), FrozenBatchNorm2d(512))
    first, second = Bottleneck(256, 128, stride=2, downsample=ds).eval(), Bottleneck(512, 128).eval()
    x = torch.randn(1, 256, 6, 5)
    with torch.no_grad():
        assert first._chain(x, first.conv2(first.conv1(x)), second) is None
        want = second(first(x))
        y, head = first(x, nxt=second)
        assert head is None and torch.equal(second(y, head=head), want)


@pytest.mark.parametrize("value", [None, "layer1", "off"])
def test_resnet_body_walks_its_stages_block_by_block(value, monkeypatch):
    """The explicit loop of ResNetBody.forward equals the stages run as nn.Sequential under every value of the knob."""
    from alonet.detr.backbone import ResNetBody, conv_bn

    if value is None:
        monkeypatch.delenv("ALO_BOTTLENECK_CHAIN", raising=False)
    else:
        monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", value)
    torch.manual_seed(0)
    body = ResNetBody("resnet50", return_layers={"layer2": "a", "layer4": "b"}).eval()
    x = torch.randn(1, 3, 40, 48)
    with torch.no_grad():
        got = body(x)
        t = body.maxpool(conv_bn(x.contiguous(memory_format=torch.channels_last), body.conv1, body.bn1, relu=True))
        want = {}
        for name in ("layer1", "layer2", "layer3", "layer4"):
            t = getattr(body, name)(t)
            if name in body.return_layers:
                want[body.return_layers[name]] = t
    assert list(got) == ["a", "b"]
    for k in want:
        assert got[k].shape == want[k].shape and torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-6), k
