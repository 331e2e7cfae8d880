"""What the bottleneck chain (alo_conv1x1_nhwc with a chain buffer, csrc/conv1x1_chain.hip) promises without a GPU: the argument checks of
the entry point, the gate on the CPU, and the hand-off loop of ResNetBody against the stages run as plain ``nn.Sequential``."""
import ctypes

import torch

import alo_hip

CHAIN, DOWN = alo_hip.CONV1X1_CHAIN, alo_hip.CONV1X1_CHAIN_DOWN


def test_flag_values_are_the_header_s():
    from helpers import header_text

    text = header_text("alo_hotpath.h")
    assert f"#define ALO_CONV1X1_CHAIN {CHAIN}\n" in text and f"#define ALO_CONV1X1_CHAIN_DOWN {DOWN}\n" in text
    assert CHAIN & DOWN == 0 and (CHAIN | DOWN) & (64 | 128) == 0 and (CHAIN | DOWN) & 1 == 0


def test_argument_errors_are_reported_before_any_launch():
    lib = alo_hip.lib()
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731  (never dereferenced: validation fails first)
    x, w, r, y = p(1 << 20), p(2 << 20), p(3 << 20), p(8 << 20)
    bf16, f32 = alo_hip.ALO_BF16, alo_hip.ALO_F32

    def call(x=x, w=w, flags=CHAIN | 64, bias=None, res=r, y=y, n=1, h=4, w_=8, cin=64, cout=256, stride=1, relu=1, dtype=bf16):
        rc = lib.alo_conv1x1_nhwc(x, w, flags, bias, res, y, n, h, w_, cin, cout, stride, relu, dtype, None)
        return rc, lib.alo_last_error()

    for kwargs in (dict(cin=128), dict(cout=512), dict(stride=2), dict(relu=0), dict(dtype=f32), dict(flags=CHAIN | 32),
                   dict(flags=CHAIN | 192), dict(flags=CHAIN | 1)):
        rc, msg = call(**kwargs)
        assert rc == 2 and b"chain buffer" in msg, (kwargs, msg)
    rc, msg = call(res=None)
    assert rc == 1 and b"residual" in msg
    rc, msg = call(bias=p(4 << 20))
    assert rc == 1 and b"bias must be NULL" in msg
    rc, msg = call(y=p((8 << 20) + 8))
    assert rc == 1 and b"16-byte aligned" in msg
    rows = 32
    # y-then-z is rows * (256 + 64) * 2 bytes from y: it may end where an input begins, not one row later
    rc, msg = call(x=p((8 << 20) + rows * 640 - 128))
    assert rc == 1 and b"overlaps" in msg
    rc, msg = call(y=p((3 << 20) + rows * 512 - 16 * 4), flags=CHAIN)            # inside the (rows, 256) identity
    assert rc == 1 and b"overlaps" in msg


def test_the_gate_refuses_cpu_tensors_and_the_bottleneck_keeps_its_path():
    from alonet.detr.backbone import Bottleneck, FrozenBatchNorm2d

    mid = torch.zeros(1, 64, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    idn = torch.zeros(1, 256, 2, 2, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w3, b3 = torch.zeros(256, 64, dtype=torch.bfloat16), torch.zeros(256, dtype=torch.bfloat16)
    with torch.no_grad():
        assert not alo_hip.conv1x1_chain_supported(mid, (w3, b3), identity=idn)
    ds = torch.nn.Sequential(torch.nn.Conv2d(64, 256, 1, bias=False), FrozenBatchNorm2d(256))
    first, second = Bottleneck(64, 64, downsample=ds).eval(), Bottleneck(256, 64).eval()
    x = torch.randn(1, 64, 6, 5)
    with torch.no_grad():
        assert first._chain(x, first.conv1(x), second) is None
        want = second(first(x))
        y, head = first(x, nxt=second)
        assert head is None and torch.equal(second(y, head=head), want)
        # a hand-off, when one is made, stands for relu(bn1(conv1(y))): the block uses it in place of its own
        made = torch.relu(second.bn1(second.conv1(y)))
        assert torch.allclose(second(y, head=made), want, rtol=1e-5, atol=1e-6)


def test_resnet_body_walks_its_stages_block_by_block():
    """The explicit loop of ResNetBody.forward equals the stages run as nn.Sequential, and returns the requested stages at their ends."""
    from alonet.detr.backbone import ResNetBody, conv_bn

    torch.manual_seed(0)
    body = ResNetBody("resnet50", return_layers={"layer1": "a", "layer3": "b", "layer4": "c"}).eval()
    x = torch.randn(1, 3, 40, 48)
    with torch.no_grad():
        got = body(x)
        t = body.maxpool(conv_bn(x.contiguous(memory_format=torch.channels_last), body.conv1, body.bn1, relu=True))
        want = {}
        for name in ("layer1", "layer2", "layer3", "layer4"):
            t = getattr(body, name)(t)
            if name in body.return_layers:
                want[body.return_layers[name]] = t
    assert list(got) == ["a", "b", "c"]
    for k in want:
        assert got[k].shape == want[k].shape and torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-6), k
