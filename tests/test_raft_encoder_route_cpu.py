"""``ALO_RAFT_ENCODER=split`` (alonet/raft/extractor.py) as far as it can be checked without a GPU: an encoder on CPU tensors, in
training mode or under autograd keeps the stock ops with the knob set, and the padded / folded tensors the route derives reproduce
the module's own layers in fp64 — the padding channels exactly 0."""
import copy

import pytest
import torch
import torch.nn.functional as F

import alo_hip
from alonet.raft import extractor
from alonet.raft.extractor import BasicEncoder, SmallEncoder, _route_weights

KNOB = "ALO_RAFT_ENCODER"
WRAPPERS = ("instancenorm_nhwc_f32", "conv3x3_f32", "conv1x1_strided_f32", "linear_f32")


def _refuse(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a HIP wrapper was called")

    for name in WRAPPERS:
        monkeypatch.setattr(alo_hip, name, refuse)


def _encoder(norm_fn, seed=3, cls=BasicEncoder):
    torch.manual_seed(seed)
    enc = cls(output_dim=128, norm_fn=norm_fn).eval()
    with torch.no_grad():
        for m in enc.modules():      # statistics and an affine that are not the identity
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.5)
                m.running_var.uniform_(0.5, 2.0)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.3)
            if isinstance(m, torch.nn.Conv2d):
                m.bias.normal_(0, 0.2)
    return enc


@pytest.mark.parametrize("norm_fn", ["instance", "batch"])
def test_cpu_encoder_takes_the_stock_ops_with_the_knob_set(monkeypatch, norm_fn):
    enc = _encoder(norm_fn)
    x = torch.randn(2, 3, 44, 76)
    monkeypatch.delenv(KNOB, raising=False)
    with torch.no_grad():
        want = enc(x)
        want_pair = enc([x[:1], x[1:]])
    monkeypatch.setenv(KNOB, "split")
    assert extractor._encoder_split_route()
    _refuse(monkeypatch)
    with torch.no_grad():
        assert not enc._split_serves(x)
        got, got_pair = enc(x), enc([x[:1], x[1:]])
    assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(got_pair, want_pair))
    assert enc(x).requires_grad                                                  # grad mode: the stock ops as well


def test_the_knob_is_read_per_call_and_only_split_sets_it(monkeypatch):
    for value, on in ((None, False), ("split", True), ("1", False), ("", False)):
        monkeypatch.delenv(KNOB, raising=False)
        if value is not None:
            monkeypatch.setenv(KNOB, value)
        assert extractor._encoder_split_route() is on


class _OnGpu:
    """What ``_split_serves`` asks of its input, answered as a CUDA fp32 batch would: the gate's other conditions without a GPU."""

    def __init__(self, dtype=torch.float32, requires_grad=False, dim=4):
        self.is_cuda, self.dtype, self.requires_grad, self._dim = True, dtype, requires_grad, dim

    def dim(self):
        return self._dim


def test_gate_of_the_route():
    with torch.no_grad():
        assert _encoder("instance")._split_serves(_OnGpu()) and _encoder("batch")._split_serves(_OnGpu())
        assert not _encoder("instance")._split_serves(_OnGpu(torch.float16)) and not _encoder("instance")._split_serves(_OnGpu(dim=3))
        assert not _encoder("batch").train()._split_serves(_OnGpu())                       # BatchNorm in training mode
        frozen = _encoder("batch").train()
        for m in frozen.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()                                                                       # RAFT.freeze_bn
        assert frozen._split_serves(_OnGpu())
        assert not _encoder("group")._split_serves(_OnGpu()) and not _encoder("none")._split_serves(_OnGpu())
        assert not _encoder("instance", cls=SmallEncoder)._split_serves(_OnGpu())          # bottlenecks of 8 to 24 channels: stock
        torch.manual_seed(0)
        dropping = BasicEncoder(128, "instance", dropout=0.5)
        assert not dropping.train()._split_serves(_OnGpu()) and dropping.eval()._split_serves(_OnGpu())
        assert not BasicEncoder(100, "instance").eval()._split_serves(_OnGpu())            # conv2's width is not a multiple of 64
        affine = _encoder("instance")
        affine.layer1[0].norm1 = torch.nn.InstanceNorm2d(64, affine=True)
        assert not affine._split_serves(_OnGpu())
    assert not _encoder("instance")._split_serves(_OnGpu())                                # grad mode on
    enc = _encoder("instance")
    for p in enc.parameters():
        p.requires_grad_(False)
    assert not enc._split_serves(_OnGpu())                                                 # ... even with every parameter frozen


def _pad_channels(t, to):
    return F.pad(t, (0, 0, 0, 0, 0, to - t.shape[1]))


@pytest.mark.parametrize("norm_fn", ["instance", "batch"])
def test_derived_weights_reproduce_every_layer_in_fp64(norm_fn):
    """F.conv2d with the derived tensors (fp64 copies of them) against the module's own convolution (+ eval BatchNorm) in fp64, layer
    by layer on zero-padded inputs: the real channels agree to fp32 rounding of the folded weights, the padding channels are exactly 0."""
    enc = _encoder(norm_fn)
    ref = copy.deepcopy(enc).double()
    g = torch.Generator().manual_seed(1)
    layers = [("conv1", enc.conv1, enc.norm1, ref.conv1, ref.norm1), ("conv2", enc.conv2, None, ref.conv2, None)]
    for li in (1, 2, 3):
        for bi in (0, 1):
            blk, rblk = getattr(enc, f"layer{li}")[bi], getattr(ref, f"layer{li}")[bi]
            layers += [(f"layer{li}.{bi}.conv1", blk.conv1, blk.norm1, rblk.conv1, rblk.norm1),
                       (f"layer{li}.{bi}.conv2", blk.conv2, blk.norm2, rblk.conv2, rblk.norm2)]
            if blk.downsample is not None:
                layers.append((f"layer{li}.{bi}.downsample", blk.downsample[0], blk.downsample[1], rblk.downsample[0], rblk.downsample[1]))
    assert len(layers) == 16
    for name, conv, norm, rconv, rnorm in layers:
        bn = norm if norm_fn == "batch" else None
        w, b = _route_weights(conv, bn)
        cout, cin = conv.weight.shape[:2]
        pin, pout = (cin if cin < 64 else extractor._pad64(cin)), extractor._pad64(cout)
        assert w.dtype == torch.float32 and b.dtype == torch.float32 and b.shape == (pout,) and w.shape[:2] == (pout, pin), name
        assert w.dim() == (2 if conv.kernel_size == (1, 1) else 4), name
        assert (w[cout:] == 0).all() and (b[cout:] == 0).all() and (w[:, cin:] == 0).all(), name
        x = torch.randn(2, cin, 9, 11, generator=g, dtype=torch.float64)
        want = rconv(x)
        if bn is not None:
            want = rnorm(want)
        w4 = w.double().view(pout, pin, *conv.kernel_size)
        got = F.conv2d(_pad_channels(x, pin), w4, b.double(), conv.stride, conv.padding)
        assert (got[:, cout:] == 0).all(), name                                            # the padding channels: exactly 0
        err = (got[:, :cout] - want).abs().max().item()
        bar = 2.0 ** -22 * want.abs().max().item() * (1 if bn is None else 4)              # fp32 roundings of the fold: scale, w * scale, the bias
        assert err <= bar, (name, err, bar)
        if bn is None:
            assert torch.equal(w[:cout, :cin].reshape(conv.weight.shape), conv.weight) and torch.equal(b[:cout], conv.bias), name
        # zero padding survives InstanceNorm, ReLU and the add: (0 - 0) * rsqrt(0 + eps)
        assert (torch.relu(F.instance_norm(got.float()))[:, cout:] == 0).all()
    assert _route_weights(enc.layer2[0].conv1, enc.layer2[0].norm1 if norm_fn == "batch" else None)[0] is \
        _route_weights(enc.layer2[0].conv1, enc.layer2[0].norm1 if norm_fn == "batch" else None)[0]         # derived once


def test_invalidate_caches_drops_the_derived_weights():
    enc = _encoder("batch")
    conv, bn = enc.layer2[0].conv1, enc.layer2[0].norm1
    w0, _ = _route_weights(conv, bn)
    w1, _ = _route_weights(conv)
    with torch.no_grad():
        conv.weight.data.mul_(2.0)                                                         # through .data: no version bump
    assert _route_weights(conv, bn)[0] is w0 and _route_weights(conv)[0] is w1             # stale: what load_weights invalidates for
    alo_hip.invalidate_caches(enc)
    assert torch.equal(_route_weights(conv)[0][:96], conv.weight) and not torch.equal(_route_weights(conv, bn)[0], w0)
    folded = _route_weights(conv, bn)[0]
    with torch.no_grad():
        bn.running_var.mul_(3.0)                                                           # a versioned update is seen without help
    assert not torch.equal(_route_weights(conv, bn)[0], folded)
