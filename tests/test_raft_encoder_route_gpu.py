"""``ALO_RAFT_ENCODER=split``: the opt-in route of RAFT's BasicEncoder through the library (alonet/raft/extractor.py) — channels-last,
3x3 convolutions on alo_hip.conv3x3_f32 and 1x1 ones on alo_hip.conv1x1_strided_f32 where they beat MIOpen, InstanceNorm on
alo_hip.instancenorm_nhwc_f32, eval BatchNorm folded, the 96-channel stage padded to 128.  The default route is held to launching and
computing what it did before the knob was ever set.  Mirrors test_raft_split_route_gpu.py."""
import copy

import numpy as np
import pytest
import torch

import alo_hip
import aloscene
from alonet.raft import RAFT
from alonet.raft.corr import TorchCorrBlock
from alonet.raft.extractor import BasicEncoder
from helpers import formula_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "ALO_RAFT_ENCODER"
ALL_KNOBS = ("ALO_RAFT_ENCODER", "ALO_RAFT_CONV3X3", "ALO_RAFT_GRU")
ROUTE_TAGS = ("instancenorm_f32", "conv3x3_f32", "conv1x1_strided_f32", "linear_f32")
t = torch.from_numpy

# The route's launches on BasicEncoder(256): layer1's four 3x3; layer2.0.conv1 (stride 2) | layer2's other three and layer3's three
# stride-1 3x3 at 128 (padded) channels — layer3.0.conv1 (128 -> 128, stride 2) lost to MIOpen and stays there; the two downsamples
# and conv2; and, for "instance", the stem's norm + 2 per block + 1 per downsample.
CONV_CALLS = {"conv3x3_f32/C=64/s=1": 4, "conv3x3_f32/C=64/s=2": 1, "conv3x3_f32/C=128/s=1": 6,
              "conv1x1_strided_f32/K=64/N=128": 1, "conv1x1_strided_f32/K=128/N=128": 1, "conv1x1_strided_f32/K=128/N=256": 1}
NORM_CALLS = {"instancenorm_f32/C=64": 5, "instancenorm_f32/C=128": 10}


def _encoder(norm_fn, seed=3):
    torch.manual_seed(seed)
    enc = BasicEncoder(output_dim=256, norm_fn=norm_fn).eval()
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


def _input():
    return torch.randn(2, 3, 44, 76, generator=torch.Generator().manual_seed(8))   # maps of 22x38 -> 11x19 -> 6x10


def _run(enc, x):
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = enc(x.to(DEV))
    calls = {tag: v["calls"] for tag, v in timer.summary().items()}
    return out.cpu(), calls, out


def _route_calls(calls):
    return {tag: n for tag, n in calls.items() if tag.startswith(ROUTE_TAGS)}


@pytest.mark.parametrize("norm_fn", ["instance", "batch"])
def test_encoder_on_the_split_route(monkeypatch, norm_fn):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)   # MIOpen's default solvers do not all repeat themselves bit for bit
    enc, x = _encoder(norm_fn), _input()
    with torch.no_grad():
        ref = copy.deepcopy(enc).double()(x.double())                                     # the fp64 copy of the encoder (CPU)
    enc = enc.to(DEV)
    monkeypatch.delenv(KNOB, raising=False)
    _run(enc, x)                                              # MIOpen picks its solvers on a shape's first call, and that call runs others
    stock, calls, _ = _run(enc, x)
    assert not _route_calls(calls), calls
    again, calls_again, _ = _run(enc, x)
    assert torch.equal(stock, again) and calls_again == calls
    monkeypatch.setenv(KNOB, "split")
    _run(enc, x)
    split, calls_split, on_device = _run(enc, x)
    assert _route_calls(calls_split) == {**CONV_CALLS, **(NORM_CALLS if norm_fn == "instance" else {})}, calls_split
    assert sum(NORM_CALLS.values()) == 15
    assert on_device.shape == (2, 256, 6, 10) and on_device.is_contiguous() and split.shape == stock.shape
    top = ref.abs().max().item()
    e_stock, e_split = (stock.double() - ref).abs().max().item(), (split.double() - ref).abs().max().item()
    print(f"BasicEncoder({norm_fn}): stock route {e_stock:.3g}, split route {e_split:.3g} against fp64 (max |ref| {top:.3g})")
    assert e_split <= 4 * e_stock + 3e-7 * top, (e_split, e_stock)                         # test_split_numerics.py's factor and floor
    monkeypatch.delenv(KNOB)
    back, calls_back, _ = _run(enc, x)
    assert torch.equal(stock, back) and calls_back == calls                               # unset again: the launches and bits of before


def test_pair_input_is_the_stacked_batch(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    enc, x = _encoder("instance").to(DEV), _input().to(DEV)
    monkeypatch.setenv(KNOB, "split")
    with torch.no_grad():
        enc(x)
        whole = enc(x)
        a, b = enc([x[:1], x[1:]])
    assert torch.equal(a, whole[:1]) and torch.equal(b, whole[1:])


@pytest.mark.parametrize("norm_fn", ["instance", "batch"])
def test_derived_weights_go_with_invalidate_caches(monkeypatch, norm_fn):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    enc, x = _encoder(norm_fn).to(DEV), _input()
    monkeypatch.setenv(KNOB, "split")
    _run(enc, x)
    before, _, _ = _run(enc, x)
    with torch.no_grad():
        for conv in (enc.layer2[0].conv1, enc.layer1[0].conv1):   # a padded and a plain layer of the route
            conv.weight.data.mul_(2.0)                             # through .data: no version bump
    stale, _, _ = _run(enc, x)
    assert torch.equal(stale, before)                              # what the cache is for (and why load_weights invalidates)
    alo_hip.invalidate_caches(enc)
    fresh, _, _ = _run(enc, x)
    want, _, _ = _run(copy.deepcopy(enc), x)                       # a copy derives its own weights
    assert torch.equal(fresh, want) and not torch.equal(fresh, before)


def test_training_mode_and_autograd_keep_the_stock_ops(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a HIP wrapper was called")

    monkeypatch.setenv(KNOB, "split")
    for name in ("instancenorm_nhwc_f32", "conv3x3_f32", "conv1x1_strided_f32", "linear_f32"):
        monkeypatch.setattr(alo_hip, name, refuse)
    x = _input().to(DEV)
    cnet = _encoder("batch").to(DEV).train()                       # BatchNorm on batch statistics
    with torch.no_grad():
        assert torch.isfinite(cnet(x)).all()
    fnet = _encoder("instance").to(DEV)
    assert fnet(x).requires_grad                                   # grad mode with trainable parameters
    for p in fnet.parameters():
        p.requires_grad_(False)
    assert fnet(x.clone().requires_grad_()).requires_grad          # a tensor requiring grad


def _g7(golden, model):
    g = golden("g7_raft.npz")
    mk = lambda a, dev, dt: aloscene.Frame(t(a).to(dt), normalization="minmax_sym", names=("B", "C", "H", "W")).to(dev)  # noqa: E731
    model.load_state_dict(formula_state_dict(model.state_dict()))
    return g, mk


def test_raft_on_the_encoder_route_matches_reference(golden, monkeypatch):
    """G7 at the bars of test_raft_on_hip_matches_reference."""
    model = RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    monkeypatch.setenv(KNOB, "split")
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        outs = model(mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32), iters=4)
    calls = {tag: v["calls"] for tag, v in timer.summary().items()}
    assert sum(n for tag, n in calls.items() if tag.startswith("instancenorm_f32")) == 15             # fnet; cnet's BatchNorm is folded
    assert sum(n for tag, n in calls.items() if tag.startswith("conv3x3_f32")) == 2 * 11              # fnet and cnet; the update block is on its default
    flows = np.stack([o["flow"].cpu().numpy() for o in outs])
    assert np.isfinite(flows).all()
    errs = (np.abs(flows - g["flow"]).max(), np.abs(outs[-1]["up_flow"].cpu().numpy() - g["up_flow_last"]).max(),
            np.abs(outs[-1]["hidden_state"].cpu().numpy() - g["hidden_last"]).max())
    print(f"G7, 4 iterations, {KNOB}=split: flow {errs[0]:.3g}, up_flow_last {errs[1]:.3g}, hidden_last {errs[2]:.3g}")
    assert errs[0] <= 1e-3 and errs[1] <= 8e-3 and errs[2] <= 1e-3, errs


def test_raft_32_iterations_on_the_encoder_route_against_fp64(golden, monkeypatch):
    """G7's frames, 32 iterations, against the fp64 copy of the model: the final 1/8-resolution flow with this knob alone, and with
    all three RAFT knobs, is within 4 x the default route's own error + 1e-4 px.  conv3x3_f32 scales an image by one power of two and
    InstanceNorm then divides each channel by its own deviation: this test is the judge of that.  Measured on MI355X: default
    4.43e-5 px, this knob 6.01e-5 px, all three knobs 7.63e-5 px (docs/experiments.md, "RAFT encoders on the split family")."""
    ref_model = RAFT(corr_block=TorchCorrBlock).eval()
    g, mk = _g7(golden, ref_model)
    with torch.no_grad():   # once, for the three routes below
        want = ref_model.double()(mk(g["img1"], "cpu", torch.float64), mk(g["img2"], "cpu", torch.float64), iters=32, only_last=True)[-1]["flow"].double()
    model = RAFT().eval()
    _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32)
    err = {}
    for route, knobs in (("default", ()), ("encoder", (KNOB,)), ("all three", ALL_KNOBS)):
        for k in ALL_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k in knobs:
            monkeypatch.setenv(k, "split")
        with torch.no_grad():
            flow = model(f1, f2, iters=32, only_last=True)[-1]["flow"].cpu().double()
        err[route] = (flow - want).abs().max().item()
    print("32 iterations, final 1/8 flow against fp64: " + ", ".join(f"{k} {v:.3g} px" for k, v in err.items()))
    assert err["encoder"] <= 4 * err["default"] + 1e-4, err
    assert err["all three"] <= 4 * err["default"] + 1e-4, err


def test_graphed_raft_on_the_encoder_route_replays_eager_bit_for_bit(golden, monkeypatch):
    """As test_graphed_raft_on_the_split_route_replays_eager_bit_for_bit: MIOpen held to deterministic solvers, the captured route —
    the norm's three launches, the magnitude pre-passes and the convolutions included — replays eager bit for bit, from one graph."""
    from alonet.common import GraphedForward

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32)
    monkeypatch.setenv(KNOB, "split")
    graphed = GraphedForward(model)
    with torch.no_grad():
        model(f1, f2, iters=4, only_last=True)               # MIOpen picks its solvers on a shape's first call
        for a, b in ((f1, f2), (f2, f1)):
            want = model(a, b, iters=4, only_last=True)[-1]
            got = graphed(a, b, iters=4, only_last=True)[-1]
            for key in ("flow", "up_flow", "hidden_state"):
                print(f"graph replay against eager, {key}: max |difference| {(got[key] - want[key]).abs().max().item():.3g}")
            for key in ("flow", "up_flow", "hidden_state"):
                assert torch.equal(got[key], want[key]), key
    assert len(graphed._graphs) == 1
