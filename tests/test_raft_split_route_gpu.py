"""``ALO_RAFT_CONV3X3=split``: the opt-in route of RAFT's update block on which the 3x3 convolutions that alo_hip.conv3x3_f32 runs
faster than MIOpen take that kernel (alonet/raft/update.py: four of the six).  The default route is held to launching and computing what it did before the route existed."""
import copy

import numpy as np
import pytest
import torch

import alo_hip
import aloscene
from alonet.raft import RAFT
from alonet.raft.corr import TorchCorrBlock
from alonet.raft.update import BasicUpdateBlock
from helpers import formula_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "ALO_RAFT_CONV3X3"
t = torch.from_numpy


def _block_and_inputs():
    """BasicUpdateBlock(4, 4) at (1, ., 12, 16): the shape of test_raft_update_block_in_fp16_stays_off_the_fp32_kernels."""
    torch.manual_seed(4)
    blk = BasicUpdateBlock(corr_levels=4, corr_radius=4).eval()
    net, inp = torch.randn(1, 128, 12, 16).tanh(), torch.randn(1, 128, 12, 16).relu()
    corr, flow = torch.randn(1, 324, 12, 16), torch.randn(1, 2, 12, 16)
    return blk, (net, inp, corr, flow)


def _run_block(blk, args):
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = blk(*[a.to(DEV) for a in args])
    return [o.cpu() for o in out], timer.summary()


def test_update_block_on_the_split_route(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)   # MIOpen's default solvers do not all repeat themselves bit for bit
    blk, args = _block_and_inputs()
    with torch.no_grad():
        ref = copy.deepcopy(blk).double()(*[a.double() for a in args])          # the fp64 copy of the block (CPU)
    blk = blk.to(DEV)
    monkeypatch.delenv(KNOB, raising=False)
    _run_block(blk, args)                                    # MIOpen picks its solvers on a shape's first call, and that call runs others
    stock, tags = _run_block(blk, args)
    assert not any(tag.startswith("conv3x3_f32") for tag in tags), tags
    again, tags_again = _run_block(blk, args)
    assert all(torch.equal(a, b) for a, b in zip(stock, again)) and set(tags) == set(tags_again)
    monkeypatch.setenv(KNOB, "split")
    _run_block(blk, args)
    split, tags_split = _run_block(blk, args)
    calls = {tag: v["calls"] for tag, v in tags_split.items() if tag.startswith("conv3x3_f32")}
    assert calls == {"conv3x3_f32/C=256/s=1": 2, "conv3x3_f32/C=128/s=1": 2}, tags_split   # convc2, conv | flow_head.conv1, mask.0
    for name, got, base, want in zip(("net", "up_mask", "delta_flow"), split, stock, ref):
        assert got.shape == base.shape and got.is_contiguous()
        e_stock, e_split = (base.double() - want).abs().max().item(), (got.double() - want).abs().max().item()
        print(f"{name}: stock route {e_stock:.3g}, split route {e_split:.3g} against fp64 (max |ref| {want.abs().max().item():.3g})")
        assert e_split <= 4 * e_stock + 3e-7 * want.abs().max().item(), (name, e_split, e_stock)   # test_split_numerics.py's factor and floor
    monkeypatch.delenv(KNOB)
    back, tags_back = _run_block(blk, args)
    assert all(torch.equal(a, b) for a, b in zip(stock, back)) and set(tags_back) == set(tags)


def test_split_weights_go_with_invalidate_caches(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    blk, args = _block_and_inputs()
    blk = blk.to(DEV)
    monkeypatch.setenv(KNOB, "split")
    _run_block(blk, args)
    before, _ = _run_block(blk, args)
    with torch.no_grad():
        for conv in (blk.encoder.conv, blk.flow_head.conv1):  # a padded and a plain layer of the route
            conv.weight.data.mul_(2.0)                       # through .data: no version bump
    stale, _ = _run_block(blk, args)
    assert all(torch.equal(a, b) for a, b in zip(stale, before))   # what the cache is for (and why load_weights invalidates)
    alo_hip.invalidate_caches(blk)
    fresh, _ = _run_block(blk, args)
    want, _ = _run_block(copy.deepcopy(blk), args)           # a copy derives its own split weights
    assert all(torch.equal(a, b) for a, b in zip(fresh, want)) and not torch.equal(fresh[0], before[0]) and not torch.equal(fresh[2], before[2])


def _g7(golden, model):
    g = golden("g7_raft.npz")
    mk = lambda a, dev, dt: aloscene.Frame(t(a).to(dt), normalization="minmax_sym", names=("B", "C", "H", "W")).to(dev)  # noqa: E731
    model.load_state_dict(formula_state_dict(model.state_dict()))
    return g, mk


def test_raft_on_the_split_route_matches_reference(golden, monkeypatch):
    """G7 at the bars of test_raft_on_hip_matches_reference."""
    model = RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    monkeypatch.setenv(KNOB, "split")
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        outs = model(mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32), iters=4)
    assert sum(v["calls"] for tag, v in timer.summary().items() if tag.startswith("conv3x3_f32")) == 4 * 4
    flows = np.stack([o["flow"].cpu().numpy() for o in outs])
    assert np.isfinite(flows).all()
    assert np.abs(flows - g["flow"]).max() <= 1e-3
    assert np.abs(outs[-1]["up_flow"].cpu().numpy() - g["up_flow_last"]).max() <= 8e-3
    assert np.abs(outs[-1]["hidden_state"].cpu().numpy() - g["hidden_last"]).max() <= 1e-3


def test_raft_32_iterations_on_the_split_route_against_fp64(golden, monkeypatch):
    """G7's frames, 32 iterations, against an fp64 copy of the model (TorchCorrBlock, .double(); CPU): the final 1/8-resolution flow
    of the split route is within 4 x the default route's own error + 1e-4 px (a tenth of the north-star bar).
    Measured on MI355X in two processes: default route 6.48e-5 / 4.96e-5 px, split route 7.63e-5 / 7.25e-5 px (docs/experiments.md,
    conv3x3_f32).  RAFT.forward keeps the correlation and the coordinates in fp32 whatever the model's dtype."""
    ref_model = RAFT(corr_block=TorchCorrBlock).eval()
    g, mk = _g7(golden, ref_model)
    with torch.no_grad():
        want = ref_model.double()(mk(g["img1"], "cpu", torch.float64), mk(g["img2"], "cpu", torch.float64), iters=32, only_last=True)[-1]["flow"].double()
    model = RAFT().eval()
    _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32)
    err = {}
    for route in ("default", "split"):
        if route == "split":
            monkeypatch.setenv(KNOB, "split")
        else:
            monkeypatch.delenv(KNOB, raising=False)
        with torch.no_grad():
            flow = model(f1, f2, iters=32, only_last=True)[-1]["flow"].cpu().double()
        err[route] = (flow - want).abs().max().item()
    print(f"32 iterations, final 1/8 flow against fp64: default route {err['default']:.3g} px, split route {err['split']:.3g} px")
    assert err["split"] <= 4 * err["default"] + 1e-4, err


def test_graphed_raft_on_the_split_route_replays_eager_bit_for_bit(golden, monkeypatch):
    """MIOpen's default solver choice for RAFT's other convolutions does not repeat itself: on MI355X two eager forwards of this very
    model differ by 3.8e-6 px on the default route and on the split route alike, and a replay differs from either by as much.  With
    MIOpen held to deterministic solvers (``torch.backends.cudnn.deterministic``) eager repeats itself on both routes, and the
    captured split route — magnitude pre-pass, its memset and the convolutions included — replays it bit for bit."""
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
