"""``ALO_RAFT_GRU=split``: the opt-in route on which RAFT's SepConvGRU runs channels-last, its 1x5 / 5x1 convolutions on
alo_hip.conv_taps_f32 and its gates on the channels-last alo_gru_gate / alo_gru_update (alonet/raft/update.py).  Alone it leaves the
rest of the update block as it is; with ``ALO_RAFT_CONV3X3=split`` the encoder writes into the GRU's buffer and ``net`` stays
channels-last into the heads.  The bars are those of test_raft_split_route_gpu.py."""
import copy

import numpy as np
import pytest
import torch

import alo_hip
from alonet.raft import RAFT
from alonet.raft.corr import TorchCorrBlock
from alonet.raft.update import SepConvGRU
from guarded import GuardedLaunches
from test_raft_split_route_gpu import KNOB as KNOB3, _block_and_inputs, _g7, _run_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "ALO_RAFT_GRU"
KNOBS = pytest.mark.parametrize("both", [False, True], ids=["gru-knob", "both-knobs"])
TAPS = ("conv1x5_f32", "conv5x1_f32")


def _set(monkeypatch, gru, conv3x3=False):
    for name, on in ((KNOB, gru), (KNOB3, conv3x3)):
        if on:
            monkeypatch.setenv(name, "split")
        else:
            monkeypatch.delenv(name, raising=False)


def _taps_calls(tags):
    return {tag: v["calls"] for tag, v in tags.items() if tag.startswith(TAPS)}


def _gru_and_inputs(b, h, w):
    torch.manual_seed(6)
    gru = SepConvGRU(hidden_dim=128, input_dim=256).eval()
    return gru, (torch.randn(b, 128, h, w).tanh(), torch.randn(b, 256, h, w))


def _run_gru(gru, args):
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = gru(*[a.to(DEV) for a in args])
    return out.cpu(), timer.summary()


def _meets_the_bar(name, got, base, want):
    e_stock, e_split = (base.double() - want).abs().max().item(), (got.double() - want).abs().max().item()
    print(f"{name}: stock route {e_stock:.3g}, split route {e_split:.3g} against fp64 (max |ref| {want.abs().max().item():.3g})")
    assert got.shape == base.shape
    assert e_split <= 4 * e_stock + 3e-7 * want.abs().max().item(), (name, e_split, e_stock)   # test_update_block_on_the_split_route's bar


@pytest.mark.parametrize("b,h,w,served", [(2, 12, 16, True), (1, 5, 7, False)], ids=["12x16", "5x7"])
def test_sepconvgru_against_its_fp64_copy(monkeypatch, b, h, w, served):
    """12 x 16: four five-tap launches and four channels-last gate passes per call.  5 x 7: H*W % 4 != 0, where the fused plumbing
    (``_fusable``) steps aside as a whole and the stock ops run — the same bar either way."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    gru, args = _gru_and_inputs(b, h, w)
    with torch.no_grad():
        want = copy.deepcopy(gru).double()(*[a.double() for a in args])
    gru = gru.to(DEV)
    _set(monkeypatch, False)
    _run_gru(gru, args)                                      # MIOpen picks its solvers on a shape's first call
    stock, tags = _run_gru(gru, args)
    assert not _taps_calls(tags) and not any(tag.startswith("gru_gate_rows") for tag in tags), tags
    _set(monkeypatch, True)
    split, tags_split = _run_gru(gru, args)
    if served:
        assert _taps_calls(tags_split) == {"conv1x5_f32/C=384": 2, "conv5x1_f32/C=384": 2}, tags_split
        assert {t: v["calls"] for t, v in tags_split.items() if t.startswith("gru_")} == {"gru_gate_rows/C=128": 2, "gru_update_rows/C=128": 2}
    else:
        assert not tags_split, tags_split
    assert split.is_contiguous()
    _meets_the_bar(f"SepConvGRU {h}x{w}", split, stock, want)
    again, _ = _run_gru(gru, args)
    assert torch.equal(again, split)
    _set(monkeypatch, False)
    back, tags_back = _run_gru(gru, args)
    assert torch.equal(back, stock) and set(tags_back) == set(tags)


@KNOBS
def test_update_block_on_the_gru_route(monkeypatch, both):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    blk, args = _block_and_inputs()
    with torch.no_grad():
        ref = copy.deepcopy(blk).double()(*[a.double() for a in args])
    blk = blk.to(DEV)
    _set(monkeypatch, False)
    _run_block(blk, args)
    stock, tags = _run_block(blk, args)
    assert not _taps_calls(tags)
    _set(monkeypatch, False, both)
    _, tags_3x3 = _run_block(blk, args)                      # what ALO_RAFT_CONV3X3=split launches without the new knob
    _set(monkeypatch, True, both)
    _run_block(blk, args)
    split, tags_split = _run_block(blk, args)
    assert _taps_calls(tags_split) == {"conv1x5_f32/C=384": 2, "conv5x1_f32/C=384": 2}, tags_split
    assert {t: v["calls"] for t, v in tags_split.items() if t.startswith("conv3x3_f32")} == \
        {t: v["calls"] for t, v in tags_3x3.items() if t.startswith("conv3x3_f32")}
    assert ("gru_gate/C=128" in tags_3x3) and "gru_gate/C=128" not in tags_split
    for name, got, base, want in zip(("net", "up_mask", "delta_flow"), split, stock, ref):
        _meets_the_bar(name, got, base, want)
    _set(monkeypatch, False)
    back, tags_back = _run_block(blk, args)
    assert all(torch.equal(a, b) for a, b in zip(stock, back)) and set(tags_back) == set(tags)


@KNOBS
def test_raft_on_the_gru_route_matches_reference(golden, monkeypatch, both):
    """G7 at the bars of test_raft_on_hip_matches_reference."""
    model = RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    _set(monkeypatch, True, both)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        outs = model(mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32), iters=4)
    tags = timer.summary()
    assert sum(_taps_calls(tags).values()) == 4 * 4
    assert sum(v["calls"] for tag, v in tags.items() if tag.startswith("conv3x3_f32")) == (4 * 4 if both else 0)
    flows = np.stack([o["flow"].cpu().numpy() for o in outs])
    assert np.isfinite(flows).all()
    assert np.abs(flows - g["flow"]).max() <= 1e-3
    assert np.abs(outs[-1]["up_flow"].cpu().numpy() - g["up_flow_last"]).max() <= 8e-3
    assert np.abs(outs[-1]["hidden_state"].cpu().numpy() - g["hidden_last"]).max() <= 1e-3


def test_raft_32_iterations_on_the_gru_route_against_fp64(golden, monkeypatch):
    """G7's frames, 32 iterations, against the fp64 CPU copy (TorchCorrBlock, .double()): with the new knob alone and with both knobs
    the final 1/8-resolution flow is within 4 x the default route's own error + 1e-4 px, the bar of
    test_raft_32_iterations_on_the_split_route_against_fp64.  (One test: the fp64 CPU reference is the expensive part.)"""
    ref_model = RAFT(corr_block=TorchCorrBlock).eval()
    g, mk = _g7(golden, ref_model)
    with torch.no_grad():
        want = ref_model.double()(mk(g["img1"], "cpu", torch.float64), mk(g["img2"], "cpu", torch.float64), iters=32, only_last=True)[-1]["flow"].double()
    model = RAFT().eval()
    _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32)
    err = {}
    for route, (gru, conv3x3) in {"default": (False, False), "gru": (True, False), "both": (True, True)}.items():
        _set(monkeypatch, gru, conv3x3)
        with torch.no_grad():
            flow = model(f1, f2, iters=32, only_last=True)[-1]["flow"].cpu().double()
        err[route] = (flow - want).abs().max().item()
    print(f"32 iterations, final 1/8 flow against fp64: default route {err['default']:.3g} px, ALO_RAFT_GRU=split {err['gru']:.3g} px, "
          f"both knobs {err['both']:.3g} px")
    assert err["gru"] <= 4 * err["default"] + 1e-4 and err["both"] <= 4 * err["default"] + 1e-4, err


@KNOBS
def test_graphed_raft_on_the_gru_route_replays_eager_bit_for_bit(golden, monkeypatch, both):
    from alonet.common import GraphedForward

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32)
    _set(monkeypatch, True, both)
    graphed = GraphedForward(model)
    with torch.no_grad():
        model(f1, f2, iters=4, only_last=True)               # MIOpen picks its solvers on a shape's first call
        for a, b in ((f1, f2), (f2, f1)):
            want = model(a, b, iters=4, only_last=True)[-1]
            got = graphed(a, b, iters=4, only_last=True)[-1]
            for key in ("flow", "up_flow", "hidden_state"):
                assert torch.equal(got[key], want[key]), key
    assert len(graphed._graphs) == 1


@KNOBS
def test_raft_three_iterations_under_guard(golden, monkeypatch, both):
    """MIOpen's solver choice varies between runs, so no bits are compared: the per-launch checks are the test."""
    model = RAFT().eval()
    g, mk = _g7(golden, model)
    model = model.to(DEV)
    f1, f2 = mk(g["img1"], DEV, torch.float32), mk(g["img2"], DEV, torch.float32)
    _set(monkeypatch, True, both)
    with torch.no_grad(), GuardedLaunches() as guard:
        outs = model(f1, f2, iters=3)
    tags = [tag or "" for _, tag in guard.seen]
    assert sum(tag.startswith(TAPS) for tag in tags) == 3 * 4 and sum(tag.startswith("gru_gate_rows") for tag in tags) == 3 * 2
    assert sum(tag.startswith("gru_update_rows") for tag in tags) == 3 * 2 and not any(tag.startswith(("gru_gate/", "gru_update/")) for tag in tags)
    for o in outs:
        assert torch.isfinite(o["flow"]).all() and torch.isfinite(o["up_flow"]).all()


@KNOBS
def test_grad_mode_takes_the_stock_route_and_reaches_the_gru_weights(monkeypatch, both):
    blk, args = _block_and_inputs()
    blk = blk.to(DEV)
    _set(monkeypatch, True, both)
    with alo_hip.LaunchTimer() as timer:
        net, up_mask, delta_flow = blk(*[a.to(DEV) for a in args])
        (net.sum() + up_mask.sum() + delta_flow.sum()).backward()
    assert not timer.summary(), timer.summary()
    for name in ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2"):
        grad = getattr(blk.gru, name).weight.grad
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0, name


def test_split_weights_go_with_invalidate_caches(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    gru, args = _gru_and_inputs(1, 12, 16)
    gru = gru.to(DEV)
    _set(monkeypatch, True)
    before, _ = _run_gru(gru, args)
    with torch.no_grad():
        for conv in (gru.convr1, gru.convq2):                # one half of a merged [z | r] weight and a plain one
            conv.weight.data.mul_(2.0)                       # through .data: no version bump
    stale, _ = _run_gru(gru, args)
    assert torch.equal(stale, before)                        # what the cache is for (and why load_weights invalidates)
    alo_hip.invalidate_caches(gru)
    fresh, _ = _run_gru(gru, args)
    want, _ = _run_gru(copy.deepcopy(gru), args)             # a copy derives its own split weights
    assert torch.equal(fresh, want) and not torch.equal(fresh, before)
