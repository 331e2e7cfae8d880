"""The backward of RAFT's convex flow up-sampling in one launch (``alo_hip.upsample_flow_grad`` / ``upsample_flow_autograd``:
ALO_UPSAMPLE_GRAD of alo_upsample_add_nhwc, aloception-oss_amd/csrc/upsample_flow.hip) and its opt-in route ``ALO_RAFT_UPSAMPLE=train``.

The reference is float64 autograd of the stock chain on the same fp32 inputs (the formulas the kernel follows are pinned to it in
test_upsample_flow_grad_cpu.py).  Error bars, u = 2^-24; the stock fp32 chain under autograd is held to the same bars on the same
inputs, which checks the bars.

  grad_mask  |got - ref64| <= 64 u T,  T = max_k sum_c |G_c| |8 flow_ck| of the entry's fine pixel (G = grad_up there, k the nine taps).
             Budget (2 C + 40) u T, C <= 8.  With d_k = logit_k - max: the subtraction and the product with log2(e) perturb w_k by
             2 |d_k| u w_k, exp and the reciprocal are good to one ulp (2 u) each, the nine positive terms of the sum add 8 u, the
             product 1 u: |dw_k| <= (13 + 2 |d_k|) u w_k, and sum_k w_k |d_k| <= 8 / e.  t_k is a C-term fma chain: C u T.
             s = sum_k w_k t_k: (13 + 16 / e) u T from the weights, C u T from the t_k, 9 u T from its own chain: (C + 28) u T.
             t_k - s rounds once: 2 u T.  Times w_k <= 1: (2 C + 30) u T.  The weight's own error multiplies |t_k - s| =
             |sum_k' w_k' (t_k - t_k')| <= 2 (1 - w_k) T, and w_k (1 - w_k) <= 1 / 4, w_k |d_k| <= 1 / e: (6.5 + 1.5) u T.  The last
             product: 1 u T.  (2 C + 39) u T.
  grad_flow  |got - ref64| <= (c_acc(576) + 16 u) A,  A = the entry's own sum (9 taps x 64 fine pixels) on |grad_up|, the weights being
             positive: a 576-term accumulation in any order (kernel_bounds.c_acc) and the weights' relative error (13 + 2 |d|) u <= 16 u
             where the weight matters.

Measured on MI355X (worst |error| / bar over this file's cases): docs/experiments.md, "RAFT flow up-sampling: the backward".
"""
import pytest
import torch

import alo_hip
import aloscene
from alonet.raft import RAFT, RAFTCriterion
from alonet.raft.corr import TorchCorrBlock
from guarded import GuardedLaunches
from helpers import formula_state_dict
from kernel_bounds import c_acc
from upsample_grad_ref import bars, stock_autograd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "ALO_RAFT_UPSAMPLE"
SHAPES = [(1, 2, 1, 1), (2, 2, 3, 5), (1, 2, 2, 65), (3, 1, 4, 6), (1, 4, 5, 7), (2, 3, 9, 67), (1, 8, 13, 21)]   # the forward's list


@pytest.fixture(autouse=True)
def no_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def _case(N, C, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    flow = (4 * torch.randn(N, C, h, w, generator=gen)).to(DEV)
    mask = (3 * torch.randn(N, 576, h, w, generator=gen)).to(DEV)
    mask.view(-1)[::997] = 30.0
    mask.view(-1)[5::1009] = -30.0
    grad_up = torch.randn(N, C, 8 * h, 8 * w, generator=gen).to(DEV)
    return flow, mask, grad_up


def _ref64(flow, mask, grad_up):
    return stock_autograd(flow.double().cpu(), mask.double().cpu(), grad_up.double().cpu())


def _worst_ratio(got, ref64, bar, what):
    """max |got - ref64| / bar (0 / 0 counts as 0) after asserting the same NaN / inf pattern."""
    got = got.double().cpu()
    assert got.shape == ref64.shape, what
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)) and torch.equal(torch.isfinite(got), fin), what
    assert torch.equal(got[~fin & ~torch.isnan(ref64)], ref64[~fin & ~torch.isnan(ref64)]), what
    err, b = (got[fin] - ref64[fin]).abs(), bar[fin]
    assert torch.isfinite(b).all(), what
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(ratio.max()) if ratio.numel() else 0.0


def _check_both(flow, mask, grad_up, what):
    ref_flow, ref_mask = _ref64(flow, mask, grad_up)
    bar_flow, bar_mask = bars(flow, mask, grad_up, c_acc(576))
    got_flow, got_mask = alo_hip.upsample_flow_grad(flow, mask, grad_up)
    assert got_flow.dtype == got_mask.dtype == torch.float32 and got_flow.shape == flow.shape and got_mask.shape == mask.shape
    stock_flow, stock_mask = stock_autograd(flow, mask, grad_up)
    r = {"kernel": (_worst_ratio(got_flow, ref_flow, bar_flow, what + ": kernel grad_flow"),
                    _worst_ratio(got_mask, ref_mask, bar_mask, what + ": kernel grad_mask")),
         "stock chain": (_worst_ratio(stock_flow, ref_flow, bar_flow, what + ": stock grad_flow"),
                         _worst_ratio(stock_mask, ref_mask, bar_mask, what + ": stock grad_mask"))}
    print(f"{what}: worst |error| / bar (grad_flow, grad_mask)  kernel {r['kernel'][0]:.3f} {r['kernel'][1]:.3f}  "
          f"stock chain {r['stock chain'][0]:.3f} {r['stock chain'][1]:.3f}")
    assert max(r["stock chain"]) <= 1.0, (what, "the stock fp32 chain misses the bar: the bar is wrong", r)
    assert max(r["kernel"]) <= 1.0, (what, r)
    return got_flow, got_mask


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_error_bars(shape):
    flow, mask, grad_up = _case(*shape, seed=sum(shape))
    assert alo_hip.upsample_flow_autograd_supported(flow, mask)
    _check_both(flow, mask, grad_up, f"backward {shape}")


def test_a_minus_inf_logit_is_weight_zero_as_in_fp64():
    flow, mask, grad_up = _case(2, 2, 4, 6, seed=3)
    mask[1, 5 * 64 + 20, 1, 1] = float("-inf")
    mask[0, 0 * 64 + 0, 0, 0] = float("-inf")
    got_flow, got_mask = _check_both(flow, mask, grad_up, "backward with -inf logits")
    assert torch.isfinite(got_flow).all() and torch.isfinite(got_mask).all()
    assert got_mask[1, 5 * 64 + 20, 1, 1] == 0 and got_mask[0, 0, 0, 0] == 0


def test_two_runs_are_bit_equal():
    flow, mask, grad_up = _case(2, 3, 9, 67, seed=4)
    a, b = alo_hip.upsample_flow_grad(flow, mask, grad_up), alo_hip.upsample_flow_grad(flow, mask, grad_up)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", [(2, 2, 3, 5), (1, 3, 2, 65), (1, 5, 3, 11)], ids=["2x2x3x5", "1x3x2x65", "1x5x3x11"])
def test_buffer_discipline(shape):
    """Guarded buffers (tests/guarded.py): `out` (grad_mask, then taps) starts as NaN bytes, then as 0x3C bytes; nothing outside it
    changes, the inputs keep their bytes and the two results agree bit for bit: every byte of `out` is written."""
    flow, mask, grad_up = _case(*shape, seed=9)
    with GuardedLaunches() as guard:
        got_flow, got_mask = alo_hip.upsample_flow_grad(flow, mask, grad_up)
    assert guard.seen == [("alo_upsample_add_nhwc", "upsample_flow_grad")]
    assert torch.isfinite(got_flow).all() and torch.isfinite(got_mask).all()
    again = alo_hip.upsample_flow_grad(flow, mask, grad_up)
    assert torch.equal(got_flow, again[0]) and torch.equal(got_mask, again[1])


def test_grad_up_views_are_absorbed_by_the_packing_copy():
    flow, mask, grad_up = _case(2, 2, 3, 5, seed=6)
    f, m = flow.clone().requires_grad_(), mask.clone().requires_grad_()
    up = alo_hip.upsample_flow_autograd(f, m)
    assert up.requires_grad and torch.equal(up.detach(), alo_hip.upsample_flow(flow, mask))
    up.sum().backward()                                             # grad_up is an expanded scalar: every stride 0
    want = alo_hip.upsample_flow_grad(flow, mask, torch.ones_like(grad_up))
    assert torch.equal(f.grad, want[0]) and torch.equal(m.grad, want[1])
    wide = torch.randn(2, 4, 24, 40, device=DEV)
    strided = wide[:, ::2]                                          # channel-strided
    assert not strided.is_contiguous()
    got, want = alo_hip.upsample_flow_grad(flow, mask, strided), alo_hip.upsample_flow_grad(flow, mask, strided.contiguous())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(RuntimeError, match="grad_up"):
        alo_hip.upsample_flow_grad(flow, mask, grad_up[:, :1])
    with pytest.raises(RuntimeError, match="upsample_flow_grad"):
        alo_hip.upsample_flow_grad(flow, None, grad_up)


@pytest.mark.parametrize("which", ["flow", "mask"])
def test_only_one_input_requires_grad(which):
    flow, mask, grad_up = _case(1, 2, 3, 5, seed=7)
    f = flow.clone().requires_grad_(which == "flow")
    m = mask.clone().requires_grad_(which == "mask")
    up = alo_hip.upsample_flow_autograd(f, m)
    up.backward(grad_up)
    want = alo_hip.upsample_flow_grad(flow, mask, grad_up)
    if which == "flow":
        assert m.grad is None and torch.equal(f.grad, want[0])
    else:
        assert f.grad is None and torch.equal(m.grad, want[1])
    with torch.no_grad():                                            # nothing recorded: the plain forward
        assert not alo_hip.upsample_flow_autograd(f, m).requires_grad
    assert not alo_hip.upsample_flow_autograd_supported(flow, None)
    assert not alo_hip.upsample_flow_autograd_supported(flow.double(), mask.double())
    assert not alo_hip.upsample_flow_autograd_supported(flow.cpu(), mask.cpu())
    with pytest.raises(RuntimeError, match="upsample_flow_autograd"):
        alo_hip.upsample_flow_autograd(flow, None)


# ---- the model route --------------------------------------------------------------------------------------------------------------
def _calls(timer):
    return {tag: v["calls"] for tag, v in timer.summary().items()}


def _frames(dtype, device):
    gen = torch.Generator().manual_seed(11)
    mk = lambda: aloscene.Frame((2 * torch.rand(1, 3, 128, 128, generator=gen) - 1).to(dtype), normalization="minmax_sym",  # noqa: E731
                                names=("B", "C", "H", "W")).to(device)
    f1, f2 = mk(), mk()
    flow_gt = (3 * torch.randn(1, 2, 128, 128, generator=gen)).to(dtype).to(device)
    return f1, f2, flow_gt


def _param_grads(model, f1, f2, flow_gt):
    model.zero_grad(set_to_none=True)
    outs = model(f1, f2, iters=2)
    loss, _, _ = RAFTCriterion.sequence_loss(outs, flow_gt)
    loss.backward()
    return outs, {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}


def test_tiny_raft_trains_through_the_kernels(monkeypatch):
    """RAFT, 2 iterations on 1 x 3 x 128 x 128, sequence loss: the smallest frame on which RAFT runs at all — the fourth correlation
    level is the 1/64-size map, and the lookup (the reference's sampler divides by size - 1; alo_corr_lookup refuses it) needs
    2 x 2 there.  ``train`` against the knob unset: the same flows, up_flow with the bits
    of the ``fused`` forward launch, and parameter gradients as close to a float64 run of the model (TorchCorrBlock, CPU) as the stock fp32
    route's are: both are fp32 chains that differ in summation order only, so the ``train`` route's max-abs error per parameter may be
    4 x the stock route's plus 1e-7 of the gradient's largest entry."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = RAFT().eval()
    state = formula_state_dict(model.state_dict())
    model.load_state_dict(state)
    model = model.to(DEV)
    f1, f2, flow_gt = _frames(torch.float32, DEV)
    _param_grads(model, f1, f2, flow_gt)                            # MIOpen picks its solvers on a shape's first call
    with alo_hip.LaunchTimer() as timer:
        off_outs, off = _param_grads(model, f1, f2, flow_gt)
    assert "upsample_flow" not in _calls(timer) and "upsample_flow_grad" not in _calls(timer)

    monkeypatch.setenv(KNOB, "fused")
    with alo_hip.LaunchTimer() as timer:
        _param_grads(model, f1, f2, flow_gt)                        # `fused` under grad mode: stock ops, as ever
    assert "upsample_flow" not in _calls(timer) and "upsample_flow_grad" not in _calls(timer)
    with torch.no_grad():
        fused_outs = model(f1, f2, iters=2)

    monkeypatch.setenv(KNOB, "train")
    with alo_hip.LaunchTimer() as timer:
        on_outs, on = _param_grads(model, f1, f2, flow_gt)
    assert _calls(timer)["upsample_flow"] == 2 and _calls(timer)["upsample_flow_grad"] == 2
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        nograd_outs = model(f1, f2, iters=2)                        # grad mode off: `train` is `fused`
    assert _calls(timer)["upsample_flow"] == 2 and "upsample_flow_grad" not in _calls(timer)
    for a, b, c, d in zip(on_outs, off_outs, fused_outs, nograd_outs):
        assert torch.equal(a["flow"], b["flow"]) and torch.equal(a["up_mask"], b["up_mask"])
        # the forward launch's bits on the same operands; with grad mode off the model's other layers take their inference kernels,
        # so `train` is compared with `fused` there
        assert a["up_flow"].requires_grad and torch.equal(a["up_flow"], alo_hip.upsample_flow(a["flow"].detach(), a["up_mask"].detach()))
        assert torch.equal(d["up_flow"], c["up_flow"]) and torch.equal(d["flow"], c["flow"])
    monkeypatch.delenv(KNOB)

    ref = RAFT(corr_block=TorchCorrBlock).eval()
    ref.load_state_dict(state)
    ref = ref.double()
    _, want = _param_grads(ref, *_frames(torch.float64, "cpu"))
    assert set(on) == set(off) == set(want) and len(want) > 50
    worst = (0.0, None)
    for k in sorted(want):
        scale = float(want[k].abs().max())
        e_on, e_off = float((on[k] - want[k]).abs().max()), float((off[k] - want[k]).abs().max())
        print(f"{k}: max |grad| {scale:.3e}  error train {e_on:.3e}  stock {e_off:.3e}")
        worst = max(worst, (e_on / (4 * e_off + 1e-7 * scale) if e_on else 0.0, k))
        assert e_on <= 4 * e_off + 1e-7 * scale, (k, e_on, e_off, scale)
    print(f"tiny RAFT: worst error(train) / (4 error(stock) + 1e-7 max |grad|) = {worst[0]:.3f} at {worst[1]}")


def test_peak_memory_is_lower_on_the_train_route(monkeypatch):
    """Forward + backward of 3 up-samplings at (2, 2, 24, 32): autograd keeps the softmax output and the broadcast product's operands
    per up-sampling on the stock route, the logits alone on the ``train`` route."""
    from alonet.raft.raft import RAFTBase
    import types

    this = types.SimpleNamespace(out_plane=2)
    gen = torch.Generator().manual_seed(1)
    flows = [(4 * torch.randn(2, 2, 24, 32, generator=gen)).to(DEV).requires_grad_() for _ in range(3)]
    masks = [(3 * torch.randn(2, 576, 24, 32, generator=gen)).to(DEV).requires_grad_() for _ in range(3)]

    def peak():
        for t in flows + masks:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ups = [RAFTBase.upsample_flow(this, f, m) for f, m in zip(flows, masks)]
        sum(u.abs().mean() for u in ups).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    stock = peak()
    monkeypatch.setenv(KNOB, "train")
    with alo_hip.LaunchTimer() as timer:
        train = peak()
    assert _calls(timer) == {"upsample_flow": 3, "upsample_flow_grad": 3}
    print(f"peak memory above the inputs, 3 up-samplings at (2, 2, 24, 32), forward + backward: stock {stock} bytes, train {train} bytes")
    assert train < stock, (train, stock)

