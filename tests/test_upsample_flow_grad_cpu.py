"""The backward of RAFT's convex flow up-sampling (ALO_UPSAMPLE_GRAD on alo_upsample_add_nhwc, aloception-oss_amd/csrc/upsample_flow.hip)
and ``alonet.raft.RAFTCriterion``, as far as they can be checked without a GPU: the C ABI is the parent's, the flagged call meets
its own argument checks, the criterion and the stock up-sampling under autograd agree with the reference's fixture (G21), the
formulas the kernel follows are autograd's, and CPU tensors and the bilinear mode never leave the stock ops.

Validation happens before anything is enqueued: every call below carries an argument that is refused, so none launches."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import alo_hip
import aloscene
import helpers
from alonet.raft import RAFTCriterion
from alonet.raft.raft import RAFTBase
from upsample_grad_ref import restated, stock_autograd, stock_up

F32, F64, BF16, F16 = alo_hip.ALO_F32, alo_hip.ALO_F64, alo_hip.ALO_BF16, alo_hip.ALO_F16
GRAD = alo_hip.ALO_UPSAMPLE_GRAD
ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
NAME = b"alo_upsample_add_nhwc: "
PREFIX = NAME + b"ALO_F32 | ALO_UPSAMPLE_GRAD: "
t = torch.from_numpy


def _call(x_low, fpn, out, BQ, Q, C, h, w, H, W, dtype):
    lib = alo_hip.lib()
    rc = lib.alo_upsample_add_nhwc(x_low, fpn, out, BQ, Q, C, h, w, H, W, dtype, None)
    return rc, lib.alo_last_error()


def test_abi_is_unchanged_and_the_flag_is_declared():
    declared = {h: helpers.declared_functions(h) for h in helpers.HEADERS}
    names = sorted(n for fns in declared.values() for n in fns)
    assert len(names) == len(set(names)) == 50 and len(declared["alo_hotpath.h"]) == 42
    assert set(names) == helpers.exported_alo_functions(alo_hip.LIB_PATH) == set(alo_hip._SIGNATURES)
    restype, argtypes = alo_hip._SIGNATURES["alo_upsample_add_nhwc"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    assert alo_hip.lib().alo_abi_version() == 3
    assert "#define ALO_UPSAMPLE_GRAD 0x100" in helpers.header_text("alo_hotpath.h") and GRAD == 0x100


# (x_low, fpn, out, BQ, Q, C, h, w, H, W) -> status, what the message names: the forward's table (test_upsample_flow_cpu.BAD_F32) with a
# mask in every row, plus the NULL mask
BAD_GRAD = {
    "x_low": ((None, ONE, ONE, 2, 1, 2, 5, 7, 40, 56), 1, b"x_low and out must not be null"),
    "out": ((ONE, ONE, None, 2, 1, 2, 5, 7, 40, 56), 1, b"x_low and out must not be null"),
    "fpn": ((ONE, None, ONE, 2, 1, 2, 5, 7, 40, 56), 1, b"fpn (the mask logits) must not be null"),
    "BQ": ((ONE, ONE, ONE, 0, 1, 2, 5, 7, 40, 56), 1, b"BQ must be positive (BQ=0)"),
    "Q": ((ONE, ONE, ONE, 2, 2, 2, 5, 7, 40, 56), 1, b"Q must be 1 (Q=2)"),
    "C=0": ((ONE, ONE, ONE, 2, 1, 0, 5, 7, 40, 56), 2, b"C must be 1 to 8 flow channels (C=0)"),
    "C=9": ((ONE, ONE, ONE, 2, 1, 9, 5, 7, 40, 56), 2, b"C must be 1 to 8 flow channels (C=9)"),
    "C=16": ((ONE, ONE, ONE, 2, 1, 16, 5, 7, 40, 56), 2, b"C must be 1 to 8 flow channels (C=16)"),
    "h": ((ONE, ONE, ONE, 2, 1, 2, 0, 7, 0, 56), 1, b"h and w must be positive (h=0 w=7)"),
    "w": ((ONE, ONE, ONE, 2, 1, 2, 5, -1, 40, -8), 1, b"h and w must be positive (h=5 w=-1)"),
    "H": ((ONE, ONE, ONE, 2, 1, 2, 5, 7, 41, 56), 1, b"H and W must be 8 h and 8 w (h=5 w=7 H=41 W=56)"),
    "W": ((ONE, ONE, ONE, 2, 1, 2, 5, 7, 40, 7), 1, b"H and W must be 8 h and 8 w (h=5 w=7 H=40 W=7)"),
    "x_low aligned": ((ODD, ONE, ONE, 2, 1, 2, 5, 7, 40, 56), 1, b"pointers must be 16-byte aligned"),
    "fpn aligned": ((ONE, ODD, ONE, 2, 1, 2, 5, 7, 40, 56), 1, b"pointers must be 16-byte aligned"),
    "out aligned": ((ONE, ONE, ODD, 2, 1, 2, 5, 7, 40, 56), 1, b"pointers must be 16-byte aligned"),
}


@pytest.mark.parametrize("name", sorted(BAD_GRAD))
def test_flagged_call_names_its_bad_argument(name):
    args, status, names = BAD_GRAD[name]
    rc, msg = _call(*args, F32 | GRAD)
    assert rc == status and msg.startswith(PREFIX) and names in msg, (name, rc, msg)
    assert b"bf16 only" not in msg and b"multiple of 8" not in msg


def test_flagged_checks_run_in_the_forwards_order():
    # everything wrong at once is answered for the pointers, the mask, then Q, C, h / w, H / W, alignment
    args = [None, None, None, 2, 3, 0, 0, 0, 1, 1]
    for fix, names in (({0: ONE, 2: ODD}, b"x_low and out must not be null"), ({1: ODD}, b"fpn (the mask logits) must not be null"),
                       ({4: 1}, b"Q must be 1"), ({5: 2}, b"C must be 1 to 8"), ({6: 5, 7: 7}, b"h and w must be positive"),
                       ({8: 40, 9: 56}, b"H and W must be 8 h and 8 w"), ({1: ONE, 2: ONE}, b"16-byte aligned")):
        rc, msg = _call(*args, F32 | GRAD)
        assert rc != 0 and msg.startswith(PREFIX) and names in msg, (args, rc, msg)
        for k, v in fix.items():
            args[k] = v
    # well formed now, and so large that the one size limit refuses it: nothing is enqueued
    rc, msg = _call(ONE, ONE, ONE, 1, 1, 2, 2000, 2000, 16000, 16000, F32 | GRAD)
    assert rc == 2 and msg == NAME + b"the mask of one image must stay below 4 GiB (h=2000 w=2000)", (rc, msg)


@pytest.mark.parametrize("dtype", [BF16 | GRAD, F16 | GRAD, F64 | GRAD, F32 | GRAD | 0x200, F32 | 0x200, F32 | 0x10000, 7 | GRAD],
                         ids=["bf16", "f16", "f64", "stray bit with the flag", "stray bit", "high stray bit", "unknown dtype"])
def test_flag_with_anything_else_is_unsupported_and_named(dtype):
    for args in ((ONE, ONE, ONE, 2, 1, 2, 5, 7, 40, 56), (ONE, ONE, ONE, 2, 1, 8, 5, 7, 40, 56), (None, None, None, 0, 0, 0, 0, 0, 0, 0)):
        rc, msg = _call(*args, dtype)
        assert rc == 2 and msg.startswith(NAME) and b"ALO_UPSAMPLE_GRAD" in msg and b"bf16 only" not in msg, (dtype, rc, msg)


def test_unflagged_dtypes_answer_as_they_always_did():
    assert _call(ONE, ONE, ONE, 2, 1, 8, 5, 7, 40, 56, 7) == (2, NAME + b"bf16 only (dtype 7)")
    assert _call(ONE, ONE, ONE, 2, 1, 8, 5, 7, 40, 56, F16) == (2, NAME + b"bf16 only (dtype %d)" % F16)
    assert _call(ONE, None, ONE, 2, 1, 8, 5, 7, 40, 56, BF16) == (1, NAME + b"null pointer argument")
    rc, msg = _call(ONE, None, ONE, 2, 1, 2, 5, 7, 40, 57, F32)          # the forward: fpn may be NULL, its own prefix
    assert rc == 1 and msg.startswith(NAME + b"ALO_F32: H and W must be 8 h and 8 w"), (rc, msg)


# ---- RAFTCriterion against the reference's fixture ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g21(golden):
    return golden("g21_raft_criterion.npz")


METRICS = ("loss", "epe", "1px", "3px", "5px")


def _run_case(g, p, valid="fixture"):
    flow = t(g[p + "flow"]).double().requires_grad_()
    mask = t(g[p + "mask"]).double().requires_grad_()
    flow_gt = t(g[p + "flow_gt"])
    if valid == "fixture":
        valid = t(g[p + "valid"]) if p + "valid" in g.files else None
    outs = [{"up_flow": stock_up(flow[i], mask[i])} for i in range(flow.shape[0])]
    loss, metrics, epe_per_iter = RAFTCriterion.sequence_loss(outs, flow_gt, valid, compute_per_iter=True)
    loss.backward()
    return outs, loss, metrics, epe_per_iter, flow.grad, mask.grad


def _close(got, want, what, tol=1e-12):
    got, want = np.asarray(got.detach() if isinstance(got, torch.Tensor) else got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max() <= tol, (what, np.abs(got - want).max())


@pytest.mark.parametrize("p", ["a_", "b_"], ids=["N=1 with valid", "N=2 without"])
def test_criterion_meets_the_reference_fixture(g21, p):
    g = g21
    assert g[p + "flow"].dtype == np.float32 and g[p + "grad_mask"].dtype == np.float64 and g[p + "flow"].shape[0] == 3
    if p == "a_":
        assert tuple(g["a_flow"].shape) == (3, 1, 2, 3, 5) and int(g["a_valid"].sum()) == 959 and g["a_epe_per_iter"].shape == (3, 958)
        assert (g["a_flow_gt"] == 2000).sum() == 1 and np.isclose(np.sqrt((g["a_flow_gt"] ** 2).sum(1)), 495).sum() == 1
    else:
        assert g["b_flow"].shape[1] == 2 and "b_valid" not in g.files
    outs, loss, metrics, epe_per_iter, grad_flow, grad_mask = _run_case(g, p)
    assert loss.dtype == torch.float64 and loss.requires_grad and all(isinstance(metrics[k], float) for k in METRICS)
    _close(torch.stack([o["up_flow"] for o in outs]), g[p + "up_flow"], "up_flow")
    _close(loss, g[p + "loss"], "loss")
    _close([metrics[k] for k in METRICS], g[p + "metrics"], "metrics")
    assert metrics["loss"] == loss.item()
    _close(torch.stack(epe_per_iter), g[p + "epe_per_iter"], "epe_per_iter")
    _close(grad_flow, g[p + "grad_flow"], "grad_flow")
    _close(grad_mask, g[p + "grad_mask"], "grad_mask")
    *_, none = RAFTCriterion.sequence_loss([{"up_flow": o["up_flow"].detach()} for o in outs], t(g[p + "flow_gt"]))
    assert none is None


def test_criterion_forward_reads_the_frames_flow(g21):
    g = g21
    up = [{"up_flow": t(a)} for a in g["a_up_flow"]]
    gt = aloscene.Flow(t(g["a_flow_gt"][0]))
    frame = aloscene.Frame(torch.zeros(1, 3, 24, 40), normalization="minmax_sym", names=("B", "C", "H", "W"), flow={"flow_forward": [gt]})
    loss, metrics, epe_per_iter = RAFTCriterion()(up, frame, compute_per_iter=True)
    _close(loss, g["a_loss"], "loss")
    _close([metrics[k] for k in METRICS], g["a_metrics"], "metrics")
    _close(torch.stack(epe_per_iter), g["a_epe_per_iter"], "epe_per_iter")
    loss_all, metrics_all, none = RAFTCriterion()(up, frame, use_valid=False)
    assert none is None and loss_all > loss and metrics_all["epe"] > metrics["epe"]      # the 2000 counts now
    with pytest.raises(AssertionError):
        RAFTCriterion()(up, torch.zeros(1, 3, 24, 40))


def test_valid_is_applied_per_sample(g21):
    """The documented difference to the reference (alonet/raft/criterion.py, module docstring): N > 1 with ``valid`` is N independent
    N = 1 evaluations — the loss their mean, the end-point errors their concatenation."""
    gen = torch.Generator().manual_seed(5)
    N, T = 3, 2
    ups = [torch.randn(N, 2, 8, 16, generator=gen, dtype=torch.float64) for _ in range(T)]
    flow_gt = 3 * torch.randn(N, 2, 8, 16, generator=gen, dtype=torch.float64)
    flow_gt[1, :, 2, 3] = torch.tensor([500.0, 1.0], dtype=torch.float64)            # past max_flow in sample 1 alone
    valid = (torch.rand(N, 8, 16, generator=gen) > 0.3).float()
    valid[1, 2, 3] = 1.0
    assert len({int(v.sum()) for v in valid}) == N                                     # a different count per sample
    loss, metrics, per_iter = RAFTCriterion.sequence_loss([{"up_flow": u} for u in ups], flow_gt, valid, compute_per_iter=True)
    singles = [RAFTCriterion.sequence_loss([{"up_flow": u[n:n + 1]} for u in ups], flow_gt[n:n + 1], valid[n:n + 1], compute_per_iter=True)
               for n in range(N)]
    _close(loss, torch.stack([s[0] for s in singles]).mean(), "loss")
    for i in range(T):
        assert torch.equal(per_iter[i], torch.cat([s[2][i] for s in singles]))
    counted = int(valid.sum()) - 1
    assert per_iter[0].numel() == counted
    epe = torch.cat([s[2][-1] for s in singles])
    _close([metrics["epe"], metrics["1px"]], [epe.mean().item(), (epe < 1).float().mean().item()], "metrics")


# ---- the formulas the kernel follows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 2, 3, 5), (1, 3, 4, 6), (1, 8, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_restated_backward_is_autograd_of_the_stock_chain(shape):
    N, C, h, w = shape
    gen = torch.Generator().manual_seed(sum(shape))
    flow = 4 * torch.randn(N, C, h, w, generator=gen, dtype=torch.float64)
    mask = 3 * torch.randn(N, 576, h, w, generator=gen, dtype=torch.float64)
    mask.view(-1)[::97] = 30.0
    mask.view(-1)[5::101] = -30.0
    grad_up = torch.randn(N, C, 8 * h, 8 * w, generator=gen, dtype=torch.float64)
    want_flow, want_mask = stock_autograd(flow, mask, grad_up)
    got_flow, got_mask, taps = restated(flow, mask, grad_up)
    assert tuple(taps.shape) == (N, 9 * C, h * w)
    _close(got_flow, want_flow, "grad_flow")
    _close(got_mask, want_mask, "grad_mask")


def test_restated_backward_on_the_fixture(g21):
    g, gt = g21, t(g21["a_flow_gt"])
    for i in range(3):
        flow, mask = t(g["a_flow"][i]).double(), t(g["a_mask"][i]).double()
        up = stock_up(flow, mask)
        # d loss / d up_flow[i] of the sequence loss: gamma^(T - 1 - i) sign(up - gt) on the counted pixels, over the mean's size
        counted = t(g["a_valid"])[:, None] & (gt.pow(2).sum(1, keepdim=True).sqrt() < 400)
        grad_up = 0.8 ** (2 - i) * torch.sign(up - gt) * counted / up.numel()
        got_flow, got_mask, _ = restated(flow, mask, grad_up)
        _close(got_flow, g["a_grad_flow"][i], "grad_flow")
        _close(got_mask, g["a_grad_mask"][i], "grad_mask")


# ---- the route -----------------------------------------------------------------------------------------------------------------------
def test_train_knob_keeps_cpu_tensors_and_the_bilinear_mode_on_stock_ops(g21, monkeypatch):
    flow, mask = t(g21["a_flow"][0]), t(g21["a_mask"][0])
    this = types.SimpleNamespace(out_plane=2)
    monkeypatch.delenv("ALO_RAFT_UPSAMPLE", raising=False)
    stock, stock_bilinear = RAFTBase.upsample_flow(this, flow, mask), RAFTBase.upsample_flow(this, flow, None)

    def refuse(*a, **k):
        raise AssertionError("a kernel wrapper was called for a CPU tensor or for the bilinear mode under grad")

    for name in ("upsample_flow", "upsample_flow_autograd", "upsample_flow_grad"):
        monkeypatch.setattr(alo_hip, name, refuse)
    monkeypatch.setenv("ALO_RAFT_UPSAMPLE", "train")
    assert os.environ["ALO_RAFT_UPSAMPLE"] == "train"
    f, m = flow.clone().requires_grad_(), mask.clone().requires_grad_()
    up = RAFTBase.upsample_flow(this, f, m)
    assert up.requires_grad and torch.equal(up.detach(), stock)
    up.sum().backward()
    assert f.grad is not None and m.grad is not None
    up = RAFTBase.upsample_flow(this, f, None)
    assert up.requires_grad and torch.equal(up.detach(), stock_bilinear)
    with torch.no_grad():
        assert torch.equal(RAFTBase.upsample_flow(this, flow, mask), stock)
        assert torch.equal(RAFTBase.upsample_flow(this, flow, None), stock_bilinear)
    # the bilinear mode under grad stays on stock ops whatever the device: the route needs a mask before it asks the gate
    from alonet.raft import raft as raft_module

    meta = torch.empty(1, 2, 3, 5, device="meta")
    assert not raft_module._upsample_train_route(meta, None)
    assert not alo_hip.upsample_flow_autograd_supported(flow, mask) and not alo_hip.upsample_flow_autograd_supported(flow, None)
