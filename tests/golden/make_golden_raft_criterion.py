#!/usr/bin/env python
"""G21 — the reference's RAFT criterion over its own convex up-sampling, under autograd (build container only).

  g21_raft_criterion.npz   alonet/raft/criterion.py (RAFTCriterion.sequence_loss) on the ``up_flow`` of alonet/raft/raft.py:109-123
                           (RAFTBase.upsample_flow), everything computed in fp64 (the inputs are fp32 values, stored as
                           such and used as their float64 copies), T = 3 iterations.
                           Two cases, keys prefixed ``a_`` and ``b_``:
                             a   N = 1, coarse map 3 x 5 (fine 24 x 40), with a ``valid`` mask, formed as RAFTCriterion.forward
                                 forms it (both ground-truth components below 1000 in magnitude).  One ground-truth component is 2000 (``valid`` false there) and one pixel
                                 has magnitude 495 (valid, but past max_flow = 400): 958 of the 960 pixels count.
                             b   N = 2, coarse map 2 x 2 (fine 16 x 16), with ``valid=None``.
                           Per case:
                             flow          (T, N, 2, h, w) fp32      coarse flows, 4 * randn
                             mask          (T, N, 576, h, w) fp32    mask logits, 3 * randn
                             flow_gt       (N, 2, 8h, 8w)            2 * randn (+ the two planted pixels in a)
                             valid         (N, 8h, 8w) bool          (a only)
                             up_flow       (T, N, 2, 8h, 8w)         upsample_flow(flow[t], mask[t])
                             loss          ()                  sequence_loss's first result
                             metrics       (5,)                loss, epe, 1px, 3px, 5px (the Python floats the reference returns)
                             epe_per_iter  (T, pixels counted) compute_per_iter=True
                             grad_flow, grad_mask             d loss / d flow, d loss / d mask, shaped as the inputs

Arrays only.  Usage:  python tests/golden/make_golden_raft_criterion.py        (from the repo root)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as G  # noqa: E402

T = 3
METRICS = ("loss", "epe", "1px", "3px", "5px")
BIG, FAR = (0, 1, 7, 11), (0, slice(None), 20, 3)     # flow_gt[BIG] = 2000; flow_gt[FAR] = (297, -396): magnitude 495


def _case(R, C, N, h, w, with_valid):
    flow32, mask32 = (4 * torch.randn(T, N, 2, h, w)).float(), (3 * torch.randn(T, N, 576, h, w)).float()
    flow, mask = flow32.double().requires_grad_(), mask32.double().requires_grad_()
    flow_gt = 2 * torch.randn(N, 2, 8 * h, 8 * w, dtype=torch.float64)
    valid = None
    if with_valid:
        flow_gt[BIG] = 2000.0
        flow_gt[FAR] = torch.tensor([297.0, -396.0], dtype=torch.float64)
        valid = (flow_gt[:, 0].abs() < 1000) & (flow_gt[:, 1].abs() < 1000)      # RAFTCriterion.forward, use_valid=True
    this = types.SimpleNamespace(out_plane=2)
    outs = [{"up_flow": R.RAFTBase.upsample_flow(this, flow[t], mask[t])} for t in range(T)]
    loss, metrics, epe_per_iter = C.RAFTCriterion.sequence_loss(outs, flow_gt, valid, compute_per_iter=True)
    loss.backward()
    assert loss.dtype == torch.float64 and metrics["loss"] == loss.item() and len(epe_per_iter) == T
    case = dict(flow=flow32, mask=mask32, flow_gt=flow_gt, up_flow=torch.stack([o["up_flow"] for o in outs]), loss=loss,
                metrics=torch.tensor([metrics[k] for k in METRICS], dtype=torch.float64), epe_per_iter=torch.stack(epe_per_iter),
                grad_flow=flow.grad, grad_mask=mask.grad)
    if with_valid:
        case["valid"] = valid
        assert int(valid.sum()) == 959 and tuple(case["epe_per_iter"].shape) == (T, 958)
    else:
        assert tuple(case["epe_per_iter"].shape) == (T, N * 64 * h * w)
    return case


def main():
    if not os.path.isdir(G.REF):
        sys.exit("make_golden_raft_criterion.py needs the reference checkout (build container only)")
    G.load_reference()
    R = importlib.import_module("alonet.raft.raft")
    C = importlib.import_module("alonet.raft.criterion")
    torch.manual_seed(2100)
    arrays = {}
    for prefix, N, (h, w), with_valid in (("a_", 1, (3, 5), True), ("b_", 2, (2, 2), False)):
        for key, value in _case(R, C, N, h, w, with_valid).items():
            arrays[prefix + key] = value.detach().numpy().copy()
    path = os.path.join(OUT, "g21_raft_criterion.npz")
    np.savez_compressed(path, **arrays)
    print("wrote g21, bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
