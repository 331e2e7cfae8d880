#!/usr/bin/env python
"""RAFT, 32 iterations, fp32, with each correlation block: pairs/s and peak device memory.

    python tools/raft_corr_blocks.py [--reps 3]
    python tools/raft_corr_blocks.py --train [--reps 2] [--large 2160x3840]

4 x 1280x720 pairs with CorrBlock and with AlternateCorrBlock; 1 x 3840x2160 with AlternateCorrBlock only (CorrBlock's volume
would take 89 GB there).  Random weights and frames: the time does not depend on them.  One JSON line per run.

``--train``: one training step instead (forward at 12 iterations, ``RAFTCriterion.sequence_loss``, backward; the blocks that can be
trained through): 1 x 1280x720 with CorrBlock and with TrainableAlternateCorrBlock, then ``--large`` with both, CorrBlock's row
reporting the error it ends with where its volume and gradient maps no longer fit.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aloception-oss_amd"))
import aloscene  # noqa: E402
from alonet.raft import RAFT  # noqa: E402
from alonet.raft import RAFTCriterion  # noqa: E402
from alonet.raft.corr import AlternateCorrBlock, CorrBlock, TrainableAlternateCorrBlock  # noqa: E402

DEV = "cuda:0"


def run(block, B, H, W, reps, iters=32):
    torch.manual_seed(0)
    model = RAFT(corr_block=block).eval().to(DEV)
    mk = lambda: aloscene.Frame(torch.rand(B, 3, H, W) * 2 - 1, normalization="minmax_sym",  # noqa: E731
                                names=("B", "C", "H", "W")).to(DEV)
    f1, f2 = mk(), mk()
    with torch.no_grad():
        model(f1, f2, iters=iters, only_last=True)   # warm-up: kernels loaded, allocator populated
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = model(f1, f2, iters=iters, only_last=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
    assert torch.isfinite(out[-1]["up_flow"]).all()
    res = dict(block=block.__name__, pairs=B, H=H, W=W, iters=iters, ms_per_forward=dt * 1e3, pairs_per_s=B / dt,
               max_memory_allocated_GB=torch.cuda.max_memory_allocated() / 1e9)
    del model, f1, f2, out
    torch.cuda.empty_cache()
    return res


def train_step(block, B, H, W, reps, iters=12):
    torch.manual_seed(0)
    model = RAFT(corr_block=block).to(DEV).train()
    model.freeze_bn()
    mk = lambda: aloscene.Frame(torch.rand(B, 3, H, W) * 2 - 1, normalization="minmax_sym",  # noqa: E731
                                names=("B", "C", "H", "W")).to(DEV)
    f1, f2 = mk(), mk()
    flow_gt = torch.randn(B, 2, H, W, device=DEV) * 5
    res = dict(block=block.__name__, mode="train", pairs=B, H=H, W=W, iters=iters)

    def step():
        model.zero_grad(set_to_none=True)
        loss, _, _ = RAFTCriterion.sequence_loss(model(f1, f2, iters=iters), flow_gt)
        loss.backward()
        return loss

    try:
        step()   # warm-up: kernels loaded, allocator populated
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(reps):
            loss = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        grad = model.fnet.conv1.weight.grad
        assert torch.isfinite(loss) and grad is not None and torch.isfinite(grad).all() and grad.abs().max().item() > 0
        res.update(ms_per_step=dt * 1e3, max_memory_allocated_GB=torch.cuda.max_memory_allocated() / 1e9)
    except (torch.OutOfMemoryError, RuntimeError) as e:   # the volume does not fit, or alo_corr_build refuses the grid
        res.update(error=str(e).splitlines()[0][:200])
    del model, f1, f2, flow_gt
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--train", action="store_true", help="one training step per block instead of the inference runs")
    ap.add_argument("--large", default="2160x3840", help="--train: the size beyond 1280x720, HxW")
    a = ap.parse_args()
    if a.train:
        LH, LW = (int(v) for v in a.large.split("x"))
        for block, H, W in ((CorrBlock, 720, 1280), (TrainableAlternateCorrBlock, 720, 1280), (CorrBlock, LH, LW),
                            (TrainableAlternateCorrBlock, LH, LW)):
            print(json.dumps(train_step(block, 1, H, W, a.reps)), flush=True)
        return
    for block, B, H, W in ((CorrBlock, 4, 720, 1280), (AlternateCorrBlock, 4, 720, 1280), (AlternateCorrBlock, 1, 2160, 3840)):
        print(json.dumps(run(block, B, H, W, a.reps)), flush=True)


if __name__ == "__main__":
    main()
