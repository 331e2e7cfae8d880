#!/usr/bin/env python
"""RAFT, 32 iterations, fp32, with each correlation block: pairs/s and peak device memory.

    python tools/raft_corr_blocks.py [--reps 3]

4 x 1280x720 pairs with CorrBlock and with AlternateCorrBlock; 1 x 3840x2160 with AlternateCorrBlock only (CorrBlock's volume
would take 89 GB there).  Random weights and frames: the time does not depend on them.  One JSON line per run.
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
from alonet.raft.corr import AlternateCorrBlock, CorrBlock  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for block, B, H, W in ((CorrBlock, 4, 720, 1280), (AlternateCorrBlock, 4, 720, 1280), (AlternateCorrBlock, 1, 2160, 3840)):
        print(json.dumps(run(block, B, H, W, a.reps)), flush=True)


if __name__ == "__main__":
    main()
