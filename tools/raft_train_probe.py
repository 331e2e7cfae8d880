"""One RAFT training step with ``ALO_RAFT_UPSAMPLE`` unset and ``train``, and the up-sampling's forward + backward alone.

    python tools/raft_train_probe.py [--batch 6] [--height 368] [--width 496] [--iters 12] [--runs 5] [--rounds 3] [--launches 20]
                                     [--skip-model] [--skip-kernel]

Up-sampling alone, at (4, 2, 90, 160) (4 pairs of 1280 x 720) and (6, 2, 46, 62) (a 368 x 496 crop at batch 6): forward + backward
(``up.backward(grad_up)`` with a dense ``grad_up``) of the stock chain under autograd against ``alo_hip.upsample_flow_autograd``
(one forward launch; one backward launch behind a packing copy, and an ``F.fold``).  The two sides alternate `rounds` times in one
process; a round is `launches` forward + backward pairs, each between its own pair of device events, and reports their median; the
pairs of a round walk over 4 mask tensors so that none is found in the Infinity Cache.  Per side: median round, spread (min - max) and
the peak memory of one pair above what is allocated before it.  `wins`: the new route's slowest round beats the stock chain's fastest.

Training step: ``RAFT`` in train mode (HIP ``CorrBlock``), `iters` iterations, ``RAFTCriterion.sequence_loss`` on every iteration's
``up_flow``, ``backward()``; no optimizer.  Knob unset and ``train`` alternate `runs` times after a warm-up of both; ms per step
(median, all runs) and ``max_memory_allocated`` of a step.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aloception-oss_amd"))
import alo_hip  # noqa: E402
import aloscene  # noqa: E402
from alonet.raft import RAFT, RAFTCriterion  # noqa: E402
from alonet.raft.raft import RAFTBase  # noqa: E402

KNOB = "ALO_RAFT_UPSAMPLE"


def _set_knob(value):
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value


def round_ms(fn, masks, launches):
    events = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    torch.cuda.synchronize()
    events[0].record()
    for i in range(launches):
        fn(masks[i % len(masks)])
        events[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(events[i].elapsed_time(events[i + 1]) for i in range(launches))


def kernel_level(shape, rounds, launches, buffers=4):
    n, c, h, w = shape
    flow = (4 * torch.randn(n, c, h, w, device="cuda")).requires_grad_()
    masks = [(3 * torch.randn(n, 576, h, w, device="cuda")).requires_grad_() for _ in range(buffers)]
    grad_up = torch.randn(n, c, 8 * h, 8 * w, device="cuda")
    this = types.SimpleNamespace(out_plane=c)
    _set_knob(None)

    def pair(forward):
        def run(mask):
            flow.grad = mask.grad = None
            forward(mask).backward(grad_up)
        return run

    sides = {"stock": pair(lambda m: RAFTBase.upsample_flow(this, flow, m)), "train": pair(lambda m: alo_hip.upsample_flow_autograd(flow, m))}
    row = {"level": "upsampling forward + backward", "shape": list(shape), "mask_bytes": 4 * masks[0].numel()}
    grads = {}
    for k, fn in sides.items():
        fn(masks[0])
        grads[k] = (flow.grad.clone(), masks[0].grad.clone())
    row["max_diff_grad_flow"] = (grads["stock"][0] - grads["train"][0]).abs().max().item()
    row["max_diff_grad_mask"] = (grads["stock"][1] - grads["train"][1]).abs().max().item()
    del grads
    times, peaks = {k: [] for k in sides}, {}
    for k, fn in sides.items():
        for m in masks:
            fn(m)
        flow.grad = None
        for m in masks:
            m.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(masks[0])
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated() - base
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(round_ms(fn, masks, launches))
    for k, v in times.items():
        row[k + "_ms"] = round(statistics.median(v), 4)
        row[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
        row[k + "_peak_bytes"] = peaks[k]
    row["train_over_stock"] = round(row["train_ms"] / row["stock_ms"], 3)
    row["wins"] = max(times["train"]) < min(times["stock"])
    print(json.dumps(row), flush=True)


def model_level(batch, height, width, iters, runs):
    torch.manual_seed(0)
    model = RAFT().train().to("cuda")
    mk = lambda: aloscene.Frame(torch.rand(batch, 3, height, width, device="cuda") * 2 - 1, normalization="minmax_sym",  # noqa: E731
                                names=("B", "C", "H", "W"))
    f1, f2 = mk(), mk()
    flow_gt = 5 * torch.randn(batch, 2, height, width, device="cuda")
    valid = torch.ones(batch, height, width, device="cuda")

    def step(value):
        _set_knob(value)
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = model(f1, f2, iters=iters)
        loss, metrics, _ = RAFTCriterion.sequence_loss(out, flow_gt, valid)
        loss.backward()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), torch.cuda.max_memory_allocated(), metrics["loss"]

    for value in (None, "train"):
        step(value)
    times, peak, loss = {"off": [], "train": []}, {}, {}
    for _ in range(runs):
        for name, value in (("off", None), ("train", "train")):
            ms, peak[name], loss[name] = step(value)
            times[name].append(ms)
    _set_knob(None)
    row = {"level": "training step", "what": f"RAFT train step, {iters} iterations, batch {batch} of {height}x{width}, sequence loss, ms per step"}
    for k, v in times.items():
        row[k + "_ms"] = round(statistics.median(v), 2)
        row[k + "_runs_ms"] = [round(x, 2) for x in v]
        row[k + "_max_memory_allocated"] = peak[k]
        row[k + "_loss"] = loss[k]
    row["wins"] = max(times["train"]) < min(times["off"])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=368)
    ap.add_argument("--width", type=int, default=496)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raft_train_probe: needs the GPU (a timing taken anywhere else says nothing)")
    torch.manual_seed(0)
    if not args.skip_kernel:
        for shape in ((4, 2, 90, 160), (6, 2, 46, 62)):
            kernel_level(shape, args.rounds, args.launches)
    if not args.skip_model:
        model_level(args.batch, args.height, args.width, args.iters, args.runs)


if __name__ == "__main__":
    main()
