"""alo_hip.upsample_flow (csrc/upsample_flow.hip) against the stock chain of ``RAFTBase.upsample_flow`` (softmax, unfold, multiply, sum,
permute + reshape), and ``RAFT.forward`` with ``ALO_RAFT_UPSAMPLE`` unset and ``fused``.

    python tools/upsample_bench.py [--rounds 3] [--launches 50] [--buffers 4] [--skip-model]

Kernel level, at (4, 2, 90, 160) (4 pairs of 1280 x 720, bench.py's config 3) and (1, 2, 55, 128): the two sides alternate `rounds`
times in one process; a round is `launches` calls, each between its own pair of device events with the next call already queued
behind it, and reports their median.  The calls of a round walk over `buffers` mask tensors, so that no call finds its mask in the
256 MiB Infinity Cache where the one before left it (in the model every mask is written once and read once).  Per side: the median
round and the spread (min - max) in ms, algorithmic bytes (mask + flow + out, each once) per ms, and that rate as a fraction of the
6.29 TB/s read stream.  `wins`: the kernel's slowest round is faster than the stock chain's fastest.

Model level: ``RAFT.forward(iters=12, only_last=False)`` on 4 pairs of 1280 x 720, knob off and on alternating, three timed runs each
after a warm-up of both; ms per pair batch.  One JSON line per measurement."""
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
from alonet.raft import RAFT  # noqa: E402
from alonet.raft.raft import RAFTBase  # noqa: E402

KNOB = "ALO_RAFT_UPSAMPLE"
READ_STREAM = 6.29e12   # bytes / s


def round_ms(fn, masks, launches):
    """Median duration (ms) of `launches` calls fn(mask), masks taken in turn, each timed by its own event pair."""
    events = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    torch.cuda.synchronize()
    events[0].record()
    for i in range(launches):
        fn(masks[i % len(masks)])
        events[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(events[i].elapsed_time(events[i + 1]) for i in range(launches))


def kernel_level(shape, with_mask, rounds, launches, buffers):
    n, c, h, w = shape
    flow = 4 * torch.randn(n, c, h, w, device="cuda")
    masks = [3 * torch.randn(n, 576, h, w, device="cuda") for _ in range(buffers)] if with_mask else [None]
    this = types.SimpleNamespace(out_plane=c)
    os.environ.pop(KNOB, None)
    sides = {"kernel": lambda m: alo_hip.upsample_flow(flow, m), "stock": lambda m: RAFTBase.upsample_flow(this, flow, m)}
    nbytes = 4.0 * (flow.numel() * 65 + (masks[0].numel() if with_mask else 0))
    row = {"level": "kernel", "mode": "convex" if with_mask else "bilinear", "shape": list(shape), "alg_bytes": nbytes}
    with torch.no_grad():
        got, want = sides["kernel"](masks[0]), sides["stock"](masks[0])
        row["max_diff"] = (got - want).abs().max().item()
        del got, want
        for fn in sides.values():
            for m in masks:
                fn(m)
        times = {k: [] for k in sides}
        for _ in range(rounds):
            for k, fn in sides.items():
                times[k].append(round_ms(fn, masks, launches))
    for k, v in times.items():
        med = statistics.median(v)
        row[k + "_ms"] = round(med, 4)
        row[k + "_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
        row[k + "_bytes_per_ms"] = round(nbytes / med)
        row[k + "_of_read_stream"] = round(nbytes / (med * 1e-3) / READ_STREAM, 3)
    row["kernel_over_stock"] = round(row["kernel_ms"] / row["stock_ms"], 3)
    row["wins"] = max(times["kernel"]) < min(times["stock"])
    print(json.dumps(row), flush=True)


def model_level(runs):
    torch.manual_seed(0)
    model = RAFT().eval().to("cuda")
    mk = lambda: aloscene.Frame(torch.rand(4, 3, 720, 1280, device="cuda") * 2 - 1, normalization="minmax_sym",  # noqa: E731
                                names=("B", "C", "H", "W"))
    f1, f2 = mk(), mk()

    def step(value):
        if value is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = value
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = model(f1, f2, iters=12, only_last=False)
        e.record()
        torch.cuda.synchronize()
        assert len(out) == 12 and all("up_flow" in o for o in out)
        return s.elapsed_time(e)

    with torch.no_grad():
        for value in (None, "fused"):
            step(value)
        times = {"off": [], "fused": []}
        for _ in range(runs):
            times["off"].append(step(None))
            times["fused"].append(step("fused"))
    os.environ.pop(KNOB, None)
    row = {"level": "model", "what": "RAFT.forward(iters=12, only_last=False), 4 pairs of 1280x720, ms per pair batch"}
    for k, v in times.items():
        row[k + "_ms"] = round(statistics.median(v), 2)
        row[k + "_runs_ms"] = [round(x, 2) for x in v]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upsample_bench: needs the GPU (a timing taken anywhere else says nothing)")
    torch.manual_seed(0)
    for shape in ((4, 2, 90, 160), (1, 2, 55, 128)):
        for with_mask in (True, False):
            kernel_level(shape, with_mask, args.rounds, max(args.launches, 50), args.buffers)
    if not args.skip_model:
        model_level(3)


if __name__ == "__main__":
    main()
