#!/usr/bin/env python
"""DeformableDETR-R50 in fp16 on the bench batch: frames/s and which launches of this library the model makes.

    python tools/f16_model_probe.py [--batch 8] [--steps 10] [--warmup 3] [--dtypes f16,bf16]

In fp16 the transformer runs on this library's kernels as it does in bf16 (attention op, short-K linears, the one-kernel FFN,
residual + LayerNorm, positional encoding), except that its encoder takes the separate launches instead of the bf16-only fused
encoder block; the backbone and the input projections are gated on fp32 / bf16 and leave fp16 to the stock ops, so the frame rate
stays below the bf16 headline by construction.  The launch tags (``alo_hip.LaunchTimer``) say which library kernels ran; what is
absent from the fp16 list next to the bf16 one is what runs on stock ops or on separate launches, and the per-step gap is the case
for giving the backbone kernels and the encoder block fp16 next.  Prints one JSON line per dtype.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aloception-oss_amd"))
import alo_hip  # noqa: E402
import bench  # noqa: E402

DTYPES = dict(f16=torch.float16, bf16=torch.bfloat16, f32=torch.float32)


def probe(name, batch, steps, warmup, device="cuda:0"):
    dtype = DTYPES[name]
    model = bench.build_detector(device, dtype)
    frames = bench.detection_inputs(batch, 0, device, dtype)

    def step():
        with torch.no_grad():
            return model.inference(model(frames))

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    with alo_hip.LaunchTimer() as timer:   # one extra, un-timed step with an event pair around every launch of the library
        step()
    tags = {tag: dict(launches=d["calls"], ms_total=round(d["ms_total"], 3)) for tag, d in sorted(timer.summary().items())}
    del model, frames
    torch.cuda.empty_cache()
    return dict(dtype=name, batch=batch, steps=steps, launch="eager", frames_per_s=round(batch * steps / seconds, 2),
                ms_per_step=round(seconds / steps * 1e3, 2), library_ms_per_step=round(sum(t["ms_total"] for t in tags.values()), 2),
                launch_tags=tags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f16,bf16")
    a = ap.parse_args()
    for name in a.dtypes.split(","):
        print(json.dumps(probe(name, a.batch, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
