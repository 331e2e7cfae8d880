"""alo_hip.conv3x3_f32 against MIOpen's fp32 F.conv2d, layer by layer: the six 3x3 convolutions of RAFT's update block at B = 4,
90 x 160 (720p / 8) and the 64- and 128-channel stride-1 shapes of RAFT's encoders.

    python tools/convbench_f32.py [--rounds 5] [--reps 20]

Per shape the two sides alternate `rounds` times in one process (same box, same minute), each round timing `reps` calls between
device events after a warm-up of every shape; printed are the median round and the spread (min - max) in microseconds per call.
The kernel's side is the whole C call: magnitude pre-pass + convolution with bias and ReLU, channels-last in and out.  MIOpen's side
is what the stock route launches: F.conv2d without bias on NCHW, then alo_hip.bias_act_nchw_ (shown with and without that pass).
One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aloception-oss_amd"))
import alo_hip  # noqa: E402

# name, (N, Cin, H, W), Cout as the layer has it (the kernel runs it padded to a multiple of 64)
LAYERS = [
    ("encoder.convc2", (4, 256, 90, 160), 192),
    ("encoder.convf2", (4, 128, 90, 160), 64),
    ("encoder.conv", (4, 256, 90, 160), 126),
    ("flow_head.conv1", (4, 128, 90, 160), 256),
    ("flow_head.conv2", (4, 256, 90, 160), 2),
    ("mask.0", (4, 128, 90, 160), 256),
    ("fnet 64 @ 1/2", (4, 64, 360, 640), 64),
    ("fnet 128 @ 1/8", (4, 128, 90, 160), 128),
]


def time_us(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convbench_f32: needs the GPU (a timing taken anywhere else says nothing)")
    torch.manual_seed(0)
    for name, (n, cin, h, w), cout in LAYERS:
        pad = (cout + 63) // 64 * 64
        x = torch.randn(n, cin, h, w, device="cuda")
        x_cl = x.contiguous(memory_format=torch.channels_last)
        wt = torch.randn(cout, cin, 3, 3, device="cuda") / (9 * cin) ** 0.5
        b = torch.randn(cout, device="cuda")
        wt_pad, b_pad = F.pad(wt, (0, 0, 0, 0, 0, 0, 0, pad - cout)).contiguous(), F.pad(b, (0, pad - cout)).contiguous()
        sides = {
            "kernel": lambda: alo_hip.conv3x3_f32(x_cl, wt_pad, b_pad, relu=True),
            "miopen": lambda: F.conv2d(x, wt, None, 1, 1),
            "miopen+bias_act": lambda: alo_hip.bias_act_nchw_(F.conv2d(x, wt, None, 1, 1), b, True),
        }
        with torch.no_grad():
            got = sides["kernel"]()[:, :cout]
            want = sides["miopen+bias_act"]()
            err = (got - want).abs().max().item() / want.abs().max().item()
            for fn in sides.values():   # warm-up: code objects, MIOpen's solver choice, the split weights
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    times[k].append(time_us(fn, args.reps))
        row = {"layer": name, "shape": [n, cin, h, w], "cout": cout, "cout_run": pad, "max_diff_over_max": err}
        for k, v in times.items():
            row[k + "_us"] = round(statistics.median(v), 1)
            row[k + "_spread_us"] = [round(min(v), 1), round(max(v), 1)]
        flops = 2.0 * 9 * cin * n * h * w * pad
        row["kernel_tflops_fp32_equivalent"] = round(flops / row["kernel_us"] / 1e6, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
