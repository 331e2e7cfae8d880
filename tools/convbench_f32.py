"""alo_hip.conv3x3_f32 against MIOpen's fp32 F.conv2d, layer by layer: the six 3x3 convolutions of RAFT's update block at B = 4,
90 x 160 (720p / 8) and the 64- and 128-channel stride-1 shapes of RAFT's encoders.

    python tools/convbench_f32.py [--rounds 5] [--reps 20] [--only conv3x3|gru|dilated]

Per shape the two sides alternate `rounds` times in one process (same box, same minute), each round timing `reps` calls between
device events after a warm-up of every shape; printed are the median round and the spread (min - max) in microseconds per call.
The kernel's side is the whole C call: magnitude pre-pass + convolution with bias and ReLU, channels-last in and out.  MIOpen's side
is what the stock route launches: F.conv2d without bias on NCHW, then alo_hip.bias_act_nchw_ (shown with and without that pass).
--only gru (or no --only): also the four five-tap launches of SepConvGRU per iteration at the same size, alo_hip.conv_taps_f32 +
the channels-last gate pass against what the fused route launches in their place (F.conv2d without bias on NCHW + the planar gate
pass), each shown with and without its gate pass.
--only dilated (or no --only): also the dilated 3x3 of a DC5 backbone (layer4.1 / layer4.2 conv2: 512 -> 512, dilation 2, padding 2, at
1/16 of 800 x 1333) at batch 8 and batch 1, alo_hip.conv3x3_f32(..., dilation=2) against the stock route of
alonet.detr.backbone.conv_bn: F.conv2d on channels-last + alo_hip.bias_act_.
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


# SepConvGRU (alonet/raft/update.py): name, kernel size, Cout, the gate pass behind it ("gate": [z | r] -> z, r*h; "update": q -> h', + net)
GRU_LAUNCHES = [
    ("gru.convz1+convr1 (1x5)", (1, 5), 256, "gate"),
    ("gru.convq1 (1x5)", (1, 5), 128, "update"),
    ("gru.convz2+convr2 (5x1)", (5, 1), 256, "gate"),
    ("gru.convq2 (5x1)", (5, 1), 128, "update+net"),
]
GRU_SHAPE, GRU_C = (4, 384, 90, 160), 128


def time_us(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def measure(sides, rounds, reps):
    """Warm every side up, then alternate them `rounds` times -> {side: [us per call, ...]}"""
    for fn in sides.values():   # warm-up: code objects, MIOpen's solver choice, the split weights
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(time_us(fn, reps))
    return times


def report(row, times):
    for k, v in times.items():
        row[k + "_us"] = round(statistics.median(v), 1)
        row[k + "_spread_us"] = [round(min(v), 1), round(max(v), 1)]
    return row


def gru_launches(rounds, reps):
    n, ct, h, w = GRU_SHAPE
    c, rows = GRU_C, n * h * w
    as_rows = lambda t: t.permute(0, 2, 3, 1).view(rows, t.shape[1])   # noqa: E731
    for name, ksize, cout, glue in GRU_LAUNCHES:
        pad = (ksize[0] // 2, ksize[1] // 2)
        hx = torch.randn(n, ct, h, w, device="cuda")
        hx[:, :c].tanh_()
        rhx = hx.clone()
        hx_cl, rhx_cl = hx.contiguous(memory_format=torch.channels_last), rhx.contiguous(memory_format=torch.channels_last)
        wt = torch.randn(cout, ct, *ksize, device="cuda") / (5 * ct) ** 0.5
        b = torch.randn(cout, device="cuda")
        zr, zr_cl = torch.randn(n, 2 * c, h, w, device="cuda"), torch.randn(n, 2 * c, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
        net = torch.empty(n, c, h, w, device="cuda") if glue == "update+net" else None
        net_cl = None if net is None else as_rows(net.contiguous(memory_format=torch.channels_last))
        if glue == "gate":
            glue_cl = lambda y: alo_hip.gru_gate_rows_(as_rows(y), b, as_rows(hx_cl), as_rows(rhx_cl), c)   # noqa: E731
            glue_planar = lambda y: alo_hip.gru_gate_(y, b, hx, rhx, c)                                       # noqa: E731
        else:
            glue_cl = lambda y: alo_hip.gru_update_rows_(as_rows(y), b, as_rows(zr_cl), as_rows(hx_cl), c, net_cl)   # noqa: E731
            glue_planar = lambda y: alo_hip.gru_update_(y, b, zr, hx, c, net)                                          # noqa: E731
        sides = {
            "kernel": lambda: alo_hip.conv_taps_f32(hx_cl, wt),
            "kernel+gate": lambda: glue_cl(alo_hip.conv_taps_f32(hx_cl, wt)),
            "miopen": lambda: F.conv2d(hx, wt, None, 1, pad),
            "miopen+gate": lambda: glue_planar(F.conv2d(hx, wt, None, 1, pad)),
        }
        with torch.no_grad():
            got, want = sides["kernel"](), sides["miopen"]()
            err = (got - want).abs().max().item() / want.abs().max().item()
            times = measure(sides, rounds, reps)
        row = report({"layer": name, "shape": [n, ct, h, w], "cout": cout, "glue": glue, "max_diff_over_max": err}, times)
        row["kernel_tflops_fp32_equivalent"] = round(2.0 * 5 * ct * rows * cout / row["kernel_us"] / 1e6, 1)
        print(json.dumps(row), flush=True)


DILATED = [("DC5 layer4.x.conv2 (d=2)", (8, 512, 50, 84), 512), ("DC5 layer4.x.conv2 (d=2), batch 1", (1, 512, 50, 84), 512)]


def dilated_layers(rounds, reps):
    for name, (n, cin, h, w), cout in DILATED:
        x = torch.randn(n, cin, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cout, cin, 3, 3, device="cuda") / (9 * cin) ** 0.5).contiguous(memory_format=torch.channels_last)
        b = torch.randn(cout, device="cuda")
        sides = {
            "kernel": lambda: alo_hip.conv3x3_f32(x, wt, b, relu=True, dilation=2),
            "miopen": lambda: F.conv2d(x, wt, None, 1, 2, 2),
            "miopen+bias_act": lambda: alo_hip.bias_act_(F.conv2d(x, wt, None, 1, 2, 2), b, None, True),
        }
        got, want = sides["kernel"](), sides["miopen+bias_act"]()
        err = (got - want).abs().max().item() / want.abs().max().item()
        times = measure(sides, rounds, reps)
        row = report({"layer": name, "shape": [n, cin, h, w], "cout": cout, "max_diff_over_max": err}, times)
        row["kernel_tflops_fp32_equivalent"] = round(2.0 * 9 * cin * n * h * w * cout / row["kernel_us"] / 1e6, 1)
        row["kernel_over_stock"] = round(row["kernel_us"] / row["miopen+bias_act_us"], 3)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["conv3x3", "gru", "dilated"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convbench_f32: needs the GPU (a timing taken anywhere else says nothing)")
    torch.manual_seed(0)
    for name, (n, cin, h, w), cout in LAYERS if args.only in (None, "conv3x3") else []:
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
            times = measure(sides, args.rounds, args.reps)
        row = report({"layer": name, "shape": [n, cin, h, w], "cout": cout, "cout_run": pad, "max_diff_over_max": err}, times)
        flops = 2.0 * 9 * cin * n * h * w * pad
        row["kernel_tflops_fp32_equivalent"] = round(flops / row["kernel_us"] / 1e6, 1)
        print(json.dumps(row), flush=True)
    if args.only in (None, "gru"):
        with torch.no_grad():
            gru_launches(args.rounds, args.reps)
    if args.only in (None, "dilated"):
        with torch.no_grad():
            dilated_layers(args.rounds, args.reps)


if __name__ == "__main__":
    main()
