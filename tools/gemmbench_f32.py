"""alo_hip.linear_f32 / conv1x1_strided_f32 against what ``linear_auto`` / ``conv1x1_as_gemm`` launch for fp32 operands today
(hipBLASLt: ``torch.addmm`` / ``torch._addmm_activation``, a gathered copy first when strided, a separate pass for the identity),
layer by layer at the (M, K, N) of the fp32 headline: Deformable-DETR R50, batch 8 of 1333 x 800 — and alo_hip.conv3x3_f32 against
MIOpen + alo_hip.bias_act_ at the bottlenecks' 3x3 convolutions of the same step, and alo_hip.ffn_f32 against the two ``linear_auto``
launches of the transformer's feed-forward block on the split route.

    python tools/gemmbench_f32.py [--rounds 5] [--reps 20] [--only SUBSTRING]

tools/convbench_f32.py's protocol: per shape the two sides alternate `rounds` times in one process, each round timing `reps` calls
between device events after a warm-up of both; printed are the median round and the spread (min - max) in microseconds per call, the
ratio of the medians, max |difference| / max |value| of the two results, and whether the kernel's median is below the stock median
by more than both spreads (the rule a shape is routed by).  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aloception-oss_amd"))
import alo_hip  # noqa: E402
from alonet.detr.backbone import conv1x1_as_gemm  # noqa: E402

KNOB = "ALO_F32_LAYERS"
B = 8
P1, P2, P3, P4 = (200, 334), (100, 167), (50, 84), (25, 42)      # the backbone's maps at 1/4 .. 1/32 of 800 x 1333
S = P2[0] * P2[1] + P3[0] * P3[1] + P4[0] * P4[1] + 13 * 21      # pixels of the four-level pyramid
rows = lambda p: B * p[0] * p[1]  # noqa: E731
# name, M, K, N, ReLU, identity
LINEAR = [
    ("layer1.0.conv1", rows(P1), 64, 64, True, False),
    ("layer1.x.conv1", rows(P1), 256, 64, True, False),
    ("layer1.x.conv3", rows(P1), 64, 256, True, True),
    ("layer1.0.downsample", rows(P1), 64, 256, False, False),
    ("layer2.0.conv1", rows(P1), 256, 128, True, False),
    ("layer2.x.conv1", rows(P2), 512, 128, True, False),
    ("layer2.x.conv3", rows(P2), 128, 512, True, True),
    ("layer3.0.conv1", rows(P2), 512, 256, True, False),
    ("layer3.x.conv1", rows(P3), 1024, 256, True, False),
    ("layer3.x.conv3", rows(P3), 256, 1024, True, True),
    ("layer4.0.conv1", rows(P3), 1024, 512, True, False),
    ("layer4.x.conv1", rows(P4), 2048, 512, True, False),
    ("layer4.x.conv3", rows(P4), 512, 2048, True, True),
    ("input_proj.0", rows(P2), 512, 256, False, False),
    ("input_proj.1", rows(P3), 1024, 256, False, False),
    ("input_proj.2", rows(P4), 2048, 256, False, False),
    ("encoder 256 -> 256", B * S, 256, 256, False, False),
    ("encoder 256 -> 128", B * S, 256, 128, False, False),
    ("encoder 256 -> 384", B * S, 256, 384, False, False),
    ("encoder linear1", B * S, 256, 1024, True, False),
    ("encoder linear2", B * S, 1024, 256, False, False),
    ("decoder 256 -> 256", B * 300, 256, 256, False, False),
    ("decoder 256 -> 512", B * 300, 256, 512, False, False),
    ("decoder linear1", B * 300, 256, 1024, True, False),
    ("decoder linear2", B * 300, 1024, 256, False, False),
]
# name, (H, W) of the input map, Cin, Cout: the strided down-samples
STRIDED = [
    ("layer2.0.downsample", P1, 256, 512),
    ("layer3.0.downsample", P2, 512, 1024),
    ("layer4.0.downsample", P3, 1024, 2048),
]


# name, (H, W) of the input map, Cin = Cout, stride: the bottlenecks' conv2 (conv_bn: MIOpen without bias, then alo_hip.bias_act_)
CONV3X3 = [
    ("layer1.x.conv2", P1, 64, 1),
    ("layer2.0.conv2", P1, 128, 2),
    ("layer2.x.conv2", P2, 128, 1),
    ("layer3.0.conv2", P2, 256, 2),
    ("layer3.x.conv2", P3, 256, 1),
    ("layer4.0.conv2", P3, 512, 2),
    ("layer4.x.conv2", P4, 512, 1),
]


# name, M, F: the transformer's feed-forward blocks (d_model = 256), alo_hip.ffn_f32 against the two launches it replaces
FFN = [
    ("encoder ffn", B * S, 1024),
    ("decoder ffn", B * 300, 1024),
    ("ffn 8400 x 2048", rows(P4), 2048),
]


def time_us(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def with_knob(value, fn):
    def call():
        if value is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = value
        return fn()
    return call


def measure(row, sides, rounds, reps):
    with torch.no_grad():
        got, want = sides["kernel"](), sides["stock"]()
        row["max_diff_over_max"] = (got - want).abs().max().item() / want.abs().max().item()
        del got, want
        for fn in sides.values():   # warm-up: code objects, hipBLASLt's algorithm choice, the split weights
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(rounds):
            for k, fn in sides.items():
                times[k].append(time_us(fn, reps))
    for k, v in times.items():
        row[k + "_us"] = round(statistics.median(v), 1)
        row[k + "_spread_us"] = [round(min(v), 1), round(max(v), 1)]
    row["kernel_over_stock"] = round(row["kernel_us"] / row["stock_us"], 3)
    spreads = sum(max(v) - min(v) for v in times.values())
    row["wins"] = row["stock_us"] - row["kernel_us"] > spreads
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemmbench_f32: needs the GPU (a timing taken anywhere else says nothing)")
    torch.manual_seed(0)
    for name, m, k, n, relu, identity in LINEAR:
        if args.only not in name:
            continue
        x = torch.randn(m, k, device="cuda")
        w, b = torch.randn(n, k, device="cuda") / k ** 0.5, torch.randn(n, device="cuda")
        res = torch.randn(m, n, device="cuda") if identity else None
        sides = {"kernel": lambda: alo_hip.linear_f32(x, w, b, relu, residual=res),
                 "stock": with_knob(None, lambda: alo_hip.linear_auto(x, w, b, relu, residual=res))}
        measure({"layer": name, "M": m, "K": k, "N": n, "relu": relu, "identity": identity}, sides, args.rounds, args.reps)
        del x, w, b, res, sides
    for name, (h, w_), cin, cout in STRIDED:
        if args.only not in name:
            continue
        x = torch.randn(B, cin, h, w_, device="cuda").contiguous(memory_format=torch.channels_last)
        w, b = torch.randn(cout, cin, 1, 1, device="cuda") / cin ** 0.5, torch.randn(cout, device="cuda")
        w2 = w.view(cout, cin)      # one object: the split copy rides on it
        sides = {"kernel": lambda: alo_hip.conv1x1_strided_f32(x, w2, b, 2),
                 "stock": with_knob(None, lambda: conv1x1_as_gemm(x, w, b, (2, 2)))}
        measure({"layer": name, "map": [B, cin, h, w_], "Cout": cout, "stride": 2}, sides, args.rounds, args.reps)
        del x, w, w2, b, sides
    for name, (h, w_), c, stride in CONV3X3:
        if args.only not in name:
            continue
        x = torch.randn(B, c, h, w_, device="cuda").contiguous(memory_format=torch.channels_last)
        w = (torch.randn(c, c, 3, 3, device="cuda") / (9 * c) ** 0.5).contiguous(memory_format=torch.channels_last)
        b = torch.randn(c, device="cuda")
        sides = {"kernel": lambda: alo_hip.conv3x3_f32(x, w, b, relu=True, stride=stride),
                 "stock": lambda: alo_hip.bias_act_(F.conv2d(x, w, None, stride, 1), b, None, True)}
        measure({"layer": name, "map": [B, c, h, w_], "Cout": c, "stride": stride}, sides, args.rounds, args.reps)
        del x, w, b, sides
    for name, m, f in FFN:
        if args.only not in name:
            continue
        x = torch.randn(m, 256, device="cuda")
        w1, b1 = torch.randn(f, 256, device="cuda") / 16, torch.randn(f, device="cuda")
        w2, b2 = torch.randn(256, f, device="cuda") / f ** 0.5, torch.randn(256, device="cuda")
        # stock: what _ffn launches without the kernel on the split route, linear_auto twice (each half on whichever of linear_f32 and
        # hipBLASLt it is routed to at this shape)
        sides = {"kernel": lambda: alo_hip.ffn_f32(x, w1, b1, w2, b2),
                 "stock": with_knob("split", lambda: alo_hip.linear_auto(alo_hip.linear_auto(x, w1, b1, relu=True), w2, b2))}
        measure({"layer": name, "M": m, "F": f}, sides, args.rounds, args.reps)
        del x, w1, b1, w2, b2, sides
    os.environ.pop(KNOB, None)


if __name__ == "__main__":
    main()
