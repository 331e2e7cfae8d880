"""Correctness + timing of alo_hip.conv3x3 against MIOpen on the ResNet-50 bottleneck shapes (B=8, 640x640 -> padded 667).

    python tools/convbench.py [--dilated]

--dilated: only the dilated 3x3 of a DC5 backbone (layer4.1 / layer4.2 conv2: 512 -> 512, dilation 2, padding 2, at 1/16 of 800 x 1333)
at batch 8 and batch 1: alo_hip.conv3x3(..., dilation=2) against the stock route of alonet.detr.backbone.conv_bn, F.conv2d on
channels-last + alo_hip.bias_act_.  The two sides alternate in one process, warm, 21 rounds of 10 calls between device events each;
printed are the median round and the spread (min - max) in microseconds per call, one JSON line per shape.  Without the flag the
dilated shapes follow the others."""
import json, os, statistics, sys, torch
import torch.nn.functional as F
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aloception-oss_amd"))
import alo_hip

def timeit(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3

def dilated(rounds=21, reps=10):
    for n, c, h, w in ((8, 512, 50, 84), (1, 512, 50, 84)):
        x = torch.randn(n, c, h, w, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(c, c, 3, 3, device="cuda") * (1.0 / (9 * c) ** 0.5)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        b = torch.randn(c, device="cuda", dtype=torch.bfloat16)
        sides = {"kernel": lambda: alo_hip.conv3x3(x, wt, b, relu=True, dilation=2),
                 "miopen": lambda: F.conv2d(x, wt, None, 1, 2, 2),
                 "miopen+bias_act": lambda: alo_hip.bias_act_(F.conv2d(x, wt, None, 1, 2, 2), b, None, True)}
        with torch.no_grad():
            ref = F.relu(F.conv2d(x.float(), wt.float(), b.float(), 1, 2, 2))
            err = {k: (sides[k]().float() - ref).abs().max().item() for k in ("kernel", "miopen+bias_act")}
            for fn in sides.values():
                timeit(fn, 3)
            times = {k: [] for k in sides}
            for _ in range(rounds):
                for k, fn in sides.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(reps): fn()
                    e.record(); torch.cuda.synchronize()
                    times[k].append(s.elapsed_time(e) / reps * 1e3)
        row = {"layer": "DC5 layer4.x.conv2 (d=2)", "shape": [n, c, h, w], "cout": c, "max_err_vs_fp32": err}
        for k, v in times.items():
            row[k + "_us"] = round(statistics.median(v), 1)
            row[k + "_spread_us"] = [round(min(v), 1), round(max(v), 1)]
        row["kernel_tflops"] = round(2.0 * 9 * c * c * n * h * w / row["kernel_us"] / 1e6, 1)
        row["kernel_over_stock"] = round(row["kernel_us"] / row["miopen+bias_act_us"], 3)
        print(json.dumps(row), flush=True)

torch.manual_seed(0)
if "--dilated" in sys.argv[1:]:
    dilated()
    sys.exit(0)
shapes = [(8, 64, 200, 334), (8, 128, 100, 167), (8, 256, 50, 84), (8, 512, 25, 42), (2, 128, 7, 9), (1, 256, 5, 70)]
import itertools
cases = [(s, 1, None) for s in shapes] + [((8, 128, 200, 334), 2, None), ((8, 256, 100, 167), 2, None), ((8, 512, 50, 84), 2, None), ((8, 2048, 25, 42), 2, 256), ((2, 1024, 9, 12), 1, 128), ((2, 128, 9, 11), 2, None), ((1, 64, 8, 8), 2, None)]
for (n, c, h, w), st, co in cases:
    x = torch.randn(n, c, h, w, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(co or c, c, 3, 3, device="cuda") * (1.0 / (9 * c) ** 0.5)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(co or c, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        ref = F.relu(F.conv2d(x.float(), wt.float(), b.float(), st, 1))
        got = alo_hip.conv3x3(x, wt, b, relu=True, stride=st)
        stock = F.relu(F.conv2d(x, wt, b, st, 1))
        err = (got.float() - ref).abs().max().item()
        err_stock = (stock.float() - ref).abs().max().item()
        t_mine = timeit(lambda: alo_hip.conv3x3(x, wt, b, relu=True, stride=st))
        t_stock = timeit(lambda: F.conv2d(x, wt, None, st, 1))
    gf = 2.0 * 9 * c * got.numel()
    print(f"{(n,c,h,w)} s{st}: err {err:.4f} (stock {err_stock:.4f})  mine {t_mine:.1f} us ({gf/t_mine/1e6:.0f} TF/s)  miopen {t_stock:.1f} us", flush=True)

# ---- the stem: conv7x7/s2 + bias + relu + maxpool3x3/s2 -------------------------------------------------------------------
x = torch.randn(8, 3, 800, 1333, device="cuda").to(torch.bfloat16)
wt = (torch.randn(64, 3, 7, 7, device="cuda") / 147 ** 0.5).to(torch.bfloat16)
b = torch.randn(64, device="cuda").to(torch.bfloat16)
with torch.no_grad():
    ref = F.max_pool2d(F.relu(F.conv2d(x[:1].float(), wt.float(), b.float(), 2, 3)), 3, 2, 1)
    got = alo_hip.stem_conv_pool(x, wt, b)
    print("stem err", (got[:1].float() - ref).abs().max().item(), flush=True)
    t_mine = timeit(lambda: alo_hip.stem_conv_pool(x, wt, b))
    xl = x.contiguous(memory_format=torch.channels_last); wl = wt.contiguous(memory_format=torch.channels_last)
    t_stock = timeit(lambda: F.max_pool2d(F.relu_(F.conv2d(xl, wl, b, 2, 3)), 3, 2, 1))
print(f"stem: mine {t_mine:.1f} us  stock (conv+relu+pool, channels_last) {t_stock:.1f} us")
dilated()
