"""``alo_hip.attention`` against the stock op it replaces, and the two detectors' inference steps with ``ALO_ATTENTION=fused`` on
and off, in one process.

    python tools/attnbench.py [--reps 5] [--window 0.2] [--batch 2] [--frame 800x1333] [--no-models]

Kernel legs: ``fused`` is ``alo_hip.attention`` on the batch-first tensors as the projections write them; ``stock`` is what
``_attend`` does without the switch: ``scaled_dot_product_attention`` between the two head-major transposes (the transposes are part
of what the kernel replaces), with the padding mask as a boolean ``attn_mask`` where the shape has one.  Both are warmed up; a sample
is one window of back-to-back calls between two device events, sized to last at least ``--window`` seconds; the legs alternate
window by window.  Printed: microseconds per call, median (min - max) over ``--reps`` windows.

Model legs: one inference step of ``DetrR50`` and of ``DeformableDetrR50`` in bf16 on a padded batch, the switch set per window.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aloception-oss_amd"))
import alo_hip  # noqa: E402

DEV = "cuda:0"
# (B, Lq, Lk, masked): a stride-32 map of 1333 x 800 frames is 42 x 25 = 1050 tokens (DETR's encoder, masked as a padded batch is);
# DETR's cross-attention (100 queries); the Deformable-DETR and DETR decoders' self-attention (300 / 100 queries)
SHAPES = [(8, 1050, 1050, True), (8, 100, 1050, True), (8, 300, 300, False), (8, 100, 100, False)]
FRAME_SIZES = [(800, 1333), (800, 1201), (704, 1333), (800, 1066), (640, 1333), (800, 1333), (736, 1103), (800, 960)]


def frame_mask(batch, h=25, w=42):
    """(B, h * w) bool: what batch_list's padding of FRAME_SIZES to 800 x 1333 becomes on the stride-32 map."""
    m = torch.ones(batch, h, w, dtype=torch.bool)
    for b in range(batch):
        fh, fw = FRAME_SIZES[b % len(FRAME_SIZES)]
        m[b, : -(-fh // 32), : -(-fw // 32)] = False
    return m.flatten(1).to(DEV)


def stock_attention(q, k, v, mask):
    B, Lq, E = q.shape
    heads = lambda t: t.reshape(B, t.shape[1], 8, E // 8).transpose(1, 2)
    keep = None if mask is None else ~mask[:, None, None, :]
    return F.scaled_dot_product_attention(heads(q), heads(k), heads(v), attn_mask=keep).transpose(1, 2).reshape(B, Lq, E)


def window(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3   # seconds


def alternate(legs, reps, seconds, setup=None):
    """{name: fn} -> {name: [seconds per call, one per window]}; ``setup(name)`` runs before each window of a leg."""
    counts = {}
    for name, fn in legs.items():
        if setup:
            setup(name)
        window(fn, 3)                                                  # warm-up: library load, packs, the allocator
        per_call = window(fn, 10) / 10
        counts[name] = max(10, int(seconds / per_call) + 1)
    samples = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            if setup:
                setup(name)
            samples[name].append(window(fn, counts[name]) / counts[name])
    return samples, counts


def show(label, samples, counts, unit=1e6, suffix="us"):
    for name, v in samples.items():
        v = [x * unit for x in v]
        print(f"{label:34s} {name:6s} {statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f}) {suffix}  x{counts[name]} per window", flush=True)


def kernels(args):
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for B, Lq, Lk, masked in SHAPES:
            gen = torch.Generator().manual_seed(Lq + Lk)
            q = torch.randn(B, Lq, 256, generator=gen).to(DEV, dtype)
            k, v = (torch.randn(B, Lk, 256, generator=gen).to(DEV, dtype) for _ in range(2))
            mask = frame_mask(B) if masked else None
            legs = {"fused": lambda: alo_hip.attention(q, k, v, mask), "stock": lambda: stock_attention(q, k, v, mask)}
            diff = (legs["fused"]().float() - legs["stock"]().float()).abs().max().item()
            samples, counts = alternate(legs, args.reps, args.window)
            show(f"{str(dtype)[6:]:8s} B={B} Lq={Lq} Lk={Lk}{' masked' if masked else ''}", samples, counts)
            print(f"{'':34s} max |fused - stock| = {diff:.3g}", flush=True)


def models(args):
    import aloscene
    from alonet.deformable_detr import DeformableDetrR50
    from alonet.detr import DetrR50

    fh, fw = (int(x) for x in args.frame.split("x"))
    gen = torch.Generator().manual_seed(1)
    frames = [aloscene.Frame(torch.rand(3, min(fh, FRAME_SIZES[i % 8][0]), min(fw, FRAME_SIZES[i % 8][1]), generator=gen) * 255,
                             normalization="255").norm_resnet() for i in range(args.batch)]
    frames[0] = aloscene.Frame(torch.rand(3, fh, fw, generator=gen) * 255, normalization="255").norm_resnet()
    batch = aloscene.Frame.batch_list(frames).to(DEV).to(torch.bfloat16)

    def switch(name):
        os.environ.pop("ALO_ATTENTION", None)
        if name == "fused":
            os.environ["ALO_ATTENTION"] = "fused"

    for cls in (DetrR50, DeformableDetrR50):
        torch.manual_seed(0)
        model = cls(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval().to(torch.bfloat16)
        legs = {"fused": lambda: model(batch), "stock": lambda: model(batch)}
        outs = {}
        for name in legs:
            switch(name)
            outs[name] = model(batch)
        diff = {k: (outs["fused"][k].float() - outs["stock"][k].float()).abs().max().item() for k in ("pred_logits", "pred_boxes")}
        samples, counts = alternate(legs, args.reps, args.window, setup=switch)
        show(f"{cls.__name__} bf16 {tuple(batch.shape)}", samples, counts, unit=1e3, suffix="ms")
        print(f"{'':34s} max |fused - stock| = {diff}", flush=True)
    switch("stock")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--frame", default="800x1333")
    ap.add_argument("--no-models", action="store_true")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; per call, "
          f"median (min - max) of {args.reps} windows of at least {args.window} s, legs alternating")
    with torch.no_grad():
        kernels(args)
        if not args.no_models:
            models(args)


if __name__ == "__main__":
    main()
