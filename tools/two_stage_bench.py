#!/usr/bin/env python
"""Two-stage Deformable-DETR glue at the headline size: the kernels of csrc/two_stage.hip next to the torch formulation they replace.

    python tools/two_stage_bench.py [--which kernels,prologue,model] [--samples 15] [--inner 10] [--B 8] [--dtype bf16|f32]

Prints one JSON object per line.  Every ``ms`` is the median of ``--samples`` samples, each the mean of ``--inner`` back-to-back
calls between one pair of device events, after >= 0.1 s of warm-up calls; ``min`` / ``max`` are the extreme samples.

  kernels   each kernel against the torch ops it stands for, on the same tensors (B x 22 223 tokens of the 800 x 1333 pyramid, image b
            padded by b / 20 of each side on the right and bottom, K = 300)
  prologue  ``DeformableTransformer._two_stage_queries`` (proposals, masking, enc_output + LayerNorm, heads, top-k, queries, pos_trans +
            LayerNorm) with the kernels and with their ``*_supported`` predicates switched off
  model     ms_per_step (HIP-graph replay of the forward + eager ``inference()``, as bench.py) of a two-stage R50-sized DeformableDETR
            (6 + 6 layers, 300 proposals, box refinement, 91 classes), with the kernels and without
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aloception-oss_amd"))
import alo_hip  # noqa: E402
from alonet.deformable_detr import DeformableDETR  # noqa: E402
from alonet.deformable_detr.backbone import Joiner  # noqa: E402
from alonet.deformable_detr.deformable_transformer import encoder_output_proposals, proposal_pos_embed  # noqa: E402

DETR_SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]
DEV = "cuda:0"
PREDICATES = ("encoder_proposals_masked_supported", "encoder_proposals_supported", "mask_rows_supported", "proposal_queries_supported")


def sample(fn, samples, inner):
    """{ms, min, max}: median / extremes over ``samples`` of the mean time of ``inner`` back-to-back calls (device events)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:   # the chip leaves its idle clocks only after some milliseconds of work
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
    got = []
    for _ in range(samples):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        torch.cuda.synchronize()
        got.append(start.elapsed_time(stop) / inner)
    got.sort()
    return dict(ms=round(got[len(got) // 2], 5), min=round(got[0], 5), max=round(got[-1], 5))


class torch_formulation:
    """Inside: the ``*_supported`` predicates of the two-stage kernels answer False, so the module runs its torch ops."""

    def __enter__(self):
        self.saved = {name: getattr(alo_hip, name) for name in PREDICATES}
        for name in PREDICATES:
            setattr(alo_hip, name, lambda *a, **k: False)

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(alo_hip, name, fn)


def padded_mask(B, shapes=DETR_SHAPES):
    levels = []
    for h, w in shapes:
        m = torch.zeros(B, h, w, dtype=torch.bool)
        for b in range(B):
            m[b, h - h * b // 20:, :] = True
            m[b, :, w - w * b // 20:] = True
        levels.append(m.flatten(1))
    return torch.cat(levels, 1).to(DEV)


def bench_kernels(a, dtype):
    B, K = a.B, 300
    mask = padded_mask(B)
    S = mask.shape[1]
    gen = torch.Generator(device=DEV).manual_seed(0)
    memory = torch.randn(B, S, 256, generator=gen, device=DEV).to(dtype)
    coords = torch.randn(B, S, 4, generator=gen, device=DEV) * 3
    topk = torch.stack([torch.randperm(S, generator=gen, device=DEV)[:K] for _ in range(B)])
    _, keep = alo_hip.encoder_proposals(mask, DETR_SHAPES)
    slab = 2 * memory.numel() * memory.element_size()

    def torch_queries():
        picked = torch.gather(coords, 1, topk.unsqueeze(-1).expand(-1, -1, 4))
        return picked.sigmoid(), proposal_pos_embed(picked).to(dtype)

    def separate():
        _, k = alo_hip.encoder_proposals(mask, DETR_SHAPES)
        return alo_hip.mask_rows(memory, k)

    def torch_both():
        _, k = encoder_output_proposals(mask, DETR_SHAPES)
        return memory.masked_fill(~k.unsqueeze(-1), 0.0)

    masked = ("proposals + mask_rows", "hip, folded into one launch", lambda: alo_hip.encoder_proposals_masked(mask, DETR_SHAPES, memory), slab + 18 * B * S)
    legs = [("encoder_proposals", "hip", lambda: alo_hip.encoder_proposals(mask, DETR_SHAPES), 18 * B * S),
            ("encoder_proposals", "torch", lambda: encoder_output_proposals(mask, DETR_SHAPES), 18 * B * S),
            ("mask_rows", "hip", lambda: alo_hip.mask_rows(memory, keep), slab),
            ("mask_rows", "torch", lambda: memory.masked_fill(~keep.unsqueeze(-1), 0.0), slab),
            ("proposals + mask_rows", "hip, two launches", separate, slab + 18 * B * S),
            masked,
            ("proposals + mask_rows", "torch", torch_both, slab + 18 * B * S),
            ("proposal_queries", "hip", lambda: alo_hip.proposal_queries(coords, topk, dtype), B * K * 512 * memory.element_size()),
            ("proposal_queries", "torch", torch_queries, B * K * 512 * memory.element_size())]
    for name, how, fn, nbytes in legs:
        r = sample(fn, a.samples, a.inner)
        yield dict(leg=name, how=how, B=B, S=S, dtype=str(dtype).split(".")[-1], alg_bytes=nbytes, GBps=round(nbytes / r["ms"] / 1e6, 1), **r)


def two_stage_model(dtype, enc_layers=6, dec_layers=6):
    torch.manual_seed(0)
    new = DeformableDETR.__new__(DeformableDETR)
    backbone = Joiner(new.build_backbone("resnet50", True, True, False), new.build_positional_encoding(256))
    transformer = new.build_transformer(hidden_dim=256, dropout=0.1, nheads=8, dim_feedforward=1024, enc_layers=enc_layers,
                                        dec_layers=dec_layers, num_feature_levels=4, two_stage=True, num_queries=300)
    model = DeformableDETR(backbone, transformer, num_classes=91, num_queries=300, aux_loss=False, with_box_refine=True,
                           device=torch.device(DEV)).eval()
    return model.to(dtype) if dtype != torch.float32 else model


def bench_prologue(a, dtype):
    B = a.B
    tr = two_stage_model(dtype, 1, 1).transformer
    mask = padded_mask(B)
    S = mask.shape[1]
    memory = torch.randn(B, S, 256, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV).to(dtype)

    def run():
        with torch.no_grad():
            return tr._two_stage_queries(memory, mask, DETR_SHAPES, {})

    with alo_hip.LaunchTimer() as timer:
        run()
    ran = sorted(tag.split("/")[0] for tag in timer.summary())
    yield dict(leg="prologue", how="hip", B=B, S=S, dtype=str(dtype).split(".")[-1], launches_of_this_library=ran, **sample(run, a.samples, a.inner))
    with torch_formulation():
        yield dict(leg="prologue", how="torch", B=B, S=S, dtype=str(dtype).split(".")[-1], **sample(run, a.samples, a.inner))


def bench_model(a, dtype):
    import aloscene
    from alonet.common import GraphedForward

    model = two_stage_model(dtype)
    gen = torch.Generator().manual_seed(1234)
    frames = [aloscene.Frame(torch.rand(3, 800 - 40 * (b % 4), 1333 - 64 * (b % 4), generator=gen) * 255, normalization="255").norm_resnet()
              for b in range(a.B)]
    frames = aloscene.Frame.batch_list(frames).to(DEV)
    frames = frames.to(dtype) if dtype != torch.float32 else frames
    for how in ("hip", "torch"):
        with torch_formulation() if how == "torch" else torch.no_grad():
            graphed = GraphedForward(model, adopt_inputs=True)

            def step():
                with torch.no_grad():
                    return model.inference(graphed(frames))

            for _ in range(a.warmup):
                step()
            got = []
            for _ in range(a.samples):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    step()
                torch.cuda.synchronize()
                got.append((time.perf_counter() - t0) / a.inner * 1e3)
            got.sort()
        yield dict(leg="two-stage DeformableDETR-R50, forward (graph replay) + inference()", how=how, B=a.B, dtype=str(dtype).split(".")[-1],
                   ms_per_step=round(got[len(got) // 2], 4), min=round(got[0], 4), max=round(got[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="kernels,prologue,model")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    dtype = dict(f32=torch.float32, bf16=torch.bfloat16)[a.dtype]
    for w in a.which.split(","):
        for r in dict(kernels=bench_kernels, prologue=bench_prologue, model=bench_model)[w](a, dtype):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
