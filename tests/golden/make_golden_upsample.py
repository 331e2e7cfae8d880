#!/usr/bin/env python
"""G20 — the reference's flow up-sampling (build container only).

  g20_raft_upsample.npz   alonet/raft/raft.py:109-123 (RAFTBase.upsample_flow, the convex combination) and
                          alonet/raft/utils/utils.py (upflow8, the bilinear mode), both run in fp64 on the float64 copies of
                          fp32 inputs:
                            flow         (2, 2, 5, 7) fp32, 4 * randn
                            mask         (2, 576, 5, 7) fp32 logits, 3 * randn; a few set to +-30, one tap of one cell to -inf
                            up           (2, 2, 40, 56) fp64, upsample_flow(flow, mask)
                            up_bilinear  (2, 2, 40, 56) fp64, upflow8(flow)

Arrays only.  The fixture pins the mask's channel order (k * 64 + i * 8 + j), the order of F.unfold's taps and the zero padding
with kept weights to the reference; the odd 5 x 7 map has border cells on every side and rows that are no multiple of anything.

Usage:  python tests/golden/make_golden_upsample.py        (from the repo root)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as G  # noqa: E402

INF_TAP = (1, 4 * 64 + 3 * 8 + 5, 2, 3)   # image 1, tap k = 4 (the centre), sub-pixel (3, 5), cell (2, 3)


def main():
    if not os.path.isdir(G.REF):
        sys.exit("make_golden_upsample.py needs the reference checkout (build container only)")
    ref = G.load_reference()
    R = importlib.import_module("alonet.raft.raft")
    torch.manual_seed(2000)
    flow = (4 * torch.randn(2, 2, 5, 7)).float()
    mask = (3 * torch.randn(2, 576, 5, 7)).float()
    pick = torch.randperm(mask.numel())[:12]
    mask.view(-1)[pick[:6]] = 30.0
    mask.view(-1)[pick[6:]] = -30.0
    mask[INF_TAP] = float("-inf")
    this = types.SimpleNamespace(out_plane=2)
    with torch.no_grad():
        up = R.RAFTBase.upsample_flow(this, flow.double(), mask.double())
        up_bilinear = ref.rutils.upflow8(flow.double())
    assert up.dtype == torch.float64 and tuple(up.shape) == (2, 2, 40, 56) and torch.isfinite(up).all()
    assert up_bilinear.dtype == torch.float64 and up_bilinear.shape == up.shape and torch.isfinite(up_bilinear).all()
    path = os.path.join(OUT, "g20_raft_upsample.npz")
    np.savez_compressed(path, flow=G._np(flow), mask=G._np(mask), up=G._np(up), up_bilinear=G._np(up_bilinear),
                        inf_tap=np.array(INF_TAP))
    print("wrote g20, bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
