"""alo_hip.stem_conv_pool_f32 against what the default fp32 route launches for the ResNet stem (``ResNetBody.forward``: a channels-last
copy of the image, MIOpen's 7x7 / stride 2 convolution, ``alo_hip.bias_act_`` over the half-resolution map, ``max_pool2d``), at the
fp32 headline's image sizes: 8 x 3 x 800 x 1333 and 1 x 3 x 800 x 1333, from an NCHW image as the detector hands it over.

    python tools/stembench_f32.py [--rounds 5] [--reps 20] [--batches 8 1]

tools/gemmbench_f32.py's protocol (its ``measure``): the two sides alternate `rounds` times in one process, each round timing `reps`
calls between device events after a warm-up of both; one JSON line per shape with the median round and the spread (min - max) in
microseconds per call, the ratio of the medians, max |difference| / max |value|, and whether the kernel's median is below the stock
median by more than both spreads — the rule alo_hip.STEM_F32_ROUTED is set by."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemmbench_f32 import alo_hip, measure  # noqa: E402  (puts the package on the path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--size", type=int, nargs=2, default=[800, 1333])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stembench_f32: needs the GPU (a timing taken anywhere else says nothing)")
    torch.manual_seed(0)
    h, w_ = args.size
    w = (torch.randn(64, 3, 7, 7, device="cuda") / 147 ** 0.5).contiguous(memory_format=torch.channels_last)   # as folded_conv_bn leaves it
    b = torch.randn(64, device="cuda")
    for n in args.batches:
        x = torch.randn(n, 3, h, w_, device="cuda")

        def stock():
            xc = x.contiguous(memory_format=torch.channels_last)
            return F.max_pool2d(alo_hip.bias_act_(F.conv2d(xc, w, None, 2, 3), b, None, True), 3, 2, 1)

        sides = {"kernel": lambda: alo_hip.stem_conv_pool_f32(x, w, b), "stock": stock}
        measure({"layer": "stem", "image": [n, 3, h, w_]}, sides, args.rounds, args.reps)
        del x, sides


if __name__ == "__main__":
    main()
