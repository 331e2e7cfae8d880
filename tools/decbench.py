"""The decoder's two fused chains (alo_hip.decoder_block_a / decoder_block_b) against the launches they replace, under HIP-graph
replay, at the decoder's row counts.

    python tools/decbench.py [--rows 300,600,2400] [--reps 7] [--inner 50]

Each form is captured once as a graph of ``--inner`` back-to-back copies (so a sample is kernel time, not launch overhead); a
sample is one replay divided by ``--inner``; forms alternate sample by sample.  Printed: median (min - max) in microseconds per
chain, both tile heights for the fused forms, and whether the outputs are bit-equal."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aloception-oss_amd"))
import alo_hip  # noqa: E402

DEV, BF = "cuda:0", torch.bfloat16


def weights(Fh=1024):
    gen = torch.Generator().manual_seed(23)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen) * scale).to(DEV, BF)
    return dict(wo=r(256, 256, scale=1 / 16), bo=r(256, scale=0.5), g=1 + r(256, scale=0.3), e=r(256, scale=0.3),
                wq=r(384, 256, scale=1 / 16), bq=r(384, scale=0.5), w1=r(Fh, 256, scale=1 / 16), b1=r(Fh, scale=0.5),
                w2=r(256, Fh, scale=Fh ** -0.5), b2=r(256, scale=0.5), wv=r(256, 256, scale=1 / 16), bv=r(256, scale=0.5),
                wqk=r(512, 256, scale=1 / 16), bqk=r(512, scale=0.5))


def forms(w, x, tgt, pos):
    norm = (w["g"], w["e"], 1e-5)

    def chain_a():
        t1, q = alo_hip.add_layernorm(alo_hip.linear_auto(x, w["wo"], w["bo"]), tgt, *norm, pos=pos)
        return t1, alo_hip.linear_auto(q, w["wq"], w["bq"])

    def chain_b():
        t2 = alo_hip.add_layernorm(alo_hip.linear_auto(x, w["wo"], w["bo"]), tgt, *norm)
        out, q = alo_hip.add_layernorm(alo_hip.ffn256(t2, w["w1"], w["b1"], w["w2"], w["b2"]), t2, *norm, pos=pos)
        return out, alo_hip.linear_auto(out, w["wv"], w["bv"]), alo_hip.linear_auto(q, w["wqk"], w["bqk"])

    fused_a = lambda t: (lambda: alo_hip.decoder_block_a(x, tgt, pos, w["wo"], w["bo"], norm, w["wq"], w["bq"], tile_rows=t))
    fused_b = lambda t: (lambda: alo_hip.decoder_block_b(x, tgt, pos, w["wo"], w["bo"], norm, w["w1"], w["b1"], w["w2"], w["b2"], norm,
                                                         w["wv"], w["bv"], w["wqk"], w["bqk"], tile_rows=t))
    return {"A": {"launches": chain_a, "fused/32": fused_a(32), "fused/64": fused_a(64)},
            "B": {"launches": chain_b, "fused/32": fused_b(32), "fused/64": fused_b(64)}}


def graph_of(fn, inner):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="300,600,2400")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    w = weights()
    print(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; "
          f"us per chain, median (min - max) of {args.reps} replays of {args.inner} copies")
    with torch.no_grad():
        for rows in (int(r) for r in args.rows.split(",")):
            gen = torch.Generator().manual_seed(rows)
            x, tgt, pos = (torch.randn(rows // 300 or 1, min(rows, 300), 256, generator=gen).to(DEV, BF) for _ in range(3))
            for chain, fs in forms(w, x, tgt, pos).items():
                want = fs["launches"]()
                equal = {name: all(torch.equal(a, b) for a, b in zip(fn(), want)) for name, fn in fs.items()}
                graphs = {name: graph_of(fn, args.inner) for name, fn in fs.items()}
                samples = {name: [] for name in fs}
                for g in graphs.values():
                    g.replay()
                torch.cuda.synchronize()
                for _ in range(args.reps):
                    for name, g in graphs.items():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        g.replay()
                        e.record()
                        torch.cuda.synchronize()
                        samples[name].append(s.elapsed_time(e) * 1e3 / args.inner)
                auto = alo_hip.decoder_block_tile_rows(x.shape[0] * x.shape[1], DEV)
                for name, v in samples.items():
                    print(f"rows={x.shape[0] * x.shape[1]:5d} chain {chain} {name:9s} {statistics.median(v):7.1f} ({min(v):.1f} - {max(v):.1f})"
                          f"  bit-equal={equal[name]}{'  <- routed' if name == f'fused/{auto}' else ''}", flush=True)


if __name__ == "__main__":
    main()
