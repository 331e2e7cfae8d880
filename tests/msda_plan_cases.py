"""The cases of tests/test_msda_generic_plans_gpu.py, one line each, with the plan every line CLAIMS: the route and, for the generic
kernels, the row of csrc/msda.hip's table (kFwdVariants / kBwdVariants) and the runs per workgroup.  tests/test_msda_plans_cpu.py
asserts every claim with ``alo_msda_generic_plan`` (host only) and that the lists cover the table; the GPU file holds the results of
exactly these launches to the float64 oracle.  A change to make_plan, make_bwd_plan, make_dims or the routes therefore fails on the
CPU, with the name of the case that moved.

Lists:
  A  every (direction, row, dtype) instantiation once: N = 2, one run per workgroup, Lq * M no multiple of the 256 / g pairs of a run
     (the last run is partial and the batch boundary falls inside the grid), a level one pixel high, M and P that are no powers of
     two on the runtime-L*P rows.
  B  every (direction, row) in fp32 and fp16 at 2, 3 or 4 runs per workgroup: iters_total % iters_per_block != 0 (the last workgroup
     leaves its loop early), a partial last run, N = 2.  Lq is the smallest that meets all of that for the row's g (make_dims:
     iters_per_block = clamp(ceil(Lq * M / (256 / g)) * N / 4096, 1, 4)).  Backward pyramids are sized so that a value row receives
     N * Lq * L * P * 4 / S <= 64 corner contributions, as in the encoder launch; forward launches have no atomics and keep small levels
     (see the note on level sizes at the list).
  C  operands that start one element into a larger allocation.
"""
import collections

import numpy as np
import torch

FWD_GENERIC, FWD_WAVE = 1, 2                 # include/alo_hotpath.h ALO_MSDA_FWD_*
BWD_GENERIC, BWD_TILED, BWD_WIDE = 0, 1, 2   # ALO_MSDA_BWD_*

DTYPES = ("f32", "f64", "bf16", "f16")
TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
ELEM = {"f32": 4, "f64": 8, "bf16": 2, "f16": 2}
CODE = {"f32": 0, "f64": 1, "bf16": 2, "f16": 3}   # alo_dtype_t

# The table of csrc/msda.hip as (wide, g, lp16).  wide: vec = 16 bytes of the dtype (4 fp32, 2 fp64, 8 bf16 / fp16), else 1.
FWD_ROWS = [(1, 4, 1), (1, 8, 1), (1, 16, 1), (1, 4, 0), (1, 8, 0), (1, 16, 0), (1, 64, 0), (0, 8, 0), (0, 64, 0)]
BWD_ROWS = [(0, 8, 0), (0, 32, 0), (0, 64, 0), (1, 64, 0), (1, 16, 1), (1, 16, 0)]   # the last two: 2-byte values only


def rows(direction, dtype):
    if direction == "fwd":
        return FWD_ROWS
    return BWD_ROWS if ELEM[dtype] == 2 else BWD_ROWS[:4]


def vec_of(wide, dtype):
    return 16 // ELEM[dtype] if wide else 1


# claim = (route, vec, g, lp16, iters_per_block); off = {operand: elements into its allocation}; hint: the backward gets host shapes
Case = collections.namedtuple("Case", "name group direction dtype N M D Lq levels P off hint kinds claim seed")

L2 = [(5, 7), (1, 3)]                                                     # a level one pixel high in every pyramid of A and C
L4 = [(6, 5), (3, 4), (1, 3), (2, 2)]
L8 = [(6, 5), (3, 4), (1, 3), (2, 2), (4, 3), (2, 5), (3, 3), (1, 1)]

# ---- A: (row, D for fp32 / fp64 / 2-byte, M, Lq, levels, P).  D reaches the row through make_plan: lanes = D / vec -> g = 4 up to 4
# lanes, 8 up to 8, 16 up to 16, else 64; the counts 3, 5, 9, 17 leave lanes of the group idle.  bf16 with L = P = 4, D % 8 == 0,
# D <= 32 takes the wave kernel, so the g = 4 row has L * P = 16 as (2, 8); the backward's scalar rows go by D alone (<= 8, <= 32, <= 64).
A_FWD = [
    ((1, 4, 1), (12, 6, 24), 3, 23, L2, 8),
    ((1, 8, 1), (20, 10, 40), 4, 23, L8, 2),
    ((1, 16, 1), (36, 18, 72), 3, 23, L4, 4),
    ((1, 4, 0), (12, 6, 24), 3, 23, L2, 3),
    ((1, 8, 0), (20, 10, 40), 3, 23, L2, 3),
    ((1, 16, 0), (36, 18, 72), 3, 23, L2, 3),
    ((1, 64, 0), (68, 34, 136), 3, 23, L2, 3),
    ((0, 8, 0), (3, 3, 3), 3, 23, L2, 3),
    ((0, 64, 0), (9, 9, 9), 3, 23, L2, 3),
]
A_BWD = [
    ((0, 8, 0), (3, 3, 3), 3, 23, L2, 3),
    ((0, 32, 0), (20, 20, 20), 3, 23, L2, 3),
    ((0, 64, 0), (40, 40, 40), 3, 23, L2, 3),
    ((1, 64, 0), (68, 66, 136), 3, 23, L2, 3),
    ((1, 16, 1), (None, None, 72), 3, 23, L2, 8),
    ((1, 16, 0), (None, None, 72), 3, 23, L2, 3),
]

# ---- B: (row, D for fp32 / fp16, M, Lq, levels, P, iters_per_block, fused ref_dim).  N = 2.
# Level sizes.  The kernels (like the reference op) place a sample with fp32 arithmetic: h_im = loc * H - 0.5 is rounded to half an ulp
# of h_im, 2^-25 * 2^ceil(log2 H) px, and an output moves by that times the value's slope (values are N(0, 1): a few units per px, times
# D^0.5 in grad_attn's sum over channels).  Under 8 px that is 2.4e-7 px: inside the 1e-6 the fp16 forward bar leaves beside half an fp16
# ulp, which the existing fp16 cases (levels up to 9 x 7) rely on too; a 23 px level is over it for a few of 10^7 outputs, and
# a 200 px level puts grad_attn at D = 72 at three times its atol of 1e-4.  What B tests, the run loop, does not depend on the size of
# a level, so the forward cases keep S3 (with a level one pixel high) and the backward pyramid that needs the most pixels is 16 levels
# of 34 x 35 instead of 4 levels up to 150 x 200 (M = 7 keeps Lq, and with it the pixel count the 64 contributions ask for, small).
# The float32 build of the oracle, fed the same inputs, predicts each of these figures without a GPU.
S3 = [(3, 4), (1, 2)]
B_FWD = [
    ((1, 4, 1), (4, 8), 3, 87382, S3, 8, 2, 2),
    ((1, 8, 1), (20, 40), 3, 43691, S3, 8, 2, 4),
    ((1, 16, 1), (36, 72), 3, 21846, S3, 8, 2, 2),
    ((1, 4, 0), (4, 8), 3, 87382, S3, 1, 2, 4),
    ((1, 8, 0), (20, 40), 3, 43691, S3, 1, 2, 2),
    ((1, 16, 0), (36, 72), 3, 32769, S3, 1, 3, 4),
    ((1, 64, 0), (68, 136), 3, 10923, S3, 1, 4, 2),
    ((0, 8, 0), (3, 3), 3, 43691, S3, 1, 2, 4),
    ((0, 64, 0), (9, 9), 3, 8193, S3, 1, 3, 2),
]
B_BWD = [
    ((0, 8, 0), (3, 3), 3, 43691, [(90, 100), (40, 50)], 1, 2, None),
    ((0, 32, 0), (9, 9), 3, 10923, [(50, 45), (25, 20)], 1, 2, None),
    ((0, 64, 0), (33, 33), 3, 8193, [(40, 42), (20, 19)], 1, 3, None),
    ((1, 64, 0), (68, 136), 3, 10923, [(50, 45), (25, 20)], 1, 4, None),
    ((1, 16, 1), (None, 72), 7, 9363, [(34, 35)] * 16, 1, 2, None),
    ((1, 16, 0), (None, 72), 3, 21846, [(70, 60), (35, 37)], 1, 2, None),
]

# ---- C: (name, direction, dtype, D, Lq, levels, P, off, hint, claim).  N = 2, M = 3.
#  1. value one element in: the scalar rows (D = 8 and 72 are wide rows when aligned; backward D = 8 is scalar either way)
#  2. loc / attn (fused: offsets, logits, reference points) one element in, value aligned: the L * P = 16 stage reads a location pair
#     in one load, which the plan admits only behind 16-byte aligned operands, so these take the runtime-L*P row of the same g; the
#     bf16 launch (L = P = 4, D = 32) also leaves the wave kernel
#  3. grad_out one element in, fp32 D = 32 L = P = 4, with (Lq == S) and without a host hint: neither tiled nor wide
#  4. out one element in
C_LINES = [(f"value+1-{d}-{dt}-D{D}", d, dt, D, 23, L2, 3, {"value": 1}, False,
            (FWD_GENERIC if d == "fwd" else BWD_GENERIC, 1, 8 if D <= 8 else 64, 0, 1))
           for dt in DTYPES for D in (8, 72) for d in ("fwd", "bwd")] + [
    ("loc+1-f32-lp16", "fwd", "f32", 12, 23, L2, 8, {"loc": 1, "attn": 1, "ref": 1}, False, (FWD_GENERIC, 4, 4, 0, 1)),
    ("loc+1-bf16-L4P4-D32", "fwd", "bf16", 32, 23, L4, 4, {"loc": 1, "attn": 1, "ref": 1}, False, (FWD_GENERIC, 8, 4, 0, 1)),
    ("grad_out+1-f32-D32", "bwd", "f32", 32, 23, L4, 4, {"grad_out": 1}, False, (BWD_GENERIC, 1, 32, 0, 1)),
    ("grad_out+1-f32-D32-hint", "bwd", "f32", 32, 49, L4, 4, {"grad_out": 1}, True, (BWD_GENERIC, 1, 32, 0, 1)),
    ("out+1-f32", "fwd", "f32", 12, 23, L2, 3, {"out": 1}, False, (FWD_GENERIC, 1, 64, 0, 1)),
]
# the aligned twins of C.2 and C.3: what the unaligned operand moves the launch away from
ALIGNED_TWINS = {"loc+1-f32-lp16": (FWD_GENERIC, 4, 4, 1, 1), "loc+1-bf16-L4P4-D32": (FWD_WAVE, 0, 0, 0, 0),
                 "grad_out+1-f32-D32": (BWD_TILED, 0, 0, 0, 0), "grad_out+1-f32-D32-hint": (BWD_WIDE, 0, 0, 0, 0)}


def _cases():
    out = []
    for direction, lines in (("fwd", A_FWD), ("bwd", A_BWD)):
        for row, Ds, M, Lq, levels, P in lines:
            for dt in DTYPES:
                D = Ds[{"f32": 0, "f64": 1}.get(dt, 2)]
                if D is None:
                    continue
                route = FWD_GENERIC if direction == "fwd" else BWD_GENERIC
                kinds = ("plain", "fused2", "fused4") if direction == "fwd" else ("bwd",)
                out.append(Case(f"A-{direction}-w{row[0]}g{row[1]}lp{row[2]}-{dt}", "A", direction, dt, 2, M, D, Lq, levels, P, {}, False,
                                kinds, (route, vec_of(row[0], dt), row[1], row[2], 1), 100 + len(out)))
    for direction, lines in (("fwd", B_FWD), ("bwd", B_BWD)):
        for row, Ds, M, Lq, levels, P, ipb, ref_dim in lines:
            for i, dt in enumerate(("f32", "f16")):
                if Ds[i] is None:
                    continue
                route = FWD_GENERIC if direction == "fwd" else BWD_GENERIC
                kinds = ("plain", f"fused{ref_dim}") if direction == "fwd" else ("bwd",)
                out.append(Case(f"B-{direction}-w{row[0]}g{row[1]}lp{row[2]}-{dt}-x{ipb}", "B", direction, dt, 2, M, Ds[i], Lq, levels, P, {},
                                False, kinds, (route, vec_of(row[0], dt), row[1], row[2], ipb), 300 + len(out)))
    for name, direction, dt, D, Lq, levels, P, off, hint, claim in C_LINES:
        kinds = ("bwd",) if direction == "bwd" else ("plain",) if "out" in off else ("plain", "fused2", "fused4")
        out.append(Case("C-" + name, "C", direction, dt, 2, 3, D, Lq, levels, P, off, hint, kinds, claim, 500 + len(out)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c, kind) for c in CASES for kind in c.kinds]   # one GPU test each; the kinds of a case are neighbours (they share inputs)


def n_levels(c):
    return len(c.levels)


def n_pixels(c):
    return sum(h * w for h, w in c.levels)


def alignment(c):
    """(aligned, all_aligned) as forward_impl / alo_msda_backward_hinted compute them from the pointers of this case."""
    first = {"value", "out"} if c.direction == "fwd" else {"value", "grad_out"}
    assert all(n == 1 for n in c.off.values())   # one element of 2, 4 or 8 bytes: never a multiple of 16
    return int(not set(c.off) & first), int(not set(c.off) - first)


def query(lib, c, fused=0, aligned=None):
    """``alo_msda_generic_plan`` for case ``c`` -> (route, vec, g, lp16, iters_per_block, blocks_per_batch, iters_total)."""
    import ctypes

    a, aa = alignment(c) if aligned is None else aligned
    hint = (ctypes.c_int32 * (2 * n_levels(c)))(*[v for hw in c.levels for v in hw]) if c.hint else None
    out = (ctypes.c_int * 6)(*[-7] * 6)
    ldt = CODE["f64"] if c.dtype == "f64" else CODE["f32"]
    route = lib.alo_msda_generic_plan(c.N, n_pixels(c), c.M, c.D, n_levels(c), c.Lq, c.P, CODE[c.dtype], ldt, hint,
                                      int(c.direction == "bwd"), fused, a, aa, out)
    return (route, *out)


# ---- inputs: seeded, one generator stream per tensor so that a test can draw the locations alone -------------------------------
def _rng(c, stream):
    return np.random.default_rng([c.seed, stream])


def _geo(c):
    return np.float64 if c.dtype == "f64" else np.float32


def storage(x, dtype):
    """``x`` rounded to the storage dtype, as a CPU tensor."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(TORCH[dtype])


def draw_loc(c):
    shape = (c.N, c.Lq, c.M, n_levels(c), c.P, 2)
    return (_rng(c, 0).random(shape, dtype=_geo(c)) * _geo(c)(1.6) - _geo(c)(0.3)).astype(_geo(c))   # loc_range (-0.3, 1.3)


def smooth_samples(c, loc):
    """grad_loc jumps where an image coordinate crosses an integer: the samples at least 1e-3 px away from one (the mask of
    tests/test_msda_f16_gpu.py::test_generic_backward_vs_oracle)."""
    size = np.asarray(c.levels, np.float64)[:, ::-1].reshape(1, 1, 1, n_levels(c), 1, 2)
    t = loc.astype(np.float64) * size - 0.5
    return (np.abs(t - np.round(t)) >= 1e-3).all(-1)


def draw_value(c):
    return storage(_rng(c, 1).standard_normal((c.N, n_pixels(c), c.M, c.D), dtype=np.float32), c.dtype)


def draw_attn(c):
    logits = _rng(c, 2).standard_normal((c.N, c.Lq, c.M, n_levels(c) * c.P), dtype=_geo(c))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).reshape(c.N, c.Lq, c.M, n_levels(c), c.P).astype(_geo(c))


def draw_grad_out(c):
    return storage(_rng(c, 3).standard_normal((c.N, c.Lq, c.M * c.D), dtype=np.float32), c.dtype)


def draw_fused(c, ref_dim):
    """Raw offsets and logits in the storage dtype, reference points in the geometry dtype (the inputs of
    tests/test_msda_f16_gpu.py::test_generic_fused_forward_vs_oracle)."""
    rng = _rng(c, 4 + ref_dim)
    L, P = n_levels(c), c.P
    offsets = storage(rng.standard_normal((c.N, c.Lq, c.M, L, P, 2), dtype=np.float32) * np.float32(2.5), c.dtype)
    logits = storage(rng.standard_normal((c.N, c.Lq, c.M, L * P), dtype=np.float32) * np.float32(2.0), c.dtype)
    ref = rng.random((c.N, c.Lq, L, ref_dim), dtype=_geo(c))
    if ref_dim == 4:
        ref[..., 2:] *= _geo(c)(0.4)
    return offsets, logits, torch.from_numpy(ref)
