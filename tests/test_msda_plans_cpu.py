"""alo_msda_generic_plan (host only): the plan functions of csrc/msda.hip seen through the ABI, and the claims of
tests/msda_plan_cases.py.  No GPU needed.

  * every plan is a row of the table for its element size and every row is some launch's plan: what the static_asserts of msda.hip
    state, observed from outside;
  * the block shape follows make_dims' formula at the thresholds between 1, 2, 3 and 4 runs per workgroup;
  * every line of the GPU test's case lists launches the instantiation it names, at the runs per workgroup it names, and the lists
    cover every instantiation (A), every row at two or more runs per workgroup in fp32 and fp16 (B), and the unaligned launches (C).
"""
import ctypes

import pytest

import alo_hip
import msda_plan_cases as T

LIB = alo_hip.lib()


def plan(N, S, M, D, L, Lq, P, dt, backward, fused=0, aligned=1, all_aligned=1, hint=None):
    out = (ctypes.c_int * 6)(*[-7] * 6)
    ldt = T.CODE["f64"] if dt == "f64" else T.CODE["f32"]
    route = LIB.alo_msda_generic_plan(N, S, M, D, L, Lq, P, T.CODE[dt], ldt, hint, backward, fused, aligned, all_aligned, out)
    return (route, *out)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("dt", T.DTYPES)
def test_every_plan_is_a_table_row_and_every_row_is_reached(dt, direction):
    backward = int(direction == "bwd")
    table = {(T.vec_of(w, dt), g, lp) for w, g, lp in T.rows(direction, dt)}
    generic = T.BWD_GENERIC if backward else T.FWD_GENERIC
    hit = set()
    for D in range(1, 257):
        for aligned in (0, 1):
            for all_aligned in (0, 1):
                for L, P in ((2, 8), (2, 3)):   # L * P == 16 or not; (2, 8) keeps bf16 off the wave kernel and fp32 D = 32 off the tiled one
                    for fused in ((0,) if backward else (0, 1)):
                        route, vec, g, lp16, ipb, blocks, iters = plan(1, 100, 2, D, L, 5, P, dt, backward, fused, aligned, all_aligned)
                        what = (dt, direction, D, aligned, all_aligned, L, P, fused)
                        assert route == generic, what
                        assert (vec, g, lp16) in table, (what, (vec, g, lp16))
                        assert (ipb, blocks, iters) == (1, iters, -(-10 // (256 // g))), what
                        # a wide row needs value and out on 16 bytes and whole vectors; the forward's unrolled stage reads location
                        # pairs in one load and needs the other operands there too (the backward's reads element by element)
                        assert vec == 1 or (aligned and D % vec == 0), what
                        assert not lp16 or (L * P == 16 and (backward or all_aligned)), what
                        hit.add((vec, g, lp16))
    assert hit == table, sorted(table - hit)


def make_dims(N, Lq, M, g):
    """make_dims of csrc/msda.hip: runs of 256 / g pairs; about 4096 workgroups, at most 4 runs each."""
    pairs = 256 // g
    iters_total = -(-Lq * M // pairs)
    ipb = min(4, max(1, iters_total * N // 4096))
    return ipb, -(-iters_total // ipb), iters_total


@pytest.mark.parametrize("direction,dt,D,g", [("fwd", "f32", 4, 4), ("fwd", "f16", 40, 8), ("fwd", "f64", 18, 16), ("fwd", "f32", 9, 64),
                                              ("bwd", "f32", 9, 32), ("bwd", "bf16", 72, 16), ("bwd", "f64", 3, 8)])
def test_block_shape_at_the_thresholds_of_runs_per_block(direction, dt, D, g):
    pairs = 256 // g
    seen = set()
    for N, iters_total in [(1, 8191), (1, 8192), (2, 4096), (1, 12287), (1, 12288), (3, 4096), (2, 6144), (1, 16383), (1, 16384), (2, 8192),
                           (4, 4096), (1, 4095), (2, 4095), (3, 2731), (1, 1000000), (7, 300000), (1, 1)]:
        for Lq, M in ((iters_total * pairs, 1), (iters_total * pairs - 1, 1), (iters_total * pairs // 2, 2)):
            if Lq < 1:
                continue
            route, vec, g_, lp16, ipb, blocks, iters = plan(N, 50, M, D, 2, Lq, 1, dt, int(direction == "bwd"))
            assert g_ == g and (ipb, blocks, iters) == make_dims(N, Lq, M, g), (N, Lq, M)
            assert iters == iters_total
            seen.add((iters_total * N, ipb))
    # the thresholds themselves: 8191 -> 1 run, 8192 -> 2, 12287 -> 2, 12288 -> 3, 16383 -> 3, 16384 -> 4, and 4 for good
    assert {(8191, 1), (8192, 2), (12287, 2), (12288, 3), (16383, 3), (16384, 4), (1000000, 4), (2100000, 4), (1, 1)} <= seen


def test_refused_launches_and_the_other_routes_report_no_row():
    assert plan(1, 100, 8, 32, 33, 100, 4, "f32", 0)[0] == -1 and plan(1, 100, 8, 32, 33, 100, 4, "f32", 0)[1:] == (-7,) * 6   # L > 32
    assert plan(1, 100, 8, 32, 4, 0, 4, "f32", 1)[0] == -1
    assert LIB.alo_msda_generic_plan(1, 100, 8, 32, 4, 100, 4, 0, 0, None, 0, 0, 1, 1, None) == -1
    out = (ctypes.c_int * 6)()
    assert LIB.alo_msda_generic_plan(1, 100, 8, 32, 4, 100, 4, T.CODE["bf16"], T.CODE["bf16"], None, 0, 0, 1, 1, out) == -1   # dtype pair
    # the matrix-core forward and the tiled backward have no row; what they need is every pointer aligned
    assert plan(1, 100, 8, 32, 4, 100, 4, "bf16", 0) == (T.FWD_WAVE, 0, 0, 0, 0, 0, 0)
    assert plan(1, 100, 8, 32, 4, 100, 4, "bf16", 0, all_aligned=0)[:4] == (T.FWD_GENERIC, 8, 4, 0)
    assert plan(1, 100, 8, 32, 4, 100, 4, "bf16", 0, aligned=0)[:4] == (T.FWD_GENERIC, 1, 64, 0)
    assert plan(1, 100, 8, 32, 4, 100, 4, "f16", 0)[:4] == (T.FWD_GENERIC, 8, 4, 1)   # pixel-major fp16 never leaves the generic kernels
    assert plan(1, 100, 8, 32, 4, 100, 4, "f32", 1) == (T.BWD_TILED, 0, 0, 0, 0, 0, 0)
    assert plan(1, 100, 8, 32, 4, 100, 4, "f32", 1, all_aligned=0)[:4] == (T.BWD_GENERIC, 1, 32, 0)
    assert plan(1, 100, 8, 32, 4, 100, 4, "f32", 1, aligned=0, all_aligned=1)[:4] == (T.BWD_GENERIC, 1, 32, 0)
    # the query and alo_msda_backward_path read one plan
    for D in (16, 32, 64, 72):
        for dt in T.DTYPES:
            ldt = T.CODE["f64"] if dt == "f64" else T.CODE["f32"]
            assert plan(2, 100, 8, D, 4, 100, 4, dt, 1)[0] == LIB.alo_msda_backward_path(2, 100, 8, D, 4, 100, 4, T.CODE[dt], ldt, None)


# ---- the case lists of the GPU test ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_case_launches_what_its_line_claims(c):
    for fused in ((0, 1) if c.direction == "fwd" else (0,)):
        got = T.query(LIB, c, fused)
        assert got[:5] == c.claim, f"{c.name} (fused={fused}) claims (route, vec, g, lp16, iters_per_block) = {c.claim}, the library plans {got[:5]}"
    assert (c.claim[1] != 1, c.claim[2], c.claim[3]) in [(bool(w), g, lp) for w, g, lp in T.rows(c.direction, c.dtype)]
    if c.name[2:] in T.ALIGNED_TWINS:   # the same launch behind aligned pointers: the kernel the offset moves it away from
        assert T.query(LIB, c, 0, aligned=(1, 1))[:5] == T.ALIGNED_TWINS[c.name[2:]], c.name


def _pairs_per_run(c):
    return 256 // c.claim[2]


def test_list_a_covers_every_instantiation_with_a_partial_last_run():
    generic = {"fwd": T.FWD_GENERIC, "bwd": T.BWD_GENERIC}
    want = {(d, dt, (T.vec_of(w, dt), g, lp)) for d in ("fwd", "bwd") for dt in T.DTYPES for w, g, lp in T.rows(d, dt)}
    assert len(want) == 36 + 20   # the fused forward is the same row: 72 forward and 20 backward instantiations
    have = set()
    for c in T.CASES:
        if c.group != "A":
            continue
        assert c.claim[0] == generic[c.direction] and c.claim[4] == 1 and c.N == 2 and not c.off, c.name
        assert (c.Lq * c.M) % _pairs_per_run(c) != 0, c.name
        assert T.query(LIB, c)[5] >= 1 and any(h == 1 for h, w in c.levels), c.name
        if not c.claim[3]:   # the runtime-L*P rows: integer divisions instead of shifts
            assert c.M & (c.M - 1) and c.P & (c.P - 1), c.name
        if c.direction == "fwd":
            assert set(c.kinds) == {"plain", "fused2", "fused4"}, c.name
        have.add((c.direction, c.dtype, c.claim[1:4]))
    assert have == want, sorted(want - have)


def test_list_b_covers_every_row_at_several_runs_per_block_in_fp32_and_fp16():
    want = {(d, dt, (T.vec_of(w, dt), g, lp)) for d in ("fwd", "bwd") for dt in ("f32", "f16") for w, g, lp in T.rows(d, dt)}
    have, runs = set(), {"fwd": set(), "bwd": set()}
    for c in T.CASES:
        if c.group != "B":
            continue
        route, vec, g, lp16, ipb, blocks, iters = T.query(LIB, c)
        assert ipb >= 2 and iters % ipb != 0 and (c.Lq * c.M) % _pairs_per_run(c) != 0 and c.N >= 2, c.name
        assert blocks == -(-iters // ipb), c.name
        # no smaller Lq does: the case is the cheapest that runs its row this way
        assert not any(_meets(c, lq, ipb) for lq in range(max(1, c.Lq - 40), c.Lq)), c.name
        if c.direction == "bwd":   # corner contributions per value row, the issue's N * Lq * M * L * P * 4 / (S * M)
            assert c.N * c.Lq * T.n_levels(c) * c.P * 4 / T.n_pixels(c) <= 64.5, c.name
        have.add((c.direction, c.dtype, (vec, g, lp16)))
        runs[c.direction].add(ipb)
    assert have == want, sorted(want - have)
    assert runs["fwd"] >= {2, 3, 4} and runs["bwd"] >= {2, 3, 4}


def _meets(c, Lq, ipb):
    got = make_dims(c.N, Lq, c.M, c.claim[2])
    return got[0] == ipb and got[2] % ipb != 0 and (Lq * c.M) % _pairs_per_run(c) != 0


def test_list_c_names_the_unaligned_launches():
    names = {c.name for c in T.CASES if c.group == "C"}
    for dt in T.DTYPES:
        for D in (8, 72):   # D <= 8 and D > 8, both directions
            assert {f"C-value+1-fwd-{dt}-D{D}", f"C-value+1-bwd-{dt}-D{D}"} <= names
    for c in T.CASES:
        if c.group == "C":
            assert c.off and c.claim[4] == 1, c.name
            if "value" in c.off or "out" in c.off:
                assert c.claim[1] == 1, c.name   # the scalar rows
    assert T.BY_NAME["C-grad_out+1-f32-D32-hint"].Lq == T.n_pixels(T.BY_NAME["C-grad_out+1-f32-D32-hint"])   # the wrapper passes the hint


@pytest.mark.parametrize("c", [c for c in T.CASES if c.direction == "bwd"], ids=lambda c: c.name)
def test_masked_share_of_grad_loc_stays_below_one_percent(c):
    """The backward tests leave out samples within 1e-3 px of an integer coordinate: about 0.4 % with two coordinates per sample."""
    smooth = T.smooth_samples(c, T.draw_loc(c))
    assert (~smooth).mean() <= 0.01, f"{c.name}: {(~smooth).mean():.4%} of the samples masked"
