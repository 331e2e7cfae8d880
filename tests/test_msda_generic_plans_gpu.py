"""The generic MSDeformAttn kernels (msda_fwd_kernel plain and fused, msda_bwd_kernel) against the float64 oracle, one launch per line
of tests/msda_plan_cases.py: every instantiation of the table once (A), every row at 2, 3 or 4 runs per workgroup in fp32 and fp16
(B), and operands that start one element into a larger allocation, also inside guarded buffers (C).  Which instantiation a line
launches is asserted on the CPU (tests/test_msda_plans_cpu.py) and again here, from the same query, before the launch.

The oracle gets the values the kernel gets: inputs are rounded to the storage dtype first, the fused forward's locations and weights
are MSDeformAttn's prologue in float64 on the rounded offsets and logits (prologue64).  Bars are the suite's own:
  fp32 / fp64  tests/test_msda_gpu.py::test_forward_backward_vs_oracle
  bf16         tests/test_msda_gpu.py::test_bf16_storage_matches_oracle_on_bf16_rounded_inputs
  fp16         tests/test_msda_f16_gpu.py::assert_forward_bound and ::test_generic_backward_vs_oracle
grad_loc leaves out samples within 1e-3 px of an integer coordinate (it jumps there), at most 1 % of a case's samples.
Every test prints ``RATIO <list> <dtype> <quantity> <worst error / bound>``.
"""
import contextlib

import numpy as np
import pytest
import torch

import alo_hip
import msda_plan_cases as T
import oracle as O
from guarded import GuardedLaunches
from helpers import level_start
from test_msda_f16_gpu import assert_forward_bound, prologue64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (rtol, atol) of |got - want| <= atol + rtol |want|; grad_loc's atol of fp32 / fp16 scales with max(1, |want|max)
BARS = {
    "f32": dict(out=(1e-5, 1e-5), gv=(1e-4, 2e-5), gl=(1e-4, 2e-5, True), ga=(1e-4, 1e-4)),
    "f64": dict(out=(1e-11, 1e-11), gv=(1e-11, 1e-11), gl=(1e-10, 1e-9, False), ga=(1e-11, 1e-11)),
    "bf16": dict(out=(2.0 ** -8, 1e-6), gv=(2.0 ** -7, 1e-3), gl=(1e-4, 1e-3, False), ga=(1e-4, 1e-4)),
    "f16": dict(out=(2.0 ** -11, 1e-6), gv=(2.0 ** -10, 2e-5), gl=(1e-4, 2e-5, True), ga=(1e-4, 1e-4)),
}


def host64(x):
    return x.double().cpu().numpy()


def held(c, quantity, got, want, rtol, atol):
    err, bound = np.abs(got - want), atol + rtol * np.abs(want)
    print(f"RATIO {c.group} {c.dtype} {quantity} {np.max(err / bound):.4f}   ({c.name}, {err.size} elements)")
    assert np.all(err <= bound), f"{c.name} {quantity}: {(~(err <= bound)).sum()} of {err.size} beyond atol {atol:g} + rtol {rtol:g}"


def held_forward(c, quantity, out, want):
    assert out.dtype == T.TORCH[c.dtype] and tuple(out.shape) == (c.N, c.Lq, c.M * c.D)
    if c.dtype == "f16":
        assert_forward_bound(out, want, f"{c.name} {quantity}")
    held(c, quantity, host64(out), want, *BARS[c.dtype]["out"])


def place(t, k=0):
    """``t`` on the GPU as a contiguous view that starts ``k`` elements into its allocation."""
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=DEV)
    view = buf[k:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + k * t.element_size() and buf.data_ptr() % 16 == 0
    return view


# ---- inputs and oracle results of the case at hand: the kinds of a case run one after the other and share them ----------------
_cache = {}


def case_data(c):
    if _cache.get("name") != c.name:
        _cache.clear()
        _cache["name"] = c.name
        _cache["shapes"] = np.asarray(c.levels, np.int32)
        _cache["start"] = level_start(c.levels)
        _cache["value"] = T.draw_value(c)
    return _cache


def metadata(d):
    return torch.from_numpy(d["shapes"]).to(DEV), torch.from_numpy(d["start"]).to(DEV)


def plain_inputs(c, d):
    if "loc" not in d:
        d["loc"], d["attn"] = T.draw_loc(c), T.draw_attn(c)
    return d["loc"], d["attn"]


def assert_plan(c, fused=0):
    got = T.query(alo_hip.lib(), c, fused)
    assert got[:5] == c.claim, f"{c.name} claims {c.claim}, the library plans {got[:5]}"


@contextlib.contextmanager
def launches(guarded, symbol):
    if not guarded:
        yield
        return
    with GuardedLaunches() as g:
        yield
    assert [s for s, _ in g.seen] == [symbol], g.seen


def run_plain(c, guarded=False):
    d = case_data(c)
    assert_plan(c)
    loc, attn = plain_inputs(c, d)
    if "ref_plain" not in d:
        d["ref_plain"] = O.msda_forward(host64(d["value"]), d["shapes"], d["start"], loc.astype(np.float64), attn.astype(np.float64))
    shapes, start = metadata(d)
    value = place(d["value"], c.off.get("value", 0))
    tl, ta = place(torch.from_numpy(loc), c.off.get("loc", 0)), place(torch.from_numpy(attn), c.off.get("attn", 0))
    with launches(guarded, "alo_msda_forward"):
        if "out" in c.off:   # the wrapper allocates its own output: the entry point directly, as tests/test_msda_f16_gpu.py does
            out = place(torch.zeros(c.N, c.Lq, c.M * c.D, dtype=T.TORCH[c.dtype]), c.off["out"])
            alo_hip._launch("alo_msda_forward", value.device, None, 0.0, 0.0, value, shapes, start, tl, ta, out, c.N, T.n_pixels(c), c.M,
                            c.D, T.n_levels(c), c.Lq, c.P, T.CODE[c.dtype], T.CODE["f64" if c.dtype == "f64" else "f32"])
        else:
            out = alo_hip.msda_forward(value, shapes, start, tl, ta, 64)
    held_forward(c, "forward", out, d["ref_plain"])


def run_fused(c, ref_dim, guarded=False):
    d = case_data(c)
    assert_plan(c, fused=1)
    offsets, logits, ref = T.draw_fused(c, ref_dim)
    loc, attn = prologue64(offsets, logits, ref, c.levels, c.P)
    want = O.msda_forward(host64(d["value"]), d["shapes"], d["start"], loc, attn)
    shapes, start = metadata(d)
    value = place(d["value"], c.off.get("value", 0))
    with launches(guarded, "alo_msda_forward_fused"):
        out = alo_hip.msda_forward_fused(value, shapes, start, place(offsets, c.off.get("loc", 0)), place(logits, c.off.get("attn", 0)),
                                         place(ref, c.off.get("ref", 0)))
    held_forward(c, f"fused{ref_dim}", out, want)


def run_backward(c, guarded=False):
    d = case_data(c)
    assert_plan(c)
    loc, attn = plain_inputs(c, d)
    grad_out = T.draw_grad_out(c)
    rgv, rgl, rga = O.msda_backward(host64(d["value"]), d["shapes"], d["start"], loc.astype(np.float64), attn.astype(np.float64),
                                    host64(grad_out))
    shapes, start = metadata(d)
    assert c.hint == alo_hip._wide_backward_wants_host_shapes(d["value"], (c.N, T.n_pixels(c), c.M, c.D, T.n_levels(c), c.Lq, c.P), alo_hip.ALO_F32)
    with launches(guarded, "alo_msda_backward_hinted"):
        gv, gl, ga = alo_hip.msda_backward(place(d["value"], c.off.get("value", 0)), shapes, start, place(torch.from_numpy(loc), c.off.get("loc", 0)),
                                           place(torch.from_numpy(attn), c.off.get("attn", 0)), place(grad_out, c.off.get("grad_out", 0)), 64)
    geo = torch.float64 if c.dtype == "f64" else torch.float32
    assert (gv.dtype, gl.dtype, ga.dtype) == (T.TORCH[c.dtype], geo, geo)
    bars = BARS[c.dtype]
    held(c, "grad_value", host64(gv), rgv, *bars["gv"])
    held(c, "grad_attn", host64(ga), rga, *bars["ga"])
    smooth = T.smooth_samples(c, loc)
    share = (~smooth).mean()
    print(f"MASKED {c.group} {c.dtype} {share:.5f}   ({c.name}: {(~smooth).sum()} of {smooth.size} samples within 1e-3 px of an integer coordinate)")
    assert share <= 0.01
    rtol, atol, scaled = bars["gl"]
    held(c, "grad_loc", host64(gl)[smooth], rgl[smooth], rtol, atol * (max(1.0, np.abs(rgl).max()) if scaled else 1.0))


def run(c, kind, guarded=False):
    if kind == "plain":
        run_plain(c, guarded)
    elif kind == "bwd":
        run_backward(c, guarded)
    else:
        run_fused(c, int(kind[-1]), guarded)


def _runs(group):
    return [pytest.param(c, kind, id=f"{c.name}-{kind}") for c, kind in T.RUNS if c.group == group]


@pytest.mark.parametrize("c,kind", _runs("A"))
def test_every_instantiation_one_run_per_block(c, kind):
    run(c, kind)


@pytest.mark.parametrize("c,kind", _runs("B"))
def test_several_runs_per_block(c, kind):
    run(c, kind)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain-buffers", "guarded"])
@pytest.mark.parametrize("c,kind", _runs("C"))
def test_unaligned_operands(c, kind, guarded):
    run(c, kind, guarded)


def test_head_major_forward_refuses_unaligned_offsets():
    """The bf16 launch of list C (L = P = 4, D = 32, offsets / logits / reference points one element in) on a head-major value: only
    the wave kernel serves that layout and it needs aligned operands, so the library refuses and says why."""
    c = T.BY_NAME["C-loc+1-bf16-L4P4-D32"]
    d = case_data(c)
    shapes, start = metadata(d)
    offsets, logits, ref = T.draw_fused(c, 2)
    vhm = alo_hip.value_head_major(place(d["value"]))
    assert alo_hip.head_major_supported(vhm.permute(0, 2, 1, 3), 4, 4)
    out = alo_hip.msda_forward_fused_hm(vhm, shapes, start, place(offsets), place(logits), place(ref), resident=False)   # aligned: served
    held_forward(c, "fused2-head-major-aligned", out, O.msda_forward(host64(d["value"]), d["shapes"], d["start"],
                                                                      *prologue64(offsets, logits, ref, c.levels, c.P)))
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        with pytest.raises(RuntimeError, match="alo_msda_forward_fused_hm: needs bf16 / fp16, L = P = 4, D % 8 == 0, D <= 32 and 16-byte aligned pointers"):
            alo_hip.msda_forward_fused_hm(vhm, shapes, start, place(offsets, off[0]), place(logits, off[1]), place(ref, off[2]), resident=False)
