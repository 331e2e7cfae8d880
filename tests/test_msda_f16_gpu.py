"""fp16 values in the multi-scale deformable attention op: the generic forward / backward kernels, the matrix-pipe (wave) forward on
a head-major value, and the operator boundary, against the float64 oracle fed the SAME fp16-rounded inputs.

Bounds (derived, not measured):
  forward     |out - ref| <= 2^-11 |ref| + 1e-6   half an fp16 ulp of the final rounding + the fp32 noise the bf16 test allows
  grad_value  rtol 2^-10, atol 2e-5               one fp16 ulp of the final rounding + the fp32 test's atomic-order allowance
  grad_loc    rtol 1e-4, atol 2e-5 max(1, |ref|max)   } the fp32 bars of test_forward_backward_vs_oracle: these outputs are fp32,
  grad_attn   rtol 1e-4, atol 1e-4                     } computed from exactly widened values
"""
import numpy as np
import pytest
import torch

import alo_hip
import oracle as O
from helpers import level_start, msda_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
WAVE_LEVELS = [(7, 9), (4, 5), (2, 3), (1, 2)]   # odd sizes and a level one pixel high


def dev(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x.to(dtype) if dtype is not None else x


def host64(x):
    return x.double().cpu().numpy()


def assert_forward_bound(out, ref, what=""):
    out = host64(out)
    err, bound = np.abs(out - ref), 2.0 ** -11 * np.abs(ref) + 1e-6
    with np.errstate(invalid="ignore"):
        print(f"{what}: worst error / bound = {np.nanmax(err / bound):.3f} over {err.size} outputs")
    assert np.all(err <= bound), f"{what}: {(err > bound).sum()} of {err.size} outputs beyond half an fp16 ulp + 1e-6"


def prologue64(offsets, logits, ref, shapes, P):
    """MSDeformAttn's arithmetic between its linear layers and the op (ms_deform_attn.py:119-133) in float64, on the values the
    kernel is given (fp16 offsets and logits, fp32 reference points)."""
    off, lg, r = host64(offsets), host64(logits), host64(ref)
    N, Lq, M, L = off.shape[:4]
    e = np.exp(lg - lg.max(-1, keepdims=True))
    attn = (e / e.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P)
    if r.shape[-1] == 2:
        wh = np.asarray(shapes, np.float64)[:, ::-1]
        loc = r[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    else:
        loc = r[:, :, None, :, None, :2] + off / P * r[:, :, None, :, None, 2:] * 0.5
    return loc, attn


# ---- generic kernels --------------------------------------------------------------------------------------------------------
GENERIC = [  # (N, M, D, Lq, levels, P)            plan
    (1, 3, 30, 21, [(6, 4), (3, 2)], 2),           # scalar path
    (2, 2, 64, 19, [(6, 5), (3, 3), (2, 2)], 2),   # vec8, group 8
    (1, 1, 256, 9, [(5, 5)], 3),                   # vec8, group 64
    (2, 4, 16, 33, [(9, 7), (5, 4)], 8),           # vec8, group 4, the unrolled L*P = 16 stage
]
_generic_cache = {}


def generic_case(case):
    """Inputs rounded to fp16 where the op takes fp16, and the oracle's outputs on exactly those; computed once per case."""
    key = (case[0], case[1], case[2], case[3], case[5])
    if key not in _generic_cache:
        N, M, D, Lq, levels, P = case
        c = msda_case(4321 + D + Lq, N, M, D, Lq, levels, P, np.float32, loc_range=(-0.3, 1.3))
        c["value"] = c["value"].astype(np.float16)
        c["grad_out"] = c["grad_out"].astype(np.float16)
        w = [c[k].astype(np.float64) for k in ("value", "loc", "attn", "grad_out")]
        c["ref"] = O.msda_forward(w[0], c["shapes"], c["level_start"], w[1], w[2])
        c["rgv"], c["rgl"], c["rga"] = O.msda_backward(w[0], c["shapes"], c["level_start"], w[1], w[2], w[3])
        _generic_cache[key] = c
    return _generic_cache[key]


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: f"N{c[0]}M{c[1]}D{c[2]}L{len(c[4])}P{c[5]}")
def test_generic_forward_vs_oracle(case):
    c = generic_case(case)
    out = alo_hip.msda_forward(dev(c["value"]), dev(c["shapes"]), dev(c["level_start"]), dev(c["loc"]), dev(c["attn"]), 64)
    assert out.dtype == F16
    assert_forward_bound(out, c["ref"], "alo_msda_forward")


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("case", GENERIC, ids=lambda c: f"N{c[0]}M{c[1]}D{c[2]}L{len(c[4])}P{c[5]}")
def test_generic_fused_forward_vs_oracle(case, ref_dim):
    N, M, D, Lq, levels, P = case
    L = len(levels)
    gen = torch.Generator(device=DEV).manual_seed(55 + D + ref_dim)
    shapes, start = dev(np.asarray(levels, np.int32)), dev(level_start(levels))
    S = sum(h * w for h, w in levels)
    value = torch.randn(N, S, M, D, generator=gen, device=DEV).half()
    offsets = (torch.randn(N, Lq, M, L, P, 2, generator=gen, device=DEV) * 2.5).half()
    logits = (torch.randn(N, Lq, M, L * P, generator=gen, device=DEV) * 2.0).half()
    ref = torch.rand(N, Lq, L, ref_dim, generator=gen, device=DEV)
    if ref_dim == 4:
        ref[..., 2:] *= 0.4
    out = alo_hip.msda_forward_fused(value, shapes, start, offsets, logits, ref)
    assert out.dtype == F16
    loc, attn = prologue64(offsets, logits, ref, levels, P)
    exact = O.msda_forward(host64(value), np.asarray(levels, np.int32), level_start(levels), loc, attn)
    assert_forward_bound(out, exact, f"alo_msda_forward_fused ref_dim={ref_dim}")


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: f"N{c[0]}M{c[1]}D{c[2]}L{len(c[4])}P{c[5]}")
def test_generic_backward_vs_oracle(case):
    c = generic_case(case)
    N, S, M, D = c["value"].shape
    _, Lq, _, L, P, _ = c["loc"].shape
    assert alo_hip.lib().alo_msda_backward_path(N, S, M, D, L, Lq, P, alo_hip.ALO_F16, alo_hip.ALO_F32, None) == 0
    gv, gl, ga = alo_hip.msda_backward(dev(c["value"]), dev(c["shapes"]), dev(c["level_start"]), dev(c["loc"]), dev(c["attn"]),
                                       dev(c["grad_out"]), 64)
    assert (gv.dtype, gl.dtype, ga.dtype) == (F16, torch.float32, torch.float32)
    gv, gl, ga = host64(gv), host64(gl), host64(ga)
    for name, got, want in (("grad_value", gv, c["rgv"]), ("grad_attn", ga, c["rga"])):
        print(f"{name}: max abs error {np.abs(got - want).max():.3e}, |ref| max {np.abs(want).max():.3e}")
    np.testing.assert_allclose(gv, c["rgv"], rtol=2.0 ** -10, atol=2e-5)
    np.testing.assert_allclose(ga, c["rga"], rtol=1e-4, atol=1e-4)
    # grad_loc jumps where an image coordinate crosses an integer: samples within 1e-3 px of one are left out
    size = np.asarray(c["shapes"], np.float64)[:, ::-1].reshape(1, 1, 1, L, 1, 2)
    t = c["loc"].astype(np.float64) * size - 0.5
    smooth = (np.abs(t - np.round(t)) >= 1e-3).all(-1)
    scale = max(1.0, np.abs(c["rgl"]).max())
    print(f"grad_loc: max abs error {np.abs(gl - c['rgl'])[smooth].max():.3e}, |ref| max {scale:.3e}, {(~smooth).sum()} samples on an edge")
    np.testing.assert_allclose(gl[smooth], c["rgl"][smooth], rtol=1e-4, atol=2e-5 * scale)


# ---- the matrix-pipe (wave) kernel: head-major fp16 values -------------------------------------------------------------------
# Only alo_msda_forward_fused_hm serves a head-major value, and only with the wave kernel (anything else is refused), so a result
# from that entry point IS the wave kernel's.  Pixel-major fp16 launches of the same shapes take the generic kernel.
WAVE = [(2, 3, 32, 37), (1, 8, 8, 16), (1, 2, 24, 300)]   # (N, M, D, Lq): two full 16-query runs + a tail of 5, odd head count; ...


def wave_inputs(N, M, D, Lq, ref_dim, seed=0, logit_scale=2.0):
    gen = torch.Generator(device=DEV).manual_seed(900 + seed + D + Lq + ref_dim)
    shapes, start = dev(np.asarray(WAVE_LEVELS, np.int32)), dev(level_start(WAVE_LEVELS))
    S = sum(h * w for h, w in WAVE_LEVELS)
    value = torch.randn(N, S, M, D, generator=gen, device=DEV).half()
    offsets = (torch.randn(N, Lq, M, 4, 4, 2, generator=gen, device=DEV) * 2.5).half()
    logits = (torch.randn(N, Lq, M, 16, generator=gen, device=DEV) * logit_scale).half()
    ref = torch.rand(N, Lq, 4, ref_dim, generator=gen, device=DEV)
    if ref_dim == 4:
        ref[..., 2:] *= 0.4
    mask = torch.rand(N, S, generator=gen, device=DEV) < 0.3
    return value, shapes, start, offsets, logits, ref, mask


def oracle_fused(value, offsets, logits, ref):
    loc, attn = prologue64(offsets, logits, ref, WAVE_LEVELS, 4)
    return O.msda_forward(host64(value), np.asarray(WAVE_LEVELS, np.int32), level_start(WAVE_LEVELS), loc, attn), loc, attn


def run_route(route, value, shapes, start, offsets, logits, ref):
    """The fused forward on a pixel-major ``value`` through the wave kernel (re-laid head-major first) or the generic one."""
    if route == "wave":
        return alo_hip.msda_forward_fused_hm(alo_hip.value_head_major(value), shapes, start, offsets, logits, ref)
    return alo_hip.msda_forward_fused(value, shapes, start, offsets, logits, ref)


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("N,M,D,Lq", WAVE)
def test_wave_kernel_head_major_vs_oracle_dense_sliced_and_never_resident(N, M, D, Lq, ref_dim):
    value, shapes, start, offsets, logits, ref, mask = wave_inputs(N, M, D, Lq, ref_dim)
    masked = value.masked_fill(mask[..., None, None], 0)
    exact, loc, attn = oracle_fused(masked, offsets, logits, ref)
    assert alo_hip.head_major_supported(value, 4, 4)
    vhm = alo_hip.value_head_major(value, mask)
    assert vhm.dtype == F16 and torch.equal(vhm, masked.permute(0, 2, 1, 3))
    assert torch.equal(alo_hip.value_head_major(value, None), value.permute(0, 2, 1, 3))
    dense = alo_hip.msda_forward_fused_hm(vhm, shapes, start, offsets, logits, ref, resident=False)
    assert dense.dtype == F16
    assert_forward_bound(dense, exact, "wave head-major, dense offsets / logits")
    # the same launch on the pixel-major value: the generic kernel, held to the same bound (the two are not bit-identical)
    assert_forward_bound(alo_hip.msda_forward_fused(masked, shapes, start, offsets, logits, ref), exact, "generic pixel-major, fused")
    loc32, attn32 = dev(loc, torch.float32), dev(attn, torch.float32)
    exact_plain = O.msda_forward(host64(masked), np.asarray(WAVE_LEVELS, np.int32), level_start(WAVE_LEVELS), host64(loc32), host64(attn32))
    assert_forward_bound(alo_hip.msda_forward(masked, shapes, start, loc32, attn32, 64), exact_plain, "generic pixel-major, plain")
    # offsets and logits as column slices of one merged buffer (the _hm_rows strides)
    both = torch.cat([offsets.reshape(N, Lq, -1), logits.reshape(N, Lq, -1)], -1).contiguous()
    off_s = both[..., :M * 32].view(N, Lq, M, 4, 4, 2)
    log_s = both[..., M * 32:].view(N, Lq, M, 16)
    assert not off_s.is_contiguous() and not log_s.is_contiguous()
    assert torch.equal(alo_hip.msda_forward_fused_hm(vhm, shapes, start, off_s, log_s, ref, resident=False), dense)
    # with a host copy of the shapes attached and the resident kernel demanded: fp16 still takes the plain head-major kernel
    shapes._alo_shapes = [tuple(hw) for hw in WAVE_LEVELS]
    with alo_hip.LaunchTimer() as timer:
        always = alo_hip.msda_forward_fused_hm(vhm, shapes, start, off_s, log_s, ref, resident="always")
    assert list(timer.summary()) == [f"msda_fwd_fused/Lq={Lq}"]
    assert torch.equal(always, dense)
    if D == 32:   # the library's own answer to a hinted fp16 launch, under either policy
        import ctypes
        host = (ctypes.c_int32 * 8)(*[v for hw in WAVE_LEVELS for v in hw])
        for policy in (alo_hip.RESIDENT_AUTO, alo_hip.RESIDENT_ALWAYS):
            out = torch.empty_like(dense)
            alo_hip._launch("alo_msda_forward_fused_hm_resident", vhm.device, None, 0.0, 0.0, vhm, shapes, start, off_s, log_s,
                            both.stride(1), both.stride(1), ref, out, N, vhm.shape[2], M, D, 4, Lq, 4, ref_dim, alo_hip.ALO_F16, host, policy)
            assert torch.equal(out, dense)


def test_fp16_stays_off_the_resident_kernel_at_a_shape_bf16_takes_it():
    """D = 32 and 13 runs of 16 queries per (image, head) slab: the smallest launch the LDS-resident kernel serves, which a bf16 launch
    of these dimensions does under ALO_RESIDENT_ALWAYS.  That kernel reads bf16 bits, so an fp16 launch that reached it would be
    silently wrong: with the host shapes attached, through the Python wrapper and through the resident entry point itself under
    both policies, fp16 must be the plain head-major kernel's bits and meet the oracle."""
    import ctypes

    N, M, D, Lq, ref_dim = 1, 2, 32, 208, 2
    value, shapes, start, offsets, logits, ref, mask = wave_inputs(N, M, D, Lq, ref_dim, seed=4)
    S = value.shape[1]
    host = (ctypes.c_int32 * 8)(*[v for hw in WAVE_LEVELS for v in hw])
    assert alo_hip.lib().alo_msda_resident_levels(host, N, S, M, 4, Lq, alo_hip.RESIDENT_ALWAYS) == 2
    shapes._alo_shapes = [tuple(hw) for hw in WAVE_LEVELS]
    # bf16 on the same tensors does go resident: the shape is one the guard is needed for
    vhm_bf16 = alo_hip.value_head_major(value.bfloat16(), mask)
    with alo_hip.LaunchTimer() as timer:
        alo_hip.msda_forward_fused_hm(vhm_bf16, shapes, start, offsets.bfloat16(), logits.bfloat16(), ref, resident="always")
    assert list(timer.summary()) == [f"msda_fwd_fused_resident/Lq={Lq}"]
    vhm = alo_hip.value_head_major(value, mask)
    exact, _, _ = oracle_fused(value.masked_fill(mask[..., None, None], 0), offsets, logits, ref)
    plain = alo_hip.msda_forward_fused_hm(vhm, shapes, start, offsets, logits, ref, resident=False)
    assert_forward_bound(plain, exact, "fp16 head-major, resident=False")
    for resident in (True, "always"):
        with alo_hip.LaunchTimer() as timer:
            out = alo_hip.msda_forward_fused_hm(vhm, shapes, start, offsets, logits, ref, resident=resident)
        assert list(timer.summary()) == [f"msda_fwd_fused/Lq={Lq}"]
        assert torch.equal(out, plain)
    for policy in (alo_hip.RESIDENT_AUTO, alo_hip.RESIDENT_ALWAYS):   # the library's own guard, without the wrapper's
        out = torch.full_like(plain, float("nan"))
        alo_hip._launch("alo_msda_forward_fused_hm_resident", vhm.device, None, 0.0, 0.0, vhm, shapes, start, offsets, logits,
                        M * 32, M * 16, ref, out, N, S, M, D, 4, Lq, 4, ref_dim, alo_hip.ALO_F16, host, policy)
        assert torch.equal(out, plain)
        assert_forward_bound(out, exact, f"fp16 through alo_msda_forward_fused_hm_resident, policy {policy}")


@pytest.mark.parametrize("gap", [12.0, 25.0])
@pytest.mark.parametrize("route", ["wave", "generic"])
def test_attention_mass_on_samples_outside_the_map(route, gap):
    """Levels 1-3 sampled far outside the map with logits ``gap`` above level 0's: almost all of a pair's attention sits on corners
    that are never read.  The wave kernel's weight scale must come from the weights that meet a value (e^-12 / 12 and e^-25 / 12
    of the total here), and the weights of unread corners must not overflow under it."""
    N, M, D, Lq = 1, 3, 32, 37
    value, shapes, start, offsets, logits, ref, _ = wave_inputs(N, M, D, Lq, 2, seed=6)
    ref[:, :, 1:] = 100.0
    logits = logits.view(N, Lq, M, 4, 4).clone()
    logits[..., 1:, :] += gap
    logits = logits.view(N, Lq, M, 16).contiguous()
    value = (value.float() * 1000.0).half()   # outputs of e^-gap / 12 x 1000: above fp16's subnormal step for the smaller gap
    exact, _, attn = oracle_fused(value, offsets, logits, ref)
    assert attn[..., 0, :].sum(-1).max() < np.exp(4.0 - gap)   # the inputs are what the test is about (the logits' own spread is +-2)
    out = run_route(route, value, shapes, start, offsets, logits, ref)
    assert torch.isfinite(out).all()
    if gap == 12.0:
        assert np.abs(exact).max() > 1e-3
    assert_forward_bound(out, exact, f"{route}, attention mass outside the map, gap {gap}")


@pytest.mark.parametrize("route", ["wave", "generic"])
def test_small_magnitudes_subnormal_values_and_tiny_attention_weights(route):
    """Values in +-[1e-6, 6e-5] (fp16 subnormals) and logits spread so that some attention weights are below 2^-14: pins the
    pre-scale of the weight split and what the matrix pipe does with subnormal operands."""
    N, M, D, Lq = 2, 3, 32, 37
    value, shapes, start, offsets, logits, ref, _ = wave_inputs(N, M, D, Lq, 2, seed=2, logit_scale=6.0)
    gen = torch.Generator(device=DEV).manual_seed(17)
    mag = torch.empty(value.shape, device=DEV).uniform_(1e-6, 6e-5, generator=gen)
    value = (mag * (torch.rand(value.shape, generator=gen, device=DEV) < 0.5).float().mul(2).sub(1)).half()
    assert value.abs().max().item() < 2.0 ** -14 and value.abs().min().item() > 0
    exact, loc, attn = oracle_fused(value, offsets, logits, ref)
    assert (attn < 2.0 ** -14).mean() > 0.05 and np.abs(exact).max() > 1e-5
    out = run_route(route, value, shapes, start, offsets, logits, ref)
    assert_forward_bound(out, exact, f"{route}, subnormal values")
    # the same launch with the values scaled by 2^10 (exact in fp16, normal numbers): the relative form of the bound alone, so that
    # the 1e-6 allowance cannot hide a flushed operand or a weight term that sank below fp16's range
    big = (value.float() * 1024.0).half()
    assert torch.equal(big.float(), value.float() * 1024.0)
    assert_forward_bound(run_route(route, big, shapes, start, offsets, logits, ref), exact * 1024.0, f"{route}, the same values x 2^10")
    err = np.abs(host64(out) - exact)
    lsb = 2.0 ** -24   # the spacing of fp16 subnormals: outputs below 2^-14 cannot be closer than half of it
    assert np.all(err <= np.maximum(2.0 ** -11 * np.abs(exact), lsb / 2) + 1e-9), f"{route}: subnormal outputs beyond half an fp16 step"


@pytest.mark.parametrize("route", ["wave", "generic"])
def test_range_and_non_finite_values(route):
    N, M, D, Lq = 1, 2, 32, 21
    value, shapes, start, offsets, logits, ref, _ = wave_inputs(N, M, D, Lq, 2, seed=3)
    run = lambda v, r=ref: run_route(route, v, shapes, start, offsets, logits, r)  # noqa: E731
    # (1) +-60000 everywhere: the weights of a query sum to at most 1, so every output fits fp16
    out = run(torch.where(value > 0, 60000.0, -60000.0).half())
    assert torch.isfinite(out).all() and out.abs().max().item() > 1000.0
    # (2) every sample outside the map, the map all NaN: nothing is read
    far = torch.full_like(ref, 100.0)   # offsets reach a few map widths on the 2- and 3-pixel levels, never a hundred
    assert (run(torch.full_like(value, float("nan")), far) == 0).all()
    # (3) NaN / inf at a few pixels: exactly the outputs the oracle makes non-finite are non-finite, the others keep the bound
    gen = torch.Generator(device=DEV).manual_seed(5)
    hit = torch.rand(value.shape[:3], generator=gen, device=DEV) < 0.04
    bad = value.clone()
    bad[hit] = float("nan")
    bad[torch.roll(hit, 1, 1)] = float("inf")
    with np.errstate(invalid="ignore"):
        want, _, _ = oracle_fused(bad, offsets, logits, ref)
    got = host64(run(bad))
    assert (~np.isfinite(want)).any() and np.isfinite(want).any()
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 2.0 ** -11 * np.abs(want[fin]) + 1e-6)


def test_the_other_library_kernels_stay_closed_to_fp16():
    """``_DTYPE_CODE`` knows fp16 now, so the gates in front of its other users must keep naming fp32 / bf16."""
    x = torch.zeros(4, 256, dtype=F16, device=DEV)
    assert alo_hip.fusable(x.float()) and alo_hip.fusable(x.bfloat16()) and not alo_hip.fusable(x)   # add_layernorm, bias_act_, pos_sine_flat
    keep = torch.ones(4, dtype=torch.bool, device=DEV)
    assert alo_hip.mask_rows_supported(x.bfloat16(), keep) and not alo_hip.mask_rows_supported(x, keep)
    coords, topk = torch.zeros(1, 8, 4, device=DEV), torch.zeros(1, 2, dtype=torch.int64, device=DEV)
    assert alo_hip.proposal_queries_supported(coords, topk, torch.bfloat16) and not alo_hip.proposal_queries_supported(coords, topk, F16)
    w = torch.zeros(256, 256, dtype=F16, device=DEV)
    assert not alo_hip.linear_shortk_supported(x, w) and not alo_hip.linear_packed_supported(x, w)
    assert not alo_hip.value_proj_head_major_supported(x[None], w, 8)


# ---- operator boundary ----------------------------------------------------------------------------------------------------
def test_dispatcher_op_and_autograd_function():
    from alonet.deformable_detr.ops.functions import MSDeformAttnFunction, load_ops

    load_ops()
    c = generic_case(GENERIC[1])
    args = (dev(c["value"]), dev(c["shapes"]), dev(c["level_start"]), dev(c["loc"]), dev(c["attn"]))
    out = torch.ops.alonet_custom.ms_deform_attn_forward(*args, 64)
    assert out.dtype == F16
    assert_forward_bound(out, c["ref"], "torch.ops.alonet_custom.ms_deform_attn_forward")
    value, loc, attn = args[0].clone().requires_grad_(True), args[3].clone().requires_grad_(True), args[4].clone().requires_grad_(True)
    res = MSDeformAttnFunction.apply(value, args[1], args[2], loc, attn, 64)
    assert torch.equal(res, out)
    res.backward(dev(c["grad_out"]))
    assert (value.grad.dtype, loc.grad.dtype, attn.grad.dtype) == (F16, torch.float32, torch.float32)
    np.testing.assert_allclose(host64(value.grad), c["rgv"], rtol=2.0 ** -10, atol=2e-5)
    np.testing.assert_allclose(host64(attn.grad), c["rga"], rtol=1e-4, atol=1e-4)


def _g4_module(golden):
    from alonet.deformable_detr.ops.modules import MSDeformAttn

    g = golden("g4_msda_module.npz")
    d_model, n_levels, n_heads, n_points = (int(x) for x in g["cfg"])
    m = MSDeformAttn(d_model, n_levels, n_heads, n_points).double()
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")})
    return g, m


def test_module_in_half_at_inference(golden):
    """The G4 module (the reference module's own float64 outputs) in ``.half()``: every linear layer and the gather in fp16.
    Two yardsticks, neither taken from the fp16 run: the bf16 run of the same call (fp16 carries three more bits through the same
    chain, so it must not be worse), and a rounding budget of 16 x 2^-11 of the largest output — the module is three chained
    stages (value_proj | offsets + logits, the gather, output_proj) and each rounds its inputs, its weights and its result once."""
    errs = {}
    for dtype in (F16, torch.bfloat16):
        g, m = _g4_module(golden)
        md = m.to(DEV, dtype).eval()
        shapes = dev(g["shapes"]).to(torch.int32)
        with alo_hip.LaunchTimer() as timer, torch.no_grad():
            outs = [md(dev(g["query"], dtype), dev(g[r], dtype), dev(g["src"], dtype), shapes, dev(g["level_start"]), dev(g["mask"]))
                    for r in ("ref2", "ref4")]
        assert any(k.startswith("msda_fwd_fused") for k in timer.summary())
        assert all(o.dtype == dtype for o in outs)
        errs[dtype] = [np.abs(host64(o) - g[k]).max() for o, k in zip(outs, ("out2", "out4"))]
    print("G4 module max-abs vs the reference, (ref_dim 2, ref_dim 4): fp16", errs[F16], "bf16", errs[torch.bfloat16])
    for e16, eb16, k in zip(errs[F16], errs[torch.bfloat16], ("out2", "out4")):
        assert e16 <= eb16 and e16 <= 16 * 2.0 ** -11 * np.abs(g[k]).max(), (k, e16, eb16)


def test_module_with_fp32_parameters_under_fp16_autocast(golden):
    g, m = _g4_module(golden)
    m = m.to(DEV).float().train()
    shapes = dev(g["shapes"]).to(torch.int32)
    query, src = dev(g["query"], torch.float32), dev(g["src"], torch.float32)
    with alo_hip.LaunchTimer() as timer, torch.autocast("cuda", dtype=F16):
        out = m(query, dev(g["ref2"], torch.float32), src, shapes, dev(g["level_start"]), dev(g["mask"]))
    assert out.dtype == F16
    assert any(k.startswith("msda_fwd/") for k in timer.summary())
    err = np.abs(host64(out.detach()) - g["out2"]).max()
    print(f"G4 module, fp32 parameters under fp16 autocast: max-abs {err:.3e}")
    assert err <= 16 * 2.0 ** -11 * np.abs(g["out2"]).max()   # the rounding budget of test_module_in_half_at_inference
    with alo_hip.LaunchTimer() as timer:
        out.float().square().sum().backward()
    assert any(k.startswith("msda_bwd/") for k in timer.summary())
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), name
    assert m.value_proj.weight.grad.abs().max().item() > 0 and m.sampling_offsets.weight.grad.abs().max().item() > 0
