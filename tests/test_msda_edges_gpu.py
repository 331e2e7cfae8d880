"""MSDA on pixel edges, on every kernel route: the samples a fresh model takes and exactly constructed edges.

grad_sampling_loc jumps where loc * size - 0.5 crosses an integer.  A freshly initialised MSDeformAttn samples there all the time:
its offsets start as integer pixel rings (ms_deform_attn.py, _reset_parameters) around the encoder's pixel-centre reference points.
Each backward route (msda_bwd_wide_kernel, msda_bwd_tiled_kernel's encoder and consecutive-query routes, the per-corner
msda_bwd_kernel) is asserted through alo_msda_backward_path and compared on EVERY sample with helpers.grad_loc_reference, which
knows which side of an edge the reference's float32 mapping takes."""
import ctypes

import numpy as np
import pytest
import torch

import alo_hip
import oracle as O
from helpers import (DETR_SHAPES, DYADIC_SHAPES, _edge_sizes, assert_one_of, exact_edge_case, grad_loc_one_sided, grad_loc_reference,
                     level_start)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_CORNER, TILED, WIDE = 0, 1, 2
SMALL_SHAPES = [(25, 42), (13, 21), (7, 11), (4, 6)]   # the DETR pyramid's coarse end: odd sizes, S = 1424

# route: (value dtype, hand the host copy of the shapes?, ALO_MSDA_BWD, D, expected path)
ROUTES = {
    "wide_f32": (torch.float32, True, None, 32, WIDE),
    "wide_bf16": (torch.bfloat16, True, None, 32, WIDE),
    "wide_d64": (torch.float32, True, None, 64, WIDE),
    "tiled_encoder": (torch.float32, True, "tiled", 32, TILED),
    "tiled_rows": (torch.float32, False, None, 32, TILED),
    "per_corner_f32_d64": (torch.float32, False, None, 64, PER_CORNER),
    "per_corner_bf16": (torch.bfloat16, False, None, 32, PER_CORNER),
    "per_corner_f64": (torch.float64, False, None, 32, PER_CORNER),
}


def dev(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x.to(dtype) if dtype is not None else x


def backward(c, route, monkeypatch):
    """Launch route ``route`` on case ``c`` through the C ABI (after asserting the path) -> float64 numpy gradients, and the case
    the kernel saw (bf16-rounded value / grad_out)."""
    dtype, hinted, env, D, path = ROUTES[route]
    if env is not None:
        monkeypatch.setenv("ALO_MSDA_BWD", env)
    else:
        monkeypatch.delenv("ALO_MSDA_BWD", raising=False)
    N, S, M, Dc = c["value"].shape
    _, Lq, _, L, P, _ = c["loc"].shape
    assert Dc == D
    shapes_l = [tuple(int(v) for v in hw) for hw in c["shapes"]]
    hint = (ctypes.c_int32 * (2 * L))(*[v for hw in shapes_l for v in hw]) if hinted else None
    vdt = alo_hip._DTYPE_CODE[dtype]
    gdt = torch.float64 if dtype == torch.float64 else torch.float32
    ldt = alo_hip._DTYPE_CODE[gdt]
    assert alo_hip.lib().alo_msda_backward_path(N, S, M, D, L, Lq, P, vdt, ldt, hint) == path, route
    value, go = dev(c["value"], dtype), dev(c["grad_out"], dtype)
    loc, attn = dev(c["loc"], gdt), dev(c["attn"], gdt)
    sh, st = dev(c["shapes"]), dev(c["level_start"])
    gv = torch.empty(value.shape, dtype=gdt, device=DEV)
    gl, ga = torch.full_like(loc, float("nan")), torch.full_like(attn, float("nan"))
    rc = alo_hip.lib().alo_msda_backward_hinted(
        *(ctypes.c_void_p(t.data_ptr()) for t in (value, sh, st, loc, attn, go, gv, gl, ga)), N, S, M, D, L, Lq, P, vdt, ldt, hint,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    seen = dict(c, value=value.double().cpu().numpy(), grad_out=go.double().cpu().numpy())
    return seen, [x.double().cpu().numpy() for x in (gv, gl, ga)]


def check_backward(seen, grads, dtype, queries=None, exact_edges=False):
    """All three gradients against the oracle on what the kernel saw; grad_loc on every sample (of ``queries``) against the edge-aware
    reference.  float64: one of the two one-sided derivatives, unless the edges are exact (``exact_edges``), where the float64 fma
    and the oracle agree and the float32 model of the reference applies unchanged."""
    gv, gl, ga = grads
    c = seen
    rgv, rgl, rga = O.msda_backward(c["value"], c["shapes"], c["level_start"], np.asarray(c["loc"], np.float64), c["attn"].astype(np.float64),
                                    c["grad_out"])
    assert np.isfinite(gl).all() and np.isfinite(ga).all()
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    assert np.abs(gv - rgv).max() <= 2 * tol * max(1.0, np.abs(rgv).max())
    assert np.abs(ga - rga).max() <= tol * max(1.0, np.abs(rga).max())
    scale = max(1.0, np.abs(rgl).max())
    if dtype == torch.float64 and not exact_edges:
        cands = grad_loc_one_sided(c["value"], c["shapes"], c["level_start"], c["loc"], c["attn"], c["grad_out"])
        assert_one_of(gl, cands, tol * scale)
        return
    ref = grad_loc_reference(c["value"], c["shapes"], c["level_start"], np.asarray(c["loc"]).astype(np.float32), c["attn"], c["grad_out"],
                             queries)
    got = gl if queries is None else gl[:, queries]
    err = np.abs(got - ref)
    assert err.max() <= tol * scale, f"grad_loc off by {err.max():.3g} (bar {tol * scale:.3g}) at {np.argwhere(err > tol * scale)[:3].tolist()}"


# ---- 1. the encoder call of a fresh model ------------------------------------------------------------------------------------------
def fresh_model_case(shapes_l, N, M, D, seed, padded=True, Lq=None, dtype=np.float32):
    """Locations exactly as a freshly initialised MSDeformAttn builds them for the encoder (reference points = pixel centres of
    the valid extent, offsets = sampling_offsets(query), the integer rings of the init): frame 0 unpadded, frame 1 (if ``padded``)
    with valid ratios < 1.  ``Lq``: the first Lq (strided) encoder reference points instead (a decoder-shaped call)."""
    from alonet.deformable_detr.deformable_transformer import DeformableTransformerEncoder
    from alonet.deformable_detr.ops.modules import MSDeformAttn

    tdt = torch.float64 if dtype == np.float64 else torch.float32
    torch.manual_seed(seed)
    m = MSDeformAttn(M * D, 4, M, 4).to(tdt)
    rng = np.random.default_rng(seed)
    S = sum(h * w for h, w in shapes_l)
    vr = torch.ones(N, 4, 2)
    if padded and N > 1:
        for lvl, (h, w) in enumerate(shapes_l):
            vr[1, lvl] = torch.tensor([np.ceil(0.8 * w) / w, np.ceil(0.7 * h) / h])
    shapes = torch.tensor(shapes_l, dtype=torch.int32)
    with torch.no_grad():
        ref = DeformableTransformerEncoder.get_reference_points(shapes, vr, device="cpu").to(tdt)   # (N, S, L, 2)
        if Lq is not None:
            ref = ref[:, :: S // Lq][:, :Lq]
        Lq = ref.shape[1]
        off = m.sampling_offsets(torch.randn(N, Lq, M * D, dtype=tdt)).view(N, Lq, M, 4, 4, 2)
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(tdt)
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    attn = rng.random((N, Lq, M, 4, 4))
    attn /= attn.reshape(N, Lq, M, 16).sum(-1)[..., None, None]
    sh = np.asarray(shapes_l, np.int32)
    return dict(value=rng.standard_normal((N, S, M, D)).astype(dtype), shapes=sh, level_start=level_start(sh), loc=loc.numpy(),
                attn=attn.astype(dtype), grad_out=rng.standard_normal((N, Lq, M * D)).astype(dtype))


def _edge_fraction(c):
    t = c["loc"].astype(np.float64) * _edge_sizes(c["shapes"], 4) - 0.5
    return (np.abs(t - np.round(t)) < 1e-3).all(-1).mean()


@pytest.mark.parametrize("route", ["wide_f32", "wide_bf16", "tiled_encoder"])
def test_fresh_model_encoder_call_at_full_size(route, monkeypatch):
    """The DETR pyramid (S = 22223), one frame: a quarter of all samples sit on a pixel corner; grad_loc of every sample of every 4th
    query and of the last ones against the edge-aware reference."""
    dtype, _, _, D, _ = ROUTES[route]
    c = fresh_model_case(DETR_SHAPES, 1, 8, D, 1, padded=False)
    assert _edge_fraction(c) > 0.2
    seen, grads = backward(c, route, monkeypatch)
    check_backward(seen, grads, dtype, queries=np.r_[0:22223:4, 22223 - 64:22223])


@pytest.mark.parametrize("route", ["wide_f32", "wide_bf16", "wide_d64", "tiled_encoder", "tiled_rows", "per_corner_f32_d64",
                                   "per_corner_bf16", "per_corner_f64"])
def test_fresh_model_encoder_call(route, monkeypatch):
    dtype, _, _, D, _ = ROUTES[route]
    c = fresh_model_case(SMALL_SHAPES, 2, 8 if D == 32 else 4, D, 2, dtype=np.float64 if dtype == torch.float64 else np.float32)
    assert _edge_fraction(c) > 0.15
    seen, grads = backward(c, route, monkeypatch)
    check_backward(seen, grads, dtype)


def test_fresh_model_decoder_shaped_call_takes_the_tiled_kernel(monkeypatch):
    """Lq = 300 queries on pixel centres (the consecutive-query route of msda_bwd_tiled_kernel, the decoder's cross-attention)."""
    c = fresh_model_case(DETR_SHAPES, 2, 8, 32, 3, Lq=300)
    seen, grads = backward(c, "tiled_rows", monkeypatch)
    check_backward(seen, grads, torch.float32)


# ---- 2. exact edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_exact_edges_on_every_backward_route(route, monkeypatch):
    """Dyadic pyramid, coordinates exactly on integers (k = 0, size - 1, interior; -1 and size: dropped; -1 + 2^-10): every route
    takes the cell to the right / below (floor), like the reference, on every sample — float64 included."""
    dtype, _, _, D, _ = ROUTES[route]
    S = sum(h * w for h, w in DYADIC_SHAPES)
    c = exact_edge_case(40 + D, 2, 8 if D == 32 else 4, D, S, dtype=np.float64 if dtype == torch.float64 else np.float32)
    seen, grads = backward(c, route, monkeypatch)
    check_backward(seen, grads, dtype, exact_edges=True)


# ---- 3. the forward kernels on exact edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_forward_on_exact_edges(dtype):
    """The forward is continuous across an edge, so this pins the corner bounds at k = size - 1 and k = -1: msda_forward (fp32 /
    fp64 per-corner kernels, bf16 MFMA kernel)."""
    S = sum(h * w for h, w in DYADIC_SHAPES)
    c = exact_edge_case(60, 2, 8, 32, S, dtype=np.float64 if dtype == torch.float64 else np.float32)
    v = dev(c["value"], dtype)
    gdt = torch.float64 if dtype == torch.float64 else torch.float32
    with alo_hip.LaunchTimer() as timer:
        out = alo_hip.msda_forward(v, dev(c["shapes"]), dev(c["level_start"]), dev(c["loc"], gdt), dev(c["attn"], gdt))
    assert f"msda_fwd/Lq={S}" in timer.summary()
    ref = O.msda_forward(v.double().cpu().numpy(), c["shapes"], c["level_start"], c["loc"].astype(np.float64), c["attn"].astype(np.float64))
    err = np.abs(out.double().cpu().numpy() - ref)
    bar = {torch.float64: 1e-12, torch.float32: 1e-5}.get(dtype)
    assert np.all(err <= (np.abs(ref) * 2.0 ** -8 + 1e-6 if dtype == torch.bfloat16 else bar))


@pytest.mark.parametrize("resident", [False, "always"])
def test_fused_head_major_forward_on_exact_edges(resident):
    """alo_msda_forward_fused_hm (plain head-major and LDS-resident kernels): per-level reference points on pixel centres plus
    integer bf16 offsets put every sample exactly on a pixel corner, incl. k = -1, 0, size - 1 and size."""
    N, M, D, L, P = 2, 8, 32, 4, 4
    shapes_l = DYADIC_SHAPES
    S = sum(h * w for h, w in shapes_l)
    Lq = S
    rng = np.random.default_rng(61)
    size = _edge_sizes(shapes_l, L)[0, 0, 0, :, 0, :]                   # (L, 2) = (W, H)
    j = np.floor(rng.random((N, Lq, L, 2)) * size).astype(np.float64)  # reference pixel per level
    pick = rng.integers(0, 5, (N, Lq, M, L, P, 2))
    sz = np.broadcast_to(size[None, None, None, :, None, :], pick.shape)
    k = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [-1.0, 0.0, sz - 1, sz], np.floor(rng.uniform(-1, sz + 1)))
    off = (k - j[:, :, None, :, None, :]).astype(np.float32)            # integers below 64: exact in bf16
    ref = ((j + 0.5) / size).astype(np.float32)
    gen = torch.Generator(device=DEV).manual_seed(61)
    shapes = dev(np.asarray(shapes_l, np.int32))
    shapes._alo_shapes = list(shapes_l)
    start = dev(level_start(shapes_l))
    value = torch.randn(N, S, M, D, generator=gen, device=DEV).bfloat16()
    logits = torch.randn(N, Lq, M, L * P, generator=gen, device=DEV).bfloat16()
    vhm = alo_hip.value_head_major(value, None)
    with alo_hip.LaunchTimer() as timer:
        got = alo_hip.msda_forward_fused_hm(vhm, shapes, start, dev(off, torch.bfloat16), logits, dev(ref), resident=resident)
    tag = "msda_fwd_fused_resident" if resident else "msda_fwd_fused"
    assert f"{tag}/Lq={Lq}" in timer.summary(), timer.summary().keys()
    loc = ref[:, :, None, :, None, :].astype(np.float64) + off.astype(np.float64) / size[None, None, None, :, None, :]
    a = torch.softmax(logits.double(), -1).view(N, Lq, M, L, P).cpu().numpy()
    exact = O.msda_forward(value.double().cpu().numpy(), np.asarray(shapes_l, np.int32), level_start(shapes_l), loc, a)
    err = np.abs(got.double().cpu().numpy() - exact)
    assert np.all(err <= np.abs(exact) * 2.0 ** -8 + 2e-5)   # half a bf16 ulp of the result + the fp32 prologue


# ---- 4. the first step's offset gradient -------------------------------------------------------------------------------------------
def test_first_step_sampling_offset_bias_gradient():
    """d loss / d sampling_offsets.bias of a fresh model's encoder call, through MSDeformAttnFunction under autograd (the wide
    kernel), against sum_q grad_loc_reference / (W_l, H_l): the gradient the first optimiser step applies to the offset ring."""
    from alonet.deformable_detr.ops.functions import MSDeformAttnFunction
    from alonet.deformable_detr.deformable_transformer import DeformableTransformerEncoder
    from alonet.deformable_detr.ops.modules import MSDeformAttn

    shapes_l, N, M, D = SMALL_SHAPES, 2, 8, 32
    torch.manual_seed(5)
    m = MSDeformAttn(M * D, 4, M, 4)
    S = sum(h * w for h, w in shapes_l)
    shapes = torch.tensor(shapes_l, dtype=torch.int32)
    vr = torch.ones(N, 4, 2)
    ref = DeformableTransformerEncoder.get_reference_points(shapes, vr, device="cpu")
    query = torch.randn(N, S, M * D)
    rng = np.random.default_rng(5)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    attn = rng.random((N, S, M, 4, 4)).astype(np.float32)
    attn /= attn.reshape(N, S, M, 16).sum(-1)[..., None, None]
    go = rng.standard_normal((N, S, M * D)).astype(np.float32)
    m = m.to(DEV)
    off = m.sampling_offsets(query.to(DEV)).view(N, S, M, 4, 4, 2)
    norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).float().to(DEV)
    loc = ref.to(DEV)[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    sh = shapes.to(DEV)
    hint = (ctypes.c_int32 * 8)(*[v for hw in shapes_l for v in hw])
    assert alo_hip.lib().alo_msda_backward_path(N, S, M, D, 4, S, 4, alo_hip.ALO_F32, alo_hip.ALO_F32, hint) == WIDE
    out = MSDeformAttnFunction.apply(dev(value), sh, dev(level_start(shapes_l)), loc, dev(attn), 64)
    out.backward(dev(go))
    got = m.sampling_offsets.bias.grad.double().cpu().numpy().reshape(M, 4, 4, 2)
    sh_np = np.asarray(shapes_l, np.int32)
    rgl = grad_loc_reference(value, sh_np, level_start(sh_np), loc.detach().cpu().numpy(), attn, go)
    terms = rgl / _edge_sizes(sh_np, 4)
    want = terms.sum((0, 1))
    err = np.abs(got - want)
    assert np.all(err <= 1e-4 * np.abs(terms).sum((0, 1)) + 1e-7), err.max()
