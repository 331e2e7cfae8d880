"""Shared generators for the parity tests (seeded, numpy), and the census of the C ABI (headers against the library)."""
import os
import re
import subprocess

import numpy as np

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = ("alo_hotpath.h", "alo_corr_alt.h", "alo_two_stage.h", "alo_encoder_block.h")   # one library, one per feature group


def header_text(header):
    """``include/<header>`` without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


def declared_functions(header):
    """Sorted names of the ``alo_*`` functions that ``include/<header>`` declares."""
    return sorted(set(re.findall(r"\b(alo_[a-z0-9_]+)\s*\(", header_text(header))))


def exported_alo_functions(path):
    """The ``alo_*`` functions that the shared object at ``path`` defines in its dynamic symbol table."""
    out = subprocess.run(["readelf", "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
    exported = set()
    for line in out.splitlines():
        cols = line.split()   # Num: Value Size Type Bind Vis Ndx Name
        if len(cols) == 8 and cols[3] == "FUNC" and cols[6] != "UND" and cols[7].startswith("alo_"):
            exported.add(cols[7].split("@")[0])
    return exported


def level_start(shapes):
    shapes = np.asarray(shapes, np.int64)
    return np.concatenate([[0], np.cumsum(shapes[:, 0] * shapes[:, 1])[:-1]]).astype(np.int32)


def msda_case(seed, N, M, D, Lq, shapes, P, dtype=np.float32, loc_range=(-0.1, 1.1)):
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, np.int32)
    L = len(shapes)
    S = int((shapes[:, 0].astype(np.int64) * shapes[:, 1]).sum())
    value = rng.standard_normal((N, S, M, D)).astype(dtype)
    loc = rng.uniform(loc_range[0], loc_range[1], (N, Lq, M, L, P, 2)).astype(dtype)
    logits = rng.standard_normal((N, Lq, M, L * P))
    attn = np.exp(logits - logits.max(-1, keepdims=True))
    attn = (attn / attn.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P).astype(dtype)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(dtype)
    return dict(value=value, shapes=shapes, level_start=level_start(shapes), loc=loc, attn=attn, grad_out=grad_out)


DETR_SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]  # 800 x 1333 frame, strides 8/16/32/64  (S = 22223)


def formula_state_dict(state_dict, seed=0):
    """Deterministic weights derived from each tensor's NAME and SHAPE only.

    Applied to the reference's module (when the golden vectors are generated) and to ours (in the tests): both models
    then hold identical parameters without a multi-megabyte checkpoint in the repository, and independently of the
    order in which either implementation constructs its sub-modules.
    """
    import zlib

    import torch

    out = {}
    for key in sorted(state_dict):
        ref = state_dict[key]
        if not ref.dtype.is_floating_point:
            out[key] = ref.clone()
            continue
        gen = torch.Generator().manual_seed((zlib.crc32(key.encode()) + seed) % (2 ** 31))
        noise = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "running_var":
            val = 1.0 + 0.1 * noise.abs()
        elif leaf == "running_mean":
            val = 0.05 * noise
        elif ref.dim() <= 1:
            is_norm_scale = leaf == "weight"
            val = (1.0 + 0.1 * noise) if is_norm_scale else 0.05 * noise
        else:
            fan_in = ref[0].numel()
            val = noise * (1.0 / fan_in) ** 0.5
        out[key] = val.to(ref.dtype)
    return out


def stub_pyramid(channels=(8, 12, 16, 24)):
    """A seeded four-stage convolution pyramid (strides 4 / 8 / 16 / 32, ceil sizes like a ResNet's) in the role of the ResNet
    body: ``forward(x) -> OrderedDict {"0": stride 4, ..., "3": stride 32}``.  The model-level fixtures (G14 / G15,
    tests/golden/make_golden_models.py) put the SAME module under the reference's ``BackboneBase`` / ``Joiner`` and under this
    repository's, so everything above the convolution stack is compared with the reference: mask resize, positional encodings,
    projections, transformer, heads, ``inference()``."""
    from collections import OrderedDict

    import torch.nn.functional as F
    from torch import nn

    class StubPyramid(nn.Module):
        def __init__(self):
            super().__init__()
            c0, c1, c2, c3 = channels
            self.layer1 = nn.Sequential(nn.Conv2d(3, c0, 3, stride=2, padding=1), nn.ReLU(), nn.Conv2d(c0, c0, 3, stride=2, padding=1))
            self.layer2 = nn.Conv2d(c0, c1, 3, stride=2, padding=1)
            self.layer3 = nn.Conv2d(c1, c2, 3, stride=2, padding=1)
            self.layer4 = nn.Conv2d(c2, c3, 3, stride=2, padding=1)

        def forward(self, x):
            out = OrderedDict()
            for i, name in enumerate(("layer1", "layer2", "layer3", "layer4")):
                x = F.relu(getattr(self, name)(x))
                out[str(i)] = x
            return out

    return StubPyramid()


def tied_formula_state_dict(model, seed=0, scale=None):
    """``formula_state_dict`` of ``model`` where keys that alias ONE parameter (Deformable-DETR's shared detection heads:
    ``class_embed.0 … .5`` are the same module) all carry the values of the alphabetically first alias, so the loaded weights do not depend on the
    order in which ``load_state_dict`` walks the aliases.  ``scale``: {key suffix: factor} applied on top (G15 widens
    ``query_embed.weight`` so that the queries of the vanilla DETR decoder do not come out as near-copies of each other)."""
    sd = formula_state_dict(model.state_dict(), seed)
    for suffix, factor in (scale or {}).items():
        for key in sd:
            if key.endswith(suffix):
                sd[key] = sd[key] * factor
    groups = {}
    for key, ref in model.state_dict(keep_vars=True).items():
        if ref.numel():
            groups.setdefault((ref.data_ptr(), tuple(ref.shape)), []).append(key)
    for keys in groups.values():
        owner = min(keys)                      # independent of the order in which either implementation registers its modules
        for key in keys:
            sd[key] = sd[owner].clone()
    return sd


def g17_inputs(g):
    """Re-draws the inputs of the G17 fixture (the reference's TensorRT-plugin test case for the MSDA kernel: 24 MB of uniform noise,
    kept as a seed) with torch's CPU generator, in the generator's call order, and checks them against the fixture's sha256 digests.
    Returns (value, loc, attn) as float32 tensors, or None when this torch build draws a different stream."""
    import hashlib

    import torch

    N, M, D, Lq, L, P = (int(v) for v in g["dims"])
    S = int(np.prod(g["shapes"].astype(np.int64), axis=1).sum())
    gen = torch.Generator().manual_seed(int(g["seed"]))
    value = torch.rand(N, S, M, D, generator=gen)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=gen)
    attn = torch.rand(N, Lq, M, L, P, generator=gen) + 1e-5
    attn /= attn.sum(-1, keepdim=True).sum(-2, keepdim=True)
    for t, key in ((value, "sha_value"), (loc, "sha_loc"), (attn, "sha_attn")):
        if hashlib.sha256(t.numpy().tobytes()).digest() != g[key].tobytes():
            return None
    return value, loc, attn


# ---- grad_sampling_loc on pixel edges ------------------------------------------------------------------------------------------
# grad_sampling_loc is the derivative of a piecewise-bilinear function: a component JUMPS where its image coordinate
# t = loc * size - 0.5 crosses an integer.  The reference maps a float32 location with one fused multiply-add and takes floor() of
# the float32 result r; the float64 oracle takes floor(t) of the exact value.  They disagree only where r is an integer k that t
# lies just below: the device then works in the cell [k, k + 1] (or drops the sample, at k = -1 or k = size), the oracle in the cell
# below.  Inside one cell d/dx is constant along x, so the device's component is the oracle's with that coordinate moved to k + 0.5.
def _edge_sizes(shapes, L):
    shapes = np.asarray(shapes, np.int64)
    return np.stack([shapes[:, 1], shapes[:, 0]], -1).astype(np.float64).reshape(1, 1, 1, L, 1, 2)   # (x, y) -> (W, H)


def _oracle_grad_loc(value, shapes, start, loc64, attn, grad_out):
    import oracle as O

    return O.msda_backward(value, shapes, start, loc64, attn, grad_out)[1]


def grad_loc_reference(value, shapes, start, loc, attn, grad_out, queries=None):
    """The grad_sampling_loc a float32 device computes for float32 ``loc`` (N, Lq, M, L, P, 2), every sample included, in float64.

    ``queries`` (index / slice / mask on the query axis): only those queries' rows are computed and returned — a sample's
    grad_loc depends on its own query's inputs alone, so the oracle then runs on Lq' < Lq queries.  Three oracle runs at most."""
    loc = np.asarray(loc)
    assert loc.dtype == np.float32, "grad_loc_reference models the float32 mapping; use grad_loc_one_sided for float64 launches"
    if queries is not None:
        loc, attn, grad_out = loc[:, queries], np.asarray(attn)[:, queries], np.asarray(grad_out)[:, queries]
    value, attn, grad_out = (np.asarray(a, np.float64) for a in (value, attn, grad_out))
    loc64 = loc.astype(np.float64)
    size = _edge_sizes(shapes, loc.shape[3])
    with np.errstate(invalid="ignore", over="ignore"):
        t = loc64 * size - 0.5                   # exact: 24-bit mantissa x an integer below 2^15
        r = t.astype(np.float32).astype(np.float64)   # the correctly rounded fma
        edge = np.isfinite(r) & (r == np.floor(r))
        inner = edge & (r >= 0) & (r <= size - 1)
        dropped = (edge & ((r == -1) | (r == size))).any(-1)
    out = _oracle_grad_loc(value, shapes, start, loc64, attn, grad_out)
    for axis in (0, 1):
        sel = inner[..., axis]
        if sel.any():
            moved = loc64.copy()
            moved[..., axis] = np.where(sel, (r[..., axis] + 1.0) / size[..., axis], loc64[..., axis])   # t -> k + 0.5
            out[..., axis] = np.where(sel, _oracle_grad_loc(value, shapes, start, moved, attn, grad_out)[..., axis], out[..., axis])
    out[dropped] = 0.0
    return out


def grad_loc_one_sided(value, shapes, start, loc, attn, grad_out, eps=1e-9):
    """For float64 launches (whose fma cannot be emulated portably): a (K, N, Lq, M, L, P, 2) float64 stack of candidates such that
    each component of the device's grad_sampling_loc must equal one of them.  Away from a pixel edge every candidate is the oracle.
    A component within ``eps`` px of an integer k has the two one-sided derivatives (the oracle with that coordinate moved to
    k -+ 0.5, which is 0 where that side drops the sample); a coordinate on the border of validity (k = -1 or k = size) adds 0 for
    the OTHER component (the sample may be dropped as a whole)."""
    value, attn, grad_out, loc = (np.asarray(a, np.float64) for a in (value, attn, grad_out, loc))
    size = _edge_sizes(shapes, loc.shape[3])
    with np.errstate(invalid="ignore", over="ignore"):
        t = loc * size - 0.5
        k = np.round(t)
        near = np.isfinite(t) & (np.abs(t - k) <= eps)
        border = (near & ((k == -1) | (k == size)))[..., ::-1]   # the other component's coordinate sits on the border
    plain = _oracle_grad_loc(value, shapes, start, loc, attn, grad_out)
    lo, hi = plain.copy(), plain.copy()
    for axis in (0, 1):
        sel = near[..., axis]
        if sel.any():
            for side, dst in ((-0.5, lo), (0.5, hi)):
                moved = loc.copy()
                moved[..., axis] = np.where(sel, (k[..., axis] + side + 0.5) / size[..., axis], loc[..., axis])
                dst[..., axis] = np.where(sel, _oracle_grad_loc(value, shapes, start, moved, attn, grad_out)[..., axis], dst[..., axis])
    return np.stack([lo, hi, np.where(border, 0.0, lo), np.where(border, 0.0, hi)])


def assert_one_of(got, candidates, atol):
    """Every component of ``got`` within ``atol`` of one of ``candidates`` (from grad_loc_one_sided)."""
    ok = (np.abs(np.asarray(got)[None] - candidates) <= atol).any(0)
    assert ok.all(), f"{(~ok).sum()} grad_loc components match no side of their edge; first at {np.argwhere(~ok)[:3].tolist()}"


DYADIC_SHAPES = [(32, 64), (16, 32), (8, 16), (4, 8)]   # power-of-two sizes: loc = (t + 0.5) / size is exact in float32 and float64


def exact_edge_case(seed, N, M, D, Lq, shapes=DYADIC_SHAPES, P=4, dtype=np.float32):
    """An msda case whose sampling points sit EXACTLY on pixel edges (power-of-two sizes, image coordinates on a 2^-10 grid): per
    sample x only, y only or both on an integer k, or neither; k = 0, size - 1 (high corner off the map), -1 and size (dropped), an
    interior k, and -1 + 2^-10 (the lowest coordinate that counts)."""
    rng = np.random.default_rng(seed)
    c = msda_case(seed, N, M, D, Lq, shapes, P, dtype)
    L = len(shapes)
    size = _edge_sizes(shapes, L)[0, 0, 0, :, 0, :]            # (L, 2)
    t = np.round(rng.uniform(-1.4, 1.0, (N, Lq, M, L, P, 2)) * (size + 1.0) * 1024) / 1024   # free: a 2^-10 grid over the map
    kind = rng.integers(0, 4, (N, Lq, M, L, P))                 # 0 free, 1 x on an edge, 2 y on an edge, 3 both
    for axis, on in ((0, (kind == 1) | (kind == 3)), (1, (kind == 2) | (kind == 3))):
        sz = np.broadcast_to(size[None, None, None, :, None, axis], on.shape)
        pick = rng.integers(0, 6, on.shape)
        k = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4],
                      [0.0, sz - 1, -1.0, sz, -1.0 + 2.0 ** -10], np.floor(rng.uniform(1, sz - 1)))
        t[..., axis] = np.where(on, k, t[..., axis])
    c["loc"] = ((t + 0.5) / size[None, None, None, :, None, :]).astype(dtype)
    assert np.array_equal(c["loc"].astype(np.float64) * size[None, None, None, :, None, :] - 0.5, t)   # exact in dtype
    return c
