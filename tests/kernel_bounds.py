"""Shared pieces of the kernel-level tests (test_backbone_kernels_gpu.py, test_glue_kernels_gpu.py, test_glue_references_cpu.py):
the per-element comparison, the fp32-accumulation constant, and the fp64 references / bounds that are re-implementations rather
than a stock op in ``.double()``.  Everything here is plain torch and runs on whatever device its arguments live on;
test_glue_references_cpu.py pins each re-implementation to the stock module on the CPU.
"""
import torch
import torch.nn.functional as F

NAN, INF = float("nan"), float("inf")


def c_acc(k):
    """fp32-accumulation constant of a K-term dot product plus the bias (test_backbone_kernels_gpu.py, module docstring)."""
    return (k + 1) * 2.0 ** -23


def _finite_abs(t):
    return torch.nan_to_num(t.double().abs(), nan=0.0, posinf=0.0)


def compare(got, ref, bound, what):
    """Same non-finite outputs as the fp64 op (NaN where it has NaN, the same infinity where it has one); every other element
    within ``bound``.  Returns the worst error / bound ratio."""
    got = got.double()
    fin_g, fin_r = torch.isfinite(got), torch.isfinite(ref)
    diff = fin_g != fin_r
    if diff.any():
        idx = diff.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(diff.sum())} outputs differ in finiteness from the fp64 op, first at {idx}: "
                             f"got {got[tuple(idx)].item()} want {ref[tuple(idx)].item()}")
    nf = ~fin_r
    if nf.any():
        assert torch.equal(torch.isnan(got[nf]), torch.isnan(ref[nf])), f"{what}: NaN where the fp64 op has an infinity (or back)"
        inf = nf & ~torch.isnan(ref)
        assert torch.equal(got[inf], ref[inf]), f"{what}: an infinity of the wrong sign"
    err = torch.where(fin_r, (got - ref).abs(), torch.zeros_like(ref))
    bound = torch.where(fin_r, bound, torch.ones_like(bound))
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    if ratio > 1.0:
        idx = (err / bound).flatten().argmax().item()
        raise AssertionError(f"{what}: |got - ref| / bound = {ratio:.3g} at flat index {idx}: got {got.flatten()[idx].item()} "
                             f"want {ref.flatten()[idx].item()} bound {bound.flatten()[idx].item():.3g}")
    return ratio


def f32(v):
    """The fp32 value a kernel receives for the Python scalar ``v``, as a Python float (exact in fp64)."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- sine positional encoding ------------------------------------------------------------------------------------------------
def pos_sine_ref(mask_flat, shapes, dim_t, level_embed, normalize, center, scale, eps=1e-6):
    """PositionEmbeddingSine per level -> flatten -> + level_embed -> cat, in fp64: cumulative count of ``~mask`` along y and x,
    the module's centre / normalise arithmetic with the fp32 values of ``scale`` and ``eps`` (the operands the fp32 chains get),
    sin on even and cos on odd channels.  mask_flat (B, S) bool, dim_t (F,) fp32, level_embed (L, 2F) or None.
    -> (ref, p), both (B, S, 2F) fp64; p = embed / dim_t is the argument of the sine / cosine."""
    b = mask_flat.shape[0]
    dt = dim_t.double()
    scale, eps = f32(scale), f32(eps)
    even = (torch.arange(2 * dt.numel(), device=mask_flat.device) % 2 == 0)
    refs, args, s0 = [], [], 0
    for lvl, (h, w) in enumerate(shapes):
        valid = ~mask_flat[:, s0:s0 + h * w].view(b, h, w)
        s0 += h * w
        y = valid.cumsum(1, dtype=torch.float64)
        x = valid.cumsum(2, dtype=torch.float64)
        if normalize:
            if center:
                y, x = y - 0.5, x - 0.5
            y = y / (y[:, -1:, :] + eps) * scale
            x = x / (x[:, :, -1:] + eps) * scale
        p = torch.cat((y[..., None] / dt, x[..., None] / dt), 3).flatten(1, 2)    # (B, h * w, 2F): the y block first
        val = torch.where(even, p.sin(), p.cos())
        if level_embed is not None:
            val = val + level_embed[lvl].double()
        refs.append(val)
        args.append(p)
    assert s0 == mask_flat.shape[1]
    return torch.cat(refs, 1), torch.cat(args, 1)


POS_SINE_ABS = 2.0 ** -22   # the device / library sine's own error; see test_glue_kernels_gpu.py for how it was checked


def pos_sine_bound(ref, p, bf16=False):
    """2^-22 + 6 * 2^-24 |p| + 2^-24 |ref| (+ 2^-8 |ref| in bf16); derivation in test_glue_kernels_gpu.py."""
    bound = POS_SINE_ABS + 6 * 2.0 ** -24 * p.abs() + 2.0 ** -24 * ref.abs()
    return bound + 2.0 ** -8 * ref.abs() if bf16 else bound


def pyramid_masks(b, shapes, kinds, device, seed):
    """(B, S) bool padding mask of a pyramid; image i gets ``kinds[i % len(kinds)]`` on every level: "none", "right", "bottom",
    "corner" (right and bottom), "scatter" (random pixels: the count along a row is not x + 1 then), "all" (the whole image padded),
    "cross" (one fully padded row and column in the middle), "scatter+right"."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for h, w in shapes:
        m = torch.zeros(b, h, w, dtype=torch.bool)
        for i in range(b):
            kind = kinds[i % len(kinds)]
            if "scatter" in kind:
                m[i] = torch.rand(h, w, generator=g) < 0.3
            if kind in ("right", "corner", "scatter+right"):
                m[i, :, (2 * w) // 3:] = True
            if kind in ("bottom", "corner"):
                m[i, h // 2:, :] = True
            if kind == "all":
                m[i] = True
            if kind == "cross":
                m[i, h // 2, :] = True
                m[i, :, w // 2] = True
        out.append(m.flatten(1))
    return torch.cat(out, 1).to(device)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
def layernorm_inputs(rows, c, device, seed, ill=False):
    """x, res (rows, C) fp32 and gamma, beta (C,).  Well-conditioned rows are drawn as test_fused_gpu.py draws them
    (|mean| <= sigma).  With ``ill``: rows 4, 15, 26, ... are constant (variance 0) and the other rows of 1, 8, 15, ... have
    mean = 1000 x std; ``res`` is zero on both so that x + res keeps them so.
    -> x, res, gamma, beta, kind (rows,): 0 well-conditioned, 1 mean = 1000 x std, 2 constant."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(rows, c, device=device, generator=g) * 3 + 0.5
    res = torch.randn(rows, c, device=device, generator=g)
    gamma, beta = torch.randn(c, device=device, generator=g), torch.randn(c, device=device, generator=g)
    kind = torch.zeros(rows, dtype=torch.int64, device=device)
    if ill:
        r = torch.arange(rows, device=device)
        kind[r % 7 == 1] = 1
        kind[r % 11 == 4] = 2
        far, const = (kind == 1).nonzero()[:, 0], (kind == 2).nonzero()[:, 0]
        x[far] = 1000.0 + torch.randn(far.numel(), c, device=device, generator=g)
        x[const] = (torch.randn(const.numel(), 1, device=device, generator=g) * 5).expand(-1, c)
        res[far] = 0.0
        res[const] = 0.0
    return x, res, gamma, beta, kind


def layernorm_ref_and_bound(v, gamma, beta, eps, bf16=False):
    """v (rows, C) fp32 = x + res as the fp32 chains form it.  -> (ref, bound) in fp64,
    bound = |gamma_c| 2^-23 ((sqrt(C) + 8) (1 + |xhat|) + 4 (|v| + |mean|) / sigma) + 2^-24 |ref|  (+ 2^-8 |ref| in bf16),
    sigma = sqrt(var + eps) (what the op divides by: on a constant row it is sqrt(eps), not 0)."""
    c = v.shape[-1]
    v64 = v.double()
    ref = F.layer_norm(v64, (c,), gamma.double(), beta.double(), eps)
    mean = v64.mean(-1, keepdim=True)
    sigma = (v64.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    xhat = (v64 - mean) / sigma
    bound = gamma.double().abs() * 2.0 ** -23 * ((c ** 0.5 + 8) * (1 + xhat.abs()) + 4 * (v64.abs() + mean.abs()) / sigma)
    bound = bound + 2.0 ** -24 * ref.abs()
    return ref, (bound + 2.0 ** -8 * ref.abs() if bf16 else bound)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
def groupnorm_ref_and_bound(x, groups, gamma, beta, eps, relu=False):
    """x (N, C, *) bf16 (any memory format).  -> (ref, bound) in fp64: F.group_norm (+ relu), and
    2^-8 |ref| + 2^-10 |gamma_c| (1 + |xhat|); derivation in test_glue_kernels_gpu.py."""
    x64 = x.double()
    xhat = F.group_norm(x64, groups, None, None, eps)
    shape = (1, -1) + (1,) * (x.dim() - 2)
    ref = xhat * gamma.double().view(shape) + beta.double().view(shape)
    if relu:
        ref = torch.relu(ref)
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -10 * gamma.double().abs().view(shape) * (1 + xhat.abs())


def groupnorm_ill_inputs(n, c, hw, groups, device, seed):
    """(N, C, HW) bf16 whose groups cycle through mean / std = 0.25, 16, 100 and a constant group (1.5: exact in bf16)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, groups, c // groups, hw, device=device, generator=g)
    ratio = torch.tensor([0.25, 16.0, 100.0, 0.0], device=device)[torch.arange(groups, device=device) % 4]
    x = x + ratio.view(1, -1, 1, 1)
    x[:, 3::4] = 1.5
    return x.view(n, c, hw).bfloat16()


# ---- RAFT's convolutional GRU (alonet/raft/update.py, _gru_step) ---------------------------------------------------------------
def gru_gate_ref(zr, bias_zr, h):
    """zr (B, 2C, H, W) pre-activations [z | r], h (B, C, H, W).  -> z = sigmoid(z + b), r * h, both fp64."""
    c = h.shape[1]
    pre = zr.double() + bias_zr.double().view(1, -1, 1, 1)
    return torch.sigmoid(pre[:, :c]), torch.sigmoid(pre[:, c:]) * h.double()


def gru_update_ref(q, bias_q, z, h):
    """(1 - z) h + z tanh(q + b) in fp64."""
    z, h = z.double(), h.double()
    return (1 - z) * h + z * torch.tanh(q.double() + bias_q.double().view(1, -1, 1, 1))


def gru_bound(h):
    """2^-21 (1 + |h|): at most 8 fp32 roundings of values <= 1 + |h| around one expf / tanhf."""
    return 2.0 ** -21 * (1 + _finite_abs(h))


# ---- panoptic one-hot ---------------------------------------------------------------------------------------------------------
def panoptic_probabilities(logits, size, threshold):
    """interpolate -> sigmoid -> F.threshold of one image's (Q, h, w) logits, in the dtype of ``logits``."""
    up = F.interpolate(logits[None], size=size, mode="bilinear", align_corners=False)[0]
    return F.threshold(up.sigmoid(), threshold, 0.0)


def panoptic_onehot_from(masks):
    """detr_panoptic.py:100-110 on thresholded probabilities (Q, H, W): the arg-max query gets 1 unless no query passed."""
    nothing = (~masks.bool()).all(dim=0, keepdim=True)
    onehot = torch.zeros_like(masks)
    onehot.scatter_(0, masks.argmax(dim=0, keepdim=True), 1)
    return onehot.long() * (~nothing)


def panoptic_near_tie(logits, size, threshold, tol=1e-5):
    """(H, W) bool: in the fp64 chain the top two probabilities, or the top one and the threshold, are closer than ``tol`` — the
    only pixels where a correct fp32 evaluation may decide differently."""
    up = F.interpolate(logits.double()[None], size=size, mode="bilinear", align_corners=False)[0].sigmoid()
    if up.shape[0] == 1:
        return (up[0] - threshold).abs() < tol
    top = up.topk(2, dim=0).values
    return ((top[0] - top[1]) < tol) | ((top[0] - threshold).abs() < tol)
