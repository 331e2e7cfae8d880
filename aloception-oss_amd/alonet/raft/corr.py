"""RAFT correlation block on the gfx950 kernels: all-pairs volume + pyramid on the fp16 matrix pipe at fp32 accuracy (scaled
two-term operand split, three products — csrc/corr.hip), windowed lookup as a gather kernel.

Drop-in for the reference's ``CorrBlock`` (alonet/raft/corr.py:12-60) through RAFT's ``corr_block=`` constructor
hook (alonet/raft/raft.py:47-60,168,185): ``CorrBlock(fmap1, fmap2, num_levels=4, radius=4)`` builds
``corr_pyramid`` (list of ``(B*H*W, 1, h_l, w_l)`` float32 tensors) and ``corr_fn(coords)`` returns the
``(B, num_levels*(2r+1)^2, H, W)`` float32 window features.  ``AlternateCorrBlock`` (corr.py:63-91) is the memory-light
variant: it keeps the feature maps instead of the volume and computes each lookup's inner products on the fly
(csrc/corr_alt.hip); see its docstring.

Differentiability.  The reference's block is plain autograd-able torch code, so RAFT can be fine-tuned through it.  Here, when
the feature maps require a gradient:

* the pyramid is built by the HIP kernel inside ``_BuildFunction``; its backward is the matmul's own gradient written out —
  ``dF1 = P_l(F2) . dC_l^T / sqrt(C)``, ``dF2 = P_l^T(F1 . dC_l) / sqrt(C)`` summed over the levels that received a gradient, ``P_l`` =
  l-fold 2x2 mean of the feature map (a mean over a cell of the correlation is the correlation with the cell's mean feature) — as
  library GEMMs (``torch.bmm``) over the gradient maps: the volume is never re-evaluated and no second copy of it is held;
* a lookup runs the HIP kernel inside ``_LookupFunction``; its backward is the kernel's exact adjoint
  (``alo_corr_lookup_backward``), ACCUMULATED into gradient maps shared by all lookups of the block (RAFT looks the pyramid up 32
  times; autograd through ``grid_sample`` would materialise a dense gradient of the whole volume for each).  The maps reach
  ``_BuildFunction.backward`` through a scalar token every lookup depends on, not as dense autograd gradients;
* a gradient with respect to the COORDINATES (RAFT detaches them, raft.py:186; the reference's block is differentiable there too)
  is a kernel as well (``alo_corr_lookup_backward_coords``: the forward's gather with the horizontal differences kept, one map per
  level);
* ``corr_pyramid`` tensors used directly in somebody's own graph receive dense gradients the ordinary way; they are added to the
  accumulated maps.
Without gradients nothing of this exists: ``CorrBlock`` is two kernel calls.
"""
import math

import warnings

import torch
import torch.nn.functional as F

import alo_hip

from .utils.utils import bilinear_sampler


# ---- the torch formulation: what the reference computes, op for op (``TorchCorrBlock``; the tests' yardstick for the gradients) ------
def pyramid_torch(fmap1, fmap2, num_levels=4):
    """corr.py:13-27,52-60: ``<fmap1[b,:,i], fmap2[b,:,j]> / sqrt(C)`` as ``(B*H*W, 1, H, W)`` + ``num_levels - 1`` 2x2 means."""
    B, C, H, W = fmap1.shape
    vol = torch.matmul(fmap1.reshape(B, C, H * W).transpose(1, 2), fmap2.reshape(B, C, H * W)) / math.sqrt(C)
    pyramid = [vol.reshape(B * H * W, 1, H, W)]
    for _ in range(num_levels - 1):
        pyramid.append(F.avg_pool2d(pyramid[-1], 2, stride=2))
    return pyramid


def lookup_torch(pyramid, coords, radius):
    """corr.py:29-50: a (2r+1)^2 window around ``coords / 2^l`` on every level; the window's FIRST axis moves x (the reference
    stacks ``meshgrid(dy, dx)`` onto (x, y) coordinates), bilinear with corners aligned and zeros outside."""
    B, _, H, W = coords.shape
    r = radius
    centre = coords.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    steps = torch.linspace(-r, r, 2 * r + 1, device=coords.device, dtype=coords.dtype)
    window = torch.stack(torch.meshgrid(steps, steps, indexing="ij"), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    feats = [bilinear_sampler(vol, centre / 2 ** lvl + window).view(B, H, W, -1) for lvl, vol in enumerate(pyramid)]
    return torch.cat(feats, dim=-1).permute(0, 3, 1, 2).contiguous().float()


class TorchCorrBlock:
    """The same block on stock torch ops only (any device, differentiable end to end): ``RAFT(corr_block=TorchCorrBlock)``."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels, self.radius = num_levels, radius
        self.corr_pyramid = pyramid_torch(fmap1, fmap2, num_levels)

    def __call__(self, coords):
        return lookup_torch(self.corr_pyramid, coords, self.radius)

    @staticmethod
    def corr(fmap1, fmap2):
        B, _, H, W = fmap1.shape
        return pyramid_torch(fmap1, fmap2, 1)[0].view(B, H, W, 1, H, W)


# ---- HIP forward and backward ----------------------------------------------------------------------------------------------------
def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# The per-pass bookkeeping below stands on two private hooks of the autograd engine; they are resolved HERE, at import, so that a torch
# build without them fails with a clear message instead of an AttributeError in the middle of a backward pass.
_graph_task_id = getattr(torch._C, "_current_graph_task_id", None)
_queue_callback = getattr(getattr(torch.autograd.Variable, "_execution_engine", None), "queue_callback", None)
if _graph_task_id is None or _queue_callback is None:
    raise ImportError("alonet.raft.corr needs torch._C._current_graph_task_id and the autograd engine's queue_callback "
                      f"(present in torch 2.x; this is torch {torch.__version__})")


class _PyramidState:
    """What the build node and the lookup nodes of one block share: what the lookups read (CorrBlock: the pyramid;
    TrainableAlternateCorrBlock: the workspace) and, during a backward pass, the gradient maps the lookups accumulate into.
    ``new_maps()`` returns the zeroed maps of a pass (default: zeros shaped like the pyramid); ``owner`` names the block in the
    warning."""

    def __init__(self, new_maps=None, owner="CorrBlock"):
        self.pyramid = None
        self.grad = None
        self.grad_pass = None
        self.owner = owner
        self.new_maps = new_maps if new_maps is not None else (lambda: [torch.zeros_like(p) for p in self.pyramid])

    @staticmethod
    def _current_pass():
        """Identity of the autograd pass that is running (the engine's graph-task id; -1 outside a backward)."""
        return _graph_task_id()

    def grad_maps(self):
        """The maps of the backward pass that is running.  They belong to THAT pass: the first lookup backward of a pass creates
        them, tags them with the engine's graph-task id and queues an end-of-pass callback that drops whatever the build node did
        not consume — a pass that never reaches the build node (``autograd.grad(loss, coords)``) must not leave volume-sized maps
        behind to be added to the next pass's gradients.  The engine skips its callbacks when a pass aborts on an exception, so
        maps tagged by another pass are also discarded here, when the next pass first asks for them."""
        now = self._current_pass()
        if self.grad is None or self.grad_pass != now:
            self.grad = self.new_maps()
            self.grad_pass = now
            _queue_callback(self._end_of_pass)
        return self.grad

    def take_grad_maps(self):
        """What the lookups of the running pass accumulated (None if none did); the state is left empty."""
        maps, tag = self.grad, self.grad_pass
        self.grad = self.grad_pass = None
        if maps is not None and tag != self._current_pass():
            # lookups ran in another pass than the build node (a nested / re-entrant backward): their maps are not this pass's
            warnings.warn(f"{self.owner}: gradient maps accumulated by another autograd pass were discarded; the feature-map gradients "
                          f"of this pass do not include those lookups (re-entrant backward through a {self.owner} is not supported)",
                          RuntimeWarning, stacklevel=2)
            return None
        return maps

    def _end_of_pass(self):
        self.grad = self.grad_pass = None


def _pooled_chain(fmap, num_levels):
    """[fmap, 2x2 mean of it, ...]: what the pyramid's level l correlates fmap1 with (avg_pool2d drops an odd last row / column on
    the volume and on the feature map alike)."""
    chain = [fmap]
    for _ in range(num_levels - 1):
        chain.append(F.avg_pool2d(chain[-1], 2, stride=2))
    return chain


class _BuildFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap1, fmap2, num_levels, state):
        ctx.save_for_backward(fmap1, fmap2)
        ctx.num_levels = num_levels
        ctx.state = state
        state.pyramid = alo_hip.corr_build(fmap1, fmap2, num_levels)
        token = fmap1.new_zeros(())   # every lookup takes it as an input: autograd runs them all before this node's backward
        # the outputs are VIEWS: autograd hangs this node on them, and the state (which this node holds) must not hold the node back
        return (token,) + tuple(p.view_as(p) for p in state.pyramid)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gtoken, *grads):
        fmap1, fmap2 = ctx.saved_tensors
        state = ctx.state
        sparse = state.take_grad_maps()   # a later backward pass through the same graph starts from zero again
        totals = []
        for lvl in range(ctx.num_levels):
            parts = [g for g in (grads[lvl], sparse[lvl] if sparse is not None else None) if g is not None]
            totals.append(None if not parts else (parts[0] if len(parts) == 1 else parts[0] + parts[1]))
        if all(t is None for t in totals):
            return None, None, None, None
        B, C, H, W = fmap1.shape
        scale = 1.0 / math.sqrt(C)
        f1 = fmap1.reshape(B, C, H * W)
        g1 = torch.zeros_like(f1) if ctx.needs_input_grad[0] else None
        g2 = None
        with torch.enable_grad():
            leaf = fmap2.detach().requires_grad_(ctx.needs_input_grad[1])
            chain = _pooled_chain(leaf, ctx.num_levels)
        heads, head_grads = [], []
        for lvl, t in enumerate(totals):
            if t is None:
                continue
            n = chain[lvl].shape[-2] * chain[lvl].shape[-1]
            dvol = t.reshape(B, H * W, n)                                   # d loss / d vol_l[b, i, j]
            if g1 is not None:                                              # sum_j dvol[i, j] * P_l(F2)[c, j]
                g1.baddbmm_(chain[lvl].detach().reshape(B, C, n), dvol.transpose(1, 2), alpha=scale)
            if ctx.needs_input_grad[1]:                                     # sum_i dvol[i, j] * F1[c, i], then back through the means
                heads.append(chain[lvl])
                head_grads.append((torch.bmm(f1, dvol) * scale).reshape(chain[lvl].shape))
        if heads:
            (g2,) = torch.autograd.grad(heads, leaf, head_grads)
        return (g1.reshape(fmap1.shape) if g1 is not None else None), g2, None, None


class _LookupFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, token, radius, state):
        ctx.save_for_backward(coords)
        ctx.radius = radius
        ctx.state = state
        return alo_hip.corr_lookup(state.pyramid, coords, radius)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (coords,) = ctx.saved_tensors
        state = ctx.state
        gcoords = None
        if ctx.needs_input_grad[0]:
            gcoords = alo_hip.corr_lookup_backward_coords(state.pyramid, coords, grad_out, ctx.radius)
        if ctx.needs_input_grad[1]:
            alo_hip.corr_lookup_backward(state.grad_maps(), coords, grad_out, ctx.radius)
        return gcoords, (coords.new_zeros(()) if ctx.needs_input_grad[1] else None), None, None


class _LookupDenseFunction(torch.autograd.Function):
    """A lookup into pyramid tensors that did not come out of ``_BuildFunction`` under autograd (somebody's own differentiable
    pyramid, or coordinates that want a gradient while the features do not): the same two backward kernels, dense gradient maps."""

    @staticmethod
    def forward(ctx, coords, radius, *pyramid):
        ctx.save_for_backward(coords, *pyramid)
        ctx.radius = radius
        return alo_hip.corr_lookup(list(pyramid), coords, radius)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        coords, *pyramid = ctx.saved_tensors
        gcoords = alo_hip.corr_lookup_backward_coords(pyramid, coords, grad_out, ctx.radius) if ctx.needs_input_grad[0] else None
        gpyr = [None] * len(pyramid)
        if any(ctx.needs_input_grad[2:]):   # dense maps: this pyramid is somebody's own tensors, autograd wants a gradient per tensor
            maps = alo_hip.corr_lookup_backward([torch.zeros_like(p) for p in pyramid], coords, grad_out, ctx.radius)
            gpyr = [m if need else None for m, need in zip(maps, ctx.needs_input_grad[2:])]
        return (gcoords, None) + tuple(gpyr)


class CorrBlock:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        fmap1, fmap2 = fmap1.float(), fmap2.float()
        self._state = self._token = None
        if _needs_grad(fmap1, fmap2):
            self._state = _PyramidState()
            self._token, *pyramid = _BuildFunction.apply(fmap1.contiguous(), fmap2.contiguous(), num_levels, self._state)
            self.corr_pyramid = list(pyramid)
        else:
            self.corr_pyramid = alo_hip.corr_build(fmap1, fmap2, num_levels)

    def __call__(self, coords):
        coords = coords.float()
        if (self._state is not None and torch.is_grad_enabled() and len(self.corr_pyramid) == len(self._state.pyramid)
                and all(a.data_ptr() == b.data_ptr() and a.shape == b.shape for a, b in zip(self.corr_pyramid, self._state.pyramid))):
            return _LookupFunction.apply(coords.contiguous(), self._token, self.radius, self._state)
        if _needs_grad(coords, *self.corr_pyramid):
            return _LookupDenseFunction.apply(coords.contiguous(), self.radius, *self.corr_pyramid)
        return alo_hip.corr_lookup(self.corr_pyramid, coords, self.radius)

    @staticmethod
    def corr(fmap1, fmap2):
        """All-pairs correlation only: (B,C,H,W) x2 -> (B,H,W,1,H,W), scaled by 1/sqrt(C)."""
        B, _, H, W = fmap1.shape
        fmap1, fmap2 = fmap1.float(), fmap2.float()
        if _needs_grad(fmap1, fmap2):
            _, vol = _BuildFunction.apply(fmap1.contiguous(), fmap2.contiguous(), 1, _PyramidState())
        else:
            (vol,) = alo_hip.corr_build(fmap1, fmap2, 1)
        return vol.view(B, H, W, 1, H, W)


# ---- the memory-light block (corr.py:63-91) ----------------------------------------------------------------------------------------
def _alt_pyramid(fmap1, fmap2, num_levels):
    """corr.py:66-71: ``[(fmap1, fmap2)]`` + one 2x2 mean (floor) of both per level.  The reference pools ``num_levels`` times and
    never reads the last pair; that pair is left out where the last level read is one pixel wide or high (nothing to pool)."""
    B, C, H, W = fmap1.shape
    h, w = H, W
    for lvl in range(num_levels):
        if h == 0 or w == 0:
            raise RuntimeError(f"AlternateCorrBlock: pyramid level {lvl} of a {H}x{W} grid is empty (num_levels={num_levels})")
        h, w = h // 2, w // 2
    pyramid = [(fmap1, fmap2)]
    for lvl in range(num_levels):
        if lvl == num_levels - 1 and (fmap2.shape[-2] < 2 or fmap2.shape[-1] < 2):
            break
        fmap1, fmap2 = F.avg_pool2d(fmap1, 2, stride=2), F.avg_pool2d(fmap2, 2, stride=2)
        pyramid.append((fmap1, fmap2))
    return pyramid


class AlternateCorrBlock:
    """RAFT's memory-light correlation block (the reference's ``AlternateCorrBlock``, corr.py:63-91), on the gfx950 kernels of
    csrc/corr_alt.hip.  ``AlternateCorrBlock(fmap1, fmap2, num_levels=4, radius=4)``; ``blk(coords)`` -> ``(B,
    num_levels*(2r+1)^2, H, W)`` float32.  ``RAFT(corr_block=AlternateCorrBlock)`` works unchanged.

    Memory: only the feature maps are kept (O(HW*C)), not the O((HW)^2) all-pairs volume of :class:`CorrBlock`; every lookup
    computes the (2r+2)^2 inner products under each query's window.  4 x 1280x720 frames take 4.4 GB of pyramid with CorrBlock and
    59 MB of feature map here; 7680x4320 runs, where ``alo_corr_build`` refuses the grid.

    Value.  The reference's lookup calls the third-party ``alt_cuda_corr`` extension, whose source is not vendored here; the pin is
    therefore CorrBlock's golden outputs.  A 2x2 mean commutes with the inner product, so this block computes the SAME function as
    ``CorrBlock(fmap1, fmap2, num_levels, radius)(coords)`` up to fp32 rounding, channel layout included: the level is the outer
    index, within a window the first axis offsets x and the second offsets y, scale 1/sqrt(C).  Level l looks up ``fmap2``
    2x2-pooled l times at ``coords / 2^l`` against the full-resolution ``fmap1``.  Coordinates are plain pixel coordinates with
    zeros outside the map (no ``2x/(w-1)-1`` round trip), so levels one pixel wide or high give finite values (CorrBlock gives NaN
    there); NaN, +-inf and |coords / 2^l| >= 1e6 read as all-zero windows; a non-finite feature reaches exactly the outputs whose
    taps touch it.

    No autograd, as in the reference (``alt_cuda_corr.forward`` is called outside any ``autograd.Function``): the output never
    requires a gradient, even when the feature maps do.

    Attributes: ``num_levels``, ``radius`` and ``pyramid``, the reference's list of ``(fmap1_i, fmap2_i)`` NCHW pairs.  The
    channels-last copies the kernel reads are made once, here; the reference re-permutes on every lookup.  Construction and lookup
    make no host synchronisation (CUDA-graph capturable).
    """

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        fmap1, fmap2 = fmap1.float(), fmap2.float()
        alo_hip._require_f32_cuda("fmap1", fmap1, 4)
        alo_hip._require_f32_cuda("fmap2", fmap2, 4)
        if fmap1.shape != fmap2.shape:
            raise RuntimeError("fmap1 and fmap2 must have the same shape")
        if not 0 <= radius <= 7:
            raise RuntimeError(f"AlternateCorrBlock: radius must be in [0,7], got {radius}")
        with torch.no_grad():
            fmap1, fmap2 = fmap1.detach().contiguous(), fmap2.detach().contiguous()
            self.pyramid = _alt_pyramid(fmap1, fmap2, num_levels)
            self._channels = fmap1.shape[1]
            self._workspace = alo_hip.corr_alt_prepare(fmap1, [f2 for _, f2 in self.pyramid[:num_levels]])

    def __call__(self, coords):
        return alo_hip.corr_alt_lookup(self._workspace, coords.detach().float(), self._channels, self.num_levels, self.radius)


def alt_feature_gradients(planes, levels, shape, need_fmap1=True, need_fmap2=True):
    """The build node's backward of :class:`TrainableAlternateCorrBlock`, on stock ops (any device): the gradient maps the lookups
    accumulated, in the layout of the workspace's gradient region (include/alo_corr_alt.h), -> ``(grad_fmap1, grad_fmap2)`` as
    ``shape`` = (B, C, H, W) tensors (``None`` where not needed).  ``planes``: per level a (B, H*W, Cp) channels-last contribution
    to grad_fmap1; they are summed.  ``levels``: per level the slice-major (Cp/16, B, h_l*w_l, 16) gradient of fmap2 pooled l
    times; each goes back through the 2x2-mean chain (floor pooling: an odd last row or column receives nothing from the coarser
    levels) and they are summed.  Padded channels C..Cp-1 are dropped."""
    B, C, H, W = shape
    g1 = g2 = None
    if need_fmap1:
        total = planes[0][:, :, :C].clone()
        for plane in planes[1:]:
            total += plane[:, :, :C]
        g1 = total.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    if need_fmap2:
        with torch.enable_grad():   # the chain is linear: its adjoint does not depend on the leaf's values
            leaf = torch.zeros(shape, dtype=levels[0].dtype, device=levels[0].device, requires_grad=True)
            chain = _pooled_chain(leaf, len(levels))
        heads = []
        for lvl, g in enumerate(levels):
            h, w = chain[lvl].shape[-2:]
            heads.append(g.permute(1, 0, 3, 2).reshape(B, -1, h, w)[:, :C])   # (s, b, p, c) -> (b, 16 s + c, y, x)
        (g2,) = torch.autograd.grad(chain, leaf, heads)
    return g1, g2


class _AltBuildFunction(torch.autograd.Function):
    """Prepares the workspace (with its gradient region) and returns the scalar token every lookup takes; its backward turns the
    gradient maps of the pass into the feature-map gradients."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, num_levels, state, prepared):
        ctx.shape = tuple(fmap1.shape)
        ctx.num_levels = num_levels
        ctx.state = state
        # "pyramid": what the lookups read.  The maps AlternateCorrBlock prepared, with the gradient region behind them
        state.pyramid = alo_hip.corr_alt_with_grad_region(prepared, ctx.shape, num_levels)
        return fmap1.new_zeros(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gtoken):
        workspace = ctx.state.take_grad_maps()
        if workspace is None:
            return None, None, None, None, None
        _, planes, levels = alo_hip.corr_alt_grad_views(workspace, ctx.shape, ctx.num_levels)
        g1, g2 = alt_feature_gradients(planes, levels, ctx.shape, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return g1, g2, None, None, None


class _AltLookupFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, token, channels, num_levels, radius, state):
        ctx.save_for_backward(coords)
        ctx.dims = (channels, num_levels, radius)
        ctx.state = state
        return alo_hip.corr_alt_lookup(state.pyramid, coords, channels, num_levels, radius)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (coords,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return (None,) * 6
        alo_hip.corr_alt_lookup_backward(ctx.state.grad_maps(), coords, grad_out, *ctx.dims)
        return None, coords.new_zeros(()), None, None, None, None


class TrainableAlternateCorrBlock(AlternateCorrBlock):
    """:class:`AlternateCorrBlock` that can be trained through: ``RAFT(corr_block=TrainableAlternateCorrBlock)``.  Same constructor,
    same call, same values.

    When grad mode is off or neither feature map requires a gradient it IS ``AlternateCorrBlock``: the same two launches, the same
    bits, no extra memory.  Otherwise it follows :class:`CorrBlock`'s pattern: a build node returns a scalar token, every lookup is
    an ``autograd.Function`` that takes the token, and a lookup's backward (``corr_alt_lookup_bwd_kernel``, csrc/corr_alt.hip)
    ACCUMULATES into gradient maps shared by all lookups of the block; the build node's backward turns them into ``grad_fmap1`` and
    ``grad_fmap2`` (:func:`alt_feature_gradients`).  The maps live in the block's own workspace, behind the prepared feature maps,
    and are zeroed by the first lookup backward of a pass: memory stays O(HW*C*num_levels); nothing of size (HW)^2 or
    HW*C*(2r+1)^2 is ever allocated.

    No gradient with respect to the coordinates (RAFT detaches them; :class:`CorrBlock` has one): coordinates that require a
    gradient under grad mode raise.  No double backward.  ``grad_fmap1`` is bitwise reproducible; ``grad_fmap2`` is summed with
    float atomics, so its last bits depend on the run (as in the reference's scatter kernels and this library's MSDA backward).
    """

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self._state = self._token = None
        super().__init__(fmap1, fmap2, num_levels, radius)   # the checks, the pyramid, the prepared maps: without gradients, all
        if not _needs_grad(fmap1, fmap2):
            return
        self._shape = tuple(fmap1.shape)
        self._state = _PyramidState(self._zeroed_maps, owner="TrainableAlternateCorrBlock")
        self._token = _AltBuildFunction.apply(fmap1.float(), fmap2.float(), num_levels, self._state, self._workspace)
        self._workspace = self._state.pyramid

    def _zeroed_maps(self):
        region, _, _ = alo_hip.corr_alt_grad_views(self._workspace, self._shape, self.num_levels)
        region.zero_()
        return self._workspace

    def __call__(self, coords):
        if torch.is_grad_enabled() and coords.requires_grad:
            raise RuntimeError("TrainableAlternateCorrBlock has no gradient with respect to the coordinates: detach them (RAFT "
                               "does), or use CorrBlock, which has one")
        if self._state is None or not torch.is_grad_enabled():
            return super().__call__(coords)
        return _AltLookupFunction.apply(coords.detach().float().contiguous(), self._token, self._channels, self.num_levels,
                                        self.radius, self._state)


def lookup_alt_torch(pyramid, coords, num_levels, radius):
    """What :class:`AlternateCorrBlock` computes, on stock torch ops: the inner product of fmap1 with fmap2_l sampled bilinearly
    (zeros outside) at every tap (interpolation commutes with the inner product), pixel coordinates mapped exactly onto
    ``grid_sample(align_corners=False)``'s grid so that maps one pixel wide work too."""
    B, _, H, W = coords.shape
    r = radius
    f1 = pyramid[0][0]
    C = f1.shape[1]
    steps = torch.arange(-r, r + 1, device=coords.device, dtype=coords.dtype)
    dx = steps.view(-1, 1).expand(2 * r + 1, 2 * r + 1)   # first window axis: x offset
    dy = steps.view(1, -1).expand(2 * r + 1, 2 * r + 1)
    x, y = coords[:, 0].reshape(B, H * W, 1), coords[:, 1].reshape(B, H * W, 1)
    valid = (x.abs() < 1e6) & (y.abs() < 1e6)
    outs = []
    for lvl in range(num_levels):
        f2 = pyramid[lvl][1]
        h, w = f2.shape[-2:]
        xl = torch.where(valid, x, torch.zeros_like(x)) / 2 ** lvl
        yl = torch.where(valid, y, torch.zeros_like(y)) / 2 ** lvl
        valid_l = valid & (xl.abs() < 1e6) & (yl.abs() < 1e6)
        gx = (2 * (xl + dx.reshape(1, 1, -1)) + 1) / w - 1
        gy = (2 * (yl + dy.reshape(1, 1, -1)) + 1) / h - 1
        grid = torch.stack([gx, gy], dim=-1)                                       # (B, HW, WIN^2, 2)
        taps = F.grid_sample(f2, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # (B, C, HW, WIN^2)
        corr = (f1.reshape(B, C, H * W, 1) * taps).sum(1) / math.sqrt(C)           # (B, HW, WIN^2)
        outs.append(torch.where(valid_l, corr, torch.zeros_like(corr)))
    return torch.cat(outs, dim=-1).permute(0, 2, 1).reshape(B, -1, H, W).contiguous().float()


class TorchAlternateCorrBlock:
    """:class:`AlternateCorrBlock` on stock torch ops only (any device; the CPU yardstick, as :class:`TorchCorrBlock` is for
    CorrBlock).  Differentiable, unlike the HIP block."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels, self.radius = num_levels, radius
        self.pyramid = _alt_pyramid(fmap1.float(), fmap2.float(), num_levels)

    def __call__(self, coords):
        return lookup_alt_torch(self.pyramid, coords.float(), self.num_levels, self.radius)
