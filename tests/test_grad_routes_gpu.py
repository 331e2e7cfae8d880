"""Gradients on every route where the inference kernels meet autograd.

The HIP layer kernels (alo_hip.add_layernorm, linear_shortk, ffn256, bias_act_, gru_*, ...) have no backward: a module may take
them only with grad mode off or with everything they read frozen.  Each case here takes three gradients of
one scalar, ``loss = sum(output * fixed random tensor)``:

  ref    a deep copy of the module in fp64 on PyTorch ops only (``is_tracing=None``: the grid_sample branch; fp64 passes no gate);
  stock  the module at its own dtype with the fast paths off (``is_tracing=None`` and ``alo_hip.fusable`` answering False):
         what PyTorch's own ops achieve in that precision;
  hip    the module as shipped.

and asserts, per parameter (and per input that requires grad):

  a) the gradient is ``None`` for hip exactly where it is for ref;
  b) where ``|g_ref| > 0`` the hip gradient is neither ``None`` nor all zero;
  c) ``e(hip) <= FACTOR * e(stock) + 8 eps(dtype)`` with ``e(route) = |g_route - g_ref|_2 / |g_ref|_2``.  Both routes run the same
     chain in the same precision; they differ in the MSDA backward (atomic accumulation order, fp32 locations) and, upstream of
     frozen parts, in fused kernels that round once where stock ops round several times.  A gradient that is zero in exact
     arithmetic (``|g_ref|`` below 1e-9 of the case's largest) has no relative error: it is held to the same inequality in
     absolute terms, in units of the case's largest ``|g_ref|``.
  d) launch tags: a case cannot pass by abandoning a fast path it may keep (everything frozen under grad; ``no_grad``).

ref and stock do not depend on which parameters are trainable, so each (module, dtype, mode) computes them once, with everything
trainable, and the freeze patterns share them.  docs/experiments.md ("Gradient routes") holds the measured e(hip) / e(stock).
"""
import copy
import functools

import pytest
import torch
from torch import nn

import alo_hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SHAPES = ((12, 17), (6, 9), (3, 5), (2, 3))
# c): 4 is the starting margin.  Two (family, dtype) pairs need more and get twice their measured ratio
# (docs/experiments.md, "Gradient routes").  Behind both: the bilinear map's derivative with respect to a sampling location JUMPS at a pixel
# edge (tests/helpers.py grad_loc_reference), so a location that a route's own roundings carry across an edge changes that
# sample's grad_sampling_loc by O(1), not by an eps.  The routes round differently upstream of the locations (the MSDA forward
# kernel against grid_sample), so each has its own few flipped samples against ref; where few samples carry the gradient one flip
# shows.  The op itself, on equal inputs, agrees with the fp64 formulation to 3e-7 in every storage type.
#   T fp16: the loss reaches the encoder through the 7 queries' samples only; encoder.layers.1's sampling_offsets (and level_embed
#           behind them) measure e(hip) = 0.125 against e(stock) = 0.021, every other parameter within 1.2: (0.125 - floor) / 0.021 = 5.64
#   W fp32: 8 eps is 1e-6, one flipped sample among the detector's 600 queries x 6 layers x 128 points moves every gradient upstream
#           of its layer by 1e-5 .. 1e-3.  Per parameter (docs/experiments.md): decoder layer 5 is clean on both routes (6e-7), hip
#           steps to 8e-6 from decoder layer 4 down (stock stays at 6e-7), stock steps to 2e-5 at decoder layer 1, both sit at
#           1e-5 .. 4e-5 in the encoder: each route has its own flips, at different layers.  Largest ratio 38.0, at
#           transformer.decoder.layers.4.norm3.bias (8.77e-6 against 2.06e-7).  With MIOpen's default (non-deterministic)
#           algorithms the flips change from run to run (4.05, 7.8, 2.88, 47 measured): the test asks for deterministic ones
FACTOR = {"T": 4.0, "M": 4.0, "B": 4.0, "I": 4.0, "R": 4.0, "P": 4.0, "W": 4.0, ("T", F16): 2 * 5.64, ("W", F32): 2 * 38.0}
ALL = object()          # every parameter trainable


def _floor(dtype):
    return 8 * torch.finfo(dtype).eps


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


class Routes:
    """One module at one dtype with its inputs.  ``forward(module, inputs, **kw) -> [output tensors]``; ``inputs`` is a dict of
    tensors (floating ones are cast for ref), ``grad_inputs`` the names that may require grad; ``kwargs_ok``: the forward takes
    ``is_tracing``."""

    def __init__(self, family, module, inputs, grad_inputs, forward, kwargs_ok, probe_shape=None):
        self.family, self.module, self.inputs, self.grad_inputs = family, module, inputs, tuple(grad_inputs)
        self.forward, self.kwargs_ok, self.probe_shape = forward, kwargs_ok, probe_shape
        self.dtype = next(module.parameters()).dtype
        self.names = [n for n, _ in module.named_parameters()] + [f"input:{k}" for k in self.grad_inputs]
        self._probes, self._ref_module, self._cache = None, None, {}

    # ---- one backward ------------------------------------------------------------------------------------------------------------
    def _loss(self, outs, dtype):
        if self._probes is None:   # fixed random tensors, drawn once per case on the host
            gen = torch.Generator().manual_seed(1234)
            shape = self.probe_shape or (lambda o: o.shape)
            self._probes = [torch.randn(shape(o), generator=gen, dtype=torch.float64).to(DEV) for o in outs]
        total = 0
        for o, p in zip(outs, self._probes):
            o = o.to(dtype)
            o = torch.where(torch.isfinite(o), o, torch.zeros((), dtype=dtype, device=o.device))   # two-stage: +inf marks a dropped token
            total = total + (o * p.to(dtype)).sum()
        return total

    def _grads(self, module, trainable, inputs_grad, train, kw, double=False):
        params = dict(module.named_parameters())
        for n, p in params.items():
            p.requires_grad_(trainable is ALL or n in trainable)
            p.grad = None
        module.train(train)
        ins = {}
        for k, v in self.inputs.items():
            cast = lambda t: t.double() if double and t.is_floating_point() else t
            v = [cast(t) for t in v] if isinstance(v, (list, tuple)) else cast(v)
            if k in self.grad_inputs and inputs_grad:
                v = [t.detach().clone().requires_grad_(True) for t in v] if isinstance(v, list) else v.detach().clone().requires_grad_(True)
            ins[k] = v
        loss = self._loss(self.forward(module, ins, **kw), torch.float64 if double else torch.float32)
        if loss.requires_grad:
            loss.backward()
        out = {n: None if p.grad is None else p.grad.detach().double() for n, p in params.items()}
        for k in self.grad_inputs:
            v = ins[k]
            g = [t.grad for t in v] if isinstance(v, list) else [v.grad]
            out[f"input:{k}"] = None if any(x is None for x in g) else torch.cat([x.detach().double().flatten() for x in g])
        for p in params.values():
            p.grad = None
        return out

    def _tracing(self):
        return dict(is_tracing=None) if self.kwargs_ok else {}

    def ref(self, train):
        if ("ref", train) not in self._cache:
            if self._ref_module is None:
                self._ref_module = copy.deepcopy(self.module).double()
            self._cache["ref", train] = self._grads(self._ref_module, ALL, True, train, self._tracing(), double=True)
        return self._cache["ref", train]

    def stock(self, train):
        if ("stock", train) not in self._cache:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(alo_hip, "fusable", lambda *a, **k: False)
                self._cache["stock", train] = self._grads(self.module, ALL, True, train, self._tracing())
        return self._cache["stock", train]

    def hip(self, trainable, inputs_grad, train):
        with alo_hip.LaunchTimer() as timer:
            grads = self._grads(self.module, trainable, inputs_grad, train, {})
        return grads, {tag: v["calls"] for tag, v in timer.summary().items()}

    # ---- the assertions ----------------------------------------------------------------------------------------------------------
    def check(self, trainable, inputs_grad, train, what=""):
        """a), b), c) for one freeze pattern -> the hip route's launch tags."""
        ref, stock = self.ref(train), self.stock(train)
        hip, tags = self.hip(trainable, inputs_grad, train)
        on = lambda n: (inputs_grad if n.startswith("input:") else (trainable is ALL or n in trainable))
        want_none = {n for n in self.names if not on(n) or ref[n] is None}
        got_none = {n for n in self.names if hip[n] is None}
        label = f"{self.family} {str(self.dtype)[6:]} {'train' if train else 'eval'} {what}"
        assert got_none == want_none, f"a) {label}: grad None only on hip {sorted(got_none - want_none)[:8]}, only on ref {sorted(want_none - got_none)[:8]}"
        live = [n for n in self.names if n not in want_none]
        assert live or not any(on(n) for n in self.names), f"{label}: the pattern selects nothing that the loss depends on"
        top = max((float(ref[n].norm()) for n in self.names if ref[n] is not None), default=0.0)
        factor, floor = FACTOR.get((self.family, self.dtype), FACTOR[self.family]), _floor(self.dtype)
        worst, e_max = (0.0, 0.0, 0.0, "-"), [0.0, 0.0]
        for n in live:
            r, h, s = ref[n], hip[n].reshape(ref[n].shape), stock[n].reshape(ref[n].shape)
            scale = float(r.norm())
            null = scale <= 1e-9 * top
            if not null:
                assert float(h.norm()) > 0.0, f"b) {label}: {n} has an all-zero gradient on hip, |g_ref| = {scale:.3e}"
            scale = top if null else scale
            e_hip, e_stock = float((h - r).norm()) / scale, float((s - r).norm()) / scale
            e_max = [max(e_max[0], e_hip), max(e_max[1], e_stock)]
            need = max(e_hip - floor, 0.0) / max(e_stock, 1e-300)       # the factor this parameter asks of c)
            if need > worst[0]:
                worst = (need, e_hip, e_stock, n)
            assert e_hip <= factor * e_stock + floor, (f"c) {label}: {n} e(hip) = {e_hip:.3e} > {factor} * e(stock) = {e_stock:.3e} "
                                                       f"+ {floor:.1e} (|g_ref| = {float(r.norm()):.3e}{', null' if null else ''})")
        print(f"GRADROUTE {label}: {len(live)} gradients, max e(hip) {e_max[0]:.3e}, max e(stock) {e_max[1]:.3e}, factor needed "
              f"{worst[0]:.3f} (e_hip {worst[1]:.3e}, e_stock {worst[2]:.3e}) at {worst[3]}")
        return tags


def _ran(tags, *prefixes):
    return sum(calls for tag, calls in tags.items() if tag.startswith(prefixes))


# ==== T: DeformableTransformer =========================================================================================================
def _say(module):
    """The stock initialisation zeroes the sampling-offset / attention weights (and several biases): give every parameter a say."""
    from alonet.deformable_detr.ops.modules import MSDeformAttn

    gen = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, MSDeformAttn):
                m.sampling_offsets.weight.copy_(_rand(gen, *m.sampling_offsets.weight.shape, scale=0.02))
                m.attention_weights.weight.copy_(_rand(gen, *m.attention_weights.weight.shape, scale=0.05))
                for lin in (m.attention_weights, m.value_proj, m.output_proj):
                    lin.bias.copy_(_rand(gen, *lin.bias.shape, scale=0.2))
            elif isinstance(m, (nn.LayerNorm, nn.GroupNorm)):
                m.weight.copy_(1 + _rand(gen, *m.weight.shape, scale=0.2))
                m.bias.copy_(_rand(gen, *m.bias.shape, scale=0.2))
            elif isinstance(m, nn.MultiheadAttention):
                m.in_proj_bias.copy_(_rand(gen, *m.in_proj_bias.shape, scale=0.2))
                m.out_proj.bias.copy_(_rand(gen, *m.out_proj.bias.shape, scale=0.2))
            elif isinstance(m, (nn.Linear, nn.Conv2d)):
                if m.bias is not None and float(m.bias.abs().max()) == 0.0:
                    m.bias.copy_(_rand(gen, *m.bias.shape, scale=0.2))
                if float(m.weight.abs().max()) == 0.0:   # the box heads' last layer
                    m.weight.copy_(_rand(gen, *m.weight.shape, scale=0.02))
    return module


def _pyramid(dtype):
    gen = torch.Generator().manual_seed(9)
    srcs = [_rand(gen, 2, 256, h, w).to(DEV, dtype) for h, w in SHAPES]
    poss = [_rand(gen, 2, 256, h, w).to(DEV, dtype) for h, w in SHAPES]
    masks = []
    for h, w in SHAPES:   # image 1 is padded on its right quarter and bottom third
        m = torch.zeros(2, h, w, dtype=torch.bool)
        m[1, :, w - max(1, w // 4):] = True
        m[1, h - max(1, h // 3):, :] = True
        masks.append(m.to(DEV))
    return srcs, poss, masks, gen


def _transformer_forward(tr, ins, **kw):
    out = tr(ins["srcs"], ins["masks"], ins["poss"], ins.get("query_embed"), **kw)
    outs = [out["hs"]]
    if tr.two_stage:   # the proposals' layers reach the loss through the encoder's scores and boxes only (the queries are detached)
        outs += [out["enc_outputs_class"], out["enc_outputs_coord_unact"]]
    return outs


@functools.lru_cache(maxsize=None)
def _t_case(dtype, two_stage):
    from alonet.deformable_detr.deformable_transformer import DeformableTransformer
    from alonet.transformers.mlp import MLP

    # two-stage: top-k cuts the encoder's tokens by score, and a cut inside a near-tie would make the routes three different
    # functions of the parameters.  The scoring row of the proposals' class head is widened and the seed is one whose 12th and
    # 13th scores lie 0.6 apart (bf16 moves a score by 0.05, 0.18 at the most): test_two_stage_routes_select_the_same_proposals
    torch.manual_seed(36 if two_stage else 4)
    tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=1024, dropout=0.0,
                               return_intermediate_dec=True, two_stage=two_stage, two_stage_num_proposals=12)
    if two_stage:
        tr.decoder.class_embed = nn.ModuleList([nn.Linear(256, 5) for _ in range(3)])
        tr.decoder.bbox_embed = nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(3)])
    tr = _say(tr)
    if two_stage:
        with torch.no_grad():
            tr.decoder.class_embed[2].weight[0].mul_(16)
    tr = tr.to(DEV, dtype)
    srcs, poss, masks, gen = _pyramid(dtype)
    inputs = dict(srcs=srcs, poss=poss, masks=masks)
    if not two_stage:
        inputs["query_embed"] = _rand(gen, 7, 512).to(DEV, dtype)
    # two-stage: top-k orders the queries by score, and two routes may order a near-tie differently: the probe of ``hs`` is the
    # same for every query, so the loss does not depend on their order
    probe_shape = (lambda o: (*o.shape[:2], 1, o.shape[3]) if o.dim() == 4 else o.shape) if two_stage else None
    return Routes("T", tr, inputs, ["srcs"], _transformer_forward, True, probe_shape)


def _params(case, *prefixes, exclude=()):
    return {n for n, _ in case.module.named_parameters() if n.startswith(prefixes) and n not in exclude}


T_PATTERNS = {
    "a-all": (lambda c: ALL, False),
    "b-all+srcs": (lambda c: ALL, True),
    "c-saliency": (lambda c: set(), True),
    "d-level_embed-frozen": (lambda c: _params(c, "", exclude=("level_embed",)), False),
}


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("pattern", list(T_PATTERNS))
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_transformer_gradients(dtype, pattern, train):
    case = _t_case(dtype, False)
    select, inputs_grad = T_PATTERNS[pattern]
    tags = case.check(select(case), inputs_grad, train, pattern)
    assert _ran(tags, "msda_bwd") == 4 and not _ran(tags, "add_layernorm", "ffn256", "encoder_block", "msda_fwd_fused")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layer", ["encoder.layers.0.", "decoder.layers.0."])
def test_transformer_one_trainable_parameter_at_a_time(dtype, layer):
    """(e): each parameter of the layer alone is trainable, everything else and the inputs frozen, ``eval()``.  What lies upstream of
    the parameter keeps its inference kernels; the parameter's own layer and everything downstream may not."""
    case = _t_case(dtype, False)
    for name in sorted(_params(case, layer)):
        tags = case.check({name}, False, False, f"e-only-{name}")
        if layer.startswith("decoder"):   # the encoder is upstream of every decoder parameter: it stays on its fused route
            assert _ran(tags, "add_layernorm", "encoder_block") and _ran(tags, "msda_fwd_fused") >= 2, (name, tags)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("pattern", ["a-all", "f-enc_output_norm", "f-pos_trans_norm", "f-enc_output", "f-pos_trans"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_two_stage_transformer_gradients(dtype, pattern, train):
    case = _t_case(dtype, True)
    trainable = ALL if pattern == "a-all" else _params(case, pattern[2:] + ".")
    case.check(trainable, False, train, pattern)


def test_two_stage_routes_select_the_same_proposals():
    """The premise of the two-stage cases: top-k picks the same 12 tokens on the three routes (a near-tie at the cut would make
    them three different functions of the parameters)."""
    for dtype in (F32, BF16):
        case = _t_case(dtype, True)
        case.ref(False)
        picks = []
        for kw, module, cast in ((dict(is_tracing=None), case._ref_module, torch.float64), (dict(is_tracing=None), case.module, dtype),
                                 ({}, case.module, dtype)):
            with torch.no_grad():
                out = module.eval()([x.to(cast) for x in case.inputs["srcs"]], case.inputs["masks"],
                                    [x.to(cast) for x in case.inputs["poss"]], None, **kw)
            picks.append(out["init_reference_out"].double().sort(1)[0])
        for got in picks[1:]:   # different tokens differ by a cell of the coarsest map or more; one token by rounding only
            assert float((got - picks[0]).abs().max()) < 0.02, dtype


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_stand_alone_encoder_gradients_on_detached_inputs(dtype, train):
    case = _encoder_case(dtype)
    tags = case.check(ALL, False, train, "encoder-alone")
    assert _ran(tags, "msda_bwd") == 2 and not _ran(tags, "add_layernorm", "ffn256", "encoder_block")


@functools.lru_cache(maxsize=None)
def _encoder_case(dtype):
    from alonet.deformable_detr.deformable_transformer import _level_geometry

    enc = copy.deepcopy(_t_case(dtype, False).module.encoder)
    srcs, poss, masks, _ = _pyramid(dtype)
    flat = lambda xs: torch.cat([x.flatten(2).transpose(1, 2) for x in xs], 1).contiguous()
    spatial_shapes, level_start_index = _level_geometry(SHAPES, torch.device(DEV))
    ratios = torch.tensor([[[1.0, 1.0]] * 4, [[0.75, 0.67]] * 4], dtype=torch.float32, device=DEV)
    inputs = dict(src=flat(srcs), pos=flat(poss), mask=torch.cat([m.flatten(1) for m in masks], 1), ratios=ratios)

    def forward(enc, ins, **kw):
        return [enc(ins["src"], spatial_shapes, level_start_index, ins["ratios"], ins["pos"], ins["mask"], **kw)]

    return Routes("T", enc, inputs, [], forward, True)


def test_frozen_transformer_under_grad_keeps_the_inference_kernels():
    """d): "saliency" in ``eval()`` with the inputs detached as well — nothing can require grad, so grad mode alone costs no kernel —
    and under ``no_grad`` the eval forward launches what it always launched."""
    case = _t_case(BF16, False)
    for p in case.module.parameters():
        p.requires_grad_(False)
    case.module.eval()
    runs = []
    for grad in (True, False):
        with torch.set_grad_enabled(grad), alo_hip.LaunchTimer() as timer:
            _transformer_forward(case.module, case.inputs)
        runs.append({tag: v["calls"] for tag, v in timer.summary().items()})
    assert runs[1] == EVAL_TAGS_BF16
    # grad mode on: the same launches, but for the kernels whose gates name grad mode itself (alo_linear_packed: K >= 512)
    assert runs[0].keys() - runs[1].keys() == set() and all(tag.startswith("linear_packed") for tag in runs[1].keys() - runs[0].keys())
    assert _ran(runs[0], "encoder_block") == 2 and _ran(runs[0], "add_layernorm") == 6 and _ran(runs[0], "msda_fwd_fused") == 4


# what the bf16 2 + 2-layer transformer launches in ``eval()`` under ``no_grad``, recorded before the gates were extended
EVAL_TAGS_BF16 = {"encoder_reference_points": 1, "linear_shortk/N=384,K=256": 3, "value_proj_hm/S=279": 3, "msda_fwd_fused/Lq=279": 2,
                  "encoder_block/tail+ffn+proj/rows=558": 1, "encoder_block/tail+ffn/rows=558": 1, "linear_shortk/N=512,K=256": 2,
                  "linear_shortk/N=256,K=256": 6, "add_layernorm/rows=14": 6, "msda_fwd_fused/Lq=7": 2, "ffn256/F=1024": 2}


# ==== M: MLP ============================================================================================================================
@functools.lru_cache(maxsize=None)
def _m_case(dtype):
    from alonet.transformers.mlp import MLP

    torch.manual_seed(6)
    mlp = _say(MLP(256, 256, 4, 3)).to(DEV, dtype)
    x = _rand(torch.Generator().manual_seed(2), 2, 7, 256).to(DEV, dtype)
    return Routes("M", mlp, dict(x=x), [], lambda m, ins, **kw: [m(ins["x"])], False)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_mlp_one_trainable_parameter_at_a_time(dtype, train):
    case = _m_case(dtype)
    for name in [n for n, _ in case.module.named_parameters()]:
        tags = case.check({name}, False, train, f"only-{name}")
        if name.startswith("layers.2.") and dtype != F32:   # both hidden layers are upstream and frozen: they stay on the MFMA kernel
            assert _ran(tags, "linear_shortk") == 2, tags
    case.check(ALL, False, train, "all")


# ==== B: ResNet-50 bottlenecks and stem =================================================================================================
def _frozen_bn_stats(module, gen):
    for m in module.modules():
        if hasattr(m, "running_var"):
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
            m.running_mean.copy_(_rand(gen, *m.running_mean.shape, scale=0.2))
            m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
            m.bias.copy_(_rand(gen, *m.bias.shape, scale=0.2))
    return module


@functools.lru_cache(maxsize=None)
def _b_case(dtype, kind):
    from alonet.detr.backbone import Bottleneck, FrozenBatchNorm2d

    torch.manual_seed(8)
    cin, planes, stride, down = {"64-256-s1": (64, 64, 1, True), "256-512-s2": (256, 128, 2, True), "256-256-plain": (256, 64, 1, False)}[kind]
    ds = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride=stride, bias=False), FrozenBatchNorm2d(planes * 4)) if down else None
    gen = torch.Generator().manual_seed(3)
    block = _frozen_bn_stats(Bottleneck(cin, planes, stride, 1, ds), gen).to(DEV, dtype)
    x = _rand(gen, 2, cin, 20, 24).to(DEV, dtype).contiguous(memory_format=torch.channels_last)
    return Routes("B", block, dict(x=x), ["x"], lambda m, ins, **kw: [m(ins["x"])], False)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", ["64-256-s1", "256-512-s2", "256-256-plain"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_bottleneck_gradients(dtype, kind, train):
    case = _b_case(dtype, kind)
    patterns = [("only-conv3", {"conv3.weight"}, False), ("only-conv1", {"conv1.weight"}, False), ("input-only", set(), True),
                ("all", ALL, True)]
    if case.module.downsample is not None:
        patterns.insert(1, ("only-downsample", {"downsample.0.weight"}, False))
    for what, trainable, inputs_grad in patterns:
        tags = case.check(trainable, inputs_grad, train, f"{kind} {what}")
        if what == "only-conv3":   # conv1 and conv2 are upstream and frozen: their bias + ReLU stays one HIP pass / GEMM epilogue
            assert _ran(tags, "bias_act", "linear_shortk", "linear_packed") >= (2 if dtype == BF16 else 1), tags


@functools.lru_cache(maxsize=None)
def _stem_case(dtype):
    from alonet.detr.backbone import ResNetBody

    torch.manual_seed(12)
    gen = torch.Generator().manual_seed(5)
    body = _frozen_bn_stats(ResNetBody("resnet50", return_layers={"layer1": "0"}), gen).to(DEV, dtype)
    x = _rand(gen, 2, 3, 40, 56).to(DEV, dtype)
    return Routes("B", body, dict(x=x), ["x"], lambda m, ins, **kw: [m(ins["x"])["0"]], False)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_stem_gradients_with_conv1_trainable(dtype):
    case = _stem_case(dtype)
    case.check({"conv1.weight"}, False, False, "stem only-conv1")
    tags = case.check(set(_params(case, "layer1.2.")), False, False, "stem frozen, layer1.2 trainable")
    assert _ran(tags, "bias_act/C=64") >= 1, tags   # the frozen stem under grad: convolution + ONE bias/ReLU pass


# ==== I: a Deformable-DETR input projection ============================================================================================
@functools.lru_cache(maxsize=None)
def _i_case(dtype):
    from alonet.deformable_detr.deformable_detr import DeformableDETR

    torch.manual_seed(14)
    holder = DeformableDETR.__new__(DeformableDETR)   # _project reads ``input_proj`` alone
    nn.Module.__init__(holder)
    holder.input_proj = nn.ModuleList([nn.Sequential(nn.Conv2d(512, 256, 1), nn.GroupNorm(32, 256)),
                                       nn.Sequential(nn.Conv2d(512, 256, 3, stride=2, padding=1), nn.GroupNorm(32, 256))])
    holder = _say(holder).to(DEV, dtype)
    x = _rand(torch.Generator().manual_seed(7), 2, 512, 10, 12).to(DEV, dtype).contiguous(memory_format=torch.channels_last)
    return Routes("I", holder, dict(x=x), ["x"], lambda m, ins, **kw: [m._project(0, ins["x"]), m._project(1, ins["x"])], False)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_input_projection_gradients(dtype, train):
    case = _i_case(dtype)
    norm = {n for n in _params(case, "input_proj.") if ".1." in n}
    conv = {n for n in _params(case, "input_proj.") if ".0." in n}
    for what, trainable, inputs_grad in (("only-groupnorm", norm, False), ("only-conv", conv, False), ("input-only", set(), True),
                                         ("only-conv-bias", {n for n in conv if n.endswith("bias")}, False), ("all", ALL, True)):
        case.check(trainable, inputs_grad, train, what)


# ==== R: RAFT's update block ============================================================================================================
@functools.lru_cache(maxsize=None)
def _r_case():
    from alonet.raft.update import BasicUpdateBlock

    torch.manual_seed(16)
    block = BasicUpdateBlock(corr_levels=4, corr_radius=4).to(DEV)
    gen = torch.Generator().manual_seed(11)
    inputs = dict(net=torch.tanh(_rand(gen, 1, 128, 8, 12)).to(DEV), inp=torch.relu(_rand(gen, 1, 128, 8, 12)).to(DEV),
                  corr=_rand(gen, 1, 324, 8, 12).to(DEV), flow=_rand(gen, 1, 2, 8, 12).to(DEV))

    def forward(m, ins, **kw):
        net, up_mask, delta = m(ins["net"], ins["inp"], ins["corr"], ins["flow"])
        return [net, up_mask, delta]

    return Routes("R", block, inputs, ["net", "inp", "corr", "flow"], forward, False)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("pattern", ["all", "flow_head.", "gru.convq1.", "encoder.convf2.", "mask.2.", "inputs-only"])
def test_raft_update_block_gradients(pattern, train):
    case = _r_case()
    if pattern == "all":
        case.check(ALL, True, train, pattern)
    elif pattern == "inputs-only":
        case.check(set(), True, train, pattern)
    else:
        tags = case.check(_params(case, pattern), False, train, "only-" + pattern)
        if pattern in ("flow_head.", "mask.2."):   # motion encoder and GRU are upstream and frozen
            assert _ran(tags, "gru_gate") == 2 and _ran(tags, "gru_update") == 2 and _ran(tags, "bias_act_nchw") == 5, tags


def test_raft_update_block_frozen_under_grad_keeps_its_kernels():
    case = _r_case()
    for p in case.module.parameters():
        p.requires_grad_(False)
    runs = []
    for grad in (True, False):
        with torch.set_grad_enabled(grad), alo_hip.LaunchTimer() as timer:
            case.forward(case.module.eval(), case.inputs)
        runs.append({tag: v["calls"] for tag, v in timer.summary().items()})
    assert runs[0] == runs[1] == {"bias_act_nchw/C=256": 3, "bias_act_nchw/C=192": 1, "bias_act_nchw/C=128": 1, "bias_act_nchw/C=64": 1,
                                  "bias_act_nchw/C=126": 1, "gru_gate/C=128": 2, "gru_update/C=128": 2}


# ==== P, W: whole R50 models ============================================================================================================
def _zero_dropout(model):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        elif isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
    return model


def _batch(sizes, dtype, seed):
    import aloscene

    gen = torch.Generator().manual_seed(seed)
    frames = [aloscene.Frame(torch.rand(3, h, w, generator=gen) * 255, normalization="255").norm_resnet() for h, w in sizes]
    return aloscene.Frame.batch_list(frames).to(DEV).to(dtype)


@functools.lru_cache(maxsize=None)
def _p_case(dtype):
    from alonet.deformable_detr_panoptic import DeformableDetrR50Panoptic

    torch.manual_seed(0)
    model = _zero_dropout(_say(DeformableDetrR50Panoptic(num_classes=5, freeze_detr=True, device=torch.device(DEV)))).to(dtype)
    keep = [torch.zeros(300, dtype=torch.bool, device=DEV) for _ in range(2)]
    keep[0][[0, 17, 299]] = True
    keep[1][[5, 6]] = True

    def forward(m, ins, **kw):
        frames = ins["frames"] if ins["frames"].dtype == next(m.parameters()).dtype else ins["frames"].to(next(m.parameters()).dtype)
        return [m(frames, filters=keep, **kw)["pred_masks"]]

    return Routes("P", model, dict(frames=_batch([(128, 160), (96, 160)], dtype, 5)), [], forward, True)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_panoptic_head_gradients_over_a_frozen_detector(dtype, train):
    case = _p_case(dtype)
    head = _params(case, "bbox_attention.", "mask_head.")
    assert head == {n for n, p in case.module.named_parameters() if not n.startswith("detr.")}
    tags = case.check(head, False, train, "freeze_detr")
    if not train:   # the frozen detector under grad in eval(): its fused inference route, attention included
        assert _ran(tags, "add_layernorm", "encoder_block") and _ran(tags, "msda_fwd_fused") == 12 and not _ran(tags, "msda_bwd"), tags
        if dtype == BF16:
            assert _ran(tags, "linear_shortk") and _ran(tags, "bias_act"), tags


@functools.lru_cache(maxsize=None)
def _w_case(dtype):
    from alonet.deformable_detr import DeformableDetrR50

    torch.manual_seed(0)
    model = _zero_dropout(_say(DeformableDetrR50(num_classes=5, aux_loss=True, device=torch.device(DEV)))).to(dtype)

    def forward(m, ins, **kw):
        frames = ins["frames"] if ins["frames"].dtype == next(m.parameters()).dtype else ins["frames"].to(next(m.parameters()).dtype)
        out = m(frames, **kw)
        levels = out["aux_outputs"] + [out]
        return [lvl[k] for lvl in levels for k in ("pred_logits", "pred_boxes")]

    return Routes("W", model, dict(frames=_batch([(192, 256), (160, 224)], dtype, 3)), [], forward, True)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_detector_training_gradients(dtype, monkeypatch):
    """configs[3] in miniature: every trainable parameter's gradient in ``train()``; the stem and ``layer1``, which ``Backbone``
    freezes, keep their HIP epilogues in bf16 while ``layer2`` and up run on stock ops."""
    # MIOpen's default convolution algorithms do not give the same bits twice; 600 x 6 x 8 x 16 sampling points sit behind the
    # backbone, and which of them a route carries across a pixel edge (see FACTOR) would change from run to run
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    case = _w_case(dtype)
    trainable = {n for n, _ in case.module.named_parameters()
                 if not n.startswith("backbone.0.body.") or any(f"body.layer{i}" in n for i in (2, 3, 4))}
    tags = case.check(trainable, False, True, "train_backbone")
    if dtype == BF16:
        layers = {tag for tag in tags if not tag.startswith(("msda_", "encoder_reference_points"))}
        assert layers == {"bias_act/C=64", "linear_shortk/N=64,K=64", "linear_shortk/N=256,K=64", "linear_shortk/N=64,K=256"}, tags
