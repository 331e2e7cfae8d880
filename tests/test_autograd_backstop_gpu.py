"""The wrappers' backstop: every ``alo_hip`` wrapper that writes through raw pointers outside an ``autograd.Function`` refuses,
by name, an operand that requires grad under grad mode — it would otherwise hand back a tensor without ``grad_fn`` (or, in place,
change a tensor behind autograd's back) and training would go on with a missing or wrong gradient.  Under ``torch.no_grad()``,
and with that operand detached, the same call runs and gives the same bits: the check changes no result.  (What the results ARE
is held to fp64 references by each kernel's own test file; a few plain ones are re-checked here against the stock ops.)

``msda_forward`` / ``msda_backward`` and ``corr_*`` sit under ``autograd.Function``s and stay as they are, and so does
``AlternateCorrBlock``'s documented no-autograd contract (tests/test_corr_alt_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import alo_hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SHAPES = [(4, 5), (3, 3), (2, 2), (1, 2)]
S = sum(h * w for h, w in SHAPES)
LQ = 6


def _gen():
    return torch.Generator().manual_seed(31)


def _r(gen, *shape, dtype=BF, scale=1.0, cl=False):
    t = (torch.randn(*shape, generator=gen) * scale).to(DEV, dtype)
    return t.contiguous(memory_format=torch.channels_last) if cl else t


def _geometry():
    shapes = torch.tensor(SHAPES, dtype=torch.int32, device=DEV)
    sizes = [h * w for h, w in SHAPES]
    start = torch.tensor([sum(sizes[:i]) for i in range(4)], dtype=torch.int32, device=DEV)
    return shapes, start


def _mask(gen):
    m = torch.rand(2, S, generator=gen) < 0.25
    m[:, 0] = False
    return m.to(DEV)


def _clone(t):
    return t.clone(memory_format=torch.preserve_format)


# name -> (operands(gen) -> dict, call(operands) -> tuple of results, stock-op reference(operands) -> tuple | None)
def _add_layernorm(g):
    return dict(x=_r(g, 6, 256), residual=_r(g, 6, 256), weight=1 + _r(g, 256, scale=0.2), bias=_r(g, 256, scale=0.2), pos=_r(g, 6, 256))


def _bias_act(g):
    return dict(x=_r(g, 2, 64, 5, 6, cl=True), bias=_r(g, 64), residual=_r(g, 2, 64, 5, 6, cl=True))


def _bias_act_nchw(g):
    return dict(x=_r(g, 1, 8, 4, 6, dtype=torch.float32), bias=_r(g, 8, dtype=torch.float32))


def _gru(g):
    f = dict(dtype=torch.float32)
    return dict(zr=_r(g, 1, 256, 4, 6, **f), bias_zr=_r(g, 256, **f), hx=_r(g, 1, 384, 4, 6, **f), rhx=_r(g, 1, 384, 4, 6, **f),
                q=_r(g, 1, 128, 4, 6, **f), bias_q=_r(g, 128, **f), net=_r(g, 1, 128, 4, 6, **f))


def _gru_gate_call(o):
    zr, rhx = _clone(o["zr"]), _clone(o["rhx"])
    alo_hip.gru_gate_(zr, o["bias_zr"], o["hx"], rhx, 128)
    return zr, rhx


def _gru_update_call(o):
    hx, net = _clone(o["hx"]), _clone(o["net"])
    alo_hip.gru_update_(o["q"], o["bias_q"], o["zr"], hx, 128, net)
    return hx, net


def _linear(k, n):
    return lambda g: dict(x=_r(g, 5, k), weight=_r(g, n, k, scale=k ** -0.5), bias=_r(g, n), residual=_r(g, 5, n))


def _linear_ref(o):
    return ((F.linear(o["x"].float(), o["weight"].float(), o["bias"].float()) + o["residual"].float()).relu(),)


def _conv1x1_strided(g):
    return dict(x=_r(g, 2, 64, 6, 8, cl=True), weight2d=_r(g, 256, 64, scale=0.125), bias=_r(g, 256))


def _ffn256(g):
    return dict(x=_r(g, 5, 256), w1=_r(g, 256, 256, scale=1 / 16), b1=_r(g, 256, scale=0.2), w2=_r(g, 256, 256, scale=1 / 16),
                b2=_r(g, 256, scale=0.2))


def _conv3x3(g):
    return dict(x=_r(g, 1, 64, 6, 8, cl=True), weight=_r(g, 64, 64, 3, 3, scale=1 / 24), bias=_r(g, 64))


def _conv3x3_small(g):
    conv = nn.Conv2d(16, 4, 3, padding=1).to(DEV, BF)
    return dict(x=_r(g, 1, 16, 6, 8, cl=True), conv=conv)


def _stem(g):
    return dict(x=_r(g, 1, 3, 32, 40), weight=_r(g, 64, 3, 7, 7, scale=1 / 12), bias=_r(g, 64))


def _groupnorm_rows(g):
    return dict(x=_r(g, 2, 12, 256), weight=1 + _r(g, 256, scale=0.2), bias=_r(g, 256, scale=0.2))


def _groupnorm_nhwc(g):
    norm = nn.GroupNorm(32, 256).to(DEV, BF)
    with torch.no_grad():
        norm.weight.copy_(1 + _r(g, 256, scale=0.2)); norm.bias.copy_(_r(g, 256, scale=0.2))
    return dict(x=_r(g, 2, 256, 3, 4, cl=True), norm=norm)


def _upsample_add(g):
    return dict(x_low=_r(g, 4, 16, 3, 4, cl=True), fpn=_r(g, 2, 16, 6, 8, cl=True))


def _value(g):
    return dict(value=_r(g, 2, S, 8, 32), mask=_mask(g))


def _value_proj(g):
    return dict(x=_r(g, 2, S, 256), weight=_r(g, 256, 256, scale=1 / 16), bias=_r(g, 256, scale=0.2), mask=_mask(g))


def _msda(dtype, head_major):
    def make(g):
        value = _r(g, 2, 8, S, 32, dtype=dtype) if head_major else _r(g, 2, S, 8, 32, dtype=dtype)
        ref = torch.rand(2, LQ, 4, 2, generator=g).to(DEV)
        return dict(value=value, sampling_offsets=_r(g, 2, LQ, 8, 4, 4, 2, dtype=dtype), attn_logits=_r(g, 2, LQ, 8, 16, dtype=dtype),
                    reference_points=ref)
    return make


def _msda_call(fn):
    def call(o):
        shapes, start = _geometry()
        return (fn(o["value"], shapes, start, o["sampling_offsets"], o["attn_logits"], o["reference_points"]),)
    return call


def _encoder_block(g):
    r = lambda *shape, scale=1.0: _r(g, *shape, scale=scale)
    return dict(src=r(2, S, 256), w1=r(1024, 256, scale=1 / 16), b1=r(1024, scale=0.5), w2=r(256, 1024, scale=1 / 32), b2=r(256, scale=0.5),
                g2=1 + r(256, scale=0.3), e2=r(256, scale=0.3), attn_out=r(2, S, 256), wo=r(256, 256, scale=1 / 16), bo=r(256, scale=0.5),
                g1=1 + r(256, scale=0.3), e1=r(256, scale=0.3), pos=r(2, S, 256), wv=r(256, 256, scale=1 / 16), bv=r(256, scale=0.5),
                wq=r(384, 256, scale=1 / 16), bq=r(384, scale=0.5), mask=_mask(g))


def _encoder_block_call(o):
    return alo_hip.encoder_block(o["src"], o["w1"], o["b1"], o["w2"], o["b2"], (o["g2"], o["e2"], 1e-5),
                                 tail=(o["attn_out"], o["wo"], o["bo"], o["g1"], o["e1"], 1e-5),
                                 nxt=(o["pos"], o["mask"], o["wv"], o["bv"], o["wq"], o["bq"]))


def _pos_sine(g):
    dim_t = 10000 ** (2 * (torch.arange(128) // 2).float() / 128)
    return dict(level_embed=_r(g, 4, 256, dtype=torch.float32), mask=_mask(g), dim_t=dim_t.to(DEV))


def _pos_sine_call(o):
    shapes, start = _geometry()
    return (alo_hip.pos_sine_flat(o["mask"], shapes, start, o["dim_t"], o["level_embed"], True, False, 6.283185307179586, torch.float32),)


def _memory(g):
    keep = ~_mask(g)
    return dict(memory=_r(g, 2, S, 256, dtype=torch.float32), keep=keep, mask=~keep)


def _proposal_queries(g):
    return dict(coords_unact=_r(g, 2, S, 4, dtype=torch.float32), topk=torch.tensor([[3, 0, 7], [1, 1, S - 1]], device=DEV))


CASES = {
    "add_layernorm": (_add_layernorm, lambda o: alo_hip.add_layernorm(o["x"], o["residual"], o["weight"], o["bias"], 1e-5, pos=o["pos"]),
                      lambda o: (F.layer_norm(o["x"].float() + o["residual"].float(), (256,), o["weight"].float(), o["bias"].float(), 1e-5),)),
    "bias_act_": (_bias_act, lambda o: (alo_hip.bias_act_(_clone(o["x"]), o["bias"], o["residual"], True),),
                  lambda o: ((o["x"].float() + o["bias"].float().view(1, -1, 1, 1) + o["residual"].float()).relu(),)),
    "bias_act_nchw_": (_bias_act_nchw, lambda o: (alo_hip.bias_act_nchw_(_clone(o["x"]), o["bias"], True),),
                       lambda o: ((o["x"] + o["bias"].view(1, -1, 1, 1)).relu(),)),
    "gru_gate_": (_gru, _gru_gate_call, None),
    "gru_update_": (_gru, _gru_update_call, None),
    "linear_shortk": (_linear(256, 64), lambda o: (alo_hip.linear_shortk(o["x"], o["weight"], o["bias"], True, o["residual"]),), _linear_ref),
    "linear_packed": (_linear(512, 128), lambda o: (alo_hip.linear_packed(o["x"], o["weight"], o["bias"], True, o["residual"]),), _linear_ref),
    "linear_auto": (_linear(128, 64), lambda o: (alo_hip.linear_auto(o["x"], o["weight"], o["bias"], True, o["residual"]),), _linear_ref),
    "conv1x1_strided": (_conv1x1_strided, lambda o: (alo_hip.conv1x1_strided(o["x"], o["weight2d"], o["bias"], 2, True),),
                        lambda o: (F.conv2d(o["x"].float(), o["weight2d"].float()[:, :, None, None], o["bias"].float(), 2).relu(),)),
    "ffn256": (_ffn256, lambda o: (alo_hip.ffn256(o["x"], o["w1"], o["b1"], o["w2"], o["b2"]),),
               lambda o: (F.linear(F.linear(o["x"].float(), o["w1"].float(), o["b1"].float()).relu().to(BF).float(), o["w2"].float(),
                                   o["b2"].float()),)),
    "conv3x3": (_conv3x3, lambda o: (alo_hip.conv3x3(o["x"], o["weight"], o["bias"], True, 1),),
                lambda o: (F.conv2d(o["x"].float(), o["weight"].float(), o["bias"].float(), 1, 1).relu(),)),
    "conv3x3_small": (_conv3x3_small, lambda o: (alo_hip.conv3x3_small(o["x"], o["conv"]),),
                      lambda o: (F.conv2d(o["x"].float(), o["conv"].weight.float(), o["conv"].bias.float(), 1, 1),)),
    "stem_conv_pool": (_stem, lambda o: (alo_hip.stem_conv_pool(o["x"], o["weight"], o["bias"]),),
                       lambda o: (F.max_pool2d(F.conv2d(o["x"].float(), o["weight"].float(), o["bias"].float(), 2, 3).relu(), 3, 2, 1),)),
    "groupnorm_rows": (_groupnorm_rows, lambda o: (alo_hip.groupnorm_rows(o["x"], o["weight"], o["bias"], 32),),
                       lambda o: (F.group_norm(o["x"].float().transpose(1, 2), 32, o["weight"].float(), o["bias"].float()).transpose(1, 2),)),
    "groupnorm_nhwc": (_groupnorm_nhwc, lambda o: (alo_hip.groupnorm_nhwc(o["x"], o["norm"], relu=True),),
                       lambda o: (F.group_norm(o["x"].float(), 32, o["norm"].weight.float(), o["norm"].bias.float()).relu(),)),
    "upsample_add": (_upsample_add, lambda o: (alo_hip.upsample_add(o["x_low"], o["fpn"]),),
                     lambda o: (o["fpn"].float().repeat_interleave(2, 0) + F.interpolate(o["x_low"].float(), size=(6, 8), mode="nearest"),)),
    "value_head_major": (_value, lambda o: (alo_hip.value_head_major(o["value"], o["mask"]),),
                         lambda o: (o["value"].float().masked_fill(o["mask"][..., None, None], 0).transpose(1, 2),)),
    "value_proj_head_major": (_value_proj, lambda o: (alo_hip.value_proj_head_major(o["x"], o["weight"], o["bias"], o["mask"], 8),),
                              lambda o: (F.linear(o["x"].float(), o["weight"].float(), o["bias"].float())
                                         .masked_fill(o["mask"][..., None], 0).view(2, S, 8, 32).transpose(1, 2),)),
    "msda_forward_fused": (_msda(torch.float32, False), _msda_call(alo_hip.msda_forward_fused), None),
    "msda_forward_fused_hm": (_msda(BF, True), _msda_call(alo_hip.msda_forward_fused_hm), None),
    "encoder_block": (_encoder_block, _encoder_block_call, None),
    "pos_sine_flat": (_pos_sine, _pos_sine_call, None),
    "mask_rows": (_memory, lambda o: (alo_hip.mask_rows(o["memory"], o["keep"]),),
                  lambda o: (o["memory"].masked_fill(~o["keep"][..., None], 0),)),
    "encoder_proposals_masked": (_memory, lambda o: alo_hip.encoder_proposals_masked(o["mask"], SHAPES, o["memory"]), None),
    "proposal_queries": (_proposal_queries, lambda o: alo_hip.proposal_queries(o["coords_unact"], o["topk"], torch.float32), None),
}
# operands of a case that the wrapper under test does not take (they belong to the sibling that shares the maker), and the fixed
# frequencies of the sine encoding, which are no parameter of anything
NOT_TAKEN = {"gru_gate_": {"q", "bias_q", "net"}, "gru_update_": {"bias_zr", "rhx"}, "mask_rows": {"mask"},
             "encoder_proposals_masked": {"keep"}, "pos_sine_flat": {"dim_t"}}
# wrappers whose ``*_supported`` names grad mode itself: with grad mode on they refuse whatever the operands (as before)
NEED_GRAD_MODE_OFF = {"linear_packed", "conv3x3", "conv3x3_small", "stem_conv_pool", "groupnorm_rows", "groupnorm_nhwc", "upsample_add"}


def _slots(name, operands):
    """(label, tensor) for every floating tensor the wrapper takes: tensors themselves, and each parameter of a module."""
    for key, v in operands.items():
        if key in NOT_TAKEN.get(name, ()):
            continue
        if isinstance(v, nn.Module):
            for pname, p in v.named_parameters():
                yield f"{key}.{pname}", p
        elif torch.is_tensor(v) and v.is_floating_point():
            yield key, v


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert (g is None) == (w is None), what
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.grad_fn is None and not g.requires_grad, what
            assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), what


@pytest.mark.parametrize("name", list(CASES))
def test_wrapper_refuses_an_operand_that_requires_grad(name):
    make, call, reference = CASES[name]
    operands = make(_gen())
    for p in (p for v in operands.values() if isinstance(v, nn.Module) for p in v.parameters()):
        p.requires_grad_(False)
    with torch.no_grad():
        want = tuple(call(operands))
    torch.cuda.synchronize()
    slots = list(_slots(name, operands))
    assert slots, name
    for label, t in slots:
        t.requires_grad_(True)
        try:
            with pytest.raises(RuntimeError, match=rf"alo_hip\.{name} has no backward"):
                call(operands)
            with torch.no_grad():                       # grad mode off: the operand's flag is not even looked at
                _same(tuple(call(operands)), want, (name, label, "no_grad"))
        finally:
            t.requires_grad_(False)
    # every operand detached, grad mode on
    if name in NEED_GRAD_MODE_OFF:
        with pytest.raises(RuntimeError, match=name):
            call(operands)
    else:
        _same(tuple(call(operands)), want, (name, "detached"))
    if reference is not None:
        # the stock ops in fp32 on the same operands: one rounding of the result to the storage type (half an eps, relative) and, for
        # the kernels that accumulate rounded products or store an intermediate (ffn256), sums whose terms are of the result's own
        # scale: 3 eps of the largest result, twice what those add up to
        for got, ref in zip(want, reference(operands)):
            ref = ref.float()
            bound = 3 * torch.finfo(got.dtype).eps * float(ref.abs().max())
            assert float((got.float() - ref).abs().max()) <= bound, (name, float((got.float() - ref).abs().max()), bound)


def test_backstop_names_what_is_wrong_and_costs_nothing_without_grad_mode():
    x = torch.randn(4, 256, device=DEV, dtype=BF)
    w = torch.randn(64, 256, device=DEV, dtype=BF, requires_grad=True)
    with pytest.raises(RuntimeError, match="call it under torch.no_grad"):
        alo_hip.linear_shortk(x, w)
    with torch.no_grad():
        assert alo_hip.linear_shortk(x, w).grad_fn is None
    assert alo_hip.linear_shortk(x, w.detach()).grad_fn is None

