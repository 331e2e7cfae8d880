"""The routes behind ``ALO_ATTENTION=fused``: DETR's transformer on the library (alonet/detr/transformer.py, ``_forward_fused``) and
the Deformable-DETR decoder's self-attention (``_attend`` of alonet/transformers/fused_layers.py) against the reference's fixtures,
the autograd gate, and a captured graph of a whole ``DetrR50``."""
import contextlib

import numpy as np
import pytest
import torch

import aloscene
import alo_hip
from helpers import formula_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = torch.from_numpy
FP32_TOL = 1e-3               # the project's bar for an fp32 route against the reference's fp64 outputs (test_models_gpu.py)
BF16_TRANSFORMER_TOL = 0.1    # test_models_gpu.py: max-abs on hs / memory through the bf16 layers vs the reference's fp64 outputs


@contextlib.contextmanager
def attention_launches():
    """Counts the launches of alo_encoder_block that carry ALO_BLOCK_ATTENTION, at the launch seam."""
    real, seen = alo_hip._launch, []

    def launch(symbol, device, tag, nbytes, flops, *args, relaunch=False):
        if symbol == "alo_encoder_block" and isinstance(args[-1], int) and args[-1] & alo_hip.ALO_BLOCK_ATTENTION:
            seen.append(tag)
        return real(symbol, device, tag, nbytes, flops, *args, relaunch=relaunch)

    alo_hip._launch = launch
    try:
        yield seen
    finally:
        alo_hip._launch = real


def _detr_transformer(dtype):
    from alonet.detr import Transformer

    tr = Transformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=512, dropout=0.0,
                     return_intermediate_dec=True).double().eval()
    assert not tr.load_state_dict(formula_state_dict(tr.state_dict())).missing_keys
    return tr.to(DEV, dtype)


def _g22_args(g, dtype):
    return (t(g["src"]).to(DEV, dtype), t(g["mask"]).to(DEV), t(g["query"]).to(DEV, dtype), t(g["pos"]).to(DEV, dtype))


def _g22_errors(out, g):
    return {key: float(np.abs(out[key].double().cpu().numpy() - g[key]).max()) for key in ("hs", "memory")}


def test_g22_fp32_on_the_library(golden, monkeypatch):
    g = golden("g22_detr_transformer_d256.npz")
    tr = _detr_transformer(torch.float32)
    monkeypatch.delenv("ALO_ATTENTION", raising=False)
    with torch.no_grad(), attention_launches() as seen:
        stock = tr(*_g22_args(g, torch.float32))
    assert seen == []
    monkeypatch.setenv("ALO_ATTENTION", "fused")
    with torch.no_grad(), attention_launches() as seen:
        out = tr(*_g22_args(g, torch.float32))
    assert len(seen) == 2 + 2 * 2, seen                      # 2 encoder + 2 x (self, cross) decoder attentions
    assert sorted(set(seen)) == ["attention/Lq=37/Lk=37", "attention/Lq=37/Lk=70", "attention/Lq=70/Lk=70"]
    errs = _g22_errors(out, g)
    print("G22 fp32, routed max-abs:", errs, "stock:", _g22_errors(stock, g))
    assert max(errs.values()) <= FP32_TOL, errs
    for key in ("hs", "memory"):                             # the shapes and layouts of the sequence-first stock route
        assert out[key].shape == stock[key].shape and out[key].stride() == stock[key].stride() and out[key].dtype == stock[key].dtype


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_g22_16_bit_routed_against_stock(golden, monkeypatch, dtype):
    """The two routes round at different points; the routed error against the fixture may exceed the stock ops' by half."""
    g = golden("g22_detr_transformer_d256.npz")
    tr = _detr_transformer(dtype)
    monkeypatch.delenv("ALO_ATTENTION", raising=False)
    with torch.no_grad():
        stock = _g22_errors(tr(*_g22_args(g, dtype)), g)
    monkeypatch.setenv("ALO_ATTENTION", "fused")
    with torch.no_grad(), attention_launches() as seen:
        routed = _g22_errors(tr(*_g22_args(g, dtype)), g)
    assert len(seen) == 6
    print(f"G22 {dtype}, max-abs against the fixture: routed {routed} stock {stock}")
    for key in routed:
        assert routed[key] <= 1.5 * stock[key], (key, routed, stock)


@pytest.mark.parametrize("dec_block", ["on", "off"])
@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, BF16_TRANSFORMER_TOL), (torch.float32, FP32_TOL)], ids=["bf16", "f32"])
def test_g12_deformable_decoder_with_the_switch_on(golden, monkeypatch, dtype, tol, dec_block):
    from alonet.deformable_detr import DeformableTransformer

    g = golden("g12_deformable_transformer_d256.npz")
    d_model, nhead, enc, dec, ffn, L, dec_p, enc_p = (int(x) for x in g["cfg"])
    tr = DeformableTransformer(d_model=d_model, nhead=nhead, num_encoder_layers=enc, num_decoder_layers=dec, dim_feedforward=ffn,
                               dropout=0.0, return_intermediate_dec=True, num_feature_levels=L, dec_n_points=dec_p,
                               enc_n_points=enc_p).double().eval()
    assert not tr.load_state_dict(formula_state_dict(tr.state_dict())).missing_keys
    tr = tr.to(DEV, dtype)
    cast = lambda a: t(a).to(DEV, dtype)  # noqa: E731
    srcs, poss = [cast(g[f"src{i}"]) for i in range(L)], [cast(g[f"pos{i}"]) for i in range(L)]
    masks = [t(g[f"mask{i}"]).to(DEV) for i in range(L)]
    monkeypatch.setenv("ALO_ATTENTION", "fused")
    monkeypatch.setenv("ALO_DEC_BLOCK", dec_block)
    monkeypatch.setattr(alo_hip, "DECODER_BLOCK_MIN_ROWS", 1)   # G12 has fewer rows than the chains are routed from: take them anyway
    with torch.no_grad(), attention_launches() as seen, alo_hip.LaunchTimer() as timer:
        out = tr(srcs, masks, poss, cast(g["query_embed"]))
    assert len(seen) == dec, seen                            # one self-attention per decoder layer
    chained = any(tag.startswith("decoder_block_a") for tag in timer.summary())
    assert chained == (dec_block == "on" and dtype == torch.bfloat16)   # the chains are bf16 only: packed [q; k] from chain B
    errs = {"hs": np.abs(out["hs"].double().cpu().numpy() - g["hs"]).max(),
            "ref": np.abs(out["inter_references_out"].double().cpu().numpy() - g["inter_references_out"]).max()}
    for i in range(L):
        errs[f"memory{i}"] = np.abs(out["memory"][i].double().cpu().numpy() - g[f"memory{i}"]).max()
    print(f"G12 {dtype} ALO_DEC_BLOCK={dec_block}, max-abs:", {k: float(v) for k, v in errs.items()})
    assert max(errs.values()) <= tol, errs


def test_trainable_parameters_take_the_stock_ops_and_the_same_gradients(golden, monkeypatch):
    g = golden("g22_detr_transformer_d256.npz")
    tr = _detr_transformer(torch.float32)
    assert all(p.requires_grad for p in tr.parameters()) and torch.is_grad_enabled()
    grads = []
    for value in (None, "fused"):
        monkeypatch.delenv("ALO_ATTENTION", raising=False) if value is None else monkeypatch.setenv("ALO_ATTENTION", value)
        tr.zero_grad(set_to_none=True)
        with attention_launches() as seen:
            out = tr(*_g22_args(g, torch.float32))
        assert seen == [] and out["hs"].grad_fn is not None
        (out["hs"].square().mean() + out["memory"].square().mean()).backward()
        grads.append({n: p.grad.clone() for n, p in tr.named_parameters()})
    assert all(v is not None and torch.isfinite(v).all() for v in grads[0].values())
    for name in grads[0]:
        torch.testing.assert_close(grads[1][name], grads[0][name], rtol=0, atol=0, msg=name)


def test_the_decoder_helper_and_the_wrapper_under_autograd(monkeypatch):
    from alonet.transformers.fused_layers import _attend

    monkeypatch.setenv("ALO_ATTENTION", "fused")
    mha = torch.nn.MultiheadAttention(256, 8).to(DEV).eval()
    qk, v = torch.randn(2, 9, 512, device=DEV), torch.randn(2, 9, 256, device=DEV)
    with attention_launches() as seen:
        with torch.no_grad():
            fused = _attend(mha, qk, v)
        assert len(seen) == 1
        stock = _attend(mha, qk.clone().requires_grad_(), v)     # grad mode, an operand that requires grad: the stock op
        assert len(seen) == 1 and stock.grad_fn is not None
    torch.testing.assert_close(fused, stock.detach(), rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.attention(qk[..., :256].clone().requires_grad_(), qk[..., 256:], v)


class _GemmProjection(torch.nn.Module):
    """``Detr.input_proj`` (a 1x1 ``nn.Conv2d``) on the library's GEMM, as the Deformable-DETR model runs its input projections.
    The stock convolution is not reproducible bit for bit from one eager call to the next on this stack (measured with the switch
    off as well), which would make "the replay equals the eager result" a statement about that op instead of about the route."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def forward(self, x):
        from alonet.detr.backbone import conv1x1_as_gemm

        return conv1x1_as_gemm(x, self.conv.weight, self.conv.bias)


def test_graphed_forward_of_detr_r50_with_the_switch_on_replays_the_eager_result(monkeypatch):
    from alonet.common import GraphedForward
    from alonet.detr import DetrR50

    monkeypatch.setenv("ALO_ATTENTION", "fused")
    torch.manual_seed(0)
    model = DetrR50(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval().to(torch.bfloat16)
    model.input_proj = _GemmProjection(model.input_proj)
    gen = torch.Generator().manual_seed(5)
    frames = aloscene.Frame.batch_list([aloscene.Frame(torch.rand(3, 160 - 32 * i, 224, generator=gen) * 255,
                                                       normalization="255").norm_resnet() for i in range(2)]).to(DEV).to(torch.bfloat16)
    assert bool(frames.mask.as_tensor().any())
    graphed = GraphedForward(model)
    with torch.no_grad():
        with attention_launches() as seen:
            want = model(frames)
        assert len(seen) == 6 + 2 * 6, seen
        again = model(frames)
        assert all(torch.equal(again[key], want[key]) for key in ("pred_logits", "pred_boxes"))   # well posed: eager repeats itself
        for _ in range(2):
            got = graphed(frames)
            for key in ("pred_logits", "pred_boxes"):
                assert torch.isfinite(want[key]).all() and torch.equal(got[key], want[key]), key
