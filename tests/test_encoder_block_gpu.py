"""alo_hip.encoder_block (csrc/encoder_block.hip): the row-local part of an encoder layer in one kernel, against the chain of
launches it stands in for — bit for bit — and the encoder's fused loop against ``ALO_ENC_BLOCK=off``."""
import ctypes

import pytest
import torch

import alo_hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
FORMS = ["ffn", "ffn+proj", "tail+ffn", "tail+ffn+proj"]   # "A without projections", "A only", and both with stage B


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def weights():
    """Random non-trivial parameters of one layer (and the next layer's projections) per hidden width; never modified."""
    gen = torch.Generator().manual_seed(11)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen) * scale).to(DEV, BF)
    out = {}
    for Fh in (1024, 256):
        out[Fh] = dict(
            wo=r(256, 256, scale=1 / 16), bo=r(256, scale=0.5), g1=1 + r(256, scale=0.3), e1=r(256, scale=0.3),
            w1=r(Fh, 256, scale=1 / 16), b1=r(Fh, scale=0.5), w2=r(256, Fh, scale=Fh ** -0.5), b2=r(256, scale=0.5),
            g2=1 + r(256, scale=0.3), e2=r(256, scale=0.3),
            wv=r(256, 256, scale=1 / 16), bv=r(256, scale=0.5), wq=r(384, 256, scale=1 / 16), bq=r(384, scale=0.5))
    return out


def _inputs(batch, S, seed, mask):
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(batch, S, 256, generator=gen).to(DEV, BF)
    src, attn_out, pos = r(), r(), r()
    m = None
    if mask:
        m = torch.rand(batch, S, generator=gen) < 0.3
        m[-1] = batch > 1   # a fully masked batch item
        m = m.to(DEV)
    return src, attn_out, pos, m


def _chain(form, w, src, attn_out, pos, mask, eps1=1e-5, eps2=1e-5):
    """The separate launches: linear_auto, add_layernorm, ffn256, add_layernorm(pos=...), value_proj_head_major, merged linear_auto."""
    x = src
    if "tail" in form:
        x = alo_hip.add_layernorm(alo_hip.linear_auto(attn_out, w["wo"], w["bo"]), src, w["g1"], w["e1"], eps1)
    h = alo_hip.ffn256(x, w["w1"], w["b1"], w["w2"], w["b2"])
    if "proj" not in form:
        return alo_hip.add_layernorm(h, x, w["g2"], w["e2"], eps2), None, None
    out, query = alo_hip.add_layernorm(h, x, w["g2"], w["e2"], eps2, pos=pos)
    return out, alo_hip.value_proj_head_major(out, w["wv"], w["bv"], mask, 8), alo_hip.linear_auto(query, w["wq"], w["bq"])


def _block(form, w, src, attn_out, pos, mask, eps1=1e-5, eps2=1e-5):
    tail = (attn_out, w["wo"], w["bo"], w["g1"], w["e1"], eps1) if "tail" in form else None
    nxt = (pos, mask, w["wv"], w["bv"], w["wq"], w["bq"]) if "proj" in form else None
    return alo_hip.encoder_block(src, w["w1"], w["b1"], w["w2"], w["b2"], (w["g2"], w["e2"], eps2), tail=tail, nxt=nxt)


def _assert_same(got, want, what):
    for name, g, x in zip(("src", "value", "offsets_logits"), got, want):
        assert (g is None) == (x is None), (what, name)
        if g is not None:
            assert g.shape == x.shape and torch.equal(_bits(g), _bits(x)), (what, name, int((_bits(g) != _bits(x)).sum()))


# 1 x 1 .. 2 x 65: ragged single tiles; 3 x 1000: ragged last tile and batch boundaries inside a tile (head-major write);
# 1 x 40000: 625 tiles on 512 workgroups, the persistent loop wraps; 8 x 300: the decoder-like row count
@pytest.mark.parametrize("batch,S", [(1, 1), (1, 63), (1, 64), (2, 65), (3, 1000), (1, 40000), (8, 300)])
@pytest.mark.parametrize("form", FORMS)
def test_block_equals_the_unfused_chain_bit_for_bit(weights, form, batch, S):
    for Fh in (1024, 256):
        for mask in ((False, True) if "proj" in form else (False,)):
            args = _inputs(batch, S, seed=batch * 100003 + S, mask=mask)
            eps = (1e-5, 1e-5) if Fh == 1024 else (1e-3, 1e-6)   # each LayerNorm takes its own eps
            _assert_same(_block(form, weights[Fh], *args, *eps), _chain(form, weights[Fh], *args, *eps), (form, Fh, mask))


@pytest.mark.parametrize("form", FORMS)
def test_a_nan_stays_in_its_row(weights, form):
    w = weights[1024]
    src, attn_out, pos, _ = _inputs(2, 65, seed=3, mask=False)
    clean = _block(form, w, src, attn_out, pos, None)
    bad_src, bad_attn = src.clone(), attn_out.clone()
    bad_src[1, 7, 100] = float("nan")
    bad_attn[1, 7, 5] = float("nan")
    got = _block(form, w, bad_src, bad_attn, pos, None)
    keep = torch.ones(2, 65, dtype=torch.bool, device=DEV)
    keep[1, 7] = False
    assert torch.isnan(got[0][1, 7].float()).all()
    assert torch.equal(_bits(got[0][keep]), _bits(clean[0][keep]))
    if "proj" in form:
        assert torch.isnan(got[1][1, :, 7].float()).all() and torch.isnan(got[2][1, 7].float()).all()
        assert torch.equal(_bits(got[1].transpose(1, 2)[keep]), _bits(clean[1].transpose(1, 2)[keep]))
        assert torch.equal(_bits(got[2][keep]), _bits(clean[2][keep]))
    # and the other rows are the chain's (inside the row only the NaN-ness is compared: which operand's NaN payload an addition keeps is not part of the contract)
    want = _chain(form, w, bad_src, bad_attn, pos, None)
    assert torch.equal(_bits(got[0][keep]), _bits(want[0][keep])) and torch.isnan(want[0][1, 7].float()).all()


def test_argument_errors_are_reported_before_anything_is_enqueued(weights):
    w = weights[1024]
    lib = alo_hip.lib()
    N, S, Fh = 2, 70, 1024
    big = lambda cols: torch.zeros(N * S * cols + 64, dtype=BF, device=DEV)   # room for a 2-byte shifted view
    bufs = dict(attn=big(256), src=big(256), out=big(256), pos=big(256), value=big(256), both=big(384))
    packed = {k: alo_hip.pack_mfma_b(w[k]) for k in ("wo", "w1", "w2", "wv", "wq")}
    p = lambda t: t.data_ptr()

    def call(dtype=alo_hip.ALO_BF16, Fh=Fh, **over):
        a = dict(attn=p(bufs["attn"]), wo=p(packed["wo"]), bo=p(w["bo"]), g1=p(w["g1"]), e1=p(w["e1"]), src=p(bufs["src"]),
                 w1=p(packed["w1"]), b1=p(w["b1"]), w2=p(packed["w2"]), b2=p(w["b2"]), g2=p(w["g2"]), e2=p(w["e2"]),
                 out=p(bufs["out"]), pos=p(bufs["pos"]), mask=None, wv=p(packed["wv"]), bv=p(w["bv"]), wq=p(packed["wq"]),
                 bq=p(w["bq"]), value=p(bufs["value"]), both=p(bufs["both"]))
        a.update(over)
        ptrs = [None if v is None else ctypes.c_void_p(v) for v in a.values()]
        return lib.alo_encoder_block(*ptrs, N, S, Fh, 1e-5, 1e-5, dtype, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    torch.cuda.synchronize()
    for name in ("src", "w1", "b1", "w2", "b2", "g2", "e2", "out"):              # the always-needed pointers
        assert call(**{name: None}) != 0, name
    for name in ("attn", "wo", "bo", "g1", "e1"):                              # a tail with a piece missing
        assert call(**{name: None}) != 0, name
    for name in ("pos", "wv", "bv", "wq", "bq", "value", "both"):               # projections with a piece missing
        assert call(**{name: None}) != 0, name
    assert "null pointer" in alo_hip.lib().alo_last_error().decode()
    for hidden in (0, 100, 1000, -256):
        assert call(Fh=hidden) != 0, hidden
    assert "multiple of 256" in alo_hip.lib().alo_last_error().decode()
    for name in ("attn", "src", "out", "pos", "value", "both", "wo", "w1", "w2", "wv", "wq"):
        base = bufs[name] if name in bufs else packed[name]
        assert call(**{name: p(base) + 2}) != 0, name
    assert "aligned" in alo_hip.lib().alo_last_error().decode()
    assert call(dtype=alo_hip.ALO_F32) != 0 and "bf16 only" in alo_hip.lib().alo_last_error().decode()
    for out_name, in_name in (("out", "src"), ("value", "src"), ("both", "pos"), ("value", "out"), ("both", "attn")):
        assert call(**{out_name: p(bufs[in_name])}) != 0, (out_name, in_name)
    assert "overlaps" in alo_hip.lib().alo_last_error().decode()
    torch.cuda.synchronize()
    assert all(float(bufs[k].float().abs().max()) == 0.0 for k in ("out", "value", "both"))   # nothing ran
    # the binding refuses other dtypes itself
    with pytest.raises(RuntimeError):
        alo_hip.encoder_block(torch.zeros(1, 8, 256, device=DEV), w["w1"], w["b1"], w["w2"], w["b2"], (w["g2"], w["e2"], 1e-5))
    assert call() == 0   # and the same arguments, whole, do run
    torch.cuda.synchronize()


# ---- the encoder's loop ------------------------------------------------------------------------------------------------------------
SHAPES = ((12, 17), (6, 9), (3, 5), (2, 3))


def _encoder(dtype, layers=2):
    from alonet.deformable_detr.deformable_transformer import DeformableTransformer

    torch.manual_seed(4)
    enc = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=layers, num_decoder_layers=1).encoder
    with torch.no_grad():   # the stock initialisation zeroes the offset / attention weights: give every parameter a say
        for layer in enc.layers:
            a = layer.self_attn
            a.sampling_offsets.weight.normal_(0, 0.02)
            a.attention_weights.weight.normal_(0, 0.05)
            for lin in (a.value_proj, a.output_proj, layer.linear1, layer.linear2):
                lin.bias.normal_(0, 0.2)
            for norm in (layer.norm1, layer.norm2):
                norm.weight.normal_(1, 0.2)
                norm.bias.normal_(0, 0.2)
    return enc.to(DEV, dtype).eval()


def _encoder_inputs(dtype):
    from alonet.deformable_detr.deformable_transformer import _level_geometry

    gen = torch.Generator().manual_seed(9)
    S = sum(h * w for h, w in SHAPES)
    src = torch.randn(2, S, 256, generator=gen).to(DEV, dtype)
    pos = torch.randn(2, S, 256, generator=gen).to(DEV, dtype)
    masks = []
    for h, w in SHAPES:   # image 1 is padded on its right quarter and bottom third
        m = torch.zeros(2, h, w, dtype=torch.bool)
        m[1, :, w - max(1, w // 4):] = True
        m[1, h - max(1, h // 3):, :] = True
        masks.append(m.flatten(1))
    mask = torch.cat(masks, 1).to(DEV)
    ratios = torch.tensor([[[1.0, 1.0]] * 4, [[0.75, 0.67]] * 4], dtype=torch.float32, device=DEV)
    spatial_shapes, level_start_index = _level_geometry(SHAPES, torch.device(DEV))
    return src, spatial_shapes, level_start_index, ratios, pos, mask


def _run(enc, inputs, monkeypatch, mode):
    monkeypatch.setenv("ALO_ENC_BLOCK", mode)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        memory = enc(*inputs)
    return memory, timer.summary()


def test_encoder_loop_equals_the_separate_launches(monkeypatch):
    enc, inputs = _encoder(BF), _encoder_inputs(BF)
    want, tags_off = _run(enc, inputs, monkeypatch, "off")
    assert not any(tag.startswith("encoder_block") for tag in tags_off)
    assert sum(v["calls"] for tag, v in tags_off.items() if tag.startswith("add_layernorm")) == 4
    rows = inputs[0].shape[0] * inputs[0].shape[1]
    got, tags = _run(enc, inputs, monkeypatch, "on")
    assert torch.equal(_bits(got), _bits(want))
    assert {tag: v["calls"] for tag, v in tags.items() if tag.startswith("encoder_block")} == {
        f"encoder_block/tail+ffn+proj/rows={rows}": 1, f"encoder_block/tail+ffn/rows={rows}": 1}
    assert not any(tag.startswith(("ffn256", "add_layernorm")) for tag in tags)
    assert sum(v["calls"] for tag, v in tags.items() if tag.startswith("msda_fwd")) == 2


def test_fp32_and_training_keep_the_separate_launches(monkeypatch):
    for dtype, train in ((torch.float32, False), (BF, True)):
        enc = _encoder(dtype).train(train)
        _, tags = _run(enc, _encoder_inputs(dtype), monkeypatch, "on")
        assert tags and not any(tag.startswith("encoder_block") for tag in tags), (dtype, train)


def test_graphed_forward_replays_the_fused_loop(monkeypatch):
    """GraphedForward captures the new path unchanged: replay == eager == the separate launches, on DeformableDETR-R50."""
    import aloscene
    from alonet.common import GraphedForward
    from alonet.deformable_detr import DeformableDetrR50

    torch.manual_seed(0)
    model = DeformableDetrR50(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval().to(BF)
    gen = torch.Generator().manual_seed(5)
    fr = [aloscene.Frame(torch.rand(3, 256 - 32 * i, 320, generator=gen) * 255, normalization="255").norm_resnet() for i in range(2)]
    frames = aloscene.Frame.batch_list(fr).to(DEV).to(BF)
    with torch.no_grad():
        monkeypatch.setenv("ALO_ENC_BLOCK", "off")
        want = {k: model(frames)[k].clone() for k in ("pred_logits", "pred_boxes")}
        monkeypatch.setenv("ALO_ENC_BLOCK", "on")
        with alo_hip.LaunchTimer() as timer:
            eager = model(frames)
        assert sum(v["calls"] for tag, v in timer.summary().items() if tag.startswith("encoder_block")) == 6
        graphed = GraphedForward(model)
        for _ in range(2):
            got = graphed(frames)
            for key in want:
                assert torch.equal(got[key], eager[key]) and torch.equal(got[key], want[key]), key
