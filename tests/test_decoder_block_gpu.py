"""alo_hip.decoder_block_a / decoder_block_b (the flagged forms of alo_encoder_block, csrc/encoder_block.hip): the two row-local
chains of a decoder layer in one kernel each, against the chain of launches they stand in for — bit for bit, at both tile heights —
and the decoder's fused loop against ``ALO_DEC_BLOCK=off``."""
import pytest
import torch

import alo_hip
from guarded import GuardedLaunches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
EPS = (1e-5, 1e-3)   # each LayerNorm takes its own eps
# 5: one partial tile; 3 x 37: ragged at both tile heights; 300, 600; 8 x 300: the headline's count, 32-row tiles; 8 x 2100: 263
# 64-row tiles, more than the chip has compute units, so 64-row tiles are chosen and the persistent loop wraps
ROWS = [(1, 5), (3, 37), (1, 300), (2, 300), (8, 300), (8, 2100)]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def weights():
    """Random non-trivial parameters of one decoder layer (and the next layer's input projections) per hidden width; never modified."""
    gen = torch.Generator().manual_seed(23)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen) * scale).to(DEV, BF)
    out = {}
    for Fh in (1024, 256):
        out[Fh] = dict(
            wo=r(256, 256, scale=1 / 16), bo=r(256, scale=0.5), g2=1 + r(256, scale=0.3), e2=r(256, scale=0.3),       # self-attention tail
            wq=r(384, 256, scale=1 / 16), bq=r(384, scale=0.5),                                                        # offsets + logits
            wc=r(256, 256, scale=1 / 16), bc=r(256, scale=0.5), g1=1 + r(256, scale=0.3), e1=r(256, scale=0.3),       # cross-attention tail
            w1=r(Fh, 256, scale=1 / 16), b1=r(Fh, scale=0.5), w2=r(256, Fh, scale=Fh ** -0.5), b2=r(256, scale=0.5),
            g3=1 + r(256, scale=0.3), e3=r(256, scale=0.3),
            wv=r(256, 256, scale=1 / 16), bv=r(256, scale=0.5), wqk=r(512, 256, scale=1 / 16), bqk=r(512, scale=0.5))
    return out


def _inputs(batch, L, seed=0):
    gen = torch.Generator().manual_seed(seed + batch * 100003 + L)
    r = lambda: torch.randn(batch, L, 256, generator=gen).to(DEV, BF)
    return r(), r(), r()   # attention output, tgt, query_pos


def _chain_a(w, attn_out, tgt, pos):
    """The separate launches: linear_auto, add_layernorm(pos=...), the merged linear_auto."""
    tgt1, query = alo_hip.add_layernorm(alo_hip.linear_auto(attn_out, w["wo"], w["bo"]), tgt, w["g2"], w["e2"], EPS[0], pos=pos)
    return tgt1, alo_hip.linear_auto(query, w["wq"], w["bq"])


def _block_a(w, attn_out, tgt, pos, tile_rows=None):
    return alo_hip.decoder_block_a(attn_out, tgt, pos, w["wo"], w["bo"], (w["g2"], w["e2"], EPS[0]), w["wq"], w["bq"], tile_rows=tile_rows)


def _chain_b(w, attn_out, tgt1, pos):
    """The separate launches: linear_auto, add_layernorm, ffn256, add_layernorm(pos=...), and the next layer's qk and v linear_auto."""
    tgt2 = alo_hip.add_layernorm(alo_hip.linear_auto(attn_out, w["wc"], w["bc"]), tgt1, w["g1"], w["e1"], EPS[0])
    out, query = alo_hip.add_layernorm(alo_hip.ffn256(tgt2, w["w1"], w["b1"], w["w2"], w["b2"]), tgt2, w["g3"], w["e3"], EPS[1], pos=pos)
    return out, alo_hip.linear_auto(out, w["wv"], w["bv"]), alo_hip.linear_auto(query, w["wqk"], w["bqk"])


def _block_b(w, attn_out, tgt1, pos, tile_rows=None):
    return alo_hip.decoder_block_b(attn_out, tgt1, pos, w["wc"], w["bc"], (w["g1"], w["e1"], EPS[0]), w["w1"], w["b1"], w["w2"], w["b2"],
                                   (w["g3"], w["e3"], EPS[1]), w["wv"], w["bv"], w["wqk"], w["bqk"], tile_rows=tile_rows)


CHAINS = {"a": (_chain_a, _block_a, ("tgt1", "offsets_logits")), "b": (_chain_b, _block_b, ("out", "v", "qk"))}


def _assert_same(names, got, want, what):
    assert len(got) == len(want) == len(names)
    for name, g, x in zip(names, got, want):
        assert g.shape == x.shape and g.is_contiguous() and x.is_contiguous(), (what, name)
        assert torch.equal(_bits(g), _bits(x)), (what, name, int((_bits(g) != _bits(x)).sum()))


@pytest.mark.parametrize("batch,L", ROWS)
@pytest.mark.parametrize("chain", ["a", "b"])
def test_block_equals_the_unfused_chain_bit_for_bit_at_both_heights(weights, chain, batch, L):
    reference, block, names = CHAINS[chain]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for Fh in ((1024, 256) if chain == "b" else (1024,)):
        args = _inputs(batch, L)
        want = reference(weights[Fh], *args)
        with alo_hip.LaunchTimer() as timer:
            got = block(weights[Fh], *args)
        # which height ran: the launch tag carries the flag the call was made with
        auto = 32 if (batch * L + 63) // 64 < cus else 64
        assert list(timer.summary()) == [f"decoder_block_{chain}/rows={batch * L}/tile={auto}"]
        if cus == 256:
            assert auto == (64 if batch * L == 16800 else 32)
        _assert_same(names, got, want, (chain, Fh, "auto"))
        for tile_rows in (32, 64):
            _assert_same(names, block(weights[Fh], *args, tile_rows=tile_rows), want, (chain, Fh, tile_rows))


@pytest.mark.parametrize("chain", ["a", "b"])
def test_a_non_finite_row_stays_in_its_row(weights, chain):
    reference, block, names = CHAINS[chain]
    w = weights[1024]
    attn_out, tgt, pos = _inputs(3, 37, seed=1)
    keep = torch.ones(3, 37, dtype=torch.bool, device=DEV)
    keep[1, 7] = keep[2, 36] = keep[0, 0] = False
    for tile_rows in (32, 64):
        clean = block(w, attn_out, tgt, pos, tile_rows=tile_rows)
        bad_attn, bad_tgt, bad_pos = attn_out.clone(), tgt.clone(), pos.clone()
        bad_attn[1, 7, 5] = float("nan")
        bad_tgt[2, 36, 100] = float("inf")
        bad_pos[0, 0, 255] = float("nan")
        got = block(w, bad_attn, bad_tgt, bad_pos, tile_rows=tile_rows)
        want = reference(w, bad_attn, bad_tgt, bad_pos)
        for name, g, c, x in zip(names, got, clean, want):
            assert torch.equal(_bits(g[keep]), _bits(c[keep])) and torch.equal(_bits(g[keep]), _bits(x[keep])), name
            # inside the row only the NaN-ness is compared: which operand's NaN payload an addition keeps is not part of the contract
            assert torch.equal(torch.isnan(g.float()), torch.isnan(x.float())), name
        assert torch.isnan(got[0][1, 7].float()).all() and torch.isnan(got[0][2, 36].float()).all()   # LayerNorm spreads it over the row
        assert torch.isnan(got[-1][0, 0].float()).all()                                                # the query took pos's NaN


@pytest.mark.parametrize("chain", ["a", "b"])
def test_repeated_launches_give_equal_bits(weights, chain):
    _, block, names = CHAINS[chain]
    args = _inputs(8, 300, seed=2)
    first = block(weights[1024], *args)
    for _ in range(3):
        _assert_same(names, block(weights[1024], *args), first, chain)


@pytest.mark.parametrize("batch,L", ROWS[:2])
@pytest.mark.parametrize("chain", ["a", "b"])
def test_both_modes_stay_in_their_buffers(weights, chain, batch, L):
    reference, block, names = CHAINS[chain]
    args = _inputs(batch, L, seed=3)
    want = reference(weights[1024], *args)
    for tile_rows in (32, 64):
        with GuardedLaunches() as g:
            got = block(weights[1024], *args, tile_rows=tile_rows)
        assert [symbol for symbol, _ in g.seen] == ["alo_encoder_block"] and g.seen[0][1].startswith(f"decoder_block_{chain}/")
        _assert_same(names, got, want, (chain, tile_rows))


def test_the_wrappers_refuse_what_the_kernel_does_not_take(weights):
    w = weights[1024]
    attn_out, tgt, pos = _inputs(1, 5)
    with pytest.raises(RuntimeError):
        _block_a(w, attn_out.float(), tgt.float(), pos.float())
    with pytest.raises(RuntimeError):
        _block_a(w, attn_out, tgt, pos, tile_rows=16)
    with pytest.raises(RuntimeError):
        _block_b(dict(w, wqk=w["wq"]), attn_out, tgt, pos)   # a 384-row query weight where the 512-row one belongs
    with pytest.raises(RuntimeError):
        _block_a(w, attn_out, tgt.requires_grad_(), pos)
    tgt.requires_grad_(False)


# ---- the decoder's loop ------------------------------------------------------------------------------------------------------------
SHAPES = ((12, 17), (6, 9), (3, 5), (2, 3))


def _transformer(return_intermediate, layers=3):
    from alonet.deformable_detr.deformable_transformer import DeformableTransformer

    torch.manual_seed(4)
    tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=layers,
                               return_intermediate_dec=return_intermediate)
    with torch.no_grad():   # the stock initialisation zeroes the offset / attention weights: give every parameter a say
        for layer in tr.decoder.layers:
            a = layer.cross_attn
            a.sampling_offsets.weight.normal_(0, 0.02)
            a.attention_weights.weight.normal_(0, 0.05)
            for lin in (a.value_proj, a.output_proj, layer.linear1, layer.linear2, layer.self_attn.out_proj):
                lin.bias.normal_(0, 0.2)
            layer.self_attn.in_proj_bias.normal_(0, 0.2)
            for norm in (layer.norm1, layer.norm2, layer.norm3):
                norm.weight.normal_(1, 0.2)
                norm.bias.normal_(0, 0.2)
    return tr.to(DEV, BF).eval()


def _pyramid(batch):
    gen = torch.Generator().manual_seed(9)
    srcs = [torch.randn(batch, 256, h, w, generator=gen).to(DEV, BF) for h, w in SHAPES]
    poss = [torch.randn(batch, 256, h, w, generator=gen).to(DEV, BF) for h, w in SHAPES]
    masks = []
    for h, w in SHAPES:   # the last image of a batch of two is padded on its right quarter and bottom third: frames of different size
        m = torch.zeros(batch, h, w, dtype=torch.bool)
        if batch > 1:
            m[-1, :, w - max(1, w // 4):] = True
            m[-1, h - max(1, h // 3):, :] = True
        masks.append(m.to(DEV))
    query_embed = torch.randn(300, 512, generator=gen).to(DEV, BF)
    return srcs, masks, poss, query_embed


def _run(tr, inputs, monkeypatch, mode):
    monkeypatch.setenv("ALO_DEC_BLOCK", mode)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = tr(*inputs)
    return out["hs"], {tag: v["calls"] for tag, v in timer.summary().items()}


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("return_intermediate", [False, True])
def test_decoder_loop_equals_the_separate_launches(monkeypatch, batch, return_intermediate):
    tr, inputs = _transformer(return_intermediate), _pyramid(batch)
    rows = batch * 300
    want, tags_off = _run(tr, inputs, monkeypatch, "off")
    assert not any(tag.startswith("decoder_block") for tag in tags_off)
    got, tags = _run(tr, inputs, monkeypatch, "on")
    assert got.shape == want.shape == ((3, batch, 300, 256) if return_intermediate else (batch, 300, 256))
    assert torch.equal(_bits(got), _bits(want))
    tile = alo_hip.decoder_block_tile_rows(rows, DEV)
    assert {tag: n for tag, n in tags.items() if tag.startswith("decoder_block")} == {
        f"decoder_block_a/rows={rows}/tile={tile}": 3, f"decoder_block_b/rows={rows}/tile={tile}": 2}
    # the last layer keeps its separate launches after the MSDA kernel; layer 0's two input projections are separate as well
    assert tags[f"add_layernorm/rows={rows}"] == 2 and tags["ffn256/F=1024"] == 1
    assert tags_off[f"add_layernorm/rows={rows}"] == 9 and tags_off["ffn256/F=1024"] == 3
    assert tags["linear_shortk/N=512,K=256"] == 1 and tags_off["linear_shortk/N=512,K=256"] == 3
    msda = lambda t: sum(n for tag, n in t.items() if tag.startswith("msda_fwd"))
    assert msda(tags) == msda(tags_off) == 4


def test_what_the_route_does_not_cover_keeps_the_separate_launches(monkeypatch):
    from alonet.deformable_detr.deformable_transformer import DeformableTransformer

    srcs, masks, poss, query_embed = _pyramid(2)
    few = (srcs, masks, poss, query_embed[:100])                     # 200 rows: below the measured range
    _, tags = _run(_transformer(False), few, monkeypatch, "on")
    assert tags and not any(tag.startswith("decoder_block") for tag in tags)
    tr = _transformer(False).train()                                 # training
    _, tags = _run(tr, (srcs, masks, poss, query_embed), monkeypatch, "on")
    assert not any(tag.startswith("decoder_block") for tag in tags)
    for dtype in (torch.float16, torch.float32):                     # the kernels are bf16
        tr = _transformer(False).to(dtype)
        cast = lambda xs: [x.to(dtype) for x in xs]
        _, tags = _run(tr, (cast(srcs), masks, cast(poss), query_embed.to(dtype)), monkeypatch, "on")
        assert tags and not any(tag.startswith("decoder_block") for tag in tags), dtype
    assert DeformableTransformer(two_stage=True, num_encoder_layers=1, num_decoder_layers=1).decoder.two_stage   # gated off in decoder_forward


def test_one_decoder_layer_on_the_route_replays_in_a_graph():
    from alonet.deformable_detr.deformable_transformer import _in_proj_rows, _level_geometry

    tr = _transformer(False, layers=2)
    layer, nxt = tr.decoder.layers
    gen = torch.Generator().manual_seed(12)
    r = lambda *shape: torch.randn(*shape, generator=gen).to(DEV, BF)
    S = sum(h * w for h, w in SHAPES)
    tgt, pos, src = r(2, 300, 256), r(2, 300, 256), r(2, S, 256)
    ref = torch.rand(2, 300, 4, 2, generator=gen).to(DEV)
    spatial_shapes, level_start_index = _level_geometry(SHAPES, torch.device(DEV))
    (w_qk, b_qk), (w_v, b_v) = _in_proj_rows(layer.self_attn)

    def step():
        qk, v = alo_hip.linear_auto(tgt + pos, w_qk, b_qk), alo_hip.linear_auto(tgt, w_v, b_v)
        return layer.forward_block(tgt, qk, v, pos, ref, src, spatial_shapes, level_start_index, None, next_layer=nxt)

    with torch.no_grad():
        eager = [t.clone() for t in step()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()   # warm up on the capture stream: packed weights and every lazily built table exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        for _ in range(2):
            for t in captured:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            _assert_same(("out", "qk", "v"), captured, eager, "replay")


def test_deformable_detr_r50_equals_the_separate_launches_eager_and_graphed(monkeypatch):
    """DeformableDETR-R50 in bf16 on two frames of different size: ``pred_logits`` / ``pred_boxes`` byte-equal with the route on and
    off, the decoder's chains among the launches next to the last layer's separate ones, and GraphedForward replays the route."""
    import aloscene
    from alonet.common import GraphedForward
    from alonet.deformable_detr import DeformableDetrR50

    torch.manual_seed(0)
    model = DeformableDetrR50(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval().to(BF)
    gen = torch.Generator().manual_seed(5)
    fr = [aloscene.Frame(torch.rand(3, 256 - 32 * i, 320, generator=gen) * 255, normalization="255").norm_resnet() for i in range(2)]
    frames = aloscene.Frame.batch_list(fr).to(DEV).to(BF)
    keys = ("pred_logits", "pred_boxes")
    with torch.no_grad():
        monkeypatch.setenv("ALO_DEC_BLOCK", "off")
        with alo_hip.LaunchTimer() as timer_off:
            out = model(frames)
        want = {k: out[k].clone() for k in keys}
        monkeypatch.setenv("ALO_DEC_BLOCK", "on")
        with alo_hip.LaunchTimer() as timer:
            eager = model(frames)
        tags, tags_off = ({tag: v["calls"] for tag, v in t.summary().items()} for t in (timer, timer_off))
        assert not any(tag.startswith("decoder_block") for tag in tags_off)
        assert sum(n for tag, n in tags.items() if tag.startswith("decoder_block_a")) == 6
        assert sum(n for tag, n in tags.items() if tag.startswith("decoder_block_b")) == 5
        assert sum(n for tag, n in tags.items() if tag.startswith("encoder_block")) == 6
        assert tags["add_layernorm/rows=600"] == 2 and tags["ffn256/F=1024"] == 1
        for key in keys:
            assert torch.isfinite(eager[key].float()).all() and torch.equal(_bits(eager[key]), _bits(want[key])), key
        graphed = GraphedForward(model)
        for _ in range(2):
            got = graphed(frames)
            for key in keys:
                assert torch.equal(_bits(got[key]), _bits(want[key])), key
