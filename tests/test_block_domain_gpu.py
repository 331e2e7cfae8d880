"""The fused transformer blocks (csrc/encoder_block.hip: alo_hip.encoder_block, decoder_block_a, decoder_block_b) across what their
gates admit: every comparison is bit for bit against the chain of launches a block stands in for (``_chain`` of
test_encoder_block_gpu.py, ``_chain_a`` / ``_chain_b`` of test_decoder_block_gpu.py), whose links are held to fp32 / fp64 references in
their own tests.  Four parts: hidden widths other than 256 and 1024 (the loop over hidden chunks, the weight hand-over, W2's stride,
and the widths whose 64-row LDS frame does not fit), the decoder chains at their tile edges, data that stresses the in-kernel
LayerNorm, the ReLU and the accumulators, and the decoder's route under the model variants it meets."""
import pytest
import torch

import alo_hip
import test_decoder_block_gpu as dec
import test_encoder_block_gpu as enc
from guarded import GuardedLaunches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
EPS = dec.EPS   # (1e-5, 1e-3): the two LayerNorms of a chain take one each
ENC_FORM = "tail+ffn+proj"


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(names, got, want, what):
    """Every output present on both sides, of one shape and dtype, and equal byte for byte."""
    assert len(got) == len(want) == len(names), what
    for name, g, x in zip(names, got, want):
        assert (g is None) == (x is None), (what, name)
        if g is not None:
            assert g.shape == x.shape and g.dtype == x.dtype, (what, name)
            assert torch.equal(_bytes(g), _bytes(x)), (what, name, int((_bytes(g) != _bytes(x)).sum()))


def _weights(Fh, seed=31, **over):
    """One layer's parameters under the names both files' helpers read: the encoder's block takes wo / bo / g1 / e1 / FFN / g2 / e2 /
    wv / bv / wq / bq, chain A wo / bo / g2 / e2 / wq / bq and chain B wc / bc / g1 / e1 / FFN / g3 / e3 / wv / bv / wqk / bqk.
    Built on the CPU from a seeded generator, scaled as the two files' fixtures scale theirs; ``over``: name -> constant."""
    gen = torch.Generator().manual_seed(seed + Fh)
    r = lambda *shape, scale=1.0: torch.randn(*shape, generator=gen) * scale
    w = dict(wo=r(256, 256, scale=1 / 16), bo=r(256, scale=0.5), wc=r(256, 256, scale=1 / 16), bc=r(256, scale=0.5),
             g1=1 + r(256, scale=0.3), e1=r(256, scale=0.3), g2=1 + r(256, scale=0.3), e2=r(256, scale=0.3),
             g3=1 + r(256, scale=0.3), e3=r(256, scale=0.3),
             w1=r(Fh, 256, scale=1 / 16), b1=r(Fh, scale=0.5), w2=r(256, Fh, scale=Fh ** -0.5), b2=r(256, scale=0.5),
             wv=r(256, 256, scale=1 / 16), bv=r(256, scale=0.5), wq=r(384, 256, scale=1 / 16), bq=r(384, scale=0.5),
             wqk=r(512, 256, scale=1 / 16), bqk=r(512, scale=0.5))
    for name, value in over.items():
        w[name] = torch.full_like(w[name], value)
    return {k: v.to(DEV, BF) for k, v in w.items()}


@pytest.fixture(scope="module")
def weights():
    """name -> parameters, built on first use and never modified."""
    made = {}

    def get(Fh=1024, **over):
        key = (Fh, tuple(sorted(over.items())))
        if key not in made:
            made[key] = _weights(Fh, **over)
        return made[key]

    return get


# ---- 1. hidden widths ---------------------------------------------------------------------------------------------------------------
# 512, 768, 2048: two, three and eight passes of the loop over hidden chunks; 4864: the widest whose 64-row decoder frame fits, 19
# passes; 5120: the first that fits at 32 rows only
WIDTHS = (512, 768, 2048, 4864, 5120)
WIDTH_ROWS = ((1, 37), (2, 65))


@pytest.mark.parametrize("batch,S", WIDTH_ROWS)
@pytest.mark.parametrize("Fh", WIDTHS)
@pytest.mark.parametrize("form", ["ffn", ENC_FORM])
def test_encoder_block_equals_the_chain_at_other_hidden_widths(weights, form, Fh, batch, S):
    src, attn_out, pos, _ = enc._inputs(batch, S, seed=Fh + S, mask=False)
    mask = torch.zeros(batch, S, dtype=torch.bool)
    mask[:, 1::3] = True
    mask[-1] |= batch > 1   # a fully masked batch item
    args = (src, attn_out, pos, mask.to(DEV))
    _same(("src", "value", "offsets_logits"), enc._block(form, weights(Fh), *args), enc._chain(form, weights(Fh), *args), (form, Fh))


@pytest.mark.parametrize("batch,L", WIDTH_ROWS)
@pytest.mark.parametrize("Fh", WIDTHS)
def test_decoder_block_b_equals_the_chain_at_other_hidden_widths(weights, Fh, batch, L):
    w, args = weights(Fh), dec._inputs(batch, L, seed=Fh)
    want = dec._chain_b(w, *args)
    for tile_rows in (32, 64, None):
        if tile_rows == 64 and Fh > 4864:   # the 64-row frame does not fit: refused by name, before anything is enqueued
            with pytest.raises(RuntimeError, match=f"hidden width {Fh} needs .* bytes of LDS"):
                dec._block_b(w, *args, tile_rows=64)
            continue
        with alo_hip.LaunchTimer() as timer:
            got = dec._block_b(w, *args, tile_rows=tile_rows)
        assert list(timer.summary()) == [f"decoder_block_b/rows={batch * L}/tile={tile_rows or 32}"]
        _same(("out", "v", "qk"), got, want, (Fh, tile_rows))


@pytest.mark.parametrize("Fh", [4864, 5120])
def test_decoder_block_b_picks_a_height_whose_frame_fits_when_the_rows_fill_the_chip(weights, Fh):
    """From ceil(rows / 64) = compute units on the rule takes 64-row tiles: at 4864 hidden units they fit, at 5120 they do not and
    the 32-row ones run.  The count follows from the device; it is no workload's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 64 * cus + 37
    w, args = weights(Fh), dec._inputs(1, rows, seed=Fh)
    tile = 64 if Fh <= 4864 else 32
    with alo_hip.LaunchTimer() as timer:
        got = dec._block_b(w, *args)
    assert list(timer.summary()) == [f"decoder_block_b/rows={rows}/tile={tile}"]
    _same(("out", "v", "qk"), got, dec._chain_b(w, *args), Fh)
    # and the prediction callers and the launch tag rely on: without a width the rule by rows alone, with it the height that ran
    assert alo_hip.decoder_block_tile_rows(rows, DEV) == 64 and alo_hip.decoder_block_tile_rows(rows, DEV, Fh) == tile


def test_the_entry_point_picks_the_height_itself_when_no_flag_fixes_it(weights):
    """A caller of the C entry point that sets neither ALO_BLOCK_TILE_32 nor _64 (the wrappers always set one): at 5120 hidden units
    and enough rows for 64-row tiles the call runs, at 32 rows, and gives the chain's bits."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Fh, rows = 5120, 64 * cus + 37
    w = weights(Fh)
    attn_out, tgt1, pos = dec._inputs(1, rows, seed=Fh)
    want = dec._chain_b(w, attn_out, tgt1, pos)
    out, value, qk = torch.empty_like(tgt1), torch.empty_like(tgt1), torch.empty(1, rows, 512, dtype=BF, device=DEV)
    packed = lambda name: alo_hip.pack_mfma_b(w[name])
    alo_hip._launch("alo_encoder_block", tgt1.device, None, 0.0, 0.0, attn_out, packed("wc"), w["bc"], w["g1"], w["e1"], tgt1, packed("w1"),
                    w["b1"], packed("w2"), w["b2"], w["g3"], w["e3"], out, pos, None, packed("wv"), w["bv"], packed("wqk"), w["bqk"], value, qk,
                    1, rows, Fh, EPS[0], EPS[1], alo_hip.ALO_BF16 | alo_hip.ALO_BLOCK_DECODER_NEXT)
    _same(("out", "v", "qk"), (out, value, qk), want, "no height flag")


def test_the_widest_hidden_layer_the_gates_admit_runs(weights):
    """21760 hidden units: chain B's 32-row frame is exactly the LDS limit and the encoder block's 512 bytes below it; 85 passes of
    the loop over hidden chunks.  What the gates say yes to runs, and gives the chain's bits."""
    Fh = 21760
    assert alo_hip.decoder_block_lds_bytes(Fh, 32) == alo_hip.BLOCK_LDS_LIMIT == alo_hip.encoder_block_lds_bytes(Fh) + 512
    w, args = weights(Fh), dec._inputs(1, 37, seed=Fh)
    with alo_hip.LaunchTimer() as timer:
        got = dec._block_b(w, *args)
    assert list(timer.summary()) == ["decoder_block_b/rows=37/tile=32"]
    _same(("out", "v", "qk"), got, dec._chain_b(w, *args), Fh)
    with pytest.raises(RuntimeError, match=f"hidden width {Fh} needs .* bytes of LDS"):
        dec._block_b(w, *args, tile_rows=64)
    args = enc._inputs(2, 65, seed=Fh, mask=True)
    _same(("src", "value", "offsets_logits"), enc._block(ENC_FORM, w, *args), enc._chain(ENC_FORM, w, *args), Fh)


def test_the_gates_keep_a_width_whose_frame_fits_nowhere_on_the_separate_launches(monkeypatch):
    """21760 is the widest hidden layer the decoder chains take and 21888 the encoder block's bound; at the next multiple of 256
    both gates say no, the layers say no, and a forward with both routes on runs the separate launches and equals the routes off."""
    from alonet.deformable_detr.deformable_transformer import DeformableTransformer

    torch.manual_seed(4)
    tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=22016).to(DEV, BF).eval()
    inputs = dec._pyramid(1)
    monkeypatch.setenv("ALO_ENC_BLOCK", "off")
    want, tags_off = dec._run(tr, inputs, monkeypatch, "off")
    monkeypatch.setenv("ALO_ENC_BLOCK", "on")
    got, tags = dec._run(tr, inputs, monkeypatch, "on")
    assert tags == tags_off and tags["ffn256/F=22016"] == 4 and not any(tag.startswith(("decoder_block", "encoder_block")) for tag in tags)
    assert torch.isfinite(want.float()).all() and torch.equal(_bytes(got), _bytes(want))
    x, vec = torch.zeros(2, 300, 256, dtype=BF, device=DEV), torch.zeros(256, dtype=BF, device=DEV)
    for Fh, fits in ((21760, True), (22016, False)):
        w1, w2 = torch.zeros(Fh, 256, dtype=BF, device=DEV), torch.zeros(256, Fh, dtype=BF, device=DEV)
        assert alo_hip.ffn256_supported(x, w1, w2)
        assert alo_hip.decoder_block_supported(x, vec, w1, w2, hidden=Fh) is fits
        assert alo_hip.encoder_block_supported(x, w1, w2, vec) is fits
    assert alo_hip.decoder_block_supported(x, vec)   # chain A: no hidden layer to ask about


# ---- 2. tile edges of the decoder chains --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 31, 32, 33, 63, 64, 65, 96])
@pytest.mark.parametrize("chain", ["a", "b"])
def test_decoder_chains_at_their_tile_edges(weights, chain, L):
    reference, block, names = dec.CHAINS[chain]
    for Fh in ((1024, 256) if chain == "b" else (1024,)):
        args = dec._inputs(1, L, seed=5)
        want = reference(weights(Fh), *args)
        for tile_rows in (32, 64):
            _same(names, block(weights(Fh), *args, tile_rows=tile_rows), want, (chain, Fh, L, tile_rows))


# a: a tile that ends one row short of full; b: one row into the second (32) / third (64 + 1) tile; 2 x 300: 19 and 10 tiles, a ragged last one
@pytest.mark.parametrize("chain,batch,L", [("a", 1, 63), ("b", 1, 65), ("a", 2, 300), ("b", 2, 300)])
def test_decoder_chains_stay_in_their_buffers_at_tile_edges_and_over_many_tiles(weights, chain, batch, L):
    reference, block, names = dec.CHAINS[chain]
    args = dec._inputs(batch, L, seed=6)
    want = reference(weights(), *args)
    for tile_rows in (32, 64):
        with GuardedLaunches() as g:
            got = block(weights(), *args, tile_rows=tile_rows)
        assert g.seen == [("alo_encoder_block", f"decoder_block_{chain}/rows={batch * L}/tile={tile_rows}")]
        _same(names, got, want, (chain, L, tile_rows))


# ---- 3. hostile data ----------------------------------------------------------------------------------------------------------------
# A target: (first projection's weight and bias, the outputs' names, chain(w, residual, attn_out, pos), block(w, ..., tile_rows),
# heights).  Every output is handed back with its rows along dim 1 (the encoder's value is head-major: (N, 8, S, 32)).
def _enc_rows(outs):
    src, value, both = outs
    return src, value.permute(0, 2, 1, 3).reshape(src.shape), both


TARGETS = {
    "enc": ("wo", "bo", ("src", "value", "offsets_logits"),
            lambda w, res, attn, pos: _enc_rows(enc._chain(ENC_FORM, w, res, attn, pos, None, *EPS)),
            lambda w, res, attn, pos, tile_rows: _enc_rows(enc._block(ENC_FORM, w, res, attn, pos, None, *EPS)), (None,)),
    "a": ("wo", "bo", dec.CHAINS["a"][2], lambda w, res, attn, pos: dec._chain_a(w, attn, res, pos),
          lambda w, res, attn, pos, tile_rows: dec._block_a(w, attn, res, pos, tile_rows=tile_rows), (32, 64)),
    "b": ("wc", "bc", dec.CHAINS["b"][2], lambda w, res, attn, pos: dec._chain_b(w, attn, res, pos),
          lambda w, res, attn, pos, tile_rows: dec._block_b(w, attn, res, pos, tile_rows=tile_rows), (32, 64)),
}
HOSTILE_ROWS = (3, 37)                       # ragged at both tile heights, batch boundaries inside a tile
PLANTED = ((0, 0), (1, 7), (2, 36))          # the first row, one inside, the last row (in a partial tile)
NO_BIAS = dict(bo=0.0, bc=0.0, b1=0.0, b2=0.0, e1=0.0, e2=0.0, e3=0.0)


def _activations(seed, residual=(0.0, 1.0), attn=1.0, pos=1.0, scale=1.0):
    """(residual, attn_out, pos) of HOSTILE_ROWS: ``residual = mean + spread * randn``, the others ``factor * randn``, all three
    times ``scale``; built in fp32 on the CPU, then rounded to bf16."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(*HOSTILE_ROWS, 256, generator=gen)
    res, a, p = residual[0] + residual[1] * r(), attn * r(), pos * r()
    return [(t * scale).to(BF).to(DEV) for t in (res, a, p)]


def _run_hostile(target, w, acts, planted=()):
    """Chain against block at every height of ``target``.  Without ``planted``: the chain's outputs are finite, ``out`` is not the
    same row everywhere (an all-NaN or a constant result proves nothing) and every byte is equal.  With ``planted`` rows: the rows
    the chain leaves non-finite are exactly those, inside them only the places of NaN and of Inf are compared (which operand's NaN
    payload an addition keeps is not part of the contract), every other row byte for byte.  -> the chain's outputs"""
    _, _, names, chain, block, heights = TARGETS[target]
    want = chain(w, *acts)
    finite_rows = torch.stack([torch.isfinite(x.float()).all(-1) for x in want]).all(0)   # (N, L)
    keep = torch.ones(HOSTILE_ROWS, dtype=torch.bool, device=DEV)
    for n, l in planted:
        keep[n, l] = False
    assert int((~keep).sum()) == len(planted) and torch.equal(finite_rows, keep), (target, (~finite_rows).nonzero().tolist())
    out = _bytes(want[0][keep])
    assert bool((out != out[:1]).any()), "every row of out is the same"
    for tile_rows in heights:
        got = block(w, *acts, tile_rows)
        for name, g, x in zip(names, got, want):
            assert g.shape == x.shape and torch.equal(_bytes(g[keep]), _bytes(x[keep])), (target, tile_rows, name)
            if planted:
                assert torch.equal(torch.isnan(g.float()), torch.isnan(x.float())), (target, tile_rows, name)
                assert torch.equal(torch.isposinf(g.float()), torch.isposinf(x.float())), (target, tile_rows, name)
                assert torch.equal(torch.isneginf(g.float()), torch.isneginf(x.float())), (target, tile_rows, name)
    return want


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_rows_whose_mean_dwarfs_their_spread(weights, target):
    """residual = 48 + 0.5 randn, attn_out = 0.05 randn: at bf16's 8 bits the residual has a step of 0.25, and the variance is what
    is left of 256 differences from a mean near 48."""
    _run_hostile(target, weights(), _activations(41, residual=(48.0, 0.5), attn=0.05))


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_zero_variance_rows(weights, target):
    """Three rows with attn_out = 0 and a constant residual c under a first projection without bias: LayerNorm1 sees c in every
    column, a variance of exactly zero, and gives its beta whatever c and eps are.  Chain A hands that row out: ``tgt1`` is beta,
    bit for bit.  The encoder block and chain B feed it to the FFN, so there the three rows of ``out`` equal each other."""
    w = weights(bo=0.0, bc=0.0)
    res, attn, pos = _activations(42)
    for (n, l), c in zip(PLANTED, (0.0, 1.5, -3.0)):
        attn[n, l] = 0.0
        res[n, l] = c
    want = _run_hostile(target, w, (res, attn, pos))
    rows = [want[0][n, l] for n, l in PLANTED]
    if target == "a":
        for row in rows:
            assert torch.equal(_bytes(row), _bytes(w["e2"]))
    else:
        assert torch.equal(_bytes(rows[0]), _bytes(rows[1])) and torch.equal(_bytes(rows[0]), _bytes(rows[2]))
    for tile_rows in TARGETS[target][5]:   # and the block's own rows, not only through the comparison with the chain
        got = TARGETS[target][4](w, res, attn, pos, tile_rows)[0]
        for (n, l), row in zip(PLANTED, rows):
            assert torch.equal(_bytes(got[n, l]), _bytes(row)), (target, tile_rows, n, l)


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_rows_whose_variance_eps_dominates(weights, target):
    """All three activations times 2^-60 (exact in bf16): a row's variance is near 2^-120 and 1 / sqrt(var + eps) is 1 / sqrt(eps),
    316 for 1e-5 and 31.6 for 1e-3, so which eps a LayerNorm takes shows in its output.  The weight set has no bias in the two
    projections and the FFN and no beta: with any of them every row would come out as that constant and the 2^-60 signal,
    which is what tells the rows apart, would be rounded away."""
    _run_hostile(target, weights(**NO_BIAS), _activations(43, scale=2.0 ** -60))


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_large_activations_stay_finite(weights, target):
    """All three activations times 2^40: row sums of squares near 2^88 in the LayerNorms, projections of a query near 2^40."""
    _run_hostile(target, weights(), _activations(44, scale=2.0 ** 40))


@pytest.mark.parametrize("target", ["b", "enc"])
def test_a_dead_relu_leaves_the_second_bias(weights, target):
    """b1 = -100: no hidden unit fires, the FFN's output is b2 in every row (checked on the chain's own links), and the bits of what
    follows include the sign of the zeros the second product sums."""
    w = weights(b1=-100.0)
    res, attn, pos = acts = _activations(45)
    first_w, first_b = TARGETS[target][:2]
    x = alo_hip.add_layernorm(alo_hip.linear_auto(attn, w[first_w], w[first_b]), res, w["g1"], w["e1"], EPS[0])
    assert not alo_hip.linear_auto(x, w["w1"], w["b1"], relu=True).any()
    assert torch.equal(_bytes(alo_hip.ffn256(x, w["w1"], w["b1"], w["w2"], w["b2"])), _bytes(w["b2"].expand(*HOSTILE_ROWS, -1)))
    _run_hostile(target, w, acts)


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_an_accumulator_overflow_stays_in_its_row(weights, target):
    """Three planted rows of attn_out times 2^126.  Before the scaling a planted row is +-sign(W[j]) of one output column j of the
    first projection, so that column's accumulator sums 256 terms of one sign, 2^126 * sum |W[j, k]| (about 12.8 * 2^126 against
    fp32's 2^128), and overflows for certain; the LayerNorm behind it spreads the row with NaN."""
    w = weights()
    res, attn, pos = _activations(46)
    first_w = w[TARGETS[target][0]].float()
    for (n, l), j, sign in zip(PLANTED, (0, 100, 255), (1.0, -1.0, 1.0)):
        assert float(first_w[j].abs().sum()) > 8.0
        attn[n, l] = (sign * torch.sign(first_w[j]) * 2.0 ** 126).to(BF)
    assert torch.isfinite(attn.float()).all()   # the inputs are finite: the overflow is the accumulator's
    _run_hostile(target, w, (res, attn, pos), planted=PLANTED)


# ---- 4. the decoder's route under the variants it meets -----------------------------------------------------------------------------
def _transformer(return_intermediate=False, layers=3, **kwargs):
    """test_decoder_block_gpu.py's ``_transformer`` with constructor arguments: every parameter of the decoder layers has a say."""
    from alonet.deformable_detr.deformable_transformer import DeformableTransformer

    torch.manual_seed(4)
    tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=layers,
                               return_intermediate_dec=return_intermediate, **kwargs)
    with torch.no_grad():
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
    return tr


def _box_heads(n):
    """``n`` box heads whose last layers are not zero (DeformableDETR's constructor zeroes them: the refined reference points would
    then not depend on the decoder's output)."""
    from alonet.transformers import MLP

    heads = torch.nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(n)])
    assert all(bool(h.layers[-1].weight.detach().any()) and bool(h.layers[-1].bias.detach().any()) for h in heads)
    return heads


def _forward(call, monkeypatch, mode):
    monkeypatch.setenv("ALO_DEC_BLOCK", mode)
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = call()
    return out, {tag: v["calls"] for tag, v in timer.summary().items()}


def _block_tags(tags):
    return {tag: n for tag, n in tags.items() if tag.startswith("decoder_block")}


def _assert_outputs_equal(got, want, keys):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.isfinite(want[key].float()).all() and torch.equal(_bytes(got[key]), _bytes(want[key])), key


@pytest.mark.parametrize("batch", [1, 2])
def test_box_refinement_on_the_route_equals_the_separate_launches(monkeypatch, batch):
    """``decoder.bbox_embed`` set: the reference points turn 4-d after layer 0 and ``ref_input`` is rebuilt for every layer from the
    layer's output, all between the fused launches."""
    tr = _transformer(True)
    tr.decoder.bbox_embed = _box_heads(3)
    tr = tr.to(DEV, BF).eval()
    inputs, rows = dec._pyramid(batch), batch * 300
    want, tags_off = _forward(lambda: tr(*inputs), monkeypatch, "off")
    got, tags = _forward(lambda: tr(*inputs), monkeypatch, "on")
    assert not _block_tags(tags_off)
    assert _block_tags(tags) == {f"decoder_block_a/rows={rows}/tile=32": 3, f"decoder_block_b/rows={rows}/tile=32": 2}
    assert want["hs"].shape == (3, batch, 300, 256) and want["inter_references_out"].shape == (3, batch, 300, 4)
    assert want["init_reference_out"].shape == (batch, 300, 2)
    refs = want["inter_references_out"].float()
    assert not torch.equal(refs[0], refs[1]) and not torch.equal(refs[1], refs[2])   # every layer moved them
    _assert_outputs_equal(got, want, ("hs", "inter_references_out", "init_reference_out"))


def test_the_refinement_model_equals_the_separate_launches_eager_and_graphed(monkeypatch):
    """DeformableDetrR50Refinement whole, in bf16 on two frames of different size, with auxiliary outputs: the last level and every
    auxiliary one byte-equal with the route on and off, and one replay through GraphedForward."""
    import aloscene
    from alonet.common import GraphedForward
    from alonet.deformable_detr import DeformableDetrR50Refinement

    torch.manual_seed(0)
    model = DeformableDetrR50Refinement(num_classes=91, aux_loss=True, device=torch.device(DEV)).eval()
    assert model.transformer.decoder.bbox_embed is model.bbox_embed and len(model.bbox_embed) == 6
    with torch.no_grad():
        for head in model.bbox_embed:   # zeroed by the constructor, which would hide the path from the output to the next reference
            head.layers[-1].weight.normal_(0, 0.05)
    model = model.to(BF)
    gen = torch.Generator().manual_seed(5)
    fr = [aloscene.Frame(torch.rand(3, 256 - 32 * i, 320, generator=gen) * 255, normalization="255").norm_resnet() for i in range(2)]
    frames = aloscene.Frame.batch_list(fr).to(DEV).to(BF)

    def flat(out):
        levels = [out] + list(out["aux_outputs"])
        assert len(levels) == 6
        return {f"{key}/{i}": lvl[key] for i, lvl in enumerate(levels) for key in ("pred_logits", "pred_boxes")}

    want, tags_off = _forward(lambda: {k: v.clone() for k, v in flat(model(frames)).items()}, monkeypatch, "off")
    got, tags = _forward(lambda: flat(model(frames)), monkeypatch, "on")
    assert not _block_tags(tags_off)
    assert _block_tags(tags) == {"decoder_block_a/rows=600/tile=32": 6, "decoder_block_b/rows=600/tile=32": 5}
    assert not torch.equal(want["pred_boxes/0"], want["pred_boxes/5"])
    _assert_outputs_equal(got, want, sorted(want))
    with torch.no_grad():
        _assert_outputs_equal(flat(GraphedForward(model)(frames)), want, sorted(want))


@pytest.mark.parametrize("Fh", [512, 2048])
def test_decoder_loop_equals_the_separate_launches_at_other_hidden_widths(monkeypatch, Fh):
    tr, inputs = _transformer(True, dim_feedforward=Fh).to(DEV, BF).eval(), dec._pyramid(2)
    want, tags_off = _forward(lambda: tr(*inputs), monkeypatch, "off")
    got, tags = _forward(lambda: tr(*inputs), monkeypatch, "on")
    assert not _block_tags(tags_off)
    assert _block_tags(tags) == {"decoder_block_a/rows=600/tile=32": 3, "decoder_block_b/rows=600/tile=32": 2}
    assert tags[f"ffn256/F={Fh}"] == 1 and tags_off[f"ffn256/F={Fh}"] == 3
    _assert_outputs_equal(got, want, ("hs", "inter_references_out"))


def test_a_two_stage_forward_keeps_the_separate_launches(monkeypatch):
    """Two-stage queries (2 x 150 proposals: enough rows for the route) run the same launches with the route on and off."""
    tr = _transformer(True, layers=2, two_stage=True, two_stage_num_proposals=150)
    tr.decoder.class_embed = torch.nn.ModuleList([torch.nn.Linear(256, 5) for _ in range(3)])
    tr.decoder.bbox_embed = _box_heads(3)
    tr = tr.to(DEV, BF).eval()
    assert tr.decoder.two_stage
    srcs, masks, poss, _ = dec._pyramid(2)
    want, tags_off = _forward(lambda: tr(srcs, masks, poss, None), monkeypatch, "off")
    got, tags = _forward(lambda: tr(srcs, masks, poss, None), monkeypatch, "on")
    assert want["hs"].shape == (2, 2, 150, 256) and alo_hip.decoder_block_routed(want["hs"][0])
    assert tags == tags_off and not _block_tags(tags) and any(tag.startswith("proposal_queries") for tag in tags)
    _assert_outputs_equal(got, want, ("hs", "inter_references_out", "init_reference_out", "enc_outputs_class"))
    coords, coords_off = got["enc_outputs_coord_unact"], want["enc_outputs_coord_unact"]   # +inf on dropped tokens
    assert not torch.isnan(coords_off).any() and torch.equal(_bytes(coords), _bytes(coords_off))


def test_a_padding_mask_or_an_expanded_query_pos_keeps_the_separate_launches(monkeypatch):
    """The decoder called directly: dense operands take the route; a ``tgt_key_padding_mask`` or a stride-0 ``query_pos`` of the
    same values does not, and gives the bits of the route switched off."""
    from alonet.deformable_detr.deformable_transformer import _level_geometry

    decoder = _transformer(False).to(DEV, BF).eval().decoder
    gen = torch.Generator().manual_seed(13)
    S = sum(h * w for h, w in dec.SHAPES)
    tgt, src = (torch.randn(2, n, 256, generator=gen).to(DEV, BF) for n in (300, S))
    one_pos = torch.randn(300, 256, generator=gen).to(DEV, BF)
    reference_points = torch.rand(2, 300, 2, generator=gen).to(DEV, BF)
    ratios = torch.tensor([[[1.0, 1.0]] * 4, [[0.75, 0.67]] * 4], dtype=torch.float32, device=DEV)
    spatial_shapes, level_start_index = _level_geometry(dec.SHAPES, torch.device(DEV))
    padding = torch.zeros(2, 300, dtype=torch.bool, device=DEV)
    padding[1, 250:] = True
    expanded = one_pos.unsqueeze(0).expand(2, -1, -1)
    assert expanded.stride(0) == 0 and expanded.shape == tgt.shape

    def call(query_pos, tgt_key_padding_mask=None):
        return lambda: decoder(tgt, reference_points, src, spatial_shapes, level_start_index, ratios, query_pos=query_pos,
                               tgt_key_padding_mask=tgt_key_padding_mask)

    dense, tags = _forward(call(expanded.contiguous()), monkeypatch, "on")
    assert _block_tags(tags) == {"decoder_block_a/rows=600/tile=32": 3, "decoder_block_b/rows=600/tile=32": 2}
    for name, run in (("padding mask", call(expanded.contiguous(), padding)), ("expanded query_pos", call(expanded))):
        want, tags_off = _forward(run, monkeypatch, "off")
        got, tags = _forward(run, monkeypatch, "on")
        assert tags and tags == tags_off and not _block_tags(tags), name
        _assert_outputs_equal(got, want, ("hs", "inter_references_out"))
    _assert_outputs_equal(got, dense, ("hs",))   # the same values, expanded or dense: the same bits on either route
