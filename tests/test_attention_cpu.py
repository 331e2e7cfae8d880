"""Dense attention on alo_encoder_block (ALO_BLOCK_ATTENTION / ALO_BLOCK_PACKED_QK above the low byte of ``dtype``,
include/alo_encoder_block.h) without a GPU: the fp64 yardstick against ``nn.MultiheadAttention``, the flags, every refusal (each call
carries one bad argument, so nothing is ever launched), the routes' gate on CPU tensors, and G22 on the stock ops."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import alo_hip
from attention_ref import HEAD_DIM, HEADS, SCALE, attention_ref
from helpers import formula_state_dict

ATT, PACKED = getattr(alo_hip, "ALO_BLOCK_ATTENTION", None), getattr(alo_hip, "ALO_BLOCK_PACKED_QK", None)
A, B = alo_hip.ALO_BLOCK_NO_FFN, alo_hip.ALO_BLOCK_DECODER_NEXT
T32, T64 = alo_hip.ALO_BLOCK_TILE_32, alo_hip.ALO_BLOCK_TILE_64
BF16, F16, F32, F64 = alo_hip.ALO_BF16, alo_hip.ALO_F16, alo_hip.ALO_F32, alo_hip.ALO_F64
INVALID, UNSUPPORTED = 1, 2
NAMES = ("attn_out", "wo_packed", "bo", "norm1_w", "norm1_b", "src", "w1_packed", "b1", "w2_packed", "b2", "norm2_w", "norm2_b",
         "src_out", "pos", "padding_mask", "wv_packed", "bv", "wq_packed", "bq", "value_hm", "offsets_logits")
WANTED = ("attn_out", "src", "src_out", "pos")          # v, q, out, k; padding_mask may be there or not
BASE = {name: (1 << 20) * (i + 1) for i, name in enumerate(NAMES)}   # distinct, 16-byte aligned, never dereferenced, 1 MiB apart
t = torch.from_numpy


def _call(dtype=None, batch=2, S=70, F=70, eps1=SCALE, eps2=0.0, **over):
    """One call with fake pointers; ``dtype`` defaults to bf16 attention.  Every caller passes one bad argument."""
    ptrs = {name: BASE[name] if name in WANTED else None for name in NAMES}
    ptrs.update(over)
    lib = alo_hip.lib()
    rc = lib.alo_encoder_block(*[None if ptrs[n] is None else ctypes.c_void_p(ptrs[n]) for n in NAMES], batch, S, F, eps1, eps2,
                               BF16 | ATT if dtype is None else dtype, None)
    return rc, lib.alo_last_error().decode()


ODD = dict(attn_out=BASE["attn_out"] + 8)   # the last check before the spans: a call that reports it passed everything before


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def test_the_yardstick_is_multihead_attention_with_identity_projections():
    """fp64, CPU: in_proj = out_proj = identity, no bias.  Image 0 partly masked, image 1 fully masked (NaN), image 2 unmasked."""
    g = torch.Generator().manual_seed(5)
    E = HEADS * HEAD_DIM
    q, k, v = (torch.randn(3, n, E, generator=g, dtype=torch.float64) for n in (9, 13, 13))
    mask = torch.zeros(3, 13, dtype=torch.bool)
    mask[0, 4:9] = True
    mask[1] = True
    mha = nn.MultiheadAttention(E, HEADS, bias=False, batch_first=True).double().eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
        want = mha(q, k, v, key_padding_mask=mask)[0]   # as DETR's layers call it (need_weights=False takes bare SDPA: 0, not NaN)
    got = attention_ref(q, k, v, mask)
    assert torch.isnan(want[1]).all() and torch.isnan(got[1]).all()
    assert torch.isfinite(got[[0, 2]]).all()
    # the module scales q by 1 / sqrt(32) in fp64, the yardstick the product by the fp32 value of it: 2^-24 relative on the scores
    torch.testing.assert_close(got[[0, 2]], want[[0, 2]], rtol=0, atol=1e-6)
    assert torch.equal(attention_ref(q, k, v, mask.to(torch.uint8))[0], got[0])
    # without the fp32 rounding of the scale the two agree to fp64 rounding
    exact = torch.softmax((q.view(3, 9, HEADS, HEAD_DIM).transpose(1, 2) @ k.view(3, 13, HEADS, HEAD_DIM).permute(0, 2, 3, 1))
                          / HEAD_DIM ** 0.5, -1) @ v.view(3, 13, HEADS, HEAD_DIM).transpose(1, 2)
    torch.testing.assert_close(exact.transpose(1, 2).reshape(3, 9, E)[2], want[2], rtol=1e-12, atol=1e-13)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_both_flags_are_declared_in_the_header_and_in_alo_hip_with_equal_values():
    assert (ATT, PACKED) == (0x2000, 0x8000)
    header = open(alo_hip.CSRC_DIR + "/../../include/alo_encoder_block.h").read()
    for name in ("ALO_BLOCK_ATTENTION", "ALO_BLOCK_PACKED_QK"):
        assert f"#define {name} {getattr(alo_hip, name):#x}\n" in header
    assert len({A, B, T32, T64, ATT, PACKED}) == 6 and all(f & 0xff == 0 for f in (ATT, PACKED))
    assert alo_hip.lib().alo_abi_version() == 3


@pytest.mark.parametrize("dt", [BF16, F16, F32])
def test_a_well_formed_call_reaches_the_alignment_check(dt):
    """With every pointer as the flag wants it, a mask or none, separate or packed, the one odd pointer is what is named."""
    es = 4 if dt == F32 else 2
    for extra in ({}, {"padding_mask": BASE["padding_mask"]}):
        rc, msg = _call(dtype=dt | ATT, **ODD, **extra)
        assert rc == INVALID and "16-byte aligned" in msg, msg
        rc, msg = _call(dtype=dt | ATT | PACKED, pos=BASE["src"] + 256 * es, **ODD, **extra)
        assert rc == INVALID and "16-byte aligned" in msg, msg
    rc, msg = _call(dtype=dt | ATT, S=33, F=65, **ODD)       # cross-attention: S != F
    assert rc == INVALID and "16-byte aligned" in msg, msg


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_wanted_pointer_that_is_null_and_an_unwanted_one_that_is_set_are_refused_by_name(name):
    if name == "padding_mask":
        return   # optional
    rc, msg = _call(**{name: None if name in WANTED else BASE[name]})
    assert rc == INVALID and name in msg and "ALO_BLOCK_ATTENTION" in msg, msg
    assert ("is NULL" in msg) == (name in WANTED), msg


def test_packed_qk_needs_the_attention_flag_equal_lengths_and_the_other_half():
    rc, msg = _call(dtype=BF16 | PACKED, pos=BASE["src"] + 512)
    assert rc == INVALID and "ALO_BLOCK_PACKED_QK without ALO_BLOCK_ATTENTION" in msg, msg
    rc, msg = _call(dtype=BF16 | ATT | PACKED, pos=BASE["src"] + 512, S=70, F=71)
    assert rc == INVALID and "ALO_BLOCK_PACKED_QK" in msg and "F == S" in msg, msg
    for pos in (BASE["pos"], BASE["src"] + 1024, BASE["src"]):          # elsewhere; 256 fp32 elements on; q itself
        rc, msg = _call(dtype=BF16 | ATT | PACKED, pos=pos)
        assert rc == INVALID and "ALO_BLOCK_PACKED_QK" in msg and "pos == src + 256 elements" in msg, msg
    rc, msg = _call(dtype=F32 | ATT | PACKED, pos=BASE["src"] + 512)    # 256 bf16 elements on, in fp32
    assert rc == INVALID and "pos == src + 256 elements" in msg, msg


@pytest.mark.parametrize("other", [A, B, T32, T64, A | T32, B | T64, A | B])
def test_the_attention_flag_with_a_chain_or_tile_flag_is_refused(other):
    for flags in (ATT | other, ATT | PACKED | other):
        rc, msg = _call(dtype=BF16 | flags)
        assert rc == INVALID and "ALO_BLOCK_ATTENTION" in msg and f"{other:#x}" in msg, msg


@pytest.mark.parametrize("stray", [0x1000, 0x4000, 0x10000, 1 << 30])
def test_an_unknown_bit_is_refused_by_name_also_beside_the_attention_flags(stray):
    for flags in (stray | ATT, stray | ATT | PACKED, stray | PACKED, stray | ATT | A, stray | ATT | B | T32):
        rc, msg = _call(dtype=BF16 | flags)
        assert rc == UNSUPPORTED and f"{stray:#x}" in msg and "ALO_BLOCK_NO_FFN" in msg and "ALO_BLOCK_DECODER_NEXT" in msg, msg


def test_the_scale_must_be_positive_and_eps2_zero():
    for eps1 in (0.0, -0.125, float("nan")):
        rc, msg = _call(eps1=eps1)
        assert rc == INVALID and "eps1" in msg and "ALO_BLOCK_ATTENTION" in msg, msg
    for eps2 in (1e-5, -1.0, float("nan")):
        rc, msg = _call(eps2=eps2)
        assert rc == INVALID and "eps2" in msg and "ALO_BLOCK_ATTENTION" in msg, msg


def test_a_dtype_outside_the_three_is_refused():
    for dt in (F64, 4, 0xff):
        rc, msg = _call(dtype=dt | ATT)
        assert rc == UNSUPPORTED and "ALO_BLOCK_ATTENTION" in msg and "ALO_F32" in msg, msg


@pytest.mark.parametrize("sizes", [dict(batch=0), dict(S=0), dict(F=0), dict(batch=-1), dict(S=-3), dict(F=-70)])
def test_non_positive_sizes_are_refused(sizes):
    rc, msg = _call(**sizes)
    assert rc == INVALID and "positive" in msg, msg


def test_a_slab_of_two_gib_is_refused_and_one_just_below_is_not():
    rows = 2 ** 31 // 512                                     # bf16 rows of 256 elements that make 2 GiB exactly
    for sizes in (dict(batch=1, S=rows, F=70), dict(batch=1, S=70, F=rows), dict(batch=2, S=rows // 2, F=70)):
        rc, msg = _call(**sizes)
        assert rc == UNSUPPORTED and "2 GiB" in msg, msg
    rc, msg = _call(dtype=F32 | ATT, batch=1, S=rows // 2, F=70)
    assert rc == UNSUPPORTED and "2 GiB" in msg, msg
    rc, msg = _call(dtype=BF16 | ATT | PACKED, batch=1, S=rows // 2, F=rows // 2, pos=BASE["src"] + 512)   # pitch 512: q ends 256 short
    assert rc == INVALID and "overlaps" in msg, msg         # below the limit: it goes on to the spans (fake pointers 1 MiB apart)
    rc, msg = _call(dtype=BF16 | ATT | PACKED, batch=1, S=rows // 2 + 1, F=rows // 2 + 1, pos=BASE["src"] + 512)
    assert rc == UNSUPPORTED and "2 GiB" in msg, msg


@pytest.mark.parametrize("name", WANTED)
def test_pointers_off_a_16_byte_boundary_are_refused(name):
    for off in (2, 4, 8):
        rc, msg = _call(**{name: BASE[name] + off})
        assert rc == INVALID and "16-byte aligned" in msg, msg


@pytest.mark.parametrize("name", ["src", "pos", "attn_out", "padding_mask"])
def test_out_overlapping_an_input_is_refused(name):
    out = BASE["src_out"]
    nbytes = {"src": 2 * 70 * 512, "pos": 2 * 70 * 512, "attn_out": 2 * 70 * 512, "padding_mask": 2 * 70}[name]
    mask = {} if name == "padding_mask" else {"padding_mask": BASE["padding_mask"]}
    for at in (out, out + 2 * 70 * 512 - 16, out - nbytes + 16):     # on it, on its last bytes, ending in its first bytes
        rc, msg = _call(**{name: at}, **mask)
        assert rc == INVALID and "overlaps" in msg, msg


# ---- the routes say no on the CPU ---------------------------------------------------------------------------------------------
def _detr_transformer(dtype=torch.float64):
    from alonet.detr import Transformer

    tr = Transformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=512, dropout=0.0,
                     return_intermediate_dec=True).to(dtype).eval()
    res = tr.load_state_dict(formula_state_dict(tr.state_dict()))
    assert not res.missing_keys and not res.unexpected_keys
    return tr


def test_attention_routed_reads_the_switch_per_call(monkeypatch):
    monkeypatch.delenv("ALO_ATTENTION", raising=False)
    assert not alo_hip.attention_routed()
    monkeypatch.setenv("ALO_ATTENTION", "fused")
    assert alo_hip.attention_routed()
    monkeypatch.setenv("ALO_ATTENTION", "off")
    assert not alo_hip.attention_routed()


def test_the_switch_changes_no_bit_of_the_detr_transformer_on_cpu_tensors(golden, monkeypatch):
    g = golden("g22_detr_transformer_d256.npz")
    tr = _detr_transformer(torch.float32)
    args = (t(g["src"]), t(g["mask"]), t(g["query"]), t(g["pos"]))
    outs = []
    for value in (None, "fused"):
        monkeypatch.delenv("ALO_ATTENTION", raising=False) if value is None else monkeypatch.setenv("ALO_ATTENTION", value)
        with torch.no_grad():
            outs.append(tr(*args))
    for key in ("hs", "memory"):
        assert torch.equal(outs[0][key], outs[1][key]) and outs[0][key].stride() == outs[1][key].stride()
    assert not alo_hip.attention_supported(torch.zeros(2, 5, 256), torch.zeros(2, 5, 256), torch.zeros(2, 5, 256))


def test_the_switch_changes_no_bit_of_the_deformable_transformer_on_cpu_tensors(golden, monkeypatch):
    from alonet.deformable_detr import DeformableTransformer

    g = golden("g12_deformable_transformer_d256.npz")
    d_model, nhead, enc, dec, ffn, L, dec_p, enc_p = (int(x) for x in g["cfg"])
    tr = DeformableTransformer(d_model=d_model, nhead=nhead, num_encoder_layers=enc, num_decoder_layers=dec, dim_feedforward=ffn,
                               dropout=0.0, return_intermediate_dec=True, num_feature_levels=L, dec_n_points=dec_p,
                               enc_n_points=enc_p).double().eval()
    assert not tr.load_state_dict(formula_state_dict(tr.state_dict())).missing_keys
    srcs, poss = ([t(g[f"{n}{i}"]).double() for i in range(L)] for n in ("src", "pos"))
    masks = [t(g[f"mask{i}"]) for i in range(L)]
    outs = []
    for value in (None, "fused"):
        monkeypatch.delenv("ALO_ATTENTION", raising=False) if value is None else monkeypatch.setenv("ALO_ATTENTION", value)
        with torch.no_grad():
            outs.append(tr(srcs, masks, poss, t(g["query_embed"]).double(), is_tracing=None))
    assert torch.equal(outs[0]["hs"], outs[1]["hs"])
    assert all(torch.equal(a, b) for a, b in zip(outs[0]["memory"], outs[1]["memory"]))


def test_the_wrapper_refuses_what_the_kernel_does_not_take():
    x = torch.zeros(2, 5, 256)
    with pytest.raises(RuntimeError, match="attention: needs CUDA"):
        alo_hip.attention(x, x, x)
    w = torch.zeros(2, 5, 256, requires_grad=True)
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.attention(w, x, x)


# ---- G22 ----------------------------------------------------------------------------------------------------------------------
def test_g22_detr_transformer_on_stock_ops_matches_the_reference(golden, monkeypatch):
    monkeypatch.delenv("ALO_ATTENTION", raising=False)
    g = golden("g22_detr_transformer_d256.npz")
    assert g["hs"].dtype == np.float64 and g["hs"].shape == (2, 2, 37, 256) and g["memory"].shape == (2, 256, 7, 10)
    assert not g["mask"][0].any() and g["mask"][1].sum() == 70 - 30 and not g["mask"][1, :5, :6].any()
    tr = _detr_transformer()
    with torch.no_grad():
        out = tr(t(g["src"]).double(), t(g["mask"]), t(g["query"]).double(), t(g["pos"]).double())
    np.testing.assert_allclose(out["hs"].numpy(), g["hs"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["memory"].numpy(), g["memory"], rtol=0, atol=1e-9)
