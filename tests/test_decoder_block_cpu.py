"""The decoder forms of alo_encoder_block (ALO_BLOCK_NO_FFN / ALO_BLOCK_DECODER_NEXT above the low byte of ``dtype``,
include/alo_encoder_block.h): every refusal happens before anything is enqueued and names the flag or the argument, so every call
here carries one bad argument and never launches.  No GPU."""
import ctypes

import pytest

import alo_hip

A, B = alo_hip.ALO_BLOCK_NO_FFN, alo_hip.ALO_BLOCK_DECODER_NEXT
T32, T64 = alo_hip.ALO_BLOCK_TILE_32, alo_hip.ALO_BLOCK_TILE_64
BF16 = alo_hip.ALO_BF16
NAMES = ("attn_out", "wo_packed", "bo", "norm1_w", "norm1_b", "src", "w1_packed", "b1", "w2_packed", "b2", "norm2_w", "norm2_b",
         "src_out", "pos", "padding_mask", "wv_packed", "bv", "wq_packed", "bq", "value_hm", "offsets_logits")
# the pointers each chain takes; every other one must be NULL
WANTED = {
    A: {"attn_out", "wo_packed", "bo", "norm1_w", "norm1_b", "src", "src_out", "pos", "wq_packed", "bq", "offsets_logits"},
    B: set(NAMES) - {"padding_mask"},
}
CHAINS = pytest.mark.parametrize("chain", [A, B], ids=["no_ffn", "decoder_next"])


def _pointers(chain, **over):
    """Distinct, 16-byte aligned, never dereferenced, 1 MiB apart: no two spans of a 2 x 70-row call overlap."""
    ptrs = {name: (1 << 20) * (i + 1) if name in WANTED[chain] else None for i, name in enumerate(NAMES)}
    ptrs.update(over)
    return [None if ptrs[name] is None else ctypes.c_void_p(ptrs[name]) for name in NAMES]


def _call(chain, dtype=None, F=1024, batch=2, S=70, **over):
    lib = alo_hip.lib()
    rc = lib.alo_encoder_block(*_pointers(chain, **over), batch, S, F, 1e-5, 1e-5, BF16 | chain if dtype is None else dtype, None)
    return rc, lib.alo_last_error().decode()


def test_the_flags_sit_above_the_low_byte_and_match_the_header():
    flags = (A, B, T32, T64)
    assert all(f & 0xff == 0 for f in flags) and len(set(flags)) == 4
    header = open(alo_hip.CSRC_DIR + "/../../include/alo_encoder_block.h").read()
    for name in ("ALO_BLOCK_NO_FFN", "ALO_BLOCK_DECODER_NEXT", "ALO_BLOCK_TILE_32", "ALO_BLOCK_TILE_64"):
        assert f"#define {name} {getattr(alo_hip, name):#x}\n" in header
    assert alo_hip.lib().alo_abi_version() == 3


@CHAINS
def test_a_flagged_call_reaches_the_alignment_check(chain):
    """Accepted as far as a call without a GPU can tell: with every pointer as the flag wants it, the one odd pointer is named."""
    for tile in (0, T32, T64):
        rc, msg = _call(chain, dtype=BF16 | chain | tile, attn_out=(1 << 20) + 8)
        assert rc == 1 and "16-byte aligned" in msg, msg


@CHAINS
def test_a_flag_with_fp16_or_fp32_is_refused_by_name(chain):
    for dt in (alo_hip.ALO_F16, alo_hip.ALO_F32):
        rc, msg = _call(chain, dtype=dt | chain)
        assert rc == 2 and ("ALO_BLOCK_NO_FFN" if chain == A else "ALO_BLOCK_DECODER_NEXT") in msg and "bf16 only" in msg, msg


def test_both_chains_at_once_are_refused_by_name():
    rc, msg = _call(B, dtype=BF16 | A | B)
    assert rc == 1 and "ALO_BLOCK_NO_FFN" in msg and "ALO_BLOCK_DECODER_NEXT" in msg, msg


@pytest.mark.parametrize("stray", [0x1000, 0x4000, 0x10000, 1 << 30])
def test_an_unknown_bit_is_refused_by_name(stray):
    for flags in (stray, stray | A, stray | B, stray | B | T32):
        rc, msg = _call(B, dtype=BF16 | flags)
        assert rc == 2 and f"{stray:#x}" in msg and "ALO_BLOCK_NO_FFN" in msg and "ALO_BLOCK_DECODER_NEXT" in msg, msg


def test_tile_heights_need_a_chain_and_exclude_each_other():
    rc, msg = _call(B, dtype=BF16 | T32)
    assert rc == 1 and "without ALO_BLOCK_NO_FFN or ALO_BLOCK_DECODER_NEXT" in msg, msg
    rc, msg = _call(B, dtype=BF16 | B | T32 | T64)
    assert rc == 1 and "ALO_BLOCK_TILE_32" in msg and "ALO_BLOCK_TILE_64" in msg, msg


@CHAINS
def test_a_missing_pointer_is_refused_by_name(chain):
    for name in sorted(WANTED[chain]):
        rc, msg = _call(chain, **{name: None})
        assert rc == 1 and f"{name} is NULL" in msg, (name, msg)


@CHAINS
def test_a_pointer_the_flag_does_not_take_is_refused_by_name(chain):
    for name in sorted(set(NAMES) - WANTED[chain]):
        rc, msg = _call(chain, **{name: 1 << 27})
        assert rc == 1 and f"{name} must be NULL" in msg, (name, msg)


def test_hidden_width_and_sizes():
    for F in (0, 100, 1000, -256):
        rc, msg = _call(B, F=F)
        assert rc == 1 and "multiple of 256" in msg, (F, msg)
    rc, msg = _call(A, F=0, attn_out=(1 << 20) + 8)   # chain A has no hidden layer: F is not looked at
    assert rc == 1 and "16-byte aligned" in msg, msg
    for kw in (dict(batch=0), dict(S=0), dict(batch=-1)):
        rc, msg = _call(A, **kw)
        assert rc == 1 and "positive" in msg, (kw, msg)


@CHAINS
def test_an_output_over_an_input_is_refused(chain):
    rows = 2 * 70
    rc, msg = _call(chain, src_out=(1 << 20) * 6 + rows * 512 - 16)            # the tail of src
    assert rc == 1 and "overlaps" in msg, msg
    rc, msg = _call(chain, offsets_logits=(1 << 20) * 14)                      # pos
    assert rc == 1 and "overlaps" in msg, msg
    if chain == B:                                                             # 512 query columns: 1024 bytes per row
        rc, msg = _call(chain, offsets_logits=(1 << 20) * 20 - rows * 1024 + 16)
        assert rc == 1 and "overlaps" in msg, msg


def test_a_call_without_flags_validates_as_before():
    lib = alo_hip.lib()
    full = [ctypes.c_void_p((1 << 20) * (i + 1)) for i in range(21)]
    full[14] = None
    call = lambda ptrs, F=1024, dtype=BF16: (lib.alo_encoder_block(*ptrs, 2, 70, F, 1e-5, 1e-5, dtype, None), lib.alo_last_error().decode())
    odd = list(full)
    odd[0] = ctypes.c_void_p((1 << 20) + 8)
    assert call(odd) == (1, "alo_encoder_block: pointers must be 16-byte aligned")
    no_w1 = list(full)
    no_w1[6] = None
    assert call(no_w1) == (1, "alo_encoder_block: null pointer argument")
    half_tail = list(full)
    half_tail[2] = None
    rc, msg = call(half_tail)
    assert rc == 1 and "go together" in msg, msg
    rc, msg = call(full, F=1000)
    assert rc == 1 and "multiple of 256" in msg, msg
    for dt in (alo_hip.ALO_F16, alo_hip.ALO_F32):
        assert call(full, dtype=dt) == (2, f"alo_encoder_block: bf16 only (dtype {dt})")
    # what chain A takes is, without its flag, an encoder call with its always-needed pointers missing
    rc, msg = call(_pointers(A))
    assert (rc, msg) == (1, "alo_encoder_block: null pointer argument")


def test_the_route_is_switched_per_call(monkeypatch):
    monkeypatch.delenv("ALO_DEC_BLOCK", raising=False)
    assert alo_hip.decoder_block_enabled()
    for off in ("off", "0", "OFF"):
        monkeypatch.setenv("ALO_DEC_BLOCK", off)
        assert not alo_hip.decoder_block_enabled()
    monkeypatch.setenv("ALO_DEC_BLOCK", "on")
    assert alo_hip.decoder_block_enabled()


# ---- the hidden widths the gates admit are the ones whose LDS frame fits ------------------------------------------------------------
def _csrc_int(header, name):
    """``constexpr int <name> = <arithmetic>;`` of a csrc header, evaluated."""
    import re

    text = open(f"{alo_hip.CSRC_DIR}/{header}").read()
    return eval(re.search(rf"constexpr int {name} = ([0-9 *+]+);", text).group(1))


def test_the_lds_formulas_use_the_kernels_constants():
    assert alo_hip.BLOCK_LDS_LIMIT == _csrc_int("common.hpp", "kLdsLimit") == 160 * 1024
    assert alo_hip.BLOCK_TILE_STRIDE == _csrc_int("mfma_tile.hpp", "kTileStride") == 528
    # the tables as the kernels lay them out: encoder b2, bo, bv, g1, e1, g2, e2 + 384 of bq; chain B bo, g1, e1, bv, b2, g2, e2 + 512 of bqk
    assert alo_hip.ENCODER_BLOCK_TABLES == 7 * 256 + 384 and alo_hip.DECODER_BLOCK_TABLES == 7 * 256 + 512
    assert alo_hip.encoder_block_lds_bytes(1024) == 2 * 64 * 528 + 4 * (1024 + 2176)
    assert alo_hip.decoder_block_lds_bytes(1024, 32) == 4 * 32 * 528 + 4 * (1024 + 2304)
    assert alo_hip.decoder_block_lds_bytes(1024, 64) == 4 * 64 * 528 + 4 * (1024 + 2304)


FRAMES = {   # the widest hidden layer each frame takes, the next width the issue of the gates names, and the frame's bytes
    "decoder64": (4864, 5120, lambda F: alo_hip.decoder_block_lds_bytes(F, 64)),     # chain B at 64 rows
    "decoder32": (21760, 22016, lambda F: alo_hip.decoder_block_lds_bytes(F, 32)),   # chain B at 32 rows: the widest the route takes
    "encoder": (21888, 22144, lambda F: alo_hip.encoder_block_lds_bytes(F)),
}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_each_frame_fits_up_to_its_boundary_and_not_beyond(name):
    fits, over, frame = FRAMES[name]
    assert frame(fits) == alo_hip.BLOCK_LDS_LIMIT          # the boundary is exact: one more hidden unit does not fit
    assert frame(fits + 1) > alo_hip.BLOCK_LDS_LIMIT and frame(over) > alo_hip.BLOCK_LDS_LIMIT
    assert frame(fits - 256) < alo_hip.BLOCK_LDS_LIMIT


def test_the_predicted_tile_height_follows_the_frame(monkeypatch):
    monkeypatch.setitem(alo_hip._CU_COUNT, 0, 256)         # no device is asked
    few, many = 2400, 64 * 256 + 37
    for hidden, at_many in ((0, 64), (256, 64), (1024, 64), (4864, 64), (5120, 32), (21760, 32)):
        assert alo_hip.decoder_block_tile_rows(few, "cuda:0", hidden) == 32, hidden
        assert alo_hip.decoder_block_tile_rows(many, "cuda:0", hidden) == at_many, hidden
    # without a width the rule is the one existing callers know: 64 rows from ceil(rows / 64) = compute units on
    assert alo_hip.decoder_block_tile_rows(64 * 255, "cuda:0") == 32 and alo_hip.decoder_block_tile_rows(64 * 255 + 1, "cuda:0") == 64
