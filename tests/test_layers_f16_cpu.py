"""ALO_F16 is a served dtype of the transformer's layer kernels: the C ABI checks the dtype first and then holds an fp16 call to
the argument checks of a bf16 call, with the same messages.  Validation happens before anything is enqueued, so no GPU is needed:
every call here carries one bad argument and never reaches a launch."""
import ctypes

import pytest

import alo_hip

ONE = ctypes.c_void_p(16)    # never dereferenced: validation fails first
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
SHAPES = (ctypes.c_int * 2)(4, 4)


def _cases(dt):
    """name -> (entry point, arguments with ONE bad argument and dtype ``dt``, what the message must name)."""
    return {
        "linear_shortk/K": ("alo_linear_shortk", (ONE, ONE, ONE, None, ONE, 8, 64, 100, 0, dt, None), b"K must be 64, 128 or 256"),
        "linear_shortk/pointer": ("alo_linear_shortk", (ONE, ODD, ONE, None, ONE, 8, 64, 64, 0, dt, None), b"16-byte aligned"),
        "linear_shortk/residual": ("alo_linear_shortk", (ONE, ONE, ONE, ODD, ONE, 8, 64, 256, 1, dt, None), b"16-byte aligned"),
        "linear_packed/K": ("alo_linear_packed", (ONE, ONE, ONE, None, ONE, 8, 128, 100, 0, dt, None), b"K must be a multiple of 256"),
        "linear_packed/pointer": ("alo_linear_packed", (ODD, ONE, ONE, None, ONE, 8, 128, 512, 0, dt, None), b"16-byte aligned"),
        "ffn256/F": ("alo_ffn256", (ONE, ONE, ONE, ONE, ONE, ONE, 8, 300, dt, None), b"multiple of 256"),
        "ffn256/pointer": ("alo_ffn256", (ONE, ONE, ONE, ODD, ONE, ONE, 8, 256, dt, None), b"16-byte aligned"),
        "value_proj_head_major/K": ("alo_value_proj_head_major", (ONE, ONE, ONE, None, ONE, 1, 8, 2, 100, dt, None), b"K must be 64, 128 or 256"),
        "value_proj_head_major/pointer": ("alo_value_proj_head_major", (ONE, ONE, ONE, None, ODD, 1, 8, 2, 64, dt, None), b"16-byte aligned"),
        "pack_mfma_b/K": ("alo_pack_mfma_b", (ONE, ONE, 32, 100, dt, None), b"K a multiple of 16"),
        "add_layernorm/pointer": ("alo_add_layernorm", (ONE, None, ONE, ODD, ONE, None, None, 4, 256, 1e-5, dt, None), b"16-byte aligned"),
        "add_layernorm/C": ("alo_add_layernorm", (ONE, None, ONE, ONE, ONE, None, None, 4, 258, 1e-5, dt, None), b"multiple of 4"),
        "bias_act/pointer": ("alo_bias_act", (ODD, ONE, None, ONE, 4, 64, 1, dt, None), b"16-byte aligned"),
        "pos_sine_flat/pointer": ("alo_pos_sine_flat", (ONE, ONE, ONE, ONE, ONE, ODD, ONE, 1, 16, 1, 128, 1, 1, 6.28, 1e-6, dt, None),
                                  b"16-byte aligned"),
        "mask_rows/pointer": ("alo_mask_rows", (ODD, ONE, ctypes.c_void_p(32), 4, 8, dt, None), b"16-byte aligned"),
        "mask_rows/C": ("alo_mask_rows", (ONE, ONE, ctypes.c_void_p(32), 4, 12, dt, None), b"16 bytes"),
        "encoder_proposals_masked/pointer": ("alo_encoder_proposals_masked", (ONE, ONE, ONE, ODD, ctypes.c_void_p(32), 1, 1, SHAPES, 8, dt, None),
                                             b"16-byte aligned"),
        "proposal_queries/pointer": ("alo_proposal_queries", (ONE, ONE, ONE, ONE, ODD, 1, 4, 1, dt, None), b"16-byte aligned"),
    }


NAMES = sorted(_cases(alo_hip.ALO_F16))


@pytest.mark.parametrize("name", NAMES)
def test_fp16_call_meets_the_argument_checks_of_a_bf16_call(name):
    lib = alo_hip.lib()
    messages = {}
    for dt in (alo_hip.ALO_F16, alo_hip.ALO_BF16):
        symbol, args, names = _cases(dt)[name]
        rc = getattr(lib, symbol)(*args)
        messages[dt] = lib.alo_last_error()
        assert rc != 0 and names in messages[dt], (name, dt, rc, messages[dt])
        for word in (b"dtype", b"bf16", b"fp16", b"F16"):
            assert word not in messages[dt], (name, dt, messages[dt])
    assert messages[alo_hip.ALO_F16] == messages[alo_hip.ALO_BF16]


@pytest.mark.parametrize("name", NAMES)
def test_fp64_is_refused_for_its_dtype_before_any_other_argument(name):
    lib = alo_hip.lib()
    symbol, args, names = _cases(alo_hip.ALO_F64)[name]
    rc = getattr(lib, symbol)(*args)
    assert rc == 2 and b"dtype" in lib.alo_last_error() and names not in lib.alo_last_error(), (name, lib.alo_last_error())


def test_encoder_block_still_refuses_fp16():
    lib = alo_hip.lib()
    ptrs = [ONE] * 21
    for dt in (alo_hip.ALO_F16, alo_hip.ALO_F32):
        rc = lib.alo_encoder_block(*ptrs, 1, 64, 256, 1e-5, 1e-5, dt, None)
        assert rc != 0 and b"bf16 only" in lib.alo_last_error(), (dt, lib.alo_last_error())


def test_conv1x1_nhwc_still_refuses_fp16():
    lib = alo_hip.lib()
    rc = lib.alo_conv1x1_nhwc(ONE, ONE, 0, ONE, None, ONE, 1, 4, 4, 64, 64, 1, 0, alo_hip.ALO_F16, None)
    assert rc == 2 and b"bf16 only" in lib.alo_last_error()
