"""The dilated flavour of alo_conv3x3_nhwc (ALO_CONV_DILATION_2 in ``stride``: 3x3, stride 1, dilation 2, zero padding 2, ALO_BF16 and
ALO_F32; aloception-oss_amd/csrc/conv.hip, conv_f32.hip) as far as it can be checked without a GPU: the C ABI checks a flagged call
before anything is enqueued, the workspace answer is stride 1's, no symbol was added, the gates' geometry table, and the fp32 flavour's
arithmetic restated in numpy (conv_dilated_ref.py) meets the fp64 convolution within the bound of conv_f32_ref.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alo_hip
from conv_dilated_ref import conv3x3_dilated_split, reference_and_bound
from helpers import HEADERS, declared_functions, exported_alo_functions
from kernel_bounds import compare

FLAG = alo_hip.ALO_CONV_DILATION_2
DTYPES = pytest.mark.parametrize("dt", [alo_hip.ALO_BF16, alo_hip.ALO_F32], ids=["bf16", "f32"])

# ---- the C ABI: validation happens before anything is enqueued, so every call here carries one bad argument and never launches ----
ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary


def _call(stride, dtype, w=ONE):
    lib = alo_hip.lib()
    rc = lib.alo_conv3x3_nhwc(ONE, w, ONE, ONE, ONE, 1, 8, 9, 64, 64, stride, 0, dtype, None)
    return rc, lib.alo_last_error()


def test_the_flag_sits_above_the_low_byte_beside_the_tap_flags():
    assert FLAG & 0xff == 0
    assert FLAG not in (alo_hip.ALO_CONV_TAPS_1X5, alo_hip.ALO_CONV_TAPS_5X1)
    assert FLAG & (alo_hip.ALO_CONV_TAPS_1X5 | alo_hip.ALO_CONV_TAPS_5X1) == 0
    header = open(alo_hip.CSRC_DIR + "/../../include/alo_hotpath.h").read()
    assert "#define ALO_CONV_DILATION_2 0x800" in header and FLAG == 0x800


@DTYPES
def test_flagged_call_reaches_the_pointer_check(dt):
    """Accepted as far as a call without a GPU can tell: the one bad pointer is what is named.  (Without the feature the flag is a
    stray bit above the low byte, refused with status 2.)"""
    rc, msg = _call(1 | FLAG, dt, w=ODD)
    assert rc == 1 and b"16-byte aligned" in msg, msg
    assert (rc, msg) == _call(1, dt, w=ODD)           # the undilated call's check, the undilated call's message


@DTYPES
def test_flag_with_stride_2_is_refused_by_name(dt):
    rc, msg = _call(2 | FLAG, dt)
    assert rc == 2 and b"ALO_CONV_DILATION_2" in msg and b"stride 1" in msg, msg


@DTYPES
@pytest.mark.parametrize("taps", [alo_hip.ALO_CONV_TAPS_1X5, alo_hip.ALO_CONV_TAPS_5X1], ids=["1x5", "5x1"])
def test_flag_with_a_tap_flag_is_refused_by_name(dt, taps):
    rc, msg = _call(1 | FLAG | taps, dt)
    assert rc == 2 and b"ALO_CONV_DILATION_2" in msg and b"ALO_CONV_TAPS" in msg, msg


@pytest.mark.parametrize("dt", [alo_hip.ALO_F16, alo_hip.ALO_F64])
def test_fp16_and_fp64_are_refused_for_their_dtype_as_without_the_flag(dt):
    rc, msg = _call(1 | FLAG, dt)
    assert rc == 2 and b"bf16 only" in msg, msg
    assert (rc, msg) == _call(1, dt)


@DTYPES
def test_a_stray_bit_beside_the_flag_is_still_refused_by_the_taps_names(dt):
    rc, msg = _call(1 | FLAG | 0x400, dt)
    assert rc == 2 and b"ALO_CONV_TAPS_1X5" in msg and b"ALO_CONV_TAPS_5X1" in msg, msg


@DTYPES
def test_a_flagged_bad_low_byte_is_a_bad_stride(dt):
    rc, msg = _call(3 | FLAG, dt)
    assert rc == 2 and b"stride must be 1 or 2 (got 3)" in msg, msg


@DTYPES
def test_the_other_checks_are_the_undilated_calls(dt):
    lib = alo_hip.lib()
    bad = {   # (x, w_packed, bias, y, workspace, N, H, W, Cin, Cout)
        "Cin": (ONE, ONE, ONE, ONE, ONE, 1, 8, 9, 96, 64),
        "null": (ONE, None, ONE, ONE, ONE, 1, 8, 9, 64, 64),
        "size": (ONE, ONE, ONE, ONE, ONE, 1, 0, 9, 64, 64),
        "large": (ONE, ONE, ONE, ONE, ONE, 1, 1 << 12, 1 << 12, 64, 64),
    }
    for name, args in bad.items():
        rc = lib.alo_conv3x3_nhwc(*args, 1 | FLAG, 0, dt, None)
        msg = lib.alo_last_error()
        assert rc != 0, name
        assert (rc, msg) == (lib.alo_conv3x3_nhwc(*args, 1, 0, dt, None), lib.alo_last_error()), name


def test_flagged_fp32_call_without_a_workspace_is_refused_by_name():
    lib = alo_hip.lib()
    rc = lib.alo_conv3x3_nhwc(ONE, ONE, ONE, ONE, None, 1, 8, 9, 64, 64, 1 | FLAG, 0, alo_hip.ALO_F32, None)
    assert rc == 1 and b"workspace" in lib.alo_last_error(), lib.alo_last_error()


def test_workspace_bytes_of_the_flagged_stride_are_stride_1s():
    """(1, 13, 21, 512 -> 512): 273 pixels = 5 tiles, 4 column blocks, so conv_zsplit gives z = 4 (512 / 8 = 64 input channels per range
    would be fewer than its 128).  Without the feature the flagged stride answers 0."""
    lib = alo_hip.lib()
    flagged = lib.alo_conv3x3_workspace_bytes(1, 13, 21, 512, 512, 1 | FLAG)
    assert flagged == lib.alo_conv3x3_workspace_bytes(1, 13, 21, 512, 512, 1) > 0
    assert flagged == 4 * 13 * 21 * 512 * 4                                     # z = 4 partial sums in fp32
    for shape in ((1, 1, 1, 64, 64), (8, 50, 84, 512, 512), (1, 4, 4, 2048, 256), (2, 5, 7, 64, 64)):
        assert lib.alo_conv3x3_workspace_bytes(*shape, 1 | FLAG) == lib.alo_conv3x3_workspace_bytes(*shape, 1)
    assert lib.alo_conv3x3_workspace_bytes(1, 13, 21, 512, 512, 2 | FLAG) == 0  # no such call
    assert lib.alo_conv3x3_workspace_bytes(1, 13, 21, 512, 512, 1 | FLAG | alo_hip.ALO_CONV_TAPS_1X5) == 0


def test_no_symbol_was_added():
    """ABI 3, the entry points of the four headers, one signature each: the flag rides in an existing argument.  (The one entry point
    added since, alo_msda_generic_plan, is a host-only query of the MSDA plans: 50 names, 42 of them in alo_hotpath.h.)"""
    assert alo_hip.lib().alo_abi_version() == 3
    declared = {name for header in HEADERS for name in declared_functions(header)}
    assert exported_alo_functions(alo_hip.LIB_PATH) == declared == set(alo_hip._SIGNATURES)
    assert len(declared) == 50 and len(declared_functions("alo_hotpath.h")) == 42


# ---- the gates, off the GPU: the geometry table alone (a CPU tensor never passes) --------------------------------------------------
def test_the_gates_know_three_geometries():
    assert set(alo_hip._CONV3X3_GEOMETRIES) == {((1, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1)), ((1, 1), (2, 2), (2, 2))}
    x = torch.zeros(1, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(64, 64, 3, 3)
    with torch.no_grad():
        assert not alo_hip.conv3x3_f32_supported(x, w, (1, 1), (2, 2), (2, 2))       # not on the GPU
        with pytest.raises(RuntimeError):
            alo_hip.conv3x3_f32(x, w, dilation=2)


def test_dc5_backbone_on_cpu_tensors_takes_the_stock_ops(monkeypatch):
    from alonet.detr.backbone import Bottleneck

    def refuse(*a, **k):
        raise AssertionError("a HIP wrapper was called for CPU tensors")

    torch.manual_seed(2)
    block = Bottleneck(256, 64, 1, 2).eval()
    assert block.conv2.dilation == (2, 2) and block.conv2.padding == (2, 2)
    x = torch.randn(1, 256, 6, 7)
    monkeypatch.setenv("ALO_F32_LAYERS", "split")
    for name in ("conv3x3", "conv3x3_f32"):
        monkeypatch.setattr(alo_hip, name, refuse)
    with torch.no_grad():
        got = block(x)
    ref = F.relu(block.bn2(block.conv2(F.relu(block.bn1(block.conv1(x))))))
    ref = F.relu(block.bn3(block.conv3(ref)) + x)
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)


# ---- the fp32 flavour's arithmetic, restated -----------------------------------------------------------------------------------------
SCALES = [(1.0, 1.0), (1e-3, 1e-3), (3e4, 7e5), (1e-20, 1e-12), (1e12, 1e-15), (5e18, 3e17)]   # test_conv3x3_f32_cpu.py


def _operands(sa, sb, seed, batch=False):
    """test_conv3x3_f32_cpu.py's operands: (2, 8, 9, 64) images whose input channels 0-6 are 10^6 times smaller than the others;
    ``batch``: four images — ordinary, all-zero, 10^6 times dimmer, ordinary — and output channel 3 10^6 times smaller."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((4 if batch else 2, 8, 9, 64)) * sa).astype(np.float32)
    x[..., :7] *= np.float32(1e-6)
    w = (rng.standard_normal((64, 3, 3, 64)) * (sb / 24.0)).astype(np.float32)
    b = (rng.standard_normal(64) * sa * sb).astype(np.float32)
    if batch:
        x[1] = 0
        x[2] *= np.float32(1e-6)
        w[3] *= np.float32(1e-6)
        b[3] *= np.float32(1e-6)
    return x, w, b


def _check(x, w, b, what):
    xt, wt = torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(0, 3, 1, 2)
    for bias, relu in ((b, True), (None, False)):
        got = torch.from_numpy(conv3x3_dilated_split(x, w, bias, relu)).permute(0, 3, 1, 2)
        ref, bound = reference_and_bound(xt, wt, None if bias is None else torch.from_numpy(bias), relu)
        ratio = compare(got, ref, bound, f"split dilated conv {what} relu={relu}")
        print(f"{what} relu={relu}: worst |err| / bound = {ratio:.3f}")
        yield got, bias


@pytest.mark.parametrize("sa,sb", SCALES)
def test_restated_arithmetic_meets_the_bound(sa, sb):
    list(_check(*_operands(sa, sb, 11), f"sa={sa} sb={sb}"))


def test_restated_arithmetic_on_a_zero_image_a_dim_image_and_a_tiny_channel():
    for got, bias in _check(*_operands(1.0, 1.0, 13, batch=True), "zero / dim / tiny"):
        assert (got[1] == (0 if bias is None else torch.relu(torch.from_numpy(bias)).view(-1, 1, 1))).all()   # the all-zero image


def test_restated_window_is_the_dilated_convolutions():
    """Small integers: every product and sum is exact, so the restatement equals F.conv2d(..., padding=2, dilation=2) bit for bit —
    the window order (ky, kx, c; zero outside) is the weight's, on maps smaller than the reach as well."""
    rng = np.random.default_rng(3)
    for h, wd in ((4, 6), (1, 1), (2, 3), (5, 2)):
        x = rng.integers(-3, 4, (1, h, wd, 64)).astype(np.float32)
        w = rng.integers(-2, 3, (64, 3, 3, 64)).astype(np.float32)
        got = torch.from_numpy(conv3x3_dilated_split(x, w, None, False)).permute(0, 3, 1, 2)
        ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), torch.from_numpy(w).permute(0, 3, 1, 2).double(), None, 1, 2, 2)
        assert torch.equal(got.double(), ref)
