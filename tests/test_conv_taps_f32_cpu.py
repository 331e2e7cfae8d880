"""The five-tap flavours of alo_conv3x3_nhwc (ALO_CONV_TAPS_1X5 / ALO_CONV_TAPS_5X1 in ``stride``, dtype = ALO_F32;
aloception-oss_amd/csrc/conv_f32.hip) as far as they can be checked without a GPU: the arithmetic restated in numpy
(conv_taps_f32_ref.py) meets the fp64 convolution within the bound of conv_f32_ref.py at 5 Cin products; the C ABI checks a flagged
call before anything is enqueued; and ``ALO_RAFT_GRU=split`` leaves a SepConvGRU on CPU tensors on the stock ops."""
import ctypes

import numpy as np
import pytest
import torch

import alo_hip
from conv_taps_f32_ref import conv_taps_split, reference_and_bound, weight_4d
from kernel_bounds import compare

SCALES = [(1.0, 1.0), (1e-3, 1e-3), (3e4, 7e5), (1e-20, 1e-12), (1e12, 1e-15), (5e18, 3e17)]   # test_conv3x3_f32_cpu.py
GEOMETRIES = pytest.mark.parametrize("vertical", [False, True], ids=["1x5", "5x1"])


def _operands(sa, sb, seed, batch=False):
    """test_conv3x3_f32_cpu.py's operands with a (64, 5, 64) tap-major weight: (2, 8, 9, 64) images whose input channels 0-6 are 10^6
    times smaller than the others; ``batch``: four images — ordinary, all-zero, 10^6 times dimmer, ordinary — and output channel 3
    10^6 times smaller than the others."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((4 if batch else 2, 8, 9, 64)) * sa).astype(np.float32)
    x[..., :7] *= np.float32(1e-6)
    w = (rng.standard_normal((64, 5, 64)) * (sb / 18.0)).astype(np.float32)
    b = (rng.standard_normal(64) * sa * sb).astype(np.float32)
    if batch:
        x[1] = 0
        x[2] *= np.float32(1e-6)
        w[3] *= np.float32(1e-6)
        b[3] *= np.float32(1e-6)
    return x, w, b


def _check(x, w, b, vertical, what):
    xt, wt = torch.from_numpy(x).permute(0, 3, 1, 2), weight_4d(w, vertical)
    for bias, relu in ((b, True), (None, False)):
        got = torch.from_numpy(conv_taps_split(x, w, bias, vertical, relu)).permute(0, 3, 1, 2)
        ref, bound = reference_and_bound(xt, wt, None if bias is None else torch.from_numpy(bias), relu)
        ratio = compare(got, ref, bound, f"split five-tap conv {what} vertical={vertical} relu={relu}")
        print(f"{what} vertical={vertical} relu={relu}: worst |err| / bound = {ratio:.3f}")
        yield got, bias


@GEOMETRIES
@pytest.mark.parametrize("sa,sb", SCALES)
def test_restated_arithmetic_meets_the_bound(sa, sb, vertical):
    list(_check(*_operands(sa, sb, 11), vertical, f"sa={sa} sb={sb}"))


@GEOMETRIES
def test_restated_arithmetic_on_a_zero_image_a_dim_image_and_a_tiny_channel(vertical):
    for got, bias in _check(*_operands(1.0, 1.0, 13, batch=True), vertical, "zero / dim / tiny"):
        assert (got[1] == (0 if bias is None else torch.relu(torch.from_numpy(bias)).view(-1, 1, 1))).all()   # the all-zero image


@GEOMETRIES
def test_restated_window_is_the_convolutions(vertical):
    """Small integers: every product and sum is exact, so the restatement equals F.conv2d bit for bit — the window order (tap-major,
    zero outside) is the weight's."""
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, (1, 4, 6, 64)).astype(np.float32)
    w = rng.integers(-2, 3, (64, 5, 64)).astype(np.float32)
    got = torch.from_numpy(conv_taps_split(x, w, None, vertical, False)).permute(0, 3, 1, 2)
    ref, _ = reference_and_bound(torch.from_numpy(x).permute(0, 3, 1, 2), weight_4d(w, vertical), None, False)
    assert torch.equal(got.double(), ref)


# ---- the C ABI: validation happens before anything is enqueued, so every call here carries one bad argument and never launches ----
ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
FLAGS = pytest.mark.parametrize("flag", [alo_hip.ALO_CONV_TAPS_1X5, alo_hip.ALO_CONV_TAPS_5X1], ids=["1x5", "5x1"])


def _call(stride, dtype, w=ONE):
    lib = alo_hip.lib()
    rc = lib.alo_conv3x3_nhwc(ONE, w, ONE, ONE, ONE, 1, 8, 9, 64, 64, stride, 0, dtype, None)
    return rc, lib.alo_last_error()


def test_the_flags_sit_above_the_low_byte():
    assert alo_hip.ALO_CONV_TAPS_1X5 & 0xff == 0 and alo_hip.ALO_CONV_TAPS_5X1 & 0xff == 0
    assert alo_hip.ALO_CONV_TAPS_1X5 != alo_hip.ALO_CONV_TAPS_5X1
    header = open(alo_hip.CSRC_DIR + "/../../include/alo_hotpath.h").read()
    for name in ("ALO_CONV_TAPS_1X5", "ALO_CONV_TAPS_5X1"):
        assert f"#define {name} {getattr(alo_hip, name):#x}" in header


@FLAGS
def test_flagged_fp32_call_reaches_the_pointer_check(flag):
    """Accepted as far as a call without a GPU can tell: the one bad pointer is what is named.  (Without the feature a flagged stride
    answers "stride must be 1 or 2".)"""
    rc, msg = _call(1 | flag, alo_hip.ALO_F32, w=ODD)
    assert rc == 1 and b"16-byte aligned" in msg, msg


@FLAGS
def test_flag_with_bf16_is_refused_by_name(flag):
    rc, msg = _call(1 | flag, alo_hip.ALO_BF16)
    assert rc == 2 and b"ALO_CONV_TAPS" in msg and b"ALO_F32" in msg, msg


@FLAGS
def test_flag_with_stride_2_is_refused_by_name(flag):
    for dt in (alo_hip.ALO_F32, alo_hip.ALO_BF16):
        rc, msg = _call(2 | flag, dt)
        assert rc == 2 and b"ALO_CONV_TAPS" in msg and b"stride 1" in msg, msg


@pytest.mark.parametrize("stride", [1 | 0x400, 1 | 0x300, 1 | 0x10000, 2 | 0x1100, 1 | (1 << 30)])
def test_stray_bits_are_refused_by_name(stride):
    for dt in (alo_hip.ALO_F32, alo_hip.ALO_BF16):
        rc, msg = _call(stride, dt)
        assert rc == 2 and b"ALO_CONV_TAPS_1X5" in msg and b"ALO_CONV_TAPS_5X1" in msg, msg


@pytest.mark.parametrize("stride", [3, 0, -1, 255])
def test_an_unflagged_bad_stride_keeps_its_message(stride):
    for dt in (alo_hip.ALO_F32, alo_hip.ALO_BF16):
        rc, msg = _call(stride, dt)
        assert rc == 2 and msg == f"alo_conv3x3_nhwc: stride must be 1 or 2 (got {stride})".encode(), msg


@FLAGS
def test_a_flagged_bad_low_byte_is_a_bad_stride(flag):
    rc, msg = _call(3 | flag, alo_hip.ALO_F32)
    assert rc == 2 and b"stride must be 1 or 2 (got 3)" in msg, msg


@FLAGS
def test_workspace_bytes_of_a_flagged_stride(flag):
    """The five-tap kernels never split K: nothing but the per-image magnitudes, which the caller adds as for the 3x3."""
    lib = alo_hip.lib()
    for n, h, w, cin, cout in ((1, 1, 1, 64, 64), (4, 90, 160, 384, 256), (1, 4, 4, 2048, 256)):
        assert lib.alo_conv3x3_workspace_bytes(n, h, w, cin, cout, 1 | flag) == 0
    assert lib.alo_conv3x3_workspace_bytes(1, 4, 4, 2048, 256, 1) > 0          # the bf16 call's split-K answer is untouched


def test_abi_version_and_entry_points_are_unchanged():
    import re

    assert alo_hip.lib().alo_abi_version() == 3
    declared = set()
    for name in ("alo_hotpath.h", "alo_corr_alt.h", "alo_two_stage.h", "alo_encoder_block.h"):
        text = open(alo_hip.CSRC_DIR + "/../../include/" + name).read()
        declared |= set(re.findall(r"^[a-z][\w \*]*?\b(alo_\w+)\s*\(", text, flags=re.M))
    assert declared == set(alo_hip._SIGNATURES), declared ^ set(alo_hip._SIGNATURES)


# ---- the route, off the GPU ---------------------------------------------------------------------------------------------------------
def test_sepconvgru_on_cpu_tensors_takes_the_stock_ops_with_the_knob_set(monkeypatch):
    from alonet.raft.update import SepConvGRU

    def refuse(*a, **k):
        raise AssertionError("a HIP wrapper was called for CPU tensors")

    torch.manual_seed(1)
    gru = SepConvGRU(hidden_dim=128, input_dim=256).eval()
    h, x = torch.randn(1, 128, 4, 8).tanh(), torch.randn(1, 256, 4, 8)
    monkeypatch.delenv("ALO_RAFT_GRU", raising=False)
    with torch.no_grad():
        want = gru(h, x)
    monkeypatch.setenv("ALO_RAFT_GRU", "split")
    for name in ("conv_taps_f32", "gru_gate_rows_", "gru_update_rows_", "gru_gate_", "gru_update_"):
        monkeypatch.setattr(alo_hip, name, refuse)
    with torch.no_grad():
        got = gru(h, x)
    assert torch.equal(got, want)
    assert gru(h, x).requires_grad                                             # grad mode: the stock ops as well
