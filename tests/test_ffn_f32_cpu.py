"""alo_ffn256 with dtype = ALO_F32 (aloception-oss_amd/csrc/ffn_f32.hip), as far as it can be checked without a GPU: the kernel's
arithmetic restated in numpy (ffn_f32_ref.py) meets the fp64 block within the bound derived there at every shape and input magnitude
the GPU test uses; the C ABI's argument checks; the gate; and the feed-forward block of the transformer stays off the kernel unless
the switch is set and the operands are fp32."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alo_hip
from alonet.deformable_detr import deformable_transformer
from ffn_f32_ref import SCALES, SHAPES, dim_rows, ffn_split, operands, reference_and_bound
from kernel_bounds import INF, NAN, compare

KNOB = "ALO_F32_LAYERS"
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _restated(x, w1, b1, w2, b2):
    np_ = lambda a: None if a is None else a.numpy()  # noqa: E731
    return torch.from_numpy(ffn_split(np_(x), np_(w1), np_(b1), np_(w2), np_(b2)))


def _check(shape, scale, bias):
    x, w1, b1, w2, b2 = operands(shape, scale)
    b1, b2 = (b1, b2) if bias else (None, None)
    ref, bound = reference_and_bound(x, w1, b1, w2, b2)
    ratio = compare(_restated(x, w1, b1, w2, b2), ref, bound, f"split ffn {shape} scale={scale} bias={bias}")
    print(f"{shape} scale={scale} bias={bias}: worst |err| / bound = {ratio:.3f}")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_restated_arithmetic_meets_the_bound(shape, scale):
    _check(shape, scale, True)
    if shape[0] <= 200:
        _check(shape, scale, False)


def test_restated_arithmetic_on_a_dim_row_a_dim_chunk_and_a_zero_row():
    x, w1, b1, w2, b2 = dim_rows()
    x[7] = 0
    got = _restated(x, w1, b1, w2, b2)
    ref, bound = reference_and_bound(x, w1, b1, w2, b2)
    compare(got, ref, bound, "dim row / dim chunk / zero row")
    # a row does not depend on its neighbours: they change, it keeps its bits (the same number of rows, so that the BLAS behind numpy
    # adds in the same order; the kernel is held to the bits of a call with M = 1 on the GPU)
    rows = [3, 7, 70]
    others = x * 1e3
    others[rows] = x[rows]
    assert torch.equal(_restated(others, w1, b1, w2, b2)[rows], got[rows])
    # without biases the zero row's hidden activation is zero and so is its output, whatever the other rows hold
    assert torch.equal(_restated(x, w1, None, w2, None)[7], torch.zeros(256))


def test_restated_arithmetic_with_non_finite_inputs():
    x, w1, b1, w2, b2 = operands((65, 256))
    x = x.clone()
    x[2, 5], x[40, 77], x[11] = INF, -INF, NAN
    got = _restated(x, w1, b1, w2, b2)
    ref, bound = reference_and_bound(x, w1, b1, w2, b2)
    compare(got, ref, bound, "non-finite inputs")
    spoiled = torch.zeros(65, dtype=torch.bool)
    spoiled[[2, 40, 11]] = True
    assert torch.isfinite(got[~spoiled]).all() and not torch.isfinite(got[spoiled]).any() and torch.isnan(got[11]).all()
    clean = _restated(operands((65, 256))[0], w1, b1, w2, b2)
    assert torch.equal(got[~spoiled], clean[~spoiled])


# ---- the C ABI: validation happens before anything is enqueued, so every call here carries one bad argument and never launches ----
ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
FFN_BAD = {   # name -> (x, w1, b1, w2, b2, y, M, F), what the message names, the status
    "F": ((ONE, ONE, ONE, ONE, ONE, ONE, 8, 300), b"multiple of 256 (M=8 F=300)", 1),
    "w2": ((ONE, ONE, ONE, ODD, ONE, ONE, 8, 256), b"16-byte aligned", 1),
    "y": ((ONE, ONE, ONE, ONE, ONE, None, 8, 256), b"null pointer", 1),
    "b1": ((ONE, ONE, ODD, ONE, ONE, ONE, 8, 256), b"16-byte aligned", 1),
    "b2": ((ONE, ONE, None, ONE, ODD, ONE, 8, 256), b"16-byte aligned", 1),
    "M": ((ONE, ONE, ONE, ONE, ONE, ONE, 0, 256), b"M must be positive", 1),
    "LDS": ((ONE, ONE, ONE, ONE, ONE, ONE, 8, alo_hip.FFN_F32_MAX_HIDDEN + 256), b"bytes of LDS", 2),
}


@pytest.mark.parametrize("name", sorted(FFN_BAD))
def test_fp32_call_is_refused_for_the_bad_argument_and_not_for_its_dtype(name):
    lib = alo_hip.lib()
    args, names, status = FFN_BAD[name]
    rc = lib.alo_ffn256(*args, alo_hip.ALO_F32, None)
    message = lib.alo_last_error()
    assert rc == status and names in message and message.startswith(b"alo_ffn256:"), (name, rc, message)
    assert b"dtype" not in message and b"bf16" not in message, message
    if name in ("F", "w2", "y", "M"):    # the checks and the messages of a bf16 call
        assert lib.alo_ffn256(*args, alo_hip.ALO_BF16, None) == status and lib.alo_last_error() == message


def test_fp64_is_still_refused_for_its_dtype():
    lib = alo_hip.lib()
    for code in (alo_hip.ALO_F64, 7):
        rc = lib.alo_ffn256(ONE, ONE, ONE, ODD, ONE, ONE, 8, 300, code, None)
        message = lib.alo_last_error()
        assert rc == 2 and b"dtype %d" % code in message and b"aligned" not in message and b"multiple" not in message, message


def test_abi_version_and_signatures_are_unchanged():
    assert alo_hip.lib().alo_abi_version() == 3
    assert not any("f32" in name for name in alo_hip._SIGNATURES)      # the fp32 flavour rides alo_ffn256 (test_cabi.py pins the set)
    assert "alo_ffn256" in alo_hip._SIGNATURES


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
class _Tensor:
    """What ffn_f32_supported asks of a tensor, for devices this machine does not have."""

    def __init__(self, *shape, dtype=torch.float32, cuda=True, requires_grad=False):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, cuda, requires_grad

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))


def test_supported_gate_truth_table():
    ok = alo_hip.ffn_f32_supported
    x, w1, w2 = _Tensor(5, 7, 256), _Tensor(1024, 256), _Tensor(256, 1024)
    bf = torch.bfloat16
    top = alo_hip.FFN_F32_MAX_HIDDEN
    with torch.no_grad():
        assert ok(x, w1, w2) and ok(_Tensor(256), w1, w2) and ok(_Tensor(0, 256), w1, w2)
        assert not ok(_Tensor(5, 7, 256, cuda=False), w1, w2)
        assert not ok(_Tensor(5, 7, 256, dtype=bf), _Tensor(1024, 256, dtype=bf), _Tensor(256, 1024, dtype=bf))
        assert not ok(x, _Tensor(1024, 256, dtype=bf), w2) and not ok(x, w1, _Tensor(256, 1024, dtype=torch.float16))
        assert not ok(_Tensor(5, 7, 256, dtype=torch.float64), w1, w2)
        assert not ok(_Tensor(5, 7, 128), _Tensor(1024, 128), _Tensor(128, 1024))                  # d_model = 256 only
        assert not ok(x, _Tensor(1000, 256), _Tensor(256, 1000))                                  # F % 256
        assert not ok(x, w1, _Tensor(256, 512)) and not ok(x, w1, _Tensor(1024, 256))             # w2 is (256, F)
        assert not ok(x, _Tensor(1024 * 256), w2) and not ok(x, _Tensor(0, 256), _Tensor(256, 0))
        assert top % 256 == 0 and ok(x, _Tensor(top, 256), _Tensor(256, top))                     # the kernel's LDS frame
        assert not ok(x, _Tensor(top + 256, 256), _Tensor(256, top + 256))
        assert ok(x, _Tensor(1024, 256, requires_grad=True), w2)                                  # grad mode off: nothing is recorded
    assert ok(x, w1, w2)                                                                          # grad mode on, nothing requires grad
    assert not ok(x, _Tensor(1024, 256, requires_grad=True), w2) and not ok(x, w1, _Tensor(256, 1024, requires_grad=True))
    assert not ok(_Tensor(5, 7, 256, requires_grad=True), w1, w2)
    real = torch.randn(4, 256)
    with pytest.raises(RuntimeError, match="ffn_f32: needs"):
        alo_hip.ffn_f32(real, torch.randn(256, 256), None, torch.randn(256, 256), None)
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.ffn_f32(real, torch.randn(256, 256), torch.randn(256).requires_grad_(), torch.randn(256, 256), None)


def test_the_route_needs_the_switch_fp32_operands_and_a_measured_shape(monkeypatch):
    routed = alo_hip.ffn_f32_routed
    x, w1, w2 = _Tensor(2, 50, 256), _Tensor(1024, 256), _Tensor(256, 1024)
    bf = torch.bfloat16
    half = (_Tensor(2, 50, 256, dtype=bf), _Tensor(1024, 256, dtype=bf), _Tensor(256, 1024, dtype=bf))
    with torch.no_grad():
        monkeypatch.setattr(alo_hip, "_FFN_F32_ROUTED", {1024: (0, None)})
        for value in (None, "1"):
            monkeypatch.delenv(KNOB, raising=False)
            if value is not None:
                monkeypatch.setenv(KNOB, value)
            assert not routed(x, w1, w2)
        monkeypatch.setenv(KNOB, "split")
        assert routed(x, w1, w2) and not routed(*half)
        assert not routed(x, _Tensor(2048, 256), _Tensor(256, 2048))                              # an F that was not measured
        monkeypatch.setattr(alo_hip, "_FFN_F32_ROUTED", {1024: (128, 4096)})
        assert not routed(x, w1, w2) and routed(_Tensor(128, 256), w1, w2) and not routed(_Tensor(4096, 256), w1, w2)
        monkeypatch.setattr(alo_hip, "_FFN_F32_ROUTED", {})
        assert not routed(x, w1, w2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ffn_block_never_reaches_the_kernel_on_the_cpu_or_in_bf16(monkeypatch, dtype):
    def never(*a, **k):
        raise AssertionError("_ffn reached alo_hip.ffn_f32")

    monkeypatch.setattr(alo_hip, "ffn_f32", never)
    monkeypatch.setattr(alo_hip, "_FFN_F32_ROUTED", {512: (0, None)})
    torch.manual_seed(3)
    l1, l2 = torch.nn.Linear(256, 512).to(dtype), torch.nn.Linear(512, 256).to(dtype)
    x = torch.randn(9, 256).to(dtype)
    out = {}
    for value in (None, "split"):
        monkeypatch.delenv(KNOB, raising=False)
        if value is not None:
            monkeypatch.setenv(KNOB, value)
        with torch.no_grad():
            out[value] = deformable_transformer._ffn(l1, F.relu, l2, x)
    assert torch.equal(out[None], out["split"])
