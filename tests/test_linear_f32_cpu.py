"""alo_linear_packed / alo_conv1x1_nhwc with dtype = ALO_F32 (aloception-oss_amd/csrc/gemm_f32.hip), as far as they can be checked
without a GPU: the kernel's arithmetic restated in numpy (linear_f32_ref.py) meets the fp64 product within the bound derived there
at every shape and input magnitude the GPU test uses; the split-weight layout; the gate; the C ABI's argument checks; and the
``ALO_F32_LAYERS`` switch leaves CPU and bf16 calls alone."""
import ctypes

import numpy as np
import pytest
import torch

import alo_hip
from kernel_bounds import INF, NAN, compare
from linear_f32_ref import SCALES, SHAPES, linear_split, operands, reference_and_bound, split_weight

KNOB = "ALO_F32_LAYERS"


def _check(shape, scale, bias, residual, relu):
    x, w, b, res = operands(shape, scale)
    b, res = (b if bias else None), (res if residual else None)
    got = torch.from_numpy(linear_split(x.numpy(), w.numpy(), None if b is None else b.numpy(), None if res is None else res.numpy(), relu))
    ref, bound = reference_and_bound(x, w, b, res, relu)
    ratio = compare(got, ref, bound, f"split linear {shape} scale={scale} bias={bias} res={residual} relu={relu}")
    print(f"{shape} scale={scale} bias={bias} res={residual} relu={relu}: worst |err| / bound = {ratio:.3f}")
    return got


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_arithmetic_meets_the_bound(shape, scale):
    _check(shape, scale, True, True, True)
    if shape[0] <= 200:
        _check(shape, scale, False, False, False)
        _check(shape, scale, True, False, True)
        _check(shape, scale, False, True, False)


def test_restated_arithmetic_on_a_dim_row_a_zero_row_and_a_tiny_channel():
    x, w, b, res = operands((65, 128, 64))
    x, w, b = x.clone(), w.clone(), b.clone()
    x[3] *= 1e-6
    x[7] = 0
    x[:, :5] *= 1e-6
    w[9] *= 1e-6
    b[9] *= 1e-6
    got = torch.from_numpy(linear_split(x.numpy(), w.numpy(), b.numpy(), None, False))
    ref, bound = reference_and_bound(x, w, b, None, False)
    compare(got, ref, bound, "dim row / zero row / tiny channel")
    assert torch.equal(got[7], b)                                                            # the all-zero row
    alone = linear_split(x[3:4].numpy(), w.numpy(), b.numpy(), None, False)
    assert np.array_equal(alone[0], got[3].numpy())                                          # a row does not depend on its neighbours


@pytest.mark.parametrize("relu", [False, True])
def test_restated_arithmetic_with_non_finite_inputs(relu):
    x, w, b, res = operands((65, 128, 64))
    x = x.clone()
    x[2, 5], x[40, 77], x[11] = INF, -INF, NAN
    got = torch.from_numpy(linear_split(x.numpy(), w.numpy(), b.numpy(), res.numpy(), relu))
    ref, bound = reference_and_bound(x, w, b, res, relu)
    compare(got, ref, bound, f"non-finite inputs relu={relu}")
    spoiled = torch.zeros(65, dtype=torch.bool)
    spoiled[[2, 40, 11]] = True
    assert torch.isfinite(got[~spoiled]).all() and torch.isnan(got[11]).all()
    assert torch.isfinite(got[spoiled]).logical_not().all() if not relu else True


# ---- the split-weight layout ------------------------------------------------------------------------------------------------------
def pack_mfma_b(w):
    """alo_pack_mfma_b in torch: (N, K) -> [N / 32][K / 16][64][8], lane = 32 kg + n holding w[32 t + n][16 s + 8 kg .. + 8]."""
    n, k = w.shape
    return w.reshape(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(n, k)


def numpy_split_packed(w):
    """The bytes of alo_hip._split_weight(w) from linear_f32_ref.split_weight and :func:`pack_mfma_b`."""
    hi, lo, k = split_weight(w.numpy())
    parts = [pack_mfma_b(torch.from_numpy(hi).half()), pack_mfma_b(torch.from_numpy(lo).half()), torch.from_numpy(k)]
    return torch.cat([p.contiguous().view(torch.uint8).flatten() for p in parts])


def test_split_weight_layout_is_the_numpy_split_packed(monkeypatch):
    monkeypatch.setattr(alo_hip, "_pack_mfma_b", pack_mfma_b)     # the pack kernel itself is held to this order on the GPU
    _, w, _, _ = operands((1, 128, 192))
    w = w.clone()
    w[5] *= 1e-6
    w[6] = 0
    got = alo_hip._split_weight(w)
    assert got.dtype == torch.uint8 and got.numel() == 2 * 2 * w.numel() + 4 * w.shape[0]
    assert torch.equal(got, numpy_split_packed(w))
    # a (Cout, Cin, 3, 3) weight is the same helper on the (Cout, 9 Cin) matrix conv3x3 lays out
    w4 = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(3))
    assert torch.equal(alo_hip._split_weight(w4), numpy_split_packed(w4.permute(0, 2, 3, 1).reshape(64, -1)))


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
class _Tensor:
    """What linear_f32_supported asks of a tensor, for devices this machine does not have."""

    def __init__(self, *shape, dtype=torch.float32, cuda=True, requires_grad=False):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, cuda, requires_grad

    def dim(self):
        return len(self.shape)


def test_supported_gate_truth_table():
    ok = alo_hip.linear_f32_supported
    x, w = _Tensor(5, 7, 128), _Tensor(192, 128)
    with torch.no_grad():
        assert ok(x, w) and ok(_Tensor(128), w) and ok(_Tensor(0, 128), w)
        assert not ok(_Tensor(5, 7, 128, cuda=False), w)
        assert not ok(_Tensor(5, 7, 128, dtype=torch.bfloat16), _Tensor(192, 128, dtype=torch.bfloat16))
        assert not ok(_Tensor(5, 7, 128, dtype=torch.float16), _Tensor(192, 128, dtype=torch.float16))
        assert not ok(x, _Tensor(192, 128, dtype=torch.bfloat16)) and not ok(_Tensor(5, 7, 128, dtype=torch.float64), w)
        assert not ok(_Tensor(5, 7, 96), _Tensor(192, 96)) and not ok(x, _Tensor(100, 128))      # K % 64, N % 64
        assert not ok(_Tensor(5, 7, 64), w)                                                       # K of x and of the weight differ
        assert not ok(x, _Tensor(192, 128, 1, 1)) and not ok(x, _Tensor(192 * 128))               # weight.dim() == 2
        assert ok(x, _Tensor(192, 128, requires_grad=True))                                       # grad mode off: nothing is recorded
    assert ok(x, w)                                                                               # grad mode on, nothing requires grad
    assert not ok(x, _Tensor(192, 128, requires_grad=True)) and not ok(_Tensor(5, 7, 128, requires_grad=True), w)
    real = torch.randn(4, 64)
    assert not ok(real, torch.randn(64, 64))                                                      # a CPU tensor
    with pytest.raises(RuntimeError, match="linear_f32: needs"):
        alo_hip.linear_f32(real, torch.randn(64, 64))
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.linear_f32(real, torch.randn(64, 64).requires_grad_())
    with pytest.raises(RuntimeError, match="conv1x1_strided_f32: needs"):
        alo_hip.conv1x1_strided_f32(torch.randn(1, 64, 4, 4), torch.randn(64, 64), None, 2)


# ---- the C ABI: validation happens before anything is enqueued, so every call here carries one bad argument and never launches ----
ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
F32 = alo_hip.ALO_F32
LINEAR_BAD = {   # name -> (x, w_packed, bias, residual, y, M, N, K, relu), what the message names, the status
    "K": ((ONE, ONE, ONE, None, ONE, 8, 128, 100, 0), b"multiples of 64 (K=100 N=128)", 2),
    "N": ((ONE, ONE, ONE, None, ONE, 8, 96, 128, 0), b"multiples of 64 (K=128 N=96)", 2),
    "pointer": ((ODD, ONE, ONE, None, ONE, 8, 128, 128, 0), b"16-byte aligned", 1),
    "residual": ((ONE, ONE, ONE, ODD, ONE, 8, 128, 128, 0), b"16-byte aligned", 1),
    "null": ((ONE, None, ONE, None, ONE, 8, 128, 128, 0), b"null pointer", 1),
    "size": ((ONE, ONE, ONE, None, ONE, 0, 128, 128, 0), b"must be positive", 1),
}
CONV_BAD = {     # name -> (x, weight, weight_is_packed, bias, residual, y, N, H, W, Cin, Cout, stride, relu), ...
    "unpacked": ((ONE, ONE, 0, ONE, None, ONE, 1, 4, 4, 64, 64, 2, 0), b"split packed weight", 2),
    "Cin": ((ONE, ONE, 1, ONE, None, ONE, 1, 4, 4, 100, 64, 2, 0), b"multiples of 64 (Cin=100 Cout=64)", 2),
    "Cout": ((ONE, ONE, 1, ONE, None, ONE, 1, 4, 4, 64, 96, 2, 0), b"multiples of 64 (Cin=64 Cout=96)", 2),
    "pointer": ((ONE, ONE, 1, ONE, None, ODD, 1, 4, 4, 64, 64, 2, 0), b"16-byte aligned", 1),
    "null": ((None, ONE, 1, ONE, None, ONE, 1, 4, 4, 64, 64, 2, 0), b"null pointer", 1),
    "size": ((ONE, ONE, 1, ONE, None, ONE, 1, 0, 4, 64, 64, 2, 0), b"must be positive", 1),
}


@pytest.mark.parametrize("name", sorted(LINEAR_BAD))
def test_fp32_linear_call_is_refused_for_the_bad_argument_and_not_for_its_dtype(name):
    lib = alo_hip.lib()
    args, names, status = LINEAR_BAD[name]
    rc = lib.alo_linear_packed(*args, F32, None)
    message = lib.alo_last_error()
    assert rc == status and names in message and message.startswith(b"alo_linear_packed:"), (name, rc, message)
    assert b"dtype" not in message and b"bf16" not in message, message


@pytest.mark.parametrize("name", sorted(CONV_BAD))
def test_fp32_conv1x1_call_is_refused_for_the_bad_argument_and_not_for_its_dtype(name):
    lib = alo_hip.lib()
    args, names, status = CONV_BAD[name]
    rc = lib.alo_conv1x1_nhwc(*args, F32, None)
    message = lib.alo_last_error()
    assert rc == status and names in message and message.startswith(b"alo_conv1x1_nhwc:"), (name, rc, message)
    assert b"dtype" not in message and b"bf16" not in message, message


def test_other_dtypes_are_refused_as_before():
    lib = alo_hip.lib()
    rc = lib.alo_linear_packed(ONE, ONE, ONE, None, ONE, 8, 128, 100, 0, alo_hip.ALO_F64, None)
    assert rc == 2 and b"dtype" in lib.alo_last_error() and b"multiple" not in lib.alo_last_error(), lib.alo_last_error()
    for dt in (alo_hip.ALO_F16, alo_hip.ALO_F64):
        rc = lib.alo_conv1x1_nhwc(ONE, ONE, 1, ONE, None, ONE, 1, 4, 4, 64, 64, 1, 0, dt, None)
        assert rc == 2 and b"bf16 only" in lib.alo_last_error() and b"dtype" in lib.alo_last_error(), lib.alo_last_error()
    for dt in (alo_hip.ALO_BF16, alo_hip.ALO_F16):      # a 16-bit call keeps its own shape rule and message
        rc = lib.alo_linear_packed(ONE, ONE, ONE, None, ONE, 8, 128, 192, 0, dt, None)
        assert rc == 2 and lib.alo_last_error() == b"alo_linear_packed: K must be a multiple of 256 and N of 128 (K=192 N=128)"
    rc = lib.alo_conv1x1_nhwc(ONE, ONE, 1, ONE, None, ONE, 1, 4, 4, 192, 128, 1, 0, alo_hip.ALO_BF16, None)
    assert rc == 2 and b"packed weights need Cin % 256 == 0 and Cout % 128 == 0 (Cin=192 Cout=128)" in lib.alo_last_error()


def test_abi_version_and_signatures_are_unchanged():
    assert alo_hip.lib().alo_abi_version() == 3
    assert not any("f32" in name for name in alo_hip._SIGNATURES)      # the fp32 flavours ride existing entry points (test_cabi.py pins the set)


# ---- the switch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_switch_leaves_cpu_and_bf16_calls_alone(monkeypatch, dtype):
    g = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(9, 128, generator=g).to(dtype), torch.randn(64, 128, generator=g).to(dtype), torch.randn(64, generator=g).to(dtype))
    res = torch.randn(9, 64, generator=g).to(dtype)
    out = {}
    for value in (None, "split", "1"):
        monkeypatch.delenv(KNOB, raising=False)
        if value is not None:
            monkeypatch.setenv(KNOB, value)
        assert alo_hip.f32_layers_split() == (value == "split")
        with torch.no_grad():
            out[value] = (alo_hip.linear_auto(x, w, b, relu=True), alo_hip.linear_auto(x, w, None, residual=res))
    for value in ("split", "1"):
        assert all(torch.equal(a, b_) for a, b_ in zip(out[value], out[None]))
