"""The fp32 InstanceNorm flavour of alo_groupnorm_rows_act (dtype = ALO_F32, groups == C, no affine;
aloception-oss_amd/csrc/instancenorm_f32.hip) as far as it can be checked without a GPU: the kernel's arithmetic restated in torch
(instancenorm_f32_ref.py) meets fp64 ``F.instance_norm`` within 4 x the stock fp32 op's own error + 3e-7 max|ref| (the factor and
floor of test_split_numerics.py) on ill-conditioned channels, and the C ABI checks an fp32 call before anything is enqueued."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

import alo_hip
import kernel_bounds as kb
from instancenorm_f32_ref import chunk_moments, instancenorm_rows, merged_moments, reference_and_bar

# (N, C, HW): one row, a partial chunk, a chunk boundary either side, several chunks with a ragged tail, more chunks than stripes
SHAPES = [(3, 64, 1), (2, 64, 63), (2, 128, 255), (2, 128, 257), (2, 64, 37 * 29), (1, 256, 4 * 256 + 5), (1, 64, 70 * 256 + 3)]


def ill_inputs(n, c, hw, seed, device="cpu"):
    """kernel_bounds.groupnorm_ill_inputs with groups = C, widened to fp32: channels cycle through mean / std = 0.25, 16, 100 and a
    constant channel.  (N, C, HW) fp32."""
    return kb.groupnorm_ill_inputs(n, c, hw, c, device, seed).float()


def _rows(x):
    return x.transpose(1, 2).contiguous()       # (N, HW, C): the kernel's layout


@pytest.mark.parametrize("n,c,hw", SHAPES)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_restated_arithmetic_meets_the_bar_on_ill_conditioned_channels(n, c, hw, relu):
    x = ill_inputs(n, c, hw, seed=c + hw)
    ref, bar, e_stock = reference_and_bar(x, relu=relu)
    got = instancenorm_rows(_rows(x), 1e-5, relu).transpose(1, 2).double()
    err = (got - ref).abs().max().item()
    print(f"N={n} C={c} HW={hw} relu={relu}: restatement {err:.3g}  stock fp32 {e_stock:.3g}  bar {bar:.3g}")
    assert e_stock <= bar                        # the stock op alone stays inside the bar on these inputs
    assert err <= bar, (err, bar)
    if hw > 1:
        assert (got[:, 3::4] == 0).all()         # a constant channel: M2 is exactly 0 and so is every output


@pytest.mark.parametrize("n,c,hw", [(2, 64, 300), (1, 128, 700)])
def test_restated_arithmetic_on_ordinary_fp32_values(n, c, hw):
    """Values with all 24 bits in use (the inputs above are bf16 values widened), channel scales from 1e-3 to 1e3."""
    g = torch.Generator().manual_seed(hw)
    x = torch.randn(n, c, hw, generator=g) * torch.logspace(-3, 3, c).view(1, -1, 1) + torch.randn(1, c, 1, generator=g)
    ref, bar, e_stock = reference_and_bar(x)
    err = (instancenorm_rows(_rows(x)).transpose(1, 2).double() - ref).abs().max().item()
    print(f"N={n} C={c} HW={hw}: restatement {err:.3g}  stock fp32 {e_stock:.3g}  bar {bar:.3g}")
    assert err <= bar, (err, bar)


def test_restated_moments_are_the_channels_moments():
    x = ill_inputs(2, 64, 1000, seed=4)
    n, mean, m2 = merged_moments(chunk_moments(_rows(x)))
    assert (n == 1000).all()
    x64 = x.double()
    assert torch.allclose(mean.double(), x64.mean(2), rtol=1e-6, atol=1e-7)
    assert torch.allclose(m2.double() / 1000, x64.var(2, unbiased=False), rtol=1e-5, atol=1e-12)


def test_restated_non_finite_element_spoils_its_own_channel_only():
    x = ill_inputs(2, 64, 300, seed=9)
    clean = instancenorm_rows(_rows(x))
    for bad in (kb.NAN, kb.INF, -kb.INF):
        y = x.clone()
        y[1, 5, 77] = bad
        got = instancenorm_rows(_rows(y))
        assert not torch.isfinite(got[1, :, 5]).any()
        assert not torch.isfinite(F.instance_norm(y)[1, 5]).any()          # as torch makes it
        keep = torch.ones(2, 64, dtype=torch.bool)
        keep[1, 5] = False
        assert torch.equal(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])


# ---- the C ABI: validation happens before anything is enqueued, so every call here carries one bad argument and never launches ----
ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
F32, BF16 = alo_hip.ALO_F32, alo_hip.ALO_BF16


def _act(x=ONE, weight=None, bias=None, y=ONE, ws=ONE, B=2, HW=9, C=64, groups=64, stride=None, dtype=F32):
    lib = alo_hip.lib()
    rc = lib.alo_groupnorm_rows_act(x, weight, bias, y, ws, B, HW, C, groups, 1e-5, HW * C if stride is None else stride, 1, dtype, None)
    return rc, lib.alo_last_error()


BAD = {   # name -> keyword arguments of an otherwise acceptable call, what the message says, the status
    "misaligned x": (dict(x=ODD), b"16-byte aligned", 1),
    "misaligned y": (dict(y=ODD), b"16-byte aligned", 1),
    "null x": (dict(x=None), b"null pointer", 1),
    "missing workspace": (dict(ws=None), b"null pointer", 1),
    "HW = 0": (dict(HW=0, stride=64), b"sizes must be positive", 1),
    "short stride": (dict(stride=9 * 64 - 4), b"y_batch_stride", 1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_fp32_call_is_refused_for_the_bad_argument_with_the_bf16_calls_message(name):
    """Fails without the feature: an fp32 call is refused for its dtype ("bf16 only") whatever else it carries."""
    kwargs, names, status = BAD[name]
    rc, msg = _act(**kwargs)
    assert rc == status and names in msg and msg.startswith(b"alo_groupnorm_rows:"), (name, rc, msg)
    assert b"dtype" not in msg and b"bf16" not in msg and b"F32" not in msg, msg
    rc16, msg16 = _act(**{"weight": ONE, "bias": ONE, "groups": 8, **kwargs}, dtype=BF16)       # the bf16 call carries its affine
    assert (rc16, msg16) == (rc, msg)


def test_fp32_call_other_than_instancenorm_is_refused_by_rule():
    rc, msg = _act(groups=8)
    assert rc == 2 and b"groups == C" in msg, msg
    rc, msg = _act(C=96, groups=96)
    assert rc == 2 and b"multiple of 64" in msg, msg
    rc, msg = _act(C=320, groups=320)
    assert rc == 2 and b"up to 256" in msg, msg
    for kwargs in (dict(weight=ONE), dict(bias=ONE), dict(weight=ONE, bias=ONE)):
        rc, msg = _act(**kwargs)
        assert rc == 2 and b"without affine" in msg and b"NULL" in msg, msg
    lib = alo_hip.lib()
    for weight in (None, ONE):
        rc = lib.alo_groupnorm_rows(ONE, weight, weight, ONE, ONE, 2, 9, 64, 64, 1e-5, 9 * 64, F32, None)
        assert rc == 2 and b"alo_groupnorm_rows_act" in lib.alo_last_error(), lib.alo_last_error()


def test_the_dtype_is_checked_first_and_fp16_fp64_stay_refused():
    lib = alo_hip.lib()
    for dt in (alo_hip.ALO_F16, alo_hip.ALO_F64, 7):
        rc, msg = _act(x=None, HW=0, dtype=dt)                                                    # two more faults: the dtype is what is named
        assert rc == 2 and b"dtype" in msg and b"null" not in msg and b"positive" not in msg, msg
        rc = lib.alo_groupnorm_rows(ONE, ONE, ONE, ONE, ONE, 2, 9, 64, 8, 1e-5, 9 * 64, dt, None)
        assert rc == 2 and b"dtype" in lib.alo_last_error()


def test_bf16_calls_keep_their_checks():
    rc, msg = _act(weight=ONE, bias=ONE, C=64, groups=7, dtype=BF16)
    assert rc == 2 and b"needs C / 8 and groups to divide 256" in msg, msg
    rc, msg = _act(weight=None, bias=ONE, groups=8, dtype=BF16)                                   # a bf16 call needs its affine
    assert rc == 1 and b"null pointer" in msg, msg
    rc, msg = _act(weight=ONE, bias=ONE, groups=8, stride=9 * 64 + 4, dtype=BF16)                 # 8 bytes off a 16-byte boundary in bf16
    assert rc == 1 and b"y_batch_stride" in msg, msg
    rc, msg = _act(x=ODD, stride=9 * 64 + 4)                                                      # ... and 16 bytes on in fp32: the pointer check is next
    assert rc == 1 and b"pointers must be 16-byte aligned" in msg, msg


def test_workspace_answer_is_unchanged():
    lib = alo_hip.lib()
    for B, HW, C in ((8, 230400, 64), (3, 1, 64), (1, 1029, 256)):
        assert lib.alo_groupnorm_rows_workspace_bytes(B, HW, C) == B * ((HW + 255) // 256) * C * 12


def test_abi_version_and_entry_points_are_unchanged():
    assert alo_hip.lib().alo_abi_version() == 3
    declared = set()
    for name in ("alo_hotpath.h", "alo_corr_alt.h", "alo_two_stage.h", "alo_encoder_block.h"):
        text = open(alo_hip.CSRC_DIR + "/../../include/" + name).read()
        declared |= set(re.findall(r"^[a-z][\w \*]*?\b(alo_\w+)\s*\(", text, flags=re.M))
    assert declared == set(alo_hip._SIGNATURES), declared ^ set(alo_hip._SIGNATURES)
    assert not any("instancenorm" in name for name in alo_hip._SIGNATURES)


def test_wrapper_refuses_what_the_kernel_does_not_serve():
    x = torch.randn(1, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    assert not alo_hip.instancenorm_nhwc_f32_supported(x)                                         # a CPU tensor
    with pytest.raises(RuntimeError, match="instancenorm_nhwc_f32: needs"):
        alo_hip.instancenorm_nhwc_f32(x)
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.instancenorm_nhwc_f32(x.requires_grad_())
