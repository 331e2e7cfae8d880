"""linear_shortk_kernel at K = 64 and 128 requests the identity of a tile AHEAD of its product (fetch_identity of mfma_tile.hpp); at
K = 256, and in linear_packed_kernel, the identity is loaded in the epilogue (docs/experiments.md, "Residual GEMMs").  Both forms are
held to the same statement.

What can go wrong is an identity that belongs to another tile or to other rows, so every case here is exact:

    y0  = wrapper(x, W, b, relu=False, residual=None)               (the staged, bf16-rounded product)
    out = wrapper(x, W, b, relu, residual=res)  ==  bf16(act(float(y0) + float(res)))        bit for bit (torch.equal),

with ``res`` distinct in every row (checked), over one tile, ragged tiles and, per (K, N), one M at which a persistent workgroup of
linear_shortk_kernel walks more than two tiles: M = 64 * (2 * gx) + 37 with gx = 512 / ceil(N / 256) workgroups along the rows
(launch_shortk).  linear_packed_kernel is not persistent: launch_packed starts ceil(M / rows) workgroups along the rows, rows = 64
(N % 256 == 0) or 128, each of which computes ONE tile, so no M gives a workgroup a second tile; its long case has more than two row
tiles in the grid and a ragged last one.
"""
import pytest
import torch

import alo_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def shortk_long_m(n):
    """gemm.hip launch_shortk: gx = 512 / ceil(N / 256) workgroups walk ceil(M / 64) tiles; more than two tiles each, ragged end."""
    return 64 * (2 * (512 // -(-n // 256))) + 37


def packed_rows(n):
    """gemm_packed.hip launch_packed: rows per workgroup (one tile each), grid.x = ceil(M / rows)."""
    return 64 if n % 256 == 0 else 128


def packed_long_m(n):
    return 3 * packed_rows(n) + 37


def make_case(m, k, n, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(m, k, device=DEV, generator=g).to(dtype)
    w = (torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).to(dtype)
    b = (0.5 * torch.randn(n, device=DEV, generator=g)).to(dtype)
    res = torch.randn(m, n, device=DEV, generator=g).to(dtype)
    # distinct in every row: an identity taken from another row or tile cannot go unseen
    key = res.double() @ torch.randn(n, device=DEV, generator=g, dtype=torch.float64)
    assert torch.unique(key).numel() == m
    return x, w, b, res


def expected(y0, res, relu):
    s = y0.float() + res.float()
    return (torch.relu(s) if relu else s).to(y0.dtype)   # torch's relu keeps NaN, as the kernels' does


def check_exact(fn, m, k, n, relu, dtype=torch.bfloat16):
    x, w, b, res = make_case(m, k, n, dtype, m + 3 * k + 7 * n)
    with torch.no_grad():
        y0 = fn(x, w, b, False, residual=None)
        got = fn(x, w, b, relu, residual=res)
    ref = expected(y0, res, relu)
    assert got.shape == ref.shape == (m, n)
    if not torch.equal(got, ref):
        bad = (got != ref).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{fn.__name__} M={m} K={k} N={n} relu={relu} {dtype}: {bad.numel()} rows differ, first {bad[:8].tolist()}")


SHORTK_KN = [(64, 256), (128, 512), (256, 1024), (256, 256)]
SHORTK_CASES = [(m, k, n, True) for k, n in SHORTK_KN for m in (1, 63, 64, 65, 200, shortk_long_m(n))]
SHORTK_CASES += [(m, k, n, False) for k, n in SHORTK_KN for m in (65, shortk_long_m(n))]


@pytest.mark.parametrize("m,k,n,relu", SHORTK_CASES)
def test_linear_shortk_identity_is_exact(m, k, n, relu):
    check_exact(alo_hip.linear_shortk, m, k, n, relu)


def test_shortk_long_cases_walk_more_than_two_tiles():
    for _, n in SHORTK_KN:
        gx = 512 // -(-n // 256)
        assert -(-shortk_long_m(n) // 64) > 2 * gx


@pytest.mark.parametrize("m", [65, shortk_long_m(256)])
@pytest.mark.parametrize("relu", [True, False])
def test_linear_shortk_identity_is_exact_fp16(m, relu):
    check_exact(alo_hip.linear_shortk, m, 64, 256, relu, torch.float16)


PACKED_KN = [(512, 2048), (512, 128)]


@pytest.mark.parametrize("k,n", PACKED_KN)
@pytest.mark.parametrize("m_kind", ["1", "65", "long"])
@pytest.mark.parametrize("relu", [True, False])
def test_linear_packed_identity_is_exact(k, n, m_kind, relu):
    m = packed_long_m(n) if m_kind == "long" else int(m_kind)
    if m_kind == "long":
        assert -(-m // packed_rows(n)) > 2
    check_exact(alo_hip.linear_packed, m, k, n, relu)


def test_linear_packed_identity_is_exact_fp16():
    check_exact(alo_hip.linear_packed, packed_long_m(2048), 512, 2048, True, torch.float16)


def _nan_stays_in_its_row(fn, m, k, n, row):
    """NaN over the 64 columns of wave 1 in ONE row of the identity: exactly those outputs are NaN (ReLU keeps NaN), every other
    element is what the run without the NaN gives."""
    x, w, b, res = make_case(m, k, n, torch.bfloat16, 11 * m + n)
    dirty = res.clone()
    dirty[row, 64:128] = NAN
    with torch.no_grad():
        clean_out = fn(x, w, b, True, residual=res)
        got = fn(x, w, b, True, residual=dirty)
    assert not torch.isnan(clean_out).any()
    planted = torch.isnan(dirty)
    assert int(planted.sum()) == 64
    assert torch.equal(torch.isnan(got), planted)
    assert torch.equal(torch.where(planted, torch.zeros_like(got), got), torch.where(planted, torch.zeros_like(got), clean_out))


@pytest.mark.parametrize("k,n", SHORTK_KN)
def test_linear_shortk_nan_in_the_identity_stays_in_its_row(k, n):
    m = shortk_long_m(n)
    gx = 512 // -(-n // 256)
    # the middle tile of a workgroup that walks three: workgroup 5's tiles are 5, 5 + gx, 5 + 2 gx
    _nan_stays_in_its_row(alo_hip.linear_shortk, m, k, n, 64 * (5 + gx) + 21)


@pytest.mark.parametrize("k,n", PACKED_KN)
def test_linear_packed_nan_in_the_identity_stays_in_its_row(k, n):
    m = packed_long_m(n)
    _nan_stays_in_its_row(alo_hip.linear_packed, m, k, n, packed_rows(n) + 21)   # the second of the four row tiles


@pytest.mark.parametrize("relu", [True, False])
def test_conv1x1_nhwc_with_identity_equals_linear_shortk(relu):
    """alo_conv1x1_nhwc at stride 1 with an identity (no wrapper passes one): the same kernel as alo_linear_shortk on the flattened rows."""
    nb, h, w_, cin, cout = 2, 5, 7, 64, 256
    x, wt, b, res = make_case(nb * h * w_, cin, cout, torch.bfloat16, 5)
    y = torch.empty(nb * h * w_, cout, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        alo_hip._launch("alo_conv1x1_nhwc", x.device, None, 0.0, 0.0, x, wt, 0, b, res, y, nb, h, w_, cin, cout, 1, 1 if relu else 0,
                        alo_hip.ALO_BF16)
        ref = alo_hip.linear_shortk(x, wt, b, relu, residual=res)
    assert torch.equal(y, ref)


def test_resnet_body_identity_in_the_epilogue_vs_bias_act(monkeypatch):
    """Routing: every stage of the bf16 backbone with the identity in the GEMM epilogues against the same network with each
    bottleneck's last convolution run residual-free and the identity applied by alo_bias_act afterwards (zero bias: the folded
    batch-norm shift stays inside the GEMM, so both routes round at the same points).  Held to one bf16 rounding of the result,
    2^-8 |ref|, the first term of the bound test_backbone_kernels_gpu.py gives every backbone kernel."""
    import alonet.detr.backbone as bb

    torch.manual_seed(0)
    body = bb.ResNetBody("resnet50", return_layers={"layer1": "0", "layer2": "1", "layer3": "2", "layer4": "3"}).to(DEV).eval()
    for m in body.modules():  # non-trivial frozen statistics
        if hasattr(m, "running_var"):
            m.running_var.uniform_(0.5, 2.0); m.running_mean.normal_(0, 0.2); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    body = body.to(torch.bfloat16)
    x = torch.randn(2, 3, 64, 96, device=DEV).to(torch.bfloat16)
    with alo_hip.LaunchTimer() as t, torch.no_grad():
        fused = body(x)
    tags = set(t.summary())
    assert {"linear_shortk/N=256,K=64", "linear_shortk/N=512,K=128", "linear_shortk/N=1024,K=256", "linear_packed/K=512/N=2048"} <= tags
    assert not any(k.startswith("bias_act") for k in tags)

    conv_bn = bb.conv_bn
    applied = []

    def split_conv_bn(x, conv, bn, relu=False, residual=None):
        if residual is None:
            return conv_bn(x, conv, bn, relu=relu)
        out = conv_bn(x, conv, bn, relu=False)
        applied.append(out.shape[1])
        return alo_hip.bias_act_(out, torch.zeros(out.shape[1], device=out.device, dtype=out.dtype), residual, relu)

    monkeypatch.setattr(bb, "conv_bn", split_conv_bn)
    with torch.no_grad():
        split = body(x)
    assert applied == [256] * 3 + [512] * 4 + [1024] * 6 + [2048] * 3
    assert fused.keys() == split.keys() and len(fused) == 4
    for k in fused:
        a, r = fused[k].float(), split[k].float()
        assert a.shape == r.shape and bool(torch.isfinite(r).all())
        excess = ((a - r).abs() - 2.0 ** -8 * r.abs()).max().item()
        assert excess <= 0.0, (k, excess)
