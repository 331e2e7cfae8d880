"""The backbone's persistent-workgroup kernels at the launch sizes the headline runs, against fp64 references.

conv3x3_kernel, stem_conv_pool_kernel and linear_shortk_kernel walk a second tile only when the launch has more tiles than
resident workgroups; the cases here take that loop (next-tile prefetch across tile and image boundaries, uneven per-XCD ranges),
the K-split and split-K routes and the idle-wave column blocks, and plant NaN / +Inf to pin down what the fused ReLUs do with
non-finite values (they keep NaN, as torch's relu does).

Every reference is computed in fp64 from the kernel's own bf16 operands (bf16 -> fp64 is exact) with plain torch ops (unfold +
matmul, max_pool2d), and every output element is held to

    |got - ref| <= 2^-8 |ref| + c(K) * A,        c(K) = (K + 1) * 2^-23,

where A is the same operation applied to |x|, |w| and |b| (fp64, no activation).  2^-8 |ref| covers the one rounding of the result
to bf16 (half an ulp: at most 2^-8 relative, bf16 carrying 8 significant bits).  c(K) * A covers the fp32 accumulation: a sum of the
K products and the bias, in ANY order and grouping (MFMA k-steps, the two K-split waves, the split-K partial sums and their
finalize), is off by at most gamma_(K+1) * sum|terms| ~= (K + 1) * 2^-24 * A (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Sec. 3.1; bf16 x bf16 products are exact in fp32); the factor 2 covers the second-order terms and the bf16
rounding of that error itself.  The residual epilogues round x W^T + b to bf16 BEFORE adding the identity; that rounding adds
2^-8 |x W^T + b| to the bound.  Non-finite inputs are replaced by 0 in A (they are compared by the non-finite set instead).
"""
import pytest
import torch
import torch.nn.functional as F

import alo_hip
from kernel_bounds import _finite_abs, c_acc, compare

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- launch arithmetic, mirrored from the kernels ----------------------------------------------------------------------------
def conv_tiles(n, h, w, stride):
    """conv.hip alo_conv3x3_nhwc: tiles_per_image = ceil(Ho * Wo / kPix), kPix = 64; ntiles = tiles_per_image * N."""
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    return n * -(-(ho * wo) // 64)


def conv_multi_tile(ntiles):
    """conv.hip launch_conv: per_xcd = ceil(ntiles / 8) capped at 128 workgroups per XCD; conv3x3_kernel walks tiles
    [xcd * per_xcd, tile_end) in steps of gridDim.x / 8 — a second tile exists iff ceil(ntiles / 8) > 128."""
    return -(-ntiles // 8) > 128


def conv_zsplit(ntiles, cin, cout):
    """conv.hip conv_zsplit."""
    if cout == 64:
        return 1
    base, z = ntiles * -(-cout // 128), 1
    while base * z * 2 <= 1024 and cin % (z * 2 * 64) == 0 and cin // (z * 2) >= 128:
        z *= 2
    return z


def conv_z_launched(n, h, w, cin, cout, stride):
    """The split-K factor alo_hip.conv3x3 launches, read back from alo_conv3x3_workspace_bytes = z * N * Ho * Wo * Cout * 4."""
    ws = alo_hip.lib().alo_conv3x3_workspace_bytes(n, h, w, cin, cout, stride)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if ws == 0:
        return 1
    assert ws % (n * ho * wo * cout * 4) == 0
    return ws // (n * ho * wo * cout * 4)


def stem_tiles(n, h, w):
    """stem.hip alo_stem_conv_pool: tiles = ceil(Hp / 8) * ceil(Wp / 7) * N; grid = min(tiles, 768): a 2nd tile iff > 768."""
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    return n * -(-hp // 8) * -(-wp // 7)


def shortk_multi_tile(m, n):
    """gemm.hip launch_shortk: tiles = ceil(M / 64), gx = min(512 / ceil(N / 256), tiles): a 2nd tile iff tiles > gx."""
    tiles = -(-m // 64)
    return tiles > max(1, min(512 // -(-n // 256), tiles))


def check_conv3x3(x, w, b, relu, stride, got, what="conv3x3"):
    """fp64 unfold + matmul per image chunk.  x (N, Cin, H, W) bf16, got (N, Cout, Ho, Wo)."""
    n, cin = x.shape[:2]
    cout = w.shape[0]
    ho, wo = got.shape[2:]
    assert tuple(got.shape) == (n, cout, (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1)
    w64 = w.double().reshape(cout, 9 * cin)
    b64 = b.double() if b is not None else torch.zeros(cout, dtype=torch.float64, device=x.device)
    c = c_acc(9 * cin)
    per = max(1, (1 << 27) // (9 * cin * ho * wo))   # <= 1 GiB of fp64 columns per chunk
    worst = 0.0
    for i0 in range(0, n, per):
        xi = x[i0:i0 + per]
        cols = F.unfold(xi.double(), 3, padding=1, stride=stride)
        ref = (w64 @ cols + b64[:, None]).view(-1, cout, ho, wo)
        if relu:
            ref = torch.relu(ref)
        cols = F.unfold(_finite_abs(xi), 3, padding=1, stride=stride)
        amag = (w64.abs() @ cols + b64.abs()[:, None]).view(-1, cout, ho, wo)
        del cols
        worst = max(worst, compare(got[i0:i0 + per], ref, 2.0 ** -8 * ref.abs() + c * amag, f"{what} images {i0}.."))
    return worst


def check_stem(x, w, b, got, what="stem"):
    """max_pool2d(relu(conv2d(x, w, b, 2, 3)), 3, 2, 1) in fp64, one image at a time.  ReLU and max are 1-Lipschitz and
    monotone, so the convolution's bound carries over as 2^-8 ref + c * max_pool(A)."""
    n, _, h, w_ = x.shape
    hc, wc = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
    w64 = w.double().reshape(64, 147)
    b64 = b.double() if b is not None else torch.zeros(64, dtype=torch.float64, device=x.device)
    worst = 0.0
    for i in range(n):
        xi = x[i:i + 1]
        conv = (w64 @ F.unfold(xi.double(), 7, padding=3, stride=2) + b64[:, None]).view(1, 64, hc, wc)
        ref = F.max_pool2d(torch.relu(conv), 3, 2, 1)
        amag = (w64.abs() @ F.unfold(_finite_abs(xi), 7, padding=3, stride=2) + b64.abs()[:, None]).view(1, 64, hc, wc)
        amag = F.max_pool2d(amag, 3, 2, 1)
        worst = max(worst, compare(got[i:i + 1], ref, 2.0 ** -8 * ref.abs() + c_acc(147) * amag, f"{what} image {i}"))
    return worst


def check_linear(x2, w, b, relu, residual, got2, what="linear"):
    """act(x2 @ w^T + b [+ residual]) in fp64, 64K rows at a time.  x2 (M, K), got2 / residual (M, N)."""
    m, k = x2.shape
    w64 = w.double()
    b64 = b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=x2.device)
    worst = 0.0
    for r0 in range(0, m, 1 << 16):
        xs = x2[r0:r0 + (1 << 16)]
        pre = xs.double() @ w64.t() + b64
        amag = _finite_abs(xs) @ w64.abs().t() + b64.abs()
        ref = pre if residual is None else pre + residual[r0:r0 + (1 << 16)].double()
        if relu:
            ref = torch.relu(ref)
        bound = 2.0 ** -8 * ref.abs() + c_acc(k) * amag
        if residual is not None:   # x W^T + b is rounded to bf16 before the identity is added
            bound = bound + 2.0 ** -8 * torch.nan_to_num(pre.abs(), nan=0.0, posinf=0.0)
        worst = max(worst, compare(got2[r0:r0 + (1 << 16)], ref, bound, f"{what} rows {r0}.."))
    return worst


def _conv_operands(n, cin, cout, h, w, seed, bias=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / (9 * cin) ** 0.5).bfloat16()
    wt = wt.contiguous(memory_format=torch.channels_last)
    b = (0.5 * torch.randn(cout, device=DEV, generator=g)).bfloat16() if bias else None
    return x, wt, b


def _run_conv(x, wt, b, relu, stride):
    with torch.no_grad():
        return alo_hip.conv3x3(x, wt, b, relu=relu, stride=stride)


# ---- 1. conv3x3 --------------------------------------------------------------------------------------------------------------
# (N, Cin, Cout, H, W, stride, relu, bias)
HEADLINE_CONV = [
    (8, 64, 64, 200, 334, 1, True, True),     # layer1: K-split, 8352 tiles
    (8, 128, 128, 200, 334, 2, True, True),   # layer2.0
    (8, 128, 128, 100, 167, 1, True, True),   # layer2
    (8, 256, 256, 100, 167, 2, True, True),   # layer3.0
    (8, 256, 256, 50, 84, 1, True, True),     # layer3
    (8, 512, 512, 50, 84, 2, True, True),     # layer4.0
    (8, 512, 512, 25, 42, 1, True, True),     # layer4
]
LOOP_CONV = [
    (2, 64, 64, 200, 334, 1, True, True),     # 2088 tiles: every XCD's range of 261 crosses the image boundary at 1044
    (1025, 64, 64, 8, 8, 1, False, True),     # one tile per image, one tile more than 1024
    (1031, 64, 128, 8, 8, 1, True, False),    # ntiles % 8 = 7
    (1031, 128, 64, 15, 15, 2, True, True),   # K-split at stride 2, 1031 tiles
]
COLUMN_CONV = [   # Cout an odd multiple of 64: wave 1 of the last column block has no columns
    (2, 64, 192, 40, 50, 1, True, True),
    (2, 128, 192, 41, 53, 2, False, True),
    (2, 64, 320, 40, 50, 1, True, False),
    (3, 128, 320, 41, 53, 2, True, True),
    (8, 64, 192, 100, 100, 1, True, True),    # 1256 tiles
    (8, 64, 320, 200, 200, 2, False, True),   # 1256 tiles at stride 2
    (1, 1024, 192, 9, 9, 1, True, True),      # also split-K, z = 8
]
SPLITK_CONV = [
    (1, 256, 128, 9, 9, 1, True, True),       # z = 2
    (1, 512, 128, 9, 9, 1, False, True),      # z = 4
    (1, 1024, 256, 9, 9, 1, True, True),      # z = 8
    (1, 2048, 256, 9, 9, 2, True, True),      # z = 16 (a single tile)
    (2, 2048, 128, 12, 10, 1, False, False),  # z = 16, 4 tiles
    (8, 2048, 256, 25, 42, 2, False, True),   # input_proj[3] of the headline, z = 8
]
GEOMETRY_CONV = [
    (2, 128, 128, 20, 20, 1, True, True),     # Wo = 20: a 64-pixel tile spans 3-4 rows
    (3, 64, 128, 13, 7, 1, False, True),      # Wo = 7
    (1, 128, 128, 300, 1, 1, True, True),     # W = 1
    (2, 64, 64, 301, 1, 2, False, False),     # W = 1, stride 2, odd H
    (3, 128, 128, 37, 53, 2, True, False),    # odd H and W at stride 2
    (2, 64, 64, 37, 53, 2, False, True),
    (1, 128, 256, 63, 1, 2, True, True),      # Ho * Wo = 32
]


def _conv_case(case, seed):
    n, cin, cout, h, w, stride, relu, bias = case
    x, wt, b = _conv_operands(n, cin, cout, h, w, seed, bias)
    got = _run_conv(x, wt, b, relu, stride)
    check_conv3x3(x, wt, b, relu, stride, got, f"conv3x3 {case}")
    return x, wt, b, got


@pytest.mark.parametrize("case", HEADLINE_CONV + LOOP_CONV)
def test_conv3x3_persistent_loop(case):
    n, cin, cout, h, w, stride = case[:6]
    ntiles = conv_tiles(n, h, w, stride)
    assert (cout == 64) == (case in (HEADLINE_CONV[0], LOOP_CONV[0], LOOP_CONV[1], LOOP_CONV[3]))
    assert conv_z_launched(n, h, w, cin, cout, stride) == 1
    if case in LOOP_CONV or cin <= 128:
        assert conv_multi_tile(ntiles), ntiles   # the route this case is here for
    _conv_case(case, seed=ntiles + cin)


@pytest.mark.parametrize("case", COLUMN_CONV)
def test_conv3x3_column_blocks_with_idle_waves(case):
    n, cin, cout, h, w, stride = case[:6]
    assert (cout // 64) % 2 == 1 and cout > 64
    ntiles = conv_tiles(n, h, w, stride)
    assert conv_z_launched(n, h, w, cin, cout, stride) == conv_zsplit(ntiles, cin, cout)
    _conv_case(case, seed=cout + h)


def test_conv3x3_column_block_cases_cover_both_routes():
    routes = {(conv_multi_tile(conv_tiles(*c[:1], *c[3:6])), conv_z_launched(c[0], c[3], c[4], c[1], c[2], c[5]) > 1) for c in COLUMN_CONV}
    assert (True, False) in routes and (False, True) in routes and {c[5] for c in COLUMN_CONV} == {1, 2}


@pytest.mark.parametrize("case", SPLITK_CONV)
def test_conv3x3_split_k(case):
    n, cin, cout, h, w, stride = case[:6]
    z = conv_z_launched(n, h, w, cin, cout, stride)
    assert z == conv_zsplit(conv_tiles(n, h, w, stride), cin, cout) and z > 1
    assert z == {256: 2, 512: 4, 1024: 8}.get(cin, z)
    _conv_case(case, seed=cin + z)


def test_conv3x3_input_proj_without_workspace():
    """The raw ABI with a NULL workspace runs the same launch with z = 1; both results meet the bound."""
    n, cin, cout, h, w, stride = 8, 2048, 256, 25, 42, 2
    assert conv_z_launched(n, h, w, cin, cout, stride) == 8
    x, wt, b = _conv_operands(n, cin, cout, h, w, seed=7)
    got_z = _run_conv(x, wt, b, False, stride)
    check_conv3x3(x, wt, b, False, stride, got_z, "conv3x3 split-K z = 8")

    def never():
        raise AssertionError("the conv3x3 call above left no packed weight on wt")

    packed = alo_hip.derived(wt, "conv3x3_b", (wt,), never)   # packed by the call above: a hit, the operand as the wrapper left it
    got_1 = torch.empty_like(got_z)
    with torch.cuda.device(x.device):
        rc = alo_hip.lib().alo_conv3x3_nhwc(x.data_ptr(), packed.data_ptr(), b.data_ptr(), got_1.data_ptr(), None, n, h, w, cin,
                                            cout, stride, 0, alo_hip.ALO_BF16, alo_hip._stream(x.device))
    assert rc == 0
    torch.cuda.synchronize()
    check_conv3x3(x, wt, b, False, stride, got_1, "conv3x3 z = 1")


@pytest.mark.parametrize("case", GEOMETRY_CONV)
def test_conv3x3_geometry(case):
    n, cin, cout, h, w, stride = case[:6]
    assert conv_z_launched(n, h, w, cin, cout, stride) == 1
    _conv_case(case, seed=h * 31 + w)


# ---- 1. stem -----------------------------------------------------------------------------------------------------------------
def _stem_operands(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    wt = (torch.randn(64, 3, 7, 7, device=DEV, generator=g) / 147 ** 0.5).bfloat16()
    b = (0.5 * torch.randn(64, device=DEV, generator=g)).bfloat16()
    return g, wt, b


@pytest.mark.parametrize("shape,layout,multi", [((8, 3, 800, 1333), "nchw", True),    # the headline launch: 9600 tiles
                                                ((1, 3, 800, 866), "nchw", True),      # 775 tiles: just over 768
                                                ((3, 3, 101, 77), "nhwc", False),      # odd H and W
                                                ((5, 3, 357, 421), "nhwc", True),      # 960 tiles
                                                ((2, 3, 100, 133), "crop", False)])    # a non-contiguous view
def test_stem_conv_pool(shape, layout, multi):
    g, wt, b = _stem_operands(sum(shape))
    n, _, h, w = shape
    if layout == "crop":
        big = torch.randn(n, 3, h + 20, w + 30, device=DEV, generator=g).bfloat16()
        x = big[:, :, 5:5 + h, 7:7 + w]
        assert not x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
    else:
        x = torch.randn(shape, device=DEV, generator=g).bfloat16()
        if layout == "nhwc":
            x = x.contiguous(memory_format=torch.channels_last)
    assert (stem_tiles(n, h, w) > 768) == multi
    with torch.no_grad():
        got = alo_hip.stem_conv_pool(x, wt, b)
    check_stem(x, wt, b, got, f"stem {shape} {layout}")


# ---- 1. linear_shortk / conv1x1 ----------------------------------------------------------------------------------------------
# (M, K, N, relu, bias, residual)
SHORTK = [
    (534400, 64, 64, True, True, False),      # layer1 conv1 of blocks 1-2 (and the N = 64 route of the persistent loop)
    (534400, 64, 256, True, True, True),      # layer1 conv3 with the identity in the epilogue
    (534400, 256, 128, True, True, False),    # layer2.0 conv1
    (300001, 128, 192, False, True, False),   # column blocks with idle waves
    (200003, 64, 320, True, False, False),
    (100003, 64, 64, False, True, False),     # ragged last tile
    (100003, 128, 320, True, True, True),
]


@pytest.mark.parametrize("case", SHORTK)
def test_linear_shortk_at_backbone_sizes(case):
    m, k, n, relu, bias, res = case
    assert shortk_multi_tile(m, n)
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    x = torch.randn(m, k, device=DEV, generator=g).bfloat16()
    w = (torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).bfloat16()
    b = (0.5 * torch.randn(n, device=DEV, generator=g)).bfloat16() if bias else None
    r = torch.randn(m, n, device=DEV, generator=g).bfloat16() if res else None
    got = alo_hip.linear_shortk(x, w, b, relu, residual=r)
    check_linear(x, w, b, relu, r, got, f"linear_shortk {case}")


@pytest.mark.parametrize("n,cin,cout,h,w,stride,packed", [(8, 256, 512, 200, 334, 2, False),   # layer2 downsample (resident kernel)
                                                           (8, 1024, 2048, 50, 84, 2, True),   # layer4 downsample (packed kernel)
                                                           (3, 512, 1024, 37, 51, 2, True)])
def test_conv1x1_strided_at_headline_size(n, cin, cout, h, w, stride, packed):
    g = torch.Generator(device=DEV).manual_seed(cin + cout)
    x = torch.randn(n, cin, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, device=DEV, generator=g) / cin ** 0.5).bfloat16()
    b = (0.5 * torch.randn(cout, device=DEV, generator=g)).bfloat16()
    with torch.no_grad():
        assert alo_hip.conv1x1_strided_supported(x, wt)
        assert alo_hip.linear_shortk_supported(x.permute(0, 2, 3, 1), wt) == (not packed)
        got = alo_hip.conv1x1_strided(x, wt, b, stride, relu=False)
    rows = x[:, :, ::stride, ::stride].permute(0, 2, 3, 1).reshape(-1, cin)
    check_linear(rows, wt, b, False, None, got.permute(0, 2, 3, 1).reshape(-1, cout), "conv1x1_strided")


# ---- 2. every backbone launch of the headline's own forward ------------------------------------------------------------------
def test_headline_forward_backbone_launches_meet_the_bound(monkeypatch):
    import bench

    device = torch.device(DEV)
    calls = []
    orig = {name: getattr(alo_hip, name) for name in ("conv3x3", "stem_conv_pool", "linear_shortk", "linear_packed", "conv1x1_strided")}

    def conv3x3(x, weight, bias=None, relu=False, stride=1):
        y = orig["conv3x3"](x, weight, bias, relu, stride)
        s = stride[0] if isinstance(stride, (tuple, list)) else stride
        n, cin, h, w = x.shape
        ntiles = conv_tiles(n, h, w, s)
        calls.append(("conv3x3", {"ksplit": weight.shape[0] == 64, "z": conv_z_launched(n, h, w, cin, weight.shape[0], s),
                                  "multi": conv_multi_tile(ntiles)}, check_conv3x3(x, weight, bias, relu, s, y)))
        return y

    def stem_conv_pool(x, weight, bias=None):
        y = orig["stem_conv_pool"](x, weight, bias)
        calls.append(("stem", {"multi": stem_tiles(x.shape[0], x.shape[2], x.shape[3]) > 768}, check_stem(x, weight, bias, y)))
        return y

    def linear_shortk(x, weight, bias=None, relu=False, residual=None):
        y = orig["linear_shortk"](x, weight, bias, relu, residual)
        n, k = weight.shape
        r = None if residual is None else residual.reshape(-1, n)
        x2 = x.reshape(-1, k)
        calls.append(("linear_shortk", {"n": n, "multi": shortk_multi_tile(x2.shape[0], n)},
                      check_linear(x2, weight, bias, relu, r, y.reshape(-1, n))))
        return y

    def linear_packed(x, weight, bias=None, relu=False, residual=None):
        y = orig["linear_packed"](x, weight, bias, relu, residual)
        n, k = weight.shape
        r = None if residual is None else residual.reshape(-1, n)
        calls.append(("linear_packed", {}, check_linear(x.reshape(-1, k), weight, bias, relu, r, y.reshape(-1, n))))
        return y

    def conv1x1_strided(x, weight2d, bias, stride, relu=False):
        y = orig["conv1x1_strided"](x, weight2d, bias, stride, relu)
        cout, cin = weight2d.shape
        rows = x[:, :, ::stride, ::stride].permute(0, 2, 3, 1).reshape(-1, cin)
        calls.append(("conv1x1_strided", {}, check_linear(rows, weight2d, bias, relu, None, y.permute(0, 2, 3, 1).reshape(-1, cout))))
        return y

    for name, fn in (("conv3x3", conv3x3), ("stem_conv_pool", stem_conv_pool), ("linear_shortk", linear_shortk),
                     ("linear_packed", linear_packed), ("conv1x1_strided", conv1x1_strided)):
        monkeypatch.setattr(alo_hip, name, fn)
    model = bench.build_detector(device, torch.bfloat16)
    frames = bench.detection_inputs(8, 0, device, torch.bfloat16)
    with torch.no_grad():
        model(frames)
    torch.cuda.synchronize()

    kinds = {k for k, _, _ in calls}
    assert kinds >= {"conv3x3", "stem", "linear_shortk", "linear_packed", "conv1x1_strided"}, kinds
    worst = max(r for _, _, r in calls)
    assert worst <= 1.0, worst   # compare() already raised on the first violation; this states the result
    conv = [route for k, route, _ in calls if k == "conv3x3"]
    assert any(r["ksplit"] and r["multi"] for r in conv), "no K-split launch with a second tile per workgroup"
    assert any(r["z"] > 1 for r in conv), "no split-K launch"
    assert any(not r["ksplit"] and r["multi"] for r in conv), "no column-block launch with a second tile"
    assert any(route["multi"] for k, route, _ in calls if k == "stem"), "the stem did not take its persistent loop"
    assert any(route["multi"] and route["n"] == 64 for k, route, _ in calls if k == "linear_shortk"), "no multi-tile N = 64 shortk"
    print(f"{len(calls)} backbone launches checked, worst error / bound = {worst:.3g}")


# ---- 3. non-finite inputs ----------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def _plant_nhwc(x, spots):
    """spots: (image, channel, y, x, value); x is (N, C, H, W) in any memory format."""
    x = x.clone(memory_format=torch.preserve_format)
    for n, c, yy, xx, v in spots:
        x[n, c, yy, xx] = v
    return x


@pytest.mark.parametrize("n,cin,cout,h,w,stride,relu", [(2, 64, 64, 40, 50, 1, True),       # K-split
                                                         (2, 64, 128, 40, 50, 1, True),
                                                         (2, 64, 128, 40, 50, 1, False),
                                                         (2, 128, 192, 40, 50, 2, True),
                                                         (1031, 64, 64, 8, 8, 1, True),       # multi-tile, one tile per image
                                                         (1031, 64, 128, 8, 8, 1, False),
                                                         (2, 1024, 192, 9, 9, 1, True)])      # split-K, z = 8
def test_conv3x3_non_finite_inputs(n, cin, cout, h, w, stride, relu):
    x, wt, b = _conv_operands(n, cin, cout, h, w, seed=n + cout + h)
    hw = h * w
    t = min(5, hw // 64 - 1) if hw >= 128 else 0
    first, last = 64 * t, min(64 * t + 63, hw - 1)   # first and last pixel of a 64-pixel tile (stride 1: output = input pixel)
    spots = [(0, 3, 0, 0, NAN),                                   # image corner
             (0, 5, first // w, first % w, NAN), (0, 6, last // w, last % w, INF),
             (0, 7, h - 1, w - 1, INF), (0, 8, h - 1, w - 1, NAN),  # the last pixel of image 0
             (n - 1, cin - 1, h - 1, w - 1, NAN), (n - 1, 1, h // 2, w // 2, -INF)]
    if n > 128:
        spots += [(128, 2, 0, 0, INF), (127, 4, h - 1, w - 1, NAN)]   # images that follow / precede one in the same workgroup
    if n > 1:
        spots += [(1, 0, 0, 0, INF)]
    x = _plant_nhwc(x, spots)
    got = _run_conv(x, wt, b, relu, stride)
    assert not torch.isfinite(got).all()
    check_conv3x3(x, wt, b, relu, stride, got, "conv3x3 non-finite")


def test_stem_non_finite_inputs_stay_in_their_windows():
    """NaN / Inf at a tile's staged pixels, including the pixel 2 lc + 7 just past an output's 7-tap window (read there only
    against zero weights) and the row 2 lr + 7 below it: the non-finite pooled outputs are exactly the fp64 op's."""
    g, wt, b = _stem_operands(5)
    n, h, w = 3, 130, 150
    x = torch.randn(n, 3, h, w, device=DEV, generator=g).bfloat16()
    # tile (ty, tx) stages input rows 32 ty - 5 .. and columns 28 tx - 5 ..; Y % 4 == 2 and X % 4 == 2 put the zero-weight
    # column / row of a convolution output into the window of a pooled pixel that the legitimate outputs do not reach
    spots = [(0, 0, 0, 0, INF), (0, 1, h - 1, w - 1, NAN), (1, 2, 0, w - 1, INF),
             (0, 0, 46, 46, INF), (0, 1, 50, 74, INF), (1, 2, 66, 90, INF), (2, 0, 38, 58, INF), (2, 1, 94, 102, NAN),
             (1, 0, 27, 27, INF), (2, 2, 59, 83, INF), (n - 1, 2, h - 1, 0, INF)]
    x = _plant_nhwc(x, spots)
    with torch.no_grad():
        got = alo_hip.stem_conv_pool(x, wt, b)
    assert not torch.isfinite(got).all()
    check_stem(x, wt, b, got, "stem non-finite")


def test_stem_non_finite_inputs_multi_tile():
    g, wt, b = _stem_operands(6)
    n, h, w = 4, 480, 640     # 4 * 15 * 23 = 1380 tiles
    assert stem_tiles(n, h, w) > 768
    x = torch.randn(n, 3, h, w, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    x = _plant_nhwc(x, [(0, 0, 0, 0, NAN), (0, 1, 30, 26, INF), (1, 2, 62, 54, INF), (2, 0, h - 1, w - 1, INF),
                        (3, 1, 250, 310, NAN), (3, 2, 254, 318, INF)])
    with torch.no_grad():
        got = alo_hip.stem_conv_pool(x, wt, b)
    check_stem(x, wt, b, got, "stem non-finite multi-tile")


def _rows_with_spots(m, k, seed, rows):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(m, k, device=DEV, generator=g).bfloat16()
    for i, (r, v) in enumerate(rows):
        x[r, (7 * i) % k] = v
    return g, x


@pytest.mark.parametrize("m,k,n,relu,res", [(100003, 64, 64, True, False), (100003, 64, 64, False, False),
                                            (5000, 128, 256, True, True), (5000, 256, 320, False, True), (777, 256, 64, True, False)])
def test_linear_shortk_non_finite_inputs(m, k, n, relu, res):
    rows = [(0, NAN), (63, INF), (64, NAN), (64 * 37 + 63, -INF), (m - 1, NAN), (m - 2, INF)]
    g, x = _rows_with_spots(m, k, m + n, [(r, v) for r, v in rows if r < m])
    w = (torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).bfloat16()
    b = (0.5 * torch.randn(n, device=DEV, generator=g)).bfloat16()
    r = None
    if res:
        r = torch.randn(m, n, device=DEV, generator=g).bfloat16()
        r[100, 3], r[101, n - 1], r[m - 3, 0] = NAN, INF, -INF
    got = alo_hip.linear_shortk(x, w, b, relu, residual=r)
    assert not torch.isfinite(got).all()
    check_linear(x, w, b, relu, r, got, "linear_shortk non-finite")


@pytest.mark.parametrize("relu,res", [(True, False), (False, False), (True, True)])
def test_linear_packed_non_finite_inputs(relu, res):
    m, k, n = 3001, 512, 256
    g, x = _rows_with_spots(m, k, 17, [(0, NAN), (63, INF), (64, NAN), (1000, -INF), (m - 1, NAN)])
    w = (torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).bfloat16()
    b = (0.5 * torch.randn(n, device=DEV, generator=g)).bfloat16()
    r = None
    if res:
        r = torch.randn(m, n, device=DEV, generator=g).bfloat16()
        r[7, 3], r[200, n - 1] = NAN, INF
    with torch.no_grad():
        got = alo_hip.linear_packed(x, w, b, relu, residual=r)
    check_linear(x, w, b, relu, r, got, "linear_packed non-finite")


def test_ffn256_non_finite_inputs():
    """relu(x W1^T + b1) W2^T + b2 with NaN in rows of x: those rows come out NaN (torch's relu keeps NaN), the rest within
    the two products' bounds (the hidden layer is rounded to bf16 in between)."""
    m, fh = 1000, 1024
    g, x = _rows_with_spots(m, 256, 23, [(0, NAN), (63, NAN), (64, NAN), (m - 1, NAN)])
    w1 = (torch.randn(fh, 256, device=DEV, generator=g) / 16).bfloat16()
    b1 = (0.5 * torch.randn(fh, device=DEV, generator=g)).bfloat16()
    w2 = (torch.randn(256, fh, device=DEV, generator=g) / 32).bfloat16()
    b2 = (0.5 * torch.randn(256, device=DEV, generator=g)).bfloat16()
    got = alo_hip.ffn256(x, w1, b1, w2, b2)
    x64, w1d, w2d = x.double(), w1.double(), w2.double()
    h = torch.relu(x64 @ w1d.t() + b1.double())
    eh = 2.0 ** -8 * h.abs() + c_acc(256) * (_finite_abs(x) @ w1d.abs().t() + b1.double().abs())   # error of the bf16 hidden
    eh = torch.nan_to_num(eh, nan=0.0)
    ref = h @ w2d.t() + b2.double()
    amag = (torch.nan_to_num(h.abs(), nan=0.0) + eh) @ w2d.abs().t() + b2.double().abs()
    bound = 2.0 ** -8 * ref.abs() + c_acc(fh) * amag + eh @ w2d.abs().t()
    assert torch.isnan(got[[0, 63, 64, m - 1]].float()).all()
    compare(got, ref, bound, "ffn256 non-finite")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("relu,res", [(True, False), (True, True), (False, True)])
def test_bias_act_non_finite_inputs(dtype, relu, res):
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(2, 64, 9, 11, device=DEV, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(64, device=DEV, generator=g).to(dtype)
    x = _plant_nhwc(x, [(0, 0, 0, 0, NAN), (0, 5, 3, 4, INF), (1, 63, 8, 10, NAN), (1, 7, 2, 2, -INF)])
    r = None
    if res:
        r = torch.randn(2, 64, 9, 11, device=DEV, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
        r = _plant_nhwc(r, [(0, 1, 0, 0, NAN), (1, 2, 4, 4, INF), (1, 3, 5, 5, -INF)])
    want = x.double() + bias.double().view(1, -1, 1, 1) + (r.double() if res else 0)
    want = torch.relu(want) if relu else want
    amag = _finite_abs(x) + bias.double().abs().view(1, -1, 1, 1) + (_finite_abs(r) if res else 0)
    got = alo_hip.bias_act_(x.clone(memory_format=torch.preserve_format), bias, r, relu)
    compare(got, want, 2.0 ** -8 * want.abs() + 2.0 ** -22 * amag, f"bias_act {dtype}")
