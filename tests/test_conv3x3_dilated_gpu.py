"""The dilated 3x3 convolution (dilation 2, padding 2, stride 1: ALO_CONV_DILATION_2 of alo_conv3x3_nhwc; conv3x3_kernel<PlanS1<2>, ..> of
aloception-oss_amd/csrc/conv.hip in bf16, conv3x3_d2_f32_kernel of conv_f32.hip in fp32) against F.conv2d(..., 1, 2, 2) in fp64 on the
kernel's own operands, every output element within the bounds of conv_dilated_ref.py (the undilated kernels' bounds over the dilated
window); then the gates, the routes of a DC5 backbone and a DC5 Deformable-DETR.

References are computed on the CPU, once per (shape, dtype), and shared by the cases that need them."""
import functools

import pytest
import torch

import alo_hip
from conv_dilated_ref import OFFSETS, reference_and_bound, reference_parts
from guarded import GuardedLaunches
from kernel_bounds import INF, NAN, compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAMES = {BF16: "bf16", F32: "fp32"}
D2_TAG = {BF16: "conv3x3/C=512/s=1/d=2", F32: "conv3x3_f32/C=512/s=1/d=2"}

# (N, Cin, Cout, H, W): where the kernels can go wrong.  A tile is 64 consecutive pixels of one image; a column block is 128 channels.
SHAPES = [
    (2, 64, 64, 5, 7),          # Cout = 64: the two waves split K; 64 -> 64 must NOT take the (undilated) register kernel
    (1, 64, 128, 1, 1),         # only the centre tap exists
    (1, 128, 64, 2, 3),         # maps smaller than the reach
    (3, 128, 128, 9, 13),       # 117 pixels: two tiles, a tile edge inside a row, clamped reads across image ends inside the batch
    (1, 64, 192, 66, 3),        # W smaller than the reach; a column block whose second wave has no columns
    (1, 64, 128, 3, 70),        # a row longer than a tile
    (2, 64, 128, 200, 167),     # 1044 tiles, 131 per XCD > 128 workgroups: the persistent loop's second tile, prefetched across the image end
]
DC5_SHAPE = (2, 512, 512, 13, 21)   # the DC5 width; 10 tiles x 4 column blocks: split-K with z = 4.  bf16 only
NONFINITE_SHAPE = (3, 128, 128, 9, 13)
CASES = [(s, dt) for s in SHAPES for dt in (BF16, F32)] + [(DC5_SHAPE, BF16)]


def _id(case):
    return "x".join(map(str, case[0])) + "-" + NAMES[case[1]]


@functools.lru_cache(maxsize=None)
def _operands(shape, dtype):
    """x (channels-last), w, b of ``dtype`` on the CPU: drawn once per shape (the bf16 ones are the rounded fp32 ones), never written to."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + cin + cout + 7 * h + w)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dtype)
    b = (0.5 * torch.randn(cout, generator=g)).to(dtype)
    return x, wt, b


@functools.lru_cache(maxsize=None)
def _parts(shape, dtype):
    x, wt, _ = _operands(shape, dtype)
    return reference_parts(x, wt)


def _run(x, wt, b, relu):
    """The public wrapper of x's dtype on CPU operands -> CPU result."""
    fn = alo_hip.conv3x3 if x.dtype == BF16 else alo_hip.conv3x3_f32
    with torch.no_grad():
        y = fn(x.to(DEV).contiguous(memory_format=torch.channels_last), wt.to(DEV), None if b is None else b.to(DEV), relu=relu, dilation=2)
    assert y.dtype == x.dtype and y.shape == (x.shape[0], wt.shape[0]) + x.shape[2:] and y.is_contiguous(memory_format=torch.channels_last)
    return y.cpu()


def _z_launched(shape):
    """The split-K factor the bf16 wrapper launches, read back from the workspace size (z partial sums of N H W Cout fp32)."""
    n, cin, cout, h, w = shape
    ws = alo_hip.lib().alo_conv3x3_workspace_bytes(n, h, w, cin, cout, 1 | alo_hip.ALO_CONV_DILATION_2)
    assert ws % (n * h * w * cout * 4) == 0
    return max(1, ws // (n * h * w * cout * 4))


# ---- 1. every element within the bound -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu_bias", [True, False], ids=["relu+bias", "plain"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_meets_the_bound(case, relu_bias):
    shape, dtype = case
    x, wt, b = _operands(shape, dtype)
    b = b if relu_bias else None
    assert _z_launched(shape) == (4 if shape == DC5_SHAPE else 1)
    ref, bound = reference_and_bound(x, wt, b, relu_bias, _parts(shape, dtype))
    ratio = compare(_run(x, wt, b, relu_bias), ref, bound, f"dilated conv3x3 {NAMES[dtype]} {shape}")
    print(f"dilated conv3x3 {NAMES[dtype]} {shape} relu+bias={relu_bias}: worst |err| / bound = {ratio:.4f}")


def test_persistent_loop_case_has_a_second_tile_per_workgroup():
    """conv.hip launch_conv_d2 / conv_f32.hip launch_conv_f32: at most 128 workgroups per XCD, each XCD an eighth of the tiles."""
    n, _, _, h, w = SHAPES[-1]
    assert -(-(n * -(-(h * w) // 64)) // 8) > 128


def test_dc5_width_without_a_workspace_runs_unsplit():
    """The raw ABI with a NULL workspace runs the same convolution with z = 1 (as test_conv3x3_input_proj_without_workspace)."""
    n, cin, cout, h, w = DC5_SHAPE
    x, wt, b = _operands(DC5_SHAPE, BF16)
    xg, wg, bg = x.to(DEV).contiguous(memory_format=torch.channels_last), wt.to(DEV), b.to(DEV)
    with torch.no_grad():
        got_z = alo_hip.conv3x3(xg, wg, bg, relu=False, dilation=2)

    def never():
        raise AssertionError("the conv3x3 call above left no packed weight on the weight")

    packed = alo_hip.derived(wg, "conv3x3_b", (wg,), never)     # the undilated call's packed matrix: one cache entry for both
    got_1 = torch.empty_like(got_z)
    with torch.cuda.device(xg.device):
        rc = alo_hip.lib().alo_conv3x3_nhwc(xg.data_ptr(), packed.data_ptr(), bg.data_ptr(), got_1.data_ptr(), None, n, h, w, cin, cout,
                                            1 | alo_hip.ALO_CONV_DILATION_2, 0, alo_hip.ALO_BF16, alo_hip._stream(xg.device))
    assert rc == 0
    torch.cuda.synchronize()
    ref, bound = reference_and_bound(x, wt, b, False, _parts(DC5_SHAPE, BF16))
    compare(got_z.cpu(), ref, bound, "dilated conv3x3 z = 4")
    compare(got_1.cpu(), ref, bound, "dilated conv3x3 z = 1")


# ---- 2. tap geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAMES.get)
@pytest.mark.parametrize("cout", [64, 128], ids=["k-split", "column-block"])
def test_a_single_pixel_spreads_the_nine_taps_two_pixels_apart(dtype, cout):
    """x = 0 except a 1 at one interior pixel and at each corner (a channel each): every output is one weight element or zero, so the
    result must equal the weight's taps at offsets {-2, 0, 2}^2 around each planted pixel bit for bit — an off-by-one tap stride cannot
    hide inside a bound.  The weights carry 8 significant bits: exact in bf16, and in fp32 a two-term fp16 split holds them whole
    (22 bits would not hold a random fp32 weight).  No two planted pixels share an output: they lie more than 4 apart in x or in y (asserted below)."""
    h, w, cin = 9, 13, 64
    g = torch.Generator().manual_seed(17 + cout)
    wt = torch.randn(cout, cin, 3, 3, generator=g).bfloat16().to(dtype)
    planted = [(4, 6, 5), (0, 0, 0), (0, w - 1, 17), (h - 1, 0, 33), (h - 1, w - 1, 63)]     # (y, x, channel)
    x = torch.zeros(1, cin, h, w, dtype=dtype).contiguous(memory_format=torch.channels_last)
    want = torch.zeros(1, cout, h, w, dtype=dtype)
    for py, px, c in planted:
        x[0, c, py, px] = 1
        for ky, oy in enumerate(OFFSETS):
            for kx, ox in enumerate(OFFSETS):
                yy, xx = py - oy, px - ox            # the output whose tap (ky, kx) reads the planted pixel
                if 0 <= yy < h and 0 <= xx < w:
                    assert (want[0, :, yy, xx] == 0).all()
                    want[0, :, yy, xx] = wt[:, c, ky, kx]
    got = _run(x, wt, None, False)
    assert torch.equal(got, want), (got != want).nonzero()[:8].tolist()


# ---- 3. non-finite inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAMES.get)
def test_non_finite_inputs_spoil_exactly_their_dilated_windows(dtype, relu):
    """NaN (image 0), +Inf (image 1) and both (image 2) at (0, 0), (H - 1, W - 1) and an interior pixel.  An output whose dilated window
    holds none of them meets the bound — also where the clamped pixel behind a padding tap is a planted one; the others have the
    reference's kind (ReLU keeps NaN)."""
    n, cin, cout, h, w = NONFINITE_SHAPE
    x, wt, b = _operands(NONFINITE_SHAPE, dtype)
    x = x.clone(memory_format=torch.preserve_format)
    spots = [(0, 0), (h - 1, w - 1), (4, 6)]
    for i, values in enumerate(((NAN, NAN, NAN), (INF, INF, INF), (NAN, INF, INF))):
        for (py, px), v, c in zip(spots, values, (3, cin - 1, 70)):
            x[i, c, py, px] = v
    ref, bound = reference_and_bound(x, wt, b, relu)
    spoiled = torch.zeros(h, w, dtype=torch.bool)
    for py, px in spots:
        for oy in OFFSETS:
            for ox in OFFSETS:
                if 0 <= py - oy < h and 0 <= px - ox < w:
                    spoiled[py - oy, px - ox] = True
    if not relu:    # (ReLU turns -Inf into 0)
        assert torch.equal(~torch.isfinite(ref), spoiled.expand_as(ref)), "the reference's own windows"
    assert torch.isnan(ref[0]).any() and torch.isinf(ref[1]).any() and torch.isfinite(ref).any()
    got = _run(x, wt, b, relu)
    compare(got, ref, bound, f"dilated conv3x3 {NAMES[dtype]} with NaN / Inf inputs")
    assert torch.equal(torch.isnan(got), torch.isnan(ref))


# ---- 4. buffer discipline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(DC5_SHAPE, BF16), ((3, 128, 128, 9, 13), F32), ((2, 64, 64, 5, 7), BF16)], ids=_id)
def test_launches_stay_in_their_buffers_and_ignore_stale_bytes(case):
    """tests/guarded.py: every launch runs twice between guard zones, y and the workspace (split-K partial sums; the fp32 flavour's
    per-image magnitudes) pre-filled with 0xFF and with 0x3C bytes; nothing else may change and the results must agree."""
    shape, dtype = case
    x, wt, b = _operands(shape, dtype)
    with GuardedLaunches() as g:
        got = _run(x, wt, b, True)
    assert "alo_conv3x3_nhwc" in {symbol for symbol, _ in g.seen}
    ref, bound = reference_and_bound(x, wt, b, True, _parts(shape, dtype))
    compare(got, ref, bound, f"guarded dilated conv3x3 {NAMES[dtype]} {shape}")


# ---- 5. gates ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAMES.get)
def test_supported_gates(dtype):
    gate, other = ((alo_hip.conv3x3_supported, alo_hip.conv3x3_f32_supported) if dtype == BF16
                   else (alo_hip.conv3x3_f32_supported, alo_hip.conv3x3_supported))
    x = torch.randn(1, 128, 6, 5, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    w = torch.randn(64, 128, 3, 3, device=DEV).to(dtype)
    with torch.no_grad():
        assert gate(x, w, (1, 1), (2, 2), (2, 2))
        assert not other(x, w, (1, 1), (2, 2), (2, 2))
        assert not gate(x, w, (2, 2), (2, 2), (2, 2))                                  # no dilation at stride 2
        assert not gate(x, w, (1, 1), (4, 4), (4, 4))                                  # no dilation 4
        for padding in ((4, 4), (1, 1), (0, 0), (3, 3), (2, 1), (1, 2)):
            assert not gate(x, w, (1, 1), padding, (2, 2)), padding
        assert not gate(x, w, (1, 1), (2, 2), (1, 1)) and not gate(x, w, (1, 1), (2, 2), (2, 1))
        assert not gate(x, w, dilation=(2, 2))                                         # the default padding (1, 1)
        assert not gate(x, w, (1, 1), (2, 2), (2, 2), groups=2)
        assert not gate(x.contiguous(), w, (1, 1), (2, 2), (2, 2))                     # NCHW
        assert gate(x, w) and gate(x, w, (2, 2))                                       # the undilated answers are what they were
        fn = alo_hip.conv3x3 if dtype == BF16 else alo_hip.conv3x3_f32
        for stride, dilation in ((2, 2), (1, 4), (1, 3)):
            with pytest.raises(RuntimeError, match="needs"):
                fn(x, w, stride=stride, dilation=dilation)
    assert not gate(x, w, (1, 1), (2, 2), (2, 2))                                      # grad mode on: no backward


def test_undilated_tags_and_packed_weights_are_what_they_were():
    x, wt, b = (t.to(DEV) for t in _operands((1, 128, 64, 2, 3), BF16))
    x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), alo_hip.LaunchTimer() as timer:
        alo_hip.conv3x3(x, wt, b)
        pack = wt.__dict__["_alo_derived"]["conv3x3_b"][1]
        alo_hip.conv3x3(x, wt, b, dilation=2)
        alo_hip.conv3x3_f32(x.float(), wt.float(), b.float(), dilation=(2, 2))
        alo_hip.conv3x3_f32(x.float(), wt.float(), b.float(), stride=2)
    torch.cuda.synchronize()
    assert wt.__dict__["_alo_derived"]["conv3x3_b"][1] is pack                          # one packed matrix serves both geometries
    tags = {t: v for t, v in timer.summary().items() if t.startswith("conv3x3")}
    assert set(tags) == {"conv3x3/C=128/s=1", "conv3x3/C=128/s=1/d=2", "conv3x3_f32/C=128/s=1/d=2", "conv3x3_f32/C=128/s=2"}, set(tags)
    a, d = tags["conv3x3/C=128/s=1"], tags["conv3x3/C=128/s=1/d=2"]
    assert a["alg_flops_avg"] == d["alg_flops_avg"] == 2.0 * 9 * 128 * 64 * 6 and a["alg_bytes_avg"] == d["alg_bytes_avg"]


# ---- 6. the DC5 backbone ---------------------------------------------------------------------------------------------------------------
def _frames(dtype):
    import aloscene

    cpu = torch.Generator().manual_seed(5)
    fr = [aloscene.Frame(torch.rand(3, 96, 128, generator=cpu) * 255, normalization="255").norm_resnet() for _ in range(2)]
    return aloscene.Frame.batch_list(fr).to(DEV).to(dtype)


def _check_launch(x, weight, bias, relu, stride, dilation, y):
    """One recorded 3x3 launch against its fp64 reference, at its bound -> worst error / bound."""
    x, weight, y = x.cpu(), weight.cpu(), y.cpu()
    bias = None if bias is None else bias.cpu()
    s = stride[0] if isinstance(stride, (tuple, list)) else stride
    d = dilation[0] if isinstance(dilation, (tuple, list)) else dilation
    if d == 2:
        assert s == 1
        ref, bound = reference_and_bound(x, weight, bias, relu)
    elif x.dtype == BF16:
        from test_backbone_kernels_gpu import check_conv3x3
        return check_conv3x3(x, weight, bias, relu, s, y)
    else:
        from conv_f32_ref import reference_and_bound as undilated
        ref, bound = undilated(x, weight, bias, s, relu)
    return compare(y, ref, bound, f"conv3x3 {tuple(x.shape)} -> {weight.shape[0]} s={s} d={d}")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAMES.get)
def test_dc5_backbone_takes_the_dilated_route_and_every_launch_meets_its_bound(dtype, monkeypatch):
    """layer4.1.conv2 and layer4.2.conv2 of a DC5 ResNet-50 (512 -> 512, dilation 2) reach the kernel exactly when the route is on, with
    their dilation; ALO_CONV3X3_DILATED=off keeps them on the stock ops.  fp32: under ALO_F32_LAYERS=split."""
    from alonet.deformable_detr.backbone import Backbone

    name = "conv3x3" if dtype == BF16 else "conv3x3_f32"
    orig, calls = getattr(alo_hip, name), []

    def recording(x, weight, bias=None, relu=False, stride=1, dilation=1):
        y = orig(x, weight, bias, relu, stride, dilation)
        calls.append((dilation, _check_launch(x, weight, bias, relu, stride, dilation, y)))
        return y

    monkeypatch.setattr(alo_hip, name, recording)
    if dtype == F32:
        monkeypatch.setenv("ALO_F32_LAYERS", "split")
    torch.manual_seed(0)
    backbone = Backbone("resnet50", False, True, dilation=True).to(DEV).to(dtype).eval()
    assert [backbone.body.layer4[i].conv2.dilation for i in range(3)] == [(1, 1), (2, 2), (2, 2)]
    frames = _frames(dtype)
    routed = alo_hip.CONV3X3_DILATED_ROUTED if dtype == BF16 else alo_hip.CONV3X3_F32_DILATED_ROUTED
    for knob in ("on", "off"):
        monkeypatch.setenv("ALO_CONV3X3_DILATED", knob)
        assert alo_hip.conv3x3_dilated_routed(dtype) == (routed and knob == "on")
        del calls[:]
        with torch.no_grad(), alo_hip.LaunchTimer() as timer:
            out = backbone(frames)
        torch.cuda.synchronize()
        tags = timer.summary()
        want = 2 if routed and knob == "on" else 0
        assert sum(v["calls"] for t, v in tags.items() if t.endswith("/d=2")) == want, tags.keys()
        assert tags.get(D2_TAG[dtype], {"calls": 0})["calls"] == want
        # 16 bottlenecks; ALO_F32_LAYERS=split leaves layer3.0.conv2 (256 channels at stride 2) on the stock ops
        assert sum(1 for d, _ in calls if d != 1) == want and len(calls) == (14 if dtype == BF16 else 13) + want, calls
        assert max(r for _, r in calls) <= 1.0            # compare() already raised on the first violation
        assert out["3"][0].shape[-2:] == out["2"][0].shape[-2:] == (6, 8) and out["3"][0].shape[1] == 2048
        assert torch.isfinite(out["3"][0].float()).all()


# ---- 7. a DC5 Deformable-DETR ------------------------------------------------------------------------------------------------------------
def test_dc5_deformable_detr_forward_inference_and_graph_replay():
    from alonet.common import GraphedForward
    from alonet.deformable_detr import DeformableDETR
    from alonet.deformable_detr.backbone import Backbone, Joiner

    class Dc5Detr(DeformableDETR):
        def __init__(self):
            backbone = Joiner(Backbone("resnet50", False, True, dilation=True), self.build_positional_encoding(256))
            transformer = self.build_transformer(hidden_dim=256, dropout=0.1, nheads=8, dim_feedforward=1024, enc_layers=2, dec_layers=2,
                                                 num_feature_levels=4, dec_n_points=4, enc_n_points=4)
            super().__init__(backbone, transformer, num_classes=91, num_queries=50, aux_loss=False, device=torch.device(DEV))

    torch.manual_seed(0)
    model = Dc5Detr().eval().to(BF16)
    frames = _frames(BF16)
    with torch.no_grad():
        with alo_hip.LaunchTimer() as timer:
            eager = model(frames)
        want = 2 if alo_hip.conv3x3_dilated_routed() else 0
        assert timer.summary().get(D2_TAG[BF16], {"calls": 0})["calls"] == want
        assert eager["pred_logits"].shape == (2, 50, 91) and eager["pred_boxes"].shape == (2, 50, 4)
        for key in ("pred_logits", "pred_boxes"):
            assert torch.isfinite(eager[key].float()).all(), key
        boxes = model.inference(eager)
        assert len(boxes) == 2 and all(b.shape[-1] == 4 for b in boxes)
        eager = {k: eager[k].clone() for k in ("pred_logits", "pred_boxes")}
        graphed = GraphedForward(model)
        for _ in range(2):
            got = graphed(frames)
            for key, value in eager.items():
                assert torch.equal(got[key], value), key
