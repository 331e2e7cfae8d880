"""alo_hip.stem_conv_pool_f32 (alo_stem_conv_pool with dtype = ALO_F32, aloception-oss_amd/csrc/stem_f32.hip) against
max_pool2d(relu(conv2d)) in fp64 on the same fp32 operands, per output element, within the bound derived in stem_f32_ref.py — which
test_stem_f32_cpu.py holds the numpy restatement of the kernel's arithmetic to.  Then the backbone's stem on the route
(``ALO_F32_LAYERS=split``): its output, its launch tag, and a graph replay."""
import copy
import functools

import pytest
import torch

import alo_hip
import guarded
from kernel_bounds import INF, NAN, compare
from stem_f32_ref import out_sizes, reference_and_bound, stock_fp32, tiles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "ALO_F32_LAYERS"
TAG = "stem_conv_pool_f32"
GRID = 256                       # csrc/stem_f32.hip: one persistent workgroup per CU

SMALL, PARTIAL, MULTI = (1, 3, 8, 8), (2, 3, 37, 53), (13, 3, 256, 224)
LAYOUTS = ["nchw", "channels_last", "crop"]


@functools.lru_cache(maxsize=None)
def _operands(shape, scale=1.0):
    """x, w, b on the CPU: drawn once per (shape, scale), never written to."""
    g = torch.Generator().manual_seed(shape[0] * 1000 + 7 * shape[2] + shape[3])
    x = torch.randn(*shape, generator=g) * scale
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    w[5] *= 1e-6                                                    # an output channel with an exponent of its own
    b = torch.randn(64, generator=g) * scale
    return x, w, b


@functools.lru_cache(maxsize=None)
def _reference(shape, scale=1.0, bias=True):
    x, w, b = _operands(shape, scale)
    return reference_and_bound(x, w, b if bias else None)


def _on_gpu(x, layout):
    xg = x.to(DEV)
    if layout == "channels_last":
        return xg.contiguous(memory_format=torch.channels_last)
    if layout == "crop":          # a window of a larger tensor: every stride differs from the dense one
        n, c, h, w = x.shape
        big = torch.full((n + 1, c + 1, h + 5, w + 3), NAN, device=DEV)
        view = big[1:, 1:, 2:2 + h, 3:3 + w]
        view.copy_(xg)
        assert not view.is_contiguous()
        return view
    return xg.contiguous()


def _run(x, w, b, layout="nchw"):
    with torch.no_grad():
        y = alo_hip.stem_conv_pool_f32(_on_gpu(x, layout), w.to(DEV), None if b is None else b.to(DEV))
    _, _, hp, wp = out_sizes(*x.shape[2:])
    assert y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0], 64, hp, wp) and y.is_contiguous(memory_format=torch.channels_last)
    return y.cpu()


def _ratio(got, ref, bound):
    """Worst |err| / bound over the finite outputs of the reference: a figure to print, not a check."""
    fin = torch.isfinite(ref)
    return ((got.double() - ref).abs()[fin] / bound[fin].clamp_min(1e-300)).max().item()


def _report(what, got, ref, bound, x, w, b):
    ratio = compare(got, ref, bound, what)
    fin = torch.isfinite(ref)
    stock_ratio = _ratio(stock_fp32(x, w, b), ref, bound)
    print(f"{what}: worst |err| / bound = {ratio:.4f}; the stock fp32 ops (CPU): {stock_ratio:.4f}; "
          f"max |err| / max |ref| = {((got.double() - ref).abs()[fin].max() / ref[fin].abs().max().clamp_min(1e-300)).item():.3g}")
    return ratio


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "plain"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_partial_tiles_in_every_layout(layout, bias):
    x, w, b = _operands(PARTIAL)
    b = b if bias else None
    ref, bound = _reference(PARTIAL, 1.0, bias)
    assert tiles(*PARTIAL[2:]) == (2, 2)                            # Hp x Wp = 10 x 14: partial tiles in both directions
    _report(f"stem_conv_pool_f32 {PARTIAL} {layout} bias={bias}", _run(x, w, b, layout), ref, bound, x, w, b)


@pytest.mark.parametrize("shape", [SMALL, MULTI], ids=["smaller-than-a-tile", "a-second-tile-per-workgroup"])
def test_small_and_multi_tile_launches_stay_in_their_buffers(shape):
    x, w, b = _operands(shape)
    ref, bound = _reference(shape)
    ty, tx = tiles(*shape[2:])
    assert (shape[0] * ty * tx > GRID) == (shape is MULTI)          # 13 x 8 x 8 = 832 tiles on 256 workgroups
    with guarded.GuardedLaunches() as g:
        got = _run(x, w, b)
    assert ("alo_stem_conv_pool", TAG) in g.seen, g.seen
    _report(f"stem_conv_pool_f32 {shape}", got, ref, bound, x, w, b)
    assert torch.equal(_run(x, w, b), got)                          # two calls give equal bits


@pytest.mark.parametrize("scale", [1e-20, 1.0, 3e4, 5e18])
def test_kernel_meets_the_bound_at_any_input_magnitude(scale):
    x, w, b = _operands(PARTIAL, scale)
    ref, bound = _reference(PARTIAL, scale)
    _report(f"stem_conv_pool_f32, image at {scale}", _run(x, w, b), ref, bound, x, w, b)


def test_a_dim_half_keeps_the_bound_of_its_own_windows():
    """The left half 10^6 dimmer than the right one: the bound of a pooled pixel knows its own window's magnitude only
    (stem_f32_ref.reference_and_bound), so the pixels whose window lies in the dim half are held to a bound 10^6 smaller."""
    x, w, _ = _operands((1, 3, 72, 128))
    x = x.clone()
    x[..., :64] *= 1e-6
    ref, bound = reference_and_bound(x, w, None)
    assert bound[0, :, :, :7].max() < 1e-5 * bound[0, :, :, 28:].max()
    got = _run(x, w, None)
    _report("stem_conv_pool_f32, halves 10^6 apart", got, ref, bound, x, w, None)
    print(f"  its dim tile column alone: worst |err| / bound = {_ratio(got[..., :7], ref[..., :7], bound[..., :7]):.4f}, "
          f"largest bound {bound[..., :7].max().item():.3g} against {bound[..., 28:].max().item():.3g} in the bright one")


def test_non_finite_pixels_spoil_exactly_the_outputs_of_the_reference():
    x, w, b = _operands(PARTIAL)
    x = x.clone()
    x[0, 1, 5, 7], x[0, 2, 30, 40], x[1, 0, 20, 20] = INF, -INF, NAN
    ref, bound = reference_and_bound(x, w, b)
    assert torch.isnan(ref).any() and torch.isinf(ref).any() and torch.isfinite(ref).any()
    for layout in ("nchw", "crop"):
        got = _run(x, w, b, layout)
        assert torch.equal(torch.isfinite(got), torch.isfinite(ref))
        compare(got, ref, bound, f"stem_conv_pool_f32 with Inf / NaN pixels, {layout}")


def test_supported_gate_and_weight_cache():
    x, w, _ = _operands(PARTIAL)
    xg, wg = x.to(DEV), w.to(DEV)
    with torch.no_grad():
        assert alo_hip.stem_conv_pool_f32_supported(xg, wg) and not alo_hip.stem_conv_pool_supported(xg, wg)
        assert not alo_hip.stem_conv_pool_f32_supported(xg.bfloat16(), wg.bfloat16()) and not alo_hip.stem_conv_pool_f32_supported(x, w)
        y0 = alo_hip.stem_conv_pool_f32(xg, wg)
        pack = wg.__dict__["_alo_derived"]["stem_f32_b"][1]
        alo_hip.stem_conv_pool_f32(xg, wg)
        assert wg.__dict__["_alo_derived"]["stem_f32_b"][1] is pack
        wg.mul_(2.0)                                                # a new version: re-derived
        y1 = alo_hip.stem_conv_pool_f32(xg, wg)
    assert wg.__dict__["_alo_derived"]["stem_f32_b"][1] is not pack
    assert torch.equal(y1, 2.0 * y0)                                # a power of two moves the exponents only
    assert alo_hip.stem_conv_pool_f32_supported(xg, wg)             # grad mode on, nothing requires grad
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.stem_conv_pool_f32(xg, wg.clone().requires_grad_())


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r50():
    import aloscene
    from alonet.deformable_detr import DeformableDetrR50

    torch.manual_seed(0)
    model = DeformableDetrR50(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval()
    gen = torch.Generator().manual_seed(0)
    frames = [aloscene.Frame(torch.rand(3, 192, 256, generator=gen) * 255, normalization="255").norm_resnet() for _ in range(2)]
    return model, aloscene.Frame.batch_list(frames).to(DEV)


def _stem_output(model, frames):
    """(what layer1 receives, {tag: calls}) of one forward."""
    body = model.backbone[0].body
    seen = []
    handle = body.layer1[0].register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    try:
        with alo_hip.LaunchTimer() as timer, torch.no_grad():
            model(frames)
    finally:
        handle.remove()
    return seen[0], {tag: v["calls"] for tag, v in timer.summary().items()}


def test_backbone_stem_on_the_kernel_matches_the_default_route(r50, monkeypatch):
    """The kernel in the backbone's place for it, whatever the routing table says: layer1's input against the default route's, within
    the kernel's bound + the stock fp32 ops' own error (the same bound: c_acc is what an fp32 dot product is allowed)."""
    model, frames = r50
    monkeypatch.delenv(KNOB, raising=False)
    want, tags = _stem_output(model, frames)
    assert TAG not in tags
    monkeypatch.setenv(KNOB, "split")
    monkeypatch.setattr(alo_hip, "STEM_F32_ROUTED", True)
    got, tags = _stem_output(model, frames)
    assert tags.get(TAG) == 1, tags
    body = model.backbone[0].body
    from alonet.detr.backbone import folded_conv_bn
    w, b = folded_conv_bn(body.conv1, body.bn1)
    ref, bound = reference_and_bound(frames.as_tensor().float().cpu(), w.float().cpu().contiguous(), b.float().cpu())
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    r_kernel = compare(got.cpu(), ref, bound, "the backbone's stem on stem_conv_pool_f32")
    r_stock = _ratio(want.cpu(), ref, bound)
    print(f"layer1's input at 2 x 192 x 256 against fp64, worst |err| / bound: kernel {r_kernel:.4f}, default route {r_stock:.4f}; "
          f"max |kernel - default| = {(got - want).abs().max().item():.3g} (max |value| {want.abs().max().item():.3g})")


def test_launch_tag_follows_the_switch_and_the_measurement(r50, monkeypatch):
    model, frames = r50
    monkeypatch.delenv(KNOB, raising=False)
    assert TAG not in _stem_output(model, frames)[1]
    monkeypatch.setenv(KNOB, "split")
    tags = _stem_output(model, frames)[1]
    if alo_hip.STEM_F32_ROUTED:
        assert tags.get(TAG) == 1, tags
        assert not any(tag.startswith(("conv3x3/", "linear_packed", "linear_shortk", "conv1x1_strided/")) for tag in tags)
    else:
        assert TAG not in tags, tags                                # measured to lose (alo_hip.STEM_F32_ROUTED): the stock ops
    half = copy.deepcopy(model).to(torch.bfloat16)
    for value in (None, "split"):
        monkeypatch.delenv(KNOB, raising=False)
        if value:
            monkeypatch.setenv(KNOB, value)
        with alo_hip.LaunchTimer() as timer, torch.no_grad():
            half(frames.to(torch.bfloat16))
        tags = timer.summary()
        assert TAG not in tags and "stem_conv_pool" in tags, sorted(tags)


def test_graphed_forward_with_the_stem_kernel_replays_eager_bit_for_bit(r50, monkeypatch):
    from alonet.common import GraphedForward

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model, frames = r50
    monkeypatch.setenv(KNOB, "split")
    monkeypatch.setattr(alo_hip, "STEM_F32_ROUTED", True)
    graphed = GraphedForward(model)
    with torch.no_grad():
        model(frames)
        want = model(frames)
        got = graphed(frames)
        again = graphed(frames)
    for key in ("pred_logits", "pred_boxes"):
        assert torch.equal(got[key], want[key]) and torch.equal(again[key], want[key]), key
    assert len(graphed._graphs) == 1
