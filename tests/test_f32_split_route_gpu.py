"""``ALO_F32_LAYERS=split``: the opt-in route on which the fp32 detector's linear layers, 1x1 and 3x3 convolutions take the split
kernels (alo_hip.linear_f32, conv1x1_strided_f32, conv3x3_f32: fp32 on the fp16 matrix cores).  The default route is held to
launching and computing what it did before the route existed, and bf16 / fp16 models to ignoring the switch."""
import numpy as np
import pytest
import torch

import alo_hip
import aloscene
import test_models_golden_cpu as M
from alonet.deformable_detr import DeformableDetrR50

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "ALO_F32_LAYERS"
SPLIT_TAGS = ("linear_f32", "conv1x1_strided_f32", "conv3x3_f32")


def _frames(sizes, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [aloscene.Frame(torch.rand(3, h, w, generator=gen) * 255, normalization="255").norm_resnet() for h, w in sizes]


def _forward(model, frames):
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = model(frames)
    return (out["pred_logits"].float().cpu(), out["pred_boxes"].float().cpu()), {tag: v["calls"] for tag, v in timer.summary().items()}


def _split_calls(tags):
    return {name: sum(n for tag, n in tags.items() if tag.split("/")[0] == name) for name in SPLIT_TAGS}


@pytest.fixture(scope="module")
def r50():
    torch.manual_seed(0)
    model = DeformableDetrR50(num_classes=91, aux_loss=False, device=torch.device(DEV)).eval()
    frames = [aloscene.Frame.batch_list(_frames([(192, 256), (160, 224)], seed)).to(DEV) for seed in (0, 1)]
    return model, frames


def test_fp32_detector_on_the_split_route_and_back(r50, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)   # MIOpen's default solvers do not all repeat themselves bit for bit
    model, (frames, _) = r50
    monkeypatch.delenv(KNOB, raising=False)
    _forward(model, frames)                                  # solver and algorithm choices are made on a shape's first call
    stock, tags = _forward(model, frames)
    assert _split_calls(tags) == dict.fromkeys(SPLIT_TAGS, 0), tags
    again, tags_again = _forward(model, frames)
    assert all(torch.equal(a, b) for a, b in zip(stock, again)) and tags_again == tags
    monkeypatch.setenv(KNOB, "split")
    _forward(model, frames)
    split, tags_split = _forward(model, frames)
    calls = _split_calls(tags_split)
    # ResNet-50: the three strided down-samples | 16 conv2 but layer3.0's (measured to lose: backbone.py) | every bottleneck's conv3
    # with its identity, and whichever other (K, N) alo_hip._F32_ROUTED holds, in the backbone and in the transformer
    assert calls["conv1x1_strided_f32"] == 3 and calls["conv3x3_f32"] == 15 and calls["linear_f32"] > 16, tags_split
    assert sum(n for tag, n in tags_split.items() if tag.startswith("linear_f32/K=256/N=256")) > 0, tags_split   # the transformer's
    assert not any(tag.startswith(("linear_packed", "linear_shortk", "conv1x1_strided/", "conv3x3/")) for tag in tags_split)
    for name, got, base in zip(("pred_logits", "pred_boxes"), split, stock):
        diff = (got - base).abs().max().item()
        print(f"{name}: split route against the default route, max |difference| {diff:.3g} (max |value| {base.abs().max().item():.3g})")
        assert torch.isfinite(got).all() and diff <= 1e-3 * max(1.0, base.abs().max().item()), (name, diff)
    monkeypatch.delenv(KNOB)
    back, tags_back = _forward(model, frames)
    assert all(torch.equal(a, b) for a, b in zip(stock, back)) and tags_back == tags


def _g14b_errors(golden, dtype, channels_last=False):
    g = golden("g14b_deformable_detr_d256.npz")
    model = M.build_g14b().to(DEV, dtype)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    frames = M.batch_from_raw(g, dtype=torch.float32).to(DEV).to(dtype)
    with torch.no_grad(), alo_hip.LaunchTimer() as timer:
        out = model(frames)
    levels = [out] + out["aux_outputs"]
    keys = [("d256.pred_logits", "d256.pred_boxes")] + [(f"d256.aux{i}.pred_logits", f"d256.aux{i}.pred_boxes")
                                                        for i in range(len(out["aux_outputs"]))]
    logits = max(float(np.abs(lvl["pred_logits"].double().cpu().numpy() - g[kl]).max()) for lvl, (kl, _) in zip(levels, keys))
    boxes = max(float(np.abs(lvl["pred_boxes"].double().cpu().numpy() - g[kb]).max()) for lvl, (_, kb) in zip(levels, keys))
    return logits, boxes, {tag: v["calls"] for tag, v in timer.summary().items()}


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "channels_last"])
def test_g14b_fp32_on_the_split_route_matches_the_reference(golden, monkeypatch, channels_last):
    """G14b at the fp32 bars of test_g14b_deformable_detr_d256_on_hip_matches_the_reference_model: logits and boxes within 1e-3 of the
    reference's outputs, every decoder level."""
    monkeypatch.delenv(KNOB, raising=False)
    l0, b0, tags0 = _g14b_errors(golden, torch.float32, channels_last)
    monkeypatch.setenv(KNOB, "split")
    l1, b1, tags1 = _g14b_errors(golden, torch.float32, channels_last)
    print(f"G14b fp32 max-abs against the reference (logits, boxes): switch unset ({l0:.3g}, {b0:.3g}), set ({l1:.3g}, {b1:.3g})")
    assert _split_calls(tags0)["linear_f32"] == 0 and _split_calls(tags1)["linear_f32"] > 0, (tags0, tags1)
    assert l1 <= 1e-3 and b1 <= 1e-3, (l1, b1)


def test_graphed_forward_on_the_split_route_replays_eager_bit_for_bit(r50, monkeypatch):
    from alonet.common import GraphedForward

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model, frames = r50
    monkeypatch.setenv(KNOB, "split")
    graphed = GraphedForward(model)
    with torch.no_grad():
        model(frames[0])
        for fr in frames:
            want = model(fr)
            got = graphed(fr)
            for key in ("pred_logits", "pred_boxes"):
                print(f"graph replay against eager, {key}: max |difference| {(got[key] - want[key]).abs().max().item():.3g}")
            for key in ("pred_logits", "pred_boxes"):
                assert torch.equal(got[key], want[key]), key
    assert len(graphed._graphs) == 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_other_dtypes_ignore_the_switch(golden, monkeypatch, dtype):
    monkeypatch.delenv(KNOB, raising=False)
    l0, b0, tags0 = _g14b_errors(golden, dtype)
    monkeypatch.setenv(KNOB, "split")
    l1, b1, tags1 = _g14b_errors(golden, dtype)
    assert tags1 == tags0 and _split_calls(tags1) == dict.fromkeys(SPLIT_TAGS, 0), (tags0, tags1)
