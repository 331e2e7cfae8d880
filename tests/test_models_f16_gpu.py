"""DeformableTransformer and the whole Deformable-DETR in fp16 on the GPU against the reference's own outputs, next to the bf16 run
of the same model in the same test: fp16 carries 11 significant bits against bf16's 8 at the same bytes, so its error must stay
within the bf16 path's stated bars and must not exceed the bf16 run's."""
import numpy as np
import pytest
import torch

import alo_hip
from test_models_cpu import build_g5_transformer
from test_models_gpu import BF16_MODEL_BOX_TOL, BF16_MODEL_LOGIT_TOL, BF16_TRANSFORMER_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = torch.from_numpy


def _transformer_errors(g, dtype):
    tr, L = build_g5_transformer(g)
    tr = tr.to(DEV, dtype).eval()
    cast = lambda a: t(a).to(DEV, dtype)  # noqa: E731
    srcs, poss = [cast(g[f"src{i}"]) for i in range(L)], [cast(g[f"pos{i}"]) for i in range(L)]
    masks = [t(g[f"mask{i}"]).to(DEV) for i in range(L)]
    with alo_hip.LaunchTimer() as timer, torch.no_grad():
        out = tr(srcs, masks, poss, cast(g["query_embed"]))
    errs = {"hs": np.abs(out["hs"].double().cpu().numpy() - g["hs"]).max(),
            "ref": np.abs(out["inter_references_out"].double().cpu().numpy() - g["inter_references_out"]).max()}
    for i in range(L):
        errs[f"memory{i}"] = np.abs(out["memory"][i].double().cpu().numpy() - g[f"memory{i}"]).max()
    return {k: float(v) for k, v in errs.items()}, set(k.split("/")[0] for k in timer.summary())


@pytest.mark.parametrize("fixture", ["g5_deformable_transformer.npz", "g12_deformable_transformer_d256.npz"])
def test_deformable_transformer_fp16_vs_reference_golden_and_vs_bf16(golden, fixture):
    g = golden(fixture)
    e16, tags16 = _transformer_errors(g, torch.float16)
    eb16, _ = _transformer_errors(g, torch.bfloat16)
    print(f"{fixture} max-abs vs the reference: fp16 {e16}")
    print(f"{fixture} max-abs vs the reference: bf16 {eb16}")
    assert "msda_fwd_fused" in tags16, tags16
    assert max(e16.values()) <= BF16_TRANSFORMER_TOL, e16
    for k in e16:
        assert e16[k] <= eb16[k], (k, e16[k], eb16[k])


def _g14b_errors(golden, dtype):
    import test_models_golden_cpu as M

    g = golden("g14b_deformable_detr_d256.npz")
    model = M.build_g14b().to(DEV, dtype)
    frames = M.batch_from_raw(g, dtype=torch.float32).to(DEV).to(dtype)
    with torch.no_grad(), alo_hip.LaunchTimer() as timer:
        out = model(frames)
    levels = [out] + out["aux_outputs"]
    keys = [("d256.pred_logits", "d256.pred_boxes")] + [(f"d256.aux{i}.pred_logits", f"d256.aux{i}.pred_boxes")
                                                        for i in range(len(out["aux_outputs"]))]
    logits = max(float(np.abs(lvl["pred_logits"].double().cpu().numpy() - g[kl]).max()) for lvl, (kl, _) in zip(levels, keys))
    boxes = max(float(np.abs(lvl["pred_boxes"].double().cpu().numpy() - g[kb]).max()) for lvl, (_, kb) in zip(levels, keys))
    return logits, boxes, set(k.split("/")[0] for k in timer.summary())


def test_g14b_whole_model_fp16_vs_reference_and_vs_bf16(golden):
    l16, b16, tags16 = _g14b_errors(golden, torch.float16)
    lb16, bb16, _ = _g14b_errors(golden, torch.bfloat16)
    l32, b32, _ = _g14b_errors(golden, torch.float32)
    print(f"G14b max-abs vs the reference (logits, boxes): fp16 ({l16:.5f}, {b16:.5f})  bf16 ({lb16:.5f}, {bb16:.5f})  fp32 ({l32:.2e}, {b32:.2e})")
    print("library launches in fp16:", sorted(tags16))
    assert "msda_fwd_fused" in tags16, tags16
    assert l16 <= BF16_MODEL_LOGIT_TOL and b16 <= BF16_MODEL_BOX_TOL, (l16, b16)
    assert l16 <= lb16 and b16 <= bb16, (l16, lb16, b16, bb16)
