"""alo_hip.ffn_f32 (alo_ffn256 with dtype = ALO_F32, aloception-oss_amd/csrc/ffn_f32.hip) against the fp64 block of the same fp32
operands, per output element, within the bound derived in ffn_f32_ref.py — which test_ffn_f32_cpu.py holds the numpy restatement of
the kernel's arithmetic to, so what is asked of the kernel here has been checked without a GPU; against the two linear_f32 launches it
replaces; and wired into the transformer's feed-forward block behind ``ALO_F32_LAYERS=split``."""
import functools

import pytest
import torch

import alo_hip
import guarded
from ffn_f32_ref import MANY_TILES, SCALES, SHAPES, dim_rows, operands, reference_and_bound
from kernel_bounds import INF, NAN, compare
from test_f32_split_route_gpu import KNOB, _g14b_errors
from test_linear_f32_cpu import numpy_split_packed

pytestmark = pytest.mark.gpu
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(shape, scale, bias):
    """Operands, fp64 reference and bound of one case, on the CPU: made once, never written to."""
    x, w1, b1, w2, b2 = operands(shape, scale)
    b1, b2 = (b1, b2) if bias else (None, None)
    return (x, w1, b1, w2, b2) + reference_and_bound(x, w1, b1, w2, b2)


def _run(x, w1, b1, w2, b2):
    dev = lambda a: None if a is None else a.cuda()  # noqa: E731
    with torch.no_grad():
        y = alo_hip.ffn_f32(dev(x), dev(w1), dev(b1), dev(w2), dev(b2))
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == x.shape
    return y.cpu()


def _hold(shape, scale, bias):
    x, w1, b1, w2, b2, ref, bound = _case(shape, scale, bias)
    got = _run(x, w1, b1, w2, b2)
    ratio = compare(got, ref, bound, f"ffn_f32 {shape} scale={scale} bias={bias}")
    print(f"ffn_f32 {shape} scale={scale} bias={bias}: worst |err| / bound = {ratio:.4f}, "
          f"max |err| / max |ref| = {((got.double() - ref).abs().max() / ref.abs().max()).item():.3g}")
    return got


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernel_meets_the_bound(shape, bias):
    if shape[0] == MANY_TILES:      # the launch arithmetic of ffn_f32.hip: one workgroup per CU, at most 256
        assert (shape[0] + 63) // 64 > 256
    _hold(shape, 1.0, bias)


@pytest.mark.parametrize("scale", SCALES)
def test_kernel_meets_the_bound_at_any_input_magnitude(scale):
    _hold((63, 512), scale, True)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernel_is_as_accurate_as_the_two_launches_it_replaces(shape):
    """Largest error against fp64 at most 2 x that of linear_f32(relu=True) followed by linear_f32 on the same operands: both are sums
    of the same order and number of fp32 roundings, a factor 2 covers the different association, and a dropped cross product or a
    wrong exponent shows as >= 2^-11 relative, thousands of times larger."""
    x, w1, b1, w2, b2, ref, _ = _case(shape, 1.0, True)
    got = _run(x, w1, b1, w2, b2)
    with torch.no_grad():
        h = alo_hip.linear_f32(x.cuda(), w1.cuda(), b1.cuda(), relu=True)
        two = alo_hip.linear_f32(h, w2.cuda(), b2.cuda()).cpu()
    err, err_two = (got.double() - ref).abs().max().item(), (two.double() - ref).abs().max().item()
    print(f"ffn_f32 {shape}: max |err| {err:.3g}, two linear_f32 launches {err_two:.3g} (max |ref| {ref.abs().max().item():.3g})")
    assert err <= 2 * err_two, (shape, err, err_two)


def test_a_dim_row_and_a_dim_chunk_keep_their_accuracy_and_their_bits():
    x, w1, b1, w2, b2 = dim_rows()
    ref, bound = reference_and_bound(x, w1, b1, w2, b2)
    got = _run(x, w1, b1, w2, b2)
    ratio = compare(got, ref, bound, "ffn_f32 with a row and a hidden chunk 10^6 dimmer")
    print(f"ffn_f32 dim row / dim chunk: worst |err| / bound = {ratio:.4f}")
    for row in (70, 3):           # the dim row of x; a row among bright ones whose second hidden chunk is dim
        alone = _run(x[row:row + 1], w1, b1, w2, b2)
        assert torch.equal(alone[0], got[row]), f"row {row}'s result depends on its neighbours"


@pytest.mark.parametrize("shape", [(65, 256), (130, 1024)], ids=ids)
def test_non_finite_inputs_spoil_exactly_their_rows(shape):
    x, w1, b1, w2, b2, _, _ = _case(shape, 1.0, True)
    clean = _run(x, w1, b1, w2, b2)
    x = x.clone()
    x[2, 5], x[40, 77], x[11] = INF, -INF, NAN      # single elements, and a whole row
    ref, bound = reference_and_bound(x, w1, b1, w2, b2)
    assert not torch.isfinite(ref[[2, 40, 11]]).any() and torch.isnan(ref[11]).all()
    got = _run(x, w1, b1, w2, b2)
    compare(got, ref, bound, f"ffn_f32 {shape} with Inf / NaN inputs")
    spoiled = torch.zeros(shape[0], dtype=torch.bool)
    spoiled[[2, 40, 11]] = True
    assert not torch.isfinite(got[spoiled]).any() and torch.isnan(got[11]).all()
    assert torch.equal(got[~spoiled], clean[~spoiled]), "a non-finite row changed another row's bits"


def test_two_calls_give_equal_bits_and_split_weights_follow_the_weight():
    x, w1, b1, w2, b2 = operands((130, 1024))
    block = torch.nn.Sequential(torch.nn.Linear(256, 1024), torch.nn.Linear(1024, 256)).cuda().requires_grad_(False)
    l1, l2 = block
    xg = x.cuda()
    with torch.no_grad():
        for p, v in ((l1.weight, w1), (l1.bias, b1), (l2.weight, w2), (l2.bias, b2)):
            p.copy_(v)
        run = lambda: alo_hip.ffn_f32(xg, l1.weight, l1.bias, l2.weight, l2.bias)  # noqa: E731
        y0 = run()
        packs = [w.__dict__["_alo_derived"]["linear_f32_b"][1] for w in (l1.weight, l2.weight)]
        assert torch.equal(packs[0].cpu(), numpy_split_packed(w1)) and torch.equal(packs[1].cpu(), numpy_split_packed(w2))
        assert torch.equal(run(), y0)
        assert all(w.__dict__["_alo_derived"]["linear_f32_b"][1] is p for w, p in zip((l1.weight, l2.weight), packs))
        # the derived copy is linear_f32's own: one split per weight, whichever kernel asks
        assert alo_hip.linear_f32(xg, l1.weight) is not None and l1.weight.__dict__["_alo_derived"]["linear_f32_b"][1] is packs[0]
        l2.weight.data.mul_(2.0)                     # through .data: no version bump, the split copy is stale ...
        l2.bias.data.mul_(2.0)
        stale = run()
        alo_hip.invalidate_caches(block)             # ... until the caches are dropped
        y1 = run()
        assert torch.equal(y1, 2.0 * y0) and not torch.equal(stale, y1)      # a power of two moves the exponents only
        l2.weight.mul_(0.5)                          # a new version: re-derived without being asked
        l2.bias.mul_(0.5)
        assert torch.equal(run(), y0)


def test_launches_stay_in_their_buffers_and_ignore_stale_bytes():
    assert guarded.ROLES["alo_ffn256"] == {5: guarded.OUT}
    with guarded.GuardedLaunches() as g:
        for shape in ((1, 256), (65, 256), (130, 1024)):
            _hold(shape, 1.0, True)
        _hold((65, 256), 1.0, False)
    tags = [tag for _, tag in g.seen if tag is not None]
    assert tags.count("ffn_f32/F=256") == 3 and tags.count("ffn_f32/F=1024") == 1
    assert {s for s, _ in g.seen} == {"alo_ffn256", "alo_pack_mfma_b"}


# ---- wiring -----------------------------------------------------------------------------------------------------------------------
class _EveryShape(dict):
    """A route table that admits every (F, M): the wiring does not depend on where the kernel was measured to win."""

    def get(self, key, default=None):
        return (0, None)


def _ffn_calls(tags):
    return sum(n for tag, n in tags.items() if tag.startswith("ffn_f32/"))


def test_g14b_fp32_takes_the_kernel_on_the_split_route_and_matches_the_reference(golden, monkeypatch):
    monkeypatch.setattr(alo_hip, "_FFN_F32_ROUTED", _EveryShape())
    monkeypatch.delenv(KNOB, raising=False)
    l0, b0, tags0 = _g14b_errors(golden, torch.float32)
    monkeypatch.setenv(KNOB, "split")
    l1, b1, tags1 = _g14b_errors(golden, torch.float32)
    print(f"G14b fp32 max-abs against the reference (logits, boxes): switch unset ({l0:.3g}, {b0:.3g}), set with ffn_f32 ({l1:.3g}, {b1:.3g}); "
          f"ffn_f32 launches: {({t: n for t, n in tags1.items() if t.startswith('ffn_f32/')})}")
    assert _ffn_calls(tags0) == 0 and _ffn_calls(tags1) > 0, (tags0, tags1)
    assert l1 <= 1e-3 and b1 <= 1e-3, (l1, b1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_other_dtypes_ignore_the_switch_and_the_table(golden, monkeypatch, dtype):
    monkeypatch.delenv(KNOB, raising=False)
    _, _, tags0 = _g14b_errors(golden, dtype)
    monkeypatch.setattr(alo_hip, "_FFN_F32_ROUTED", _EveryShape())
    monkeypatch.setenv(KNOB, "split")
    _, _, tags1 = _g14b_errors(golden, dtype)
    assert tags1 == tags0 and _ffn_calls(tags1) == 0, (tags0, tags1)
