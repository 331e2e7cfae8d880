"""conv1x1_chain_l2_kernel (csrc/conv1x1_chain_l2.hip; alo_conv1x1_nhwc with a chain buffer at Cin = 128, Cout = 512): a layer2
bottleneck's conv3 with its downsample convolution folded in (DOWN, stride 1 or 2, 256 input channels) or its identity given (RES), and
optionally the next bottleneck's conv1 (NEXT, 512 -> 128) made from the tile of the result while it is on chip.

Every intermediate is rounded where the separate launches round it, so every case here is exact (torch.equal on the bit patterns)
against those launches, composed as alonet/detr/backbone.py composes them with ``ALO_BOTTLENECK_CHAIN=off``:

    identity = conv1x1_strided(x0, wd, bd, 2)  or  linear_shortk(x0, wd, bd)     (DOWN, stride 2 / 1; given for RES)
    y        = linear_shortk(mid, w3, b3, relu=True, residual=identity)
    z        = linear_packed(y, w1, b1, relu=True)                                (NEXT)

over one tile, ragged tiles, and one M at which a persistent workgroup walks more than two tiles with a ragged end: launch_chain2
starts gx = min(256, ceil(M / 64)) workgroups, workgroup b takes tiles b, b + gx, ..., so M = 64 * (2 * 256) + 37 = 32805 rows.
Identities and x0 are distinct in every row (checked): a tile or row mix-up cannot pass.
"""
import os

import pytest
import torch

import alo_hip
from guarded import GuardedLaunches

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
GRID = 256                                # launch_chain2: at most this many persistent workgroups
LONG_M = 64 * (2 * GRID) + 37
KINDS = ("down1", "down2", "res")         # the downsample convolution at stride 1 and 2, the identity given
WIDTHS = (0, 128)                         # channels of the next convolution; 0: none
FORMS = [(k, n2) for k in KINDS for n2 in WIDTHS]
NAN, INF = float("nan"), float("inf")


def rows_as_map(t):
    """(M, C) rows -> the channels-last (1, C, 1, M) map that holds them."""
    return t.view(1, 1, t.shape[0], t.shape[1]).permute(0, 3, 1, 2)


def map_as_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def distinct_rows(t, g):
    key = t.double() @ torch.randn(t.shape[1], device=DEV, generator=g, dtype=torch.float64)
    return torch.unique(key).numel() == t.shape[0]


def make_case(shape, n2, seed):
    """``shape`` = (N, Ho, Wo) of mid and y, or a row count M for (1, 1, M).  ``x0_s2`` is the (N, 256, 2 Ho - 1, 2 Wo - 1) map whose
    stride-2 pixels are ``x0``'s rows; every pixel the stride skips is NaN."""
    n, ho, wo = (1, 1, shape) if isinstance(shape, int) else shape
    m = n * ho * wo
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rand(*shape, scale=1.0):
        return (scale * torch.randn(*shape, device=DEV, generator=g)).to(BF16)

    c = dict(dims=(n, ho, wo), mid=rand(m, 128), x0=rand(m, 256), identity=rand(m, 512), w3=rand(512, 128, scale=0.09), b3=rand(512, scale=0.5),
             wd=rand(512, 256, scale=0.0625), bd=rand(512, scale=0.5))
    if n2:
        c.update(w1=rand(n2, 512, scale=0.044), b1=rand(n2, scale=0.5))
    assert distinct_rows(c["identity"], g) and distinct_rows(c["x0"], g)
    full = torch.full((n, 2 * ho - 1, 2 * wo - 1, 256), NAN, device=DEV, dtype=BF16)
    full[:, ::2, ::2] = c["x0"].view(n, ho, wo, 256)
    c["x0_s2"] = full.permute(0, 3, 1, 2)   # channels-last (N, 256, H, W)
    return c


def as_map(c, rows):
    n, ho, wo = c["dims"]
    return rows.view(n, ho, wo, rows.shape[1]).permute(0, 3, 1, 2)


def separate_launches(c, kind, n2):
    if kind == "down2":
        identity = map_as_rows(alo_hip.conv1x1_strided(c["x0_s2"], c["wd"], c["bd"], 2))
    else:
        identity = alo_hip.linear_shortk(c["x0"], c["wd"], c["bd"]) if kind == "down1" else c["identity"]
    y = alo_hip.linear_shortk(c["mid"], c["w3"], c["b3"], relu=True, residual=identity)
    return y, (alo_hip.linear_packed(y, c["w1"], c["b1"], relu=True) if n2 else None)


def chain(c, kind, n2):
    down = {"down1": (as_map(c, c["x0"]), c["wd"], c["bd"]), "down2": (c["x0_s2"], c["wd"], c["bd"], 2), "res": None}[kind]
    y, z = alo_hip.conv1x1_chain(as_map(c, c["mid"]), (c["w3"], c["b3"]), identity=as_map(c, c["identity"]) if kind == "res" else None,
                                 down=down, nxt=(c["w1"], c["b1"]) if n2 else None)
    return map_as_rows(y), (None if z is None else map_as_rows(z))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def check_exact(c, kind, n2, what):
    with torch.no_grad():
        want_y, want_z = separate_launches(c, kind, n2)
        got_y, got_z = chain(c, kind, n2)
    for name, got, want in (("y", got_y, want_y), ("z", got_z, want_z)):
        if want is None:
            assert got is None
            continue
        if not same_bits(got, want):
            bad = (got.contiguous().view(torch.int16) != want.view(torch.int16)).any(dim=1).nonzero().flatten()
            raise AssertionError(f"{what}: {name} differs in {bad.numel()} rows, first {bad[:8].tolist()}")
    return got_y, got_z


def test_the_long_case_walks_more_than_two_tiles_with_a_ragged_end():
    tiles = -(-LONG_M // 64)
    assert tiles == 2 * GRID + 1 and LONG_M % 64 != 0


# ---- 1. every built form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 200, LONG_M])
@pytest.mark.parametrize("kind,n2", FORMS)
def test_chain_equals_the_launches_it_replaces(kind, n2, m):
    check_exact(make_case(m, n2, 3 * m + n2 + KINDS.index(kind)), kind, n2, f"{kind} next={n2} M={m}")


# ---- 2. stride-2 addressing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 2, 2), (2, 5, 7), (3, 9, 13)])
@pytest.mark.parametrize("n2", WIDTHS)
def test_stride_2_reads_the_kept_pixels_only(n2, n, h, w):
    """x0's map is (N, H, W): every kept pixel distinct, every skipped one NaN.  An even H or W leaves a last row or column that the
    stride never reaches, as layer2.0 has at the headline (200 x 334 -> 100 x 167)."""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    c = make_case((n, ho, wo), n2, 11 * h + w + n2)
    full = torch.full((n, h, w, 256), NAN, device=DEV, dtype=BF16)
    full[:, ::2, ::2] = c["x0"].view(n, ho, wo, 256)
    c["x0_s2"] = full.permute(0, 3, 1, 2)
    assert c["x0_s2"].shape == (n, 256, h, w) and int(torch.isnan(c["x0_s2"][:, 0]).sum()) == n * (h * w - ho * wo)
    got_y, got_z = check_exact(c, "down2", n2, f"stride 2 on {n} x {h} x {w} next={n2}")
    assert got_y.shape == (n * ho * wo, 512) and not torch.isnan(got_y).any() and (got_z is None or not torch.isnan(got_z).any())


# ---- 3. non-finite inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n2", FORMS)
def test_nan_and_inf_travel_as_in_the_separate_launches(kind, n2):
    """NaN, +Inf and -Inf in mid and in the identity / x0, in all three tiles of workgroup 0's walk (tiles 0, 256 and the ragged 512):
    compared on the bit patterns (ReLU keeps NaN), and the rows next to the planted ones stay finite."""
    m = LONG_M
    c = make_case(m, n2, 77 + n2 + KINDS.index(kind))
    rows = [21, 64 * GRID + 21, 64 * (2 * GRID) + 3, m - 1]
    other, col = ("identity", 70) if kind == "res" else ("x0", 70)
    for i, value in zip(rows, (NAN, INF, -INF, NAN)):
        c["mid"][i, 7] = value
        j = i + 1 if i + 1 < m else i - 1
        c[other][j, col] = value
        if kind == "down2":
            c["x0_s2"][0, col, 0, 2 * j] = value
    got_y, got_z = check_exact(c, kind, n2, f"{kind} next={n2} non-finite")
    assert torch.isnan(got_y[21]).all() and torch.isnan(got_y[m - 1]).all() and not torch.isnan(got_y[20]).any()
    hit = torch.zeros(m, dtype=torch.bool, device=DEV)
    for i in rows:
        hit[i] = True
        hit[i + 1 if i + 1 < m else i - 1] = True
    assert bool(torch.isfinite(got_y[~hit].float()).all()) and (got_z is None or bool(torch.isfinite(got_z[~hit].float()).all()))
    assert not bool(torch.isfinite(got_y[rows].float()).all(dim=1).any())   # a non-finite value in mid reaches columns of both signs


# ---- 4. buffers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n2", FORMS)
def test_chain_stays_in_its_buffers_and_ignores_stale_bytes(kind, n2):
    """Guarded buffers with poisoned slack either side of every input and output, the output pre-filled with stale bytes, twice with
    different fills (tests/guarded.py); M = 200: three full tiles and a ragged fourth, whose missing rows are read from the last row
    and never stored."""
    c = make_case(200, n2, 5 + n2)
    with torch.no_grad():
        want_y, want_z = separate_launches(c, kind, n2)
        with GuardedLaunches() as g:
            got_y, got_z = chain(c, kind, n2)
    # the chain buffer is made by this first call: Wd and W1 are packed into it (one guarded alo_pack_mfma_b launch each), then the chain
    packs = (kind != "res") + (n2 != 0)
    assert [symbol for symbol, _ in g.seen] == ["alo_pack_mfma_b"] * packs + ["alo_conv1x1_nhwc"]
    assert g.seen[-1][1].startswith("bottleneck_chain/C=128/")
    assert same_bits(got_y, want_y) and (want_z is None or same_bits(got_z, want_z))


def test_the_gate_and_the_wrapper_refuse_what_the_kernel_does_not_serve(monkeypatch):
    c = make_case(65, 128, 1)
    mid, idn, x0 = rows_as_map(c["mid"]), rows_as_map(c["identity"]), rows_as_map(c["x0"])
    conv3, nxt = (c["w3"], c["b3"]), (c["w1"], c["b1"])
    ok = alo_hip.conv1x1_chain_supported
    with torch.no_grad():
        assert ok(mid, conv3, identity=idn, nxt=nxt) and ok(mid, conv3, down=(x0, c["wd"], c["bd"]))
        assert ok(mid, conv3, down=(c["x0_s2"], c["wd"], c["bd"], 2), nxt=nxt)
        assert not ok(mid, conv3, down=(c["x0_s2"], c["wd"], c["bd"], 1))   # the map does not have mid's size at stride 1
        assert not ok(mid, conv3, down=(x0, c["wd"], c["bd"], 3))
        assert not ok(mid, conv3, identity=idn, nxt=(torch.zeros(64, 512, device=DEV, dtype=BF16), torch.zeros(64, device=DEV, dtype=BF16)))
        assert not ok(mid, conv3, identity=idn[:, :256])
        assert not ok(mid, conv3, down=(x0[:, :64], c["wd"][:, :64].contiguous(), c["bd"]))   # layer1's downsample width
        monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", "off")
        assert not ok(mid, conv3, identity=idn, nxt=nxt)
        monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", "layer1")   # the knob routes; the wrapper still serves every built form
        assert ok(mid, conv3, identity=idn, nxt=nxt) and not alo_hip.bottleneck_chain_routed(128, False, 128)
        assert alo_hip.bottleneck_chain_routed(64, True, 64)
        monkeypatch.delenv("ALO_BOTTLENECK_CHAIN")
        buf = torch.cat([c["w3"].reshape(-1), c["b3"]])
        with pytest.raises(RuntimeError, match="overlaps"):
            alo_hip._launch("alo_conv1x1_nhwc", mid.device, None, 0.0, 0.0, mid, buf, alo_hip.CONV1X1_CHAIN, None, idn, idn, 1, 1, 65, 128, 512,
                            1, 1, alo_hip.ALO_BF16)


# ---- 5. the backbone -----------------------------------------------------------------------------------------------------------------
STAGES = {"layer1": "0", "layer2": "1", "layer3": "2", "layer4": "3"}
PREFIX = "bottleneck_chain/C=128/"
# layer2.0 folds its stride-2 downsample and layer2.1's conv1; layer2.1 and layer2.2 hand their tile to the next block's conv1; layer2.3,
# the last block of its stage, hands nothing on
ROUTED_TAGS = {PREFIX + "down+next128": 1, PREFIX + "res+next128": 2}
INPUTS = {"72x104": (2, 3, 72, 104), "64x96": (2, 3, 64, 96)}


class knob:
    """``ALO_BOTTLENECK_CHAIN`` set to ``value`` (None: unset) for a block, then put back."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("ALO_BOTTLENECK_CHAIN")
        if self.value is None:
            os.environ.pop("ALO_BOTTLENECK_CHAIN", None)
        else:
            os.environ["ALO_BOTTLENECK_CHAIN"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ALO_BOTTLENECK_CHAIN", None)
        else:
            os.environ["ALO_BOTTLENECK_CHAIN"] = self.old


@pytest.fixture(scope="module")
def body():
    import alonet.detr.backbone as bb

    torch.manual_seed(0)
    body = bb.ResNetBody("resnet50", return_layers=STAGES).to(DEV).eval()
    for m in body.modules():  # non-trivial frozen statistics
        if hasattr(m, "running_var"):
            m.running_var.uniform_(0.5, 2.0); m.running_mean.normal_(0, 0.2); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    return body.to(BF16)


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator(device=DEV).manual_seed(4)
    return {k: torch.randn(*shape, device=DEV, generator=g).to(BF16) for k, shape in INPUTS.items()}


@pytest.fixture(scope="module")
def separate_stages(body, inputs):
    """Every stage with ``ALO_BOTTLENECK_CHAIN=off`` for both inputs, and the launch tags: computed once, left unchanged."""
    out = {}
    with knob("off"), torch.no_grad():
        for k, x in inputs.items():
            with alo_hip.LaunchTimer() as t:
                stages = {name: v.clone() for name, v in body(x).items()}
            out[k] = (stages, {tag: d["calls"] for tag, d in t.summary().items()})
    return out


def assert_same_stages(got, want):
    assert got.keys() == want.keys() and len(want) == 4
    for k in want:
        assert got[k].shape == want[k].shape and bool(torch.isfinite(want[k].float()).all())
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("which", list(INPUTS))
def test_resnet_body_default_equals_layer1_equals_off(body, inputs, separate_stages, which):
    x = inputs[which]
    want, off_calls = separate_stages[which]
    calls = {}
    for value in (None, "layer1"):
        with knob(value), alo_hip.LaunchTimer() as t, torch.no_grad():
            got = body(x)
        calls[value] = {tag: d["calls"] for tag, d in t.summary().items()}
        assert_same_stages(got, want)
    # off: the four conv3 launches with the identity in their epilogue, the strided downsample, three conv1 launches; no chain at all
    assert off_calls["linear_shortk/N=512,K=128"] == 4 and off_calls["linear_packed/K=512/N=128"] == 3
    assert off_calls["conv1x1_strided/K=256/N=512"] == 1
    assert not any(tag.startswith(("conv1x1_chain", "bottleneck_chain")) for tag in off_calls)
    # layer1: the routing before layer2 had a chain
    assert not any(tag.startswith("bottleneck_chain") for tag in calls["layer1"])
    assert calls["layer1"]["linear_shortk/N=512,K=128"] == 4 and calls["layer1"]["linear_packed/K=512/N=128"] == 3
    assert [tag for tag in calls["layer1"] if tag.startswith("conv1x1_chain")] == [tag for tag in calls[None] if tag.startswith("conv1x1_chain")]
    # default: the routed forms, layer2.3's plain launch, and no conv1 launch of layer2 left
    assert {tag: n for tag, n in calls[None].items() if tag.startswith("bottleneck_chain")} == ROUTED_TAGS
    assert calls[None]["linear_shortk/N=512,K=128"] == 1
    assert "linear_packed/K=512/N=128" not in calls[None] and "conv1x1_strided/K=256/N=512" not in calls[None]


def test_resnet_body_under_graph_capture_and_two_replays(body, inputs, separate_stages):
    x = inputs["72x104"]
    want, _ = separate_stages["72x104"]
    with knob(None):
        static_x = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            body(static_x)   # derived tensors (folded weights, the chain buffers) are made here, outside the graph
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = body(static_x)
        for _ in range(2):
            static_x.zero_()
            graph.replay()   # on zeros in between: a replay that kept the old outputs would pass otherwise
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert_same_stages(out, want)


def test_a_swapped_conv_bn_is_handed_every_convolution(body, inputs, separate_stages, monkeypatch):
    import alonet.detr.backbone as bb

    x = inputs["72x104"]
    want, _ = separate_stages["72x104"]
    conv_bn, seen = bb.conv_bn, []

    def counting_conv_bn(x, conv, bn, relu=False, residual=None):
        seen.append(residual is not None)
        return conv_bn(x, conv, bn, relu=relu, residual=residual)

    monkeypatch.setattr(bb, "conv_bn", counting_conv_bn)
    with knob(None), alo_hip.LaunchTimer() as t, torch.no_grad():
        got = body(x)
    assert not any(tag.startswith(("conv1x1_chain", "bottleneck_chain")) for tag in t.summary())
    assert sum(seen) == 16 and len(seen) in (52, 53)   # 3 * 16 + 4 downsamples, and the stem where it is not fused with its max-pool
    assert_same_stages(got, want)


def test_with_grad_enabled_the_separate_launches_run_and_gradients_reach_the_weights(body):
    block, nxt = body.layer2[0], body.layer2[1]
    xin = torch.randn(2, 256, 18, 26, device=DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    params = [block.conv3.weight, block.downsample[0].weight, nxt.conv1.weight]
    try:
        for p in params:
            p.requires_grad_(True)
        with knob(None), alo_hip.LaunchTimer() as t:
            y, head = block(xin, nxt=nxt)
            assert head is None and y.requires_grad
            out = nxt(y)
        assert not any(tag.startswith("bottleneck_chain") for tag in t.summary())
        out.float().square().mean().backward()
        for p in params:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    finally:
        for p in params:
            p.requires_grad_(False)
            p.grad = None


# ---- 6. a layer2 bottleneck alone ----------------------------------------------------------------------------------------------------
def test_a_layer2_bottleneck_alone_gives_the_same_result(body):
    """``Bottleneck.forward(x)`` without the hand-off: layer2.0 still folds its stride-2 downsample convolution (an odd and an even map
    side), layer2.1 has nothing to fold."""
    x = torch.randn(2, 256, 18, 27, device=DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        with knob("off"):
            want0 = body.layer2[0](x)
            want1 = body.layer2[1](want0)
        with knob(None), alo_hip.LaunchTimer() as t:
            got0 = body.layer2[0](x)
            got1 = body.layer2[1](got0)
            y, head = body.layer2[0](x, nxt=body.layer2[1])
            got1_handed = body.layer2[1](y, head=head)
    assert {tag: d["calls"] for tag, d in t.summary().items() if tag.startswith("bottleneck_chain")} == {
        PREFIX + "down": 1, PREFIX + "down+next128": 1}
    assert head is not None and want0.shape == (2, 512, 9, 14)
    assert torch.equal(got0, want0) and torch.equal(y, want0) and torch.equal(got1, want1) and torch.equal(got1_handed, want1)
