"""conv1x1_chain_kernel (csrc/conv1x1_chain.hip; alo_conv1x1_nhwc with a chain buffer): a layer1 bottleneck's conv3 with its downsample
convolution folded in (DOWN) or its identity given (RES), and optionally the next bottleneck's conv1 (NEXT, 64 or 128 channels) made from
the tile of the result while it is on chip.

Every intermediate is rounded where the separate launches round it, so every case here is exact (torch.equal) against those launches,
composed as alonet/detr/backbone.py composes them with ``ALO_BOTTLENECK_CHAIN=off``:

    identity = linear_shortk(x0, wd, bd)                                   (DOWN; given for RES)
    y        = linear_shortk(mid, w3, b3, relu=True, residual=identity)
    z        = linear_shortk(y, w1, b1, relu=True)                         (NEXT)

over one tile, ragged tiles, and one M at which a persistent workgroup walks more than two tiles with a ragged end: launch_chain starts
gx = min(512, ceil(M / 64)) workgroups, workgroup b takes tiles b, b + gx, ..., so M = 64 * (2 * 512) + 37 = 65573 rows (33.6 MB of y).
Identities and x0 are distinct in every row (checked): a tile or row mix-up cannot pass.
"""
import pytest
import torch

import alo_hip
from guarded import GuardedLaunches

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
GRID = 512                                # launch_chain: at most this many persistent workgroups
LONG_M = 64 * (2 * GRID) + 37
KINDS = ("down", "res")
WIDTHS = (0, 64, 128)                     # channels of the next convolution; 0: none


def rows_as_map(t):
    """(M, C) rows -> the channels-last (1, C, 1, M) map that holds them."""
    return t.view(1, 1, t.shape[0], t.shape[1]).permute(0, 3, 1, 2)


def map_as_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def distinct_rows(t, g):
    key = t.double() @ torch.randn(t.shape[1], device=DEV, generator=g, dtype=torch.float64)
    return torch.unique(key).numel() == t.shape[0]


def make_case(m, n2, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rand(*shape, scale=1.0):
        return (scale * torch.randn(*shape, device=DEV, generator=g)).to(BF16)

    c = dict(mid=rand(m, 64), x0=rand(m, 64), identity=rand(m, 256), w3=rand(256, 64, scale=0.125), b3=rand(256, scale=0.5),
             wd=rand(256, 64, scale=0.125), bd=rand(256, scale=0.5))
    if n2:
        c.update(w1=rand(n2, 256, scale=0.0625), b1=rand(n2, scale=0.5))
    assert distinct_rows(c["identity"], g) and distinct_rows(c["x0"], g)
    return c


def separate_launches(c, kind, n2):
    identity = alo_hip.linear_shortk(c["x0"], c["wd"], c["bd"]) if kind == "down" else c["identity"]
    y = alo_hip.linear_shortk(c["mid"], c["w3"], c["b3"], relu=True, residual=identity)
    return y, (alo_hip.linear_shortk(y, c["w1"], c["b1"], relu=True) if n2 else None)


def chain(c, kind, n2):
    y, z = alo_hip.conv1x1_chain(rows_as_map(c["mid"]), (c["w3"], c["b3"]),
                                 identity=rows_as_map(c["identity"]) if kind == "res" else None,
                                 down=(rows_as_map(c["x0"]), c["wd"], c["bd"]) if kind == "down" else None,
                                 nxt=(c["w1"], c["b1"]) if n2 else None)
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
    assert tiles > 2 * min(GRID, tiles) and LONG_M % 64 != 0


@pytest.mark.parametrize("m", [1, 63, 64, 65, 200, LONG_M])
@pytest.mark.parametrize("n2", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_equals_the_launches_it_replaces(kind, n2, m):
    check_exact(make_case(m, n2, 3 * m + n2 + (kind == "down")), kind, n2, f"{kind} next={n2} M={m}")


@pytest.mark.parametrize("n2", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_nan_and_inf_travel_as_in_the_separate_launches(kind, n2):
    """NaN, +Inf and -Inf in the inputs, in all three tiles of one workgroup's walk: compared on the bit patterns (ReLU keeps NaN)."""
    m = LONG_M
    c = make_case(m, n2, 77 + n2)
    rows = [21, 64 * GRID + 21, 64 * (2 * GRID) + 3, m - 1]   # workgroup 0's three tiles, 0, 512 and 1024 (the ragged one, 37 rows)
    for i, value in zip(rows, (float("nan"), float("inf"), float("-inf"), float("nan"))):
        c["mid"][i, 7] = value
        c["x0" if kind == "down" else "identity"][i + 1 if i + 1 < m else i - 1, 70 % (64 if kind == "down" else 256)] = value
    got_y, _ = check_exact(c, kind, n2, f"{kind} next={n2} non-finite")
    assert torch.isnan(got_y[21]).all() and torch.isnan(got_y[m - 1]).all() and not torch.isnan(got_y[20]).any()


@pytest.mark.parametrize("kind,n2", [("down", 64), ("res", 64), ("res", 128), ("down", 0)])
def test_chain_stays_in_its_buffers_and_ignores_stale_bytes(kind, n2):
    """Guarded buffers with poisoned slack either side, twice with different fills (tests/guarded.py); M = 200: three full tiles and a
    ragged fourth, whose missing rows are read from the last row and never stored."""
    c = make_case(200, n2, 5 + n2)
    with torch.no_grad():
        want_y, want_z = separate_launches(c, kind, n2)
        with GuardedLaunches() as g:
            got_y, got_z = chain(c, kind, n2)
    assert [symbol for symbol, _ in g.seen] == ["alo_conv1x1_nhwc"] and g.seen[0][1].startswith("conv1x1_chain/")
    assert same_bits(got_y, want_y) and (want_z is None or same_bits(got_z, want_z))


def test_the_gate_and_the_wrapper_refuse_what_the_kernel_does_not_serve(monkeypatch):
    c = make_case(65, 64, 1)
    mid, idn, x0 = rows_as_map(c["mid"]), rows_as_map(c["identity"]), rows_as_map(c["x0"])
    conv3, nxt = (c["w3"], c["b3"]), (c["w1"], c["b1"])
    ok = alo_hip.conv1x1_chain_supported
    with torch.no_grad():
        assert ok(mid, conv3, identity=idn, nxt=nxt) and ok(mid, conv3, down=(x0, c["wd"], c["bd"]))
        assert not ok(mid, conv3) and not ok(mid, conv3, identity=idn, down=(x0, c["wd"], c["bd"]))
        assert not ok(mid.float(), conv3, identity=idn.float(), nxt=nxt)
        assert not ok(mid, conv3, identity=idn, nxt=(torch.zeros(256, 256, device=DEV, dtype=BF16), torch.zeros(256, device=DEV, dtype=BF16)))
        assert not ok(mid, (c["w3"], None), identity=idn)
        assert not ok(mid, conv3, identity=idn[:, :, :, :64])
        monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", "off")
        assert not ok(mid, conv3, identity=idn, nxt=nxt)
        with pytest.raises(RuntimeError, match="conv1x1_chain"):
            alo_hip.conv1x1_chain(mid, conv3, identity=idn, nxt=nxt)
        monkeypatch.delenv("ALO_BOTTLENECK_CHAIN")
        # y-then-z is one buffer: the library refuses an output that overlaps an input
        buf = torch.cat([c["w3"].reshape(-1), c["b3"]])
        with pytest.raises(RuntimeError, match="overlaps"):
            alo_hip._launch("alo_conv1x1_nhwc", mid.device, None, 0.0, 0.0, mid, buf, alo_hip.CONV1X1_CHAIN, None, idn, idn, 1, 1, 65, 64, 256,
                            1, 1, alo_hip.ALO_BF16)
    assert not ok(mid, conv3, identity=idn, nxt=nxt)   # grad mode on: the separate launches


# ---- the backbone -------------------------------------------------------------------------------------------------------------------
STAGES = {"layer1": "0", "layer2": "1", "layer3": "2", "layer4": "3"}
CHAIN_TAGS = ["conv1x1_chain/down+next64", "conv1x1_chain/res+next64"]


@pytest.fixture(scope="module")
def body_and_input():
    import alonet.detr.backbone as bb

    torch.manual_seed(0)
    body = bb.ResNetBody("resnet50", return_layers=STAGES).to(DEV).eval()
    for m in body.modules():  # non-trivial frozen statistics
        if hasattr(m, "running_var"):
            m.running_var.uniform_(0.5, 2.0); m.running_mean.normal_(0, 0.2); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    return body.to(BF16), torch.randn(2, 3, 72, 104, device=DEV).to(BF16)


@pytest.fixture(scope="module")
def separate_stages(body_and_input):
    """Every stage with ``ALO_BOTTLENECK_CHAIN=off``, and the launch tags of that forward: computed once, left unchanged."""
    import os

    body, x = body_and_input
    old = os.environ.get("ALO_BOTTLENECK_CHAIN")
    os.environ["ALO_BOTTLENECK_CHAIN"] = "off"
    try:
        with alo_hip.LaunchTimer() as t, torch.no_grad():
            out = {k: v.clone() for k, v in body(x).items()}
        return out, sorted(t.summary())
    finally:
        if old is None:
            del os.environ["ALO_BOTTLENECK_CHAIN"]
        else:
            os.environ["ALO_BOTTLENECK_CHAIN"] = old


def assert_same_stages(got, want):
    assert got.keys() == want.keys() and len(want) == 4
    for k in want:
        assert got[k].shape == want[k].shape and bool(torch.isfinite(want[k].float()).all())
        assert torch.equal(got[k], want[k]), k


def test_resnet_body_knob_on_equals_knob_off(body_and_input, separate_stages, monkeypatch):
    body, x = body_and_input
    want, off_tags = separate_stages
    monkeypatch.delenv("ALO_BOTTLENECK_CHAIN", raising=False)
    with alo_hip.LaunchTimer() as t, torch.no_grad():
        got = body(x)
    calls = {tag: d["calls"] for tag, d in t.summary().items()}
    # layer1.0 folds its downsample and layer1.1's conv1, layer1.1 folds layer1.2's conv1: five launches become two.  layer1.2, the last
    # block of its stage, hands nothing on: its conv3 stays the plain launch with the identity in its epilogue
    assert [calls.get(tag) for tag in CHAIN_TAGS] == [1, 1], calls
    assert [tag for tag in calls if tag.startswith("conv1x1_chain")] == CHAIN_TAGS
    assert not any(tag.startswith("conv1x1_chain") for tag in off_tags)
    assert "linear_shortk/N=64,K=256" not in calls and calls["linear_shortk/N=256,K=64"] == 1 and calls["linear_shortk/N=128,K=256"] == 1
    assert {"linear_shortk/N=256,K=64", "linear_shortk/N=64,K=256", "linear_shortk/N=128,K=256"} <= set(off_tags)
    assert_same_stages(got, want)


def test_a_swapped_conv_bn_is_handed_every_convolution(body_and_input, separate_stages, monkeypatch):
    """``backbone.conv_bn`` is the one name every convolution of the body goes through: with another function in its place the chain
    steps aside, that function sees all 52 convolutions of the bottlenecks (16 of them with an identity), and the stages are those of the knob off."""
    import alonet.detr.backbone as bb

    body, x = body_and_input
    want, _ = separate_stages
    monkeypatch.delenv("ALO_BOTTLENECK_CHAIN", raising=False)
    conv_bn, seen = bb.conv_bn, []

    def counting_conv_bn(x, conv, bn, relu=False, residual=None):
        seen.append(residual is not None)
        return conv_bn(x, conv, bn, relu=relu, residual=residual)

    monkeypatch.setattr(bb, "conv_bn", counting_conv_bn)
    with alo_hip.LaunchTimer() as t, torch.no_grad():
        got = body(x)
    assert not any(tag.startswith("conv1x1_chain") for tag in t.summary())
    assert sum(seen) == 16 and len(seen) in (52, 53)   # 3 * 16 + 4 downsamples, and the stem where it is not fused with its max-pool
    assert_same_stages(got, want)


def test_resnet_body_under_graph_capture_and_two_replays(body_and_input, separate_stages, monkeypatch):
    body, x = body_and_input
    want, _ = separate_stages
    monkeypatch.delenv("ALO_BOTTLENECK_CHAIN", raising=False)
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


def test_a_bottleneck_alone_gives_the_same_result(body_and_input, monkeypatch):
    """``Bottleneck.forward(x)`` without the hand-off: layer1.0 still folds its downsample convolution, layer1.1 has nothing to fold."""
    body, _ = body_and_input
    x = torch.randn(2, 64, 18, 26, device=DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        monkeypatch.setenv("ALO_BOTTLENECK_CHAIN", "off")
        want0 = body.layer1[0](x)
        want1 = body.layer1[1](want0)
        monkeypatch.delenv("ALO_BOTTLENECK_CHAIN")
        with alo_hip.LaunchTimer() as t:
            got0 = body.layer1[0](x)
            got1 = body.layer1[1](got0)
            y, head = body.layer1[0](x, nxt=body.layer1[1])
            got1_handed = body.layer1[1](y, head=head)
    assert {tag: d["calls"] for tag, d in t.summary().items() if tag.startswith("conv1x1_chain")} == {
        "conv1x1_chain/down": 1, "conv1x1_chain/down+next64": 1}
    assert torch.equal(got0, want0) and torch.equal(y, want0) and torch.equal(got1, want1) and torch.equal(got1_handed, want1)


def test_with_grad_enabled_the_separate_launches_run_and_gradients_reach_the_weights(body_and_input):
    body, x = body_and_input
    block = body.layer1[0]
    xin = torch.randn(2, 64, 18, 26, device=DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    params = [block.conv3.weight, block.downsample[0].weight, body.layer1[1].conv1.weight]
    try:
        for p in params:
            p.requires_grad_(True)
        with alo_hip.LaunchTimer() as t:
            y, head = block(xin, nxt=body.layer1[1])
            assert head is None and y.requires_grad
            out = body.layer1[1](y)
        assert not any(tag.startswith("conv1x1_chain") for tag in t.summary())
        out.float().square().mean().backward()
        for p in params:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
        # frozen weights under grad mode (a detector in training freezes layer1): still the separate launches
        for p in params:
            p.requires_grad_(False)
        with alo_hip.LaunchTimer() as t:
            block(xin, nxt=body.layer1[1])
        assert "linear_shortk/N=256,K=64" in t.summary() and not any(tag.startswith("conv1x1_chain") for tag in t.summary())
    finally:
        for p in params:
            p.requires_grad_(False)
            p.grad = None
