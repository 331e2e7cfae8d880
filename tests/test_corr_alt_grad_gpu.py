"""TrainableAlternateCorrBlock on the GPU: the lookup's adjoint kernel (csrc/corr_alt.hip, ALO_CORR_ALT_GRAD) and the block's autograd
wiring.

Yardstick: fp64 autograd through ``lookup_alt_torch(_alt_pyramid(f1.double(), f2.double(), L), coords.double(), L, r)``.
Bar (the project's G18 test): ``max|got - want| <= 1e-4 * max(1, max|want|)`` per gradient."""
import numpy as np
import pytest
import torch

import alo_hip
from alonet.raft import RAFT, TrainableAlternateCorrBlock
from alonet.raft.corr import AlternateCorrBlock, CorrBlock, TorchCorrBlock, _alt_pyramid, lookup_alt_torch
from alonet.raft.utils.utils import coords_grid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def yardstick(f1, f2, L, r, coords, weights):
    """-> (outs, grad_f1, grad_f2) in fp64."""
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    pyr = _alt_pyramid(a, b, L)
    outs = [lookup_alt_torch(pyr, c.double(), L, r) for c in coords]
    g1, g2 = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, weights)), (a, b))
    return [o.detach() for o in outs], g1, g2


def through_block(f1, f2, L, r, coords, weights, need=(True, True), cls=TrainableAlternateCorrBlock):
    a, b = f1.clone().requires_grad_(need[0]), f2.clone().requires_grad_(need[1])
    blk = cls(a, b, num_levels=L, radius=r)
    outs = [blk(c) for c in coords]
    grads = list(torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, weights)), [t for t in (a, b) if t.requires_grad]))
    return [o.detach() for o in outs], (grads.pop(0) if need[0] else None), (grads.pop(0) if need[1] else None)


def check(got, want, what):
    err = (got.double() - want).abs().max().item()
    bar = 1e-4 * max(1.0, want.abs().max().item())
    print(f"{what}: max|got-want| = {err:.3e}, bar {bar:.3e}, max|want| = {want.abs().max().item():.3g}")
    assert err <= bar, (what, err, bar)


def coordinate_sets(gen, B, H, W):
    grid = coords_grid(B, H, W)
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    smooth = torch.stack([3.0 * torch.sin(ys / 5.0 + 0.3) + 1.7 * torch.cos(xs / 7.0), 2.5 * torch.cos(xs / 6.0) - 1.3 * torch.sin(ys / 4.0)])
    rand = torch.stack([torch.rand(B, H, W, generator=gen) * W, torch.rand(B, H, W, generator=gen) * H], 1)
    outside = grid + torch.tensor([W * 0.6, -H * 0.55]).view(1, 2, 1, 1)
    return [(grid + smooth[None]).to(DEV), rand.to(DEV), outside.to(DEV)]


def test_g18_through_the_trainable_block(golden):
    """G18 (the reference's CorrBlock under fp64 autograd: B 2, C 24, 13x18, 3 levels, r 2, three lookups, windows off the map, a row
    on integer coordinates): outputs at CorrBlock's bar, both gradients at the G18 bar; and the yardstick of this file against it."""
    g = golden("g18_corr_grad.npz")
    f1, f2 = dev(g["f1"]), dev(g["f2"])
    coords, wts = list(dev(g["coords"])), list(dev(g["weights"]))
    outs, g1, g2 = through_block(f1, f2, 3, 2, coords, wts)
    for o, want in zip(outs, dev(g["out"])):
        assert (o - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())
    check(g1, dev(g["grad_f1"]).double(), "g18 grad_f1")
    check(g2, dev(g["grad_f2"]).double(), "g18 grad_f2")
    _, y1, y2 = yardstick(f1, f2, 3, 2, coords, wts)
    check(y1, dev(g["grad_f1"]).double(), "yardstick vs g18 grad_f1")
    check(y2, dev(g["grad_f2"]).double(), "yardstick vs g18 grad_f2")


@pytest.mark.parametrize("B,C,H,W,r,L", [(1, 8, 13, 17, 0, 1), (3, 24, 19, 23, 1, 3), (1, 96, 21, 30, 2, 2), (3, 256, 16, 24, 3, 4),
                                         (1, 257, 11, 13, 4, 2), (1, 8, 37, 35, 5, 5), (3, 96, 17, 9, 7, 2)])
def test_gradients_against_fp64_autograd(B, C, H, W, r, L):
    """Partial tiles, channel padding, several channel slices, every radius, one-pixel levels; smooth, random-over-the-map and
    partly-outside coordinates, random grad_out."""
    gen = torch.Generator().manual_seed(B * 7919 + C * 31 + H + r)
    f1 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    coords = coordinate_sets(gen, B, H, W)
    wts = [torch.randn(B, L * (2 * r + 1) ** 2, H, W, generator=gen).to(DEV) for _ in coords]
    outs, g1, g2 = through_block(f1, f2, L, r, coords, wts)
    _, w1, w2 = yardstick(f1, f2, L, r, coords, wts)
    for o, c in zip(outs, coords):
        assert torch.equal(o, AlternateCorrBlock(f1, f2, num_levels=L, radius=r)(c))
    check(g1, w1, "grad_fmap1")
    check(g2, w2, "grad_fmap2")


@pytest.mark.parametrize("kind", ["random", "discontinuous"])
def test_oversized_footprints(kind):
    """Tiles over the footprint budget take the direct path (global reads, one atomic per query, point and channel)."""
    B, C, H, W, r, L = 2, 40, 40, 96, 4, 3
    gen = torch.Generator().manual_seed(5)
    f1 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    if kind == "random":
        coords = torch.stack([torch.rand(B, H, W, generator=gen) * (W + 8) - 4, torch.rand(B, H, W, generator=gen) * (H + 8) - 4], 1)
    else:   # the right half of every 8-wide tile moves 60 px further than the left half
        coords = coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen) * 0.5
        coords[:, 0] += torch.where(torch.arange(W) % 8 >= 4, 60.0, 0.0)[None, None, :] - 30.0
    coords = [coords.to(DEV)]
    wts = [torch.randn(B, L * 81, H, W, generator=gen).to(DEV)]
    _, g1, g2 = through_block(f1, f2, L, r, coords, wts)
    _, w1, w2 = yardstick(f1, f2, L, r, coords, wts)
    check(g1, w1, "grad_fmap1")
    check(g2, w2, "grad_fmap2")


def test_non_finite_and_huge_coordinates_contribute_nothing():
    B, C, H, W, r, L = 1, 32, 24, 24, 4, 3
    gen = torch.Generator().manual_seed(11)
    f1 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    coords = coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen)
    bad = [(0, 3, 3, float("nan")), (1, 3, 4, float("nan")), (0, 9, 10, float("inf")), (1, 9, 11, float("-inf")), (0, 17, 2, 1e7),
           (1, 17, 3, -1e7), (0, 5, 20, 1e30)]
    hit = torch.zeros(H, W, dtype=torch.bool)
    for c, y, x, v in bad:
        coords[0, c, y, x] = v
        hit[y, x] = True
    coords = [coords.to(DEV)]
    gout = torch.randn(B, L * 81, H, W, generator=gen).to(DEV)
    zeroed = gout.clone()
    zeroed[:, :, hit.to(DEV)] = 0
    _, g1, g2 = through_block(f1, f2, L, r, coords, [gout])
    _, z1, z2 = through_block(f1, f2, L, r, coords, [zeroed])
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    assert torch.equal(g1[0][:, hit.to(DEV)], z1[0][:, hit.to(DEV)]) and not g1[0][:, hit.to(DEV)].any()
    assert torch.equal(g1, z1)                                  # grad_fmap1 has no atomics: the whole map is bit-equal
    check(g2, z2.double(), "grad_fmap2 vs zeroed grad_out")     # up to the order of the atomic sums
    _, w1, w2 = yardstick(f1, f2, L, r, coords, [gout])
    check(g1, w1, "grad_fmap1")
    check(g2, w2, "grad_fmap2")


def test_many_lookups_repeated_and_partial_backward():
    """RAFT's pattern: one block, 8 lookups, one backward; a second backward over the retained graph starts from zeroed maps; only one
    feature map training; a pass that runs the lookups' backward without reaching the build node leaves nothing behind."""
    gen = torch.Generator().manual_seed(5)
    B, C, H, W, L, r = 2, 40, 15, 22, 3, 3
    f1 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    coords = [(coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen) * (1.0 + 0.5 * k)).to(DEV) for k in range(8)]
    wts = [torch.randn(B, L * 49, H, W, generator=gen).to(DEV) for _ in coords]
    _, w1, w2 = yardstick(f1, f2, L, r, coords, wts)
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    blk = TrainableAlternateCorrBlock(a, b, num_levels=L, radius=r)
    loss = sum((blk(c) * w_).sum() for c, w_ in zip(coords, wts))
    torch.autograd.grad(loss, blk._token, retain_graph=True)     # the lookups' backward only: its maps belong to that pass
    loss.backward(retain_graph=True)
    first = (a.grad.clone(), b.grad.clone())
    a.grad = b.grad = None
    loss.backward()
    for k, (got, again, want) in enumerate(zip(first, (a.grad, b.grad), (w1, w2))):
        check(got, want, f"first pass, fmap{k + 1}")
        check(again, want, f"second pass, fmap{k + 1}")
        check(again, got.double(), f"second against first pass, fmap{k + 1}")
    assert torch.equal(first[0], a.grad)                         # grad_fmap1 is reproducible
    _, g1, none = through_block(f1, f2, L, r, coords, wts, need=(True, False))
    assert none is None
    check(g1, w1, "only fmap1 trains")
    _, none, g2 = through_block(f1, f2, L, r, coords, wts, need=(False, True))
    assert none is None
    check(g2, w2, "only fmap2 trains")


def test_flagged_call_stays_in_its_buffers_and_accumulates():
    B, C, H, W, L, r = 2, 24, 13, 18, 3, 2
    gen = torch.Generator().manual_seed(7)
    f1 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    coords = (coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen) * 2).to(DEV)
    gout = torch.randn(B, L * 25, H, W, generator=gen).to(DEV)
    levels = [p[1] for p in _alt_pyramid(f1, f2, L)[:L]]
    made = alo_hip.corr_alt_prepare(f1, levels, grad=True)
    lib = alo_hip.lib()
    total, prepared = lib.alo_corr_alt_workspace_bytes(B, C, H, W, L | 0x100), lib.alo_corr_alt_workspace_bytes(B, C, H, W, L)
    assert made.numel() == total
    assert torch.equal(made[:prepared], alo_hip.corr_alt_prepare(f1, levels))       # prepare fills a workspace of either size alike

    def run(fill):
        big = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        big[:total] = made
        ws = big[:total]
        region, planes, lvls = alo_hip.corr_alt_grad_views(ws, (B, C, H, W), L)
        region.view(torch.float32).fill_(fill)
        alo_hip.corr_alt_lookup_backward(ws, coords, gout, C, L, r)
        torch.cuda.synchronize()
        assert torch.equal(big[:prepared], made[:prepared])      # the prepared part is only read
        assert (big[total:] == 0xA5).all()                       # nothing behind the workspace is touched
        return region.view(torch.float32).clone(), planes, lvls

    zero, _, _ = run(0.0)
    half, planes, lvls = run(0.5)
    assert zero.abs().max().item() > 0.1
    tol = 1e-5 * max(1.0, zero.abs().max().item())
    assert (half - (zero + 0.5)).abs().max().item() <= tol       # added to, not overwritten
    for v in planes:                                             # padded channels 24..31: the constant, exactly
        assert (v[:, :, C:] == 0.5).all()
    for v in lvls:
        assert (v[1, :, :, C - 16:] == 0.5).all()
    with pytest.raises(RuntimeError, match="workspace"):         # a workspace without the region is refused before any launch
        alo_hip.corr_alt_lookup_backward(made[:prepared], coords, gout, C, L, r)


def test_without_gradients_it_is_the_alternate_block():
    gen = torch.Generator().manual_seed(3)
    f1 = torch.randn(1, 16, 12, 14, generator=gen).to(DEV)
    f2 = torch.randn(1, 16, 12, 14, generator=gen).to(DEV)
    coords = (coords_grid(1, 12, 14) + torch.randn(1, 2, 12, 14, generator=gen)).to(DEV)
    with alo_hip.LaunchTimer() as t:
        want = AlternateCorrBlock(f1, f2, num_levels=2, radius=2)(coords)
    tags = sorted(t.summary())
    assert tags == ["corr_alt_lookup", "corr_alt_prepare"]
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    for x, y, no_grad in ((f1, f2, False), (a, b, True)):        # frozen feature maps; torch.no_grad()
        with alo_hip.LaunchTimer() as t, torch.set_grad_enabled(not no_grad):
            blk = TrainableAlternateCorrBlock(x, y, num_levels=2, radius=2)
            got = blk(coords)
        assert sorted(t.summary()) == tags and {k: v["calls"] for k, v in t.summary().items()} == dict.fromkeys(tags, 1)
        assert torch.equal(got, want) and not got.requires_grad and got.grad_fn is None
        assert blk._workspace.numel() == alo_hip.lib().alo_corr_alt_workspace_bytes(1, 16, 12, 14, 2)   # no gradient region
    blk = TrainableAlternateCorrBlock(a, b, num_levels=2, radius=2)
    out = blk(coords)
    assert out.requires_grad and torch.equal(out.detach(), want)
    with torch.no_grad():                                        # a block built under grad mode, looked up without
        assert torch.equal(blk(coords), want) and not blk(coords).requires_grad
    for block in (blk, TrainableAlternateCorrBlock(f1, f2, num_levels=2, radius=2)):
        with pytest.raises(RuntimeError, match="no gradient with respect to the coordinates"):
            block(coords.clone().requires_grad_(True))
        with torch.no_grad():
            assert torch.equal(block(coords.clone().requires_grad_(True)), want)


def test_memory_stays_far_below_the_volume():
    """B 1, C 32, 64x64, L 4, r 4, two lookups + backward: the rise of the peak over the baseline before the block is built stays below
    V / 2, V = 4 HW sum_l h_l w_l = 89 MB being CorrBlock's pyramid alone.  Derived: two outputs and one grad_out of 5.3 MB, a
    flagged workspace of 3.9 MB, the NCHW gradients."""
    B, C, H, W, L, r = 1, 32, 64, 64, 4, 4
    gen = torch.Generator().manual_seed(1)
    f1 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    f2 = torch.randn(B, C, H, W, generator=gen).to(DEV)
    coords = [(coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen) * k).to(DEV) for k in (1.0, 2.0)]
    V = 4 * H * W * sum((H >> lvl) * (W >> lvl) for lvl in range(L))
    rise = {}
    for cls in (TrainableAlternateCorrBlock, CorrBlock):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        blk = cls(a, b, num_levels=L, radius=r)
        sum(blk(c).square().sum() for c in coords).backward()
        torch.cuda.synchronize()
        rise[cls.__name__] = torch.cuda.max_memory_allocated() - base
        assert a.grad is not None and b.grad is not None
        del blk, a, b
    print(f"peak rise in MB: { {k: round(v / 2 ** 20, 1) for k, v in rise.items()} }, V = {V / 2 ** 20:.1f} MB")
    assert rise["TrainableAlternateCorrBlock"] < V / 2, (rise, V)


def biases_in_front_of_an_instance_norm(net):
    """Names of the convolution biases of ``net`` whose output goes straight into an ``InstanceNorm2d`` without affine parameters:
    the norm subtracts the channel's mean, so such a bias has no gradient at all (``convN`` -> ``normN`` in the encoder and its
    blocks, ``downsample.0`` -> ``downsample.1``)."""
    plain = lambda m: isinstance(m, torch.nn.InstanceNorm2d) and not m.affine   # noqa: E731
    names = set()
    for prefix, m in net.named_modules():
        dot = prefix + "." if prefix else ""
        for k in "1234":
            if isinstance(getattr(m, "conv" + k, None), torch.nn.Conv2d) and plain(getattr(m, "norm" + k, None)):
                names.add(f"{dot}conv{k}.bias")
        down = getattr(m, "downsample", None)
        if isinstance(down, torch.nn.Sequential) and isinstance(down[0], torch.nn.Conv2d) and plain(down[1]):
            names.add(f"{dot}downsample.0.bias")
    return names


def test_raft_trains_through_the_block_like_through_corr_block():
    """One set of weights, three blocks.  For every fnet parameter d = max|g - g_CorrBlock| / max|g_CorrBlock|, and
    d(new) <= 10 d(TorchCorrBlock), the disagreement of two existing fp32 evaluations of the same function through the same recurrent
    graph on THAT parameter, and d(new) <= 1e-2.

    Left out of d: the convolution biases in front of an InstanceNorm (found from the modules, not from the figures).  Their gradient
    is exactly zero — the sum over a channel's pixels of the norm's input gradient — so max|g_CorrBlock| is rounding noise and d of any
    block, the existing ones included, is of order one (measured 0.9-2.1 for TorchCorrBlock).  They are held to what an fp32 sum that
    cancels can leave instead: with N <= 64 x 80 pixels per channel, about sqrt(N) eps = 4e-6 of the uncancelled sums the same
    convolution's weight gradient is made of; the bar is 1e-5 of max|g_CorrBlock(weight)| (measured 5e-7)."""
    import aloscene

    mk = lambda x: aloscene.Frame(x, normalization="minmax_sym", names=("B", "C", "H", "W")).to(DEV)  # noqa: E731
    torch.manual_seed(0)
    f1 = torch.rand(1, 3, 128, 160) * 2 - 1
    f2 = torch.roll(f1, shifts=(2, -3), dims=(2, 3))
    grads, state = {}, None
    for cls in (CorrBlock, TorchCorrBlock, TrainableAlternateCorrBlock):
        torch.manual_seed(0)
        model = RAFT(corr_block=cls)
        if state is None:
            state = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)
        model = model.to(DEV).train()
        model.freeze_bn()
        outs = model(mk(f1), mk(f2), iters=2)
        sum(o["up_flow"].abs().mean() for o in outs).backward()
        grads[cls] = {n: p.grad.clone() for n, p in model.fnet.named_parameters() if p.grad is not None}
        assert grads[cls] and all(torch.isfinite(g).all() for g in grads[cls].values())
    base = grads[CorrBlock]
    assert grads[TrainableAlternateCorrBlock].keys() == base.keys() == grads[TorchCorrBlock].keys()
    dead = biases_in_front_of_an_instance_norm(model.fnet)
    live = [n for n in base if n not in dead]
    assert dead <= base.keys() and "conv1.bias" in dead and "conv2.bias" in live and all(n.endswith(".weight") for n in live[:-1])
    diff = {cls: {n: (grads[cls][n] - g).abs().max().item() for n, g in base.items()} for cls in (TorchCorrBlock, TrainableAlternateCorrBlock)}
    size = {n: g.abs().max().item() for n, g in base.items()}
    for n in base:
        print(f"{n:32s} max|g| {size[n]:.3e}  |torch - corr| {diff[TorchCorrBlock][n]:.3e}  |new - corr| "
              f"{diff[TrainableAlternateCorrBlock][n]:.3e}{'  (in front of an InstanceNorm: no gradient)' if n in dead else ''}")
    d = {cls: {n: diff[cls][n] / size[n] for n in live} for cls in diff}
    print(f"d(TrainableAlternateCorrBlock) = {max(d[TrainableAlternateCorrBlock].values()):.3e}, "
          f"d(TorchCorrBlock) = {max(d[TorchCorrBlock].values()):.3e}, max|g_CorrBlock| = {max(size.values()):.3e}")
    for n in live:
        new, floor = d[TrainableAlternateCorrBlock][n], d[TorchCorrBlock][n]
        assert size[n] > 0 and new <= 10 * floor and new <= 1e-2, (n, new, floor)
    for n in dead:
        got = grads[TrainableAlternateCorrBlock][n].abs().max().item()
        assert got <= 1e-5 * size[n[:-len("bias")] + "weight"], (n, got)
