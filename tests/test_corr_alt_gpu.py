"""AlternateCorrBlock on the gfx950 kernels (csrc/corr_alt.hip): CorrBlock's goldens, the fp32 oracle, edge cases, sizes CorrBlock
cannot take, RAFT end to end and under graph capture."""
import math

import numpy as np
import pytest
import torch

import alo_hip
import aloscene
import oracle as O
from alonet.raft import RAFT
from alonet.raft import AlternateCorrBlock as ExportedAlternateCorrBlock
from alonet.raft.corr import AlternateCorrBlock, CorrBlock, TorchAlternateCorrBlock
from alonet.raft.utils.utils import coords_grid
from helpers import formula_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def alt(f1, f2, L, r, coords):
    return AlternateCorrBlock(dev(f1), dev(f2), num_levels=L, radius=r)(dev(coords)).cpu().numpy()


def feature_scale(f1, f2):
    """max |f1_i| |f2_j| / sqrt(C): the size of the largest possible output; errors are bounded relative to it."""
    C = f1.shape[1]
    n1 = np.sqrt((f1.astype(np.float64) ** 2).sum(1)).max()
    n2 = np.sqrt((f2.astype(np.float64) ** 2).sum(1)).max()
    return n1 * n2 / math.sqrt(C)


def test_exported_from_the_package():
    assert ExportedAlternateCorrBlock is AlternateCorrBlock


def test_g6_through_the_hip_block(golden):
    g = golden("g6_corr.npz")
    blk = AlternateCorrBlock(dev(g["f1"]), dev(g["f2"]), radius=4)
    assert blk.num_levels == 4 and blk.radius == 4 and len(blk.pyramid) == 5
    for k in "abc":
        out = blk(dev(g["coords_" + k]))
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == g["out_" + k].shape
        np.testing.assert_allclose(out.cpu().numpy(), g["out_" + k], rtol=0, atol=3e-5)
    blk = AlternateCorrBlock(dev(g["f1o"]), dev(g["f2o"]), radius=3)
    np.testing.assert_allclose(blk(dev(g["coords_o"])).cpu().numpy(), g["out_o"], rtol=0, atol=1e-5)


def test_g7_raft_end_to_end_with_the_alternate_block(golden):
    g = golden("g7_raft.npz")
    model = RAFT(corr_block=AlternateCorrBlock).eval()
    model.load_state_dict(formula_state_dict(model.state_dict()))
    model = model.to(DEV)
    f1 = aloscene.Frame(t(g["img1"]).float(), normalization="minmax_sym", names=("B", "C", "H", "W")).to(DEV)
    f2 = aloscene.Frame(t(g["img2"]).float(), normalization="minmax_sym", names=("B", "C", "H", "W")).to(DEV)
    with torch.no_grad():
        outs = model(f1, f2, iters=4)
    flows = np.stack([o["flow"].cpu().numpy() for o in outs])
    assert np.isfinite(flows).all()
    assert np.abs(flows - g["flow"]).max() <= 1e-3
    assert np.abs(outs[-1]["up_flow"].cpu().numpy() - g["up_flow_last"]).max() <= 8e-3
    assert np.abs(outs[-1]["hidden_state"].cpu().numpy() - g["hidden_last"]).max() <= 1e-3


def coordinate_sets(rng, B, H, W):
    grid = coords_grid(B, H, W).numpy()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    smooth = np.stack([3.0 * np.sin(ys / 5.0 + 0.3) + 1.7 * np.cos(xs / 7.0), 2.5 * np.cos(xs / 6.0) - 1.3 * np.sin(ys / 4.0)])
    rand = np.stack([rng.uniform(0, W, (B, H, W)), rng.uniform(0, H, (B, H, W))], 1)
    return {
        "identity": grid,
        "smooth": grid + smooth[None],
        "random": rand,
        "partly_outside": grid + np.array([W * 0.6, -H * 0.55]).reshape(1, 2, 1, 1),
        "in_minus_one_zero": rng.uniform(-1, 0, (B, 2, H, W)),
    }


@pytest.mark.parametrize("B,C,H,W,r,L", [(1, 8, 13, 17, 0, 1), (3, 24, 19, 23, 1, 3), (1, 96, 21, 30, 2, 2), (3, 256, 16, 24, 3, 4),
                                         (1, 257, 11, 13, 4, 2), (1, 8, 37, 35, 5, 5), (1, 24, 20, 27, 6, 3), (3, 96, 17, 9, 7, 2),
                                         (1, 256, 33, 40, 4, 4)])
def test_against_the_fp32_oracle(B, C, H, W, r, L):
    rng = np.random.default_rng(B * 7919 + C * 31 + H + r)
    f1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    pyr = O.corr_pyramid(f1, f2, L)
    tol = 1e-5 * feature_scale(f1, f2)
    blk = AlternateCorrBlock(dev(f1), dev(f2), num_levels=L, radius=r)
    for name, coords in coordinate_sets(rng, B, H, W).items():
        coords = coords.astype(np.float32)
        got = blk(dev(coords)).cpu().numpy()
        want = O.corr_lookup(pyr, coords, r)
        assert got.shape == want.shape == (B, L * (2 * r + 1) ** 2, H, W)
        err = np.abs(got - want).max()
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("kind", ["random", "discontinuous"])
def test_oversized_footprints_match_the_oracle(kind):
    """Tiles whose windows spread over more of fmap2 than the LDS budget holds read their lattice from global memory."""
    B, C, H, W, r, L = 2, 40, 40, 96, 4, 3
    rng = np.random.default_rng(5)
    f1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    grid = coords_grid(B, H, W).numpy()
    if kind == "random":
        coords = np.stack([rng.uniform(-4, W + 4, (B, H, W)), rng.uniform(-4, H + 4, (B, H, W))], 1)
    else:   # the right half of every 8-wide tile moves 60 px further than the left half
        coords = grid + rng.standard_normal(grid.shape) * 0.5
        coords[:, 0] += np.where(np.arange(W) % 8 >= 4, 60.0, 0.0)[None, None, :] - 30.0
    coords = coords.astype(np.float32)
    got = alt(f1, f2, L, r, coords)
    want = O.corr_lookup(O.corr_pyramid(f1, f2, L), coords, r)
    assert np.abs(got - want).max() <= 1e-5 * feature_scale(f1, f2)


def test_non_finite_and_huge_coordinates_read_as_zero():
    B, C, H, W, r, L = 1, 32, 24, 24, 4, 3
    rng = np.random.default_rng(11)
    f1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    coords = (coords_grid(B, H, W).numpy() + rng.standard_normal((B, 2, H, W))).astype(np.float32)
    bad = [(0, 0, 3, 3, np.nan), (0, 1, 3, 4, np.nan), (0, 0, 9, 10, np.inf), (0, 1, 9, 11, -np.inf), (0, 0, 17, 2, 1e30),
           (0, 1, 17, 3, -1e30), (0, 0, 5, 20, 2.5e6)]
    broken = coords.copy()
    for b, c, y, x, v in bad:
        broken[b, c, y, x] = v
    got = alt(f1, f2, L, r, broken)
    want = O.corr_lookup(O.corr_pyramid(f1, f2, L), coords, r)   # the same queries, all finite
    hit = np.zeros((H, W), bool)
    for _, _, y, x, _ in bad:
        hit[y, x] = True
        assert (got[0, :, y, x] == 0).all()
    assert np.isfinite(got).all()
    assert np.abs(got[0][:, ~hit] - want[0][:, ~hit]).max() <= 1e-5 * feature_scale(f1, f2)


def test_one_pixel_wide_levels_match_the_torch_block():
    B, C, H, W, r, L = 2, 16, 20, 9, 3, 4   # level 3 is 2 x 1
    rng = np.random.default_rng(3)
    f1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    coords = (coords_grid(B, H, W).numpy() + rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    got = alt(f1, f2, L, r, coords)
    want = TorchAlternateCorrBlock(t(f1).double(), t(f2).double(), num_levels=L, radius=r)(t(coords).double()).numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-5 * feature_scale(f1, f2)


def test_non_finite_features_spoil_exactly_their_taps():
    B, C, H, W, r, L = 1, 24, 20, 22, 3, 3
    rng = np.random.default_rng(13)
    f1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f1[0, 5, 6, 7] = np.inf
    f2[0, 7, 10, 4] = np.nan
    # off integer positions on every level: no bilinear weight is 0 (0 * NaN is NaN in both computations anyway)
    coords = (coords_grid(B, H, W).numpy() + 0.3 + 0.1 * rng.random((B, 2, H, W))).astype(np.float32)
    got = alt(f1, f2, L, r, coords)
    want = O.corr_lookup(O.corr_pyramid(f1, f2, L), coords, r)
    bad = ~np.isfinite(want)
    assert bad.any() and (~bad).any()
    np.testing.assert_array_equal(~np.isfinite(got), bad)
    assert np.abs(got[~bad] - want[~bad]).max() <= 1e-5 * feature_scale(np.nan_to_num(f1, posinf=0), np.nan_to_num(f2))


def test_configs2_size_agrees_with_corr_block():
    """4 x 1280x720 frames at 1/8 resolution: one lookup against CorrBlock on smooth flow; a pair does not see its neighbours."""
    B, C, H, W = 4, 256, 90, 160
    gen = torch.Generator(device=DEV).manual_seed(0)
    f1 = torch.randn(B, C, H, W, device=DEV, generator=gen)
    f2 = torch.randn(B, C, H, W, device=DEV, generator=gen)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    flow = torch.stack([3 * torch.sin(ys / 9.0) + 2 * torch.cos(xs / 13.0), 2 * torch.cos(xs / 11.0) - 1.5 * torch.sin(ys / 7.0)])
    coords = coords_grid(B, H, W).to(DEV) + flow[None] + 0.25 * torch.arange(B, device=DEV).view(B, 1, 1, 1)
    got = AlternateCorrBlock(f1, f2)(coords)
    want = CorrBlock(f1, f2)(coords)
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    alone = AlternateCorrBlock(f1[2:3], f2[2:3])(coords[2:3])
    torch.testing.assert_close(alone, got[2:3], rtol=0, atol=0)


def direct_fp64(f1, f2_levels, coords, r, idx):
    """fp64 on the CPU at query pixels ``idx`` of item 0: window sums of the lattice's inner products, bilinear, zeros outside."""
    C = f1.shape[1]
    H, W = coords.shape[-2:]
    qy, qx = idx // W, idx % W
    q1 = f1[0, :, qy, qx].double().cpu().T                       # (Q, C)
    out = []
    for lvl, f2 in enumerate(f2_levels):
        h, w = f2.shape[-2:]
        cx = coords[0, 0, qy, qx].double().cpu() / 2 ** lvl
        cy = coords[0, 1, qy, qx].double().cpu() / 2 ** lvl
        x0, y0 = torch.floor(cx).long() - r, torch.floor(cy).long() - r
        fx, fy = cx - torch.floor(cx), cy - torch.floor(cy)
        S = 2 * r + 2
        k = torch.arange(S)
        px, py = torch.broadcast_tensors(x0[:, None, None] + k[None, None, :], y0[:, None, None] + k[None, :, None])   # (Q, S rows, S cols)
        inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        flat = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).to(DEV)
        vecs = f2[0].reshape(C, h * w)[:, flat.reshape(-1)].double().cpu().T.reshape(*flat.shape, C)   # (Q, S, S, C)
        lat = torch.where(inside, (vecs * q1[:, None, None, :]).sum(-1), torch.zeros((), dtype=torch.float64)) / math.sqrt(C)
        fx, fy = fx[:, None, None], fy[:, None, None]
        top = (1 - fx) * lat[:, :-1, :-1] + fx * lat[:, :-1, 1:]     # [q, y offset, x offset]
        bot = (1 - fx) * lat[:, 1:, :-1] + fx * lat[:, 1:, 1:]
        win = (1 - fy) * top + fy * bot
        out.append(win.transpose(1, 2).reshape(len(idx), -1))      # first window axis: x offset
    return torch.cat(out, 1)                                       # (Q, L * (2r+1)^2)


def test_a_grid_corr_block_cannot_take():
    """7680x4320 frames at 1/8 resolution: the all-pairs volume would be 1.1 TB; the alternate block keeps 1.1 GB of features."""
    B, C, H, W, r = 1, 256, 540, 960, 4
    gen = torch.Generator(device=DEV).manual_seed(1)
    f1 = torch.randn(B, C, H, W, device=DEV, generator=gen)
    f2 = torch.randn(B, C, H, W, device=DEV, generator=gen)
    with pytest.raises(RuntimeError):
        alo_hip.corr_build(f1, f2, 4)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    flow = torch.stack([6 * torch.sin(ys / 40.0) + 3 * torch.cos(xs / 30.0), 4 * torch.cos(xs / 50.0) - 2 * torch.sin(ys / 25.0)])
    coords = coords_grid(B, H, W).to(DEV) + flow[None]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    blk = AlternateCorrBlock(f1, f2)
    out = blk(coords)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert grew < 3 * 2 ** 30, grew
    assert out.shape == (B, 4 * 81, H, W)
    idx = torch.from_numpy(np.random.default_rng(2).choice(H * W, 512, replace=False))
    want = direct_fp64(f1, [p[1] for p in blk.pyramid[:4]], coords, r, idx)
    got = out[0].reshape(4 * 81, H * W)[:, idx.to(DEV)].T.double().cpu()
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item() + 1e-6


def test_graphed_forward_replays_raft_with_the_alternate_block(golden):
    from alonet.common import GraphedForward

    g = golden("g7_raft.npz")
    model = RAFT(corr_block=AlternateCorrBlock).eval()
    model.load_state_dict(formula_state_dict(model.state_dict()))
    model = model.to(DEV)
    mk = lambda a: aloscene.Frame(t(a).float(), normalization="minmax_sym", names=("B", "C", "H", "W")).to(DEV)  # noqa: E731
    f1, f2 = mk(g["img1"]), mk(g["img2"])
    graphed = GraphedForward(model)
    flows = []
    with torch.no_grad():
        for a, b in ((f1, f2), (f2, f1)):
            want = model(a, b, iters=3, only_last=True)
            got = graphed(a, b, iters=3, only_last=True)
            assert (got[-1]["up_flow"] - want[-1]["up_flow"]).abs().max().item() <= 1e-3
            flows.append(got[-1]["up_flow"].clone())
    assert (flows[0] - flows[1]).abs().max().item() > 0.1
    assert len(graphed._graphs) == 1


def test_no_autograd():
    f1 = torch.randn(1, 16, 12, 14, device=DEV, requires_grad=True)
    f2 = torch.randn(1, 16, 12, 14, device=DEV, requires_grad=True)
    out = AlternateCorrBlock(f1, f2, num_levels=2, radius=2)(coords_grid(1, 12, 14).to(DEV))
    assert not out.requires_grad and out.grad_fn is None
