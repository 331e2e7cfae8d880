"""TrainableAlternateCorrBlock without a GPU: the ALO_CORR_ALT_GRAD flag of include/alo_corr_alt.h through ctypes (every call
carries one bad argument and never reaches a launch), the build node's host adjoint against autograd, the class's exports."""
import ctypes

import pytest
import torch

import alo_hip
from alonet.raft.corr import _alt_pyramid, alt_feature_gradients

FLAG = 0x100


def test_the_flag_is_the_headers():
    import os

    header = open(os.path.join(os.path.dirname(alo_hip.LIB_PATH), "..", "include", "alo_corr_alt.h")).read()
    assert "#define ALO_CORR_ALT_GRAD 0x100" in header
    assert alo_hip.ALO_CORR_ALT_GRAD == FLAG


def test_flagged_lookup_checks_before_any_launch():
    lib = alo_hip.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    big = ctypes.c_size_t(1 << 40)
    need = lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 4 | FLAG)
    assert need > lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 4) > 0
    rc = lib.alo_corr_alt_lookup(one, need - 1, one, one, 1, 8, 8, 8, 4, 4 | FLAG, None)
    assert rc == 1 and b"workspace" in lib.alo_last_error()
    # the unflagged size is not enough for a flagged call
    rc = lib.alo_corr_alt_lookup(one, lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 4), one, one, 1, 8, 8, 8, 4, 4 | FLAG, None)
    assert rc == 1 and b"workspace" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 8, 4 | FLAG, None)
    assert rc == 2 and b"radius" in lib.alo_last_error()
    for levels in (4 | 0x200, 4 | FLAG | 0x200, 4 | 0x4000):
        rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 4, levels, None)
        assert rc == 2 and b"ALO_CORR_ALT_GRAD" in lib.alo_last_error(), levels
    rc = lib.alo_corr_alt_lookup(one, big, None, one, 1, 8, 16, 16, 4, 4 | FLAG, None)
    assert rc == 1 and b"null pointer" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, None, 1, 8, 16, 16, 4, 4 | FLAG, None)
    assert rc == 1 and b"null pointer" in lib.alo_last_error()
    # the unflagged call's checks, in its order, behind the flag
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 4, 9 | FLAG, None)
    assert rc == 1 and b"num_levels" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 8, 8, 4, 5 | FLAG, None)
    assert rc == 1 and b"level 4" in lib.alo_last_error() and b"empty" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(ctypes.c_void_p(24), need, one, one, 1, 8, 8, 8, 4, 4 | FLAG, None)
    assert rc == 1 and b"aligned" in lib.alo_last_error()
    # an unflagged call answers as before
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 4, 9, None)
    assert rc == 1 and b"num_levels" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 8, 4, None)
    assert rc == 2 and b"radius" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 4, -1, None)
    assert rc == 1 and b"num_levels" in lib.alo_last_error()


def test_flagged_workspace_size():
    lib = alo_hip.lib()
    pad = lambda n: (n + 255) // 256 * 256   # noqa: E731
    sizes = [(90, 160), (45, 80), (22, 40), (11, 20)]
    plane = pad(2 * 90 * 160 * 256 * 4)
    plain = plane + sum(pad(2 * h * w * 256 * 4) for h, w in sizes)
    assert lib.alo_corr_alt_workspace_bytes(2, 256, 90, 160, 4) == plain          # unflagged: unchanged
    flagged = lib.alo_corr_alt_workspace_bytes(2, 256, 90, 160, 4 | FLAG)
    assert flagged >= 2 * plain
    assert flagged == plain + 4 * plane + (plain - plane)                          # the documented layout
    assert lib.alo_corr_alt_workspace_bytes(1, 17, 5, 5, 1) == pad(25 * 32 * 4) * 2
    assert lib.alo_corr_alt_workspace_bytes(1, 17, 5, 5, 1 | FLAG) == pad(25 * 32 * 4) * 4
    assert lib.alo_corr_alt_workspace_bytes(1, 70000, 8, 8, 1 | FLAG) == 0         # past the limits
    assert lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 9 | FLAG) == 0
    assert lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 4 | 0x200) == 0            # a stray bit
    assert lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 4 | FLAG | 0x200) == 0
    assert lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 0) == 0 and lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, -1) == 0


def test_grad_views_follow_the_documented_layout():
    lib = alo_hip.lib()
    B, C, H, W, L = 2, 24, 13, 18, 3
    total = lib.alo_corr_alt_workspace_bytes(B, C, H, W, L | FLAG)
    ws = torch.zeros(total, dtype=torch.uint8)
    region, planes, levels = alo_hip.corr_alt_grad_views(ws, (B, C, H, W), L)
    assert region.numel() == total - lib.alo_corr_alt_workspace_bytes(B, C, H, W, L)
    assert [tuple(p.shape) for p in planes] == [(B, H * W, 32)] * L
    assert [tuple(v.shape) for v in levels] == [(2, B, 13 * 18, 16), (2, B, 6 * 9, 16), (2, B, 3 * 4, 16)]
    for k, v in enumerate(planes + levels):   # disjoint, in order, inside the region
        v.fill_(k + 1)
    got = region.view(torch.float32)
    edges = [0] + [int(i) + 1 for i in torch.nonzero(got[1:] != got[:-1]).flatten()]
    assert [got[e].item() for e in edges if got[e].item() != 0] == [1, 2, 3, 4, 5, 6]
    assert not ws[:total - region.numel()].any()
    with pytest.raises(RuntimeError):
        alo_hip.corr_alt_grad_views(ws[:-1], (B, C, H, W), L)


def to_slice_major(g, cp):
    """(B, C, h, w) -> the kernel's (Cp/16, B, h*w, 16), padded channels filled with junk that must be dropped."""
    B, C, h, w = g.shape
    full = torch.full((B, cp, h * w), 7.0, dtype=g.dtype)
    full[:, :C] = g.reshape(B, C, h * w)
    return full.reshape(B, cp // 16, 16, h * w).permute(1, 0, 3, 2).contiguous()


@pytest.mark.parametrize("B,C,H,W,L", [(2, 24, 13, 18, 3), (1, 24, 9, 5, 3), (1, 3, 8, 8, 1)])
def test_host_adjoint_matches_autograd_through_the_pyramid(B, C, H, W, L):
    """Odd sizes (pooling drops a row and a column), padded channels, a last level one pixel wide: fp64 against autograd through
    ``_alt_pyramid`` with the gradients relaid into the kernel's layouts."""
    gen = torch.Generator().manual_seed(B + C + H)
    cp = (C + 15) // 16 * 16
    f1 = torch.randn(B, C, H, W, dtype=torch.float64, generator=gen, requires_grad=True)
    f2 = torch.randn(B, C, H, W, dtype=torch.float64, generator=gen, requires_grad=True)
    pyr = _alt_pyramid(f1, f2, L)[:L]
    if (B, C, H, W, L) == (1, 24, 9, 5, 3):
        assert pyr[-1][1].shape[-1] == 1
    plane_grads = [torch.randn(B, C, H, W, dtype=torch.float64, generator=gen) for _ in range(L)]
    level_grads = [torch.randn(p[1].shape, dtype=torch.float64, generator=gen) for p in pyr]
    loss = sum((f1 * g).sum() for g in plane_grads) + sum((p[1] * g).sum() for p, g in zip(pyr, level_grads))
    want1, want2 = torch.autograd.grad(loss, (f1, f2))
    planes = []
    for g in plane_grads:
        full = torch.full((B, H * W, cp), -3.0, dtype=torch.float64)
        full[:, :, :C] = g.permute(0, 2, 3, 1).reshape(B, H * W, C)
        planes.append(full)
    levels = [to_slice_major(g, cp) for g in level_grads]
    got1, got2 = alt_feature_gradients(planes, levels, (B, C, H, W))
    torch.testing.assert_close(got1, want1)
    torch.testing.assert_close(got2, want2)
    only1 = alt_feature_gradients(planes, levels, (B, C, H, W), need_fmap2=False)
    only2 = alt_feature_gradients(planes, levels, (B, C, H, W), need_fmap1=False)
    assert only1[1] is None and only2[0] is None
    torch.testing.assert_close(only1[0], want1)
    torch.testing.assert_close(only2[1], want2)


def test_exported_and_refuses_cpu_tensors_like_the_alternate_block():
    import alonet.raft
    from alonet.raft import AlternateCorrBlock, TrainableAlternateCorrBlock
    from alonet.raft.corr import TrainableAlternateCorrBlock as FromCorr

    assert TrainableAlternateCorrBlock is FromCorr and "TrainableAlternateCorrBlock" in alonet.raft.__all__
    assert issubclass(TrainableAlternateCorrBlock, AlternateCorrBlock)
    f = torch.randn(1, 8, 16, 16)
    with pytest.raises(RuntimeError) as want:
        AlternateCorrBlock(f, f)
    for grad in (False, True):
        a = f.clone().requires_grad_(grad)
        with pytest.raises(RuntimeError) as got:
            TrainableAlternateCorrBlock(a, f)
        assert str(got.value) == str(want.value)
