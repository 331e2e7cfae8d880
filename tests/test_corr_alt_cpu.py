"""AlternateCorrBlock without a GPU: the torch yardstick on the G6 goldens, and the C ABI of include/alo_corr_alt.h (exports,
argument checks before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import alo_hip
from alonet.raft.corr import TorchAlternateCorrBlock
from helpers import declared_functions


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_torch_block_reproduces_the_g6_corr_block_outputs(golden):
    """The alternate block is CorrBlock's function: its torch form meets CorrBlock's goldens."""
    g = golden("g6_corr.npz")
    blk = TorchAlternateCorrBlock(t(g["f1"]), t(g["f2"]), num_levels=4, radius=4)
    for k in "abc":
        out = blk(t(g["coords_" + k]))
        assert out.shape == g["out_" + k].shape and out.dtype == torch.float32
        np.testing.assert_allclose(out.numpy(), g["out_" + k], rtol=0, atol=3e-5)
    blk = TorchAlternateCorrBlock(t(g["f1o"]), t(g["f2o"]), num_levels=4, radius=3)
    np.testing.assert_allclose(blk(t(g["coords_o"])).numpy(), g["out_o"], rtol=0, atol=3e-5)


def test_torch_block_keeps_the_reference_pyramid():
    f = torch.randn(2, 8, 20, 24)
    blk = TorchAlternateCorrBlock(f, f * 2, num_levels=4, radius=2)
    assert len(blk.pyramid) == 5   # the reference pools num_levels times (the last pair is never read)
    assert [tuple(p[1].shape[-2:]) for p in blk.pyramid] == [(20, 24), (10, 12), (5, 6), (2, 3), (1, 1)]
    torch.testing.assert_close(blk.pyramid[1][0], torch.nn.functional.avg_pool2d(f, 2, stride=2))


def test_library_exports_every_function_of_the_header():
    names = declared_functions("alo_corr_alt.h")
    assert names == ["alo_corr_alt_lookup", "alo_corr_alt_prepare", "alo_corr_alt_workspace_bytes"]
    lib = alo_hip.lib()
    for name in names:
        assert hasattr(lib, name), f"{name} missing from {alo_hip.LIB_PATH}"


def test_workspace_size():
    lib = alo_hip.lib()
    # channels padded to 16, every part rounded up to 256 bytes: fmap1 + levels 0..L-1 of fmap2
    pad = lambda n: (n + 255) // 256 * 256   # noqa: E731
    want = pad(2 * 90 * 160 * 256 * 4) + sum(pad(2 * h * w * 256 * 4) for h, w in [(90, 160), (45, 80), (22, 40), (11, 20)])
    assert lib.alo_corr_alt_workspace_bytes(2, 256, 90, 160, 4) == want
    assert lib.alo_corr_alt_workspace_bytes(1, 17, 5, 5, 1) == pad(25 * 32 * 4) * 2
    assert lib.alo_corr_alt_workspace_bytes(1, 70000, 8, 8, 1) == 0   # past the limits
    assert lib.alo_corr_alt_workspace_bytes(1, 256, 540, 960, 4) > 0  # 7680x4320 frames at 1/8 resolution


def test_argument_errors_are_reported_before_any_launch():
    lib = alo_hip.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    ptrs = (ctypes.c_void_p * 8)(*([16] * 8))
    big = ctypes.c_size_t(1 << 40)
    # lookup: radius, null pointers, empty level, undersized workspace, limits
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 8, 4, None)
    assert rc == 2 and b"radius" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, -1, 4, None)
    assert rc == 2 and b"radius" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(None, big, one, one, 1, 8, 16, 16, 4, 4, None)
    assert rc == 1 and b"null pointer" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, None, 1, 8, 16, 16, 4, 4, None)
    assert rc == 1 and b"null pointer" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 8, 8, 4, 5, None)   # level 4 of an 8x8 grid is 0x0
    assert rc == 1 and b"level 4" in lib.alo_last_error() and b"empty" in lib.alo_last_error()
    need = lib.alo_corr_alt_workspace_bytes(1, 8, 8, 8, 4)
    rc = lib.alo_corr_alt_lookup(one, need - 1, one, one, 1, 8, 8, 8, 4, 4, None)
    assert rc == 1 and b"workspace" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(ctypes.c_void_p(24), need, one, one, 1, 8, 8, 8, 4, 4, None)   # not 16-byte aligned
    assert rc == 1 and b"aligned" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 10000, 10000, 4, 4, None)
    assert rc == 2 and b"limits" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 70000, 16, 16, 4, 4, None)
    assert rc == 2 and b"limits" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 70000, 8, 16, 16, 4, 4, None)
    assert rc == 2 and b"limits" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 0, 16, 16, 4, 4, None)
    assert rc == 1 and b"positive" in lib.alo_last_error()
    rc = lib.alo_corr_alt_lookup(one, big, one, one, 1, 8, 16, 16, 4, 9, None)
    assert rc == 1 and b"num_levels" in lib.alo_last_error()
    # prepare: null pointers (a null level included), empty level, undersized workspace, limits
    rc = lib.alo_corr_alt_prepare(None, ptrs, one, big, 1, 8, 16, 16, 4, None)
    assert rc == 1 and b"null pointer" in lib.alo_last_error()
    holes = (ctypes.c_void_p * 4)(16, 16, None, 16)
    rc = lib.alo_corr_alt_prepare(one, holes, one, big, 1, 8, 16, 16, 4, None)
    assert rc == 1 and b"fmap2_levels[2] is null" in lib.alo_last_error()
    rc = lib.alo_corr_alt_prepare(one, ptrs, one, big, 1, 8, 1, 64, 2, None)
    assert rc == 1 and b"level 1" in lib.alo_last_error() and b"empty" in lib.alo_last_error()
    need = lib.alo_corr_alt_workspace_bytes(1, 8, 16, 16, 4)
    rc = lib.alo_corr_alt_prepare(one, ptrs, one, need - 1, 1, 8, 16, 16, 4, None)
    assert rc == 1 and b"workspace" in lib.alo_last_error()
    rc = lib.alo_corr_alt_prepare(one, ptrs, None, need, 1, 8, 16, 16, 4, None)
    assert rc == 1 and b"workspace" in lib.alo_last_error()
    rc = lib.alo_corr_alt_prepare(one, ptrs, one, big, 1, 8, 1 << 14, 1 << 13, 4, None)
    assert rc == 2 and b"limits" in lib.alo_last_error()


def test_cpu_tensors_are_refused_like_corr_build():
    from alonet.raft.corr import AlternateCorrBlock

    f = torch.randn(1, 8, 16, 16)
    with pytest.raises(RuntimeError) as want:
        alo_hip.corr_build(f, f, 4)
    with pytest.raises(RuntimeError) as got:
        AlternateCorrBlock(f, f)
    assert str(got.value) == str(want.value)
