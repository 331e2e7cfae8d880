"""alo_hip.gru_gate_rows_ / gru_update_rows_: the channels-last flavour of alo_gru_gate / alo_gru_update (B = rows, HW = 1;
aloception-oss_amd/csrc/fused.hip).  Same formulas per element as the planar kernels: their results bit for bit on the permuted data,
and inside kernel_bounds.gru_bound against the fp64 formulas, the bar of test_glue_kernels_gpu.py.  Every launch runs under the guard of
guarded.py with the existing role table."""
import pytest
import torch

import alo_hip
import guarded
import kernel_bounds as kb
from kernel_bounds import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731

# (rows as (B, H, W) of the planar twin, C, Cx)
CASES = [((1, 1, 1), 4, 4), ((1, 7, 11), 128, 256), ((2, 4, 6), 8, 12)]


def _buffers(shape, c, cx, seed):
    """Planar operands (H*W may be odd: the planar kernels get a 4-fold padded copy below) drawn as test_glue_kernels_gpu.py draws them."""
    b, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    zr = torch.randn(b, 2 * c, h, w, device=DEV, generator=g) * 2
    hx = torch.randn(b, c + cx, h, w, device=DEV, generator=g)
    hx[:, :c] = torch.tanh(hx[:, :c])
    rhx = torch.randn(b, c + cx, h, w, device=DEV, generator=g)
    q = torch.randn(b, c, h, w, device=DEV, generator=g) * 2
    return zr, hx, rhx, q, torch.randn(2 * c, device=DEV, generator=g), torch.randn(c, device=DEV, generator=g)


def _rows(t):
    """(B, C, H, W) -> a fresh contiguous (B H W, C) matrix."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _planar(zr, hx, rhx, q, bzr, bq, c, with_net):
    """The planar kernels on the same values, each plane repeated to four times its length (they need H*W % 4 == 0, and every element
    is computed on its own); -> z | r, r*h | x, h' | x, net as row matrices."""
    wide = lambda t: t.flatten(2).repeat(1, 1, 4).unsqueeze(-1).contiguous()      # noqa: E731  (B, C, 4 HW, 1)
    narrow = lambda t, like: t[:, :, :like.shape[2] * like.shape[3], 0].reshape(like.shape[0], -1, *like.shape[2:])   # noqa: E731
    zr4, hx4, rhx4, q4 = wide(zr), wide(hx), wide(rhx), wide(q)
    net4 = torch.full_like(q4, 3.0) if with_net else None
    alo_hip.gru_gate_(zr4, bzr, hx4, rhx4, c)
    alo_hip.gru_update_(q4, bq, zr4, hx4, c, net4)
    return [_rows(narrow(t, zr)) for t in (zr4, rhx4, hx4)] + [None if net4 is None else _rows(narrow(net4, zr))]


@pytest.mark.parametrize("with_net", [True, False], ids=["net", "no-net"])
@pytest.mark.parametrize("shape,c,cx", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rows_kernels_equal_the_planar_kernels_and_meet_their_bound(shape, c, cx, with_net):
    zr, hx, rhx, q, bzr, bq = _buffers(shape, c, cx, seed=c + cx)
    want_zr, want_rhx, want_hx, want_net = _planar(zr, hx, rhx, q, bzr, bq, c, with_net)
    zr_r, hx_r, rhx_r, q_r = _rows(zr), _rows(hx), _rows(rhx), _rows(q)
    assert hx_r.stride(0) == c + cx and zr_r.shape == (shape[0] * shape[1] * shape[2], 2 * c)
    zr0, hx0, rhx0 = zr_r.clone(), hx_r.clone(), rhx_r.clone()
    h0 = hx0[:, :c]
    as_maps = lambda m: m.t()[None, :, :, None]      # noqa: E731  (rows, C) -> (1, C, rows, 1) for the NCHW references
    bound = kb.gru_bound(as_maps(h0))

    with guarded.GuardedLaunches() as g:
        alo_hip.gru_gate_rows_(zr_r, bzr, hx_r, rhx_r, c)
    assert [s for s, _ in g.seen] == ["alo_gru_gate"]
    z_ref, rh_ref = kb.gru_gate_ref(as_maps(zr0), bzr, as_maps(h0))
    worst = max(compare(as_maps(zr_r[:, :c]), z_ref, bound, "rows gate: z"), compare(as_maps(rhx_r[:, :c]), rh_ref, bound, "rows gate: r * h"))
    assert torch.equal(bits(zr_r[:, c:]), bits(zr0[:, c:])), "the r half of zr changed"
    assert torch.equal(bits(rhx_r[:, c:]), bits(rhx0[:, c:])) and torch.equal(bits(hx_r), bits(hx0)), "channels >= C / hx changed"
    assert torch.equal(bits(zr_r), bits(want_zr)) and torch.equal(bits(rhx_r), bits(want_rhx)), "not the planar gate kernel's bits"

    z = zr_r[:, :c].clone()
    zr1 = zr_r.clone()
    net = torch.full_like(q_r, 3.0) if with_net else None
    with guarded.GuardedLaunches() as g:
        alo_hip.gru_update_rows_(q_r, bq, zr_r, hx_r, c, net)
    assert [s for s, _ in g.seen] == ["alo_gru_update"]
    new_ref = kb.gru_update_ref(as_maps(q_r), bq, as_maps(z), as_maps(h0))
    worst = max(worst, compare(as_maps(hx_r[:, :c]), new_ref, bound, "rows update"))
    assert torch.equal(bits(hx_r[:, c:]), bits(hx0[:, c:])) and torch.equal(bits(zr_r), bits(zr1))
    assert torch.equal(bits(hx_r), bits(want_hx)), "not the planar update kernel's bits"
    if with_net:
        assert torch.equal(bits(net), bits(hx_r[:, :c])) and torch.equal(bits(net), bits(want_net))
    print(f"rows={zr_r.shape[0]} C={c} Cx={cx} net={with_net}: kernels {worst:.3g} of the bound")


def test_rows_wrappers_refuse_what_the_kernels_cannot_take():
    zr, hx, rhx, q, bzr, bq = _buffers((1, 2, 3), 8, 8, seed=1)
    zr_r, hx_r, rhx_r, q_r = _rows(zr), _rows(hx), _rows(rhx), _rows(q)
    with pytest.raises(RuntimeError, match="gru_gate_rows_"):
        alo_hip.gru_gate_rows_(zr_r[:, :12].contiguous(), bzr[:12], hx_r, rhx_r, 6)          # C % 4
    with pytest.raises(RuntimeError, match="zr must be"):
        alo_hip.gru_gate_rows_(zr, bzr, hx_r, rhx_r, 8)                                      # a 4-d map is the planar wrapper's
    with pytest.raises(RuntimeError, match="gru_update_rows_"):
        alo_hip.gru_update_rows_(q_r, bq, zr_r, hx_r[:3].contiguous(), 8)
    lib = alo_hip.lib()
    ptr = lambda t: t.data_ptr()   # noqa: E731
    rc = lib.alo_gru_gate(ptr(zr_r), ptr(bzr), ptr(hx_r), ptr(rhx_r), 6, 6, 1, 16, 16, None)  # HW = 1 with C % 4 != 0: refused, not launched
    assert rc == 1 and b"multiples of 4" in lib.alo_last_error()
    rc = lib.alo_gru_gate(ptr(zr_r), ptr(bzr), ptr(hx_r), ptr(rhx_r), 1, 8, 6, 96, 96, None)  # the planar refusal is as it was
    assert rc == 1 and b"H*W and the batch strides must be multiples of 4" in lib.alo_last_error()
