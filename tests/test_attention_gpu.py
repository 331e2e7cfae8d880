"""``alo_hip.attention`` (ALO_BLOCK_ATTENTION of include/alo_encoder_block.h, csrc/attention.hip) against the fp64 yardstick of
tests/attention_ref.py, every launch inside ``guarded.GuardedLaunches``: the kernel stays in its buffers, never reads a key past Lk
(not even multiplied by zero: the guard behind the last k and v row is NaN in one run and finite in the other) and overwrites all of
``out``.  The packed form (q and k the halves of one (B, L, 512) tensor) shares one storage, which the harness relocates as one hull.

The bound, per output of head h of query i, with u the unit roundoff tests/test_backbone_kernels_gpu.py takes for the storage type
(2^-8 bf16, 2^-11 fp16), A = max |v| over the image's unmasked keys, c_acc of tests/kernel_bounds.py:

    |err| <= 2 A (u_out + u_P + 2 ds + c_acc(Lk) 2^-24),      ds = c_acc(32) 2^-24 scale max_k sum_d |q_d k_d|

  * out = sum_k p_k v_k / sum_k p_k is a convex combination of the v_k, so a relative error e_k on each p_k moves it by at most
    2 A max_k |e_k| (numerator and denominator each by a factor within 1 +- max |e_k|);
  * e_k has three sources: the score's error ds (an fp32 dot product of 32 exact products, scaled in fp32) enters through
    exp(s + ds) = p (1 + ds + ..), once for the key and once for the running max it is measured against: 2 ds; the rounding of p to
    the storage type before the second product: u_P = u (16-bit flavours; the sum l is taken on the unrounded p, so the two no longer
    cancel), u_P = 0 for fp32 operands; the exponential's own error, which with the second-order terms is what the leading 2 is for;
  * the second product and l are fp32 sums of Lk terms of one sign pattern: c_acc(Lk) 2^-24 relative to A;
  * the result is rounded once to the storage type: u_out = u, or 2^-24 in fp32.

c_acc(n) of tests/kernel_bounds.py is (n + 1) 2^-23, so ``c_acc(32) 2^-24`` and ``c_acc(Lk) 2^-24`` are of the order 1e-12: in fp32 the
bound comes to 2 A 2^-24, one ulp of max |v|, which no fp32 arithmetic on the scores can hold (at |score| ~ 100 the rounding of one
fp32 score, 100 x 2^-24, is 50 times the bound).  The fp32 flavour therefore widens its operands and runs both products, the
exponentials and the sums in fp64; its only rounding is the store's, 2^-24 |out| <= 2^-24 A.

Measured on an MI355X (worst |err| / bound; docs/experiments.md, "Dense attention"): bf16 0.10 over the sizes and masks and 0.13 at
|score| ~ 100, fp16 0.09 and 0.13, fp32 0.23 and 0.32.  (A first fp32 kernel on the fp32 matrix instructions measured 0.79 - 2.09, 3.5
on the constant heads and 30 at |score| ~ 100, and was replaced.)

Sizes: QB = 32 queries per wave, KT = 32 keys per tile; the host takes 2 or 4 waves per workgroup once that still gives each of the
device's compute units a workgroup, which at 256 compute units the two B = 16 cases do (2 waves at 70 queries, 4 at 129; the last
workgroup of each then holds a wave with a partial block and waves with no query at all).
"""
import pytest
import torch

import alo_hip
from attention_ref import HEAD_DIM, HEADS, UNIT_ROUNDOFF, attention_bound, attention_ref
from guarded import GuardedLaunches
from kernel_bounds import compare

pytestmark = pytest.mark.gpu

QB, KT, E = 32, 32, HEADS * HEAD_DIM
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
DEV = "cuda"


class _Seam:
    """The launch seam: what reaches ``alo_hip._launch`` (symbol, the dtype word), then the real launch."""

    def __init__(self):
        self.real, self.calls = alo_hip._launch, []

    def __call__(self, symbol, device, tag, nbytes, flops, *args, relaunch=False):
        self.calls.append((symbol, args[-1], tag))
        return self.real(symbol, device, tag, nbytes, flops, *args, relaunch=relaunch)


def _operands(B, Lq, Lk, dtype, seed, packed=False, q_scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if packed:
        assert Lq == Lk
        qk = torch.randn(B, Lq, 2 * E, device=DEV, generator=g)
        qk[..., :E] *= q_scale
        qk = qk.to(dtype)
        q, k = qk[..., :E], qk[..., E:]
    else:
        q = (torch.randn(B, Lq, E, device=DEV, generator=g) * q_scale).to(dtype)
        k = torch.randn(B, Lk, E, device=DEV, generator=g).to(dtype)
    v = (torch.randn(B, Lk, E, device=DEV, generator=g) * 2 + 0.5).to(dtype)
    return q, k, v


def _run(q, k, v, mask, packed):
    """The guarded launch -> out; asserts through the seam that alo_encoder_block got the attention flag (and the packed one)."""
    seam = _Seam()
    packed = packed and not (q.is_contiguous() and k.is_contiguous())   # one row: the halves are contiguous tensors of their own
    with GuardedLaunches(real_launch=seam) as guard:
        out = alo_hip.attention(q, k, v, mask)
    assert [s for s, _ in guard.seen] == ["alo_encoder_block"] and guard.seen[0][1] == f"attention/Lq={q.shape[1]}/Lk={k.shape[1]}"
    assert len(seam.calls) == 2   # one launch, run under both fills
    for symbol, word, _ in seam.calls:
        assert symbol == "alo_encoder_block" and word & alo_hip.ALO_BLOCK_ATTENTION
        assert bool(word & alo_hip.ALO_BLOCK_PACKED_QK) == packed and word & 0xff == alo_hip._DTYPE_CODE[q.dtype]
        assert word & ~(0xff | alo_hip.ALO_BLOCK_ATTENTION | alo_hip.ALO_BLOCK_PACKED_QK) == 0
    assert out.shape == (q.shape[0], q.shape[1], E) and out.dtype == q.dtype and out.is_contiguous()
    return out


def _check(q, k, v, mask, packed, what):
    out = _run(q, k, v, mask, packed)
    ratio = compare(out, attention_ref(q, k, v, mask), attention_bound(q, k, v, mask, q.dtype), what)
    print(f"{what}: worst |err| / bound = {ratio:.3g}")
    return out


def _mask(kind, B, Lk):
    m = torch.zeros(B, Lk, dtype=torch.bool, device=DEV)
    if kind == "ragged":                 # valid lengths per image: Lk, Lk - 7, about half, 1
        lengths = [Lk, max(Lk - 7, 1), (Lk + 1) // 2, 1]
        for b in range(B):
            m[b, lengths[b % 4]:] = True
    elif kind == "late_start":           # the first KT + 3 keys masked: the running max is -inf for a whole tile and more
        m[:, :KT + 3] = True
    elif kind == "middle_tile":
        m[:, KT:2 * KT] = True
    elif kind == "last_key_only":
        m[:, :-1] = True
    elif kind == "one_image_dead":       # its rows NaN, the other images unaffected
        m[B - 1] = True
        m[0, 3:11] = True
    else:
        assert kind == "none"
        return None
    return m


SIZES = [(1, 1, 1), (2, 33, 65),
         (2, QB - 1, 40), (2, QB, 40), (2, QB + 1, 40), (2, 4 * QB + 1, 40),
         (2, 33, KT - 1), (2, 33, KT), (2, 33, KT + 1), (2, 33, 2 * KT), (2, 33, 2 * KT + 1),
         (2, 100, 131), (3, 75, 75),
         (16, 70, 40), (16, 4 * QB + 1, 40)]
SIZES = list(dict.fromkeys(SIZES))   # (2, 33, 2 KT + 1) is (2, 33, 65)


@DT
@pytest.mark.parametrize("B,Lq,Lk", SIZES, ids=[f"{b}x{lq}x{lk}" for b, lq, lk in SIZES])
def test_sizes_without_a_mask(B, Lq, Lk, dtype):
    for packed in ((False, True) if Lq == Lk else (False,)):
        q, k, v = _operands(B, Lq, Lk, dtype, seed=Lq * 1000 + Lk, packed=packed)
        _check(q, k, v, None, packed, f"attention {B}x{Lq}x{Lk} {dtype} packed={packed}")


@DT
@pytest.mark.parametrize("kind", ["ragged", "late_start", "middle_tile", "last_key_only", "one_image_dead"])
@pytest.mark.parametrize("B,Lq,Lk,packed", [(2, 33, 65, False), (2, 100, 131, False), (3, 75, 75, True)],
                         ids=["2x33x65", "cross_2x100x131", "packed_3x75x75"])
def test_masks(B, Lq, Lk, packed, kind, dtype):
    q, k, v = _operands(B, Lq, Lk, dtype, seed=17 + Lk, packed=packed)
    mask = _mask(kind, B, Lk)
    out = _check(q, k, v, mask, packed, f"attention {B}x{Lq}x{Lk} {dtype} mask={kind} packed={packed}")
    dead = mask.all(1)
    assert torch.isnan(out[dead]).all() and torch.isfinite(out[~dead]).all()
    assert bool(dead.any()) == (kind == "one_image_dead")
    if dtype == torch.bfloat16:   # a uint8 mask is the same launch
        again = alo_hip.attention(q, k, v, mask.to(torch.uint8))
        assert torch.equal(again.isnan(), out.isnan()) and torch.equal(torch.nan_to_num(again), torch.nan_to_num(out))


# ---- exact data: the layout of both products, asymmetric in every index ----------------------------------------------------------
@DT
@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
def test_zero_queries_give_the_mean_of_the_unmasked_values(dtype, packed):
    B, L = 3, 75
    q, k, _ = _operands(B, L, L, dtype, seed=3, packed=packed)
    q.zero_()
    key, col = torch.arange(L, device=DEV)[:, None], torch.arange(E, device=DEV)[None, :]
    v = ((37 * key + col) % 64).to(dtype).expand(B, L, E).contiguous()       # integers below 64: exact in every type, every sum exact
    mask = _mask("ragged", B, L)
    out = _run(q, k, v, mask, packed)
    keep = (~mask).double()
    mean = (keep[:, :, None] * v.double()).sum(1) / keep.sum(1)[:, None]        # (B, E)
    u_out = 2.0 ** -24 if dtype == torch.float32 else UNIT_ROUNDOFF[dtype]
    err = (out.double() - mean[:, None, :]).abs()
    assert bool((err <= (u_out + 2.0 ** -23) * mean[:, None, :].abs()).all()), err.max().item()   # one division, one rounding


@DT
@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
def test_a_single_unmasked_key_gives_its_value_row_bit_for_bit(dtype, packed):
    B, L = 3, 75
    q, k, v = _operands(B, L, L, dtype, seed=4, packed=packed)
    alive = [0, 37, 74]                       # first tile's first key, a middle one, the last key of the last (partial) tile
    mask = torch.ones(B, L, dtype=torch.bool, device=DEV)
    for b, j in enumerate(alive):
        mask[b, j] = False
    out = _run(q, k, v, mask, packed)
    for b, j in enumerate(alive):
        assert torch.equal(out[b], v[b, j].expand(L, E)), (b, j)


@DT
@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
def test_a_dominant_key_selects_its_value_row(dtype, packed):
    """k_j = the +-1 code of j's bits (head h: rotated by h channels), q_i = 512 x the code of pi(i), pi(i) = 3 i + 1 mod L (no
    involution): the score of pi(i) beats every other by at least 2 x 512 / sqrt(32) = 181, so p is exactly 1 there and 0 elsewhere."""
    B, L = 2, 70
    code = torch.ones(L, HEAD_DIM, device=DEV)
    for bit in range(7):
        code[:, bit] = 1.0 - 2.0 * ((torch.arange(L, device=DEV) >> bit) & 1)
    heads = torch.cat([code.roll(h, dims=1) for h in range(HEADS)], dim=1)          # (L, 256)
    pi = (3 * torch.arange(L, device=DEV) + 1) % L
    assert not torch.equal(pi[pi], torch.arange(L, device=DEV))
    qk = torch.empty(B, L, 2 * E, device=DEV, dtype=dtype)
    qk[..., :E] = (512.0 * heads[pi]).to(dtype)
    qk[..., E:] = heads.to(dtype)
    q, k = (qk[..., :E], qk[..., E:]) if packed else (qk[..., :E].contiguous(), qk[..., E:].contiguous())
    _, _, v = _operands(B, L, L, dtype, seed=6)
    out = _run(q, k, v, None, packed)
    assert torch.equal(out, v[:, pi])


@DT
def test_heads_filled_with_different_constants_do_not_mix(dtype):
    B, Lq, Lk = 2, 33, 65
    q, k, v = _operands(B, Lq, Lk, dtype, seed=8)
    const = torch.arange(1, HEADS + 1, device=DEV).repeat_interleave(HEAD_DIM).to(dtype)      # head h: h + 1
    v = const.expand(B, Lk, E).contiguous()
    out = _check(q, k, v, _mask("ragged", B, Lk), False, f"attention constant heads {dtype}")
    assert bool(((out.double() - const.double()).abs() <= 2.0 ** -6 * const.double()).all())


@DT
def test_scores_near_80_neither_overflow_nor_leave_the_bound(dtype):
    B, Lq, Lk = 2, 100, 131
    q, k, v = _operands(B, Lq, Lk, dtype, seed=9, q_scale=20.0)
    scores = torch.einsum("bqhd,bkhd->bhqk", q.double().view(B, Lq, HEADS, HEAD_DIM), k.double().view(B, Lk, HEADS, HEAD_DIM)) * HEAD_DIM ** -0.5
    assert 60 < scores.abs().max().item() < 120
    out = _check(q, k, v, _mask("ragged", B, Lk), False, f"attention scores to {scores.abs().max().item():.0f} {dtype}")
    assert torch.isfinite(out).all()


@DT
def test_a_captured_graph_replays_the_eager_launch_bit_for_bit(dtype):
    B, L = 3, 75
    q, k, v = _operands(B, L, L, dtype, seed=10, packed=True)
    mask = _mask("ragged", B, L)
    eager = alo_hip.attention(q, k, v, mask)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = alo_hip.attention(q, k, v, mask)
    replayed.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)


def test_an_operand_that_requires_grad_is_refused():
    q, k, v = _operands(1, 5, 5, torch.float32, seed=11)
    with pytest.raises(RuntimeError, match="no backward"):
        alo_hip.attention(q.requires_grad_(), k, v)
    with torch.no_grad():
        alo_hip.attention(q, k, v)
