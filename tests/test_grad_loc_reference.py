"""The grad_sampling_loc reference for pixel edges (helpers.grad_loc_reference / grad_loc_one_sided) against the float64 C oracle (CPU).

grad_sampling_loc jumps where an image coordinate loc * size - 0.5 crosses an integer; the GPU parity tests compare every sample
against these helpers instead of masking the samples near an edge, so the helpers themselves are pinned here."""
import numpy as np

import oracle as O
from helpers import DYADIC_SHAPES, _edge_sizes, exact_edge_case, grad_loc_one_sided, grad_loc_reference, msda_case

ODD_SHAPES = [(25, 42), (13, 21), (7, 11), (3, 5)]


def _oracle(c, loc=None):
    loc = c["loc"] if loc is None else loc
    return O.msda_backward(c["value"].astype(np.float64), c["shapes"], c["level_start"], np.asarray(loc, np.float64),
                           c["attn"].astype(np.float64), c["grad_out"].astype(np.float64))[1]


def _image(c):
    return c["loc"].astype(np.float64) * _edge_sizes(c["shapes"], len(c["shapes"])) - 0.5


def test_exact_edges_take_the_right_hand_cell():
    """Dyadic pyramid, coordinates exactly on integers: the reference's floor() takes the cell to the right / below, i.e. each edge
    component equals the oracle with that coordinate moved to k + 0.5; coordinates exactly -1 or size drop the sample."""
    c = exact_edge_case(3, 2, 3, 8, 24)
    ref = grad_loc_reference(c["value"], c["shapes"], c["level_start"], c["loc"], c["attn"], c["grad_out"])
    t = _image(c)
    size = _edge_sizes(c["shapes"], 4)
    on = t == np.floor(t)
    inner = on & (t >= 0) & (t <= size - 1)
    dropped = (on & ((t == -1) | (t == size))).any(-1)
    assert inner[..., 0].sum() > 50 and inner[..., 1].sum() > 50 and dropped.sum() > 50
    assert (inner & (t == size - 1)).sum() > 10 and (inner & (t == 0)).sum() > 10
    for axis in (0, 1):
        moved = c["loc"].astype(np.float64)
        moved[..., axis] = np.where(inner[..., axis], (t[..., axis] + 1.0) / size[..., axis], moved[..., axis])
        right = _oracle(c, moved)[..., axis]
        sel = inner[..., axis] & ~dropped
        assert np.array_equal(ref[..., axis][sel], right[sel])
    assert np.all(ref[dropped] == 0)
    assert np.abs(ref[~dropped]).max() > 0.1
    # exact edges: the float64 oracle's floor() already sits in the right-hand cell
    assert np.array_equal(ref, _oracle(c))


def test_rounded_edges_differ_from_the_oracle_and_take_one_side():
    """Non-dyadic sizes, float32 locations that the float32 fma rounds onto an integer although the exact coordinate lies just
    below it: there the reference (and the helper) work in the cell above, the float64 oracle in the cell below."""
    rng = np.random.default_rng(7)
    c = msda_case(8, 2, 4, 8, 40, ODD_SHAPES, 4)
    size = _edge_sizes(c["shapes"], 4)
    k = np.floor(rng.uniform(-1, size + 1, c["loc"].shape))
    near = ((k + 0.5) / size).astype(np.float32)                 # t = k +- an fp32 ulp of the location, times size
    c["loc"] = np.where(rng.random(c["loc"].shape) < 0.7, near, c["loc"]).astype(np.float32)
    t = _image(c)
    r = t.astype(np.float32).astype(np.float64)
    below = (r == np.floor(r)) & (t < r)                         # rounds UP onto an integer: the reference's cell != the oracle's
    assert below.sum() > 100
    ref = grad_loc_reference(c["value"], c["shapes"], c["level_start"], c["loc"], c["attn"], c["grad_out"])
    plain = _oracle(c)
    jumped = below & (r >= 0) & (r <= size - 1)
    assert np.abs(ref - plain)[jumped].max() > 1e-2               # the jump the masks used to hide
    # every component is one of the two one-sided derivatives (candidates over the float64 neighbourhood of the edge)
    cands = grad_loc_one_sided(c["value"], c["shapes"], c["level_start"], c["loc"], c["attn"], c["grad_out"], eps=1e-4)
    assert (np.abs(ref[None] - cands) <= 1e-9 * max(1.0, np.abs(plain).max())).any(0).all()
    # samples with no integer r: the plain oracle bit for bit (over the same query subset too)
    none = ~(r == np.floor(r)).any(-1)
    assert none.sum() > 100 and np.array_equal(ref[none], plain[none])
    sub = grad_loc_reference(c["value"], c["shapes"], c["level_start"], c["loc"], c["attn"], c["grad_out"], queries=slice(3, 40, 7))
    assert np.array_equal(sub, ref[:, 3:40:7])
    # r == -1 or r == size: the reference's `> -1 && < size` test drops the sample, both components are 0
    drop = ((r == -1) | (r == size)).any(-1)
    assert drop.sum() > 20 and np.all(ref[drop] == 0)


def test_one_sided_candidates_on_exact_edges_hold_the_right_hand_value():
    c = exact_edge_case(5, 1, 2, 8, 16, DYADIC_SHAPES, dtype=np.float64)
    ref = grad_loc_reference(c["value"], c["shapes"], c["level_start"], c["loc"].astype(np.float32), c["attn"], c["grad_out"])
    cands = grad_loc_one_sided(c["value"], c["shapes"], c["level_start"], c["loc"], c["attn"], c["grad_out"])
    assert (ref[None] == cands).any(0).all()
    # and the left-hand side is a real alternative on interior edges (the candidates are not all the same value)
    t = _image(c)
    inner = (t == np.floor(t)) & (t >= 0) & (t <= _edge_sizes(c["shapes"], 4) - 1)
    assert np.abs(cands[0] - cands[1])[inner].max() > 1e-2
