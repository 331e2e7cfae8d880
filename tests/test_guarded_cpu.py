"""The guarded-launch harness (tests/guarded.py) proves itself on CPU tensors: ``real_launch`` is a Python function in the role of a
kernel.  A correct fake passes; every planted defect is reported with its kind and argument.  Defects live in these fakes only.
Two census tests hold the role table to the library's entry points and to the GPU sweep."""
import ctypes
import re

import pytest
import torch

import alo_hip
import guarded
from guarded import INOUT, OUT, WORK, BufferDisciplineError, GuardedLaunches

G = 1024   # guard bytes of these tests (a multiple of 256): the checks do not depend on the size


def run(kernel, roles, *args, guard_bytes=G):
    """Launch ``kernel(*tensors and scalars)`` as symbol "k" through ``alo_hip._launch`` under the harness."""
    def real(symbol, device, tag, nbytes, flops, *a, relaunch=False):
        kernel(*a)

    with GuardedLaunches(real_launch=real, guard_bytes=guard_bytes, roles={"k": roles}) as g:
        alo_hip._launch("k", "cpu", "k/tag", 0.0, 0.0, *args)
    return g


def flat(t):
    """A 1-D view over everything from ``t``'s first element on, to plant out-of-bounds accesses with."""
    return t.as_strided((t.untyped_storage().nbytes() // t.element_size() - t.storage_offset(),), (1,), t.storage_offset())


def before(t, n=1):
    return t.as_strided((n,), (1,), t.storage_offset() - n)


def scale(x, y):
    y.copy_(2 * x)


def test_a_correct_kernel_passes_and_its_result_is_copied_back():
    x, y = torch.arange(7.0), torch.empty(7)
    g = run(scale, {1: OUT}, x, y)
    assert torch.equal(y, 2 * torch.arange(7.0)) and torch.equal(x, torch.arange(7.0))
    assert g.seen == [("k", "k/tag")]
    assert alo_hip._launch.__module__ == "alo_hip" and alo_hip._launch.__name__ == "_launch"   # restored on exit


def test_the_default_guard_is_one_tile_of_the_widest_kernel():
    assert guarded.DEFAULT_GUARD_BYTES == 64 * 2048 * 2 and guarded.DEFAULT_GUARD_BYTES % 256 == 0
    x, y = torch.arange(7.0), torch.empty(7)
    run(scale, {1: OUT}, x, y, guard_bytes=guarded.DEFAULT_GUARD_BYTES)
    with pytest.raises(ValueError):
        GuardedLaunches(guard_bytes=100)


def expect(kind, position, offset=None, item=None):
    class Ctx:
        def __enter__(self):
            self.r = pytest.raises(BufferDisciplineError)
            self.info = self.r.__enter__()
            return self

        def __exit__(self, *exc):
            out = self.r.__exit__(*exc)
            e = self.info.value
            assert (e.symbol, e.kind, e.position, e.item) == ("k", kind, position, item), str(e)
            if offset is not None:      # the first byte that differs lies somewhere inside the fp32 element at this offset
                assert e.offset // 4 * 4 == offset, str(e)
            assert "k:" in str(e) and kind in str(e) and f"argument {position}" in str(e)
            return out
    return Ctx()


def test_a_store_one_element_past_the_end():
    def kernel(x, y):
        flat(y)[:8] = 1.0
    with expect("guard-after", 1, offset=7 * 4):
        run(kernel, {1: OUT}, torch.arange(7.0), torch.empty(7))


def test_a_store_one_element_before_the_start():
    def kernel(x, y):
        scale(x, y)
        before(y)[0] = 1.0
    with expect("guard-before", 1, offset=-4):
        run(kernel, {1: OUT}, torch.arange(7.0), torch.empty(7))


def test_one_output_element_left_unwritten():
    def kernel(x, y):
        y[:6] = 2 * x[:6]
    with expect("differs-between-fills", 1, offset=6 * 4):
        run(kernel, {1: OUT}, torch.arange(7.0), torch.empty(7))


def test_a_read_one_element_past_the_input_times_zero():
    def kernel(x, y):
        y.copy_(2 * x)
        y[6] += 0.0 * flat(x)[7]     # NaN under the first fill, finite under the second
    with expect("differs-between-fills", 1, offset=6 * 4):
        run(kernel, {1: OUT}, torch.arange(7.0), torch.empty(7))


def test_an_input_modified():
    def kernel(x, y):
        scale(x, y)
        x[3] = -1.0
    with expect("input-modified", 0, offset=3 * 4):
        run(kernel, {1: OUT}, torch.arange(7.0), torch.empty(7))


def test_a_gap_of_a_batch_strided_output_written():
    flat_out = torch.zeros(2, 10, 4)
    out = flat_out[:, 2:5]                      # (2, 3, 4) rows inside a (2, 10, 4) buffer: batch stride 40 > 12
    x = torch.arange(24.0).reshape(2, 3, 4)
    g = run(lambda x, y: y.copy_(x + 1), {1: OUT}, x, out)
    assert torch.equal(flat_out[:, 2:5], x + 1) and float(flat_out[:, :2].abs().sum() + flat_out[:, 5:].abs().sum()) == 0.0

    def kernel(x, y):
        y.copy_(x + 1)
        flat(y)[12] = 5.0                       # the row after item 0's last: not an element of y
    with expect("gap-modified", 1, offset=12 * 4):
        run(kernel, {1: OUT}, x, out)


def test_an_output_that_depends_on_a_workspace_s_prior_contents():
    def good(x, y, ws):
        ws.zero_()
        ws += x
        y.copy_(ws)

    def bad(x, y, ws):
        ws += x                                 # accumulates without clearing
        y.copy_(ws)
    x = torch.arange(7.0)
    run(good, {1: OUT, 2: WORK}, x, torch.empty(7), torch.zeros(7))
    with expect("differs-between-fills", 1, offset=0):
        run(bad, {1: OUT, 2: WORK}, x, torch.empty(7), torch.zeros(7))


def test_a_wrong_role_row_fails_on_its_first_launch():
    x = torch.arange(7.0)
    with expect("input-modified", 1):           # y listed as an input
        run(scale, {}, x, torch.empty(7))
    with expect("differs-between-fills", 0):    # x listed as an output: the kernel reads what the harness pre-filled
        run(scale, {0: OUT, 1: OUT}, x, torch.empty(7))
    with pytest.raises(KeyError):
        run(scale, {5: OUT}, x, torch.empty(7))
    with pytest.raises(KeyError):
        with GuardedLaunches(real_launch=lambda *a, **k: None, roles={}):
            alo_hip._launch("unlisted", "cpu", None, 0.0, 0.0, x)


def test_the_same_tensor_passed_twice_lands_in_one_arena():
    seen = []

    def kernel(x, bias, y):                     # bias_act_: y is x
        seen.append((x.data_ptr(), y.data_ptr(), x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr()))
        y.copy_(torch.relu(x + bias))
    x = torch.tensor([-2.0, 1.0, 3.0])
    run(kernel, {2: OUT}, x, torch.ones(3), x)
    assert all(a == b and same for a, b, same in seen) and len(seen) == 2
    assert torch.equal(x, torch.tensor([0.0, 2.0, 4.0]))


def test_two_column_slices_of_one_buffer_land_in_one_arena():
    both = torch.arange(2 * 5 * 12.0).reshape(2, 5, 12)
    off, log = both[..., :8], both[..., 8:]
    gaps = []

    def kernel(off, log, y):
        gaps.append(log.data_ptr() - off.data_ptr())
        assert off.stride() == (60, 12, 1) and log.stride() == (60, 12, 1)
        y.copy_(off.sum(-1) + log.sum(-1))
    y = torch.empty(2, 5)
    run(kernel, {2: OUT}, off, log, y)
    assert gaps == [8 * 4, 8 * 4] and torch.equal(y, both.sum(-1))

    def spill(off, log, y):                     # a store into the sibling slice's columns
        kernel(off, log, y)
        flat(off)[8] = 0.0
    with expect("input-modified", 1, offset=0):
        run(spill, {2: OUT}, off, log, y)


def test_a_list_of_tensors_is_relocated():
    levels = [torch.empty(4), torch.empty(2)]
    originals = [t.data_ptr() for t in levels]
    seen = []

    def kernel(x, levels):
        seen.append([t.data_ptr() for t in levels])
        levels[0].copy_(x)
        levels[1].copy_(x[:2] + x[2:])
    x = torch.arange(4.0)
    run(kernel, {1: OUT}, x, levels)
    assert all(p not in originals for ptrs in seen for p in ptrs)
    assert torch.equal(levels[0], x) and torch.equal(levels[1], torch.tensor([2.0, 4.0]))

    def short(x, levels):
        kernel(x, levels)
        flat(levels[1])[2] = 9.0
    with expect("guard-after", 1, offset=2 * 4, item=1):
        run(short, {1: OUT}, x, levels)
    with pytest.raises(TypeError):
        run(kernel, {1: OUT}, x, [levels[0], 3])


@pytest.mark.parametrize("skew", [0, 16, 48, 100, 252])
def test_payload_alignment_modulo_256_is_preserved(skew):
    backing = torch.zeros(1024, dtype=torch.uint8)
    first = (-backing.data_ptr()) % 256 + skew
    x = backing[first:first + 64].view(torch.float32)
    y = torch.empty(16)
    seen = []

    def kernel(x, y):
        seen.append((x.data_ptr() % 256, y.data_ptr() % 256))
        y.copy_(x)
    run(kernel, {1: OUT}, x, y)
    assert seen == [(skew, y.data_ptr() % 256)] * 2


def test_inout_keeps_its_contents_and_nothing_else_is_prefilled():
    def kernel(h, net):                         # gru_update_: the first 2 of 3 channels in place, and a copy
        h[:, :2] += 1.0
        net.copy_(h[:, :2])
    h = torch.zeros(2, 3, 4)
    net = torch.empty(2, 2, 4)
    run(kernel, {0: INOUT, 1: OUT}, h, net)
    assert float(h[:, :2].sum()) == 16.0 and float(h[:, 2].abs().sum()) == 0.0 and torch.equal(net, h[:, :2])


def test_nondeterministic_outputs_are_compared_at_the_listed_tolerance(monkeypatch):
    assert list(guarded.NONDETERMINISTIC) == [("alo_msda_backward_hinted", 6)]
    monkeypatch.setitem(guarded.NONDETERMINISTIC, ("k", 1), {torch.float32: (1e-4, 2e-5)})
    calls = []

    def kernel(x, y, jitter):
        calls.append(1)
        y.copy_(x * (1.0 + jitter * len(calls)))
    x = torch.arange(1.0, 8.0)
    run(lambda x, y: kernel(x, y, 1e-6), {1: OUT}, x, torch.empty(7))
    with expect("differs-between-fills", 1):
        run(lambda x, y: kernel(x, y, 1e-2), {1: OUT}, x, torch.empty(7))
    with expect("differs-between-fills", 1, offset=6 * 4):    # unwritten stays a difference: NaN against a finite number
        run(lambda x, y: y[:6].copy_(x[:6]), {1: OUT}, x, torch.empty(7))


def test_ctypes_arguments_host_arrays_pass_and_pointers_are_refused():
    x, y = torch.arange(7.0), torch.empty(7)
    shapes = (ctypes.c_int32 * 2)(3, 4)
    got = []
    run(lambda x, y, s, n, none: (got.append(list(s)), scale(x, y)), {1: OUT}, x, y, shapes, 7, None)
    assert got == [[3, 4]] * 2
    for bad in ((ctypes.c_void_p * 1)(y.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.pointer(ctypes.c_int(1))):
        with pytest.raises(TypeError):
            run(lambda x, y, p: scale(x, y), {1: OUT}, x, y, bad)


def test_refuses_to_run_while_a_stream_is_capturing(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        run(scale, {1: OUT}, torch.arange(7.0), torch.empty(7))


def test_launch_takes_a_list_of_tensors_for_a_host_array_of_their_pointers(monkeypatch):
    """The product side of the seam: ``alo_hip._launch`` builds the pointer array inside the call."""
    got = {}

    class Lib:
        @staticmethod
        def fake(ptrs, n, stream):
            got["ptrs"], got["n"] = [int(p) for p in ptrs], n
            return 0

    class NoDevice:
        def __init__(self, device):
            pass

        def __enter__(self):
            pass

        def __exit__(self, *exc):
            pass

    monkeypatch.setattr(alo_hip, "lib", lambda: Lib)
    monkeypatch.setattr(alo_hip, "_stream", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", NoDevice)
    levels = [torch.zeros(3), torch.zeros(2)]
    alo_hip._launch("fake", "cpu", None, 0.0, 0.0, levels, 2)
    assert got == {"ptrs": [t.data_ptr() for t in levels], "n": 2}


# ---- census ---------------------------------------------------------------------------------------------------------------------
def test_the_role_table_lists_exactly_the_entry_points_alo_hip_launches():
    source = open(alo_hip.__file__).read()
    launched = set(re.findall(r'"(alo_[a-z0-9_]+)"', source.split("\ndef lib()", 1)[1]))   # symbol names past the signature table
    host_only = {n for n in alo_hip._SIGNATURES if n in guarded.HOST_ONLY or n.endswith("_workspace_bytes")}
    assert guarded.HOST_ONLY <= set(alo_hip._SIGNATURES)
    assert set(guarded.NEVER_LAUNCHED) == {"alo_msda_backward", "alo_msda_forward_fused_hm"} and all(guarded.NEVER_LAUNCHED.values())
    for name in guarded.NEVER_LAUNCHED:                # confirmed against the source: the name appears in the signature table only
        assert name not in launched and name in alo_hip._SIGNATURES
    assert set(guarded.ROLES) == set(alo_hip._SIGNATURES) - host_only - set(guarded.NEVER_LAUNCHED)
    assert set(guarded.ROLES) == launched & set(guarded.ROLES) and launched - set(alo_hip._SIGNATURES) == set()
    for symbol, roles in guarded.ROLES.items():
        n_args = len(alo_hip._SIGNATURES[symbol][1]) - 1          # the stream goes last
        assert roles and all(0 <= p < n_args and r in (OUT, INOUT, WORK) for p, r in roles.items()), symbol


def test_the_gpu_sweep_expects_every_entry_point_of_the_role_table():
    import test_buffer_discipline_gpu as sweep

    expected = set()
    for case in sweep.CASES:
        expected |= set(case.values[1])
    assert expected == set(guarded.ROLES), (sorted(set(guarded.ROLES) - expected), sorted(expected - set(guarded.ROLES)))
