"""Run every launch of ``alo_hip`` inside guarded buffers: does a kernel stay in its buffers, and does it ignore stale bytes?

``alo_hip._launch(symbol, device, tag, nbytes, flops, *args)`` is the one seam every device launch of the package goes through; a
tensor in ``args`` stands for its device pointer and a list of tensors for a host array of their pointers.  :class:`GuardedLaunches`
replaces that function for the length of a ``with`` block.  Each launch then runs TWICE, on copies of its buffers that sit between two
guard zones, once with guards / outputs / workspaces pre-filled with ``0xFF`` bytes (NaN in every float type, -1 as int32, 255 as
uint8) and once with ``0x3C`` (a small finite number in every float type):

  * a guard byte that changed                        -> ``guard-before`` / ``guard-after``   (a store outside the buffer)
  * a byte of an input that changed                  -> ``input-modified``
  * a byte between the elements of strided arguments -> ``gap-modified``                     (``y_batch_stride`` outputs, column slices)
  * an output that differs between the two fills     -> ``differs-between-fills``            (an element left unwritten, a result that
                                                                                             depends on a workspace's old contents, on
                                                                                             an output's, or on a guard: a read past the
                                                                                             end, even one multiplied by zero)

The first run's buffers are copied back over the originals, so the wrapper returns ordinary tensors and the caller's reference check
applies as usual.  Nothing here needs a GPU: with ``real_launch`` a Python function acting on CPU tensors stands in for the kernel
(tests/test_guarded_cpu.py plants the defects there; none is ever planted in a HIP kernel).
"""
import ctypes

import torch

IN, OUT, INOUT, WORK = "in", "out", "inout", "work"
FILLS = (0xFF, 0x3C)
KINDS = ("guard-before", "guard-after", "input-modified", "gap-modified", "differs-between-fills")
DEFAULT_GUARD_BYTES = 64 * 2048 * 2   # one full tile of the widest kernel in the sweep: 64 rows x 2048 columns x 2 bytes

# {symbol: {position in _launch's *args: OUT | INOUT | WORK}}, read off the headers under include/ and the wrapper's _launch line.
# A tensor (or list of tensors) at a position that is not listed is IN.  OUT: fully overwritten, never read.  INOUT: read and / or
# partly written in place.  WORK: scratch whose contents after the call are unspecified.  A wrong row fails on its first launch.
ROLES = {
    # include/alo_hotpath.h
    "alo_msda_forward": {5: OUT},
    "alo_msda_forward_fused": {6: OUT},
    "alo_msda_forward_fused_hm_rows": {8: OUT},
    "alo_msda_forward_fused_hm_resident": {8: OUT},
    "alo_msda_backward_hinted": {6: OUT, 7: OUT, 8: OUT},           # grad_value is "zeroed by this call": an output like the others
    "alo_corr_build": {2: OUT, 3: WORK},                            # 2: the list of levels
    "alo_corr_lookup": {2: OUT},
    "alo_corr_lookup_backward": {0: INOUT},                         # the list of gradient maps: read-modify-write
    "alo_corr_lookup_backward_coords": {3: OUT},
    "alo_value_head_major": {2: OUT},
    "alo_value_proj_head_major": {4: OUT},
    "alo_bias_act_nchw": {2: OUT},                                  # y aliases x in the wrapper: the bytes it shares with an input keep theirs
    "alo_gru_gate": {0: INOUT, 3: INOUT},                           # zr: z in place, r read; rhx: the first C of C + Cx channels written
    "alo_gru_update": {3: INOUT, 4: OUT},                           # hx: the first C channels in place; net
    "alo_pack_mfma_b": {1: OUT},
    "alo_linear_shortk": {4: OUT},
    "alo_linear_packed": {4: OUT},
    "alo_ffn256": {5: OUT},
    "alo_conv1x1_nhwc": {5: OUT},
    "alo_conv3x3_nhwc": {3: OUT, 4: WORK},
    "alo_conv3x3_small_nhwc": {3: OUT},
    "alo_stem_conv_pool": {3: OUT},
    "alo_groupnorm_rows": {3: OUT, 4: WORK},
    "alo_groupnorm_rows_act": {3: OUT, 4: WORK},
    "alo_upsample_add_nhwc": {2: OUT},
    "alo_mask_pyramid": {2: OUT, 3: OUT},
    "alo_encoder_reference_points": {1: OUT},
    "alo_panoptic_onehot": {1: OUT},
    "alo_pos_sine_flat": {5: OUT, 6: WORK},
    "alo_add_layernorm": {4: OUT, 6: OUT},
    "alo_bias_act": {3: OUT},                                       # y aliases x in the wrapper, as above
    # include/alo_corr_alt.h
    "alo_corr_alt_prepare": {2: WORK},                              # the lookup's workspace: its pad bytes may stay unwritten
    "alo_corr_alt_lookup": {3: OUT},
    # include/alo_two_stage.h
    "alo_encoder_proposals": {1: OUT, 2: OUT},
    "alo_encoder_proposals_masked": {1: OUT, 2: OUT, 4: OUT},
    "alo_mask_rows": {2: OUT},
    "alo_proposal_queries": {3: OUT, 4: OUT},
    # include/alo_encoder_block.h: 5 tail operands, 8 FFN operands (the last is out), 8 projection operands (the last two are outputs)
    "alo_encoder_block": {12: OUT, 19: OUT, 20: OUT},
}

# Entries of alo_hip._SIGNATURES that enqueue nothing: queries answered on the host.
HOST_ONLY = {"alo_abi_version", "alo_last_error", "alo_corr_level_shape", "alo_msda_resident_levels", "alo_msda_backward_path",
             "alo_msda_generic_plan"}
# Entry points the header documents as another entry point with fixed arguments, and that alo_hip never calls: {name: reason}.
NEVER_LAUNCHED = {
    "alo_msda_backward": "include/alo_hotpath.h: 'alo_msda_backward is this call [alo_msda_backward_hinted] with a NULL hint'; "
                         "alo_hip.msda_backward always launches the hinted entry point",
    "alo_msda_forward_fused_hm": "include/alo_hotpath.h: alo_msda_forward_fused_hm_rows is 'the same' with row strides; "
                                 "alo_hip.msda_forward_fused_hm always launches the _rows or the _resident entry point",
}

# {(symbol, position): {dtype of the buffer: (rtol, atol)}} — outputs whose bits depend on the schedule, compared at a tolerance
# instead of bit for bit.  One entry: grad_value of the MSDA backward is accumulated with floating-point atomics ("its low-order bits
# depend on scheduling", include/alo_hotpath.h).  The figures are what tests/test_msda_gpu.py::test_forward_backward_vs_oracle allows
# grad_value against the float64 oracle (an fp32 buffer also serves bf16 / fp16 values; an fp64 buffer fp64 values).
NONDETERMINISTIC = {
    ("alo_msda_backward_hinted", 6): {torch.float32: (1e-4, 2e-5), torch.float64: (1e-11, 1e-11)},
}


class BufferDisciplineError(AssertionError):
    """A launch wrote outside what it owns, or its result depends on bytes it does not own."""

    def __init__(self, symbol, position, kind, offset, item=None):
        assert kind in KINDS
        self.symbol, self.position, self.kind, self.offset, self.item = symbol, position, kind, offset, item
        where = f"argument {position}" + ("" if item is None else f"[{item}]")
        super().__init__(f"{symbol}: {kind} at {where}, first offending byte {offset:+d} from that argument's pointer")


def _is_host_data(a):
    """ctypes arrays of plain numbers are host data by construction (level_shapes_host, the resident kernel's host shapes)."""
    return isinstance(a, ctypes.Array) and isinstance(getattr(a._type_, "_type_", None), str) and a._type_._type_ in "bBhHiIlLqQfd"


def _is_ctypes(a):
    return isinstance(a, (ctypes.Array, ctypes._Pointer, ctypes._SimpleCData, ctypes.Structure, ctypes.Union, ctypes._CFuncPtr))


def _span_bytes(t):
    """Bytes from ``t.data_ptr()`` to the end of the last element ``t`` addresses."""
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _u8(storage, offset, nbytes, device):
    return torch.empty(0, dtype=torch.uint8, device=device).set_(storage, offset, (nbytes,), (1,))


def _element_bytes(buf, t, rel):
    """The bytes of ``buf`` (1-D, one entry per byte of a hull) that the elements of ``t``, ``rel`` bytes into the hull, occupy."""
    e = t.element_size()
    return buf.as_strided((*t.shape, e), (*[s * e for s in t.stride()], 1), buf.storage_offset() + rel)


def _first(mask):
    return int(torch.nonzero(mask)[0])


class _Arg:
    __slots__ = ("pos", "item", "t", "role", "group", "rel", "span")

    def __init__(self, pos, item, t, role):
        self.pos, self.item, self.t, self.role = pos, item, t, role


class _Group:
    """The tensor arguments of one launch that share an untyped storage, and the hull of their byte spans."""

    def __init__(self, args):
        self.args = args
        t0 = args[0].t
        self.device = t0.device
        self.lo = min(a.t.data_ptr() for a in args)
        for a in args:
            a.group, a.rel, a.span = self, a.t.data_ptr() - self.lo, _span_bytes(a.t)
        self.nbytes = max(a.rel + a.span for a in args)
        storage = t0.untyped_storage()
        self.original = _u8(storage, self.lo - storage.data_ptr(), self.nbytes, self.device)
        self.cover = {role: self._cover(role) for role in (IN, OUT, INOUT, WORK)}
        self.read = self.cover[IN] | self.cover[INOUT]
        self.written = self.cover[OUT] | self.cover[INOUT] | self.cover[WORK]
        self.prefill = (self.cover[OUT] | self.cover[WORK]) & ~self.read   # bytes an input shares with an output keep the input
        self.payloads = []

    def _cover(self, role):
        mask = torch.zeros(self.nbytes, dtype=torch.bool, device=self.device)
        for a in self.args:
            if a.role == role:
                _element_bytes(mask, a.t, a.rel).fill_(True)
        return mask

    def relocate(self, fill, guard):
        """A fresh arena ``guard | hull | guard`` of ``fill`` bytes whose payload has the original's address modulo 256."""
        arena = torch.full((2 * guard + self.nbytes + 256,), fill, dtype=torch.uint8, device=self.device)
        start = guard + (self.lo - arena.data_ptr() - guard) % 256
        payload = arena[start:start + self.nbytes]
        payload.copy_(self.original)
        payload.masked_fill_(self.prefill, fill)
        self.arena, self.start, self.fill, self.payload, self.before = arena, start, fill, payload, payload.clone()
        self.payloads.append(payload)
        assert payload.data_ptr() % 256 == self.lo % 256

    def view(self, a):
        e = a.t.element_size()
        assert (self.start + a.rel) % e == 0, "a tensor argument is not aligned to its element size"
        return torch.empty(0, dtype=a.t.dtype, device=self.device).set_(self.arena.untyped_storage(), (self.start + a.rel) // e,
                                                                        a.t.shape, a.t.stride())

    def _owner(self, offset, roles=None):
        """The argument a hull byte is charged to: one that covers it, else the last one that starts at or before it."""
        for a in self.args:
            if (roles is None or a.role in roles) and a.rel <= offset < a.rel + a.span:
                probe = torch.zeros(self.nbytes, dtype=torch.bool, device=self.device)
                _element_bytes(probe, a.t, a.rel).fill_(True)
                if bool(probe[offset]):
                    return a
        return max((a for a in self.args if a.rel <= offset), key=lambda a: a.rel)

    def check_run(self, symbol):
        head, tail = self.arena[:self.start], self.arena[self.start + self.nbytes:]
        if not bool((head == self.fill).all()):
            a = min(self.args, key=lambda a: a.rel)
            raise BufferDisciplineError(symbol, a.pos, "guard-before", _first(head != self.fill) - self.start - a.rel, a.item)
        if not bool((tail == self.fill).all()):
            a = max(self.args, key=lambda a: a.rel + a.span)
            raise BufferDisciplineError(symbol, a.pos, "guard-after", self.nbytes + _first(tail != self.fill) - a.rel, a.item)
        changed = (self.payload != self.before) & ~self.written
        if bool(changed.any()):
            gap = changed & ~self.read
            if bool(gap.any()):
                offset = _first(gap)
                a = self._owner(offset)
                raise BufferDisciplineError(symbol, a.pos, "gap-modified", offset - a.rel, a.item)
            offset = _first(changed)
            a = self._owner(offset, (IN,))
            raise BufferDisciplineError(symbol, a.pos, "input-modified", offset - a.rel, a.item)

    def check_across(self, symbol):
        first, second = self.payloads
        exact = torch.zeros(self.nbytes, dtype=torch.bool, device=self.device)
        for a in self.args:
            if a.role not in (OUT, INOUT):
                continue
            tol = NONDETERMINISTIC.get((symbol, a.pos))
            if tol is None:
                _element_bytes(exact, a.t, a.rel).fill_(True)
                continue
            rtol, atol = tol[a.t.dtype]
            x, y = (torch.empty(0, dtype=a.t.dtype, device=self.device).set_(p.untyped_storage(), (p.storage_offset() + a.rel) // a.t.element_size(),
                                                                              a.t.shape, a.t.stride()) for p in (first, second))
            bad = ~((x - y).abs() <= atol + rtol * y.abs())   # a NaN on either side is a difference
            if bool(bad.any()):
                flat = _first(bad.reshape(-1))
                offset = 0
                for n, s in zip(reversed(a.t.shape), reversed(a.t.stride())):
                    flat, i = divmod(flat, n)
                    offset += i * s * a.t.element_size()
                raise BufferDisciplineError(symbol, a.pos, "differs-between-fills", offset, a.item)
        differs = (first != second) & exact
        if bool(differs.any()):
            offset = _first(differs)
            a = self._owner(offset, (OUT, INOUT))
            raise BufferDisciplineError(symbol, a.pos, "differs-between-fills", offset - a.rel, a.item)


class GuardedLaunches:
    """``with GuardedLaunches() as g: alo_hip.linear_shortk(...)``: every launch inside the block runs under the checks of this
    module (see the top of the file) and is logged as ``(symbol, tag)`` in ``g.seen``.  ``real_launch``: what performs a launch,
    ``alo_hip._launch`` as found on entry by default.  ``guard_bytes``: a multiple of 256."""

    def __init__(self, real_launch=None, guard_bytes=DEFAULT_GUARD_BYTES, roles=None):
        if guard_bytes <= 0 or guard_bytes % 256:
            raise ValueError("guard_bytes must be a positive multiple of 256")
        self.real_launch, self.guard_bytes, self.roles = real_launch, guard_bytes, ROLES if roles is None else roles
        self.seen = []

    def __enter__(self):
        import alo_hip

        self._module, self._saved = alo_hip, alo_hip._launch
        if self.real_launch is None:
            self.real_launch = self._saved
        alo_hip._launch = self._launch
        return self

    def __exit__(self, *exc):
        self._module._launch = self._saved

    def _launch(self, symbol, device, tag, nbytes, flops, *args, relaunch=False):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"GuardedLaunches: {symbol} was launched while a stream is capturing; the harness synchronises and "
                               f"cannot run inside a graph capture")
        if symbol not in self.roles:
            raise KeyError(f"GuardedLaunches: no row for {symbol} in the role table")
        roles = self.roles[symbol]
        found = []
        for pos, a in enumerate(args):
            if isinstance(a, torch.Tensor):
                found.append(_Arg(pos, None, a, roles.get(pos, IN)))
            elif isinstance(a, list):
                if not all(isinstance(t, torch.Tensor) for t in a):
                    raise TypeError(f"GuardedLaunches: {symbol} argument {pos} is a list that holds something else than tensors")
                found += [_Arg(pos, i, t, roles.get(pos, IN)) for i, t in enumerate(a)]
            elif _is_ctypes(a) and not _is_host_data(a):
                raise TypeError(f"GuardedLaunches: {symbol} argument {pos} is a {type(a).__name__}: a device pointer must reach "
                                f"_launch as a tensor or a list of tensors, and only arrays of plain numbers count as host data")
        stray = set(roles) - {a.pos for a in found} - {pos for pos, a in enumerate(args) if a is None}
        if stray:
            raise KeyError(f"GuardedLaunches: the role table of {symbol} names positions {sorted(stray)}, which hold no tensor")
        live = [a for a in found if a.t.numel()]
        by_storage = {}
        for a in live:
            by_storage.setdefault((a.t.device, a.t.untyped_storage().data_ptr()), []).append(a)
        groups = [_Group(members) for members in by_storage.values()]
        on_gpu = [g.device for g in groups if g.device.type == "cuda"]

        for run, fill in enumerate(FILLS):
            for g in groups:
                g.relocate(fill, self.guard_bytes)
            views = {id(a): a.group.view(a) for a in live}
            moved = []
            for pos, a in enumerate(args):
                if isinstance(a, torch.Tensor):
                    moved.append(next((views[id(r)] for r in live if r.pos == pos), a))
                elif isinstance(a, list):
                    at = {r.item: views[id(r)] for r in live if r.pos == pos}
                    moved.append([at.get(i, t) for i, t in enumerate(a)])
                else:
                    moved.append(a)
            # the timer sees one record per launch: the second run goes untimed
            self.real_launch(symbol, device, tag if run == 0 else None, nbytes, flops, *moved, relaunch=relaunch and run == 0)
            for d in set(on_gpu):
                torch.cuda.synchronize(d)
            for g in groups:
                g.check_run(symbol)
        for g in groups:
            g.check_across(symbol)
        for g in groups:
            g.original.copy_(g.payloads[0])
        self.seen.append((symbol, tag))
