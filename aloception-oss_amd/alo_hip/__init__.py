"""ctypes binding of ``libalo_hotpath.so``: one library, one ABI number, declared by the four headers under ``include/``
(``alo_hotpath.h``, ``alo_corr_alt.h``, ``alo_two_stage.h``, ``alo_encoder_block.h``).

This is the only place the host code touches the native library.  PyTorch is used for what it is good at here —
device memory, streams, dtypes — and nothing else: every function below takes torch tensors, validates them the way
the reference op validates its ``at::Tensor`` arguments (alonet/deformable_detr/ops/src/cuda/ms_deform_attn_cuda.cu:28-52),
allocates the outputs (so torch owns the memory, as with the reference op) and enqueues the HIP kernels on the
current torch stream.

There is NO fallback: if the library is missing or a tensor lives on the CPU these functions raise ``RuntimeError``.
"""
import ctypes
import warnings
import os
import subprocess

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG_ROOT, "libalo_hotpath.so")
CSRC_DIR = os.path.join(_PKG_ROOT, "csrc")

ALO_F32, ALO_F64, ALO_BF16, ALO_F16 = 0, 1, 2, 3
RESIDENT_AUTO, RESIDENT_ALWAYS = 0, 1   # ALO_RESIDENT_* of include/alo_hotpath.h
# fp16 is served by the MSDA entry points and the transformer's layer kernels (linear_shortk, linear_packed, ffn256,
# value_proj_head_major, add_layernorm, bias_act, pos_sine_flat, pack_mfma_b, the two-stage glue); the backbone / projection kernels
# (conv*, stem, groupnorm, conv1x1_strided, upsample_add) and encoder_block are bf16 only (attention, on encoder_block's entry point,
# takes bf16 / fp16 / fp32; conv3x3_f32, stem_conv_pool_f32, linear_f32
# and conv1x1_strided_f32 are the fp32 flavours of four of them, each behind a gate of its own; upsample_flow rides upsample_add's
# entry point with ALO_F32).  fp16 is opt-in per call site: `fusable`
# and the `*_supported` gates answer for fp32 / bf16 unless asked with ``f16=True``, which only the callers whose whole route has
# fp16 kernels do (the transformer's layers), so an fp16 tensor never reaches a kernel that lacks it
_DTYPE_CODE = {torch.float32: ALO_F32, torch.float64: ALO_F64, torch.bfloat16: ALO_BF16, torch.float16: ALO_F16}


def _half(f16):
    """The 16-bit storage types a gate of the MFMA layer kernels lets through."""
    return (torch.bfloat16, torch.float16) if f16 else (torch.bfloat16,)


_lib = None
_warned_inference_tensor = False


def tensor_version(t):
    """``t._version`` for the ``(version, data_ptr)`` cache keys of this package.  Inference tensors (``torch.inference_mode()``)
    carry no version counter and raise when asked for one (round-3 advisor finding), yet can still be updated in place inside
    inference mode with their ``data_ptr`` unchanged — so for them the key is a fresh object that equals nothing, itself of an
    earlier call included: whatever is derived from an inference tensor is re-derived on every use instead of being cached
    (round-4 advisor finding: a constant there made stale packed weights / host shapes possible)."""
    if t.is_inference():
        global _warned_inference_tensor
        if not _warned_inference_tensor:
            _warned_inference_tensor = True
            warnings.warn("alo_hip: a parameter / shape tensor created under torch.inference_mode() carries no version counter, so what is "
                          "derived from it (packed MFMA weights, folded convolutions, the host copy of spatial_shapes) is re-derived on "
                          "every call instead of being cached — results are right, the forward is slower.  Build / load the model outside "
                          "inference_mode() (torch.no_grad() is enough for inference).", RuntimeWarning, stacklevel=3)
        return object()
    return t._version


_DERIVED = "_alo_derived"      # owner.__dict__[_DERIVED] = {name: (key, payload)}: every derived tensor of this package lives there
_EPOCH = "_alo_cache_epoch"    # model.__dict__[_EPOCH]: how often invalidate_caches ran on it


def derived(owner, name, sources, build, no_grad=True):
    """What ``build()`` makes (a tensor or a tuple of them) from the tensors in ``sources`` (``None`` stands for an absent bias),
    cached on ``owner`` (an ``nn.Module`` or a tensor) under ``name`` until a source changes: its version counter (in-place
    updates), its pointer (``p.data = other``), its dtype or its device (``module.to(...)``).  A pack rides on the tensor
    it was packed from and dies with it; a derived tensor may own derived tensors in turn.  ``build`` runs under
    ``torch.no_grad()`` unless ``no_grad=False`` (then in the caller's grad mode).  An owner without a ``__dict__`` gets no
    caching.  Writes through ``.data`` bump no version counter: :func:`invalidate_caches` is for those."""
    entries = owner.__dict__.setdefault(_DERIVED, {}) if hasattr(owner, "__dict__") else {}
    key = tuple([None if t is None else (tensor_version(t), t.data_ptr(), t.dtype, t.device) for t in sources])
    hit = entries.get(name)
    if hit is None or hit[0] != key:
        with torch.set_grad_enabled(torch.is_grad_enabled() and not no_grad):
            hit = entries[name] = (key, build())
    return hit[1]


class HotpathUnavailable(RuntimeError):
    """libalo_hotpath.so cannot be loaded (not built, or built for another ABI)."""


def build(force=False):
    """Compile the HIP kernels for gfx950 with hipcc (``make -C aloception-oss_amd/csrc``). Needs no GPU."""
    cmd = ["make", "-C", CSRC_DIR, "-j4"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


_vp, _ip, _i32p, _long, _f32, _size = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_long, ctypes.c_float, ctypes.c_size_t
_vpp, _ipp = ctypes.POINTER(_vp), ctypes.POINTER(_ip)
# name -> (restype, argtypes) of every function the four headers declare; an entry point that enqueues work ends in the stream
_SIGNATURES = {
    # include/alo_hotpath.h
    "alo_abi_version": (_ip, []),
    "alo_last_error": (ctypes.c_char_p, []),
    "alo_msda_forward": (_ip, [_vp] * 6 + [_ip] * 9 + [_vp]),
    "alo_msda_forward_fused": (_ip, [_vp] * 7 + [_ip] * 9 + [_vp]),
    "alo_msda_forward_fused_hm": (_ip, [_vp] * 7 + [_ip] * 9 + [_vp]),
    "alo_msda_forward_fused_hm_rows": (_ip, [_vp] * 5 + [_long, _long, _vp, _vp] + [_ip] * 9 + [_vp]),
    "alo_msda_forward_fused_hm_resident": (_ip, [_vp] * 5 + [_long, _long, _vp, _vp] + [_ip] * 9 + [_i32p, _ip, _vp]),
    "alo_msda_resident_levels": (_ip, [_i32p] + [_ip] * 6),
    "alo_msda_backward": (_ip, [_vp] * 9 + [_ip] * 9 + [_vp]),
    "alo_msda_backward_hinted": (_ip, [_vp] * 9 + [_ip] * 9 + [_i32p, _vp]),
    "alo_msda_backward_path": (_ip, [_ip] * 9 + [_i32p]),
    "alo_msda_generic_plan": (_ip, [_ip] * 9 + [_i32p] + [_ip] * 4 + [_ipp]),
    "alo_corr_level_shape": (None, [_ip, _ip, _ip, _ipp, _ipp]),
    "alo_corr_build_workspace_bytes": (_size, [_ip] * 5),
    "alo_corr_build": (_ip, [_vp, _vp, _vpp, _vp, _size] + [_ip] * 5 + [_vp]),
    "alo_corr_lookup": (_ip, [_vpp, _vp, _vp] + [_ip] * 5 + [_vp]),
    "alo_corr_lookup_backward": (_ip, [_vpp, _vp, _vp] + [_ip] * 5 + [_vp]),
    "alo_corr_lookup_backward_coords": (_ip, [_vpp, _vp, _vp, _vp] + [_ip] * 5 + [_vp]),
    "alo_value_head_major": (_ip, [_vp] * 3 + [_ip] * 5 + [_vp]),
    "alo_value_proj_head_major": (_ip, [_vp] * 5 + [_ip] * 5 + [_vp]),
    "alo_bias_act_nchw": (_ip, [_vp] * 3 + [_ip] * 4 + [_vp]),
    "alo_gru_gate": (_ip, [_vp] * 4 + [_ip] * 3 + [_long, _long, _vp]),
    "alo_gru_update": (_ip, [_vp] * 5 + [_ip] * 3 + [_long, _vp]),
    "alo_pack_mfma_b": (_ip, [_vp, _vp, _ip, _ip, _ip, _vp]),
    "alo_linear_shortk": (_ip, [_vp] * 5 + [_long, _ip, _ip, _ip, _ip, _vp]),
    "alo_linear_packed": (_ip, [_vp] * 5 + [_long, _ip, _ip, _ip, _ip, _vp]),
    "alo_ffn256": (_ip, [_vp] * 6 + [_long, _ip, _ip, _vp]),
    "alo_conv1x1_nhwc": (_ip, [_vp, _vp, _ip, _vp, _vp, _vp] + [_ip] * 8 + [_vp]),
    "alo_conv3x3_workspace_bytes": (_size, [_ip] * 6),
    "alo_conv3x3_nhwc": (_ip, [_vp] * 5 + [_ip] * 8 + [_vp]),
    "alo_conv3x3_small_nhwc": (_ip, [_vp] * 4 + [_ip] * 6 + [_vp]),
    "alo_stem_conv_pool": (_ip, [_vp] * 4 + [_ip] * 3 + [_long] * 4 + [_ip, _vp]),
    "alo_groupnorm_rows_workspace_bytes": (_size, [_ip, _ip, _ip]),
    "alo_groupnorm_rows": (_ip, [_vp] * 5 + [_ip] * 4 + [_f32, _long, _ip, _vp]),
    "alo_groupnorm_rows_act": (_ip, [_vp] * 5 + [_ip] * 4 + [_f32, _long, _ip, _ip, _vp]),
    "alo_upsample_add_nhwc": (_ip, [_vp] * 3 + [_ip] * 8 + [_vp]),
    "alo_mask_pyramid": (_ip, [_vp, _ip, _vp, _vp, _ip, _ip, _ip, _ip, _ipp, ctypes.c_uint, _vp]),
    "alo_encoder_reference_points": (_ip, [_vp, _vp, _ip, _ip, _ipp, _vp]),
    "alo_panoptic_onehot": (_ip, [_vp, _vp] + [_ip] * 6 + [_f32, _vp]),
    "alo_pos_sine_flat": (_ip, [_vp] * 7 + [_ip] * 6 + [_f32, _f32, _ip, _vp]),
    "alo_add_layernorm": (_ip, [_vp] * 7 + [_long, _ip, _f32, _ip, _vp]),
    "alo_bias_act": (_ip, [_vp] * 4 + [_long, _ip, _ip, _ip, _vp]),
    # include/alo_corr_alt.h
    "alo_corr_alt_workspace_bytes": (_size, [_ip] * 5),
    "alo_corr_alt_prepare": (_ip, [_vp, _vpp, _vp, _size] + [_ip] * 5 + [_vp]),
    "alo_corr_alt_lookup": (_ip, [_vp, _size, _vp, _vp] + [_ip] * 6 + [_vp]),
    # include/alo_two_stage.h
    "alo_encoder_proposals": (_ip, [_vp, _vp, _vp, _ip, _ip, _ipp, _vp]),
    "alo_encoder_proposals_masked": (_ip, [_vp, _vp, _vp, _vp, _vp, _ip, _ip, _ipp, _ip, _ip, _vp]),
    "alo_mask_rows": (_ip, [_vp, _vp, _vp, _long, _ip, _ip, _vp]),
    "alo_proposal_queries": (_ip, [_vp, _vp, _vp, _vp, _vp, _ip, _ip, _ip, _ip, _vp]),
    # include/alo_encoder_block.h
    "alo_encoder_block": (_ip, [_vp] * 21 + [_ip] * 3 + [_f32] * 2 + [_ip, _vp]),
}


def lib():
    """The loaded library; raises :class:`HotpathUnavailable` (never falls back) when it cannot be loaded, lacks an entry of
    ``_SIGNATURES`` (built from an older tree) or has another ABI number."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HotpathUnavailable(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C {CSRC_DIR}` (hipcc, --offload-arch=gfx950). There is no CPU fallback for this path."
            )
        try:
            handle = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the box
            raise HotpathUnavailable(f"cannot load {LIB_PATH}: {e}") from e
        for name, (restype, argtypes) in _SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:
                raise HotpathUnavailable(f"{LIB_PATH} does not export {name}: it was built from an older tree; "
                                         f"rebuild it with `make -C {CSRC_DIR}`") from None
            fn.restype, fn.argtypes = restype, argtypes
        if handle.alo_abi_version() != 3:
            raise HotpathUnavailable(f"{LIB_PATH} has ABI version {handle.alo_abi_version()}, expected 3")
        _lib = handle
    return _lib


def is_available():
    try:
        lib()
        return True
    except HotpathUnavailable:
        return False


def _check(rc):
    if rc != 0:
        raise RuntimeError(lib().alo_last_error().decode() or f"alo_hotpath error {rc}")


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _require_cuda_contiguous(named):
    # same order and wording as the reference's AT_ASSERTM list (ms_deform_attn_cuda.cu:28-38,91-105)
    for name, t in named:
        if not t.is_contiguous():
            raise RuntimeError(f"{name} tensor has to be contiguous")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")


class LaunchTimer:
    """Times every kernel launch made through this module with HIP events recorded on the launch stream.

    ``with alo_hip.LaunchTimer() as t: ...``; afterwards ``t.summary()`` maps a kernel tag (e.g. ``"msda_fwd/Lq=22223"``)
    to ``dict(calls, ms_total, ms_avg, alg_bytes_avg, alg_flops_avg)``.  Used by bench.py for the roofline numbers:
    the algorithmic byte / flop counts are the SURVEY.md section 8(d) formulas evaluated on the actual launch shape.
    """

    def __init__(self, only=None):
        self.records = []
        self.relaunch = {}  # tag -> closure that enqueues the tag's most recent launch again (same buffers)
        self.only = only    # tag prefix: time just these launches (an event pair per launch is not free on the GPU either)

    def __enter__(self):
        global _timer
        self._prev, _timer = _timer, self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = self._prev

    def replay_ms(self, tag, reps=20):
        """Average duration of ``reps`` back-to-back re-launches of the last launch recorded under ``tag`` (same device
        buffers).  An event pair around ONE launch also measures the dispatch gap either side of it (tens of microseconds
        on ROCm); a back-to-back train does not, and agrees with rocprofv3's per-kernel average."""
        fn = self.relaunch[tag]
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / reps

    def replay_samples(self, tag, reps=7):
        """Durations (ms) of ``reps`` re-launches of the last launch recorded under ``tag``, each one timed by its own event
        pair with the next already queued behind it (so a sample is the kernel sequence itself, not the dispatch gap): for
        launches that happen once per step (the correlation build) a median and a minimum instead of a single reading."""
        fn = self.relaunch[tag]
        fn()
        torch.cuda.synchronize()
        events = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        events[0].record()
        for i in range(reps):
            fn()
            events[i + 1].record()
        torch.cuda.synchronize()
        return [events[i].elapsed_time(events[i + 1]) for i in range(reps)]

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, start, stop, nbytes, flops in self.records:
            d = out.setdefault(tag, dict(calls=0, ms_total=0.0, alg_bytes_avg=0.0, alg_flops_avg=0.0))
            d["calls"] += 1
            d["ms_total"] += start.elapsed_time(stop)
            d["alg_bytes_avg"] += nbytes
            d["alg_flops_avg"] += flops
        for d in out.values():
            d["ms_avg"] = d["ms_total"] / d["calls"]
            d["alg_bytes_avg"] /= d["calls"]
            d["alg_flops_avg"] /= d["calls"]
        return out


_timer = None


class _timed:
    def __init__(self, tag, nbytes=0.0, flops=0.0, relaunch=None):
        self.tag, self.nbytes, self.flops, self.relaunch = tag, nbytes, flops, relaunch

    def __enter__(self):
        self.on = _timer is not None and self.tag is not None and (_timer.only is None or self.tag.startswith(_timer.only))
        if self.on:
            self.start = torch.cuda.Event(enable_timing=True)
            self.stop = torch.cuda.Event(enable_timing=True)
            self.start.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.stop.record()
            _timer.records.append((self.tag, self.start, self.stop, self.nbytes, self.flops))
            if self.relaunch is not None:
                _timer.relaunch[self.tag] = self.relaunch


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _launch(symbol, device, tag, nbytes, flops, *args, relaunch=False):
    """Enqueue entry point ``symbol`` on ``device``'s current torch stream: what ``alo::launch`` is to csrc.  A tensor in ``args``
    stands for its device pointer (it is alive for the call), a list of tensors for a host array of their device pointers (built for
    the call), ``None`` for a null pointer, everything else is passed as it is (ctypes arrays are host data); the stream goes last.
    The call is timed under ``tag`` (``None``: untimed) with its algorithmic ``nbytes`` / ``flops``; with
    ``relaunch`` a running :class:`LaunchTimer` also gets a closure that repeats the call and keeps ``args`` alive for that."""
    fn = getattr(lib(), symbol)

    def call():
        _check(fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else _pointers(a) if isinstance(a, list) else a for a in args],
                  _stream(device)))

    with torch.cuda.device(device), _timed(tag, nbytes, flops, relaunch=call if relaunch and _timer else None):
        call()


def msda_forward_bytes(N, S, M, D, L, Lq, P, elem, loc_elem=4):
    """Algorithmic HBM bytes of one forward launch: value once + out once + (loc, attn) once."""
    return elem * (N * S * M * D + N * Lq * M * D) + loc_elem * (N * Lq * M * L * P * 3)


def msda_backward_bytes(N, S, M, D, L, Lq, P, elem, loc_elem=4):
    return elem * (2 * N * S * M * D + N * Lq * M * D) + loc_elem * (N * Lq * M * L * P * 3 * 2)


def _msda_prepare(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, extra=()):
    if not value.is_cuda:
        raise RuntimeError("Not implemented on the CPU")  # ms_deform_attn.h:38,60
    _require_cuda_contiguous(
        [("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
         ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)] + list(extra)
    )
    if value.dim() != 4 or sampling_loc.dim() != 6 or attn_weight.dim() != 5:
        raise RuntimeError("value must be (N,S,M,D), sampling_loc (N,Lq,M,L,P,2), attn_weight (N,Lq,M,L,P)")
    if spatial_shapes.dtype != torch.int32 or level_start_index.dtype != torch.int32:
        # this fork of the op reads int32 metadata (ms_deform_attn_cuda.cu:67-68)
        raise RuntimeError("spatial_shapes and level_start_index must be int32 tensors")
    N, S, M, D = value.shape
    _, Lq, M2, L, P, two = sampling_loc.shape
    if (M2, two) != (M, 2) or tuple(attn_weight.shape) != (N, Lq, M, L, P) or sampling_loc.shape[0] != N:
        raise RuntimeError("sampling_loc / attn_weight shapes do not match value")
    if tuple(spatial_shapes.shape) != (L, 2) or tuple(level_start_index.shape) != (L,):
        raise RuntimeError("spatial_shapes must be (L,2) and level_start_index (L,)")
    step = min(N, int(im2col_step))
    if step <= 0 or N % step != 0:
        raise RuntimeError(f"batch({N}) must divide im2col_step({step})")
    vdt = _DTYPE_CODE.get(value.dtype)
    if vdt is None:
        raise RuntimeError(f"ms_deform_attn: unsupported value dtype {value.dtype}")
    if value.dtype in (torch.bfloat16, torch.float16):
        # 16-bit storage: sampling geometry stays fp32 (bf16 locations would cost ~0.3 px at 167-wide maps, fp16 ones 0.08 px)
        sampling_loc, attn_weight = sampling_loc.float(), attn_weight.float()
    elif sampling_loc.dtype != value.dtype or attn_weight.dtype != value.dtype:
        raise RuntimeError("sampling_loc and attn_weight must have the dtype of value")
    ldt = _DTYPE_CODE[sampling_loc.dtype]
    return (N, S, M, D, L, Lq, P), vdt, ldt, sampling_loc.contiguous(), attn_weight.contiguous()


def msda_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=64):
    """-> (N, Lq, M*D) tensor of ``value``'s dtype.  Replaces ``alonet_custom::ms_deform_attn_forward``."""
    dims, vdt, ldt, loc, attn = _msda_prepare(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)
    N, S, M, D, L, Lq, P = dims
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    nbytes = msda_forward_bytes(N, S, M, D, L, Lq, P, value.element_size(), loc.element_size())
    _launch("alo_msda_forward", value.device, f"msda_fwd/Lq={Lq}", nbytes, 0.0, value, spatial_shapes, level_start_index, loc, attn,
            out, N, S, M, D, L, Lq, P, vdt, ldt)
    return out


def _check_fused_operands(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points, dims):
    """Dtype and shape checks the two fused forwards share -> the last dim of ``reference_points`` (2 or 4)."""
    N, Lq, M, L, P = dims
    if sampling_offsets.dtype != value.dtype or attn_logits.dtype != value.dtype:
        raise RuntimeError("sampling_offsets and attn_logits must have the dtype of value")
    if spatial_shapes.dtype != torch.int32 or level_start_index.dtype != torch.int32:
        raise RuntimeError("spatial_shapes and level_start_index must be int32 tensors")
    ref_dim = reference_points.shape[-1]
    if tuple(reference_points.shape) != (N, Lq, L, ref_dim) or attn_logits.numel() != N * Lq * M * L * P:
        raise RuntimeError("reference_points must be (N,Lq,L,2|4) and attn_logits (N,Lq,M,L*P)")
    return ref_dim


def msda_forward_fused(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points):
    """MSDeformAttn's prologue + gather in one launch (inference): raw offsets (N,Lq,M,L,P,2) and raw attention logits
    (N,Lq,M,L*P) in ``value``'s dtype (fp32, fp64, bf16 or fp16), reference points (N,Lq,L,2|4) in fp32 (fp64 for fp64 values)
    -> (N,Lq,M*D)."""
    _no_autograd("msda_forward_fused", value, sampling_offsets, attn_logits, reference_points)
    if not value.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_offsets.shape
    geo = torch.float64 if value.dtype == torch.float64 else torch.float32
    reference_points = reference_points.to(geo).contiguous()
    _require_cuda_contiguous([("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                              ("sampling_offsets", sampling_offsets), ("attn_logits", attn_logits),
                              ("reference_points", reference_points)])
    ref_dim = _check_fused_operands(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points,
                                    (N, Lq, M, L, P))
    vdt = _DTYPE_CODE.get(value.dtype)
    if vdt is None:
        raise RuntimeError(f"ms_deform_attn: unsupported value dtype {value.dtype}")
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    # bytes actually streamed by the fused launch: value + out + raw offsets/logits (value dtype) + reference points
    e = value.element_size()
    nbytes = e * (N * S * M * D + N * Lq * M * D + N * Lq * M * L * P * 3) + reference_points.element_size() * reference_points.numel()
    _launch("alo_msda_forward_fused", value.device, f"msda_fwd_fused/Lq={Lq}", nbytes, 0.0, value, spatial_shapes, level_start_index,
            sampling_offsets, attn_logits, reference_points, out, N, S, M, D, L, Lq, P, ref_dim, vdt)
    return out


def head_major_supported(value, L, P):
    """The head-major fast path of the fused forward exists for the DETR-family shape only: bf16 or fp16, L = P = 4, D in {8..32}."""
    return (value.is_cuda and value.dtype in (torch.bfloat16, torch.float16) and L == 4 and P == 4 and value.shape[-1] % 8 == 0
            and value.shape[-1] <= 32)


def value_head_major(value, padding_mask=None):
    """(N, S, M, D) bf16 / fp16 -> (N, M, S, D) with the rows of padded pixels zeroed: ``value.masked_fill(mask[..., None], 0)``
    and the re-layout for ``msda_forward_fused_hm`` in one pass."""
    _no_autograd("value_head_major", value)
    _require_cuda_contiguous([("value", value)])
    N, S, M, D = value.shape
    if padding_mask is not None:
        if padding_mask.dtype != torch.bool or tuple(padding_mask.shape) != (N, S) or not padding_mask.is_cuda:
            raise RuntimeError("padding_mask must be a (N, S) bool CUDA tensor")
        padding_mask = padding_mask.contiguous()
    out = torch.empty((N, M, S, D), dtype=value.dtype, device=value.device)
    _launch("alo_value_head_major", value.device, f"value_head_major/S={S}", 2 * value.element_size() * value.numel(), 0.0,
            value, padding_mask, out, N, S, M, D, _DTYPE_CODE[value.dtype])
    return out


def _query_rows(t, inner):
    """Row stride (elements) of a (N, Lq, ...) tensor whose per-query block of ``inner`` elements is dense and whose queries are
    evenly spaced — a dense tensor or a column slice of a wider (N, Lq, C) buffer; None otherwise."""
    if t.dim() < 3 or t.shape[0] == 0 or t.shape[1] == 0:
        return None
    expect = 1
    for size, stride in zip(reversed(t.shape[2:]), reversed(t.stride()[2:])):
        if size != 1 and stride != expect:
            return None
        expect *= size
    if expect != inner:
        return None
    rs = t.stride(1) if t.shape[1] > 1 else inner
    if rs < inner or (t.shape[0] > 1 and t.stride(0) != rs * t.shape[1]):
        return None
    return rs


def msda_forward_fused_hm(value_hm, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points,
                          resident=True):
    """``msda_forward_fused`` on a head-major value (N, M, S, D) (see ``value_head_major``).
    ``sampling_offsets`` (N, Lq, M, L, P, 2) and ``attn_logits`` (N, Lq, M, L*P) may be column slices of one wider (N, Lq, C)
    buffer (a merged projection): only their per-query blocks have to be dense.
    ``resident`` (default): when a host copy of ``spatial_shapes`` rides on the tensor (``_alo_shapes``, set by
    DeformableTransformer) and D = 32, large launches keep the coarse pyramid levels in LDS
    (``alo_msda_forward_fused_hm_resident``: same products, fp32 accumulation order of the levels unchanged; the library takes
    the plain head-major kernel by itself where that one is faster — launches with less than one 16-query run per wave of the
    chip).  ``resident="always"`` takes the resident kernel wherever it can run (ALO_RESIDENT_ALWAYS), ``resident=False`` always
    runs the plain kernel, whose bf16 output is bit-identical to ``msda_forward_fused``.  fp16 values never go resident (the
    resident kernel is bf16 only): no hint is passed and ``resident`` changes nothing; their output is within half an fp16 ulp of
    the exact result like ``msda_forward_fused``'s, not bit-identical to it (two-term weight split, see include/alo_hotpath.h)."""
    _no_autograd("msda_forward_fused_hm", value_hm, sampling_offsets, attn_logits, reference_points)
    if not value_hm.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    N, M, S, D = value_hm.shape
    _, Lq, _, L, P, _ = sampling_offsets.shape
    reference_points = reference_points.float().contiguous()
    _require_cuda_contiguous([("value", value_hm), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index)])
    ref_dim = _check_fused_operands(value_hm, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points,
                                    (N, Lq, M, L, P))
    off_rs, log_rs = _query_rows(sampling_offsets, M * L * P * 2), _query_rows(attn_logits, M * L * P)
    if off_rs is None or log_rs is None or off_rs % 8 or log_rs % 8 or not sampling_offsets.is_cuda or not attn_logits.is_cuda:
        sampling_offsets, attn_logits = sampling_offsets.contiguous(), attn_logits.contiguous()
        off_rs, log_rs = M * L * P * 2, M * L * P
    out = torch.empty((N, Lq, M * D), dtype=value_hm.dtype, device=value_hm.device)
    e = value_hm.element_size()
    nbytes = e * (N * S * M * D + N * Lq * M * D + N * Lq * M * L * P * 3) + 4 * reference_points.numel()
    # coarse levels resident in LDS: needs a HOST copy of the shapes (it picks the resident levels, fixes the LDS layout and sizes the
    # grid; the kernel re-checks it against the device copy).  Only a copy that is already at hand is used — no device read in a forward.
    host = _host_spatial_shapes(spatial_shapes, read=False) if resident and value_hm.dtype == torch.bfloat16 else None
    starts = None
    if host is not None and D == 32 and len(host) == L and sum(int(h) * int(w) for h, w in host) == S:
        starts = (ctypes.c_int32 * (2 * L))(*[int(v) for hw in host for v in hw])

    policy = RESIDENT_ALWAYS if resident == "always" else RESIDENT_AUTO
    tag = "msda_fwd_fused_resident" if starts is not None and lib().alo_msda_resident_levels(starts, N, S, M, L, Lq, policy) else "msda_fwd_fused"
    symbol, hint = ("alo_msda_forward_fused_hm_rows", ()) if starts is None else ("alo_msda_forward_fused_hm_resident", (starts, policy))
    _launch(symbol, value_hm.device, f"{tag}/Lq={Lq}", nbytes, 0.0, value_hm, spatial_shapes, level_start_index, sampling_offsets,
            attn_logits, off_rs, log_rs, reference_points, out, N, S, M, D, L, Lq, P, ref_dim, _DTYPE_CODE[value_hm.dtype], *hint,
            relaunch=True)
    return out


def _host_spatial_shapes(spatial_shapes, read=True):
    """Host copy of a device ``spatial_shapes`` tensor.  It rides on the tensor OBJECT (``_alo_shapes``, tagged with the version
    counter it was read at; DeformableTransformer attaches its own list when it builds the tensor), so it dies with the tensor: a cache
    keyed on the storage pointer would hand a stale copy to the next 32-byte tensor the caching allocator places at that address.
    Without the attribute: one device-to-host read, then cached on the object — or, with ``read=False``, None unless an earlier
    read is still valid."""
    host = getattr(spatial_shapes, "_alo_shapes", None)   # attached by the model that built the tensor
    if host is not None:
        return host
    hit = getattr(spatial_shapes, "_alo_shapes_read", None)
    if hit is not None and hit[0] == tensor_version(spatial_shapes):
        return hit[1]
    if not read:
        return None
    host = [tuple(int(v) for v in hw) for hw in spatial_shapes.tolist()]
    spatial_shapes._alo_shapes_read = (tensor_version(spatial_shapes), host)
    return host


def _wide_backward_wants_host_shapes(value, dims, ldt):
    """Whether a host copy of the shapes is worth a device-to-host read: the launches msda_bwd_wide_kernel can take once it has
    one (fp32 / bf16 values, D = 32 or 64, L = P = 4, queries = the pyramid's own pixels; never fp16, whose backward is the generic
    kernel).  The library decides the route
    (csrc/msda.hip plan_backward) but needs the host shapes to do so, hence this pre-filter; tests/test_cabi.py holds the two together."""
    N, S, M, D, L, Lq, P = dims
    return value.dtype in (torch.float32, torch.bfloat16) and ldt == ALO_F32 and D in (32, 64) and L == 4 and P == 4 and Lq == S


def msda_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step=64):
    """-> [grad_value, grad_sampling_loc, grad_attn_weight].  Replaces ``alonet_custom::ms_deform_attn_backward``."""
    dims, vdt, ldt, loc, attn = _msda_prepare(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                              im2col_step, extra=[("grad_output", grad_output)])
    N, S, M, D, L, Lq, P = dims
    if grad_output.dtype != value.dtype or grad_output.numel() != N * Lq * M * D:
        raise RuntimeError("grad_output must be (N, Lq, M*D) with the dtype of value")
    gdt = torch.float64 if value.dtype == torch.float64 else torch.float32
    grad_value = torch.empty(value.shape, dtype=gdt, device=value.device)
    grad_loc = torch.empty(loc.shape, dtype=gdt, device=value.device)
    grad_attn = torch.empty(attn.shape, dtype=gdt, device=value.device)
    nbytes = msda_backward_bytes(N, S, M, D, L, Lq, P, value.element_size(), loc.element_size())
    # only the encoder's self-attention on the DETR-family shape can use the hint (it sizes the grid of query blocks)
    host = _host_spatial_shapes(spatial_shapes) if _wide_backward_wants_host_shapes(value, dims, ldt) else None
    hint = None if host is None else (ctypes.c_int32 * (2 * L))(*[int(v) for hw in host for v in hw])
    _launch("alo_msda_backward_hinted", value.device, f"msda_bwd/Lq={Lq}", nbytes, 0.0, value, spatial_shapes, level_start_index, loc,
            attn, grad_output, grad_value, grad_loc, grad_attn, N, S, M, D, L, Lq, P, vdt, ldt, hint, relaunch=True)
    return [grad_value.to(value.dtype), grad_loc.to(sampling_loc.dtype), grad_attn.to(attn_weight.dtype)]


def corr_level_shapes(H, W, num_levels):
    out = []
    h, w = ctypes.c_int(), ctypes.c_int()
    for lvl in range(num_levels):
        lib().alo_corr_level_shape(H, W, lvl, ctypes.byref(h), ctypes.byref(w))
        out.append((h.value, w.value))
    return out


def _require_f32_cuda(name, t, ndim):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (the correlation path has no CPU implementation here)")
    if t.dtype != torch.float32 or t.dim() != ndim:
        raise RuntimeError(f"{name} must be a {ndim}-d float32 tensor, got {tuple(t.shape)} {t.dtype}")


def corr_build(fmap1, fmap2, num_levels=4):
    """fmaps (B,C,H,W) float32 -> list of ``num_levels`` tensors (B*H*W, 1, h_l, w_l)  (corr.py:13-27)."""
    _require_f32_cuda("fmap1", fmap1, 4)
    _require_f32_cuda("fmap2", fmap2, 4)
    if fmap1.shape != fmap2.shape:
        raise RuntimeError("fmap1 and fmap2 must have the same shape")
    fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
    B, C, H, W = fmap1.shape
    shapes = corr_level_shapes(H, W, num_levels)
    levels = [torch.empty((B * H * W, 1, h, w), dtype=torch.float32, device=fmap1.device) for h, w in shapes]
    nbytes = lib().alo_corr_build_workspace_bytes(B, C, H, W, num_levels)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=fmap1.device)
    ncols = sum(h * w for h, w in shapes)
    # relaunch: the closure keeps the feature maps and the workspace alive for LaunchTimer.replay_samples
    _launch("alo_corr_build", fmap1.device, "corr_build", 4.0 * (2 * B * C * H * W + B * H * W * ncols), 2.0 * B * (H * W) * (H * W) * C,
            fmap1, fmap2, levels, ws, nbytes, B, C, H, W, num_levels, relaunch=True)
    # ws may be released now: the caching allocator keeps the block bound to this stream until the kernels retire
    return levels


def _corr_lookup_args(levels, levels_name, coords, radius, grad_out=None, fn=None):
    """What the three lookup entry points check alike -> (coords, grad_out) contiguous, the levels as a list, (B, H, W, L).
    ``fn``: the name the backward entry points put before their message on coords / grad_out."""
    _require_f32_cuda("coords", coords, 4)
    coords = coords.contiguous()
    B, two, H, W = coords.shape
    L = len(levels)
    if grad_out is None:
        if two != 2:
            raise RuntimeError("coords must be (B,2,H,W)")
    else:
        _require_f32_cuda("grad_out", grad_out, 4)
        grad_out = grad_out.contiguous()
        if two != 2 or tuple(grad_out.shape) != (B, L * (2 * radius + 1) ** 2, H, W):
            raise RuntimeError(f"{fn}: coords must be (B,2,H,W) and grad_out (B, L*(2r+1)^2, H, W)")
    for lvl, t in enumerate(levels):
        _require_f32_cuda(f"{levels_name}[{lvl}]", t, 4)
        if not t.is_contiguous() or t.shape[0] != B * H * W:
            raise RuntimeError(f"{levels_name}[{lvl}] must be a contiguous (B*H*W,1,h,w) tensor")
    return coords, grad_out, list(levels), (B, H, W, L)


def corr_lookup(levels, coords, radius=4):
    """levels from :func:`corr_build`, coords (B,2,H,W) -> (B, L*(2r+1)^2, H, W) float32  (corr.py:29-50)."""
    coords, _, levels, (B, H, W, L) = _corr_lookup_args(levels, "corr_pyramid", coords, radius)
    out = torch.empty((B, L * (2 * radius + 1) ** 2, H, W), dtype=torch.float32, device=coords.device)
    taps = (2 * radius + 2) ** 2
    nbytes = 4.0 * B * H * W * (L * (2 * radius + 1) ** 2 + L * taps + 2)
    _launch("alo_corr_lookup", coords.device, "corr_lookup", nbytes, 0.0, levels, coords, out, B, H, W, radius, L)
    return out


def corr_lookup_backward(grad_levels, coords, grad_out, radius=4):
    """Adds the pyramid gradients of ONE lookup to ``grad_levels`` (tensors shaped like the pyramid, zeroed by the caller before the
    first lookup whose gradients are to be summed): the adjoint of :func:`corr_lookup` with respect to the levels (autograd through
    the reference's bilinear_sampler, corr.py:29-50).  In place; returns ``grad_levels``."""
    coords, grad_out, maps, (B, H, W, L) = _corr_lookup_args(grad_levels, "grad_levels", coords, radius, grad_out,
                                                             "corr_lookup_backward")
    taps = (2 * radius + 2) ** 2
    nbytes = 4.0 * B * H * W * (L * (2 * radius + 1) ** 2 + 2 * L * taps + 2)
    _launch("alo_corr_lookup_backward", coords.device, "corr_lookup_backward", nbytes, 0.0, maps, coords, grad_out, B, H, W, radius, L)
    return grad_levels


def corr_lookup_backward_coords(levels, coords, grad_out, radius=4):
    """Gradient of :func:`corr_lookup` with respect to ``coords`` -> (B, 2, H, W): grid_sample's gradient with respect to the grid
    chained through the reference's coordinate arithmetic (corr.py:29-50); per-level maps from the kernel, added here."""
    coords, grad_out, levels, (B, H, W, L) = _corr_lookup_args(levels, "corr_pyramid", coords, radius, grad_out,
                                                             "corr_lookup_backward_coords")
    per_level = torch.empty((B, L, 2, H, W), dtype=torch.float32, device=coords.device)
    taps = (2 * radius + 2) ** 2
    nbytes = 4.0 * B * H * W * (L * (2 * radius + 1) ** 2 + L * taps + 2 + 2 * L)
    _launch("alo_corr_lookup_backward_coords", coords.device, "corr_lookup_backward_coords", nbytes, 0.0, levels, coords, grad_out,
            per_level, B, H, W, radius, L)
    return per_level.sum(1)


ALO_CORR_ALT_GRAD = 0x100   # include/alo_corr_alt.h: OR-ed into num_levels


def corr_alt_prepare(fmap1, fmap2_levels, grad=False):
    """AlternateCorrBlock.__init__ (corr.py:63-71): fmap1 (B,C,H,W) and the 2x2-mean chain of fmap2 (level l: (B,C,h_l,w_l)) ->
    the workspace of :func:`corr_alt_lookup` (uint8 tensor): channels-last copies of fmap1 and of every level, made once.
    ``grad``: the workspace also carries the gradient region of :func:`corr_alt_lookup_backward` (``ALO_CORR_ALT_GRAD`` size;
    not initialised: :func:`corr_alt_grad_views` reaches it)."""
    _require_f32_cuda("fmap1", fmap1, 4)
    for lvl, t in enumerate(fmap2_levels):
        _require_f32_cuda(f"fmap2_levels[{lvl}]", t, 4)
    B, C, H, W = fmap1.shape
    L = len(fmap2_levels)
    for lvl, ((h, w), t) in enumerate(zip(corr_level_shapes(H, W, L), fmap2_levels)):
        if tuple(t.shape) != (B, C, h, w) or t.device != fmap1.device:
            raise RuntimeError(f"fmap2_levels[{lvl}] must be ({B}, {C}, {h}, {w}) on {fmap1.device}, got {tuple(t.shape)} on {t.device}")
    fmap1 = fmap1.contiguous()
    levels = [t.contiguous() for t in fmap2_levels]
    nbytes = lib().alo_corr_alt_workspace_bytes(B, C, H, W, L)   # 0 past the limits: the call below says which
    total = lib().alo_corr_alt_workspace_bytes(B, C, H, W, L | ALO_CORR_ALT_GRAD) if grad else nbytes
    ws = torch.empty((max(total, 16),), dtype=torch.uint8, device=fmap1.device)
    moved = 4.0 * 2 * (fmap1.numel() + sum(t.numel() for t in levels))
    _launch("alo_corr_alt_prepare", fmap1.device, "corr_alt_prepare", moved, 0.0, fmap1, levels, ws, nbytes, B, C, H, W, L)
    return ws


def corr_alt_lookup(workspace, coords, channels, num_levels, radius=4):
    """AlternateCorrBlock.__call__ (corr.py:73-91): workspace from :func:`corr_alt_prepare` (same feature maps' C = ``channels``
    and ``num_levels``), coords (B,2,H,W) -> (B, L*(2r+1)^2, H, W) float32, the layout and value of :func:`corr_lookup`."""
    _require_f32_cuda("coords", coords, 4)
    if not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.device != coords.device:
        raise RuntimeError("workspace must be the uint8 CUDA tensor corr_alt_prepare returned, on the device of coords")
    coords = coords.contiguous()
    B, two, H, W = coords.shape
    if two != 2:
        raise RuntimeError("coords must be (B,2,H,W)")
    L, C, win = num_levels, channels, (2 * radius + 1) ** 2
    out = torch.empty((B, L * win, H, W), dtype=torch.float32, device=coords.device)
    flops = 2.0 * B * H * W * L * (2 * radius + 2) ** 2 * C          # the lattice's inner products (the mixes are noise)
    nbytes = 4.0 * B * H * W * (L * win + 2 + L * C)                 # out + coords + fmap1 once per level (footprints: cache hits)
    _launch("alo_corr_alt_lookup", coords.device, "corr_alt_lookup", nbytes, flops, workspace, workspace.numel(), coords, out,
            B, C, H, W, radius, L)
    return out


def corr_alt_with_grad_region(workspace, shape, num_levels):
    """A copy of a prepared ``workspace`` (:func:`corr_alt_prepare` for feature maps of ``shape`` = (B, C, H, W)) with the gradient
    region of :func:`corr_alt_lookup_backward` behind it (not initialised)."""
    B, C, H, W = shape
    total = lib().alo_corr_alt_workspace_bytes(B, C, H, W, num_levels | ALO_CORR_ALT_GRAD)
    if total == 0 or workspace.numel() != lib().alo_corr_alt_workspace_bytes(B, C, H, W, num_levels):
        raise RuntimeError("workspace must be the tensor corr_alt_prepare returned for these sizes")
    out = torch.empty((total,), dtype=torch.uint8, device=workspace.device)
    out[:workspace.numel()].copy_(workspace)
    return out


def corr_alt_grad_views(workspace, shape, num_levels):
    """The gradient region of a workspace made with ``grad=True`` for feature maps of ``shape`` = (B, C, H, W), as views (layout:
    include/alo_corr_alt.h) -> (region, planes, levels): the whole region as uint8 (to zero it), ``num_levels`` float32 planes
    (B, H*W, Cp) whose sum is grad_fmap1 channels-last, and per level the slice-major (Cp/16, B, h_l*w_l, 16) gradient of fmap2's
    level.  Works on any device (the layout is arithmetic on the sizes)."""
    B, C, H, W = shape
    cp = (C + 15) // 16 * 16
    pad = lambda n: (n + 255) // 256 * 256   # noqa: E731
    sizes = [(H, W)]
    for _ in range(num_levels - 1):
        sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
    plane = pad(B * H * W * cp * 4)
    parts = [pad(B * h * w * cp * 4) for h, w in sizes]
    start = plane + sum(parts)
    if workspace.dtype != torch.uint8 or workspace.numel() < start + num_levels * plane + sum(parts):
        raise RuntimeError("workspace must be the uint8 tensor corr_alt_prepare(..., grad=True) returned for these sizes")
    at = start
    planes, levels = [], []
    for _ in range(num_levels):
        planes.append(workspace[at:at + B * H * W * cp * 4].view(torch.float32).view(B, H * W, cp))
        at += plane
    for (h, w), part in zip(sizes, parts):
        levels.append(workspace[at:at + B * h * w * cp * 4].view(torch.float32).view(cp // 16, B, h * w, 16))
        at += part
    return workspace[start:at], planes, levels


def corr_alt_lookup_backward(workspace, coords, grad_out, channels, num_levels, radius=4):
    """Adds the feature-map gradients of ONE :func:`corr_alt_lookup` to the gradient region of ``workspace``
    (``corr_alt_prepare(..., grad=True)``; zeroed by the caller before the first lookup whose gradients are to be summed): the
    adjoint of the lookup with respect to fmap1 and every level of fmap2 (``alo_corr_alt_lookup`` with ``ALO_CORR_ALT_GRAD``).
    The prepared part of the workspace is only read.  The level gradients are summed with float atomics: their last bits depend
    on the run.  In place; returns ``workspace``."""
    _require_f32_cuda("coords", coords, 4)
    _require_f32_cuda("grad_out", grad_out, 4)
    if not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.device != coords.device:
        raise RuntimeError("workspace must be the uint8 CUDA tensor corr_alt_prepare returned, on the device of coords")
    coords, grad_out = coords.contiguous(), grad_out.contiguous()
    B, two, H, W = coords.shape
    L, C, win = num_levels, channels, (2 * radius + 1) ** 2
    if two != 2 or tuple(grad_out.shape) != (B, L * win, H, W) or grad_out.device != coords.device:
        raise RuntimeError("corr_alt_lookup_backward: coords must be (B,2,H,W) and grad_out (B, L*(2r+1)^2, H, W)")
    flops = 4.0 * B * H * W * L * (2 * radius + 2) ** 2 * C          # both adjoints of the lattice's inner products
    nbytes = 4.0 * B * H * W * (L * win + 2 + 3 * L * C)             # grad_out + coords + fmap1 once and its plane twice per level
    _launch("alo_corr_alt_lookup", coords.device, "corr_alt_lookup_backward", nbytes, flops, workspace, workspace.numel(), coords,
            grad_out, B, C, H, W, radius, L | ALO_CORR_ALT_GRAD)
    return workspace


def _grad_tensors(operands):
    """The tensors an operand list stands for: a tensor for itself, an ``nn.Module`` for every parameter it holds (its sub-modules'
    included), ``None`` (an absent bias, mask, residual) for nothing."""
    for t in operands:
        if isinstance(t, torch.nn.Module):
            yield from t.parameters()
        elif t is not None:
            yield t


def needs_autograd(*operands):
    """True when autograd would record an op on these operands (tensors, modules, ``None``): grad mode is on and one of the tensors,
    or one parameter of one of the modules, requires grad.  With grad mode off nothing is looked at."""
    return torch.is_grad_enabled() and any(t.requires_grad for t in _grad_tensors(operands))


def fusable(*operands, f16=False):
    """True when the fused epilogues may replace the stock ops: inference (no autograd graph), CUDA, fp32 or bf16 — and fp16 with
    ``f16=True``, which a caller passes when every kernel behind it serves fp16 (the transformer's layers do; the backbone, the
    input projections, the mask head and RAFT's update block do not).  The first operand is the activation (a tensor); the others
    are whatever else the fast path consumes: tensors, ``None`` for an absent one, and modules, which stand for all their
    parameters.  A call site names EVERYTHING its fast path reads — the kernels have no backward, so one trainable operand left out
    loses its gradient (and that of everything upstream of the detached result) without an error."""
    if needs_autograd(*operands):
        return False
    first = operands[0]
    return first.is_cuda and first.dtype in (torch.float32, *_half(f16))


def _no_autograd(name, *operands):
    """The wrappers' backstop, called first in every wrapper that writes through raw pointers outside an ``autograd.Function``:
    what they return carries no ``grad_fn``, so an operand that requires grad under grad mode is a caller's gate that forgot it
    (:func:`fusable`) — an error here instead of a silently missing or wrong gradient."""
    if needs_autograd(*operands):
        raise RuntimeError(f"alo_hip.{name} has no backward and an operand requires grad: call it under torch.no_grad() or with "
                           f"every operand frozen / detached, and take the stock PyTorch ops otherwise (alo_hip.fusable answers "
                           f"for a call site when given every tensor and module its fast path reads)")


def add_layernorm_supported(x):
    """What ``alo_add_layernorm`` can take: rows of C % 4 == 0, C <= 1024 elements, 16-byte aligned (callers fall back to
    ``norm(x + y)`` otherwise, e.g. for a non-default d_model)."""
    C = x.shape[-1]
    return C % 4 == 0 and 0 < C <= 1024 and (C * x.element_size()) % 16 == 0 and x.data_ptr() % 16 == 0


def invalidate_caches(module):
    """Drop every derived inference-time tensor (:func:`derived`: packed MFMA weights, folded batch-norm convolutions, merged
    projections) held by ``module``'s sub-modules, parameters and buffers; what those derived tensors own in turn goes with
    them.  In-place writes through ``.data`` (``p.data.copy_``, EMA updates, ``nn.init.*_(w.data)``) do not bump the version
    counter the entries are keyed on, so call this after such weight surgery — ``alonet.common.load_weights`` and
    ``GraphedForward`` do."""
    module.__dict__[_EPOCH] = cache_epoch(module) + 1   # GraphedForward re-captures on a new epoch
    for owner in (*module.modules(), *module.parameters(), *module.buffers()):
        owner.__dict__.pop(_DERIVED, None)


def cache_epoch(module):
    """How many times :func:`invalidate_caches` ran on ``module`` — graphs captured under an older epoch read freed tensors."""
    return module.__dict__.get(_EPOCH, 0)


# ---- one-pass epilogues around the attention op (alo_add_layernorm / alo_bias_act) ---------------------------------------
def add_layernorm(x, residual, weight, bias, eps=1e-5, pos=None):
    """``LayerNorm(x + residual)`` over the last dim in one pass; with ``pos`` also returns ``out + pos`` (the next
    layer's ``with_pos_embed``).  Replaces ``norm(src + dropout(src2))`` of the (de)formable transformer layers at
    inference.  -> out  |  (out, out_plus_pos)"""
    _no_autograd("add_layernorm", x, residual, weight, bias, pos)
    C = x.shape[-1]
    rows = x.numel() // C
    x = x.contiguous()
    residual = None if residual is None else residual.contiguous()
    pos = None if pos is None else pos.contiguous()
    for name, t in (("residual", residual), ("pos", pos)):
        if t is not None and (t.shape != x.shape or t.dtype != x.dtype):
            raise RuntimeError(f"add_layernorm: {name} must have the shape and dtype of x")
    weight, bias = weight.to(x.dtype).contiguous(), bias.to(x.dtype).contiguous()
    out = torch.empty_like(x)
    out_pos = None if pos is None else torch.empty_like(x)
    nbytes = x.element_size() * x.numel() * (2 + (residual is not None) + 2 * (pos is not None))
    _launch("alo_add_layernorm", x.device, f"add_layernorm/rows={rows}", nbytes, 0.0, x, residual, weight, bias, out, pos, out_pos,
            rows, C, float(eps), _DTYPE_CODE[x.dtype])
    return out if pos is None else (out, out_pos)


def bias_act_(x, bias, residual=None, relu=True):
    """In place on a channels-last activation ``x`` (N,C,H,W with NHWC strides) or a (rows, C) matrix:
    ``x = act(x + bias[c] (+ residual))``.  Replaces folded FrozenBatchNorm bias -> (+ identity) -> ReLU of the ResNet."""
    _no_autograd("bias_act_", x, bias, residual)
    if x.dim() == 4:
        if not x.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("bias_act_: 4-D input must be channels_last")
        C = x.shape[1]
        if residual is not None and not (residual.shape == x.shape and residual.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError("bias_act_: residual must be channels_last with the shape of x")
    else:
        if not x.is_contiguous():
            raise RuntimeError("bias_act_: matrix input must be contiguous")
        C = x.shape[-1]
        if residual is not None and not (residual.shape == x.shape and residual.is_contiguous()):
            raise RuntimeError("bias_act_: residual must be contiguous with the shape of x")
    if residual is not None and residual.dtype != x.dtype:
        raise RuntimeError("bias_act_: residual must have the dtype of x")
    bias = bias.to(x.dtype).contiguous()
    nbytes = x.element_size() * x.numel() * (2 + (residual is not None))
    _launch("alo_bias_act", x.device, f"bias_act/C={C}", nbytes, 0.0, x, bias, residual, x, x.numel() // C, C, 1 if relu else 0,
            _DTYPE_CODE[x.dtype])
    return x


# ---- RAFT update block glue (fp32, NCHW) ------------------------------------------------------------------------------------
def _require_f32_nchw(name, t):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous float32 CUDA tensor (B, C, H, W)")


def bias_act_nchw_(x, bias, relu=True):
    """In place: ``x = act(x + bias[None, :, None, None])`` — the bias MIOpen would add in a second kernel plus the ReLU."""
    _no_autograd("bias_act_nchw_", x, bias)
    _require_f32_nchw("x", x)
    B, C, H, W = x.shape
    _launch("alo_bias_act_nchw", x.device, f"bias_act_nchw/C={C}", 8.0 * x.numel(), 0.0, x, bias.float().contiguous(), x, B, C, H * W,
            1 if relu else 0)
    return x


def gru_gate_(zr, bias_zr, hx, rhx, C):
    """``zr`` (B,2C,H,W): pre-activations [z | r].  z <- sigmoid(z + b) in place; ``rhx[:, :C] <- sigmoid(r + b) * hx[:, :C]``."""
    _no_autograd("gru_gate_", zr, bias_zr, hx, rhx)
    _require_f32_nchw("zr", zr); _require_f32_nchw("hx", hx); _require_f32_nchw("rhx", rhx)
    B, C2, H, W = zr.shape
    if C2 != 2 * C or hx.shape != rhx.shape or hx.shape[0] != B or hx.shape[2:] != zr.shape[2:] or hx.shape[1] < C:
        raise RuntimeError("gru_gate_: zr must be (B,2C,H,W) and hx / rhx (B,C+Cx,H,W)")
    _launch("alo_gru_gate", zr.device, f"gru_gate/C={C}", 4.0 * B * C * H * W * 5, 0.0, zr, bias_zr, hx, rhx, B, C, H * W,
            hx.stride(0), rhx.stride(0))


def gru_update_(q, bias_q, zr, hx, C, net=None):
    """``hx[:, :C] <- (1 - z) * hx[:, :C] + z * tanh(q + b)`` with z = ``zr[:, :C]``; ``net`` (B,C,H,W) also receives the result."""
    _no_autograd("gru_update_", q, bias_q, zr, hx, net)
    _require_f32_nchw("q", q); _require_f32_nchw("zr", zr); _require_f32_nchw("hx", hx)
    B, Cq, H, W = q.shape
    if Cq != C or zr.shape != (B, 2 * C, H, W) or hx.shape[0] != B or hx.shape[2:] != q.shape[2:]:
        raise RuntimeError("gru_update_: q must be (B,C,H,W), zr (B,2C,H,W), hx (B,C+Cx,H,W)")
    if net is not None:
        _require_f32_nchw("net", net)
    _launch("alo_gru_update", q.device, f"gru_update/C={C}", 4.0 * B * C * H * W * (4 + (net is not None)), 0.0, q, bias_q, zr, hx, net,
            B, C, H * W, hx.stride(0))


def _require_f32_rows(name, t, cols=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and (cols is None or t.shape[1] == cols)):
        raise RuntimeError(f"{name} must be a contiguous float32 CUDA matrix (rows, {'channels' if cols is None else cols})")


def gru_gate_rows_(zr, bias_zr, hx, rhx, C):
    """:func:`gru_gate_` channels-last: ``zr`` (rows, 2C), ``hx`` / ``rhx`` (rows, C + Cx), a row per pixel; C % 4 == 0.  The planar
    call's results bit for bit."""
    _no_autograd("gru_gate_rows_", zr, bias_zr, hx, rhx)
    _require_f32_rows("zr", zr, 2 * C); _require_f32_rows("hx", hx); _require_f32_rows("rhx", rhx)
    rows = zr.shape[0]
    if C % 4 or hx.shape != rhx.shape or hx.shape[0] != rows or hx.shape[1] < C or hx.shape[1] % 4 or bias_zr.numel() != 2 * C:
        raise RuntimeError("gru_gate_rows_: zr must be (rows, 2C), hx / rhx (rows, C + Cx), bias_zr (2C,), C and C + Cx multiples of 4")
    _launch("alo_gru_gate", zr.device, f"gru_gate_rows/C={C}", 4.0 * rows * C * 5, 0.0, zr, bias_zr.float().contiguous(), hx, rhx, rows, C, 1,
            hx.stride(0), rhx.stride(0))


def gru_update_rows_(q, bias_q, zr, hx, C, net=None):
    """:func:`gru_update_` channels-last: ``q`` and ``net`` (rows, C), ``zr`` (rows, 2C), ``hx`` (rows, C + Cx)."""
    _no_autograd("gru_update_rows_", q, bias_q, zr, hx, net)
    _require_f32_rows("q", q, C); _require_f32_rows("zr", zr, 2 * C); _require_f32_rows("hx", hx)
    rows = q.shape[0]
    if C % 4 or zr.shape[0] != rows or hx.shape[0] != rows or hx.shape[1] < C or hx.shape[1] % 4 or bias_q.numel() != C:
        raise RuntimeError("gru_update_rows_: q must be (rows, C), zr (rows, 2C), hx (rows, C + Cx), bias_q (C,), C and C + Cx multiples of 4")
    if net is not None:
        _require_f32_rows("net", net, C)
        if net.shape[0] != rows:
            raise RuntimeError("gru_update_rows_: net must be (rows, C)")
    _launch("alo_gru_update", q.device, f"gru_update_rows/C={C}", 4.0 * rows * C * (4 + (net is not None)), 0.0, q, bias_q.float().contiguous(),
            zr, hx, net, rows, C, 1, hx.stride(0))


def pos_sine_flat(mask_flatten, spatial_shapes, level_start_index, dim_t, level_embed, normalize, center, scale, dtype,
                  eps=1e-6):
    """Sine positional encoding of the flattened pyramid + level embedding -> (B, S, 2F) in ``dtype`` (two launches).
    ``mask_flatten`` (B, S) bool, ``dim_t`` (F,) fp32, ``level_embed`` (L, 2F) or None."""
    _no_autograd("pos_sine_flat", level_embed)
    B, S = mask_flatten.shape
    L, F = spatial_shapes.shape[0], dim_t.numel()
    if mask_flatten.dtype != torch.bool or dim_t.dtype != torch.float32:
        raise RuntimeError("pos_sine_flat: mask must be bool and dim_t float32")
    mask_flatten, dim_t = mask_flatten.contiguous(), dim_t.contiguous()
    if level_embed is not None:
        level_embed = level_embed.to(dtype).contiguous()
        if tuple(level_embed.shape) != (L, 2 * F):
            raise RuntimeError("pos_sine_flat: level_embed must be (L, 2 * num_pos_feats)")
    out = torch.empty((B, S, 2 * F), dtype=dtype, device=mask_flatten.device)
    work = torch.empty((B, S, 2), dtype=torch.float32, device=mask_flatten.device)
    _launch("alo_pos_sine_flat", out.device, f"pos_sine_flat/S={S}", out.element_size() * out.numel(), 0.0, mask_flatten, spatial_shapes,
            level_start_index, dim_t, level_embed, out, work, B, S, L, F, 1 if normalize else 0, 1 if center else 0, float(scale),
            float(eps), _DTYPE_CODE[dtype])
    return out


# ---- short-K linear layers on the streaming MFMA kernel (alo_linear_shortk) -----------------------------------------------------
def linear_shortk_supported(x, weight, f16=False):
    """bf16 (with ``f16=True``: or fp16) CUDA input and weight of one dtype, K in (64, 128, 256), N % 64 == 0."""
    return (x.is_cuda and x.dtype in _half(f16) and weight.dtype == x.dtype and x.shape[-1] in (64, 128, 256)
            and weight.dim() == 2 and weight.shape[1] == x.shape[-1] and weight.shape[0] % 64 == 0)


def linear_shortk(x, weight, bias=None, relu=False, residual=None):
    """``act(x @ weight.T + bias [+ residual])`` over the last dim (64 / 128 / 256) of a bf16 / fp16 ``x``; weight (N, K), N % 64 == 0;
    ``residual`` has the shape of the result and is added before the activation."""
    _no_autograd("linear_shortk", x, weight, bias, residual)
    if not linear_shortk_supported(x, weight, f16=True):
        raise RuntimeError("linear_shortk: needs bf16 / fp16 CUDA tensors of one dtype, K in (64, 128, 256) and N % 64 == 0")
    if bias is not None and bias.dtype != x.dtype:
        raise RuntimeError("linear_shortk: bias must have the dtype of x")
    N, K = weight.shape
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], N), dtype=x.dtype, device=x.device)
    M = x2.shape[0]
    if residual is not None:
        residual = residual.reshape(-1, N)
        if residual.shape[0] != M or residual.dtype != x.dtype or not residual.is_contiguous():
            raise RuntimeError("linear_shortk: residual must be a contiguous (M, N) tensor of x's dtype")
    if M:
        nbytes = 2.0 * (x2.numel() + y.numel() * (2 if residual is not None else 1))
        _launch("alo_linear_shortk", x.device, f"linear_shortk/N={N},K={K}", nbytes, 2.0 * M * N * K, x2, weight.contiguous(),
                None if bias is None else bias.contiguous(), residual, y, M, N, K, 1 if relu else 0, _DTYPE_CODE[x.dtype])
    return y.view(*x.shape[:-1], N)


def linear_packed_supported(x, weight, f16=False):
    """bf16 (with ``f16=True``: or fp16) CUDA (input and weight of one dtype), K % 256 == 0 (K >= 512: below that linear_shortk keeps the weights in
    registers), N % 128 == 0, inference."""
    return (x.is_cuda and x.dtype in _half(f16) and weight.dtype == x.dtype and weight.dim() == 2
            and x.shape[-1] == weight.shape[1] and weight.shape[1] % 256 == 0 and weight.shape[1] >= 512
            and weight.shape[0] % 128 == 0 and not torch.is_grad_enabled())


def linear_packed(x, weight, bias=None, relu=False, residual=None):
    """``act(F.linear(x, weight, bias) [+ residual])`` with the weight streamed in MFMA fragment order (packed once per weight
    version, cached on the tensor)."""
    _no_autograd("linear_packed", x, weight, bias, residual)
    if not linear_packed_supported(x, weight, f16=True):
        raise RuntimeError("linear_packed: needs bf16 / fp16 CUDA tensors of one dtype, K % 256 == 0, K >= 512, N % 128 == 0, no autograd")
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M, K = x2.shape
    N = weight.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if residual is not None:
        residual = residual.reshape(M, N)
        if residual.dtype != x.dtype or not residual.is_contiguous():
            raise RuntimeError("linear_packed: residual must be a contiguous (M, N) tensor of the input's dtype")
    if M:
        packed = pack_mfma_b(weight)
        bias_c = None if bias is None else bias.to(x.dtype).contiguous()
        _launch("alo_linear_packed", x.device, f"linear_packed/K={K}/N={N}", 2.0 * (M * K + M * N * (2 if residual is not None else 1)),
                2.0 * M * N * K, x2, packed, bias_c, residual, y, M, N, K, 1 if relu else 0, _DTYPE_CODE[x.dtype])
    return y.view(*x.shape[:-1], N)


def conv1x1_strided_supported(x, weight2d):
    """Strided 1x1 convolution of a channels-last bf16 map addressed inside the GEMM's tile loader: the shapes linear_auto
    would send to one of the streaming kernels."""
    if not (x.dim() == 4 and x.is_cuda and x.is_contiguous(memory_format=torch.channels_last)):
        return False   # (alo_conv1x1_nhwc is bf16 only: the two GEMM gates below are asked without f16)
    if os.environ.get("ALO_CONV1X1_GATHER") == "0":   # A/B knob: gather the kept pixels with a copy kernel first
        return False
    rows = x.permute(0, 2, 3, 1)
    if linear_shortk_supported(rows, weight2d):
        return True
    return linear_packed_supported(rows, weight2d) and (weight2d.shape[0] >= 1024 or tuple(weight2d.shape) == (128, 512))


def conv1x1_strided(x, weight2d, bias, stride, relu=False):
    """``act(F.conv2d(x, weight2d[:, :, None, None], bias, stride))`` for a channels-last bf16 ``x``; returns channels-last."""
    _no_autograd("conv1x1_strided", x, weight2d, bias)
    if not conv1x1_strided_supported(x, weight2d):
        raise RuntimeError("conv1x1_strided: unsupported dtype / layout / shape")
    n, cin, h, w_ = x.shape
    cout = weight2d.shape[0]
    ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
    y = torch.empty((n, cout, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    packed = not linear_shortk_supported(x.permute(0, 2, 3, 1), weight2d)
    wt = pack_mfma_b(weight2d) if packed else weight2d.contiguous()
    bias_c = None if bias is None else bias.to(x.dtype).contiguous()
    _launch("alo_conv1x1_nhwc", x.device, f"conv1x1_strided/K={cin}/N={cout}", 2.0 * (y.numel() // cout * cin + y.numel()),
            2.0 * y.numel() * cin, x, wt, 1 if packed else 0, bias_c, None, y, n, h, w_, cin, cout, stride, 1 if relu else 0, ALO_BF16)
    return y


# ---- a bottleneck's last 1x1 convolution with its row-local neighbours (alo_conv1x1_nhwc with a chain buffer) ------------------------
CONV1X1_CHAIN, CONV1X1_CHAIN_DOWN = 2, 4   # ALO_CONV1X1_CHAIN* of include/alo_hotpath.h

# The two shape families of the entry point, keyed by conv3's input channels: conv3's output channels, the downsample convolution's
# input channels and the strides it may carry, the widths of the next convolution (csrc/conv1x1_chain.hip, csrc/conv1x1_chain_l2.hip).
_CHAIN_FAMILIES = {64: (256, 64, (1,), (64, 128)), 128: (512, 256, (1, 2), (128,))}

# The layer2 forms (down, next width) that Bottleneck._chain routes: the ones whose launch was measured faster than the launches it
# stands in for (docs/experiments.md, "Bottleneck chain for layer2").  The others are built and tested and reached through
# conv1x1_chain only.
CHAIN_LAYER2_ROUTED = frozenset({(True, 128), (False, 128), (True, 0)})


def _chain_knob():
    return os.environ.get("ALO_BOTTLENECK_CHAIN", "on").lower()


def bottleneck_chain_enabled():
    """``ALO_BOTTLENECK_CHAIN=off`` (read per call) keeps the bottlenecks on their separate launches: for tests and profiling."""
    return _chain_knob() not in ("off", "0")


def bottleneck_chain_routed(channels, down, n2):
    """Whether ``Bottleneck._chain`` sends a bottleneck whose conv3 has ``channels`` inputs through the chain launch, with its
    downsample convolution (``down``) and a next convolution of ``n2`` outputs (0: none).  ``ALO_BOTTLENECK_CHAIN=layer1`` (read per
    call) keeps ``layer2`` on its separate launches, which is the routing before ``layer2`` had a chain: for A/B runs and tests."""
    if not bottleneck_chain_enabled():
        return False
    if channels == 64:
        return True
    return channels == 128 and _chain_knob() != "layer1" and (bool(down), int(n2)) in CHAIN_LAYER2_ROUTED


def _chain_map(t, channels):
    return (t.dim() == 4 and t.is_cuda and t.dtype == torch.bfloat16 and t.shape[1] == channels and t.numel() > 0
            and t.is_contiguous(memory_format=torch.channels_last))


def _chain_vectors(*pairs):
    return all(w.dtype == torch.bfloat16 and tuple(w.shape[:2]) == (cout, cin) and w.numel() == cout * cin
               and b is not None and b.dtype == torch.bfloat16 and tuple(b.shape) == (cout,) for w, b, cout, cin in pairs)


def _chain_stride(down):
    return 1 if down is None or len(down) < 4 else int(down[3])


def conv1x1_chain_supported(mid, conv3, identity=None, down=None, nxt=None):
    """What :func:`conv1x1_chain` takes, with grad mode off: channels-last bf16 CUDA maps in one of two shape families.  ``layer1``:
    ``mid`` (N, 64, H, W), ``conv3 = (w, b)`` with 256 output channels, either ``identity`` (N, 256, H, W) or ``down = (x0, wd, bd)``
    with ``x0`` (N, 64, H, W), and, if given, ``nxt = (w1, b1)`` with 256 input and 64 or 128 output channels.  ``layer2``: ``mid``
    (N, 128, Ho, Wo), 512 output channels, ``identity`` (N, 512, Ho, Wo) or ``down = (x0, wd, bd[, stride])`` with ``x0``
    (N, 256, H, W), stride 1 or 2 and Ho = (H - 1) // stride + 1, ``nxt`` 512 -> 128.  Weights (Cout, Cin, 1, 1) or (Cout, Cin),
    every bias present."""
    if (identity is None) == (down is None) or not bottleneck_chain_enabled() or torch.is_grad_enabled():
        return False
    if mid.dim() != 4 or mid.shape[1] not in _CHAIN_FAMILIES:
        return False
    cin = mid.shape[1]
    cout, cin0, strides, widths = _CHAIN_FAMILIES[cin]
    stride = _chain_stride(down)
    if stride not in strides:
        return False
    other = identity if down is None else down[0]
    if not (_chain_map(mid, cin) and _chain_map(other, cout if down is None else cin0) and other.shape[0] == mid.shape[0]
            and tuple((d - 1) // stride + 1 for d in other.shape[2:]) == tuple(mid.shape[2:]) and other.device == mid.device):
        return False
    pairs = [(*conv3, cout, cin)] + ([] if down is None else [(down[1], down[2], cout, cin0)])
    if nxt is not None:
        if nxt[0].shape[0] not in widths:
            return False
        pairs.append((*nxt, nxt[0].shape[0], cout))
    return _chain_vectors(*pairs) and fusable(mid, other, *[t for w, b, _, _ in pairs for t in (w, b)])


def conv1x1_chain(mid, conv3, identity=None, down=None, nxt=None):
    """``y = relu(conv1x1(mid, *conv3) + identity)`` with ``identity`` given or ``conv1x1(x0, wd, bd, stride)`` for
    ``down = (x0, wd, bd[, stride])``, and with ``nxt = (w1, b1)`` also ``z = relu(conv1x1(y, w1, b1))``, in one launch; bit for bit
    the launches it stands in for (include/alo_hotpath.h, alo_conv1x1_nhwc with a chain buffer).  -> (y, z | None), channels-last."""
    _no_autograd("conv1x1_chain", mid, *conv3, identity, *((down or ())[:3]), *(nxt or ()))
    if not conv1x1_chain_supported(mid, conv3, identity, down, nxt):
        raise RuntimeError("conv1x1_chain: needs channels-last bf16 CUDA maps outside autograd, a 64 -> 256 convolution, an identity or "
                           "a 64 -> 256 downsample convolution, a next convolution 256 -> 64 or 128 (or 128 -> 512, a 256 -> 512 "
                           "downsample convolution of stride 1 or 2, a next convolution 512 -> 128), and ALO_BOTTLENECK_CHAIN not off")
    n, cin, h, w_ = mid.shape
    cout, cin0 = _CHAIN_FAMILIES[cin][:2]
    stride = _chain_stride(down)
    n2 = 0 if nxt is None else nxt[0].shape[0]
    parts = [*conv3, *(down[1:3] if down is not None else ()), *(nxt or ())]

    def chain_buffer():
        # layer2: the matrices the kernel streams (Wd, W1) go in MFMA fragment order, W3 (resident in registers) as it is (alo_hotpath.h)
        flat = [p.reshape(-1) for p in parts]
        if cin == 128:
            for i in range(2, len(parts), 2):
                flat[i] = _pack_mfma_b(parts[i].reshape(parts[i].shape[0], -1).contiguous()).reshape(-1)
        return torch.cat(flat)

    # the chain buffer rides on the convolution's (cached, folded) weight and is rebuilt when any part changes
    buf = derived(conv3[0], f"chain/{down is not None}/{n2}", parts, chain_buffer)
    rows = n * h * w_
    out = torch.empty(rows * (cout + n2), dtype=mid.dtype, device=mid.device)   # y, then z: one buffer (alo_hotpath.h)
    other = identity if down is None else down[0]
    # what the result needs: mid, the identity or the kept pixels of x0, y (+ z)
    nbytes = 2.0 * rows * (cin + (cout if down is None else cin0) + cout + n2)
    flops = 2.0 * rows * cout * (cin + (cin0 if down is not None else 0) + n2)
    form = f"{'down' if down is not None else 'res'}{f'+next{n2}' if n2 else ''}"
    tag = f"conv1x1_chain/{form}" if cin == 64 else f"bottleneck_chain/C={cin}/{form}"
    _launch("alo_conv1x1_nhwc", mid.device, tag, nbytes, flops, mid, buf, CONV1X1_CHAIN | (CONV1X1_CHAIN_DOWN if down is not None else 0) | n2,
            None, other, out, n, other.shape[2], other.shape[3], cin, cout, stride, 1, ALO_BF16)
    y = out[:rows * cout].view(n, h, w_, cout).permute(0, 3, 1, 2)
    z = None if nxt is None else out[rows * cout:].view(n, h, w_, n2).permute(0, 3, 1, 2)
    return y, z


# ---- fp32 linear layers and 1x1 convolutions on the fp16 matrix cores (alo_linear_packed / alo_conv1x1_nhwc with ALO_F32) -----------
def f32_layers_split():
    """``ALO_F32_LAYERS=split``: at inference the fp32 linear layers, 1x1 and 3x3 convolutions, feed-forward blocks and the ResNet
    stem that the split kernels serve (:func:`linear_f32`, :func:`conv1x1_strided_f32`, :func:`conv3x3_f32`, :func:`ffn_f32`,
    :func:`stem_conv_pool_f32`: fp32 on the fp16 matrix cores, two-term splits of both operands) take them instead of hipBLASLt /
    MIOpen.  Read per call; unset, every route is what it was."""
    return os.environ.get("ALO_F32_LAYERS") == "split"


# (K, N) -> the rows M at which linear_f32 beat hipBLASLt by more than both spreads (tools/gemmbench_f32.py on MI355X at the fp32
# headline's shapes; docs/experiments.md, section "`linear_f32`"), kernel / stock medians in the comments.  An M that was not measured
# goes by the nearest one that was.  Off the route because they lost or tied, K-N at M: 256-64 at 534400 (1.16), 256-128 at 534400
# (0.96, inside the spreads), 256-256 at 177784 (1.09), 256-1024 at 2400 (1.01), 512-256 at 133600 (1.13), 1024-256 at 33600 / 177784 /
# 2400 (1.41 / 1.33 / 2.45), 1024-512 at 33600 (1.00), 2048-256 at 8400 (1.89), 2048-512 at 8400 (1.15): the kernel streams its weights
# once per 64 rows, and hipBLASLt's fp32 GEMM is within a sixth of the fp32 peak at long K.
_F32_ROUTED = {
    (64, 64): (0, None),          # 0.73 at 534400
    (64, 256): (0, None),         # 0.90 at 534400
    (256, 128): (0, 1 << 18),     # 0.91 at 177784
    (256, 256): (0, 1 << 14),     # 0.84 at 2400
    (256, 384): (0, None),        # 0.95 at 177784
    (256, 512): (0, None),        # 0.86 at 2400
    (256, 1024): (1 << 14, None), # 0.96 at 177784
    (512, 128): (0, None),        # 0.98 at 133600
}


def _f32_gemm_routed(M, K, N, identity):
    """Whether ``ALO_F32_LAYERS=split`` sends a (M, K) x (N, K) product to :func:`linear_f32`.  With an identity to add the kernel won
    everywhere it was measured (K = 64, 128, 256, 512: 0.65, 0.64, 0.71, 0.74 of hipBLASLt + the separate add / ReLU pass); without
    one the table above decides."""
    if identity:
        return K <= 512
    lo, hi = _F32_ROUTED.get((K, N), (0, 0))
    return M >= lo and (hi is None or M < hi)


def linear_f32_supported(x, weight):
    """fp32 CUDA input and fp32 (N, K) weight, K % 64 == 0, N % 64 == 0, no autograd on either."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2 and x.dim() >= 1
            and x.shape[-1] == weight.shape[1] and weight.shape[1] % 64 == 0 and weight.shape[0] % 64 == 0 and weight.shape[0] > 0
            and weight.shape[1] > 0 and not needs_autograd(x, weight))


def linear_f32_routed(x, weight, identity=False):
    """Whether :func:`linear_auto` sends this product to :func:`linear_f32`: the switch is set, the kernel serves the operands and
    the shape is one it was measured to win at."""
    return (f32_layers_split() and linear_f32_supported(x, weight)
            and _f32_gemm_routed(x.numel() // max(x.shape[-1], 1), weight.shape[1], weight.shape[0], identity))


def _split_weight_of(weight):
    """The split copy of an fp32 (N, K) weight, riding on the weight (:func:`derived`): split once per weight version."""
    return derived(weight, "linear_f32_b", (weight,), lambda: _split_weight(weight))


def linear_f32(x, weight, bias=None, relu=False, residual=None):
    """``act(F.linear(x, weight, bias) [+ residual])`` for fp32 tensors on the fp16 matrix cores at fp32-class accuracy
    (csrc/gemm_f32.hip: two-term split of both operands, a power of two per row of ``x`` and per output channel, fp32
    accumulation); ``residual`` has the shape of the result and is added before the activation."""
    _no_autograd("linear_f32", x, weight, bias, residual)
    if not linear_f32_supported(x, weight):
        raise RuntimeError("linear_f32: needs fp32 CUDA tensors, a (N, K) weight, K % 64 == 0, N % 64 == 0, no autograd")
    N, K = weight.shape
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if residual is not None:
        residual = residual.reshape(M, N)
        if residual.dtype != x.dtype or not residual.is_contiguous():
            raise RuntimeError("linear_f32: residual must be a contiguous (M, N) fp32 tensor")
    if M:
        bias_c = None if bias is None else bias.float().contiguous()
        _launch("alo_linear_packed", x.device, f"linear_f32/K={K}/N={N}", 4.0 * (M * K + M * N * (2 if residual is not None else 1)),
                2.0 * M * N * K, x2, _split_weight_of(weight), bias_c, residual, y, M, N, K, 1 if relu else 0, ALO_F32)
    return y.view(*x.shape[:-1], N)


def conv1x1_strided_f32(x, weight2d, bias, stride, relu=False):
    """``act(F.conv2d(x, weight2d[:, :, None, None], bias, stride))`` for a channels-last fp32 ``x`` on :func:`linear_f32`'s kernel,
    which addresses the kept pixels itself; returns channels-last."""
    _no_autograd("conv1x1_strided_f32", x, weight2d, bias)
    if not (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and stride >= 1
            and linear_f32_supported(x.permute(0, 2, 3, 1), weight2d)):
        raise RuntimeError("conv1x1_strided_f32: needs a channels-last fp32 CUDA activation, an fp32 (Cout, Cin) weight, Cin % 64 == 0, "
                           "Cout % 64 == 0, no autograd")
    n, cin, h, w_ = x.shape
    cout = weight2d.shape[0]
    ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
    y = torch.empty((n, cout, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if y.numel():
        bias_c = None if bias is None else bias.float().contiguous()
        _launch("alo_conv1x1_nhwc", x.device, f"conv1x1_strided_f32/K={cin}/N={cout}", 4.0 * (y.numel() // cout * cin + y.numel()),
                2.0 * y.numel() * cin, x, _split_weight_of(weight2d), 1, bias_c, None, y, n, h, w_, cin, cout, stride, 1 if relu else 0, ALO_F32)
    return y


def linear_auto(x, weight, bias=None, relu=False, residual=None):
    """Inference-time ``act(F.linear(x, weight, bias) [+ residual])``: the streaming MFMA kernels when the shape allows it
    (bf16 / fp16; K in {64, 128, 256} with N % 64 == 0, or K % 256 == 0 with N % 128 == 0), otherwise the stock GEMM with the bias /
    ReLU epilogue — or, for fp32 operands under ``ALO_F32_LAYERS=split``, :func:`linear_f32`."""
    _no_autograd("linear_auto", x, weight, bias, residual)
    if linear_shortk_supported(x, weight, f16=True) and (bias is None or bias.dtype == x.dtype):
        return linear_shortk(x, weight, bias, relu, residual=residual)
    if linear_packed_supported(x, weight, f16=True) and (bias is None or bias.dtype == x.dtype) and (
            residual is not None or weight.shape[0] >= 1024 or tuple(weight.shape) == (128, 512)):
        # measured on MI355X at the backbone's shapes: the streaming kernel wins with many output columns, with the identity
        # fused in, and at (N, K) = (128, 512); hipBLASLt wins the rest
        return linear_packed(x, weight, bias, relu, residual=residual)
    if linear_f32_routed(x, weight, residual is not None):
        return linear_f32(x, weight, bias, relu, residual=residual)
    x2 = x.reshape(-1, x.shape[-1])
    fused_act = relu and residual is None
    if bias is not None:
        y = torch._addmm_activation(bias, x2, weight.t(), use_gelu=False) if fused_act else torch.addmm(bias, x2, weight.t())
    else:
        y = torch.mm(x2, weight.t())
        y = torch.relu_(y) if fused_act else y
    if residual is not None:
        y = y + residual.reshape(y.shape)
        y = torch.relu_(y) if relu else y
    return y.view(*x.shape[:-1], weight.shape[0])


def ffn256_supported(x, w1, w2, f16=False):
    """bf16 (with ``f16=True``: or fp16) CUDA (input and both weights of one dtype), d_model = 256, hidden width % 256 == 0."""
    return (x.is_cuda and x.dtype in _half(f16) and x.shape[-1] == 256 and w1.dtype == x.dtype
            and w2.dtype == x.dtype and w1.dim() == 2 and w1.shape[1] == 256 and w1.shape[0] % 256 == 0
            and tuple(w2.shape) == (256, w1.shape[0]))


def pack_mfma_b(weight):
    """(N, K) bf16 / fp16 weight -> MFMA B-fragment order (16-bit elements moved as bits).  The packed copy rides on the weight tensor object itself
    (:func:`derived`): packed once per weight update, gone with the tensor."""
    return derived(weight, "mfma_b", (weight,), lambda: _pack_mfma_b(weight.contiguous()))


def _pack_mfma_b(w):
    """The pack kernel on a contiguous (N, K) bf16 / fp16 matrix."""
    if w.dtype not in _half(True):
        raise RuntimeError("pack_mfma_b: needs a bf16 / fp16 weight")
    packed = torch.empty_like(w)
    _launch("alo_pack_mfma_b", w.device, None, 0.0, 0.0, w, packed, w.shape[0], w.shape[1], _DTYPE_CODE[w.dtype])   # once per weight version: untimed
    return packed


def ffn256(x, w1, b1, w2, b2):
    """``relu(x @ w1.T + b1) @ w2.T + b2`` over the last dim (= 256) of a bf16 / fp16 ``x`` in one kernel (hidden width % 256 == 0);
    the hidden activation is rounded to ``x``'s dtype before the second product, as two launches would store it."""
    _no_autograd("ffn256", x, w1, b1, w2, b2)
    if not ffn256_supported(x, w1, w2, f16=True):
        raise RuntimeError("ffn256: needs bf16 / fp16 CUDA tensors of one dtype, d_model = 256 and a hidden width that is a multiple of 256")
    x2 = x.reshape(-1, 256)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = torch.empty_like(x2)
    M, Fh = x2.shape[0], w1.shape[0]
    if M:
        p1, p2 = pack_mfma_b(w1), pack_mfma_b(w2)
        _launch("alo_ffn256", x.device, f"ffn256/F={Fh}", 4.0 * x2.numel(), 4.0 * M * 256 * Fh, x2, p1,
                None if b1 is None else b1.to(x.dtype).contiguous(), p2, None if b2 is None else b2.to(x.dtype).contiguous(), y, M, Fh,
                _DTYPE_CODE[x.dtype])
    return y.view(x.shape)


# ---- the fp32 feed-forward block in one kernel on the fp16 matrix cores (alo_ffn256 with ALO_F32) ----------------------------------
# The widest hidden layer whose LDS frame fits (csrc/ffn_f32.hip: two split 64 x 256 tiles of 66560 bytes, (F + 256) x 8 bytes of
# biases and exponents, 1280 bytes of row tables, against alo::launch's 160 KiB); the entry point refuses the next multiple of 256.
FFN_F32_MAX_HIDDEN = 3328


def ffn_f32_supported(x, w1, w2):
    """fp32 CUDA input with last dimension 256, an fp32 (F, 256) ``w1`` with F % 256 == 0 and F <= :data:`FFN_F32_MAX_HIDDEN`, an
    fp32 (256, F) ``w2``, no autograd on any of them."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 1 and x.shape[-1] == 256 and w1.dtype == torch.float32
            and w2.dtype == torch.float32 and w1.dim() == 2 and w1.shape[1] == 256 and w1.shape[0] % 256 == 0
            and 0 < w1.shape[0] <= FFN_F32_MAX_HIDDEN and w2.dim() == 2 and tuple(w2.shape) == (256, w1.shape[0])
            and not needs_autograd(x, w1, w2))


# F -> the rows M at which ffn_f32 beat the two launches that _ffn otherwise makes on the split route (linear_auto twice) by more than
# both spreads (tools/gemmbench_f32.py on MI355X at the fp32 headline's shapes; docs/experiments.md, section "`ffn_f32`"), kernel /
# stock medians in the comments.  An M that was not measured goes by the nearest one that was; an F that was not measured is not
# routed.  Off the route: F = 1024 at M = 2400 (0.96, inside the spreads: one tile per workgroup on 38 of 256 CUs).
_FFN_F32_ROUTED = {
    1024: (1 << 14, None),        # 0.45 at 177784
    2048: (0, None),              # 0.54 at 8400
}


def ffn_f32_routed(x, w1, w2):
    """Whether the transformer's feed-forward block takes :func:`ffn_f32`: the switch is set (:func:`f32_layers_split`), the kernel
    serves the operands and (F, M) is a shape it was measured to win at."""
    if not (f32_layers_split() and ffn_f32_supported(x, w1, w2)):
        return False
    lo, hi = _FFN_F32_ROUTED.get(w1.shape[0], (0, 0))
    M = x.numel() // 256
    return M >= lo and (hi is None or M < hi)


def ffn_f32(x, w1, b1, w2, b2):
    """``relu(x @ w1.T + b1) @ w2.T + b2`` over the last dim (= 256) of an fp32 ``x`` in one kernel on the fp16 matrix cores at
    fp32-class accuracy (csrc/ffn_f32.hip: :func:`linear_f32`'s two-term splits, a power of two per row of ``x`` and per row and
    256-unit chunk of the hidden activation, which never leaves the chip)."""
    _no_autograd("ffn_f32", x, w1, b1, w2, b2)
    if not ffn_f32_supported(x, w1, w2):
        raise RuntimeError(f"ffn_f32: needs fp32 CUDA tensors, d_model = 256, a hidden width that is a multiple of 256 and at most "
                           f"{FFN_F32_MAX_HIDDEN}, no autograd")
    x2 = x.reshape(-1, 256)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = torch.empty_like(x2)
    M, Fh = x2.shape[0], w1.shape[0]
    if M:
        _launch("alo_ffn256", x.device, f"ffn_f32/F={Fh}", 8.0 * M * 256, 4.0 * M * 256 * Fh, x2, _split_weight_of(w1),
                None if b1 is None else b1.float().contiguous(), _split_weight_of(w2), None if b2 is None else b2.float().contiguous(),
                y, M, Fh, ALO_F32)
    return y.view(x.shape)


ALO_CONV_DILATION_2 = 0x800   # include/alo_hotpath.h: OR-ed into alo_conv3x3_nhwc's stride (stride 1, dilation 2, padding 2)
_CONV3X3_GEOMETRIES = (((1, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1)), ((1, 1), (2, 2), (2, 2)))   # (stride, padding, dilation)


def _conv3x3_gate(dtype, x, weight, stride, padding, dilation, groups):
    """3x3 convolution — padding 1 at stride 1 or 2, or dilation 2 with padding 2 at stride 1 — of a channels-last CUDA activation of
    ``dtype``, Cin % 64 == 0, Cout % 64 == 0."""
    return (x.is_cuda and x.dtype == dtype and weight.dtype == dtype and x.dim() == 4 and weight.dim() == 4
            and tuple(weight.shape[2:]) == (3, 3) and (tuple(stride), tuple(padding), tuple(dilation)) in _CONV3X3_GEOMETRIES
            and groups == 1 and weight.shape[1] == x.shape[1] and x.shape[1] % 64 == 0
            and weight.shape[0] % 64 == 0 and x.is_contiguous(memory_format=torch.channels_last)
            and not torch.is_grad_enabled())


def conv3x3_supported(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1):
    """3x3 / padding 1 / stride 1 or 2 convolution, or 3x3 / dilation 2 / padding 2 / stride 1, of a channels-last bf16 CUDA
    activation, Cin % 64 == 0, Cout % 64 == 0."""
    return _conv3x3_gate(torch.bfloat16, x, weight, stride, padding, dilation, groups)


# Whether a model's dilated 3x3 (layer4.1 / layer4.2 conv2 of a DC5 backbone) takes the kernel instead of MIOpen + bias_act_: set by
# the measurement at 8 x 512 x 50 x 84 and 1 x 512 x 50 x 84 (tools/convbench.py --dilated, tools/convbench_f32.py --only dilated;
# docs/experiments.md, "Dilated 3x3"): 0.53 and 0.49 of the stock route in bf16 (198 against 374 us, 48 against 97), 0.54 and 0.45 in fp32
# (752 against 1381 us, 224 against 495), every difference above the larger spread.  The wrappers serve the dilated call either way.
CONV3X3_DILATED_ROUTED = True
CONV3X3_F32_DILATED_ROUTED = True


def conv3x3_dilated_routed(dtype=torch.bfloat16):
    """Whether ``conv_bn`` sends a dilated 3x3 of ``dtype`` to :func:`conv3x3` / :func:`conv3x3_f32`: measured to win, and
    ``ALO_CONV3X3_DILATED=off`` (read per call: A/B runs and tests) not set."""
    routed = CONV3X3_F32_DILATED_ROUTED if dtype == torch.float32 else CONV3X3_DILATED_ROUTED
    return routed and os.environ.get("ALO_CONV3X3_DILATED", "on").lower() not in ("off", "0")


def _conv3x3_geometry(stride, dilation):
    """(stride, dilation) as ints, the ``stride`` argument of alo_conv3x3_nhwc and the tag's suffix for them."""
    stride = stride[0] if isinstance(stride, (tuple, list)) else stride
    dilation = dilation[0] if isinstance(dilation, (tuple, list)) else dilation
    if dilation == 1:
        return stride, dilation, stride, f"s={stride}"
    return stride, dilation, stride | ALO_CONV_DILATION_2, f"s={stride}/d={dilation}"


def conv3x3(x, weight, bias=None, relu=False, stride=1, dilation=1):
    """``act(F.conv2d(x, weight, bias, stride, dilation, dilation))`` for a channels-last bf16 ``x`` (N, Cin, H, W): implicit GEMM on
    MFMA with the bias and the ReLU in its epilogue; ``dilation`` 2 (padding 2) at stride 1 only.  Returns a channels-last
    (N, Cout, Ho, Wo) tensor."""
    _no_autograd("conv3x3", x, weight, bias)
    stride, dilation, flagged, suffix = _conv3x3_geometry(stride, dilation)
    if not conv3x3_supported(x, weight, (stride, stride), (dilation, dilation), (dilation, dilation)):
        raise RuntimeError("conv3x3: needs a channels-last bf16 CUDA activation, a (Cout, Cin, 3, 3) weight, Cin % 64 == 0, "
                           "Cout % 64 == 0, stride 1 or 2 (dilation 2: stride 1), no autograd")
    n, cin, h, w_ = x.shape
    cout = weight.shape[0]
    # (Cout, ky, kx, Cin) row-major = the channels-last memory of the weight; pack it as a (Cout, 9 Cin) matrix
    packed = derived(weight, "conv3x3_b", (weight,),
                     lambda: _pack_mfma_b(weight.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()))
    ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
    y = torch.empty((n, cout, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bias_c = None if bias is None else bias.contiguous()
    ws_bytes = lib().alo_conv3x3_workspace_bytes(n, h, w_, cin, cout, flagged)   # split-K partial sums (few-tile shapes only)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if ws_bytes else None
    _launch("alo_conv3x3_nhwc", x.device, f"conv3x3/C={cin}/{suffix}", 2.0 * (x.numel() + y.numel()), 2.0 * 9 * cin * y.numel(),
            x, packed, bias_c, y, ws, n, h, w_, cin, cout, flagged, 1 if relu else 0, ALO_BF16)
    return y


def conv3x3_f32_supported(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1):
    """The shape rules of :func:`conv3x3_supported` for a channels-last fp32 CUDA activation and an fp32 weight."""
    return _conv3x3_gate(torch.float32, x, weight, stride, padding, dilation, groups)


def split_exponent(absmax):
    """``split_exponent`` of csrc/split_f16.hpp on a tensor of non-negative fp32 magnitudes: the power of two that brings each into
    [2^14, 2^15); 0 for zero, subnormal and non-finite entries.  -> int32"""
    e = absmax.contiguous().view(torch.int32) >> 23
    return torch.where((e == 0) | (e == 255), torch.zeros_like(e), (e - 141).clamp(-110, 110))


def _split_weight(weight):
    """``w_packed`` of an ALO_F32 call of ``alo_conv3x3_nhwc`` (a (Cout, Cin, 3, 3), (1, 5) or (5, 1) weight), ``alo_linear_packed`` or
    ``alo_conv1x1_nhwc`` (a (N, K) weight) as one uint8 tensor (include/alo_hotpath.h): the packed high terms, the packed low terms,
    the output channels' exponents."""
    if weight.dim() == 4:
        weight = weight.permute(0, 2, 3, 1).reshape(weight.shape[0], -1)   # as conv3x3 lays the matrix out
    rows = weight.float()
    mag = rows.abs()
    k = split_exponent(torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)).amax(1))
    scaled = rows * ((127 - k) << 23).view(torch.float32)[:, None]   # 2^-k built from its bits: exact (torch.ldexp on the GPU multiplies
                                                                     # by a computed power, and is off by an ulp on most elements)
    hi = scaled.half()
    lo = (scaled - hi.float()).half()                            # the difference is exact in fp32
    return torch.cat([_pack_mfma_b(hi.contiguous()).view(torch.uint8).flatten(), _pack_mfma_b(lo.contiguous()).view(torch.uint8).flatten(),
                      k.view(torch.uint8).flatten()])


def conv3x3_f32(x, weight, bias=None, relu=False, stride=1, dilation=1):
    """``act(F.conv2d(x, weight, bias, stride, dilation, dilation))`` for a channels-last fp32 ``x`` (N, Cin, H, W) and an fp32 weight,
    on the fp16 matrix cores at fp32-class accuracy (csrc/conv_f32.hip: two-term split of both operands, a power of two per image and
    per output channel, fp32 accumulation); ``dilation`` 2 (padding 2) at stride 1 only.  Returns a channels-last fp32
    (N, Cout, Ho, Wo) tensor."""
    _no_autograd("conv3x3_f32", x, weight, bias)
    stride, dilation, flagged, suffix = _conv3x3_geometry(stride, dilation)
    if not conv3x3_f32_supported(x, weight, (stride, stride), (dilation, dilation), (dilation, dilation)):
        raise RuntimeError("conv3x3_f32: needs a channels-last fp32 CUDA activation, an fp32 (Cout, Cin, 3, 3) weight, Cin % 64 == 0, "
                           "Cout % 64 == 0, stride 1 or 2 (dilation 2: stride 1), no autograd")
    n, cin, h, w_ = x.shape
    cout = weight.shape[0]
    packed = derived(weight, "conv3x3_f32_b", (weight,), lambda: _split_weight(weight))
    ho, wo = (h - 1) // stride + 1, (w_ - 1) // stride + 1
    y = torch.empty((n, cout, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bias_c = None if bias is None else bias.float().contiguous()
    # the split-K bytes of the bf16 call (unused by this kernel) + the per-image magnitudes, rounded up to 256 bytes
    ws_bytes = lib().alo_conv3x3_workspace_bytes(n, h, w_, cin, cout, flagged) + (4 * n + 255) // 256 * 256
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    _launch("alo_conv3x3_nhwc", x.device, f"conv3x3_f32/C={cin}/{suffix}", 4.0 * (x.numel() + y.numel()), 2.0 * 9 * cin * y.numel(),
            x, packed, bias_c, y, ws, n, h, w_, cin, cout, flagged, 1 if relu else 0, ALO_F32)
    return y


ALO_CONV_TAPS_1X5, ALO_CONV_TAPS_5X1 = 0x100, 0x200   # include/alo_hotpath.h: OR-ed into alo_conv3x3_nhwc's stride
_CONV_TAPS = {(1, 5): ((0, 2), ALO_CONV_TAPS_1X5, "1x5"), (5, 1): ((2, 0), ALO_CONV_TAPS_5X1, "5x1")}   # kernel -> padding, flag, name


def conv_taps_f32_supported(x, weight, padding):
    """1x5 / padding (0, 2) or 5x1 / padding (2, 0) convolution (stride 1, no dilation, no groups) of a channels-last fp32 CUDA
    activation with an fp32 weight, Cin % 64 == 0, Cout % 64 == 0, no autograd."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and weight.dim() == 4
            and tuple(weight.shape[2:]) in _CONV_TAPS and tuple(padding) == _CONV_TAPS[tuple(weight.shape[2:])][0]
            and weight.shape[1] == x.shape[1] and x.shape[1] % 64 == 0 and weight.shape[0] % 64 == 0
            and x.is_contiguous(memory_format=torch.channels_last) and not torch.is_grad_enabled())


def conv_taps_f32(x, weight, bias=None, relu=False):
    """``act(F.conv2d(x, weight, bias, 1, padding))`` for a (Cout, Cin, 1, 5) weight with padding (0, 2) or a (Cout, Cin, 5, 1) weight with
    padding (2, 0) — RAFT's SepConvGRU — on a channels-last fp32 ``x``: the arithmetic of :func:`conv3x3_f32` over five taps
    (csrc/conv_f32.hip, conv_taps_f32_kernel).  Returns a channels-last fp32 (N, Cout, H, W) tensor."""
    _no_autograd("conv_taps_f32", x, weight, bias)
    taps = _CONV_TAPS.get(tuple(weight.shape[2:])) if weight.dim() == 4 else None
    if taps is None or not conv_taps_f32_supported(x, weight, taps[0]):
        raise RuntimeError("conv_taps_f32: needs a channels-last fp32 CUDA activation, an fp32 (Cout, Cin, 1, 5) or (Cout, Cin, 5, 1) weight, "
                           "Cin % 64 == 0, Cout % 64 == 0, no autograd")
    _, flag, name = taps
    n, cin, h, w_ = x.shape
    cout = weight.shape[0]
    packed = derived(weight, "conv_taps_f32_b", (weight,), lambda: _split_weight(weight))   # tap-major (Cout, 5 Cin) either way
    y = torch.empty((n, cout, h, w_), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bias_c = None if bias is None else bias.float().contiguous()
    ws_bytes = lib().alo_conv3x3_workspace_bytes(n, h, w_, cin, cout, 1 | flag) + (4 * n + 255) // 256 * 256   # the per-image magnitudes
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    _launch("alo_conv3x3_nhwc", x.device, f"conv{name}_f32/C={cin}", 4.0 * (x.numel() + y.numel()), 2.0 * 5 * cin * y.numel(),
            x, packed, bias_c, y, ws, n, h, w_, cin, cout, 1 | flag, 1 if relu else 0, ALO_F32)
    return y


def stem_conv_pool_supported(x, weight):
    """bf16 CUDA (N, 3, H, W) image (any strides), (64, 3, 7, 7) bf16 weight, inference."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] == 3
            and tuple(weight.shape) == (64, 3, 7, 7) and not torch.is_grad_enabled())


def stem_conv_pool(x, weight, bias=None):
    """``max_pool2d(relu(conv2d(x, weight, bias, stride=2, padding=3)), 3, 2, 1)`` — the ResNet stem — in one kernel.
    Returns a channels-last (N, 64, Hp, Wp) bf16 tensor."""
    _no_autograd("stem_conv_pool", x, weight, bias)
    if not stem_conv_pool_supported(x, weight):
        raise RuntimeError("stem_conv_pool: needs a bf16 CUDA (N, 3, H, W) image, a (64, 3, 7, 7) bf16 weight, no autograd")
    n, _, h, w_ = x.shape

    def pack():
        # (64, 7 tap rows x 24): per tap row the 7 taps x 3 channels interleaved as the image rows are, then 3 zero columns
        wm = torch.zeros((64, 8, 24), dtype=weight.dtype, device=weight.device)
        wm[:, :7, :21] = weight.permute(0, 2, 3, 1).reshape(64, 7, 21)
        return _pack_mfma_b(wm.reshape(64, 192)[:, :176].contiguous())

    packed = derived(weight, "stem_b", (weight,), pack)
    hc, wc = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    y = torch.empty((n, 64, hp, wp), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bias_c = None if bias is None else bias.contiguous()
    sn, sc, sh, sw = x.stride()
    _launch("alo_stem_conv_pool", x.device, "stem_conv_pool", 2.0 * (x.numel() + y.numel()), 2.0 * 147 * 64 * n * hc * wc,
            x, packed, bias_c, y, n, h, w_, sn, sc, sh, sw, ALO_BF16)
    return y


# ---- the fp32 stem in one kernel on the fp16 matrix cores (alo_stem_conv_pool with ALO_F32) ------------------------------------------
def stem_conv_pool_f32_supported(x, weight):
    """fp32 CUDA (N, 3, H, W) image (any strides), (64, 3, 7, 7) fp32 weight, no autograd on either."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
            and tuple(weight.shape) == (64, 3, 7, 7) and not needs_autograd(x, weight))


# Whether ``ALO_F32_LAYERS=split`` sends the fp32 ResNet stem to :func:`stem_conv_pool_f32`: the kernel against what the default fp32
# route launches (channels-last copy + MIOpen's 7x7 + bias_act_ + max_pool2d), tools/stembench_f32.py on MI355X, medians (min - max) of
# 5 rounds x 20 calls; docs/experiments.md, section "`stem_conv_pool_f32`".  8 x 3 x 800 x 1333: 384.4 us (382.7 - 408.5) against 1000.9
# (998.3 - 1026.6), 0.38; 1 x 3 x 800 x 1333: 60.7 (60.2 - 63.0) against 141.4 (140.3 - 145.8), 0.43: below the stock median by more than
# both spreads at both, so the route is on
STEM_F32_ROUTED = True


def stem_f32_routed(x, weight):
    """Whether the backbone's fp32 stem takes :func:`stem_conv_pool_f32`: the switch is set (:func:`f32_layers_split`), the kernel
    serves the operands and it was measured to win (:data:`STEM_F32_ROUTED`)."""
    return STEM_F32_ROUTED and f32_layers_split() and stem_conv_pool_f32_supported(x, weight)


def stem_matrix(weight):
    """The (64, 176) matrix of ``alo_stem_conv_pool`` from a (64, 3, 7, 7) weight: per tap row the 7 taps x 3 channels interleaved as
    the staged image rows are, then 3 zero columns; the eighth tap row is cut after its first 8 (zero) columns."""
    wm = torch.zeros((64, 8, 24), dtype=weight.dtype, device=weight.device)
    wm[:, :7, :21] = weight.permute(0, 2, 3, 1).reshape(64, 7, 21)
    return wm.reshape(64, 192)[:, :176].contiguous()


def stem_conv_pool_f32(x, weight, bias=None):
    """``max_pool2d(relu(conv2d(x, weight, bias, stride=2, padding=3)), 3, 2, 1)`` — the ResNet stem — for an fp32 image of any strides
    in one kernel on the fp16 matrix cores at fp32-class accuracy (csrc/stem_f32.hip: :func:`conv3x3_f32`'s two-term splits, a power
    of two per output channel and per staged window of the image).  Returns a channels-last (N, 64, Hp, Wp) fp32 tensor."""
    _no_autograd("stem_conv_pool_f32", x, weight, bias)
    if not stem_conv_pool_f32_supported(x, weight):
        raise RuntimeError("stem_conv_pool_f32: needs an fp32 CUDA (N, 3, H, W) image, a (64, 3, 7, 7) fp32 weight, no autograd")
    n, _, h, w_ = x.shape
    packed = derived(weight, "stem_f32_b", (weight,), lambda: _split_weight(stem_matrix(weight)))
    hc, wc = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    y = torch.empty((n, 64, hp, wp), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if y.numel():
        bias_c = None if bias is None else bias.float().contiguous()
        sn, sc, sh, sw = x.stride()
        _launch("alo_stem_conv_pool", x.device, "stem_conv_pool_f32", 4.0 * (x.numel() + y.numel()), 2.0 * 147 * 64 * n * hc * wc,
                x, packed, bias_c, y, n, h, w_, sn, sc, sh, sw, ALO_F32)
    return y


def groupnorm_rows_supported(x, weight, groups, narrow=False):
    """bf16 CUDA channels-last rows (B, HW, C); C / 8 and ``groups`` divide 256; whole 8-channel slices per group — or, with
    ``narrow`` (``groupnorm_nhwc``), 2 or 4 channels per group."""
    c_ = x.shape[-1]
    cpg = c_ // groups if groups and c_ % groups == 0 else 0
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3 and weight is not None and weight.dtype == torch.bfloat16
            and c_ % 8 == 0 and 256 % (c_ // 8) == 0 and cpg > 0 and (cpg % 8 == 0 or (narrow and cpg in (2, 4))) and 256 % groups == 0
            and not torch.is_grad_enabled())


def groupnorm_nhwc_supported(x, norm):
    """``groupnorm_nhwc`` covers: bf16 CUDA (N, C, H, W) channels-last maps, affine GroupNorm with 2, 4 or a multiple of 8 channels
    per group, no autograd."""
    return (x.dim() == 4 and x.is_cuda and x.is_contiguous(memory_format=torch.channels_last) and norm.affine
            and groupnorm_rows_supported(x.new_empty((1, 1, x.shape[1])), norm.weight, norm.num_groups, narrow=True))


def groupnorm_nhwc(x, norm, relu=False):
    """``relu?(norm(x))`` for a channels-last bf16 map (N, C, H, W) and an ``nn.GroupNorm``; channels-last result.  ATen's GroupNorm
    works on NCHW: on a channels-last activation it costs a layout copy before and (for the next convolution) after."""
    _no_autograd("groupnorm_nhwc", x, norm)
    if not groupnorm_nhwc_supported(x, norm):
        raise RuntimeError("groupnorm_nhwc: needs a channels-last bf16 CUDA map and 2, 4 or 8k channels per group, no autograd")
    n, c_, h, w_ = x.shape
    rows = x.permute(0, 2, 3, 1)            # (N, H, W, C) view of the same memory
    out = torch.empty_like(x)               # preserves channels-last
    if n and h * w_:
        nbytes = lib().alo_groupnorm_rows_workspace_bytes(n, h * w_, norm.num_groups)
        ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
        _launch("alo_groupnorm_rows_act", x.device, f"groupnorm_nhwc/C={c_}", 6.0 * x.numel(), 0.0, rows, norm.weight.contiguous(),
                norm.bias.contiguous(), out, ws, n, h * w_, c_, norm.num_groups, float(norm.eps), h * w_ * c_, 1 if relu else 0, ALO_BF16)
    return out


def instancenorm_nhwc_f32_supported(x):
    """``instancenorm_nhwc_f32`` covers: fp32 CUDA (N, C, H, W) channels-last maps with C % 64 == 0, C <= 256, no autograd."""
    return (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 64 == 0 and 0 < x.shape[1] <= 256
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0 and not needs_autograd(x))


def instancenorm_nhwc_f32(x, eps=1e-5, relu=False, out=None):
    """``relu?(F.instance_norm(x, eps=eps))`` (no affine, no running statistics: ``nn.InstanceNorm2d``'s default) for a channels-last
    fp32 map (N, C, H, W); channels-last result (csrc/instancenorm_f32.hip: chunk statistics, a merge, the normalise pass).  ``out``:
    where the result goes — ``x`` itself (in place), or a channels-last (N, C, H, W) fp32 map whose images may lie further apart than
    H * W * C elements; what lies between them is not touched."""
    _no_autograd("instancenorm_nhwc_f32", x, out)
    if not instancenorm_nhwc_f32_supported(x):
        raise RuntimeError("instancenorm_nhwc_f32: needs a channels-last fp32 CUDA map with C % 64 == 0, C <= 256, no autograd")
    n, c_, h, w_ = x.shape
    if out is None:
        out = torch.empty_like(x)           # preserves channels-last
    elif (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or out.data_ptr() % 16
          or any(out.stride(d) != s for d, s in ((1, 1), (2, w_ * c_), (3, c_)) if out.shape[d] > 1)
          or (n > 1 and (out.stride(0) < h * w_ * c_ or out.stride(0) % 4))):
        raise RuntimeError("instancenorm_nhwc_f32: out must be an fp32 (N, C, H, W) map of the input's shape and device with channels-last "
                           "images, 16-byte aligned")
    image_stride = out.stride(0) if n > 1 else h * w_ * c_
    if n and h * w_:
        nbytes = lib().alo_groupnorm_rows_workspace_bytes(n, h * w_, c_)
        ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
        _launch("alo_groupnorm_rows_act", x.device, f"instancenorm_f32/C={c_}", 12.0 * x.numel(), 0.0, x, None, None, out, ws,
                n, h * w_, c_, c_, float(eps), image_stride, 1 if relu else 0, ALO_F32)
    return out


def conv3x3_small_supported(x, conv):
    """``conv3x3_small`` covers: an ``nn.Conv2d`` 3x3 / stride 1 / padding 1 with Cin in (16, 32, 64) and Cout = 1 or 4k <= 32 on a
    channels-last bf16 CUDA map, no autograd."""
    w = conv.weight
    return (isinstance(conv, torch.nn.Conv2d) and x.dim() == 4 and x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros" and w.shape[1] == x.shape[1] and x.shape[1] in (16, 32, 64)
            and (w.shape[0] == 1 or (w.shape[0] % 4 == 0 and w.shape[0] <= 32))
            and x.is_contiguous(memory_format=torch.channels_last) and not torch.is_grad_enabled())


def _small_conv_operands(conv):
    """(w_frag, bias32) of alo_conv3x3_small_nhwc, cached on the module per weight / bias version."""
    w, b = conv.weight, conv.bias

    def build():
        cout, cin = w.shape[:2]
        full = torch.zeros((32, 3, 3, cin), dtype=w.dtype, device=w.device)
        full[:cout] = w.permute(0, 2, 3, 1)                                            # (m, ky, kx, c)
        frag = full.view(32, 9, cin // 16, 2, 8).permute(1, 2, 3, 0, 4).contiguous()   # (tap, cs, kg, m, 8) = [k-step][lane][8]
        bias32 = torch.zeros(32, dtype=torch.float32, device=w.device)
        if b is not None:
            bias32[:cout] = b.float()
        return frag, bias32

    return derived(conv, "small_frag", (w, b), build)


def conv3x3_small(x, conv):
    """``conv(x)`` for the few-channel 3x3 convolutions of the mask decoder (channels-last bf16 in and out)."""
    _no_autograd("conv3x3_small", x, conv)
    if not conv3x3_small_supported(x, conv):
        raise RuntimeError("conv3x3_small: needs a channels-last bf16 CUDA map, a 3x3 / stride 1 / padding 1 convolution with Cin in "
                           "(16, 32, 64) and Cout = 1 or 4k <= 32, no autograd")
    n, cin, h, w_ = x.shape
    cout = conv.weight.shape[0]
    frag, bias32 = _small_conv_operands(conv)
    y = torch.empty((n, cout, h, w_), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if y.numel():
        _launch("alo_conv3x3_small_nhwc", x.device, f"conv3x3_small/C={cin}->{cout}", 2.0 * (x.numel() + y.numel()),
                2.0 * 9 * cin * cout * n * h * w_, x, frag, bias32, y, n, h, w_, cin, cout, ALO_BF16)
    return y


def upsample_add_supported(x_low, fpn):
    return (x_low.dim() == 4 and fpn.dim() == 4 and x_low.is_cuda and x_low.dtype == torch.bfloat16 and fpn.dtype == torch.bfloat16
            and x_low.shape[1] == fpn.shape[1] and x_low.shape[1] % 8 == 0 and fpn.shape[0] > 0 and x_low.shape[0] % fpn.shape[0] == 0
            and x_low.is_contiguous(memory_format=torch.channels_last) and fpn.is_contiguous(memory_format=torch.channels_last)
            and not torch.is_grad_enabled())


def upsample_add(x_low, fpn):
    """``fpn.repeat_interleave(Q, 0) + F.interpolate(x_low, size=fpn.shape[-2:], mode="nearest")`` in one pass (Q = x_low.shape[0]
    // fpn.shape[0]); channels-last bf16 in and out, bit-identical to the stock ops."""
    _no_autograd("upsample_add", x_low, fpn)
    if not upsample_add_supported(x_low, fpn):
        raise RuntimeError("upsample_add: needs channels-last bf16 CUDA maps with C % 8 == 0 and x_low.shape[0] a multiple of fpn.shape[0]")
    bq, c_, h, w_ = x_low.shape
    b_, _, H, W = fpn.shape
    out = torch.empty((bq, c_, H, W), dtype=x_low.dtype, device=x_low.device, memory_format=torch.channels_last)
    if out.numel():
        _launch("alo_upsample_add_nhwc", x_low.device, f"upsample_add/C={c_}", 2.0 * (out.numel() + x_low.numel() + fpn.numel()), 0.0,
                x_low, fpn, out, bq, bq // b_, c_, h, w_, H, W, ALO_BF16)
    return out


def upsample_flow_supported(flow, mask=None):
    """``upsample_flow`` covers: a contiguous fp32 CUDA flow (N, C, h, w) with 1 <= C <= 8, 16-byte aligned, and a contiguous fp32
    mask (N, 576, h, w) on the same device, 16-byte aligned, or ``None`` (bilinear); no autograd on either."""
    if not (flow.dim() == 4 and flow.is_cuda and flow.dtype == torch.float32 and flow.is_contiguous() and 1 <= flow.shape[1] <= 8
            and flow.data_ptr() % 16 == 0 and not needs_autograd(flow, mask)):
        return False
    return mask is None or (mask.dim() == 4 and mask.device == flow.device and mask.dtype == torch.float32 and mask.is_contiguous()
                            and tuple(mask.shape) == (flow.shape[0], 576, flow.shape[2], flow.shape[3]) and mask.data_ptr() % 16 == 0)


def upsample_flow(flow, mask=None):
    """RAFT's x8 flow up-sampling in one launch (csrc/upsample_flow.hip), (N, C, h, w) -> (N, C, 8h, 8w) fp32.  With the
    (N, 576, h, w) mask logits of the update block (channel k * 64 + i * 8 + j): the convex combination of
    ``RAFTBase.upsample_flow`` — softmax over the 9 taps k, zero-padded 3x3 neighbours of ``8 * flow``.  With ``mask=None``:
    ``8 * F.interpolate(flow, scale 8, mode="bilinear", align_corners=True)`` (``upflow8``).  Forward only."""
    _no_autograd("upsample_flow", flow, mask)
    if not upsample_flow_supported(flow, mask):
        raise RuntimeError("upsample_flow: needs a contiguous fp32 CUDA flow (N, C, h, w) with 1 <= C <= 8 and a contiguous fp32 mask "
                           "(N, 576, h, w) or None, both 16-byte aligned, no autograd")
    n, c_, h, w_ = flow.shape
    out = torch.empty((n, c_, 8 * h, 8 * w_), dtype=flow.dtype, device=flow.device)
    if out.numel():
        nbytes = 4.0 * (flow.numel() + out.numel() + (0 if mask is None else mask.numel()))
        _launch("alo_upsample_add_nhwc", flow.device, "upsample_flow", nbytes, 0.0, flow, mask, out, n, 1, c_, h, w_, 8 * h, 8 * w_, ALO_F32)
    return out


ALO_UPSAMPLE_GRAD = 0x100   # include/alo_hotpath.h: OR-ed into alo_upsample_add_nhwc's dtype (ALO_F32): the convex mode's backward


def _upsample_flow_operands_ok(flow, mask):
    return (flow.dim() == 4 and flow.is_cuda and flow.dtype == torch.float32 and flow.is_contiguous() and 1 <= flow.shape[1] <= 8
            and flow.data_ptr() % 16 == 0 and mask is not None and mask.dim() == 4 and mask.device == flow.device
            and mask.dtype == torch.float32 and mask.is_contiguous()
            and tuple(mask.shape) == (flow.shape[0], 576, flow.shape[2], flow.shape[3]) and mask.data_ptr() % 16 == 0)


def upsample_flow_autograd_supported(flow, mask):
    """``upsample_flow_autograd`` covers what ``upsample_flow`` covers in its convex mode, whether or not autograd records: a
    contiguous fp32 CUDA flow (N, C, h, w) with 1 <= C <= 8 and a contiguous fp32 mask (N, 576, h, w) on the same device, both
    16-byte aligned.  The mask is required: the bilinear mode has no fused backward."""
    return _upsample_flow_operands_ok(flow, mask)


def upsample_flow_grad(flow, mask, grad_up):
    """The backward of ``upsample_flow(flow, mask)`` (convex mode) in one launch (csrc/upsample_flow.hip, ALO_UPSAMPLE_GRAD):
    ``grad_up`` (N, C, 8h, 8w) -> ``(grad_flow (N, C, h, w), grad_mask (N, 576, h, w))``.  No atomics: the same bits on every run.
    ``grad_up`` may be any fp32 view (expanded, strided): it is copied once into the launch's input buffer, behind the flow.  The
    kernel writes ``grad_mask`` and, per coarse pixel, the nine tap sums of every channel (the columns of ``F.unfold``'s adjoint);
    ``F.fold`` of those, a tensor 1 / 32 of the mask's size, is ``grad_flow``.  The results are views of one buffer."""
    if not _upsample_flow_operands_ok(flow, mask):
        raise RuntimeError("upsample_flow_grad: needs a contiguous fp32 CUDA flow (N, C, h, w) with 1 <= C <= 8 and a contiguous fp32 "
                           "mask (N, 576, h, w), both 16-byte aligned")
    n, c_, h, w_ = flow.shape
    if not (grad_up.dtype == torch.float32 and grad_up.device == flow.device and tuple(grad_up.shape) == (n, c_, 8 * h, 8 * w_)):
        raise RuntimeError(f"upsample_flow_grad: grad_up must be fp32 ({n}, {c_}, {8 * h}, {8 * w_}) on {flow.device}, got "
                           f"{tuple(grad_up.shape)} {grad_up.dtype} on {grad_up.device}")
    nf = flow.numel()
    start = (nf + 3) // 4 * 4
    packed = torch.empty((start + 64 * nf,), dtype=torch.float32, device=flow.device)
    out = torch.empty((n * (576 + 9 * c_) * h * w_,), dtype=torch.float32, device=flow.device)
    grad_mask = out[:mask.numel()].view(mask.shape)
    taps = out[mask.numel():].view(n, 9 * c_, h * w_)
    if nf:
        with torch.no_grad():
            packed[:nf].copy_(flow.detach().reshape(-1))
            packed[nf:start].zero_()
            packed[start:].view(grad_up.shape).copy_(grad_up.detach())
        nbytes = 4.0 * (packed.numel() + mask.numel() + out.numel())
        _launch("alo_upsample_add_nhwc", flow.device, "upsample_flow_grad", nbytes, 0.0, packed, mask.detach(), out, n, 1, c_, h, w_,
                8 * h, 8 * w_, ALO_F32 | ALO_UPSAMPLE_GRAD)
    with torch.no_grad():
        grad_flow = torch.nn.functional.fold(taps, (h, w_), 3, padding=1) if nf else torch.zeros_like(flow)
    return grad_flow, grad_mask


class _UpsampleFlow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask):
        ctx.save_for_backward(flow, mask)
        return upsample_flow(flow, mask)       # grad mode is off in here

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_up):
        flow, mask = ctx.saved_tensors
        grad_flow, grad_mask = upsample_flow_grad(flow, mask, grad_up)
        return (grad_flow if ctx.needs_input_grad[0] else None), (grad_mask if ctx.needs_input_grad[1] else None)


def upsample_flow_autograd(flow, mask):
    """``upsample_flow(flow, mask)`` (convex mode) that autograd can differentiate once: the forward is that launch, the backward
    ``upsample_flow_grad``.  An input that does not require grad gets ``None``."""
    if not upsample_flow_autograd_supported(flow, mask):
        raise RuntimeError("upsample_flow_autograd: needs a contiguous fp32 CUDA flow (N, C, h, w) with 1 <= C <= 8 and a contiguous "
                           "fp32 mask (N, 576, h, w), both 16-byte aligned")
    return _UpsampleFlow.apply(flow, mask)


def groupnorm_rows(x, weight, bias, groups, eps=1e-5, out=None):
    """``F.group_norm`` over channels-last rows: x (B, HW, C) contiguous -> out (B, HW, C), which may be a slice
    ``flat[:, start:start + HW]`` of a larger (B, S, C) buffer (rows contiguous, any batch stride)."""
    _no_autograd("groupnorm_rows", x, weight, bias, out)
    if not groupnorm_rows_supported(x, weight, groups):
        raise RuntimeError("groupnorm_rows: needs bf16 CUDA rows (B, HW, C) with C / 8 and groups dividing 256, no autograd")
    x = x.contiguous()
    b_, hw, c_ = x.shape
    if out is None:
        out = torch.empty_like(x)
    if tuple(out.shape) != (b_, hw, c_) or out.dtype != x.dtype or out.stride(2) != 1 or out.stride(1) != c_:
        raise RuntimeError("groupnorm_rows: out must be (B, HW, C) of the input's dtype with contiguous rows")
    if b_ and hw:
        nbytes = lib().alo_groupnorm_rows_workspace_bytes(b_, hw, groups)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        _launch("alo_groupnorm_rows", x.device, f"groupnorm_rows/HW={hw}", 6.0 * x.numel(), 0.0, x, weight.contiguous(), bias.contiguous(),
                out, ws, b_, hw, c_, groups, float(eps), out.stride(0) if b_ > 1 else hw * c_, ALO_BF16)
    return out


def _host_shapes(shapes):
    flat = [int(v) for hw in shapes for v in hw]
    return (ctypes.c_int * len(flat))(*flat), len(flat) // 2


def mask_pyramid(frame_mask, shapes, nearest_levels=()):
    """Padding mask of every level + valid ratios from the frame mask, in two small kernels.

    frame_mask: (B, H, W) or (B, 1, H, W), float32 or bool / uint8, non-zero on padding.  shapes: [(h_l, w_l)].  Level l is
    resized like ``F.interpolate(mask.float(), (h_l, w_l), mode="bilinear", align_corners=False) != 0``, or with
    ``mode="nearest"`` for l in ``nearest_levels``.  Returns (mask_flat (B, S) bool, valid_ratios (B, L, 2) float32 as (w, h))."""
    if frame_mask.dim() == 4:
        frame_mask = frame_mask[:, 0]
    if not frame_mask.is_cuda or frame_mask.dim() != 3:
        raise RuntimeError("mask_pyramid: needs a CUDA (B, H, W) or (B, 1, H, W) mask")
    if frame_mask.dtype not in (torch.float32, torch.bool, torch.uint8):
        frame_mask = frame_mask != 0
    frame_mask = frame_mask.contiguous()
    b_, h, w_ = frame_mask.shape
    arr, L = _host_shapes(shapes)
    S = sum(int(a) * int(b) for a, b in shapes)
    mask_flat = torch.empty((b_, S), dtype=torch.uint8, device=frame_mask.device)
    ratios = torch.empty((b_, L, 2), dtype=torch.float32, device=frame_mask.device)
    bits = 0
    for l in nearest_levels:
        bits |= 1 << int(l)
    _launch("alo_mask_pyramid", frame_mask.device, "mask_pyramid", float(frame_mask.numel() + mask_flat.numel()), 0.0, frame_mask,
            1 if frame_mask.dtype == torch.float32 else 0, mask_flat, ratios, b_, h, w_, L, arr, bits)
    return mask_flat.view(torch.bool), ratios


def encoder_reference_points(valid_ratios, shapes):
    """(B, S, L, 2) float32 reference points of the encoder (pixel centres over the valid extent) in one kernel."""
    if not valid_ratios.is_cuda or valid_ratios.dtype != torch.float32 or valid_ratios.dim() != 3 or valid_ratios.shape[2] != 2:
        raise RuntimeError("encoder_reference_points: needs CUDA float32 valid ratios of shape (B, L, 2)")
    valid_ratios = valid_ratios.contiguous()
    arr, L = _host_shapes(shapes)
    if L != valid_ratios.shape[1]:
        raise RuntimeError("encoder_reference_points: one (h, w) per level of valid_ratios")
    S = sum(int(a) * int(b) for a, b in shapes)
    out = torch.empty((valid_ratios.shape[0], S, L, 2), dtype=torch.float32, device=valid_ratios.device)
    _launch("alo_encoder_reference_points", valid_ratios.device, "encoder_reference_points", 4.0 * out.numel(), 0.0, valid_ratios, out,
            valid_ratios.shape[0], L, arr)
    return out


def value_proj_head_major_supported(x, weight, heads, f16=False):
    return (linear_shortk_supported(x, weight, f16) and heads % 2 == 0 and weight.shape[0] == heads * 32 and x.dim() == 3)


def value_proj_head_major(x, weight, bias, padding_mask, heads):
    """``value_proj`` + ``masked_fill(padding_mask, 0)`` + head-major layout in one kernel: x (N, S, K) bf16 / fp16 ->
    (N, heads, S, 32) for ``msda_forward_fused_hm``."""
    _no_autograd("value_proj_head_major", x, weight, bias)
    if not value_proj_head_major_supported(x, weight, heads, f16=True):
        raise RuntimeError("value_proj_head_major: needs bf16 / fp16 (N, S, K) input, K in (64, 128, 256), head dimension 32")
    if bias is not None and bias.dtype != x.dtype:
        raise RuntimeError("value_proj_head_major: bias must have the dtype of x")
    N, S, K = x.shape
    x = x if x.is_contiguous() else x.contiguous()
    if padding_mask is not None:
        if padding_mask.dtype != torch.bool or tuple(padding_mask.shape) != (N, S):
            raise RuntimeError("padding_mask must be a (N, S) bool tensor")
        padding_mask = padding_mask.contiguous()
    out = torch.empty((N, heads, S, 32), dtype=x.dtype, device=x.device)
    _launch("alo_value_proj_head_major", x.device, f"value_proj_hm/S={S}", 2.0 * (x.numel() + out.numel()), 2.0 * N * S * heads * 32 * K,
            x, weight.contiguous(), None if bias is None else bias.contiguous(), padding_mask, out, N, S, heads, K, _DTYPE_CODE[x.dtype])
    return out


# ---- the encoder layer's row-local chain in one kernel (include/alo_encoder_block.h) -------------------------------------------------
def encoder_block_enabled():
    """``ALO_ENC_BLOCK=off`` (read per call) keeps the encoder on its separate launches: for tests and profiling."""
    return os.environ.get("ALO_ENC_BLOCK", "on").lower() not in ("off", "0")


# The LDS frames of csrc/encoder_block.hip against alo::launch's limit (kLdsLimit of csrc/common.hpp; kTileStride of
# csrc/mfma_tile.hpp: a 256-wide bf16 row plus 16 bytes).  Behind its tiles a kernel keeps b1 (one fp32 per hidden unit) and its
# other biases and LayerNorm vectors as fp32 tables, so the widest hidden layer a form takes follows from its tiles and tables.
BLOCK_LDS_LIMIT = 160 * 1024
BLOCK_TILE_STRIDE = 256 * 2 + 16
ENCODER_BLOCK_TABLES = 256 * 7 + 384          # b2, bo, bv, two LayerNorms' gamma / beta; bq over the merged 384 columns
DECODER_BLOCK_TABLES = 256 * 7 + 512          # chain B: bo, bv, b2, two LayerNorms' gamma / beta; bqk over 512 columns


def encoder_block_lds_bytes(hidden):
    """Dynamic LDS of encoder_block_kernel: two 64-row tiles, b1 and the tables."""
    return 2 * 64 * BLOCK_TILE_STRIDE + 4 * (hidden + ENCODER_BLOCK_TABLES)


def decoder_block_lds_bytes(hidden, tile_rows):
    """Dynamic LDS of chain B (decoder_block_kernel<tile_rows, true>): four tiles, b1 and the tables.  Chain A has no hidden layer
    and fits at both heights."""
    return 4 * tile_rows * BLOCK_TILE_STRIDE + 4 * (hidden + DECODER_BLOCK_TABLES)


def encoder_block_supported(src, w1, w2, *vectors, heads=8, levels=4, points=4, value_weight=None):
    """What :func:`encoder_block` takes: a bf16 CUDA (N, S, 256) ``src`` outside autograd (:func:`fusable`), FFN weights
    :func:`ffn256` takes with a hidden width whose LDS frame fits (:func:`encoder_block_lds_bytes`: up to 21888), 8 heads and
    L = P = 4, a value projection :func:`value_proj_head_major` takes (when the next layer's projections are asked for) and every
    bias / LayerNorm vector in ``vectors`` present."""
    if not (fusable(src, w1, w2, value_weight, *vectors) and src.dtype == torch.bfloat16 and src.dim() == 3 and src.shape[-1] == 256
            and src.numel() > 0 and ffn256_supported(src, w1, w2) and encoder_block_lds_bytes(w1.shape[0]) <= BLOCK_LDS_LIMIT
            and heads == 8 and levels == 4 and points == 4 and all(v is not None for v in vectors)):
        return False
    return value_weight is None or value_proj_head_major_supported(src, value_weight, heads)


def _vec(t, dtype):
    return t.to(dtype).contiguous()


def encoder_block(src, w1, b1, w2, b2, norm2, tail=None, nxt=None):
    """The row-local part of an encoder layer in one kernel, bit for bit the chain of launches it stands in for.

    ``src`` (N, S, 256) bf16; ``norm2 = (weight, bias, eps)``: ``src' = LayerNorm2(ffn256(x) + x)`` with ``x = src``, or with
    ``tail = (attn_out, wo, bo, norm1_weight, norm1_bias, eps1)``, ``x = LayerNorm1(linear(attn_out, wo, bo) + src)``.
    With ``nxt = (pos, padding_mask | None, wv, bv, wq, bq)`` also the next layer's ``value_proj_head_major(src', wv, bv,
    padding_mask, 8)`` and ``linear(src' + pos, wq, bq)`` for the merged (384, 256) offsets + logits weight.
    -> (src', value_hm | None, offsets_logits | None)"""
    _no_autograd("encoder_block", src, w1, b1, w2, b2, *norm2[:2], *(tail or ())[:5], *(nxt or ()))
    if not encoder_block_supported(src, w1, w2, b1, b2, norm2[0], norm2[1]):
        raise RuntimeError("encoder_block: needs a bf16 CUDA (N, S, 256) src outside autograd, bf16 FFN weights with a hidden width "
                           "that is a multiple of 256 and whose LDS frame fits (up to 21888), and every bias")
    N, S, C = src.shape
    dt, dev = src.dtype, src.device
    src = src.contiguous()
    Fh = w1.shape[0]
    out = torch.empty_like(src)
    named = [("w1", w1, (Fh, 256)), ("w2", w2, (256, Fh))]
    t_args = [None] * 5
    eps1 = 0.0
    if tail is not None:
        attn_out, wo, bo, g1, e1, eps1 = tail
        if attn_out.shape != src.shape or attn_out.dtype != dt or attn_out.device != dev:
            raise RuntimeError("encoder_block: attn_out must have the shape, dtype and device of src")
        named.append(("wo", wo, (256, 256)))
        attn_out = attn_out.contiguous()
        t_args = [attn_out, pack_mfma_b(wo), _vec(bo, dt), _vec(g1, dt), _vec(e1, dt)]
    n_args = [None] * 8
    value = both = None
    if nxt is not None:
        pos, padding_mask, wv, bv, wq, bq = nxt
        if pos.shape != src.shape or pos.dtype != dt or pos.device != dev:
            raise RuntimeError("encoder_block: pos must have the shape, dtype and device of src")
        if padding_mask is not None:
            if padding_mask.dtype != torch.bool or tuple(padding_mask.shape) != (N, S) or padding_mask.device != dev:
                raise RuntimeError("padding_mask must be a (N, S) bool tensor on src's device")
            padding_mask = padding_mask.contiguous()
        named += [("wv", wv, (256, 256)), ("wq", wq, (384, 256))]
        value = torch.empty((N, 8, S, 32), dtype=dt, device=dev)
        both = torch.empty((N, S, 384), dtype=dt, device=dev)
        n_args = [pos.contiguous(), padding_mask, pack_mfma_b(wv), _vec(bv, dt), pack_mfma_b(wq), _vec(bq, dt), value, both]
    for name, w, shape in named:
        if tuple(w.shape) != shape or w.dtype != dt or w.device != dev:
            raise RuntimeError(f"encoder_block: {name} must be a {shape} tensor of src's dtype on its device")
    f_args = [src, pack_mfma_b(w1), _vec(b1, dt), pack_mfma_b(w2), _vec(b2, dt), _vec(norm2[0], dt), _vec(norm2[1], dt), out]
    rows = N * S
    # what the result needs: src, src' (+ attn_out) (+ pos, value, offsets + logits, mask bytes)
    nbytes = 2.0 * rows * (256 * (2 + (tail is not None) + 2 * (nxt is not None)) + 384 * (nxt is not None)) + rows * (nxt is not None)
    flops = 2.0 * rows * 256 * (2 * Fh + 256 * (tail is not None) + (256 + 384) * (nxt is not None))
    tag = f"encoder_block/{'tail+' if tail is not None else ''}ffn{'+proj' if nxt is not None else ''}/rows={rows}"
    _launch("alo_encoder_block", dev, tag, nbytes, flops, *t_args, *f_args, *n_args, N, S, Fh, float(eps1), float(norm2[2]), ALO_BF16)
    return out, value, both


# ---- the decoder layer's two row-local chains on the same entry point (ALO_BLOCK_* of include/alo_encoder_block.h) ------------------
ALO_BLOCK_NO_FFN, ALO_BLOCK_DECODER_NEXT, ALO_BLOCK_TILE_32, ALO_BLOCK_TILE_64 = 0x100, 0x200, 0x400, 0x800   # OR-ed into the dtype


def decoder_block_enabled():
    """``ALO_DEC_BLOCK=off`` (read per call) keeps the decoder on its separate launches: for tests and profiling."""
    return os.environ.get("ALO_DEC_BLOCK", "on").lower() not in ("off", "0")


def decoder_block_supported(tgt, *operands, hidden=None):
    """What :func:`decoder_block_a` / :func:`decoder_block_b` take: a bf16 CUDA (N, Lq, 256) ``tgt`` outside autograd and every
    tensor in ``operands`` (weights, biases, LayerNorm vectors, ``query_pos``) present, bf16 and on its device.  ``hidden``: chain
    B's hidden width; its LDS frame must fit at the 32-row height (:func:`decoder_block_lds_bytes`: up to 21760)."""
    return (all(t is not None for t in operands) and fusable(tgt, *operands) and tgt.dtype == torch.bfloat16 and tgt.dim() == 3
            and tgt.shape[-1] == 256 and tgt.numel() > 0
            and all(t.dtype == tgt.dtype and t.device == tgt.device for t in operands)
            and (hidden is None or decoder_block_lds_bytes(hidden, 32) <= BLOCK_LDS_LIMIT))


# The fewest rows (batch x queries) the decoder takes the fused chains at: the smallest count tools/decbench.py timed them against
# the separate launches (docs/experiments.md); below it the layers keep their separate launches.
DECODER_BLOCK_MIN_ROWS = 300


def decoder_block_routed(tgt):
    """Whether a decoder over ``tgt`` (N, Lq, 256) is sent through the fused chains: ``ALO_DEC_BLOCK`` and the measured row range."""
    return decoder_block_enabled() and tgt.dim() == 3 and tgt.shape[0] * tgt.shape[1] >= DECODER_BLOCK_MIN_ROWS


_CU_COUNT = {}


def decoder_block_tile_rows(rows, device, hidden=0):
    """The tile height the decoder chains run at (the rule of include/alo_encoder_block.h): 32 rows while 64-row tiles would leave
    compute units without work or, with chain B's ``hidden`` width, while their LDS frame does not fit; else 64."""
    if decoder_block_lds_bytes(hidden, 64) > BLOCK_LDS_LIMIT:
        return 32
    index = torch.device(device).index
    index = torch.cuda.current_device() if index is None else index
    if index not in _CU_COUNT:
        _CU_COUNT[index] = torch.cuda.get_device_properties(index).multi_processor_count
    return 32 if (rows + 63) // 64 < _CU_COUNT[index] else 64


def _decoder_block(name, flag, attn_out, tgt, pos, tail, ffn, nxt, tile_rows):
    """One flagged launch: ``tail = (wo, bo, g1, e1, eps1)``, ``ffn = (w1, b1, w2, b2, g2, e2, eps2) | None``,
    ``nxt = (wv, bv) | None`` and the query projection ``(wq, bq)`` -> (out, value | None, projected query)."""
    wo, bo, g1, e1, eps1 = tail
    N, L, C = tgt.shape
    dt, dev, rows = tgt.dtype, tgt.device, N * L
    for label, t in (("attn_out", attn_out), ("pos", pos)):
        if t.shape != tgt.shape or t.dtype != dt or t.device != dev:
            raise RuntimeError(f"{name}: {label} must have the shape, dtype and device of tgt")
    (wq, bq), qc = nxt[2:], (512 if ffn is not None else 384)
    named = [("wo", wo, (256, 256)), ("wq", wq, (qc, 256))]
    f_args, v_args, value, eps2, Fh = [None] * 6, [None, None], None, 0.0, 0
    if ffn is not None:
        w1, b1, w2, b2, g2, e2, eps2 = ffn
        Fh = w1.shape[0]
        if not ffn256_supported(tgt, w1, w2):
            raise RuntimeError(f"{name}: needs bf16 FFN weights with a hidden width that is a multiple of 256")
        named += [("w1", w1, (Fh, 256)), ("w2", w2, (256, Fh)), ("wv", nxt[0], (256, 256))]
        f_args = [pack_mfma_b(w1), _vec(b1, dt), pack_mfma_b(w2), _vec(b2, dt), _vec(g2, dt), _vec(e2, dt)]
        v_args = [pack_mfma_b(nxt[0]), _vec(nxt[1], dt)]
        value = torch.empty((N, L, 256), dtype=dt, device=dev)
    for label, w, shape in named:
        if tuple(w.shape) != shape or w.dtype != dt or w.device != dev:
            raise RuntimeError(f"{name}: {label} must be a {shape} tensor of tgt's dtype on its device")
    if tile_rows not in (None, 32, 64):
        raise RuntimeError(f"{name}: tile_rows must be 32, 64 or None")
    tile_rows = tile_rows or decoder_block_tile_rows(rows, dev, Fh)
    out = torch.empty_like(tgt, memory_format=torch.contiguous_format)
    query = torch.empty((N, L, qc), dtype=dt, device=dev)
    nbytes = 2.0 * rows * (256 * (4 + (ffn is not None)) + qc)   # attn_out, tgt, pos, out (+ value), the projected query
    flops = 2.0 * rows * 256 * (256 + qc + (2 * Fh + 256) * (ffn is not None))
    _launch("alo_encoder_block", dev, f"{name}/rows={rows}/tile={tile_rows}", nbytes, flops,
            attn_out.contiguous(), pack_mfma_b(wo), _vec(bo, dt), _vec(g1, dt), _vec(e1, dt), tgt.contiguous(), *f_args, out,
            pos.contiguous(), None, *v_args, pack_mfma_b(wq), _vec(bq, dt), value, query, N, L, Fh, float(eps1), float(eps2),
            ALO_BF16 | flag | (ALO_BLOCK_TILE_32 if tile_rows == 32 else ALO_BLOCK_TILE_64))
    return out, value, query


def decoder_block_a(attn_out, tgt, pos, wo, bo, norm, wq, bq, tile_rows=None):
    """Chain A of a decoder layer, between self-attention and the MSDA launch, in one kernel and bit for bit the launches it stands
    in for: ``tgt1 = LayerNorm(linear(attn_out, wo, bo) + tgt)`` with ``norm = (weight, bias, eps)`` and
    ``linear(tgt1 + pos, wq, bq)`` for the merged (384, 256) offsets + logits weight.  All of (N, Lq, 256) bf16.
    ``tile_rows``: 32 or 64 instead of :func:`decoder_block_tile_rows`.  -> (tgt1, offsets_logits (N, Lq, 384))"""
    _no_autograd("decoder_block_a", attn_out, tgt, pos, wo, bo, *norm[:2], wq, bq)
    if not decoder_block_supported(tgt, attn_out, pos, wo, bo, norm[0], norm[1], wq, bq):
        raise RuntimeError("decoder_block_a: needs bf16 CUDA (N, Lq, 256) tensors outside autograd and every weight, bias and pos")
    out, _, both = _decoder_block("decoder_block_a", ALO_BLOCK_NO_FFN, attn_out, tgt, pos, (wo, bo, *norm), None,
                                  (None, None, wq, bq), tile_rows)
    return out, both


def decoder_block_b(attn_out, tgt1, pos, wo, bo, norm1, w1, b1, w2, b2, norm3, wv, bv, wqk, bqk, tile_rows=None):
    """Chain B of a decoder layer, between the MSDA launch and the NEXT layer's self-attention:
    ``tgt2 = LayerNorm1(linear(attn_out, wo, bo) + tgt1)``, ``out = LayerNorm3(ffn256(tgt2) + tgt2)``, and the next layer's
    ``v = linear(out, wv, bv)`` (row-major, as ``linear_auto`` writes it) and ``qk = linear(out + pos, wqk, bqk)`` with the
    (512, 256) [q; k] rows of its ``in_proj_weight``.  -> (out, v (N, Lq, 256), qk (N, Lq, 512))"""
    _no_autograd("decoder_block_b", attn_out, tgt1, pos, wo, bo, *norm1[:2], w1, b1, w2, b2, *norm3[:2], wv, bv, wqk, bqk)
    if not decoder_block_supported(tgt1, attn_out, pos, wo, bo, norm1[0], norm1[1], w1, b1, w2, b2, norm3[0], norm3[1], wv, bv, wqk, bqk,
                                   hidden=None if w1 is None else w1.shape[0]):
        raise RuntimeError("decoder_block_b: needs bf16 CUDA (N, Lq, 256) tensors outside autograd, every weight, bias and pos, and "
                           "a hidden width whose LDS frame fits (up to 21760)")
    return _decoder_block("decoder_block_b", ALO_BLOCK_DECODER_NEXT, attn_out, tgt1, pos, (wo, bo, *norm1), (w1, b1, w2, b2, *norm3),
                          (wv, bv, wqk, bqk), tile_rows)


# ---- dense multi-head attention (ALO_BLOCK_ATTENTION of include/alo_encoder_block.h, csrc/attention.hip) ------------------------------
ALO_BLOCK_ATTENTION, ALO_BLOCK_PACKED_QK = 0x2000, 0x8000   # OR-ed into alo_encoder_block's dtype
ATTENTION_HEADS, ATTENTION_HEAD_DIM = 8, 32                 # the header's fixed geometry: d_model = 256


def attention_routed():
    """``ALO_ATTENTION=fused`` (read per call, opt-in) sends the dense attention of the Deformable-DETR decoder and of DETR's
    transformer through :func:`attention`; unset, both keep the stock ops."""
    return os.environ.get("ALO_ATTENTION", "").lower() == "fused"


def _attention_packed(q, k):
    """Whether q and k are the two 256-column halves of one contiguous (B, L, 512) tensor: chain B's [q; k] matrix, read in place."""
    return (q.shape == k.shape and q.stride() == k.stride() == (q.shape[1] * 512, 512, 1)
            and k.data_ptr() == q.data_ptr() + 256 * q.element_size())


def attention_supported(q, k, v, key_padding_mask=None):
    """What :func:`attention` takes: CUDA bf16 / fp16 / fp32 tensors outside autograd, q (B, Lq, 256), k and v (B, Lk, 256) with
    Lq, Lk > 0, one dtype and device, 16-byte aligned; q and k contiguous or the halves of one (B, L, 512) tensor; a (B, Lk) bool or
    uint8 mask or none; every operand below 2 GiB."""
    if not (q.dim() == k.dim() == v.dim() == 3 and fusable(q, k, v, f16=True)):
        return False
    B, Lq, E = q.shape
    Lk = k.shape[1]
    if not (E == ATTENTION_HEADS * ATTENTION_HEAD_DIM and k.shape == v.shape == (B, Lk, E) and B > 0 and Lq > 0 and Lk > 0):
        return False
    if not all(t.dtype == q.dtype and t.device == q.device and t.data_ptr() % 16 == 0 for t in (k, v)) or q.data_ptr() % 16:
        return False
    if not ((q.is_contiguous() and k.is_contiguous()) or _attention_packed(q, k)):
        return False
    if key_padding_mask is not None and not (key_padding_mask.shape == (B, Lk) and key_padding_mask.device == q.device
                                             and key_padding_mask.dtype in (torch.bool, torch.uint8)):
        return False
    return B * max(Lq, Lk) * 512 * q.element_size() < 2 ** 31


def attention(q, k, v, key_padding_mask=None):
    """``softmax(q k^T / sqrt(32) + mask) v`` over 8 heads of 32 channels in one kernel, on batch-first tensors as the projections
    write them (head h = columns 32 h .. 32 h + 31): no head-major reshapes.  q (B, Lq, 256), k and v (B, Lk, 256), bf16 / fp16 /
    fp32; q and k may be the two halves ``qk[..., :256]`` / ``qk[..., 256:]`` of one (B, L, 512) tensor, which is then read in place.
    ``key_padding_mask`` (B, Lk) bool / uint8: non-zero keys are ignored; a query with every key masked gets NaN, as
    ``nn.MultiheadAttention`` gives.  -> (B, Lq, 256), before the output projection."""
    _no_autograd("attention", q, k, v)
    if not attention_supported(q, k, v, key_padding_mask):
        raise RuntimeError("attention: needs CUDA bf16 / fp16 / fp32 (B, Lq, 256) q and (B, Lk, 256) k, v of one dtype outside autograd, "
                           "q and k contiguous or the halves of one (B, L, 512) tensor, and a (B, Lk) bool / uint8 mask or none")
    B, Lq, E = q.shape
    Lk = k.shape[1]
    packed = not (q.is_contiguous() and k.is_contiguous())
    v = v.contiguous()
    mask = None
    if key_padding_mask is not None:
        mask = key_padding_mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = torch.empty((B, Lq, E), dtype=q.dtype, device=q.device)
    es = q.element_size()
    nbytes = es * E * B * (2.0 * Lq + 2.0 * Lk) + (0 if mask is None else B * Lk)
    flops = 4.0 * B * Lq * Lk * E
    _launch("alo_encoder_block", q.device, f"attention/Lq={Lq}/Lk={Lk}", nbytes, flops,
            v, None, None, None, None, q, None, None, None, None, None, None, out, k, mask, None, None, None, None, None, None,
            B, Lq, Lk, ATTENTION_HEAD_DIM ** -0.5, 0.0,
            _DTYPE_CODE[q.dtype] | ALO_BLOCK_ATTENTION | (ALO_BLOCK_PACKED_QK if packed else 0))
    return out


def panoptic_onehot(mask_logits, frame_size, threshold=0.5):
    """(B, Q, h, w) mask logits -> (B, Q, H, W) int64 one-hot instance masks: bilinear up-sampling, sigmoid, threshold and the
    per-pixel arg-max over the queries in one pass (PanopticHead.inference).  A NaN probability selects its query (the first one
    if there are several), as ``F.threshold`` (which keeps NaN) followed by ``argmax`` (for which NaN is the maximum) does."""
    if not mask_logits.is_cuda or mask_logits.dim() != 4:
        raise RuntimeError("panoptic_onehot: needs CUDA (B, Q, h, w) logits")
    x = mask_logits.float().contiguous()
    b_, q, h, w_ = x.shape
    H, W = int(frame_size[0]), int(frame_size[1])
    out = torch.empty((b_, q, H, W), dtype=torch.long, device=x.device)
    if out.numel():
        _launch("alo_panoptic_onehot", x.device, "panoptic_onehot", 8.0 * out.numel(), 0.0, x, out, b_, q, h, w_, H, W, float(threshold))
    return out


# ---- two-stage Deformable-DETR: proposals, row masking, decoder queries (include/alo_two_stage.h) ---------------------------------
def encoder_proposals_supported(mask_flatten, shapes):
    """CUDA, contiguous (B, S) bool / uint8 mask of fewer than 2^31 tokens over at most 8 non-empty levels.  (The mask carries no
    gradient; whether the caller's other tensors do is the caller's question: :func:`fusable`.)"""
    return (mask_flatten.is_cuda and mask_flatten.dim() == 2 and mask_flatten.dtype in (torch.bool, torch.uint8)
            and mask_flatten.is_contiguous() and 0 < len(shapes) <= 8 and mask_flatten.shape[0] > 0 and mask_flatten.numel() < 2 ** 31
            and all(int(h) > 0 and int(w) > 0 for h, w in shapes)
            and sum(int(h) * int(w) for h, w in shapes) == mask_flatten.shape[1])


def encoder_proposals(mask_flatten, shapes):
    """Box proposal of every encoder token in one kernel -> (proposals (B, S, 4) float32: inverse sigmoid of (cx, cy, w, h),
    +inf where the token is dropped; keep (B, S) bool).  Equals ``encoder_output_proposals`` of
    alonet.deformable_detr.deformable_transformer in float32: same ``keep``, same +inf pattern."""
    if not encoder_proposals_supported(mask_flatten, shapes):
        raise RuntimeError("encoder_proposals: needs a contiguous CUDA (B, S) bool / uint8 mask and 1..8 non-empty levels whose sizes sum to S")
    B, S = mask_flatten.shape
    arr, L = _host_shapes(shapes)
    proposals = torch.empty((B, S, 4), dtype=torch.float32, device=mask_flatten.device)
    keep = torch.empty((B, S), dtype=torch.uint8, device=mask_flatten.device)
    _launch("alo_encoder_proposals", mask_flatten.device, f"encoder_proposals/S={S}", 18.0 * B * S, 0.0, mask_flatten, proposals, keep,
            B, L, arr)
    return proposals, keep.view(torch.bool)


def encoder_proposals_masked_supported(mask_flatten, shapes, memory, f16=False):
    """What :func:`encoder_proposals` needs of the mask and :func:`mask_rows` of the rows, for memory (B, S, C) on the mask's device."""
    return (encoder_proposals_supported(mask_flatten, shapes) and memory.dim() == 3 and memory.device == mask_flatten.device
            and tuple(memory.shape[:2]) == tuple(mask_flatten.shape) and mask_rows_supported(memory, mask_flatten, f16))


def encoder_proposals_masked(mask_flatten, shapes, memory):
    """:func:`encoder_proposals` and :func:`mask_rows` in one launch -> (proposals, keep, memory with the dropped rows zeroed):
    0.026 against 0.029 ms for the two launches at the headline size (docs/experiments.md)."""
    _no_autograd("encoder_proposals_masked", memory)
    if not encoder_proposals_masked_supported(mask_flatten, shapes, memory, f16=True):
        raise RuntimeError("encoder_proposals_masked: needs what encoder_proposals and mask_rows need, memory (B, S, C) on the mask's device")
    B, S = mask_flatten.shape
    arr, L = _host_shapes(shapes)
    proposals = torch.empty((B, S, 4), dtype=torch.float32, device=mask_flatten.device)
    keep = torch.empty((B, S), dtype=torch.uint8, device=mask_flatten.device)
    out = torch.empty_like(memory)
    _launch("alo_encoder_proposals_masked", memory.device, f"encoder_proposals_masked/S={S}",
            2.0 * memory.element_size() * memory.numel() + 18.0 * B * S, 0.0, mask_flatten, proposals, keep, memory, out, B, L, arr,
            memory.shape[-1], _DTYPE_CODE[memory.dtype])
    return proposals, keep.view(torch.bool), out


def mask_rows_supported(memory, keep, f16=False):
    """CUDA, contiguous fp32 / bf16 (with ``f16=True``: or fp16) rows of a multiple of 8 channels, one bool / uint8 per row, 16-byte
    aligned."""
    return (memory.is_cuda and memory.dtype in (torch.float32, *_half(f16)) and memory.is_contiguous() and memory.dim() >= 2
            and memory.shape[-1] % 8 == 0 and memory.numel() > 0 and memory.data_ptr() % 16 == 0
            and keep.is_cuda and keep.dtype in (torch.bool, torch.uint8) and keep.is_contiguous()
            and tuple(keep.shape) == tuple(memory.shape[:-1]))


def mask_rows(memory, keep):
    """``memory.masked_fill(~keep[..., None], 0)`` in one pass of 16-byte vectors; dropped rows are written, not read."""
    _no_autograd("mask_rows", memory)
    if not mask_rows_supported(memory, keep, f16=True):
        raise RuntimeError("mask_rows: needs contiguous CUDA fp32 / bf16 / fp16 rows with C % 8 == 0 and one bool / uint8 `keep` per row")
    C = memory.shape[-1]
    rows = memory.numel() // C
    out = torch.empty_like(memory)
    _launch("alo_mask_rows", memory.device, f"mask_rows/rows={rows}", 2.0 * memory.element_size() * memory.numel() + rows, 0.0,
            memory, keep, out, rows, C, _DTYPE_CODE[memory.dtype])
    return out


def proposal_queries_supported(coords_unact, topk, dtype, f16=False):
    return (coords_unact.is_cuda and coords_unact.dtype == torch.float32 and coords_unact.dim() == 3 and coords_unact.shape[2] == 4
            and coords_unact.is_contiguous() and coords_unact.numel() > 0 and coords_unact.data_ptr() % 16 == 0
            and topk.is_cuda and topk.dtype == torch.int64 and topk.dim() == 2 and topk.shape[0] == coords_unact.shape[0]
            and topk.is_contiguous() and topk.numel() > 0 and dtype in (torch.float32, *_half(f16)))


def proposal_dim_t(device, owner=None):
    """(64,) float32 frequencies of the proposal embedding, ``10000 ** (k / 64)``, by the torch ops the torch formulation uses, on
    ``device``.  With ``owner`` (a weight on that device) they are kept on it with the other derived tensors (:func:`derived`)."""
    def build():
        return 10000 ** (torch.arange(64, dtype=torch.float32, device=device) / 64)
    if owner is None or owner.device != torch.device(device):
        return build()
    return derived(owner, "proposal_dim_t", (owner,), build)


def proposal_queries(coords_unact, topk, dtype, owner=None):
    """Decoder queries of the selected proposals in one kernel: coords_unact (B, S, 4) float32, topk (B, K) int64 ->
    (reference_points (B, K, 4) float32 = sigmoid of the gathered rows, embed (B, K, 512) ``dtype`` = their sine embedding,
    ``get_proposal_pos_embed``).  ``owner``: the weight the embedding feeds (``pos_trans.weight``), which keeps the 64 frequencies
    (:func:`proposal_dim_t`); without one they are computed per call."""
    _no_autograd("proposal_queries", coords_unact)
    if not proposal_queries_supported(coords_unact, topk, dtype, f16=True):
        raise RuntimeError("proposal_queries: needs contiguous CUDA (B, S, 4) float32 coordinates, (B, K) int64 indices, fp32 / bf16 / fp16 output")
    B, S, _ = coords_unact.shape
    K = topk.shape[1]
    ref = torch.empty((B, K, 4), dtype=torch.float32, device=coords_unact.device)
    embed = torch.empty((B, K, 512), dtype=dtype, device=coords_unact.device)
    dim_t = proposal_dim_t(coords_unact.device, owner)
    _launch("alo_proposal_queries", coords_unact.device, f"proposal_queries/K={K}", B * K * (8.0 + 32.0 + 512.0 * embed.element_size()),
            0.0, coords_unact, topk, dim_t, ref, embed, B, S, K, _DTYPE_CODE[dtype])
    return ref, embed
