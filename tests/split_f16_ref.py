"""The two-term fp16 split of aloception-oss_amd/csrc/split_f16.hpp restated in numpy, once: the scale (``split_exponent`` of the
largest finite magnitude), the split (``split_terms``: hi, lo, a non-finite element as (0, itself)) and their per-row / per-channel
forms.  conv_f32_ref.py, linear_f32_ref.py and ffn_f32_ref.py build their kernels' arithmetic from these; the derivation of the bound
stays in conv_f32_ref.py, where the bound is."""
import numpy as np


def split_exponent(absmax):
    """split_exponent of csrc/split_f16.hpp: 2^-k absmax lands in [2^14, 2^15); 0 for zero, fp32-subnormal and non-finite values."""
    if not np.isfinite(absmax) or absmax == 0:
        return 0
    e = int(np.floor(np.log2(float(absmax))))
    if e < -126:
        return 0
    return int(np.clip(e - 14, -110, 110))


def finite_amax(a):
    mag = np.abs(a)
    mag = np.where(np.isfinite(mag), mag, 0)
    return float(mag.max()) if mag.size else 0.0


def split_terms(a32, k):
    """a 2^-k -> (hi, lo) as fp32 arrays holding fp16 values; a non-finite element -> (0, itself), as the kernel parks it."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.ldexp(a32, -k).astype(np.float32)                # exact
        hi = s.astype(np.float16).astype(np.float32)
        lo = (s - hi).astype(np.float16).astype(np.float32)     # the difference is exact in fp32, then rounded
        bad = ~np.isfinite(s)
        return np.where(bad, np.float32(0), hi), np.where(bad, s, lo)


def row_exponents(a):
    """split_exponent of every row's largest finite magnitude -> int32 (rows,)."""
    amax = np.where(np.isfinite(a), np.abs(a), 0).max(axis=1) if a.shape[1] else np.zeros(a.shape[0])
    return np.array([split_exponent(np.float32(v)) for v in amax], dtype=np.int32)


def split_weight(w):
    """(N, K) fp32 -> (hi, lo, k): what alo_hip._split_weight packs (fp32 arrays holding fp16 values; int32 exponents)."""
    k = np.array([split_exponent(np.float32(finite_amax(r))) for r in w], dtype=np.int32)
    hi, lo = split_terms(w, k[:, None])
    return hi, lo, k
