"""fp16 values in the MSDA op, the parts that need no GPU: the dtype code, the backward dispatch and the Python pre-filter."""
import ctypes
import re

import torch

import alo_hip
from helpers import header_text

DETR_SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]   # the dispatch shapes of tests/test_cabi.py
S = sum(h * w for h, w in DETR_SHAPES)


def test_header_declares_alo_f16_as_3():
    enum = re.search(r"typedef enum alo_dtype \{(.*?)\}", header_text("alo_hotpath.h"), re.S).group(1)
    values = dict(re.findall(r"(ALO_\w+)\s*=\s*(\d+)", enum))
    assert values == {"ALO_F32": "0", "ALO_F64": "1", "ALO_BF16": "2", "ALO_F16": "3"}


def test_python_dtype_code():
    assert alo_hip.ALO_F16 == 3
    assert alo_hip._DTYPE_CODE[torch.float16] == 3
    assert alo_hip.lib().alo_abi_version() == 3   # a new value of an existing argument: the ABI number stays


def test_every_fp16_backward_is_the_generic_kernel_hinted_or_not():
    lib = alo_hip.lib()
    hint = (ctypes.c_int32 * 8)(*[v for hw in DETR_SHAPES for v in hw])
    f16, f32, f64 = alo_hip.ALO_F16, alo_hip.ALO_F32, alo_hip.ALO_F64
    path = lambda D, Lq, ldt, h, L=4, P=4: lib.alo_msda_backward_path(4, S, 8, D, L, Lq, P, f16, ldt, h)  # noqa: E731
    for D in (32, 64, 128):
        for Lq in (S, 300):
            assert path(D, Lq, f32, hint) == 0 and path(D, Lq, f32, None) == 0, (D, Lq)
    assert path(32, S, f32, hint, P=8) == 0
    assert path(32, S, f16, hint) == -1 and path(32, S, f16, None) == -1     # fp16 locations are not offered
    assert b"dtype pair" in lib.alo_last_error()
    assert path(32, S, f64, hint) == -1 and path(32, S, f64, None) == -1


def test_no_host_shapes_are_read_back_for_fp16():
    for D in (32, 64):
        dims = (4, S, 8, D, 4, S, 4)
        assert alo_hip._wide_backward_wants_host_shapes(torch.empty(0, dtype=torch.bfloat16), dims, alo_hip.ALO_F32)
        assert not alo_hip._wide_backward_wants_host_shapes(torch.empty(0, dtype=torch.float16), dims, alo_hip.ALO_F32)
