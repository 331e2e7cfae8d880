"""ALO_CONV3X3_PIPE (aloception-oss_amd/csrc/conv.hip) also chooses the kernel of a stride-2 call: unset, the pipelined stride-2 kernel;
"stride1", the streaming kernel for stride 2 alone; "off", the streaming kernels throughout.  The kernels agree bit for bit and the knob
is read after the argument checks of alo_conv3x3_nhwc.  So every refusal of a stride-2 call, with its status and its message, is the
same whatever the knob holds, and nothing is enqueued: each call here carries one bad argument and never launches.  The workspace
answer does not depend on it either, and no symbol was added for it."""
import ctypes

import pytest

import alo_hip
from helpers import HEADERS, declared_functions, exported_alo_functions

ONE = ctypes.c_void_p(16)    # never dereferenced
ODD = ctypes.c_void_p(24)    # not on a 16-byte boundary
BF16, F32 = alo_hip.ALO_BF16, alo_hip.ALO_F32
KNOBS = ("off", "stride1", "on", "", "STRIDE1", "stride2")

# (x, w_packed, bias, y, workspace, N, H, W, Cin, Cout, stride, relu, dtype): stride-2 shapes the route would take, one bad argument each
BAD = {
    "null x": (None, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 2, 1, BF16),
    "null weights": (ONE, None, ONE, ONE, None, 1, 8, 9, 256, 256, 2, 1, BF16),
    "null y": (ONE, ONE, ONE, None, None, 1, 8, 9, 256, 256, 2, 1, BF16),
    "zero width": (ONE, ONE, ONE, ONE, None, 1, 8, 0, 128, 128, 2, 0, BF16),
    "negative batch": (ONE, ONE, ONE, ONE, None, -1, 8, 9, 512, 512, 2, 0, BF16),
    "stride 4": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 4, 0, BF16),
    "Cin not a multiple of 64": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 96, 128, 2, 0, BF16),
    "Cout not a multiple of 64": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 128, 160, 2, 0, BF16),
    "fp16": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 2, 0, alo_hip.ALO_F16),
    "odd input": (ODD, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 2, 0, BF16),
    "odd output": (ONE, ONE, ONE, ODD, None, 1, 8, 9, 256, 512, 2, 0, BF16),
    "image too large": (ONE, ONE, ONE, ONE, None, 1, 1 << 12, 1 << 12, 128, 128, 2, 0, BF16),
    "five taps at stride 2": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 2 | alo_hip.ALO_CONV_TAPS_5X1, 0, F32),
    "dilated at stride 2": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 2 | alo_hip.ALO_CONV_DILATION_2, 0, BF16),
    "fp32 without a workspace": (ONE, ONE, ONE, ONE, None, 1, 8, 9, 128, 128, 2, 0, F32),
}


def _call(args):
    lib = alo_hip.lib()
    rc = lib.alo_conv3x3_nhwc(*args, None)
    return rc, lib.alo_last_error()


@pytest.mark.parametrize("name", sorted(BAD))
def test_refusals_do_not_depend_on_the_knob(name, monkeypatch):
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    unset = _call(BAD[name])
    assert unset[0] in (1, 2) and unset[1], (name, unset)     # invalid argument / unsupported, with a message
    for value in KNOBS:
        monkeypatch.setenv("ALO_CONV3X3_PIPE", value)
        assert _call(BAD[name]) == unset, (name, value)


def test_the_messages_name_the_entry_point_and_the_argument(monkeypatch):
    for value in (None, "off", "stride1"):
        if value is None:
            monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
        else:
            monkeypatch.setenv("ALO_CONV3X3_PIPE", value)
        assert _call(BAD["null x"]) == (1, b"alo_conv3x3_nhwc: null pointer argument")
        rc, msg = _call(BAD["stride 4"])
        assert rc == 2 and b"stride must be 1 or 2 (got 4)" in msg
        rc, msg = _call(BAD["Cout not a multiple of 64"])
        assert rc == 2 and b"Cin=128 Cout=160" in msg
        rc, msg = _call(BAD["odd input"])
        assert rc == 1 and b"16-byte aligned" in msg
        rc, msg = _call(BAD["image too large"])
        assert rc == 2 and b"image too large" in msg
        rc, msg = _call(BAD["dilated at stride 2"])
        assert rc == 2 and b"ALO_CONV_DILATION_2" in msg and b"stride 1 only" in msg


def test_workspace_answer_does_not_depend_on_the_knob(monkeypatch):
    lib = alo_hip.lib()
    # the headline's layer2.0 / layer3.0 / layer4.0 conv2 and its input_proj[3]
    shapes = [(8, 200, 334, 128, 128), (8, 100, 167, 256, 256), (8, 50, 84, 512, 512), (8, 25, 42, 2048, 256)]
    monkeypatch.delenv("ALO_CONV3X3_PIPE", raising=False)
    unset = [lib.alo_conv3x3_workspace_bytes(*s, 2) for s in shapes]
    assert unset[:3] == [0, 0, 0] and unset[3] > 0      # the three backbone shapes do not split K: they are the route's
    for value in KNOBS:
        monkeypatch.setenv("ALO_CONV3X3_PIPE", value)
        assert [lib.alo_conv3x3_workspace_bytes(*s, 2) for s in shapes] == unset, value


def test_no_symbol_was_added():
    declared = {name for header in HEADERS for name in declared_functions(header)}
    assert exported_alo_functions(alo_hip.LIB_PATH) == declared == set(alo_hip._SIGNATURES)
