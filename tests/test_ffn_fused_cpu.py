"""The one-launch FFN forward's knob (mmt_set_ffn_fused, env MMT_FFN_FUSED; include/mmt.h) and its op's argument
checks without a device: the setter returns the previous value, and a fresh process starts from the environment
variable (default 1)."""
import ctypes
import os
import subprocess
import sys

import pytest

import mmt_lib as ML


def test_setter_returns_previous_value():
    L = ML.lib()
    first = L.mmt_set_ffn_fused(0)
    try:
        assert first in (0, 1)
        for v in (1, 0, 1):
            L.mmt_set_ffn_fused(v)
            assert L.mmt_set_ffn_fused(v) == v
    finally:
        L.mmt_set_ffn_fused(first)


def _start_value(env_value):
    """The knob's start value in a fresh process that only loads the library (no torch, no device)."""
    code = ("import ctypes, sys\n"
            "L = ctypes.CDLL(sys.argv[1])\n"
            "f = L.mmt_set_ffn_fused; f.restype = ctypes.c_int; f.argtypes = [ctypes.c_int]\n"
            "print(f(0))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MMT_")}
    if env_value is not None:
        env["MMT_FFN_FUSED"] = env_value
    out = subprocess.run([sys.executable, "-c", code, ML.LIB_PATH], env=env, check=True, capture_output=True, text=True,
                         timeout=60).stdout
    return int(out.strip())


@pytest.mark.parametrize("env_value,expect", [(None, 1), ("0", 0), ("1", 1)])
def test_environment_sets_the_start_value(env_value, expect):
    assert _start_value(env_value) == expect


def test_symbols_declared_with_the_library():
    assert "mmt_set_ffn_fused" in ML.EXPORTED and "mmt_op_ffn" in ML.EXPORTED
    L = ML.lib()
    assert hasattr(L, "mmt_op_ffn")


def test_op_refuses_other_widths_before_any_launch():
    """C = 512 and more than four problems are refused from the arguments alone (no device touched)."""
    L = ML.lib()
    one = (ctypes.c_int32 * 1)(128)
    p = (ctypes.c_void_p * 1)(4096)
    args = lambda n, Ms, c: (None, n, Ms, c, p, c, 4096, c, 4096, 4096, 4 * c, 4096, p, 4 * c, p, p, None, 0, 0, 1.0,
                             None, None, None, None, None)
    assert L.mmt_op_ffn(*args(1, one, 512)) == -2  # MMT_ERR_UNSUPPORTED
    assert L.mmt_op_ffn(*args(5, (ctypes.c_int32 * 5)(*[128] * 5), 256)) == -2
    assert L.mmt_op_ffn(*args(0, one, 256)) == -1  # MMT_ERR_INVALID
