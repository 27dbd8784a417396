"""The on-chip self-attention Q/K/V knob (mmt_set_attn_qkv_onchip, env MMT_ATTN_QKV_ONCHIP; include/mmt.h) without
a device: the setter returns the previous value, keeps only bits 0 and 1, and a fresh process starts from
the environment variable (default 3)."""
import ctypes
import os
import subprocess
import sys

import pytest

import mmt_lib as ML


def test_setter_returns_previous_value_and_masks_bits():
    L = ML.lib()
    first = L.mmt_set_attn_qkv_onchip(0)
    try:
        assert first in (0, 1, 2, 3)
        for v in (1, 2, 3, 0):
            old = L.mmt_set_attn_qkv_onchip(v)
            assert L.mmt_set_attn_qkv_onchip(v) == v, (v, old)
        assert L.mmt_set_attn_qkv_onchip(7) == 0
        assert L.mmt_set_attn_qkv_onchip(0) == 3  # only the two defined bits are kept
    finally:
        L.mmt_set_attn_qkv_onchip(first)


def _start_value(env_value):
    """The knob's start value in a fresh process that only loads the library (no torch, no device)."""
    code = ("import ctypes, sys\n"
            "L = ctypes.CDLL(sys.argv[1])\n"
            "f = L.mmt_set_attn_qkv_onchip; f.restype = ctypes.c_int; f.argtypes = [ctypes.c_int]\n"
            "print(f(0))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MMT_")}
    if env_value is not None:
        env["MMT_ATTN_QKV_ONCHIP"] = env_value
    out = subprocess.run([sys.executable, "-c", code, ML.LIB_PATH], env=env, check=True, capture_output=True, text=True,
                         timeout=60).stdout
    return int(out.strip())


@pytest.mark.parametrize("env_value,expect", [(None, 3), ("0", 0), ("1", 1), ("2", 2), ("3", 3), ("7", 3)])
def test_environment_sets_the_start_value(env_value, expect):
    assert _start_value(env_value) == expect


def test_symbols_declared_with_the_library():
    assert "mmt_set_attn_qkv_onchip" in ML.EXPORTED
    assert "mmt_op_attention_fwd_h1" in ML.EXPORTED and "mmt_op_attention_bwd_h1" in ML.EXPORTED
    L = ML.lib()
    assert L.mmt_set_attn_qkv_onchip.restype is ctypes.c_int32 or L.mmt_set_attn_qkv_onchip.restype is ctypes.c_int
