"""The GEMM dispatch policy (csrc/mmt_gemm.hip, mmt_gemm_plan): which kernel, tile, pipeline and grid a launch
takes, read through mmt_op_gemm_plan, which needs no device.

Every expected plan comes from the commit before the plan function existed, never from the function itself:
  rec   recorded on an MI355X from that commit's build, one launch per case through mmt_op_gemm, mmt_op_gemm_qkv,
        mmt_op_gemm_wgrad, mmt_op_gemm_ln_bwd and mmt_op_gemm_f8 under a kernel trace (kernel name with its template
        arguments, grid, workgroup size); the same trace of this build is equal (profiles/r19_gemm_plan.txt)
  hand  written by hand from that commit's launch_t / use_big / auto_splits, for what no single-problem op entry
        reaches (tile_hint, dw_blocks, grouped batches, the residual + LayerNorm launcher); the engine's step
        traces confirm them where the engine reaches them
A row is (origin, call, plan). Plans: "invalid", "empty", or (family, tile, K-step, stages, blocks per CU, grid),
for weight gradients followed by ("slabs" | "acc", reduce blocks).
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import mmt_lib as ML

LINEAR, WGRAD, RESID_LN, LN_BWD, F8 = range(5)
FAMILY = ["ring", "pingpong", "fp8"]
TILE = ["128", "128x256", "256", "128x512"]
MIB = 1 << 20

C1_FFN0 = (16384, 1024, 256)
TGT_FFN0 = (32768, 2048, 512)
DW = (1024, 256, 16384)


def call(kind, shapes, a_kc=1, b_kc=1, epi="store_bf16", splits=1, lda=0, ldb=0, hint=0, dw_blocks=0, slab=0, flags=0):
    shapes = [shapes] if isinstance(shapes[0], int) else list(shapes)
    return dict(kind=kind, shapes=shapes, a_kc=a_kc, b_kc=b_kc, epi=ML.EPI[epi], splits=splits, lda=lda, ldb=ldb,
                hint=hint, dw_blocks=dw_blocks, slab=slab, flags=flags)


def lin(shape, epi, **kw):
    return call(LINEAR, shape, epi=epi, **kw)


def dx(shape, epi, **kw):
    return call(LINEAR, shape, a_kc=1, b_kc=0, epi=epi, **kw)


def wg(shapes=DW, **kw):
    return call(WGRAD, shapes, **kw)


def raw_plan(L, c):
    n = len(c["shapes"])
    arr = lambda k: (ctypes.c_int32 * n)(*[s[k] for s in c["shapes"]])
    out = (ctypes.c_int32 * 16)()
    assert L.mmt_op_gemm_plan(c["kind"], c["a_kc"], c["b_kc"], c["epi"], c["splits"], n, arr(0), arr(1), arr(2), c["lda"],
                              c["ldb"], c["hint"], c["dw_blocks"], ctypes.c_int64(c["slab"]), c["flags"], out) == 0
    return list(out)


def readable(c, p):
    status, family, tile, bk, stages, minb, swap, a_kc, b_kc, epi, gx, gy, gz, slabs, reduce_blocks, xcd = p
    if status:
        return ["ok", "empty", "invalid"][status]
    r = (FAMILY[family], TILE[tile], bk, stages, minb, (gx, gy, gz))
    if c["kind"] == WGRAD:
        assert epi == (ML.EPI["store_f32"] if slabs else ML.EPI["acc_f32"]) and not a_kc and not b_kc and swap
        r += ("slabs" if slabs else "acc", reduce_blocks)
    return r


def plan(c):
    return readable(c, raw_plan(ML.lib(), c))


PP = ("pingpong", "256", 64, 2, 1)      # the ping-pong kernel: BK 64, two K-tile buffers, one block per CU
OCC3 = ("ring", "128", 32, 2, 3)        # 128 x 128, bf16-output epilogues: BK 32 x 2 at 3 blocks per CU
DEF = ("ring", "128", 64, 2, 1)         # 128 x 128, the other epilogues: BK 64 x 2
T2 = ("ring", "128x256", 32, 3, 2)

CASES = {
    # ---- forward linear (A and B K-contiguous) ----
    "c1_ffn0": ("rec", lin(C1_FFN0, "bias_relu_bf16"), OCC3 + ((1024, 1, 1),)),
    "target_ffn0": ("rec", lin(TGT_FFN0, "bias_relu_bf16"), PP + ((1024, 1, 1),)),
    "target_ffn0_hint1": ("hand", lin(TGT_FFN0, "bias_relu_bf16", hint=1), T2 + ((2048, 1, 1),)),
    "under_gemm8_min_tiles": ("rec", lin((16384, 2048, 512), "bias_relu_bf16"), OCC3 + ((2048, 1, 1),)),
    "k1024": ("rec", lin((4096, 1024, 1024), "bias_relu_bf16"), PP + ((64, 1, 1),)),
    "m_below_big_tile": ("rec", lin((200, 1024, 1024), "bias_relu_bf16"), OCC3 + ((16, 1, 1),)),
    "store_f32": ("rec", lin((4096, 1024, 256), "store_f32"), DEF + ((256, 1, 1),)),
    "bias_resid": ("rec", lin((16384, 256, 1024), "bias_resid_f32"), PP + ((64, 1, 1),)),
    "bias_resid_small": ("rec", lin((4096, 512, 256), "bias_resid_f32"), DEF + ((128, 1, 1),)),
    "qkv2_small": ("rec", lin((16384, 96, 256), "bias_tanh_bf16", flags=1), OCC3 + ((128, 1, 1),)),
    "qkv2_big": ("rec", lin((16384, 768, 1024), "bias_tanh_bf16", flags=1), "invalid"),
    # ---- backward data (A K-contiguous, B MN-contiguous) ----
    "dx_dtanh": ("rec", dx((16384, 128, 256), "dtanh_bf16"), DEF + ((128, 1, 1),)),
    "dx_drelu": ("rec", dx((16384, 1024, 256), "drelu_bf16"), DEF + ((1024, 1, 1),)),
    "dx_drelu_target": ("rec", dx(TGT_FFN0, "drelu_bf16"), PP + ((1024, 1, 1),)),
    "dx_acc": ("rec", dx((16384, 256, 1024), "acc_f32"), PP + ((64, 1, 1),)),
    # ---- atomic split-K (A MN-contiguous; N on lanes, so never the ping-pong kernel) ----
    "atomic_nn_auto": ("rec", call(LINEAR, DW, 0, 0, "atomic_f32", splits=0), ("ring", "256", 32, 4, 1, (4, 32, 1))),
    "atomic_nn_4": ("rec", call(LINEAR, DW, 0, 0, "atomic_f32", splits=4), ("ring", "256", 32, 4, 1, (4, 4, 1))),
    "atomic_nk_auto": ("rec", call(LINEAR, DW, 0, 1, "atomic_f32", splits=0), ("ring", "256", 64, 2, 1, (4, 32, 1))),
    "atomic_nk_4": ("rec", call(LINEAR, DW, 0, 1, "atomic_f32", splits=4), ("ring", "256", 64, 2, 1, (4, 4, 1))),
    "atomic_small_auto": ("rec", call(LINEAR, (6, 32, 300), 0, 0, "atomic_f32", splits=0), DEF + ((1, 1, 1),)),
    # ---- weight gradients (slabs + reduce) ----
    "dw_slab64": ("rec", wg(slab=64 * MIB), ("ring", "256", 32, 4, 1, (4, 32, 1), "slabs", 256)),
    "dw_no_slab": ("rec", wg(), ("ring", "256", 32, 4, 1, (4, 1, 1), "acc", 0)),
    "dw_slab_caps": ("rec", wg(slab=8 * MIB), ("ring", "256", 32, 4, 1, (4, 8, 1), "slabs", 256)),
    "dw_blocks96": ("hand", wg(slab=64 * MIB, dw_blocks=96), ("ring", "256", 32, 4, 1, (4, 24, 1), "slabs", 256)),
    "dw_hint2": ("hand", wg(slab=64 * MIB, hint=2), DEF + ((16, 8, 1), "slabs", 256)),
    "dw_tiny": ("rec", wg((6, 32, 300), slab=64 * MIB), DEF + ((1, 1, 1), "acc", 0)),
    "dw_group4": ("hand", wg([DW, (256, 1024, 16384), (256, 256, 16384), (768, 256, 16384)], slab=64 * MIB),
                  ("ring", "256", 32, 4, 1, (4, 10, 4), "slabs", 256)),
    # ---- row-wide launches (the block owns whole rows: any K) ----
    "resid_ln_256": ("hand", call(RESID_LN, (16384, 256, 1024), flags=2), PP + ((64, 1, 1),)),
    "resid_ln_512": ("hand", call(RESID_LN, (32768, 512, 2048)), ("ring", "128x512", 32, 3, 1, (256, 1, 1))),
    "resid_ln_384": ("hand", call(RESID_LN, (16384, 384, 1024)), "invalid"),
    "ln_bwd_256": ("rec", call(LN_BWD, (16384, 256, 1024)), PP + ((64, 1, 1),)),
    "ln_bwd_512": ("rec", call(LN_BWD, (32768, 512, 2048)), ("ring", "128x512", 32, 3, 1, (256, 1, 1))),
    "ln_bwd_384": ("rec", call(LN_BWD, (16384, 384, 1024)), "invalid"),
    # ---- MX-fp8 ----
    "f8_k1024": ("rec", call(F8, (4096, 1024, 1024), epi="bias_relu_bf16"), ("fp8", "256", 128, 2, 1, (64, 1, 1))),
    "f8_k512": ("rec", call(F8, TGT_FFN0, epi="bias_relu_bf16"), ("fp8", "128", 128, 2, 1, (4096, 1, 1))),
    "f8_hint1": ("hand", call(F8, (4096, 1024, 1024), epi="bias_relu_bf16", hint=1), ("fp8", "128", 128, 2, 1, (256, 1, 1))),
    "f8_k1000": ("rec", call(F8, (4096, 1024, 1000), epi="bias_relu_bf16"), "invalid"),
    # ---- invalid inputs ----
    "lda_260": ("rec", lin((4096, 1024, 256), "store_f32", lda=260), "invalid"),
    "span_2gib": ("hand", lin((4096, 1024, 256), "store_f32", lda=(1 << 21) + 8), "invalid"),
    "dx_bias_tanh": ("rec", dx((4096, 1024, 256), "bias_tanh_bf16"), "invalid"),
    "empty": ("rec", lin((0, 1024, 256), "store_f32"), "empty"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_default_policy(name):
    origin, c, want = CASES[name]
    assert origin in ("rec", "hand")
    assert plan(c) == want


def test_issue_worked_examples():
    """The four plans worked out in the issue that asked for the plan function."""
    assert plan(CASES["c1_ffn0"][1]) == ("ring", "128", 32, 2, 3, (1024, 1, 1))
    assert plan(CASES["target_ffn0"][1])[:2] + plan(CASES["target_ffn0"][1])[5:] == ("pingpong", "256", (1024, 1, 1))
    assert plan(CASES["target_ffn0_hint1"][1]) == ("ring", "128x256", 32, 3, 2, (2048, 1, 1))
    assert plan(CASES["dw_slab64"][1]) == ("ring", "256", 32, 4, 1, (4, 32, 1), "slabs", 256)


# mmt_gemm_set_variant(v), each on a shape that shows its effect. SMALL takes the 128 x 128 tile by default, MID has
# M, N >= 256 and K = 512: the 256 x 256 tile only when bit 16 forces it. All "rec".
SMALL = lin((4096, 1024, 256), "store_f32")
MID = lin((512, 256, 512), "store_f32")
MID_NK = call(LINEAR, (512, 256, 512), 0, 1, "atomic_f32", splits=4)
VARIANTS = [
    (1, SMALL, ("ring", "128", 32, 2, 1, (256, 1, 1))),
    (2, SMALL, ("ring", "128", 32, 3, 1, (256, 1, 1))),
    (3, SMALL, ("ring", "128", 32, 4, 1, (256, 1, 1))),
    (4, SMALL, ("ring", "128", 64, 3, 1, (256, 1, 1))),
    (5, SMALL, ("ring", "128", 32, 3, 3, (256, 1, 1))),
    (6, SMALL, ("ring", "128", 32, 2, 3, (256, 1, 1))),
    (0x60, SMALL, DEF + ((256, 1, 1),)),  # bits 4-7 reach only the atomic launches ...
    (0x60, call(LINEAR, (6, 32, 300), 0, 0, "atomic_f32", splits=0), OCC3 + ((1, 1, 1),)),
    (-1, MID, DEF + ((8, 1, 1),)),
    (-1, MID_NK, DEF + ((8, 4, 1),)),
    # bit 16 alone: the big tile at K = 512, and with the ping-pong kernel on by default that is where an
    # A-K-contiguous launch lands whatever bits 8-11 say; they choose the ring of the launches that stay on it
    (0x10000, MID, PP + ((2, 1, 1),)),
    (0x10000 | 0x100, MID, PP + ((2, 1, 1),)),
    (0x10000, MID_NK, ("ring", "256", 64, 2, 1, (2, 4, 1))),
    (0x10000 | 0x100, MID_NK, ("ring", "256", 32, 4, 1, (2, 4, 1))),
    (0x10000 | 0x200, MID_NK, ("ring", "256", 32, 3, 1, (2, 4, 1))),
    (0x10000 | 0x300, MID_NK, ("ring", "256", 32, 2, 1, (2, 4, 1))),
    (0x40000 | 0x10000 | 0x100, MID, ("ring", "256", 32, 4, 1, (2, 1, 1))),
    (0x40000 | 0x10000 | 0x300, MID, ("ring", "256", 32, 2, 1, (2, 1, 1))),
    (0x20000 | 0x10000, MID, PP + ((2, 1, 1),)),
    (0x20000 | 0x10000, CASES["ln_bwd_256"][1], PP + ((64, 1, 1),)),
    (0x40000, CASES["ln_bwd_256"][1], ("ring", "256", 64, 2, 1, (64, 1, 1))),
    # (any v >= 0 also sets bits 0-3, here to variant 0: BK 64 x 2 where the default policy has 32 x 2 at 3 per CU)
    (0x40000, CASES["target_ffn0"][1], DEF + ((4096, 1, 1),)),
    (0x40000, CASES["k1024"][1], ("ring", "256", 64, 2, 1, (64, 1, 1))),
    (0x30000, CASES["dw_slab64"][1], PP + ((4, 32, 1), "slabs", 256)),
    (0x300, CASES["dw_slab64"][1], ("ring", "256", 32, 2, 1, (4, 32, 1), "slabs", 256)),
]


@pytest.mark.parametrize("i", range(len(VARIANTS)))
def test_variant_setter(i):
    v, c, want = VARIANTS[i]
    L = ML.lib()
    assert L.mmt_gemm_set_variant(v) == 0
    try:
        assert plan(c) == want
    finally:
        L.mmt_gemm_set_variant(-1)
    assert L.mmt_gemm_set_variant(7) == -1 and L.mmt_gemm_set_variant(0x400) == -1


def test_t2_setter():
    L = ML.lib()
    old = L.mmt_gemm_set_t2(1)
    try:
        assert plan(CASES["target_ffn0"][1]) == T2 + ((2048, 1, 1),)  # rec
        assert plan(CASES["k1024"][1]) == PP + ((64, 1, 1),)          # K at the threshold: unchanged
        assert plan(CASES["c1_ffn0"][1]) == OCC3 + ((1024, 1, 1),)    # not a big launch: unchanged
    finally:
        assert L.mmt_gemm_set_t2(old) == 1


# (variable, value, case, plan with it set); every case's plan without it is its CASES row. All "rec", in fresh
# processes with nothing but the variable set.
ENV = [
    ("MMT_GEMM_T2", 1, "target_ffn0", T2 + ((2048, 1, 1),)),
    ("MMT_GEMM_BIG", 0, "k1024", OCC3 + ((256, 1, 1),)),
    ("MMT_GEMM_BIG_KMIN", 2048, "k1024", OCC3 + ((256, 1, 1),)),
    ("MMT_GEMM_BIG_VARIANT", 2, "dw_slab64", ("ring", "256", 32, 3, 1, (4, 32, 1), "slabs", 256)),
    ("MMT_GEMM8", 0, "target_ffn0", OCC3 + ((4096, 1, 1),)),
    ("MMT_GEMM8_LN", 0, "ln_bwd_256", ("ring", "256", 64, 2, 1, (64, 1, 1))),
    ("MMT_GEMM8_DW", 1, "dw_slab64", PP + ((4, 32, 1), "slabs", 256)),
    ("MMT_GEMM8_KMIN", 1024, "target_ffn0", OCC3 + ((4096, 1, 1),)),
    ("MMT_GEMM8_MIN_TILES", 512, "under_gemm8_min_tiles", PP + ((512, 1, 1),)),
    ("MMT_GEMM_DW_VARIANT", 2, "dw_tiny", ("ring", "128", 32, 3, 1, (1, 1, 1), "acc", 0)),
    ("MMT_DW_SMALL", 1, "dw_slab64", DEF + ((16, 8, 1), "slabs", 256)),
    ("MMT_WGRAD_BLOCKS", 64, "dw_slab64", ("ring", "256", 32, 4, 1, (4, 16, 1), "slabs", 256)),
]

_CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
for c in json.loads(sys.argv[2]):
    n = len(c["shapes"])
    arr = lambda k: (ctypes.c_int32 * n)(*[s[k] for s in c["shapes"]])
    out = (ctypes.c_int32 * 16)()
    rc = L.mmt_op_gemm_plan(c["kind"], c["a_kc"], c["b_kc"], c["epi"], c["splits"], n, arr(0), arr(1), arr(2), c["lda"],
                            c["ldb"], c["hint"], c["dw_blocks"], ctypes.c_int64(c["slab"]), c["flags"], out)
    print(json.dumps([rc] + list(out)))
"""


def _plans_in_child(extra_env, names):
    """The named cases' plans in a fresh process that only loads the library (no torch, no device)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MMT_")}
    env.update(extra_env)
    cs = [CASES[n][1] for n in names]
    out = subprocess.run([sys.executable, "-c", _CHILD, ML.LIB_PATH, json.dumps(cs)], env=env, check=True,
                         capture_output=True, text=True, timeout=60).stdout
    rows = [json.loads(line) for line in out.splitlines()]
    assert len(rows) == len(cs) and all(r[0] == 0 for r in rows)
    return [(readable(c, r[1:]), r[1:]) for c, r in zip(cs, rows)]


ENV_CASES = sorted({e[2] for e in ENV})


def test_env_unset_is_the_default_policy():
    for n, (got, raw) in zip(ENV_CASES, _plans_in_child({}, ENV_CASES)):
        assert got == CASES[n][2], n
        assert raw[15] == (1 if CASES[n][1]["kind"] == WGRAD else 0), n  # XCD-major remap of the weight gradients


@pytest.mark.parametrize("var,val,name,want", ENV)
def test_env_knob_flips_the_plan(var, val, name, want):
    assert want != CASES[name][2]
    (got, raw), = _plans_in_child({var: str(val)}, [name])
    assert got == want


def test_env_xcd_plane():
    (got, raw), = _plans_in_child({"MMT_DW_XCD_PLANE": "0"}, ["dw_slab64"])
    assert got == CASES["dw_slab64"][2] and raw[15] == 0
