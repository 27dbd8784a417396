"""The attention dispatch policy (csrc/mmt_attn.hip, mmt_attn_plan / mmt_attn_mask_plan): which kernels, template
arguments and grids a launch takes, read through mmt_op_attention_plan, which needs no device.

Every expected plan comes from the commit before the plan function existed, never from the function itself:
  rec   recorded on an MI355X from that commit's build, one launch per case through mmt_op_attention_fwd_drop,
        mmt_op_attention_bwd_drop, mmt_op_attention_fwd_h1_drop, mmt_op_attention_bwd_h1_drop and
        mmt_op_attention_mask under a kernel trace (kernel name with its template arguments, grid, workgroup size);
        the decoded trace (tools/attn_plan_trace.py) is tests/golden/attn_plan_rec.json, and the same trace of this build is equal
        (profiles/r23_attn_plan.txt)
  hand  written by hand from that commit's attn_dispatch / attn_launch / fused32_ok / ring64_fits, for what no
        single-problem op entry reaches: grouped batches, the stage-2 fields without the on-chip ones, the
        deterministic launch, spans of 2^31 bytes, stream counts the entries refuse themselves; and the two rows whose
        Q rows are not 16-byte aligned, which no GPU test feeds the chunked kernels, so none was launched to record
A row is (origin, knob, call[, plan]); a "rec" row's plan is the fixture's. Plans: "invalid", "empty", or one
(family, template arguments as in the kernel's name, grid in workgroups) per launch (attn_plan.readable).
"""
import json
import os
import subprocess
import sys

import pytest

import attn_plan as AP
import mmt_lib as ML
from attn_plan import BWD, FWD, MASK, call

DEFAULT_RING = 15 | 64
REC_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plan_rec.json")

CASES = {}


def rec(name, c, **knob):
    assert name not in CASES
    CASES[name] = ("rec", knob, c)


def hand(name, c, want, **knob):
    assert name not in CASES
    CASES[name] = ("hand", knob, c, want)


def chunk_pair(hs, drop, gdq, gdkdv, gz=1):
    return (("chunk_dq", (hs, drop), (gdq, 1, gz)), ("chunk_dkdv", (hs, drop), (gdkdv, 1, gz)))


# ---- every labelled row of the GPU tests (attn_plan.py has the tables) ----
for path, ring, hs, T, ns, scratch in AP.PATHS:
    for pas in (FWD, BWD):
        rec(f"readout-{path}-hs{hs}-T{T}-ns{ns}-{'fb'[pas]}", AP.readout_call(pas, T, hs, ns, scratch), ring=ring)
for ring, hs, T, ns, scratch in AP.DROP_PATHS:
    for pas in (FWD, BWD):
        rec(f"drop-r{ring}-hs{hs}-T{T}-ns{ns}-{'fb'[pas]}", AP.kernel_test_call(pas, 2, T, 3, hs, ns, scratch, True),
            ring=ring)
for ring in AP.HS64_RINGS:
    for B, T, H, ns in AP.HS64_SHAPES:
        for pas in (FWD, BWD):
            rec(f"hs64-r{ring}-B{B}-T{T}-H{H}-ns{ns}-{'fb'[pas]}", AP.kernel_test_call(pas, B, T, H, 64, ns), ring=ring)
for ring in AP.HS32_RINGS:
    for B, T, H, ns, scratch in AP.HS32_SHAPES:
        rec(f"hs32-r{ring}-B{B}-T{T}-H{H}-ns{ns}-{'ws' if scratch else 'nows'}-b",
            AP.kernel_test_call(BWD, B, T, H, 32, ns, scratch), ring=ring)

# ---- boundaries ----
for T in (256, 257):
    for ns in (1, 2):
        rec(f"edge32-T{T}-ns{ns}", call(BWD, 2, T, 2, 32, ns), ring=79)
for T in (512, 513):
    for ns in (1, 2):
        rec(f"edge64-T{T}-ns{ns}", call(BWD, 2, T, 2, 64, ns), ring=47)
rec("ms32-bit7-scratch", call(BWD, 2, 256, 2, 32, 2, flags=AP.SCRATCH, dq32_ld=68), ring=79 | 128)
rec("ms32-bit7-noscratch", call(BWD, 2, 256, 2, 32, 2), ring=79 | 128)
# alignment: the one-pass hs-32 kernel needs 16-B aligned Q rows; without them the two-pass pair, not a refusal
hand("q_ld-not-8", call(BWD, 2, 100, 2, 32, q_ld=68), chunk_pair(32, 0, 4, 4), ring=79)
hand("q-base-8mod16", call(BWD, 2, 100, 2, 32, flags=AP.Q_8MOD16), chunk_pair(32, 0, 4, 4), ring=79)
hand("q_ld-not-8-fwd", call(FWD, 2, 100, 2, 32, q_ld=68), (("chunk_fwd", (32, 0), (4, 1, 1)),), ring=79)
# the stage-2 and the on-chip fields
ONE32 = lambda drop, ms, q2, det, oc, grid: (("onepass32", (drop, ms, q2, det, oc), grid),)
rec("oc-fwd-T256", call(FWD, 2, 256, 2, 32, flags=AP.OC))
rec("oc-fwd-T257", call(FWD, 2, 257, 2, 32, flags=AP.OC))
rec("oc-fwd-drop", call(FWD, 2, 100, 2, 32, drop=True, flags=AP.OC))
rec("oc-bwd-T256", call(BWD, 2, 256, 2, 32, flags=AP.OC | AP.Q2))
rec("oc-bwd-T257", call(BWD, 2, 257, 2, 32, flags=AP.OC | AP.Q2))
rec("oc-bwd-drop", call(BWD, 2, 100, 2, 32, drop=True, flags=AP.OC | AP.Q2))
rec("oc-bwd-bit6-off", call(BWD, 2, 100, 2, 32, flags=AP.OC | AP.Q2), ring=15)
hand("q2-bwd", call(BWD, 2, 100, 2, 32, flags=AP.Q2), ONE32(0, 0, 1, 0, 0, (4, 1, 1)))
hand("q2-bwd-ns2", call(BWD, 2, 100, 2, 32, 2, flags=AP.Q2), "invalid")
hand("q2-bwd-ns2-bit7", call(BWD, 2, 100, 2, 32, 2, flags=AP.Q2 | AP.SCRATCH), "invalid", ring=79 | 128)
hand("q2-bwd-T257", call(BWD, 2, 257, 2, 32, flags=AP.Q2), "invalid")
hand("oc-without-q2-bwd", call(BWD, 2, 100, 2, 32, flags=AP.OC), "invalid")
hand("oc-bwd-hs64", call(BWD, 2, 100, 2, 64, flags=AP.OC | AP.Q2), "invalid")
hand("oc-fwd-hs64-chunked", call(FWD, 2, 100, 2, 64, flags=AP.OC), "invalid", ring=0)
hand("oc-fwd-ns2", call(FWD, 2, 100, 2, 32, 2, flags=AP.OC), "invalid")
hand("oc-fwd-h1_ld-not-8", call(FWD, 2, 100, 2, 32, flags=AP.OC, h1_ld=100), "invalid")
# the deterministic stage-2 launch: per-problem partials of B * 3 H * (512 + 16) floats
hand("q2-det", call(BWD, 4, 256, 2, 32, [1, 1], flags=AP.Q2 | AP.DET), ONE32(0, 0, 1, 1, 0, (8, 1, 2)))
hand("q2-det-oc-drop", call(BWD, 4, 256, 2, 32, [1, 1], True, AP.Q2 | AP.OC | AP.DET), ONE32(1, 0, 1, 1, 1, (8, 1, 2)))
hand("det-without-q2", call(BWD, 4, 256, 2, 32, flags=AP.DET), ONE32(0, 0, 0, 0, 0, (8, 1, 1)))
# grouped batches
hand("group3-fwd", call(FWD, 2, 100, 2, 32, [1, 1, 1]), (("chunk_fwd", (32, 0), (4, 1, 3)),))
hand("group3-bwd", call(BWD, 2, 100, 2, 32, [1, 1, 1]), ONE32(0, 0, 0, 0, 0, (4, 1, 3)))
hand("group2-bwd-hs64-ns2", call(BWD, 2, 300, 2, 64, [2, 2]),
     (("ring64_dq", (0, 4), (8, 1, 2)), ("ring64_dkdv", (0, 3, 4, 4), (24, 1, 2))))
hand("group2-fwd-hs64-mixed-ns", call(FWD, 2, 300, 2, 64, [1, 3]), (("ring64_fwd", (0, 4), (8, 1, 2)),))
# spans of 2^31 bytes (hs 64, B = H = 1): the rings address a sequence with 32-bit byte offsets
RING_PAIR = lambda gdq, gdkdv: (("ring64_dq", (0, 4), (gdq, 1, 1)), ("ring64_dkdv", (0, 3, 4, 4), (gdkdv, 1, 1)))
for what in ("q_ld", "dout_ld", "kv_ld"):
    hand(f"span-{what}-under-fwd", call(FWD, 1, 1024, 1, 64, **{what: (1 << 20) - 8}), (("ring64_fwd", (0, 4), (4, 1, 1)),))
    hand(f"span-{what}-at-fwd", call(FWD, 1, 1024, 1, 64, **{what: 1 << 20}), (("chunk_fwd", (64, 0), (4, 1, 1)),))
    hand(f"span-{what}-under-bwd", call(BWD, 1, 1024, 1, 64, **{what: (1 << 20) - 8}), RING_PAIR(4, 8))
    hand(f"span-{what}-at-bwd", call(BWD, 1, 1024, 1, 64, **{what: 1 << 20}), chunk_pair(64, 0, 4, 4))
hand("span-q_ld-at-onepass64", call(BWD, 1, 512, 1, 64, q_ld=1 << 21), chunk_pair(64, 0, 2, 2), ring=47)
# the keep-bit records of one (batch, head): ntri * 128 bytes, ntri = nt (nt + 1) / 2; nt = 5792 is the last under
hand("span-ntri-under-fwd", call(FWD, 1, 5792 * 32, 1, 64), (("ring64_fwd", (0, 4), (724, 1, 1)),))
hand("span-ntri-at-fwd", call(FWD, 1, 5792 * 32 + 1, 1, 64), (("chunk_fwd", (64, 0), (725, 1, 1)),))
hand("span-ntri-under-bwd", call(BWD, 1, 5792 * 32, 1, 64), RING_PAIR(724, 1448))
hand("span-ntri-at-bwd", call(BWD, 1, 5792 * 32 + 1, 1, 64), chunk_pair(64, 0, 725, 725))
# (the one-pass hs-32 kernel's own rule: Q / dO rows behind a buffer descriptor)
hand("span32-q_ld-under", call(BWD, 1, 256, 1, 32, q_ld=(1 << 22) - 8), ONE32(0, 0, 0, 0, 0, (1, 1, 1)))
hand("span32-q_ld-at", call(BWD, 1, 256, 1, 32, q_ld=1 << 22), chunk_pair(32, 0, 1, 1))
# each MMT_ATTN_RING bit set alone and cleared alone
for k in range(8):
    for tag, ring in (("set", 1 << k), ("clear", 255 & ~(1 << k))):
        rec(f"bit{k}-{tag}-hs64-f", call(FWD, 2, 300, 2, 64), ring=ring)
        rec(f"bit{k}-{tag}-hs64-b", call(BWD, 2, 300, 2, 64), ring=ring)
        rec(f"bit{k}-{tag}-hs32-b", call(BWD, 2, 100, 2, 32, 3, flags=AP.SCRATCH, dq32_ld=68), ring=ring)

# ---- refusals and empties ----
hand("mixed-dropout", call(FWD, 2, 100, 2, 32, [1, 1], [True, False]), "invalid")
hand("mixed-dropout-bwd", call(BWD, 2, 100, 2, 32, [1, 1], [False, True]), "invalid")
rec("o_ld-not-8", call(FWD, 2, 100, 2, 32, o_ld=68))
rec("o_ld-not-8-bwd", call(BWD, 2, 100, 2, 32, o_ld=68))
hand("o-base-8mod16", call(FWD, 2, 100, 2, 32, flags=AP.O_8MOD16), "invalid")
rec("dkv_ld-not-8", call(BWD, 2, 100, 2, 32, dkv_ld=68))
rec("dkv_hs-not-8", call(BWD, 2, 100, 2, 32, dkv_hs=36))
rec("dq_ld-not-8", call(BWD, 2, 100, 2, 32, dq_ld=68))
hand("dq-base-8mod16", call(BWD, 2, 100, 2, 32, flags=AP.DQ_8MOD16), "invalid")
hand("unequal-nstreams-bwd", call(BWD, 2, 100, 2, 32, [1, 2]), "invalid")
hand("unequal-nstreams-fwd", call(FWD, 2, 100, 2, 32, [1, 2]), (("chunk_fwd", (32, 0), (4, 1, 2)),))
hand("nstreams-0", call(FWD, 2, 100, 2, 32, 0), "invalid")
hand("nstreams-9", call(BWD, 2, 100, 2, 32, 9), "invalid")
rec("hs40", call(FWD, 2, 100, 2, 40))
rec("hs40-bwd", call(BWD, 2, 100, 2, 40))
hand("count-0", call(FWD, 2, 100, 2, 32, []), "empty")
rec("B-0", call(BWD, 0, 100, 2, 32))
rec("T-0", call(FWD, 2, 0, 2, 32))
hand("T-0-hs40", call(FWD, 2, 0, 2, 40), "empty")  # (nothing to launch is decided before the head size is looked at)

# ---- the keep-bit mask kernel ----
rec("mask-T1023", call(MASK, 1, 1023, 2, 0, drop=True))
rec("mask-T1024", call(MASK, 1, 1024, 2, 0, drop=True))
for g in (1, 2, 4, 8, 16, 3):  # 180 tiles: no multiple of 4 g for any g; 3 is not a legal value and falls to 8
    rec(f"mask-g{g}", call(MASK, 2, 100, 3, 0, 3, True), mask_g=g)
rec("mask-batch", call(MASK, 2, 33, 3, 0, [1, 3, 2], [True, False, True]))
rec("mask-no-dropout", call(MASK, 2, 33, 3, 0, [1, 2], [False, False]))
hand("mask-count-0", call(MASK, 2, 33, 3, 0, []), "empty")
hand("mask-nstreams-9", call(MASK, 2, 33, 3, 0, 9, True), "invalid")
hand("mask-nstreams-9-no-dropout", call(MASK, 2, 33, 3, 0, 9, False), "empty")

# ---- environment: a fresh process per value with nothing but the variable set; all "rec" ----
# the same calls with no knob touched (hs 64: by hand, no recorded row has the default ring; the others are above)
hand("default-hs64-f", call(FWD, 2, 300, 2, 64), (("ring64_fwd", (0, 4), (8, 1, 1)),))
hand("default-hs64-b", call(BWD, 2, 300, 2, 64), (("ring64_dq", (0, 4), (8, 1, 1)), ("ring64_dkdv", (0, 3, 4, 4), (12, 1, 1))))
ENV_CASES = ["default-hs64-f", "default-hs64-b", "edge32-T256-ns1", "mask-T1023"]
ENV = [("MMT_ATTN_RING", 0), ("MMT_ATTN_RING", 47), ("MMT_MASK_G", 4)]
for var, val in ENV:
    for n in ["bit0-set-hs64-f", "bit0-set-hs64-b", "edge32-T256-ns1", "mask-T1023"]:  # (the first two: the same calls)
        rec(f"env-{var}={val}-{n}", CASES[n][2], env={var: str(val)})
rec("env-MMT_MASK_G=4-setter-2", CASES["mask-T1023"][2], env={"MMT_MASK_G": "4"}, mask_g=2)

REC = json.load(open(REC_PATH)) if os.path.exists(REC_PATH) else {}


def _tuples(x):
    return tuple(_tuples(v) for v in x) if isinstance(x, list) else x


def want_of(name):
    row = CASES[name]
    return row[3] if row[0] == "hand" else _tuples(REC[name])


class knobs:
    """The row's setter values for the length of a `with`; defaults: the ring as loaded, tiles per wave by T."""

    def __init__(self, knob):
        self.knob = knob

    def __enter__(self):
        L = ML.lib()
        self.ring = L.mmt_attn_set_ring(self.knob.get("ring", DEFAULT_RING))
        self.g = L.mmt_attn_set_mask_g(self.knob.get("mask_g", 0))
        return L

    def __exit__(self, *exc):
        ML.lib().mmt_attn_set_ring(self.ring)
        ML.lib().mmt_attn_set_mask_g(self.g)


IN_PROCESS = [n for n in CASES if "env" not in CASES[n][1]]


def test_fixture_is_complete():
    assert sorted(REC) == sorted(n for n in CASES if CASES[n][0] == "rec")


@pytest.mark.parametrize("name", IN_PROCESS)
def test_policy(name):
    with knobs(CASES[name][1]) as L:
        assert AP.plan(L, CASES[name][2]) == want_of(name)


def test_det_stride():
    with knobs({}) as L:
        assert AP.raw_plan(L, CASES["q2-det"][2])[30:] == [4 * 3 * 2 * (512 + 16), 0]  # (low, high 32 bits)
        assert AP.raw_plan(L, CASES["q2-bwd"][2])[30:] == [0, 0]
        # B * H = 2^21: 3 * 528 * 2^21 floats, past 32 bits; the launch is planned as before the plan existed
        big = AP.raw_plan(L, call(BWD, 1 << 11, 256, 1 << 10, 32, flags=AP.Q2 | AP.DET))
        assert big[0] == 0 and (big[31] << 32) + (big[30] & 0xFFFFFFFF) == 3 * 528 << 21


def _fams(name):
    w = want_of(name)
    return w if isinstance(w, str) else tuple(l[0] for l in w)


def test_labelled_rows_take_the_family_they_are_named_for():
    """The recorded plans against what the GPU tests' labels and docstrings claim (attn_plan.py)."""
    for path, ring, hs, T, ns, scratch in AP.PATHS:
        fwd, bwd = AP.PATH_FAMILIES[path]
        assert _fams(f"readout-{path}-hs{hs}-T{T}-ns{ns}-f") == (fwd,), (path, hs, T, ns)
        assert _fams(f"readout-{path}-hs{hs}-T{T}-ns{ns}-b") == bwd, (path, hs, T, ns)
    path_of = {p[1:]: p[0] for p in AP.PATHS}
    for ring, hs, T, ns, scratch in AP.DROP_PATHS:  # "one T per kernel path of test_gpu_attn_dropout.py's table"
        fwd, bwd = AP.PATH_FAMILIES[path_of[(ring, hs, T, ns, scratch)]]
        assert _fams(f"drop-r{ring}-hs{hs}-T{T}-ns{ns}-f") == (fwd,) and _fams(f"drop-r{ring}-hs{hs}-T{T}-ns{ns}-b") == bwd
    for ring in AP.HS64_RINGS:
        for B, T, H, ns in AP.HS64_SHAPES:
            fwd, bwd, occ = AP.hs64_claim(ring, T, ns)
            n = f"hs64-r{ring}-B{B}-T{T}-H{H}-ns{ns}"
            assert _fams(n + "-f") == fwd and _fams(n + "-b") == bwd, n
            if occ:
                assert want_of(n + "-b")[1][1][1] == occ, n
    for ring in AP.HS32_RINGS:
        for B, T, H, ns, scratch in AP.HS32_SHAPES:
            n = f"hs32-r{ring}-B{B}-T{T}-H{H}-ns{ns}-{'ws' if scratch else 'nows'}-b"
            assert _fams(n) == AP.hs32_claim(ring, T, ns, scratch), n


HS32_BWD = [n for n in IN_PROCESS if CASES[n][2]["pas"] == BWD and CASES[n][2]["hs"] == 32]


@pytest.mark.parametrize("name", HS32_BWD)
def test_stage2_query_is_the_plan_with_the_stage2_fields(name):
    """What the engine asks before it sets the stage-2 fields (mmt_attn_bwd_fuses_qkv2: the plan under
    ATTN_ASSUME_Q2) against the plan of the same batch with the fields set."""
    c = CASES[name][2]
    fuses = lambda p: not p[0] and AP.FAMILY[p[2]] == "onepass32" and bool(p[6])
    with knobs(CASES[name][1]) as L:
        asked = AP.raw_plan(L, dict(c, flags=(c["flags"] & ~AP.Q2) | AP.ASSUME_Q2))
        with_fields = AP.raw_plan(L, dict(c, flags=c["flags"] | AP.Q2))
    assert fuses(asked) == fuses(with_fields)


def test_stage2_query_says_yes_and_no():
    with knobs({}) as L:
        yes = AP.raw_plan(L, dict(CASES["edge32-T256-ns1"][2], flags=AP.ASSUME_Q2))
        no = AP.raw_plan(L, dict(CASES["edge32-T257-ns1"][2], flags=AP.ASSUME_Q2))
    assert (yes[0], AP.FAMILY[yes[2]], yes[6]) == (0, "onepass32", 1) and no[0] == 2


# ---------------------------------------------------------------------------------------------- environment
_CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
g = int(sys.argv[3])
if g:
    L.mmt_attn_set_mask_g(g)
for c in json.loads(sys.argv[2]):
    n = len(c["ns"])
    out = (ctypes.c_int32 * 32)()
    rc = L.mmt_op_attention_plan(c["pas"], n, c["B"], c["T"], c["H"], c["hs"], (ctypes.c_int32 * max(n, 1))(*c["ns"]),
                                 (ctypes.c_int32 * 10)(*c["ld"]), c["flags"], out)
    print(json.dumps([rc] + list(out)))
"""


def _plans_in_child(extra_env, names, mask_g=0):
    """The named cases' plans in a fresh process that only loads the library (no torch, no device)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MMT_")}
    env.update(extra_env)
    cs = [CASES[n][2] for n in names]
    out = subprocess.run([sys.executable, "-c", _CHILD, ML.LIB_PATH, json.dumps(cs), str(mask_g)], env=env, check=True,
                         capture_output=True, text=True, timeout=60).stdout
    rows = [json.loads(line) for line in out.splitlines()]
    assert len(rows) == len(cs) and all(r[0] == 0 for r in rows)
    return [AP.readable(r[1:]) for r in rows]


def test_env_unset_is_the_default_policy():
    assert _plans_in_child({}, ENV_CASES) == [want_of(n) for n in ENV_CASES]


@pytest.mark.parametrize("var,val", ENV)
def test_env_knob(var, val):
    want = [want_of(f"env-{var}={val}-{n}") for n in ["bit0-set-hs64-f", "bit0-set-hs64-b", "edge32-T256-ns1", "mask-T1023"]]
    assert want != [want_of(n) for n in ENV_CASES]
    assert _plans_in_child({var: str(val)}, ENV_CASES) == want


def test_mask_g_setter_is_ahead_of_the_variable():
    n = "env-MMT_MASK_G=4-setter-2"
    assert _plans_in_child(CASES[n][1]["env"], ["mask-T1023"], mask_g=2) == [want_of(n)]
    assert want_of(n) != want_of("env-MMT_MASK_G=4-mask-T1023") != want_of("mask-T1023")
