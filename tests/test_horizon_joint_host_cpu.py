"""The host side of generate's horizon={"baskets": ..., "pairs": ...} and of mmt_horizon_joint: check_horizon's accepted
forms and refusals, the absence of anything joint without the two keys, horizon_joint's argument checks and the entry's
refusals, none of which needs a device."""
import ctypes

import numpy as np
import pytest
import torch

import mmt_build
import mmt_lib as ML
import mmt_sample as MS
from model import check_horizon, plan_joint

V = [900, 13, 144, 5]
SHAPES = [(2, 8)] * 4
VALS = {1: np.linspace(-1.0, 1.0, 13), 2: np.linspace(-2.0, 2.0, 144), 3: [0.0, 1.0, 2.0, 3.0, 4.0]}
OK = {"values": VALS}


def plan(**keys):
    return plan_joint([1, 2, 3], None, V, SHAPES, 6, horizon=dict(OK, **keys)).horizon


def test_without_the_keys_nothing_joint_is_planned():
    h = plan()
    assert "baskets" not in h and "pairs" not in h and "joint_modalities" not in h
    assert sorted(h) == ["barriers", "is_percent", "modalities", "quantiles", "values"]
    assert check_horizon(None, [1], V) is None
    assert "mmt_horizon_joint.hip" in mmt_build.SOURCES
    assert "mmt_horizon_joint" in ML.EXPORTED and "mmt_horizon_joint_scratch_bytes" in ML.EXPORTED


def test_accepted_forms():
    h = plan(baskets=[{"weights": {3: 2, 1: -0.5}, "barriers": [1, -2.5]}, {"weights": {2: 1.0}}], pairs="all")
    assert h["baskets"] == [{"weights": {1: -0.5, 3: 2.0}, "barriers": [1.0, -2.5]}, {"weights": {2: 1.0}, "barriers": []}]
    assert h["pairs"] == [(1, 2), (1, 3), (2, 3)] and h["joint_modalities"] == [1, 2, 3]
    h = plan(pairs=[(3, 1)])
    assert h["baskets"] == [] and h["pairs"] == [(3, 1)] and h["joint_modalities"] == [1, 3]
    h = plan(baskets=[{"weights": {2: 1.0, 3: 0.0}}])  # a zero beside a non-zero coefficient is a coefficient
    assert h["pairs"] == [] and h["joint_modalities"] == [2, 3]
    h = plan(baskets=[{"weights": {1: 1.0}}] * 8, pairs=None)
    assert len(h["baskets"]) == 8
    # "all" pairs the modalities with values only
    h = plan_joint("all", None, V, SHAPES, 6, horizon={"values": {1: VALS[1], 3: VALS[3]}, "pairs": "all"}).horizon
    assert h["pairs"] == [(1, 3)]


@pytest.mark.parametrize("bad", [
    {"baskets": [{"weights": {0: 1.0}}]},                      # modality 0 is not generated
    {"baskets": [{"weights": {True: 1.0}}]}, {"baskets": [{"weights": {"1": 1.0}}]},
    {"baskets": [{"weights": {1: 0.0}}]}, {"baskets": [{"weights": {1: 0.0, 2: 0.0}}]},  # all zero
    {"baskets": [{"weights": {1: float("nan")}}]}, {"baskets": [{"weights": {1: float("inf")}}]},
    {"baskets": [{"weights": {1: "x"}}]}, {"baskets": [{"weights": {1: None}}]},
    {"baskets": [{"weights": {}}]}, {"baskets": [{"weights": [1.0, 0.0, 0.0]}]}, {"baskets": [{}]},
    {"baskets": [{"weights": {1: 1.0}, "levels": [0.5]}]}, {"baskets": {"weights": {1: 1.0}}}, {"baskets": [[1.0]]},
    {"baskets": [{"weights": {1: 1.0}, "barriers": [0.0]}]}, {"baskets": [{"weights": {1: 1.0}, "barriers": [1.0] * 9}]},
    {"baskets": [{"weights": {1: 1.0}}] * 9},
    {"pairs": "some"}, {"pairs": [(1, 1)]}, {"pairs": [(1, 0)]}, {"pairs": [(1, 4)]}, {"pairs": [(1, 2), (1, 2)]},
    {"pairs": [(1, 2, 3)]}, {"pairs": [1, 2]}, {"pairs": 3}, {"pairs": [(1, True)]},
    {"baskets": [], "pairs": []}, {"baskets": None, "pairs": None}, {"pairs": []},
])
def test_refusals(bad):
    with pytest.raises(ValueError):
        plan(**bad)


def test_a_modality_without_values_cannot_take_part():
    hz = {"values": {1: VALS[1], 3: VALS[3]}}
    for bad in ({"baskets": [{"weights": {2: 1.0}}]}, {"pairs": [(1, 2)]}):
        with pytest.raises(ValueError, match="values"):
            plan_joint([1, 2, 3], None, V, SHAPES, 6, horizon=dict(hz, **bad))


def test_check_baskets_and_pairs():
    coef, bars = MS.check_baskets([{"weights": (1, 0, -2), "barriers": (1, -1)}, {"weights": [0.0, 0.5, 0.0]}], 3)
    assert coef == [[1.0, 0.0, -2.0], [0.0, 0.5, 0.0]] and bars == [[1.0, -1.0], []]
    assert MS.check_baskets(None, 3) == ([], [])
    for bad in ([{"weights": [1.0, 2.0]}], [{"weights": [0.0] * 3}], [{"weights": [1.0, float("nan"), 0.0]}], [{}],
                [{"weights": [1.0, 0.0, 0.0], "barriers": [0.0]}], [{"weights": [1.0, 0.0, 0.0]}] * 9, {"weights": [1.0] * 3},
                [{"weights": [1.0] * 3, "levels": 1}], [{"weights": 1.0}]):
        with pytest.raises(ValueError):
            MS.check_baskets(bad, 3)
    assert MS.check_pairs("all", 4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and MS.check_pairs(None, 4) == []
    assert MS.check_pairs([(2, 0)], 3) == [(2, 0)] and len(MS.check_pairs("all", 8)) == 28
    for bad in ("some", [(0, 0)], [(0, 3)], [(-1, 0)], [(0, 1), (0, 1)], [(0, 1, 2)], [0, 1], 5, [(0, 1.0)],
                [(p, q) for p in range(8) for q in range(8) if p != q]):
        with pytest.raises(ValueError):
            MS.check_pairs(bad, 3 if not isinstance(bad, list) or len(bad) < 29 else 8)
    assert MS.JOINT_FIELDS[2:5] == ("p_down", "p_flat", "p_up") and len(MS.JOINT_FIELDS) == 9


def test_horizon_joint_refuses_before_touching_a_device():
    tok = [torch.zeros(8, 3, dtype=torch.int64)] * 2
    kw = dict(samples=4, values=[VALS[1], VALS[3]], is_percent=True)
    for bad in (dict(kw, samples=0), dict(kw, samples=4097), dict(kw, values=[VALS[1]]), dict(kw, values=None),
                dict(kw, baskets=[{"weights": [1.0]}]), dict(kw, baskets=[{"weights": [0.0, 0.0]}]),
                dict(kw, pairs=[(0, 2)]), dict(kw, pairs=[(1, 1)]), dict(kw, quantiles=[1.5]), dict(kw, samples=3),
                dict(kw, pairs="all")):  # the last: tokens on the CPU
        with pytest.raises(ValueError):
            MS.horizon_joint(tok, **bad)
    with pytest.raises(ValueError):
        MS.horizon_joint([], **kw)
    with pytest.raises(ValueError):
        MS.horizon_joint(tok * 5, samples=4, values=[VALS[1]] * 10, is_percent=True)  # more than 8 series


def test_entry_refusals_need_no_device():
    """What mmt_horizon_joint refuses is refused before any HIP call; so is what it skips."""
    L = ML.lib()
    i32, i64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    cells, rows = 3 * 8 * 5, 3 * 8
    need = L.mmt_horizon_joint_scratch_bytes(2, 3, 8, 5, 3)
    # x and d per problem, y / hi / lo per basket, the two spare planes of the walk, one dead flag per row
    assert need >= 2 * cells * 9 + 3 * cells * 24 + 2 * cells * 8 + rows * 4 and need % 16 == 0
    assert L.mmt_horizon_joint_scratch_bytes(2, 3, 8, 5, 0) < need
    for args in ((-1, 3, 8, 5, 1), (1, -3, 8, 5, 1), (1, 3, 0, 5, 1), (1, 3, 8, -5, 1), (1, 1 << 20, 1 << 11, 5, 1),
                 (1, 1, 4097, 5, 1), (9, 3, 8, 5, 1), (2, 3, 8, 5, 9), (2, 3, 8, 5, -1)):
        assert L.mmt_horizon_joint_scratch_bytes(*args) == -1, args
    nan, inf = float("nan"), float("inf")
    need = L.mmt_horizon_joint_scratch_bytes(2, 3, 8, 5, 1)  # what the calls below take

    def call(count=2, batch=3, samples=8, steps=5, V_=13, stride=5, pct=1, origin=True, nq=1, levels=(0.5,), nbk=1,
             coef=(1.0, -1.0), nb=1, bars=(1.0,), npair=1, pairs=(0, 1), tok=256, val=256, out=256, scratch=256,
             nbytes=need):
        n = max(count, 1)
        arr = lambda x: (vp * 28)(*[x] * 28)  # noqa: E731
        return L.mmt_horizon_joint(None, count, batch, samples, steps, (i32 * n)(*[V_] * n), (vp * n)(*[tok] * n),
                                   (i64 * n)(*[stride] * n), (vp * n)(*[val] * n), (i32 * n)(*[pct] * n),
                                   (vp * n)(*[256] * n) if origin else None, (i64 * n)(*[1] * n), None, nq,
                                   (f64 * 16)(*levels), nbk, (f64 * 128)(*coef), nb, (f64 * 64)(*bars), npair,
                                   (i32 * 56)(*pairs), arr(out), arr(256), arr(256), arr(256), arr(256), arr(256), None,
                                   None, scratch, nbytes)

    assert call(nbk=0, npair=0) == 0 and call(batch=0) == 0 and call(steps=0) == 0
    assert call(nbk=0, npair=0, scratch=None, tok=None) == 0  # nothing to launch: nothing else is looked at
    for kw in (dict(count=-1), dict(count=0), dict(batch=-1), dict(steps=-1), dict(samples=0),
               dict(batch=1 << 20, samples=1 << 11), dict(nq=17), dict(nb=9), dict(nbk=9), dict(nbk=-1), dict(npair=29),
               dict(npair=-1), dict(levels=(0.0,)), dict(levels=(nan,)), dict(bars=(0.0,)), dict(bars=(nan,)),
               dict(bars=(inf,)), dict(coef=(nan, 1.0)), dict(coef=(1.0, -inf)), dict(coef=(0.0, 0.0)), dict(pairs=(0, 0)),
               dict(pairs=(0, 2)), dict(pairs=(-1, 0)), dict(V_=0), dict(stride=4), dict(tok=None), dict(val=None),
               dict(out=None), dict(pct=0, origin=False), dict(scratch=None), dict(scratch=264), dict(nbytes=need - 1)):
        assert call(**kw) == -1, kw
    assert call(V_=(1 << 20) + 1) == -2
    assert call(batch=1, samples=4097, nbytes=1 << 40) == -2
    assert call(count=9, coef=(1.0,) * 9, nbytes=1 << 40) == -2
