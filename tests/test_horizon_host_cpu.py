"""The host side of generate's horizon keyword and of mmt_horizon_stats: plan_joint's refusals and defaults, check_barriers,
the array bookkeeping of HorizonLaunch, and the entry's refusals, none of which needs a device."""
import ctypes

import numpy as np
import pytest
import torch

import mmt_sample as MS
from model import DEFAULT_QUANTILES, check_horizon, plan_joint

V = [900, 13, 144, 5]
SHAPES = [(2, 8)] * 4
VALS1 = np.linspace(-1.0, 1.0, 13)


def test_horizon_is_planned_and_inherits_from_forecast():
    assert plan_joint([1, 3], None, V, SHAPES, 6).horizon is None
    assert plan_joint([1, 3], None, V, SHAPES, 6, horizon=False).horizon is None
    h = plan_joint([1, 3], None, V, SHAPES, 6, horizon={"values": {1: VALS1}}).horizon
    assert h["quantiles"] == list(DEFAULT_QUANTILES) and h["modalities"] == [1] and h["barriers"] == {}
    assert h["values"][1].dtype == torch.float64 and h["values"][1].tolist() == VALS1.tolist() and h["is_percent"] == {}
    # values and is_percent default to forecast='s; horizon's own entries win
    fc = {"values": {1: VALS1, 3: [0.0, 1.0, 2.0, 3.0, 4.0]}, "is_percent": {1: True}}
    h = plan_joint("all", None, V, SHAPES, 6, forecast=fc, horizon=True).horizon
    assert h["modalities"] == [1, 3] and h["is_percent"] == {1: True}
    h = plan_joint("all", None, V, SHAPES, 6, forecast=fc,
                   horizon={"is_percent": {1: False, 3: True}, "values": {1: VALS1 * 2}, "quantiles": (0.5,),
                            "barriers": {3: [-2, 2.5]}}).horizon
    assert h["is_percent"] == {1: False, 3: True} and h["values"][1].tolist() == (VALS1 * 2).tolist()
    assert h["quantiles"] == [0.5] and h["barriers"] == {3: [-2.0, 2.5]}
    # positional calls of before keep working: horizon is the last keyword
    assert plan_joint([1], None, V, SHAPES, 6, None, None, 1, 0.5, None).horizon is None
    assert check_horizon(None, [1], V) is None


def test_horizon_needs_the_list_form_and_says_how():
    with pytest.raises(ValueError, match=r"\[2\]"):
        plan_joint(2, None, V, SHAPES, 6, horizon=True)
    with pytest.raises(ValueError, match=r"\[0\]"):
        plan_joint(0, None, V, SHAPES, 6, horizon={"values": {0: np.zeros(900)}})
    assert plan_joint(2, None, V, SHAPES, 6, horizon=None) is None
    assert plan_joint(2, None, V, SHAPES, 6, horizon=False) is None


@pytest.mark.parametrize("bad", [
    True, {},                                                 # no values anywhere: token indices have no horizon
    {"values": {0: np.zeros(900)}},                           # modality 0 is not generated
    {"values": {1: VALS1[::-1].copy()}}, {"values": {1: np.zeros(12)}}, {"values": [VALS1]},
    {"values": {1: VALS1}, "is_percent": {2: True}},
    {"values": {1: VALS1}, "barriers": {2: [1.0]}},           # an ungenerated modality
    {"values": {1: VALS1}, "barriers": {1: [0.5] * 9}},       # too many
    {"values": {1: VALS1}, "barriers": {1: [0.0]}}, {"values": {1: VALS1}, "barriers": {1: [float("nan")]}},
    {"values": {1: VALS1}, "barriers": {1: [float("inf")]}}, {"values": {1: VALS1}, "barriers": {1: "up"}},
    {"values": {1: VALS1}, "barriers": [1.0]},
    {"values": {1: VALS1}, "quantiles": [0.5, 1.0]}, {"values": {1: VALS1}, "quantiles": [k / 18 for k in range(1, 18)]},
    {"values": {1: VALS1}, "levels": [0.5]}, 3, "yes", [0.5],
])
def test_horizon_refusals(bad):
    with pytest.raises(ValueError):
        plan_joint([1, 3], None, V, SHAPES, 6, horizon=bad)


def test_too_many_samples_are_refused_at_planning():
    ok = {"values": {1: VALS1}}
    assert plan_joint([1], None, V, SHAPES, 6, 4096, horizon=ok).horizon is not None
    with pytest.raises(ValueError, match="4096"):
        plan_joint([1], None, V, SHAPES, 6, 4097, horizon=ok)
    assert plan_joint([1], None, V, SHAPES, 6, 4097).horizon is None  # without the keyword any number


def test_check_barriers_and_launch_arrays():
    assert MS.check_barriers(None) == [] and MS.check_barriers((1, -2.5)) == [1.0, -2.5]
    for bad in ([0.0], [1.0, float("nan")], [float("-inf")], [1.0] * 9, "x", 3):
        with pytest.raises(ValueError):
            MS.check_barriers(bad)
    hl = MS.HorizonLaunch([900, 5], [136, 136], [True, False], (0.05, 0.5), [[1.0, -1.0, 3.0], [2.0, -2.0, 0.5]])
    assert (hl.P, hl.nq, hl.nb) == (2, 2, 3)
    assert list(hl.V) == [900, 5] and list(hl.tok_stride) == [136, 136] and list(hl.is_percent) == [1, 0]
    assert list(hl.levels) == [0.05, 0.5] and list(hl.origin_stride) == [1, 1]
    got = [list((ctypes.c_double * 3).from_address(hl.barriers[p])) for p in range(2)]
    assert got == [[1.0, -1.0, 3.0], [2.0, -2.0, 0.5]]
    assert all(x is None for x in list(hl.tok) + list(hl.values) + list(hl.origin) + list(hl.stats) + list(hl.hit))
    with pytest.raises(ValueError):
        MS.HorizonLaunch([5, 5], [4, 4], [True, True], (0.5,), [[1.0], [1.0, 2.0]])  # one nb per call
    with pytest.raises(ValueError):
        MS.HorizonLaunch([5], [4], [True], (1.5,), [[]])
    assert MS.HORIZON_FIELDS[2:5] == ("p_down", "p_flat", "p_up") and len(MS.HORIZON_FIELDS) == 12


def test_entry_refusals_need_no_device():
    """What mmt_horizon_stats refuses is refused before any HIP call; so is what it skips."""
    import mmt_lib as ML
    L = ML.lib()
    i32, i64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    need = L.mmt_horizon_scratch_bytes(2, 3, 8, 5)
    assert need >= 2 * (3 * 8 * 5 * 25 + 3 * 8 * 4) and need % 16 == 0
    assert L.mmt_horizon_scratch_bytes(0, 3, 8, 5) == 0
    for args in ((-1, 3, 8, 5), (1, -3, 8, 5), (1, 3, 0, 5), (1, 3, 8, -5), (1, 1 << 20, 1 << 11, 5), (1, 1, 4097, 5)):
        assert L.mmt_horizon_scratch_bytes(*args) == -1, args
    nan = float("nan")
    need = L.mmt_horizon_scratch_bytes(1, 3, 8, 5)  # what the one problem of the calls below takes

    def call(count=1, batch=3, samples=8, steps=5, V_=13, stride=5, pct=1, origin=True, nq=1, levels=(0.5,), nb=1,
             bars=(1.0,), tok=256, val=256, st=256, scratch=256, nbytes=need):
        barr = (f64 * 8)(*bars)
        return L.mmt_horizon_stats(None, count, batch, samples, steps, (i32 * 1)(V_), (vp * 1)(tok), (i64 * 1)(stride),
                                   (vp * 1)(val), (i32 * 1)(pct), (vp * 1)(256) if origin else None, (i64 * 1)(1), None,
                                   nq, (f64 * 16)(*levels), nb, (vp * 1)(ctypes.addressof(barr)), (vp * 1)(st),
                                   (vp * 1)(256), (vp * 1)(256), (vp * 1)(256), None, None, scratch, nbytes)

    assert call(count=0) == 0 and call(batch=0) == 0 and call(steps=0) == 0
    for kw in (dict(count=-1), dict(batch=-1), dict(steps=-1), dict(samples=0), dict(batch=1 << 20, samples=1 << 11),
               dict(nq=17), dict(nb=9), dict(levels=(0.0,)), dict(levels=(1.0,)), dict(levels=(nan,)), dict(bars=(0.0,)),
               dict(bars=(nan,)), dict(bars=(float("inf"),)), dict(V_=0), dict(stride=4), dict(tok=None), dict(val=None),
               dict(st=None), dict(pct=0, origin=False), dict(scratch=None), dict(scratch=264), dict(nbytes=need - 1)):
        assert call(**kw) == -1, kw
    assert call(V_=(1 << 20) + 1) == -2
    assert call(batch=1, samples=4097, nbytes=1 << 40) == -2
