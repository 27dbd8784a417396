"""The host side of generate's forecast keyword and of the two forecast entries: plan_joint's refusals, the array
bookkeeping of ForecastLaunch / StatsLaunch, and the entries' refusals, none of which needs a device."""
import ctypes

import numpy as np
import pytest
import torch

import mmt_sample as MS
from model import DEFAULT_QUANTILES, JointPlan, check_forecast, plan_joint

V = [900, 13, 144, 5]
SHAPES = [(2, 8)] * 4


def test_forecast_is_planned():
    p = plan_joint([1, 3], None, V, SHAPES, 6)
    assert isinstance(p, JointPlan) and p.forecast is None
    assert plan_joint([1, 3], None, V, SHAPES, 6, forecast=False).forecast is None
    p = plan_joint([1, 3], None, V, SHAPES, 6, forecast=True)
    assert p.forecast == {"quantiles": list(DEFAULT_QUANTILES), "values": {}, "is_percent": {}}
    vals = np.linspace(-1.0, 1.0, 13)
    p = plan_joint("all", None, V, SHAPES, 6, forecast={"quantiles": (0.25, 0.75), "values": {1: vals},
                                                        "is_percent": {1: 1, 3: False}})
    f = p.forecast
    assert f["quantiles"] == [0.25, 0.75] and f["is_percent"] == {1: True, 3: False}
    assert f["values"][1].dtype == torch.float64 and f["values"][1].tolist() == vals.tolist()
    assert check_forecast({"values": {1: [0.0] * 13}}, [1], V)["values"][1].shape == (13,)  # ties are in order


def test_forecast_needs_the_list_form_and_says_how():
    with pytest.raises(ValueError, match=r"\[2\]"):
        plan_joint(2, None, V, SHAPES, 6, forecast=True)
    with pytest.raises(ValueError, match=r"\[0\]"):
        plan_joint(0, None, V, SHAPES, 6, forecast={"quantiles": [0.5]})
    assert plan_joint(2, None, V, SHAPES, 6, forecast=None) is None
    assert plan_joint(2, None, V, SHAPES, 6, forecast=False) is None


@pytest.mark.parametrize("bad", [
    {"values": {1: np.linspace(1.0, -1.0, 13)}},             # not in token order
    {"values": {1: [0.0, 1.0] + [float("nan")] + [2.0] * 10}},
    {"values": {1: np.zeros(12)}},                           # not V_1 numbers
    {"values": {0: np.zeros(900)}},                          # modality 0 is not generated
    {"values": [np.zeros(13)]},
    {"is_percent": {2: True}},
    {"quantiles": [0.5, 1.0]}, {"quantiles": [0.0]}, {"quantiles": [-0.1]}, {"quantiles": [float("nan")]},
    {"quantiles": "median"}, {"quantiles": [0.5 / 17 * k for k in range(1, 18)]},  # seventeen levels
    {"levels": [0.5]}, 3, "yes", [0.5],
])
def test_forecast_refusals(bad):
    with pytest.raises(ValueError):
        plan_joint([1, 3], None, V, SHAPES, 6, forecast=bad)


def test_forecast_launch_arrays():
    settings = [MS.check_settings(0.8, 8, 0.9), MS.check_settings(None, None, None), MS.check_settings(0, 3, 0.5)]
    fl = MS.ForecastLaunch([900, 13, 5], settings, [128 * 900, 128 * 13, 128 * 5], [4096, 8192], [128, 128])
    assert (fl.P, fl.G) == (3, 2)
    assert list(fl.V) == [900, 13, 5] and list(fl.row_stride) == [900, 13, 5]
    assert list(fl.top_k) == [8, 0, 3] and list(fl.temperature) == [np.float32(0.8), 1.0, 0.0]
    assert list(fl.top_p) == [np.float32(0.9), 1.0, 0.5]
    assert list(fl.pmf_stride) == [128 * 900, 128 * 13, 128 * 5]
    assert list(fl.lp) == [4096, 8192] and list(fl.lp_stride) == [128, 128]
    assert all(x is None for x in list(fl.logits) + list(fl.pmf) + list(fl.ess) + list(fl.live))
    fl.pmf[1] = 1 << 40  # a step moves pointers; the other arrays keep their contents
    fl.ess[2] = 64
    assert fl.pmf[1] == 1 << 40 and fl.pmf[0] is None and fl.ess[2] == 64 and list(fl.V) == [900, 13, 5]
    empty = MS.ForecastLaunch([], [], [])
    assert (empty.P, empty.G) == (0, 0) and len(empty.V) == 1 and len(empty.lp) == 1
    with pytest.raises(ValueError):
        MS.ForecastLaunch([5], settings[:1], [5], [256] * 9, [4] * 9)
    with pytest.raises(ValueError):
        MS.ForecastLaunch([5, 13], settings[:1], [5, 13])
    st = MS.StatsLaunch([13, 5], [13, 5], [False, True], (0.05, 0.5, 0.95))
    assert st.nq == 3 and list(st.levels) == [0.05, 0.5, 0.95] and list(st.is_percent) == [0, 1]
    assert list(st.origin_stride) == [1, 1] and all(x is None for x in list(st.values) + list(st.origin))
    with pytest.raises(ValueError):
        MS.StatsLaunch([13], [13], [False], (0.5, 1.5))
    assert MS.check_quantiles((0.5,)) == [0.5] and MS.STATS_FIELDS[4:7] == ("p_down", "p_flat", "p_up")


def test_entry_refusals_need_no_device():
    """What mmt_forecast_multi and mmt_pmf_stats refuse is refused before any HIP call; so is what they skip."""
    import mmt_lib as ML
    L = ML.lib()
    i32, i64, f32, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_double
    need = L.mmt_forecast_scratch_bytes(1, 2, 8)
    assert need >= 2 * 8 * (16 + 4) + 2 * 24
    assert L.mmt_forecast_scratch_bytes(0, 2, 8) == 0 and L.mmt_forecast_scratch_bytes(3, 0, 8) == 0
    for args in ((-1, 2, 8), (1, -2, 8), (1, 2, 0), (1, 1 << 20, 1 << 11)):
        assert L.mmt_forecast_scratch_bytes(*args) == -1, args

    def forecast(count=1, batch=2, samples=8, V_=13, stride=13, t=1.0, k=0, p=1.0, pmf_stride=13, wcount=0, lp=256,
                 lp_stride=4, j0=0, j1=0, logw=None, scratch=256, nbytes=need, logw_out=None):
        return L.mmt_forecast_multi(None, count, batch, samples, (i32 * 1)(V_), (vp * 1)(256), (i64 * 1)(stride),
                                    (f32 * 1)(t), (i32 * 1)(k), (f32 * 1)(p), (vp * 1)(256), (i64 * 1)(pmf_stride),
                                    wcount, (vp * 1)(lp), (i64 * 1)(lp_stride), j0, j1, logw, logw_out, None, None,
                                    scratch, nbytes)

    assert forecast(count=0) == 0 and forecast(batch=0) == 0
    nan = float("nan")
    for kw in (dict(count=-1), dict(batch=-1), dict(samples=0), dict(batch=1 << 20, samples=1 << 11), dict(V_=0),
               dict(stride=12), dict(t=-1.0), dict(t=nan), dict(k=-1), dict(p=nan), dict(pmf_stride=12),
               dict(wcount=-1), dict(wcount=9), dict(j0=-1), dict(j0=2, j1=1), dict(wcount=1, j1=5),
               dict(wcount=1, j1=2, lp=None), dict(scratch=None), dict(scratch=264), dict(nbytes=need - 1),
               dict(logw_out=512), dict(logw=512, logw_out=512)):  # logw_out without weights, or equal to logw
        assert forecast(**kw) == -1, kw
    assert forecast(V_=(1 << 20) + 1, stride=1 << 21, pmf_stride=1 << 21) == -2
    big = L.mmt_forecast_scratch_bytes(1, 1, 4097)
    assert forecast(batch=1, samples=4097, logw=256, nbytes=big) == -2  # weights above the on-chip cap
    assert forecast(batch=1, samples=4097, wcount=1, j1=2, nbytes=big) == -2

    def stats(count=1, rows=4, V_=13, stride=13, nq=2, levels=(0.25, 0.75), pmf=256, st=256, qtok=True):
        return L.mmt_pmf_stats(None, count, rows, (i32 * 1)(V_), (vp * 1)(pmf), (i64 * 1)(stride), None, None, None,
                               None, nq, (f64 * 16)(*levels), (vp * 1)(st), (vp * 1)(256) if qtok else None)

    assert stats(count=0) == 0 and stats(rows=0) == 0
    for kw in (dict(count=-1), dict(rows=-1), dict(V_=0), dict(stride=12), dict(nq=17), dict(nq=-1),
               dict(levels=(0.0, 0.5)), dict(levels=(0.5, 1.0)), dict(levels=(nan, 0.5)), dict(pmf=None),
               dict(st=None), dict(qtok=False)):
        assert stats(**kw) == -1, kw
    assert stats(V_=(1 << 20) + 1, stride=1 << 21) == -2
