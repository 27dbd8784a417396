"""The host side of generate's evidence keywords: plan_joint's refusals that need no device, and the resampling
schedule."""
import pytest
import torch

from model import JointPlan, plan_joint, resample_points

V = [900, 13, 144, 5]
SHAPES = [(2, 8)] * 4


def given(N=6, rows=2, i=3):
    return {i: torch.zeros(rows, N, dtype=torch.long)}


def test_evidence_defaults_change_nothing():
    p = plan_joint([0, 1], given(), V, SHAPES, 6)
    assert isinstance(p, JointPlan) and p.evidence is None and p.points == []
    assert plan_joint(0, None, V, SHAPES, 6) is None


def test_evidence_is_planned():
    p = plan_joint([0], given(), V, SHAPES, 6, None, "weights")
    assert p.evidence == "weights" and p.points == []
    p = plan_joint([0], given(rows=6), V, SHAPES, 6, 3, "resample", 2, 0.25)
    assert p.evidence == "resample" and p.resample_every == 2 and p.ess_threshold == 0.25 and p.points == [1, 3]
    p = plan_joint([0], given(), V, SHAPES, 6, 3, "resample", ess_threshold=0)
    assert p.ess_threshold == 0.0 and p.points == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("kw", [
    dict(evidence="weights", given=None),            # no given modality
    dict(evidence="weights", given={}),
    dict(evidence="posterior"),                      # unknown value
    dict(evidence=True),
    dict(evidence="resample", resample_every=0, num_samples=2),
    dict(evidence="resample", resample_every=1.5, num_samples=2),
    dict(evidence="resample", resample_every=True, num_samples=2),
    dict(evidence="weights", ess_threshold=-0.1),
    dict(evidence="weights", ess_threshold=float("nan")),
    dict(evidence="weights", ess_threshold="half"),
    dict(evidence="resample"),                       # without num_samples
])
def test_evidence_refusals(kw):
    g = kw.pop("given", given())
    ns = kw.pop("num_samples", None)
    with pytest.raises(ValueError):
        plan_joint([0, 1], g, V, SHAPES, 6, ns, **kw)


def test_evidence_needs_the_list_form():
    with pytest.raises(ValueError):
        plan_joint(0, None, V, SHAPES, 6, None, "weights")
    with pytest.raises(ValueError):
        plan_joint(0, given(), V, SHAPES, 6, None, "weights")


def test_resampling_schedule():
    """After the sampling of new token j whenever (j + 1) % resample_every == 0 and j < N - 1."""
    assert resample_points(12, 1) == list(range(11))
    assert resample_points(12, 3) == [2, 5, 8]
    assert resample_points(12, 4) == [3, 7]
    assert resample_points(12, 12) == [] and resample_points(12, 50) == []
    assert resample_points(1, 1) == [] and resample_points(0, 1) == []
    assert resample_points(2, 1) == [0]


def test_entry_refusals_need_no_device():
    """What mmt_score_multi, mmt_resample and mmt_fanout_gather refuse is refused before any HIP call."""
    import ctypes

    import mmt_lib as ML
    L = ML.lib()
    one32 = (ctypes.c_int32 * 1)(13)
    ptrs = (ctypes.c_void_p * 1)(256)
    s13, s12 = (ctypes.c_int64 * 1)(13), (ctypes.c_int64 * 1)(12)
    assert L.mmt_score_multi(None, 0, 4, None, None, None, None, None, None, None) == 0
    assert L.mmt_score_multi(None, 1, 0, one32, ptrs, s13, ptrs, s13, ptrs, s13) == 0  # no rows: nothing launched
    assert L.mmt_score_multi(None, -1, 4, one32, ptrs, s13, ptrs, s13, ptrs, s13) == -1
    assert L.mmt_score_multi(None, 1, -1, one32, ptrs, s13, ptrs, s13, ptrs, s13) == -1
    assert L.mmt_score_multi(None, 1, 4, one32, ptrs, s12, ptrs, s13, ptrs, s13) == -1  # row_stride < V
    assert L.mmt_score_multi(None, 1, 4, one32, ptrs, s13, None, s13, ptrs, s13) == -1
    null = (ctypes.c_void_p * 1)(None)
    assert L.mmt_score_multi(None, 1, 4, one32, null, s13, ptrs, s13, ptrs, s13) == -1
    big = (ctypes.c_int32 * 1)(2 ** 20 + 1)
    sbig = (ctypes.c_int64 * 1)(2 ** 21)
    assert L.mmt_score_multi(None, 1, 4, big, ptrs, sbig, ptrs, s13, ptrs, s13) == -2  # MMT_ERR_UNSUPPORTED

    def resample(batch=2, samples=8, count=1, j0=0, j1=4, thr=0.5, logw=256, stride=s13):
        return L.mmt_resample(None, batch, samples, count, ptrs, stride, j0, j1, logw, 256, thr, 1, 0, 256, 256)

    assert resample(batch=0) == 0
    for kw in (dict(batch=-1), dict(samples=0), dict(count=9), dict(count=-1), dict(j0=-1), dict(j0=3, j1=2),
               dict(thr=float("nan")), dict(j1=14), dict(logw=None), dict(batch=1 << 20, samples=4096)):
        assert resample(**kw) == -1, kw
    assert resample(samples=4097) == -2  # above the on-chip fan
    assert L.mmt_fanout_gather(None, None, 1, 1, 1, 1, 1, 256, 256, 512) == -1
