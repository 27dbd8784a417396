"""The numpy restatement of mmt_resample's rule (tests/evidence_ref.py) against the consequences the header states,
and the GPU tests' input families against the thresholds those tests use."""
import math

import numpy as np
import pytest

import evidence_ref as E
from test_gpu_sample import delta


def test_equal_weights_give_the_identity():
    for S in E.SAMPLES:
        for seed in E.SEEDS:
            r = E.resample_prompt(np.full(S, -3.25), 2.0, seed, 1, 7)
            assert r["trigger"] and np.array_equal(r["ancestor"], np.arange(S)), (S, seed)
            assert r["ess"] == S and r["evidence"] == -3.25


def test_one_live_path_takes_every_slot():
    for S in (2, 17, 1000):
        a = np.full(S, -np.inf)
        a[S // 3] = -2.0
        r = E.resample_prompt(a, 2.0, 3, 0, 11)
        assert r["trigger"] and np.all(r["ancestor"] == S // 3)
        assert np.all(np.isinf(r["margin"]))
        assert r["evidence"] == pytest.approx(-2.0 - math.log(S))


def test_no_live_path_and_untriggered_prompts_are_the_identity():
    r = E.resample_prompt(np.full(9, -np.inf), 2.0, 1, 0, 0)
    assert not r["live"] and not r["trigger"] and np.array_equal(r["ancestor"], np.arange(9))
    r = E.resample_prompt(E.family(64, 0.3, 0)[0], 0.6, 1, 0, 0)
    assert not r["trigger"] and np.array_equal(r["ancestor"], np.arange(64))


@pytest.mark.parametrize("S", E.SAMPLES)
def test_dead_paths_are_never_chosen_and_counts_are_floor_or_ceil(S):
    for sigma in E.SIGMAS:
        for seed in E.SEEDS[:4]:
            a = E.family(S, sigma, seed)
            a[2, ::3] = -np.inf  # dead paths
            if S == 1:
                a[2, 0] = 0.0
            for b in range(3):
                r = E.resample_prompt(a[b], 2.0, seed, b, 5)
                assert r["trigger"]
                assert np.all(r["e"][r["ancestor"]] > 0), (S, sigma, seed, b)
                want = S * r["e"] / r["W"]
                got = np.bincount(r["ancestor"], minlength=S)
                assert np.all(got >= np.floor(want - 1e-9)) and np.all(got <= np.ceil(want + 1e-9)), (S, sigma, seed, b)
                assert np.all(np.diff(r["ancestor"]) >= 0)


def test_accumulate_is_serial_and_maps_nan_to_minus_inf():
    lp0 = np.array([[-1.0, np.nan], [-0.5, -0.25]], dtype=np.float32)
    lp1 = np.array([[-2.0, -1.0], [-np.inf, -0.125]], dtype=np.float32)
    a = E.accumulate(np.array([0.5, np.nan]), [lp0, lp1], 0, 1)
    assert a[0] == 0.5 - 1.0 - 2.0 and a[1] == -np.inf
    a = E.accumulate(np.zeros(2), [lp0, lp1], 0, 2)
    assert a[0] == -np.inf and a[1] == -np.inf
    a = E.accumulate(np.zeros(2), [lp0, lp1], 1, 2)
    assert a[0] == -np.inf and a[1] == -0.375


def test_gpu_families_stay_clear_of_the_thresholds():
    """ESS / S of every family member is at least 1e-3 away from the thresholds the GPU tests resample with, so the
    kernel's tree (fp64, roundings of 2^-53) cannot flip a trigger."""
    for S in E.SAMPLES:
        for sigma in E.SIGMAS:
            for seed in E.SEEDS:
                a = E.family(S, sigma, seed)
                for b in range(3):
                    r = E.resample_prompt(a[b], 0.0, seed, b, 0)
                    for thr in E.THRESHOLDS:
                        assert abs(r["ess"] / S - thr) >= 1e-3, (S, sigma, seed, b, r["ess"] / S)


def test_ambiguous_share_of_the_restatement():
    """With the sampler's delta (S for V) the restatement leaves few slots within delta of a boundary: the GPU test's
    5 % cap has room."""
    for S in (257, 1000, 4096):
        worst = 0.0
        for sigma in E.SIGMAS:
            for seed in E.SEEDS:
                a = E.family(S, sigma, seed)
                for b in range(3):
                    r = E.resample_prompt(a[b], 2.0, seed, b, E.POS)
                    worst = max(worst, float((r["margin"] < delta(S)).mean()))
        assert worst <= 0.05, (S, worst)
