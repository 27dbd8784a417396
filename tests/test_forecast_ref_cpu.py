"""tests/forecast_ref.py against brute force on tiny cases, and the two caps the GPU tests rely on, on their own input
families: at most 5 % of a family's rows have a top-p margin below delta (test_gpu_forecast.py), at most 1 % of the
(row, level) cases of a stats family have a prefix sum within 1e-12 T of the level (test_gpu_pmf_stats.py)."""
import math

import numpy as np
import pytest

import forecast_ref as F


def tiny_rows(V, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 2.0, size=(S, V)).astype(np.float32)
    if S > 2:
        x[1] = -np.inf  # a dead row
        x[2, 0] = np.nan
    if V > 3:
        x[0, 1] = x[0, 2]  # a tie
    return x


@pytest.mark.parametrize("V,S", [(1, 1), (2, 3), (5, 1), (5, 4), (7, 6)])
def test_mixture_matches_brute_force(V, S):
    for seed, (t, k, p) in enumerate(F.SETTINGS + [(1.0, 2, 0.7), (0.5, 0, 0.0)]):
        x = tiny_rows(V, S, 10 * seed + V)
        laws = F.row_laws(x, t, k, p)
        for a in (None, np.linspace(-3.0, 1.0, S), np.where(np.arange(S) % 3 == 0, -np.inf, 0.25 * np.arange(S))):
            want, ess, live = F.brute_mixture(x, t, k, p, a)
            # brute force does not round a - mx to fp32: 2^-23 |d| relative per weight, in a ratio
            got = F.mixture(laws, np.arange(S), a, extra_rel=2.0 ** -22 * 8)
            if not laws["amb"].any():
                err = np.abs(got["pmf"] - want)
                assert np.all(err <= got["bound"]), (V, S, t, k, p, float((err / got["bound"]).max()))
            assert got["live"] == live
            assert math.isclose(got["ess"], ess, rel_tol=1e-5) or (ess == 0 and got["ess"] == 0)
            if live:
                assert abs(got["pmf"].sum() - 1.0) < 1e-12
                assert np.all(got["lo"] <= got["pmf"] + 1e-300) and np.all(got["pmf"] <= got["hi"] + 1e-300)
            else:
                assert not got["pmf"].any()


def test_mixture_of_one_path_is_its_law_and_dead_paths_do_not_count():
    x = F.make_rows(13)
    laws = F.row_laws(x, 0.8, 8, 1.0)
    one = F.mixture(laws, [5])
    assert np.array_equal(one["pmf"], laws["P"][5]) and one["live"] == 1 and one["ess"] == 1.0
    with_dead = F.mixture(laws, [5, 56, 58])
    assert np.array_equal(with_dead["pmf"], laws["P"][5]) and with_dead["live"] == 1
    a = np.array([0.0, -np.inf, 0.0])
    cut = F.mixture(laws, [5, 7, 5], a)
    assert np.allclose(cut["pmf"], laws["P"][5], rtol=1e-15) and cut["live"] == 2 and cut["ess"] == 2.0
    dead = F.mixture(laws, [56, 58])
    assert dead["live"] == 0 and dead["ess"] == 0.0 and not dead["pmf"].any()


def test_greedy_law_is_a_point_mass_on_the_first_maximum():
    x = np.array([[1.0, 3.0, 3.0, -1.0], [np.nan, -np.inf, 0.0, 0.0]], dtype=np.float32)
    laws = F.row_laws(x, 0.0, 7, 0.3)
    assert np.array_equal(laws["P"], [[0, 1, 0, 0], [0, 0, 1, 0]])


@pytest.mark.parametrize("V", F.VS)
def test_families_keep_the_ambiguous_rows_under_the_cap(V):
    x = F.make_rows(V)
    for (t, k, p) in F.SETTINGS:
        laws = F.row_laws(x, t, k, p)
        assert laws["amb"].sum() <= 0.05 * len(x), (V, t, k, p, int(laws["amb"].sum()))
        assert list(np.nonzero(laws["dead"])[0]) == [56, 58]
        live = ~laws["dead"]
        assert np.allclose(laws["P"][live].sum(1), 1.0, rtol=1e-12)
    for S in F.SAMPLES:
        idx = F.prompt_rows(S)
        assert idx.shape == (3, S) and not np.isin(idx[0], [56, 58]).any() and idx[2, 0] == 56


def test_pmf_stats_on_hand_cases():
    v = np.array([-2.0, -1.0, 0.0, 0.0, 1.5])
    q = np.array([0.125, 0.125, 0.25, 0.25, 0.25], dtype=np.float32)
    st, qt, alt = F.pmf_stats(q, v, True, None, (0.1, 0.5, 0.9))
    assert st[0] == 1.0 and math.isclose(st[1], -(2 * 0.125 * math.log(0.125) + 3 * 0.25 * math.log(0.25)))
    assert math.isclose(st[2], 0.125 * -3 + 0.25 * 1.5) and (st[4], st[5], st[6]) == (0.25, 0.5, 0.25)
    assert list(qt) == [0, 2, 4] and st[7] == 0.25
    assert list(alt) == [0, 3, 4]  # the prefix at token 2 is exactly 0.5: ambiguous by the rule
    st, qt, _ = F.pmf_stats(q, v, False, 1, (0.5,))  # a value series against token 1
    assert (st[4], st[5], st[6]) == (0.125, 0.125, 0.75)
    st, qt, _ = F.pmf_stats(q, v, False, 5, (0.5,))  # origin out of range
    assert np.isnan(st[4:7]).all() and not np.isnan(st[2])
    st, qt, _ = F.pmf_stats(q, None, False, None, (0.5,))
    assert np.isnan(st[2:7]).all() and qt[0] == 2
    st, qt, _ = F.pmf_stats(np.zeros(4, np.float32), v[:4], True, None, (0.5,))
    assert st[0] == 0 and np.isnan(st[1:]).all() and qt[0] == -1
    st, qt, _ = F.pmf_stats(q * 4, v, True, None, (0.1, 0.5, 0.9))  # unnormalised: the same summaries
    assert st[0] == 4.0 and (st[4], st[5], st[6]) == (0.25, 0.5, 0.25) and list(qt) == [0, 2, 4]


@pytest.mark.parametrize("V,seed", [(v, 0) for v in (1, 5, 13, 64, 65, 900, 8193)] + [(144, 1)])
def test_stats_families_keep_the_ambiguous_levels_under_the_cap(V, seed):
    rows, names = F.stats_cases(V, seed)
    levels = (0.05, 0.5, 0.95)
    amb = 0
    for r in rows:
        _, qt, alt = F.pmf_stats(r, None, False, None, levels)
        amb += int((qt != alt).sum())
    assert amb <= 0.01 * len(rows) * len(levels), (V, amb)
    for rep in (False, True):
        v = F.stats_values(V, rep, seed)
        assert np.all(np.diff(v) >= 0)
        # the mean is the one sum with terms of both signs: it is exactly zero or well away from cancelling
        for r in rows:
            st, _, _ = F.pmf_stats(r, v, True, None, levels)
            if st[0] > 0 and st[2] != 0:
                p = np.where(r > 0, r, 0).astype(np.float64) / st[0]
                assert abs(st[2]) >= 1e-3 * float((p * np.abs(v)).sum()), (V, rep, st[2])
