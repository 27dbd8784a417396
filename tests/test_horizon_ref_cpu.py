"""horizon_ref (the numpy restatement of mmt_horizon_stats' rule) against a brute-force restatement in Python floats,
its properties, and the ambiguity caps of every input the GPU test uses. No device."""
import math

import numpy as np
import pytest

import horizon_ref as H


def _prompt(tok, v, pct, origin, a, levels, barriers):
    pq = H.paths(tok, v, pct, origin)
    return H.prompt(*pq, a, levels, barriers)


@pytest.mark.parametrize("pct", [True, False])
@pytest.mark.parametrize("sigma", [None, 0.3, 8.0])
@pytest.mark.parametrize("S,N,V", [(1, 1, 1), (2, 3, 5), (17, 4, 5), (40, 6, 900), (9, 2, 1)])
def test_reference_matches_brute_force(S, N, V, sigma, pct):
    rng = np.random.default_rng(S * 100 + N * 10 + V)
    tok = rng.integers(0, V, size=(S, N))
    origin = rng.integers(0, V, size=S)
    if S > 4:
        tok[3, N - 1] = V  # a dead row
    v = H.values_for(V)
    a = None if sigma is None else rng.normal(0, sigma, size=S)
    if a is not None and S > 2:
        a[1] = -np.inf
    ref = _prompt(tok, v, pct, origin, a, H.LEVELS, H.BARRIERS)
    stats, qrow, qval, hit, live = H.brute(tok.tolist(), v, pct, origin, a, H.LEVELS, H.BARRIERS)
    assert ref["live"] == live
    # the brute weights are not rounded to fp32: one ulp of fp32 on every weight, inside the bound's EPS
    assert (np.abs(np.array(stats) - ref["stats"])[:, :10] <= ref["bound"][:, :10] + 1e-300).all()
    assert np.array_equal(np.array(stats)[:, 10:], ref["stats"][:, 10:])
    assert (np.abs(np.array(hit) - ref["hit"]) <= ref["hit_bound"] + 1e-300).all()
    clear = ref["margin"] >= H.DELTA
    qrow, qval = np.array(qrow), np.array(qval)
    ok = (qrow == ref["qrow"]) & (qval == ref["qval"]) | ~clear & (qrow == ref["qalt"])
    assert ok.all()


def test_percent_series_is_the_cumulative_product_of_a_price():
    rng = np.random.default_rng(3)
    V, R, N = 41, 6, 20
    v = np.sort(np.round(rng.normal(0, 2, V), 2)) + 0.0
    tok = rng.integers(0, V, size=(R, N))
    x, hi, lo, d, dead = H.paths(tok, v, True)
    price = 100.0 * np.cumprod(1.0 + v[tok] / 100.0, axis=1)  # a synthetic price from 100
    assert np.allclose(x, price - 100.0, rtol=0, atol=1e-11) and not dead.any()
    assert np.array_equal(hi, np.maximum.accumulate(np.maximum(x, 0), axis=1))
    assert np.array_equal(d, np.sign(v[tok]).astype(np.int64))
    xv, _, lov, dv, _ = H.paths(tok, v, False, tok[:, 0])
    assert (xv[:, 0] == 0).all() and (dv[:, 0] == 0).all() and (lov <= 0).all()
    assert np.array_equal(dv[:, 1:], np.sign(v[tok[:, 1:]] - v[tok[:, :-1]]).astype(np.int64))


def test_properties():
    c = H.case(65, 33, 5, 8.0)
    for p in range(2):
        for r in c["ref"][p]:
            st = r["stats"]
            assert (np.diff(r["hit"], axis=0) >= 0).all()  # touched by step j: monotone in j
            assert np.allclose(st[:, 2:5].sum(axis=1), 1.0, atol=1e-12)
            assert np.allclose(st[:, 5:8].sum(axis=1), 1.0, atol=1e-12)
            assert (st[:, 10:11] <= r["qval"]).all() and (r["qval"] <= st[:, 11:12]).all()
            assert (st[:, 8] >= np.maximum(st[:, 0], 0) - 1e-12).all() and (st[:, 9] <= 0).all()
    # equal weights and no ties: the order statistic ceil(level S) - 1
    rng = np.random.default_rng(5)
    S = 40
    x = rng.permutation(S).astype(np.float64)[:, None] - 7.0
    r = H.prompt(x, np.maximum(x, 0), np.minimum(x, 0), np.zeros((S, 1), int), np.zeros(S, bool), None, H.LEVELS16, ())
    for k, lv in enumerate(H.LEVELS16):
        assert r["qval"][0, k] == np.sort(x[:, 0])[math.ceil(lv * S) - 1]
    # V = 1: every x equal, the order is that of s
    c = H.case(17, 2, 1, None)
    for r in c["ref"][0]:
        assert (r["qrow"] == [math.ceil(lv * 17) - 1 for lv in H.LEVELS]).all()


def test_dead_rows_and_empty_prompts():
    v = H.values_for(5)
    tok = np.array([[0, 1], [5, 1], [2, -1], [3, 3]])
    x, hi, lo, d, dead = H.paths(tok, v, False, np.array([0, 0, 0, 7]))
    assert dead.tolist() == [False, True, True, True]
    r = H.prompt(x, hi, lo, d, dead, None, H.LEVELS, H.BARRIERS)
    assert r["live"] == 1 and (r["qrow"] == 0).all() and r["ess"] == 1.0
    r = H.prompt(x[1:], hi[1:], lo[1:], d[1:], dead[1:], None, H.LEVELS, H.BARRIERS)
    assert r["live"] == 0 and r["ess"] == 0.0 and np.isnan(r["stats"]).all() and (r["qrow"] == -1).all()
    vinf = np.array([-np.inf, 0.0, 1.0])
    assert H.paths(np.array([[0, 1], [1, 2]]), vinf, True)[4].tolist() == [True, False]  # a non-finite x


@pytest.mark.parametrize("S", H.SAMPLES)
def test_ambiguity_caps_of_the_gpu_inputs(S):
    """At most max(1, 2 %) of a case's (prompt, step, level) triples lie within DELTA of a prefix boundary, on every
    input of test_gpu_horizon.py; none without weights."""
    total = [0, 0]
    for N in H.steps_for(S):
        for V in H.VS:
            for sigma in H.SIGMAS:
                c = H.case(S, N, V, sigma)
                for p in range(2):
                    amb, n = H.ambiguous(c["ref"][p])
                    if sigma is None:
                        amb = 0  # integer prefix sums: the device takes the same decision
                    assert amb <= H.cap(n), (S, N, V, sigma, p, amb, n)
                    total[0] += amb
                    total[1] += n
    print(f"S={S}: {total[0]} ambiguous triples of {total[1]}")
    for extra in (H.case(64, 5, 900, 0.3, 1, H.LEVELS16, H.BARRIERS8), H.case(65, 3, 144, 8.0, 2)):
        for p in range(2):
            amb, n = H.ambiguous(extra["ref"][p])
            assert amb <= H.cap(n)
