"""CPU checks of the sampling rule's restatement (tests/sampling_ref.py) and of the hash uniform it draws with;
the C entry's presence in the header and the binding. No GPU."""
import math
import os
import re

import numpy as np

import sampling_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(logits, temperature, top_k, top_p, u):
    """The rule by sorting, element by element in Python floats: returns (token, logprob, kept set)."""
    z = [float(x) for x in R.scaled(logits, temperature)]
    V = len(z)
    m = max(z)
    kept = set(range(V))
    if 0 < top_k < V:
        t_k = sorted(z, reverse=True)[top_k - 1]
        kept = {i for i in kept if z[i] >= t_k}
    e = {i: math.exp(z[i] - m) for i in kept}
    S = sum(e.values())
    p = float(np.float32(top_p))
    if p < 1.0:
        t_p = None
        for v in sorted({z[i] for i in kept}, reverse=True):
            if t_p is None and (p <= 0.0 or sum(e[i] for i in kept if z[i] >= v) >= p * S):
                t_p = v
        kept = {i for i in kept if z[i] >= t_p}
        S = sum(e[i] for i in kept)
    acc = 0.0
    for i in range(V):
        if i in kept:
            acc += e[i]
            if acc >= u * S:
                return i, math.log(e[i] / S), kept
    return max(kept), math.log(e[max(kept)] / S), kept


def test_helper_matches_brute_force_with_ties():
    rng = np.random.default_rng(7)
    n = 0
    for V in (1, 2, 5, 13, 24):
        for trial in range(30):
            # few distinct values: ties at the top-k threshold, at the maximum and inside top-p groups
            logits = rng.integers(-3, 3, size=V).astype(np.float32) * np.float32(0.75)
            if trial % 3 == 0:
                logits = rng.normal(0, 3, size=V).astype(np.float32)
            for (t, k, p) in ((1.0, 0, 1.0), (0.8, 3, 1.0), (0.8, 0, 0.9), (1.3, 4, 0.5), (1.0, 1, 1.0),
                              (1.0, V + 5, 1.0), (1.0, 0, 1e-6), (0.7, 2, 0.0), (1.0, V, 0.3)):
                r = R.sample_row(logits, t, k, p, seed=1234 + trial, row=V, pos=trial)
                tok, lp, kept = brute(logits, t, k, p, r["u"])
                if min(r["margin_u"], r["margin_p"]) < 1e-12:
                    continue  # two fp64 summation orders may disagree on a boundary this close
                assert set(np.nonzero(r["kept"])[0]) == kept, (V, trial, t, k, p)
                assert r["token"] == tok, (V, trial, t, k, p)
                assert abs(r["logprob"] - lp) < 1e-12, (V, trial, t, k, p)
                assert r["neighbor"] in kept
                n += 1
    assert n > 1000


def test_helper_ties_and_special_rows():
    # ties at the top-k threshold are all kept; the maximal group survives top_p <= 0 and a tiny top_p
    z = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 0.0], dtype=np.float32)
    r = R.sample_row(z, 1.0, 3, 1.0, 5, 0, 0)
    assert list(np.nonzero(r["kept"])[0]) == [1, 2, 3, 4]
    for p in (0.0, -1.0, 1e-6):
        r = R.sample_row(z, 1.0, 0, p, 5, 0, 0)
        assert list(np.nonzero(r["kept"])[0]) == [1, 3] and r["token"] in (1, 3)
        assert abs(r["logprob"] - math.log(0.5)) < 1e-12
    # greedy: the lowest index among the maxima, raw log-softmax
    r = R.sample_row(z, 0, 2, 0.1, 5, 0, 0)
    assert r["token"] == 1 and abs(r["logprob"] + math.log(np.exp(z.astype(np.float64) - 3).sum())) < 1e-12
    # NaN and -inf entries are never chosen; a row without a finite logit gives token 0 and NaN
    bad = np.array([np.nan, -np.inf, 0.5, np.nan], dtype=np.float32)
    for pos in range(20):
        assert R.sample_row(bad, 1.0, 0, 1.0, 9, 0, pos)["token"] == 2
    r = R.sample_row(np.array([-np.inf, np.nan], dtype=np.float32), 1.0, 0, 1.0, 9, 0, 0)
    assert r["token"] == 0 and math.isnan(r["logprob"])
    # an all-equal row is uniform
    r = R.sample_row(np.full(8, 2.5, np.float32), 0.5, 0, 1.0, 9, 3, 4)
    assert abs(r["logprob"] - math.log(1 / 8)) < 1e-12 and r["token"] == int(r["u"] * 8 - 1e-12)


def _chi2_sf_quantile(df, q):
    """The q quantile of chi-square(df) for even df, by bisection on the closed form of its survival function,
    exp(-x / 2) * sum_{j < df / 2} (x / 2)^j / j!."""
    assert df % 2 == 0

    def sf(x):
        return math.exp(-x / 2) * sum((x / 2) ** j / math.factorial(j) for j in range(df // 2))

    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if sf(mid) > 1 - q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def test_hash_uniform_chi_square_and_correlations():
    """65 536 draws at a fixed seed over a 13-way distribution: chi-square below the 1 - 1e-6 quantile of
    chi-square(12) (about 50.6), lag-1 correlation across positions and adjacent-row correlation small."""
    seed = 0x1234567890ABCDEF
    rng = np.random.default_rng(3)
    probs = np.exp(rng.normal(0, 1, 13))
    probs /= probs.sum()
    edges = np.cumsum(probs)
    rows, npos = 256, 256
    u = np.array([[R.uniform(seed, r, p) for p in range(npos)] for r in range(rows)])
    assert u.min() > 0.0 and u.max() < 1.0
    counts = np.bincount(np.minimum(np.searchsorted(edges, u.ravel(), side="left"), 12), minlength=13)
    n = rows * npos
    chi2 = float(((counts - n * probs) ** 2 / (n * probs)).sum())
    bound = _chi2_sf_quantile(12, 1 - 1e-6)
    assert 45 < bound < 56
    assert chi2 < bound, chi2
    c = u - 0.5
    lag = float((c[:, :-1] * c[:, 1:]).mean() / c.var())
    adj = float((c[:-1] * c[1:]).mean() / c.var())
    # 65 280 pairs: the standard error of a correlation of independent draws is 1 / sqrt(65 280) = 3.9e-3
    assert abs(lag) < 4 * 3.9e-3 and abs(adj) < 4 * 3.9e-3, (lag, adj)


def test_mmt_sample_in_header_and_binding():
    import mmt_lib as ML
    src = open(os.path.join(REPO, "include", "mmt.h")).read()
    assert re.search(r"\bint\s+mmt_sample\s*\(", src)
    assert "model.py:425-427" in src
    res, args = ML._SIGS["mmt_sample"]
    assert res is ML.c_i32 and len(args) == 16
    assert "mmt_sample" in ML.EXPORTED
