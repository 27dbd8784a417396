"""horizon_joint_ref (the fp64 numpy restatement of mmt_horizon_joint's rules) against a brute force in Python floats,
its closed cases, and what the GPU tests rely on for every input they use: the cap on ambiguous quantiles and that corr
goes uncompared only where a series is constant over the rows with weight."""
import numpy as np
import pytest

import horizon_joint_ref as J
import horizon_ref as H


def tiny(S, N, count, V, sigma, seed, cfg="full"):
    problems = J.problems_for(S, N, count, V, seed)
    coefs, barriers, pairs = J.config(cfg, count)
    a = None if sigma is None else J.F.log_weights(S, sigma, seed).reshape(-1)
    return problems, coefs, barriers, pairs, a


@pytest.mark.parametrize("S,N,count,V,sigma", [(7, 3, 3, 5, None), (16, 2, 2, 900, 0.3), (9, 4, 8, 900, 8.0),
                                               (1, 2, 2, 5, None), (5, 2, 3, 1, 0.3)])
def test_restatement_matches_brute_force(S, N, count, V, sigma):
    problems, coefs, barriers, pairs, a = tiny(S, N, count, V, sigma, 3)
    problems[1]["tok"][2 % S, 0] = V  # a row dead in one series
    refs = J.reference(problems, S, coefs, barriers, pairs, a)
    for b, ref in enumerate(refs):
        sl = slice(b * S, (b + 1) * S)
        one = [dict(q, tok=q["tok"][sl], origin=q["origin"][sl]) for q in problems]
        br = J.brute(one, coefs, barriers, pairs, None if a is None else a[sl], J.LEVELS)
        if br is None:
            assert ref["live"] == 0
            continue
        live, bks, prs = br
        assert live == ref["live"]
        got = {"ess": ref["ess"], "live": live,
               "bstats": [np.array(x[0]) for x in bks], "bqrow": [np.array(x[1]) for x in bks],
               "bqval": [np.array(x[2]) for x in bks], "btail": [np.array(x[3]) for x in bks],
               "bhit": [np.array(x[4]).reshape(N, -1) for x in bks], "pstats": [np.array(x) for x in prs]}
        # the brute force does not round its weights to fp32: it is a weighted implementation within EPS per weight
        J.check(got, ref, a is not None, f"brute S={S} b={b}")


@pytest.mark.parametrize("S", J.SAMPLES)
def test_gpu_inputs_ambiguity_cap_and_skipped_corr_cells(S):
    skipped = 0
    for N, count, V, sigma, cfg in J.GRID[S]:
        c = J.case(S, N, count, V, sigma, cfg)
        # without weights the prefix sums are integers: `check` treats no triple as ambiguous
        for k in range(len(c["coefs"]) if sigma is not None else 0):
            amb, n = J.ambiguous(c["ref"], k)
            assert amb <= J.cap(n), (S, N, count, V, sigma, cfg, k, amb, n)
        skip, bad = J.corr_skipped(c["ref"])
        assert bad == 0, (S, N, count, V, sigma, cfg)
        skipped += skip
        if V > 1 and S >= 15:
            # several distinct values over many rows: every cell of a prompt with more than one live row is compared
            for r in c["ref"]:
                if r["live"] > 1:
                    assert all(pr["corr_cmp"].all() or pr["const"].any() for pr in r["pairs"])
    print(f"S={S}: corr cells not compared: {skipped}")


def test_grid_covers_every_level_of_every_factor():
    for S in J.SAMPLES:
        g = J.GRID[S]
        assert {x[0] for x in g} == set(J.STEPS) and {x[1] for x in g} == set(J.COUNTS)
        assert {x[2] for x in g} == set(H.VS) and {x[3] for x in g} == set(H.SIGMAS) and {x[4] for x in g} == set(J.CONFIGS)
    full = J.config("full", 8)
    assert len(full[0]) == 8 and len(full[2]) == 28 and len(set(full[2])) == 28
    assert J.config("one_basket", 3)[2] == [] and J.config("pairs_only", 3)[0] == []


def two_equal(negate, sigma=0.3, S=40, N=6, V=900):
    rng = np.random.default_rng(5)
    tok = rng.integers(0, V, size=(S, N))
    org = rng.integers(0, V, size=S)
    v = H.values_for(V)
    q0 = dict(tok=tok, values=v, pct=False, origin=org)
    # the negated series: the values mirrored (still sorted) and the tokens with them
    q1 = dict(tok=V - 1 - tok, values=-v[::-1] + 0.0, pct=False, origin=V - 1 - org) if negate else dict(q0)
    a = J.F.log_weights(S, sigma, 1)[0]
    return J.reference([q0, q1], S, [], [], [(0, 1)], a)[0]["pairs"][0]


def test_equal_series_correlate_fully_and_negated_ones_inversely():
    pr = two_equal(False)
    assert pr["corr_cmp"].all()
    assert (np.abs(pr["stats"][:, 1] - 1.0) <= pr["bound"][:, 1]).all()
    table = pr["stats"][:, 4:13].reshape(-1, 3, 3)
    off = table.copy()
    off[:, [0, 1, 2], [0, 1, 2]] = 0.0
    assert (off == 0.0).all() and np.allclose(table.sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-12)
    pr = two_equal(True)
    assert (np.abs(pr["stats"][:, 1] + 1.0) <= pr["bound"][:, 1]).all()
    table = pr["stats"][:, 4:13].reshape(-1, 3, 3)
    assert (table[:, [0, 0, 1, 1, 2, 2], [0, 1, 0, 2, 1, 2]] == 0.0).all()  # only the anti-diagonal holds mass


def test_unit_basket_is_the_series_own_horizon():
    S, N, V = 33, 5, 900
    problems = J.problems_for(S, N, 3, V, 2)
    a = J.F.log_weights(S, 8.0, 2).reshape(-1)
    for p in range(3):
        coef = [1.0 if i == p else 0.0 for i in range(3)]
        refs = J.reference(problems, S, [coef], [list(H.BARRIERS)], [], a)
        q = problems[p]
        pq = H.paths(q["tok"], q["values"], q["pct"], q["origin"])
        for b in range(J.PROMPTS):
            sl = slice(b * S, (b + 1) * S)
            own = H.prompt(*[t[sl] for t in pq], a[sl], H.LEVELS, H.BARRIERS)
            r = refs[b]["baskets"][0]
            assert np.array_equal(r["stats"].view(np.int64), own["stats"][:, J.BSTATS].view(np.int64))
            assert np.array_equal(r["qrow"], own["qrow"]) and np.array_equal(r["qval"].view(np.int64),
                                                                             own["qval"].view(np.int64))
            assert np.array_equal(r["hit"].view(np.int64), own["hit"].view(np.int64))
            assert refs[b]["ess"] == own["ess"] and refs[b]["live"] == own["live"]


def test_tail_mean_lies_below_its_quantile_and_starts_at_the_first_row():
    S, N, V = 50, 4, 900
    for sigma in (None, 0.3, 8.0):
        problems, coefs, barriers, pairs, a = tiny(S, N, 3, V, sigma, 4)
        levels = (1e-9, 0.05, 0.5, 0.95)  # the first level selects the first row in the order
        for r in J.reference(problems, S, coefs, barriers, [], a, levels):
            if r["live"] == 0:
                continue
            for bk in r["baskets"]:
                assert (bk["tail"] <= bk["qval"] + bk["tail_bound"]).all()
                # (target * y) / target: the row's y to the two roundings of the rule, inside the bound
                # (rows of next to no weight may precede it under sigma = 8: every row up to the quantile's then holds
                # the minimum, and the mean of equal values is that value)
                first = bk["qval"] == bk["stats"][:, 7:8]
                assert sigma == 8.0 or first[:, 0].all()
                assert (np.abs(bk["tail"] - bk["qval"]) <= bk["tail_bound"])[first].all()
