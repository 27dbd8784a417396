"""The restatement of mmt_eval_temperatures and of the fit (tests/calib_ref.py) against torch's fp64 log_softmax, a
vectorised count of the tables, hand-made cases of the fit and the convexity of the NLL in 1 / tau. No device."""
import math

import numpy as np
import pytest
import torch

import calib_ref as C
import eval_ref as E
import mmt_eval as ME

GRID = ME.default_temperatures()


def small_problem(V=13, B=3, T=5, seed=0, kind="value"):
    rng = np.random.default_rng(900 + V + seed)
    logits = rng.normal(0.0, 3.0, size=(B, T, V)).astype(np.float32)
    xb, yb = rng.integers(0, V, size=(B, T)), rng.integers(0, V, size=(B, T))
    return logits, xb, yb, E.series(V, "repeated" if kind == "repeated" else "value"), kind == "percent"


@pytest.mark.parametrize("V", [2, 13, 300])
def test_log_scores_against_fp64_log_softmax(V):
    """The restatement scales in fp32 as the device does: z' = fl(x * fl(1 / tau)). fl(1 / tau) is off by at most
    2^-24 relative and the product by 2^-24 more, so |z'_i - x_i / tau| <= 2 * 2^-24 |z_i| to first order. The log
    score z_y - logsumexp(z) moves by at most |dz_y| + max_i |dz_i| (logsumexp is 1-Lipschitz in the sup norm):
    at most 4 * max|z| * 2^-24. Everything after the product is fp64 on both sides (1e-16 relative, far below)."""
    logits, xb, yb, values, pct = small_problem(V)
    temps = [0.25, 0.7, 1.0, 1.7, 4.0]
    rec = C.records(logits, xb, yb, values, pct, temps)
    for k, tau in enumerate(temps):
        tau32 = float(np.float32(tau))
        want = torch.log_softmax(torch.from_numpy(logits).double() / tau32, dim=-1)
        want = want.gather(-1, torch.from_numpy(yb)[..., None])[..., 0].numpy()
        zmax = np.abs(logits.astype(np.float64) / tau32).max(axis=-1)
        err = np.abs(rec[..., k, 0] - want)
        assert np.all(err <= 4 * zmax * 2.0 ** -24), (V, tau, float((err / zmax).max() * 2 ** 24))
        # the masses sum to 1 and match the class sums of the fp64 softmax to the same order
        p = torch.softmax(torch.from_numpy(logits).double() / tau32, dim=-1).numpy()
        assert np.allclose(rec[..., k, 1:].sum(axis=-1), 1.0, atol=1e-12)
        for b in range(logits.shape[0]):
            for t in range(logits.shape[1]):
                sg = np.array([E.sign(values[i], values[xb[b, t]], pct) for i in range(V)])
                for f, s in ((1, -1), (2, 0), (3, 1)):
                    assert abs(rec[b, t, k, f] - p[b, t][sg == s].sum()) <= 8 * zmax[b, t] * 2.0 ** -24
    # at tau = 1 the four fields are eval_ref's
    one = E.records(logits, xb, yb, values, pct)
    assert np.array_equal(E.bits(rec[..., 2, :]), E.bits(one[..., 0:4]))


def test_dead_rows_and_t_begin():
    logits, xb, yb, values, pct = small_problem(5)
    logits, xb, yb = logits.copy(), xb.copy(), yb.copy()
    logits[0, 3] = -np.inf
    logits[1, 3] = np.nan
    logits[2, 3, 1] = np.inf
    yb[0, 4], xb[1, 4] = 5, -1
    rec = C.records(logits, xb, yb, values, pct, [0.5, 2.0], t_begin=2)
    assert np.isnan(rec[:, :2]).all()
    for b, t in ((0, 3), (1, 3), (0, 4), (1, 4)):
        assert np.isnan(rec[b, t]).all()
    assert not np.isnan(rec[2, 3]).any() and not np.isnan(rec[2, 2]).any()
    none = C.records(logits, xb, yb, None, False, [0.5, 2.0])
    assert np.isnan(none[..., 1:]).all() and np.array_equal(E.bits(none[:, 2:, :, 0]), E.bits(rec[:, 2:, :, 0]))


@pytest.mark.parametrize("bins", [1, 10, 64])
def test_tables_against_a_vectorised_count(bins):
    logits, xb, yb, values, pct = small_problem(13, B=4, T=6, kind="repeated")
    yb = yb.copy()
    yb[1, 4] = 13  # a dead row counts nowhere
    temps = [0.5, 1.0, 3.0]
    t_begin = 2
    rec = C.records(logits, xb, yb, values, pct, temps, t_begin)
    real = C.realised(xb, yb, values, pct)
    tot, rel = C.tables(rec, t_begin, bins, real)
    live = ~np.isnan(rec[:, t_begin:, :, 0])
    assert live.sum(axis=(0, 1)).tolist() == [4 * 4 - 1] * 3 == tot[:, 0].tolist()
    assert np.allclose(tot[:, 1], np.where(live, -rec[:, t_begin:, :, 0], 0.0).sum(axis=(0, 1)), rtol=1e-13)
    for k in range(3):
        for d in range(3):
            p = rec[:, t_begin:, k, 1 + d][live[..., k]]
            r = real[:, t_begin:][live[..., k]]
            j = np.minimum(bins - 1, np.floor(p * bins).astype(int))
            assert np.array_equal(rel[k, d, :, 0], np.bincount(j, minlength=bins))
            assert np.allclose(rel[k, d, :, 1], np.bincount(j, weights=p, minlength=bins), rtol=1e-13)
            assert np.array_equal(rel[k, d, :, 2], np.bincount(j, weights=(r == d - 1) * 1.0, minlength=bins))
    # without values: no reliability cell
    tot2, rel2 = C.tables(C.records(logits, xb, yb, None, False, temps, t_begin), t_begin, bins, C.realised(xb, yb, None, False))
    assert np.array_equal(tot2, tot) and not rel2.any()


@pytest.mark.parametrize("fit", [ME.fit_temperature, C.fit], ids=["mmt_eval", "calib_ref"])
def test_fit_cases(fit):
    grid = GRID.astype(np.float64)
    x = np.log(grid)
    # an exact parabola in ln tau: the vertex comes back
    for x_star in (math.log(1.7), math.log(0.9), x[5], 0.5 * (x[5] + x[6])):
        y = 2.0 + 0.75 * (x - x_star) ** 2
        tau, ks, at_bound = fit(GRID, 100, 100 * y)
        assert not at_bound and ks == int(np.argmin(y)) and tau == pytest.approx(math.exp(x_star), rel=1e-12)
    # both ends
    assert fit(GRID, 10, 10 * (x + 5.0)) == (0.25, 0, True)
    assert fit(GRID, 10, 10 * (5.0 - x)) == (4.0, 16, True)
    # K = 1
    assert fit(np.array([0.8], dtype=np.float32), 4, [12.0]) == (float(np.float32(0.8)), 0, True)
    # ties: the lowest index wins
    y = np.full(17, 3.0)
    y[[6, 9]] = 1.0
    tau, ks, at_bound = fit(GRID, 7, 7 * y)
    assert ks == 6 and not at_bound and grid[5] <= tau <= grid[7]
    assert fit(GRID, 7, 7 * np.full(17, 3.0)) == (0.25, 0, True)
    # non-finite means count as +inf; a non-finite neighbour leaves the grid point
    y = 2.0 + (x - x[4]) ** 2
    y[3] = np.inf
    assert fit(GRID, 5, 5 * y) == (float(grid[4]), 4, False)
    y[3] = np.nan
    assert fit(GRID, 5, 5 * y) == (float(grid[4]), 4, False)
    y = np.full(17, np.inf)
    y[16] = 1.0
    assert fit(GRID, 5, 5 * y) == (4.0, 16, True)
    for tau, ks, at_bound in (fit(GRID, 5, np.full(17, np.inf)), fit(GRID, 5, np.full(17, np.nan)),
                              fit(GRID, 0, np.zeros(17)), fit([1.0], 0, [0.0])):
        assert math.isnan(tau) and ks == -1 and at_bound


@pytest.mark.parametrize("fit", [ME.fit_temperature, C.fit], ids=["mmt_eval", "calib_ref"])
def test_fit_degenerate_parabola_returns_the_grid_point(fit):
    """With k* interior y0 > y1 <= y2, so the denominator (x1 - x0)(y1 - y2) + (x2 - x1)(y1 - y0) is negative in exact
    arithmetic and the vertex lies inside the bracket. In floating point the denominator can still round to 0 (a
    difference of one denormal) and the formula can overflow: both leave the grid point."""
    g = np.array([0.5, 1.0, 2.0], dtype=np.float32)
    assert fit(g, 1, [5e-324, 0.0, 0.0]) == (1.0, 1, False)  # (x2 - x1) * 5e-324 rounds to 0: denominator 0
    assert fit(g, 1, [1e308, -1e308, 1e308]) == (1.0, 1, False)  # inf / inf: the vertex is not finite
    tau, ks, at_bound = fit(g, 1, [2.0, 1.0, 1.0])  # a tie with the right neighbour: an ordinary vertex
    assert ks == 1 and not at_bound and 1.0 < tau < 2.0
    assert fit(g, 1, [1.0, 1.0, 1.0]) == (0.5, 0, True)  # all equal: the lowest index, at the grid's edge


def test_derive_matches_between_the_two():
    rng = np.random.default_rng(3)
    K, bins = 17, 10
    tot = np.zeros((K, 2))
    tot[:, 0] = 500
    tot[:, 1] = 500 * (2.0 + (np.log(GRID.astype(np.float64)) - 0.3) ** 2)
    rel = rng.integers(0, 50, size=(K, 3, bins, 3)).astype(np.float64)
    rel[:, 1] = 0  # no flat row: its ECE is NaN
    a, b = ME.derive_temperature(tot, rel, GRID), C.derive(tot, rel, GRID)
    assert (a["tau"], a["k_star"], a["at_bound"], a["k_one"], a["rows"]) == (b["tau"], b["k_star"], b["at_bound"], 8, 500)
    assert a["tau"] == pytest.approx(math.exp(0.3), rel=1e-9) and b["k_one"] == 8
    assert np.allclose(a["nll"], b["nll"], rtol=0, atol=0)
    for name in ("down", "flat", "up"):
        assert np.array_equal(np.isnan(a["ece"][name]), np.isnan(b["ece"][name]))
        assert np.allclose(a["ece"][name], b["ece"][name], equal_nan=True, rtol=1e-15)
    assert np.isnan(a["ece"]["flat"]).all()
    text = ME.temperature_summary_text(a)
    assert text.startswith(f"tau* {a['tau']:.4f} | NLL {a['nll'][8]:.4f} -> {a['nll'][a['k_star']]:.4f} | ECE up ")
    assert " down " in text and "edge" not in text
    edge = ME.derive_temperature(tot[:3], rel[:3], GRID[:3])
    assert edge["at_bound"] and edge["k_one"] is None and "tau* 0.3536 (at the grid's edge) | NLL n/a -> " in \
        ME.temperature_summary_text(edge)
    empty = ME.derive_temperature(np.zeros((K, 2)), np.zeros((K, 3, bins, 3)), GRID)
    assert empty["k_star"] == -1 and ME.temperature_summary_text(empty) == "no fit (no scored row)"


def test_bracket_property_on_the_restatement():
    """NLL(tau) is convex in 1 / tau, so with k* the grid's minimum (interior here) the true minimiser lies strictly
    between tau_{k*-1} and tau_{k*+1}; so does the fitted tau*."""
    x, yb = C.bracket_input()
    assert len(x) == 4096 and x.shape[1] == 16
    rec = C.records(x[:, None, :], np.zeros((4096, 1), dtype=np.int64), yb[:, None], None, False, GRID)
    tot, rel = C.tables(rec, 0, 10, C.realised(yb[:, None], yb[:, None], None, False))
    r = C.derive(tot, rel, GRID)
    ks = r["k_star"]
    assert 0 < ks < 16 and not r["at_bound"] and r["rows"] == 4096
    tau_hat = C.newton_tau(x, yb)
    assert GRID[ks - 1] < tau_hat < GRID[ks + 1], (tau_hat, ks)
    assert GRID[ks - 1] < r["tau"] < GRID[ks + 1]
    assert ME.fit_temperature(GRID, tot[0, 0], tot[:, 1]) == (r["tau"], ks, False)
    print(f"newton tau {tau_hat:.5f}, fitted {r['tau']:.5f}, k* {ks} (tau_k* {GRID[ks]:.5f})")
    assert abs(math.log(tau_hat / 1.7)) < 0.1  # the generating temperature, up to sampling noise
