"""horizon_score_ref (the CPU restatement of mmt_horizon_score's rules) against brute force and hand-worked cases, so
that what the GPU tests compare the kernels with is itself checked. No GPU."""
import math

import numpy as np
import pytest

import forecast_ref as F
import horizon_ref as H
import horizon_score_ref as HS


def one_step(x, xr, a=None, levels=(0.5,), barriers=(0.5,)):
    """records() for a one-step value-like sample: x [S], the realised change xr; the forecast from horizon_ref."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    S = len(x)
    dead = np.zeros(S, dtype=bool)
    hi, lo, d = np.maximum(x, 0.0), np.minimum(x, 0.0), H.sign(x)
    fc = H.prompt(x, hi, lo, d, dead, a, levels, barriers)
    xr = np.array([float(xr)])
    real = (xr, np.maximum(xr, 0.0), np.minimum(xr, 0.0), H.sign(xr), False)
    return HS.records(x, a, dead, real, fc["stats"], fc["qval"], fc["hit"], levels, barriers), fc


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("weighted", [False, True])
def test_integral_form_is_the_energy_form(weighted):
    rng = np.random.default_rng(5)
    worst = 0.0
    for S in (1, 2, 3, 7, 64, 300):
        for trial in range(6):
            x = np.round(rng.normal(0, 2, size=S), 1 if trial % 2 else 6)  # one decimal: heavy ties
            a = rng.normal(0, 3, size=S) if weighted else None
            w = F.path_weights(np.zeros(S) if a is None else a, np.zeros(S, dtype=bool))[0]
            for xr in (x[rng.integers(0, S)], rng.normal(0, 2), x.min() - 1.5, x.max() + 0.25, x.min(), x.max()):
                r, _ = one_step(x, xr, a)
                e = HS.energy(x, w, float(xr))
                got = r["sc"][0, 1]
                assert got >= 0.0
                if e > 1e-9:
                    assert rel(got, e) <= 1e-12, (S, trial, xr, got, e)
                    worst = max(worst, rel(got, e))
                else:
                    assert abs(got - e) <= 1e-15 * (1 + np.abs(x).max())
    print("integral against energy form, largest relative difference", worst)


def test_all_equal_paths_and_one_path():
    for S in (1, 2, 9):
        for xr in (0.75, -1.25, 0.5):
            r, _ = one_step([0.5] * S, xr)
            assert r["sc"][0, 1] == abs(0.5 - xr)  # exactly: no gap has width, the tail is one subtraction
            assert r["sc"][0, 2] == (0.0 if xr < 0.5 else 1.0 if xr > 0.5 else 0.5)


def test_pit_of_a_realised_row_that_is_one_of_the_paths():
    S, N, V = 17, 5, 900
    c = HS.case(S, N, V, None)
    for p in range(2):
        x, hi, lo, d, dead = H.paths(c["tok"][p], c["values"], p == 0, c["origin"])
        for b in range(H.PROMPTS):
            s = 3
            sl = slice(b * S, (b + 1) * S)
            row = c["tok"][p][b * S + s][None]
            rz = HS.realised(row, c["values"], p == 0, c["origin"][b * S + s][None])
            assert np.array_equal(rz[0][0].view(np.int64), x[b * S + s].view(np.int64))  # x* is x_s bit for bit
            ref = c["ref"][p][b]
            r = HS.records(x[sl], None, dead[sl], [t[0] for t in rz], ref["stats"], ref["qval"], ref["hit"], H.LEVELS,
                           H.BARRIERS)
            for j in range(N):
                below, equal = (x[sl, j] < x[b * S + s, j]).sum(), (x[sl, j] == x[b * S + s, j]).sum()
                assert equal >= 1 and r["sc"][j, 2] == (below + 0.5 * equal) / S
                assert 0.0 < r["sc"][j, 2] < 1.0
                assert r["sc"][j, 1] <= x[sl, j].max() - x[sl, j].min()  # CRPS of a member: at most the spread


def test_two_paths_two_steps_by_hand():
    # a value series over the values (0, 1, 2, 4) from origin token 1 (value 1): path 0 goes 2, 4, path 1 goes 0, 0;
    # realised 1 (no change), then 4
    values = np.array([0.0, 1.0, 2.0, 4.0])
    tok = np.array([[2, 3], [0, 0]])
    x, hi, lo, d, dead = H.paths(tok, values, False, np.array([1, 1]))
    assert x.tolist() == [[1.0, 3.0], [-1.0, -1.0]]
    levels, bars = (0.25, 0.75), (2.0, -0.5)
    fc = H.prompt(x, hi, lo, d, dead, None, levels, bars)
    rz = HS.realised(np.array([[1, 3]]), values, False, np.array([1]))
    assert rz[0].tolist() == [[0.0, 3.0]] and rz[1].tolist() == [[0.0, 3.0]] and rz[2].tolist() == [[0.0, 0.0]]
    assert rz[3].tolist() == [[0, 1]]
    r = HS.records(x, None, dead, [t[0] for t in rz], fc["stats"], fc["qval"], fc["hit"], levels, bars)
    sc = r["sc"]
    # step 0: paths at -1 and 1, realised 0: one gap, F = 1/2, s = 0: (0 - -1) / 4 + (1 - 0) / 4 = 0.5; energy form:
    # (1 + 1) / 2 - 0.5 * (2 * 2 / 4) = 0.5. PIT = 1/2. mean 0: error 0. x* == 0 selects p_flat = 0; d* = 0 selects
    # step_flat = 0.
    assert sc[0].tolist() == [0.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0]
    # step 1: paths at -1 and 3, realised 3: the gap gives (3 - -1) / 4 = 1, no tail; energy: (4 + 0) / 2 - 0.5 * (2 * 4
    # / 4) = 1. PIT = (1 + 0.5) / 2. mean 1: error -2. x* > 0 selects p_up = 1/2; d* = +1 selects step_up = 1/2 (path
    # 0 rose, path 1 stayed at 0). hi* = 3, lo* = 0.
    assert sc[1].tolist() == [3.0, 1.0, 0.75, -2.0, 0.5, 0.5, 3.0, 0.0]
    # quantiles 0.25 / 0.75 are the lower / upper path. step 0: q = -1: (0 - -1) * 0.25; q = 1: (0 - 1) * (0.75 - 1)
    assert r["pin"].tolist() == [[0.25, 0.25], [1.0, 0.0]]
    # barriers 2 and -0.5. step 0: hit = (0, 1/2), realised touched neither: (0, 1/4). step 1: hit = (1/2, 1/2),
    # realised touched 2 only: (1/4, 1/4)
    assert r["bs"].tolist() == [[0.0, 0.25], [0.25, 0.25]]
    agg, aggq, aggb, pit = HS.tables(sc[None], r["pin"][None], r["bs"][None], fc["stats"][None], fc["qval"][None],
                                     fc["hit"][None], rz[3], bars, 4)
    # step 1: count, crps, |x*|, |err|, err^2, mass on sign, sign hit (down and up tie at 1/2: down is predicted, the
    # realised sign is up), mass on step, step hit (down 0, flat 1/2, up 1/2: flat predicted, up realised), variance 4
    assert agg[1].tolist() == [1.0, 1.0, 3.0, 2.0, 4.0, 0.5, 0.0, 0.5, 0.0, 4.0]
    assert agg[0].tolist() == [1.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert aggq[1].tolist() == [[1.0, 0.0], [0.0, 1.0]] and aggq[0].tolist() == [[0.25, 0.0], [0.25, 1.0]]
    assert aggb[1].tolist() == [[0.25, 0.5, 1.0], [0.25, 0.5, 0.0]]
    assert pit.tolist() == [[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]


def test_tables_against_a_plain_loop():
    S, N, V = 16, 33, 900
    c = HS.case(S, N, V, 0.3)
    bins = 10
    for p in range(2):
        paths = H.paths(c["tok"][p], c["values"], p == 0, c["origin"])
        recs = []
        for b in range(H.PROMPTS):
            sl = slice(b * S, (b + 1) * S)
            ref = c["ref"][p][b]
            recs.append((HS.records(paths[0][sl], c["logw"][sl], paths[4][sl], [t[b] for t in c["rz"][p]], ref["stats"],
                                    ref["qval"], ref["hit"], H.LEVELS, H.BARRIERS), ref))
        sc = np.stack([r["sc"] for r, _ in recs])
        pin, bs = np.stack([r["pin"] for r, _ in recs]), np.stack([r["bs"] for r, _ in recs])
        st, qv, ht = (np.stack([f[k] for _, f in recs]) for k in ("stats", "qval", "hit"))
        agg, aggq, aggb, pit = HS.tables(sc, pin, bs, st, qv, ht, c["rz"][p][3], H.BARRIERS, bins)
        for j in range(N):
            crps = n = cover = hits = 0.0
            hist = [0] * bins
            for b in range(H.PROMPTS):
                n += 1
                crps += sc[b, j, 1]
                cover += sc[b, j, 0] <= qv[b, j, 2]
                hits += int(np.argmax(st[b, j, 2:5])) - 1 == HS.sgn(sc[b, j, 0])  # np.argmax: the first of the maxima
                hist[min(bins - 1, int(sc[b, j, 2] * bins))] += 1
            assert agg[j, 0] == n and agg[j, 1] == crps and aggq[j, 2, 1] == cover and agg[j, 6] == hits
            assert pit[j].tolist() == hist
            assert agg[j, 2] == sum(abs(sc[b, j, 0]) for b in range(H.PROMPTS))
            assert math.isclose(aggb[j, 1, 1], ht[:, j, 1].sum(), rel_tol=1e-15)


def test_the_family_holds_every_kind_of_realised_row_and_the_bounds_are_small():
    kinds = set()
    for S in (1, 16, 17):
        for N in HS.STEPS:
            c = HS.case(S, N, 900, 8.0)
            kinds |= {k for row in c["kinds"] for k in row}
            for p in range(2):
                paths = H.paths(c["tok"][p], c["values"], p == 0, c["origin"])
                for b in range(H.PROMPTS):
                    sl = slice(b * S, (b + 1) * S)
                    ref = c["ref"][p][b]
                    r = HS.records(paths[0][sl], c["logw"][sl], paths[4][sl], [t[b] for t in c["rz"][p]],
                                   ref["stats"], ref["qval"], ref["hit"], H.LEVELS, H.BARRIERS)
                    x = paths[0][sl]
                    if c["kinds"][p][b] == "below" and not np.isnan(r["sc"][0, 0]):
                        assert (r["sc"][:, 0] <= x.min(axis=0)).all() and (r["sc"][:, 2] <= 0.5).all()
                    if c["kinds"][p][b] == "above" and not np.isnan(r["sc"][0, 0]):
                        assert (r["sc"][:, 0] >= x.max(axis=0)).all() and (r["sc"][:, 2] >= 0.5).all()
                    live = ~np.isnan(r["sc"][:, 1])
                    assert (r["crps_bound"][live] <= 2e-6 * (r["sc"][live, 1] + 1e-9) + 1e-10).all()
                    assert (r["pit_bound"][live] <= 1e-6).all()
    assert kinds == set(HS.KINDS)


# ------------------------------------------------------------------------------------------
# the host side: generate's realised keyword, the config keys, RolloutMetrics' arithmetic, the entry's refusals
# ------------------------------------------------------------------------------------------
V4 = [900, 13, 144, 5]
SHAPES = [(2, 8)] * 4
VALS1 = np.linspace(-1.0, 1.0, 13)


def test_realised_is_planned_and_refused_like_horizon():
    import torch
    from model import plan_joint
    hz = {"values": {1: VALS1}}
    y = torch.zeros(2, 6, dtype=torch.int64)
    assert plan_joint([1, 3], None, V4, SHAPES, 6, horizon=hz).realised is None
    p = plan_joint([1, 3], None, V4, SHAPES, 6, horizon=hz, realised={1: y})
    assert list(p.realised) == [1] and p.realised[1] is y
    # positional calls of before keep working: realised is the last keyword
    assert plan_joint([1], None, V4, SHAPES, 6, None, None, 1, 0.5, None, hz).realised is None
    with pytest.raises(ValueError, match="horizon="):
        plan_joint([1, 3], None, V4, SHAPES, 6, realised={1: y})           # no horizon
    with pytest.raises(ValueError, match=r"\[1\]"):
        plan_joint(1, None, V4, SHAPES, 6, realised={1: y})                # the int form
    for bad in ({3: y},                                                     # generated, but without values
                {0: y},                                                     # not generated
                {1: y.int()}, {1: y[:, :5]}, {1: y[:1]}, {1: y.tolist()}, {True: y}, {}, [y], y):
        with pytest.raises(ValueError):
            plan_joint([1, 3], None, V4, SHAPES, 6, horizon=hz, realised=bad)


def test_config_keys_defaults_and_refusals():
    import config_utils as C
    old = C._config_cache
    try:
        C._config_cache = {"block_size": 32}
        assert C._get_eval_rollout_paths() == 0 and C._get_eval_rollout_steps() == 16
        assert C._get_eval_rollout_seed() == 0
        C._config_cache = {"block_size": 32, "eval_rollout_paths": 64, "eval_rollout_steps": 31, "eval_rollout_seed": 7}
        assert (C._get_eval_rollout_paths(), C._get_eval_rollout_steps(), C._get_eval_rollout_seed()) == (64, 31, 7)
        for key, get, bads in (("eval_rollout_paths", C._get_eval_rollout_paths, (-1, 4097, 1.5, True, "8", None)),
                               ("eval_rollout_steps", C._get_eval_rollout_steps, (0, 32, 33, 2.0, True, None)),
                               ("eval_rollout_seed", C._get_eval_rollout_seed, (-1, 0.5, True, "0", None))):
            for bad in bads:
                C._config_cache = {"block_size": 32, key: bad}
                with pytest.raises(ValueError, match=key):
                    get()
        assert C._DEFAULTS["training_parameters"]["eval_rollout_paths"] == 0
    finally:
        C._config_cache = old


def test_rollout_metrics_arithmetic():
    import mmt_eval as ME
    N, bins = 3, 4
    agg = np.zeros((N, 10))
    agg[0] = [4, 2.0, 8.0, 6.0, 16.0, 1.0, 3, 2.0, 1, 36.0]
    agg[1] = [2, 3.0, 0.0, 0.0, 0.0, 2.0, 2, 2.0, 2, 0.0]  # nothing moved: no skill defined
    aggq = np.zeros((N, 2, 2))
    aggq[0] = [[0.4, 1], [0.8, 3]]
    aggb = np.zeros((N, 1, 3))
    aggb[0] = [[0.5, 1.0, 2]]
    pit = np.zeros((N, bins))
    pit[0] = [1, 1, 1, 1]
    pit[1] = [2, 0, 0, 0]
    r = ME.derive_rollout(agg, aggq, aggb, pit, (0.25, 0.75), (1.5,))
    assert r["count"].tolist() == [4, 2, 0]
    assert r["crps"][0] == 0.5 and r["skill"][0] == 0.75 and np.isnan(r["skill"][1]) and np.isnan(r["crps"][2])
    assert r["mae"][0] == 1.5 and r["rmse"][0] == 2.0 and r["spread"][0] == 3.0
    assert r["coverage"][0].tolist() == [0.25, 0.75] and r["pinball"][0].tolist() == [0.1, 0.2]
    assert r["brier"][0, 0] == 0.125 and r["hit_forecast"][0, 0] == 0.25 and r["hit_observed"][0, 0] == 0.5
    assert r["sign_accuracy"][0] == 0.75 and r["step_accuracy"][0] == 0.25 and r["sign_mass"][0] == 0.25
    assert r["pit_deviation"][0] == 0.0 and r["pit_deviation"][1] == 0.75 and np.isnan(r["pit_deviation"][2])
    assert r["pit_hist"][1].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert ME.rollout_steps(16) == [0, 7, 15] and ME.rollout_steps(4) == [0, 1, 3] and ME.rollout_steps(1) == [0]
    text = ME.rollout_summary_text(r)
    assert text.startswith("step 1: skill 0.750 | coverage 25.0%:25.0% 75.0%:75.0% | direction 75.0% | PIT dev 0.000")
    assert "step 3: no scored prompt" in text
    rm = ME.RolloutMetrics((0.25, 0.75))
    assert rm.result() == {} and rm.batches == 0
    for bad in (None, {}, {1: {"agg": None}}, [1]):
        with pytest.raises(ValueError):
            rm.add(bad)


def test_entry_refusals_need_no_device():
    import mmt_lib as ML
    L = ML.lib()
    assert L.mmt_horizon_score_scratch_bytes(1, 2, 4, 3) > 0
    assert L.mmt_horizon_score_scratch_bytes(2, 2, 4, 3) == 2 * L.mmt_horizon_score_scratch_bytes(1, 2, 4, 3)
    assert L.mmt_horizon_score_scratch_bytes(1, 2, 4, 3) > L.mmt_horizon_scratch_bytes(1, 2, 4, 3)
    for bad in ((-1, 2, 4, 3), (1, -1, 4, 3), (1, 2, 0, 3), (1, 2, 4097, 3), (1, 2, 4, -1), (1, 1 << 20, 1 << 11, 3)):
        assert L.mmt_horizon_score_scratch_bytes(*bad) == -1, bad
    for kw, rc in ((dict(bins=0), -1), (dict(bins=65), -1), (dict(batch=-1), -1), (dict(nq=17), -1),
                   (dict(tok_stride=2), -1), (dict(real_stride=2), -1), (dict(), -1),  # the last: null entries
                   (dict(batch=0), 0), (dict(count=0), 0)):
        assert null_call(L, **kw) == rc, kw


def null_call(L, count=1, batch=2, bins=10, nq=1, tok_stride=3, real_stride=3):
    """mmt_horizon_score with null device pointers: every case is settled before a pointer is followed or a kernel
    launched (a percent problem, 4 samples, 3 steps, one level, no barrier)."""
    import ctypes
    i32, c64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    nul = (vp * 1)(None)
    return L.mmt_horizon_score(None, count, batch, 4, 3, (i32 * 1)(5), nul, (c64 * 1)(tok_stride), nul, (i32 * 1)(1),
                               None, None, nul, (c64 * 1)(real_stride), None, None, None, nq, (f64 * 17)(*[0.5] * 17), 0,
                               None, nul, nul, None, bins, 0, nul, nul, None, nul, nul, None, nul, None, 0)
