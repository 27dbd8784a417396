"""mmt_pmf_stats (csrc/mmt_forecast.hip) on pmf rows made on the host, against forecast_ref.pmf_stats (fp64 numpy). No
forecast kernel runs here, so a failure names this kernel.

Rows (forecast_ref.stats_cases): dense rows, point masses at both ends, two-point rows whose prefix sum sits on the
levels 0.5 and 0.05, zeros, an unnormalised row (T = 3.7), a sparse row; V = 1 among the sizes. Vocabulary values
sorted, with and without runs of repeated entries; percent and value series; origins at both ends, in the middle and
out of range.

Tolerances: the stats to a relative 1e-12 of the numpy result (kernel and numpy sum the same fp64 terms in different
orders: at most V roundings of 2^-53 each, 1e-12 at V = 8193; the mean is the one sum with terms of both signs, and
test_forecast_ref_cpu.py shows that on these rows and values it never cancels below 1e-3 of the sum of its terms'
magnitudes, so the relative bound stands for it too). qtok equal to the reference's; where a prefix sum lies within 1e-12 T
of the level the next token with mass is accepted as well, for at most 1 % of the (row, level) cases
(test_forecast_ref_cpu.py checks the cap on these rows)."""
import ctypes

import numpy as np
import pytest
import torch

import forecast_ref as F
import mmt_lib as ML
import mmt_sample as MS

pytestmark = pytest.mark.gpu

LEVELS = (0.05, 0.5, 0.95)
RTOL = 1e-12


def run(problems, levels=LEVELS, pad=2):
    """problems: dicts with rows fp32 [rows, V] and optional values fp64 [V], is_percent, origin int64 [rows]. The
    pmf rows are handed in with a row stride of V + pad (the pad holds a large mass that must not be read) and the
    origins with stride 2. Returns [(stats [rows, 8], qtok [rows, nq])] after checking the guard rows."""
    dev = torch.device("cuda")
    nq, rows = len(levels), problems[0]["rows"].shape[0]
    st = MS.StatsLaunch([q["rows"].shape[1] for q in problems], [q["rows"].shape[1] + pad for q in problems],
                        [q.get("is_percent", False) for q in problems], levels)
    keep, outs = [], []
    for p, q in enumerate(problems):
        V = q["rows"].shape[1]
        padded = np.full((rows, V + pad), 1e6, dtype=np.float32)
        padded[:, :V] = q["rows"]
        t = torch.from_numpy(padded).to(dev)
        stats = torch.full((rows + 2, 8), -7.0, dtype=torch.float64, device=dev)
        qtok = torch.full((rows + 2, max(nq, 1)), -7, dtype=torch.int32, device=dev)
        keep += [t, stats, qtok]
        st.pmf[p], st.stats[p], st.qtok[p] = t.data_ptr(), stats[1].data_ptr(), qtok[1].data_ptr()
        if q.get("values") is not None:
            keep.append(torch.from_numpy(np.asarray(q["values"], dtype=np.float64)).to(dev))
            st.values[p] = keep[-1].data_ptr()
        if q.get("origin") is not None:
            o = torch.full((rows, 2), 10 ** 9, dtype=torch.int64, device=dev)  # the odd entries would be out of range
            o[:, 0] = torch.from_numpy(np.asarray(q["origin"], dtype=np.int64)).to(dev)
            keep.append(o)
            st.origin[p], st.origin_stride[p] = o.data_ptr(), 2
        outs.append((stats, qtok))
    st.run(ML.lib(), ML.stream_ptr(dev), rows)
    torch.cuda.synchronize()
    res = []
    for stats, qtok in outs:
        assert bool((stats[0] == -7.0).all()) and bool((stats[-1] == -7.0).all()), "wrote outside its stats rows"
        assert bool((qtok[0] == -7).all()) and bool((qtok[-1] == -7).all()), "wrote outside its qtok rows"
        res.append((stats[1:-1].cpu().numpy(), qtok[1:-1, :nq].cpu().numpy()))
    return res


def compare(got, q, levels=LEVELS, what=""):
    stats, qtok = got
    rows = q["rows"]
    amb = 0
    for r in range(len(rows)):
        origin = None if q.get("origin") is None else q["origin"][r]
        want, wt, alt = F.pmf_stats(rows[r], q.get("values"), q.get("is_percent", False), origin, levels)
        assert np.array_equal(np.isnan(stats[r]), np.isnan(want)), (what, r, stats[r], want)
        tol = RTOL * np.abs(want)
        ok = ~np.isnan(want)
        assert np.all(np.abs(stats[r][ok] - want[ok]) <= tol[ok]), (what, r, stats[r], want)
        good = (qtok[r] == wt) | (qtok[r] == alt)
        assert good.all(), (what, r, qtok[r], wt, alt)
        amb += int((wt != alt).sum())
    assert amb <= 0.01 * len(rows) * len(levels), (what, amb)
    return amb


@pytest.mark.parametrize("V", [1, 5, 13, 64, 65, 900, 8193])
def test_stats_match_numpy(V):
    """One launch of six problems over the same rows: no values; percent values; a value series with its origin at
    token 0, at V - 1, in the middle and out of range (per row), values with repeated entries; a percent series with
    repeated entries (exact zeros: the flat class)."""
    rows, names = F.stats_cases(V)
    n = len(rows)
    v, vr = F.stats_values(V), F.stats_values(V, repeated=True)
    spread = np.array([0, V - 1, V // 2, V, -1, 10 ** 9])[np.arange(n) % 6]
    problems = [
        dict(rows=rows),
        dict(rows=rows, values=v, is_percent=True),
        dict(rows=rows, values=v, is_percent=False, origin=np.zeros(n, dtype=np.int64)),
        dict(rows=rows, values=vr, is_percent=False, origin=np.full(n, V - 1)),
        dict(rows=rows, values=vr, is_percent=False, origin=spread),
        dict(rows=rows, values=vr, is_percent=True, origin=spread),
        dict(rows=rows, values=v, is_percent=False),  # a value series without origins: no direction
    ]
    got = run(problems)
    for p, q in enumerate(problems):
        amb = compare(got[p], q, what=f"V={V} problem {p}")
    print(f"pmf_stats V={V}: {n} rows x {len(problems)} problems, ambiguous levels {amb}")
    stats = got[4][0]
    bad_origin = ~((spread >= 0) & (spread < V))
    zero = np.array([nm == "zeros" for nm in names])
    assert np.isnan(stats[bad_origin][:, 4:7]).all() and not np.isnan(stats[~bad_origin & ~zero][:, 4:7]).any()
    assert np.isnan(got[6][0][:, 4:7]).all() and not np.isnan(got[5][0][~zero][:, 4:7]).any()
    assert (got[0][1][zero] == -1).all() and (got[0][0][zero][:, 0] == 0).all()


def test_many_levels_problem_chunks_and_the_public_wrapper():
    V = 144
    rows, names = F.stats_cases(V, seed=1)
    levels = tuple((k + 0.5) / 16 for k in range(16))
    v = F.stats_values(V, repeated=True, seed=1)
    problems = [dict(rows=rows, values=v, is_percent=bool(p % 2), origin=np.full(len(rows), (7 * p) % V))
                for p in range(9)]  # nine problems: two launches
    got = run(problems, levels)
    for p, q in enumerate(problems):
        compare(got[p], q, levels, what=f"chunk problem {p}")
    n = len(rows) // 4 * 4
    t = torch.from_numpy(rows[:n]).cuda().reshape(4, n // 4, V)
    org = torch.full((4, n // 4), 7, dtype=torch.int64, device="cuda")
    stats, qtok = MS.pmf_stats([t], values=[v], is_percent=True, origin=[org], quantiles=levels)
    assert stats[0].shape == (4, n // 4, 8) and qtok[0].shape == (4, n // 4, 16)
    assert np.array_equal(stats[0].reshape(-1, 8).cpu().numpy().view(np.int64), got[1][0][:n].view(np.int64))
    assert np.array_equal(qtok[0].reshape(-1, 16).cpu().numpy(), got[1][1][:n])
    with pytest.raises(ValueError):
        MS.pmf_stats([t], values=[v[::-1].copy()])
    with pytest.raises(ValueError):
        MS.pmf_stats([t], quantiles=(0.5, 1.0))


def test_refusals_write_nothing():
    V, rows = 13, 3
    dev = torch.device("cuda")
    L = ML.lib()
    pmf = torch.full((rows, V), 1.0 / V, dtype=torch.float32, device=dev)
    i32, i64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double

    def call(count=1, rows_=rows, V_=V, stride=V, nq=2, levels=(0.25, 0.75), pmf_=pmf, with_stats=True, with_qtok=True,
             arrays=True):
        stats = torch.full((rows, 8), -7.0, dtype=torch.float64, device=dev)
        qtok = torch.full((rows, 16), -7, dtype=torch.int32, device=dev)
        rc = L.mmt_pmf_stats(ML.stream_ptr(dev), count, rows_, (i32 * 1)(V_) if arrays else None,
                             (vp * 1)(pmf_.data_ptr() if pmf_ is not None else None), (i64 * 1)(stride), None, None, None,
                             None, nq, (f64 * 16)(*levels) if levels is not None else None,
                             (vp * 1)(stats.data_ptr() if with_stats else None),
                             (vp * 1)(qtok.data_ptr()) if with_qtok else None)
        torch.cuda.synchronize()
        return rc, bool((stats == -7.0).all()) and bool((qtok == -7).all())

    nan = float("nan")
    for kw in (dict(count=-1), dict(rows_=-1), dict(V_=0), dict(stride=V - 1), dict(nq=17), dict(nq=-1),
               dict(levels=(0.0, 0.5)), dict(levels=(0.5, 1.0)), dict(levels=(nan, 0.5)), dict(levels=(-0.1, 0.5)),
               dict(levels=None), dict(pmf_=None), dict(with_stats=False), dict(with_qtok=False), dict(arrays=False)):
        rc, clean = call(**kw)
        assert rc == -1 and clean, kw
    rc, clean = call(V_=(1 << 20) + 1, stride=1 << 21)
    assert rc == -2 and clean
    for kw in (dict(count=0), dict(rows_=0)):
        rc, clean = call(**kw)
        assert rc == 0 and clean, kw
    rc, clean = call(nq=0, with_qtok=False)  # no quantiles: qtok may be absent
    assert rc == 0
    rc, clean = call()
    assert rc == 0 and not clean
