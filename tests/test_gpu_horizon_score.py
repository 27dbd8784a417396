"""mmt_horizon_score (csrc/mmt_horizon_score.hip) on host-made tokens, against horizon_score_ref (fp64 numpy). No model
runs here, so a failure names these kernels.

Inputs (horizon_score_ref.case): horizon_ref.case's three prompts of S paths, a percent and a value problem per launch,
and per prompt and problem a realised row whose kind cycles over a copy of one of the prompt's paths, an independent
draw, a row below every path and a row above. Token rows with a stride of steps + 3 whose pad holds out-of-range tokens,
origins with stride 2, guard rows around every output and bytes behind the scratch. The forecast that is scored is the
device's own mmt_horizon_stats output on the same inputs.

Bounds (derived in horizon_score_ref's docstring). Always: x*, hi*, lo* as int64 bits; sc[3..5], pin and bs bit for bit
from the restatement applied to the device's stats / qval / hit; the four tables bit for bit from the restatement's rule
8 applied to the device's own records. Without weights the PIT exactly and the CRPS within 1e-12 relative; with weights
within crps_bound / pit_bound."""
import ctypes

import numpy as np
import pytest
import torch

import horizon_ref as H
import horizon_score_ref as HS
import mmt_lib as ML
import mmt_sample as MS

pytestmark = pytest.mark.gpu

BIG = 10 ** 9
TABLES = ("agg", "aggq", "aggb", "pit")


def launch(problems, B, S, N, logw=None, levels=H.LEVELS, barriers=H.BARRIERS, bins=10, pad=3, into=None,
           with_sc=True):
    """problems: dicts with tok int64 [B S, N], real int64 [B, N], values fp64 [V], pct and (value series) origin int64
    [B S] and real_origin int64 [B]. Runs mmt_horizon_stats, then mmt_horizon_score on its outputs. `into`: the
    guarded table tensors of an earlier call, to accumulate into. Returns (results, guarded): per problem a dict of
    numpy arrays (stats, qval, hit: the forecast; sc, pin, bs, agg, aggq, aggb, pit), after checking the guard rows
    around every output and the bytes behind the scratch."""
    dev = torch.device("cuda")
    R, nq, nb, P = B * S, len(levels), len(barriers), len(problems)
    V = [len(q["values"]) for q in problems]
    pct = [q["pct"] for q in problems]
    bars = [q.get("bars", barriers) for q in problems]
    hl = MS.HorizonLaunch(V, [N + pad] * P, pct, levels, bars)
    sl = MS.HorizonScoreLaunch(V, [N + pad] * P, [N + pad + 1] * P, pct, levels, bars, bins)
    f64 = dict(dtype=torch.float64, device=dev)
    keep, outs, fcs = [], [], []
    for p, q in enumerate(problems):
        t = torch.full((R, N + pad), BIG, dtype=torch.int64, device=dev)
        t[:, :N] = torch.from_numpy(np.ascontiguousarray(q["tok"])).to(dev)
        y = torch.full((B, N + pad + 1), -BIG, dtype=torch.int64, device=dev)
        y[:, :N] = torch.from_numpy(np.ascontiguousarray(q["real"])).to(dev)
        v = torch.from_numpy(np.asarray(q["values"], dtype=np.float64)).to(dev)
        o = torch.full((R, 2), BIG, dtype=torch.int64, device=dev)  # the odd entries would be out of range
        ro = torch.full((B, 3), BIG, dtype=torch.int64, device=dev)
        if not q["pct"]:
            o[:, 0] = torch.from_numpy(np.asarray(q["origin"], dtype=np.int64)).to(dev)
            ro[:, 0] = torch.from_numpy(np.asarray(q["real_origin"], dtype=np.int64)).to(dev)
            hl.origin[p], hl.origin_stride[p] = o.data_ptr(), 2
            sl.origin[p], sl.origin_stride[p] = o.data_ptr(), 2
            sl.real_origin[p], sl.real_origin_stride[p] = ro.data_ptr(), 3
        fc = {"stats": torch.full((B, N, 12), -7.0, **f64), "qval": torch.full((B, N, max(nq, 1)), -7.0, **f64),
              "qrow": torch.full((B, N, max(nq, 1)), -7, dtype=torch.int32, device=dev),
              "hit": torch.full((B, N, max(nb, 1)), -7.0, **f64)}
        if nq:  # the entry reads [B, N, nq]: give it that layout
            fc["qval"] = fc["qval"][:, :, :nq].contiguous()
            fc["qrow"] = fc["qrow"][:, :, :nq].contiguous()
        if nb:
            fc["hit"] = fc["hit"][:, :, :nb].contiguous()
        g = {"sc": torch.full((B + 2, N, 8), -7.0, **f64), "pin": torch.full((B + 2, N, max(nq, 1)), -7.0, **f64),
             "bs": torch.full((B + 2, N, max(nb, 1)), -7.0, **f64)}
        if into is None:
            g.update(agg=torch.full((N + 2, 10), -7.0, **f64), aggq=torch.full((N + 2, max(nq, 1), 2), -7.0, **f64),
                     aggb=torch.full((N + 2, max(nb, 1), 3), -7.0, **f64), pit=torch.full((N + 2, bins), -7.0, **f64))
        else:
            g.update({k: into[p][k] for k in TABLES})
        keep += [t, y, v, o, ro]
        hl.tok[p], hl.values[p] = t.data_ptr(), v.data_ptr()
        hl.stats[p] = fc["stats"].data_ptr()
        sl.tok[p], sl.values[p], sl.real[p] = t.data_ptr(), v.data_ptr(), y.data_ptr()
        sl.stats[p] = fc["stats"].data_ptr()
        if nq:
            hl.qval[p], hl.qrow[p] = fc["qval"].data_ptr(), fc["qrow"].data_ptr()
            sl.qval[p], sl.pin[p], sl.aggq[p] = fc["qval"].data_ptr(), g["pin"][1].data_ptr(), g["aggq"][1].data_ptr()
        if nb:
            hl.hit[p] = fc["hit"].data_ptr()
            sl.hit[p], sl.bs[p], sl.aggb[p] = fc["hit"].data_ptr(), g["bs"][1].data_ptr(), g["aggb"][1].data_ptr()
        if with_sc:
            sl.sc[p] = g["sc"][1].data_ptr()
        sl.agg[p], sl.pit[p] = g["agg"][1].data_ptr(), g["pit"][1].data_ptr()
        outs.append(g)
        fcs.append(fc)
    lw = None if logw is None else torch.from_numpy(np.asarray(logw, dtype=np.float64)).to(dev)
    lwp = lw.data_ptr() if lw is not None else 0
    L = ML.lib()
    nbytes = hl.scratch_bytes(L, B, S, N)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    hl.run(L, ML.stream_ptr(dev), B, S, N, lwp, scratch.data_ptr(), nbytes)
    nbytes = sl.scratch_bytes(L, B, S, N)
    scratch = torch.full((max(nbytes, 16) + 64,), 0x5a, dtype=torch.uint8, device=dev)
    sl.run(L, ML.stream_ptr(dev), B, S, N, lwp, scratch.data_ptr(), nbytes, accumulate=into is not None)
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0x5a).all()), "wrote behind its scratch"
    res = []
    for g, fc in zip(outs, fcs):
        for name, t in g.items():
            if into is None or name not in TABLES:
                assert bool((t[0] == -7).all()) and bool((t[-1] == -7).all()), f"wrote outside its {name} rows"
        if not nq:
            assert bool((g["pin"] == -7).all()) and bool((g["aggq"] == -7).all())
        if not nb:
            assert bool((g["bs"] == -7).all()) and bool((g["aggb"] == -7).all())
        if not with_sc:
            assert bool((g["sc"] == -7).all())
        res.append({"stats": fc["stats"].cpu().numpy(), "qval": fc["qval"][:, :, :nq].cpu().numpy(),
                    "hit": fc["hit"][:, :, :nb].cpu().numpy(), "sc": g["sc"][1:-1].cpu().numpy(),
                    "pin": g["pin"][1:-1, :, :nq].cpu().numpy(), "bs": g["bs"][1:-1, :, :nb].cpu().numpy(),
                    "agg": g["agg"][1:-1].cpu().numpy(), "aggq": g["aggq"][1:-1, :nq].cpu().numpy(),
                    "aggb": g["aggb"][1:-1, :nb].cpu().numpy(), "pit": g["pit"][1:-1].cpu().numpy()})
    return res, outs


def problems_of(c):
    return [dict(tok=c["tok"][0], real=c["real"][0], values=c["values"], pct=True),
            dict(tok=c["tok"][1], real=c["real"][1], values=c["values"], pct=False, origin=c["origin"],
                 real_origin=c["real_origin"])]


def i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b, keys=None):
    return all(np.array_equal(i64(x[k]), i64(y[k])) for x, y in zip(a, b) for k in (keys or x))


def check_tables(r, rz, B, bars, bins, what):
    """The four tables of one problem, bit for bit from rule 8 applied to the device's own records."""
    ref = HS.tables(r["sc"], r["pin"], r["bs"], r["stats"], r["qval"], r["hit"], rz[3], bars, bins)
    for name, t in zip(TABLES, ref):
        assert np.array_equal(i64(r[name]), i64(t)), (what, name, r[name], t)


def compare(r, paths, rz, logw, S, levels, bars, bins, what):
    """One problem's records and tables; returns the largest (CRPS error / bound, PIT error / bound) with weights."""
    B = r["sc"].shape[0]
    weighted = logw is not None
    worst = [0.0, 0.0]
    for b in range(B):
        sl = slice(b * S, (b + 1) * S)
        ref = HS.records(paths[0][sl], logw[sl] if weighted else None, paths[4][sl], [t[b] for t in rz], r["stats"][b],
                         r["qval"][b], r["hit"][b], levels, bars)
        sc, w = r["sc"][b], f"{what} prompt {b}"
        if np.isnan(ref["sc"][:, 0]).all():
            assert np.isnan(sc).all() and np.isnan(r["pin"][b]).all() and np.isnan(r["bs"][b]).all(), w
            continue
        for k in (0, 3, 4, 5, 6, 7):
            assert np.array_equal(i64(sc[:, k]), i64(ref["sc"][:, k])), (w, "sc", k, sc[:, k], ref["sc"][:, k])
        assert np.array_equal(i64(r["pin"][b]), i64(ref["pin"])), (w, "pin")
        assert np.array_equal(i64(r["bs"][b]), i64(ref["bs"])), (w, "bs")
        ec, ep = np.abs(sc[:, 1] - ref["sc"][:, 1]), np.abs(sc[:, 2] - ref["sc"][:, 2])
        print(f"{w}: crps err {ec.max():.3e} bound {ref['crps_bound'].max():.3e}; "
              f"pit err {ep.max():.3e} bound {ref['pit_bound'].max():.3e}")
        assert (sc[:, 1] >= 0).all() and (ec <= ref["crps_bound"]).all(), (w, "crps", sc[:, 1], ref["sc"][:, 1])
        if not weighted:
            assert np.array_equal(i64(sc[:, 2]), i64(ref["sc"][:, 2])), (w, "pit", sc[:, 2], ref["sc"][:, 2])
        else:
            assert (ep <= ref["pit_bound"]).all(), (w, "pit", sc[:, 2], ref["sc"][:, 2])
            with np.errstate(all="ignore"):
                for i, (e, bd) in enumerate(((ec, ref["crps_bound"]), (ep, ref["pit_bound"]))):
                    ratio = np.where(e > 0, e / np.where(bd > 0, bd, 1.0), 0.0)
                    worst[i] = max(worst[i], float(ratio.max()))
    check_tables(r, rz, B, bars, bins, what)
    return worst


@pytest.mark.parametrize("S", HS.SAMPLES)
def test_matches_numpy(S):
    worst = {}
    for N in HS.STEPS:
        for V in H.VS:
            for sigma in H.SIGMAS:
                c = HS.case(S, N, V, sigma)
                res, _ = launch(problems_of(c), H.PROMPTS, S, N, c["logw"])
                for p in range(2):
                    paths = H.paths(c["tok"][p], c["values"], p == 0, c["origin"])
                    w = compare(res[p], paths, c["rz"][p], c["logw"], S, H.LEVELS, H.BARRIERS, 10,
                                f"S={S} N={N} V={V} sigma={sigma} p={p}")
                    if sigma is not None:
                        old = worst.get(sigma, [0.0, 0.0])
                        worst[sigma] = [max(old[0], w[0]), max(old[1], w[1])]
    print(f"horizon score S={S}: largest error / bound (CRPS, PIT) " +
          ", ".join(f"sigma {k}: {v[0]:.3f}, {v[1]:.3f}" for k, v in worst.items()))


def test_dead_realised_rows_an_all_dead_prompt_and_a_token_outside_the_vocabulary():
    S, N, V = 65, 3, 144
    c = HS.case(S, N, V, 8.0, 2)
    tok = [t.copy() for t in c["tok"]]
    real = [t.copy() for t in c["real"]]
    origin, real_origin = c["origin"].copy(), c["real_origin"].copy()
    tok[0][5, 1] = V              # prompt 0: a path token past the vocabulary, in the percent problem only
    tok[1][7, 2] = -1             # and a negative one in the value problem
    real[0][1, N - 1] = V         # prompt 1: the realised row's last token is out of range (percent problem)
    real_origin[0] = -1           # prompt 0: a bad realised origin (value problem)
    tok[0][2 * S:] = BIG          # prompt 2: all paths dead in the percent problem
    probs = [dict(tok=tok[0], real=real[0], values=c["values"], pct=True),
             dict(tok=tok[1], real=real[1], values=c["values"], pct=False, origin=origin, real_origin=real_origin)]
    res, _ = launch(probs, H.PROMPTS, S, N, c["logw"])
    for p in range(2):
        paths = H.paths(tok[p], c["values"], p == 0, origin)
        rz = HS.realised(real[p], c["values"], p == 0, real_origin)
        compare(res[p], paths, rz, c["logw"], S, H.LEVELS, H.BARRIERS, 10, f"dead p={p}")
    for p, b in ((0, 1), (0, 2), (1, 0)):
        assert np.isnan(res[p]["sc"][b]).all() and np.isnan(res[p]["pin"][b]).all() and np.isnan(res[p]["bs"][b]).all()
    assert (res[0]["agg"][:, 0] == 1).all() and (res[1]["agg"][:, 0] == 2).all()  # dead (b, j) enter no table
    assert (res[0]["pit"].sum(axis=1) == 1).all() and (res[1]["pit"].sum(axis=1) == 2).all()
    # a dead path changes nothing else: the same bits as the intact row with weight zero
    lw = c["logw"].copy()
    lw[[5]] = -np.inf
    ref, _ = launch(problems_of(c), H.PROMPTS, S, N, lw)
    assert same([{k: res[0][k][0] for k in ("sc", "pin", "bs")}], [{k: ref[0][k][0] for k in ("sc", "pin", "bs")}])


def test_accumulate_over_two_calls_is_the_sum():
    S, N, V = 17, 5, 900
    c1, c2 = HS.case(S, N, V, 0.3, 3), HS.case(S, N, V, 0.3, 4)
    one, g = launch(problems_of(c1), H.PROMPTS, S, N, c1["logw"])
    two, _ = launch(problems_of(c2), H.PROMPTS, S, N, c2["logw"])
    both, _ = launch(problems_of(c2), H.PROMPTS, S, N, c2["logw"], into=g)
    for p in range(2):
        for k in TABLES:
            assert np.array_equal(i64(both[p][k]), i64(one[p][k] + two[p][k])), (p, k)
        assert (both[p]["agg"][:, 0] == 2 * H.PROMPTS).all()
        assert same([both[p]], [two[p]], ("sc", "pin", "bs"))


def test_alone_is_in_company_nine_problems_and_runs_repeat():
    S, N, V = 257, 33, 5
    c = HS.case(S, N, V, 0.3)
    probs = problems_of(c)
    res, _ = launch(probs, H.PROMPTS, S, N, c["logw"])
    again, _ = launch(probs, H.PROMPTS, S, N, c["logw"])
    assert same(res, again)  # run to run
    for b in range(H.PROMPTS):
        sl = slice(b * S, (b + 1) * S)
        one = [dict(q, tok=q["tok"][sl], real=q["real"][b:b + 1], origin=c["origin"][sl],
                    real_origin=c["real_origin"][b:b + 1]) for q in probs]
        alone, _ = launch(one, 1, S, N, c["logw"][sl])  # batch 1
        for p in range(2):
            for k in ("sc", "pin", "bs"):
                assert np.array_equal(i64(alone[p][k][0]), i64(res[p][k][b])), (b, p, k)
            check_tables(alone[p], [t[b:b + 1] for t in c["rz"][p]], 1, H.BARRIERS, 10, f"alone b={b} p={p}")
    for p in range(2):
        solo, _ = launch([probs[p]], H.PROMPTS, S, N, c["logw"])
        assert same(solo, [res[p]])
    nine, _ = launch([probs[p % 2] for p in range(9)], H.PROMPTS, S, N, c["logw"])  # two chunks of problems
    for p in range(9):
        assert same([nine[p]], [res[p % 2]]), p
    # the records in the scratch: the same tables, the sc buffer untouched
    hidden, _ = launch(probs, H.PROMPTS, S, N, c["logw"], with_sc=False)
    assert same(hidden, res, ("pin", "bs") + TABLES)


@pytest.mark.parametrize("bins", [1, 10, 64])
def test_bins(bins):
    S, N, V = 16, 2, 900
    c = HS.case(S, N, V, None, 5)
    res, _ = launch(problems_of(c), H.PROMPTS, S, N, None, bins=bins)
    for p in range(2):
        paths = H.paths(c["tok"][p], c["values"], p == 0, c["origin"])
        compare(res[p], paths, c["rz"][p], None, S, H.LEVELS, H.BARRIERS, bins, f"bins={bins} p={p}")
        assert res[p]["pit"].shape == (N, bins) and (res[p]["pit"].sum(axis=1) == res[p]["agg"][:, 0]).all()


def test_no_quantiles_no_barriers_and_no_steps():
    S, N, V = 15, 2, 5
    c = HS.case(S, N, V, 0.3, 6, (), ())
    res, _ = launch(problems_of(c), H.PROMPTS, S, N, c["logw"], (), ())  # qval / hit / pin / bs / aggq / aggb NULL
    for p in range(2):
        paths = H.paths(c["tok"][p], c["values"], p == 0, c["origin"])
        compare(res[p], paths, c["rz"][p], c["logw"], S, (), (), 10, f"bare p={p}")
    probs = [dict(q, tok=q["tok"][:, :0], real=q["real"][:, :0]) for q in problems_of(c)]
    launch(probs, H.PROMPTS, S, 0, c["logw"])  # steps 0: launches nothing, the guards hold


def test_the_public_wrapper():
    S, N, V = 64, 5, 900
    c = HS.case(S, N, V, 0.3, 1, H.LEVELS16, H.BARRIERS8)
    res, _ = launch(problems_of(c), H.PROMPTS, S, N, c["logw"], H.LEVELS16, H.BARRIERS8, bins=7)
    dev = torch.device("cuda")
    toks = [torch.from_numpy(t).to(dev) for t in c["tok"]]
    real = [torch.from_numpy(t).to(dev) for t in c["real"]]
    kw = dict(samples=S, values=[c["values"]] * 2, is_percent=[True, False],
              origin=[None, torch.from_numpy(c["origin"]).to(dev)], logw=torch.from_numpy(c["logw"]).to(dev),
              quantiles=H.LEVELS16, barriers=[H.BARRIERS8] * 2)
    hz = MS.horizon_stats(toks, **kw)
    ro = [None, torch.from_numpy(c["real_origin"]).to(dev)]
    sc = MS.horizon_score(toks, real, realised_origin=ro, forecast=hz, bins=7, **kw)
    for p in range(2):
        d = sc[p]
        assert d["crps"].shape == (3, N) and d["pinball"].shape == (3, N, 16) and d["brier"].shape == (3, N, 8)
        got = {"sc": torch.stack([d[k] for k in MS.SCORE_FIELDS], dim=-1).cpu().numpy(),
               "pin": d["pinball"].cpu().numpy(), "bs": d["brier"].cpu().numpy(), "agg": d["agg"].cpu().numpy(),
               "aggq": d["aggq"].cpu().numpy(), "aggb": d["aggb"].cpu().numpy(), "pit": d["pit_hist"].cpu().numpy()}
        assert same([got], [res[p]], tuple(got))
    with pytest.raises(ValueError):
        MS.horizon_score(toks, real, realised_origin=ro, forecast=hz, bins=65, **kw)
    with pytest.raises(ValueError):
        MS.horizon_score(toks, real, realised_origin=None, forecast=hz, **kw)  # a value series, no realised origin
    with pytest.raises(ValueError):
        MS.horizon_score(toks, real[:1], realised_origin=ro, forecast=hz, **kw)
    with pytest.raises(ValueError):
        MS.horizon_score(toks, [t[:2] for t in real], realised_origin=ro, forecast=hz, **kw)
    with pytest.raises(ValueError):
        MS.horizon_score(toks, real, realised_origin=ro, forecast=hz[:1], **kw)
    with pytest.raises(ValueError):
        MS.horizon_score(toks, real, realised_origin=ro, forecast=hz, **dict(kw, quantiles=H.LEVELS))


def test_refusals_write_nothing():
    B, S, N, V = 2, 4, 3, 13
    dev = torch.device("cuda")
    L = ML.lib()
    i32, c64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    tok = torch.zeros(B * S, N, dtype=torch.int64, device=dev)
    real = torch.zeros(B, N, dtype=torch.int64, device=dev)
    val = torch.linspace(-1, 1, V, dtype=torch.float64, device=dev)
    org = torch.zeros(B * S, dtype=torch.int64, device=dev)
    rorg = torch.zeros(B, dtype=torch.int64, device=dev)
    fc = [torch.zeros(B * N * 16, dtype=torch.float64, device=dev) for _ in range(3)]
    need = L.mmt_horizon_score_scratch_bytes(1, B, S, N)
    assert need > 0
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")
    NAMES = ("sc", "pin", "bs", "agg", "aggq", "aggb", "pit")

    def call(count=1, batch=B, samples=S, steps=N, V_=V, stride=N, rstride=N, pct=0, nq=2, levels=(0.25, 0.75), nb=2,
             bars=(1.0, -1.0), bins=10, tok_=tok, real_=real, val_=val, org_=org, rorg_=rorg, arrays=True,
             bar_array=True, null=(), null_array=(), sc=0, nbytes=need):
        outs = {k: torch.full((B * N * 64,), -7.0, dtype=torch.float64, device=dev) for k in NAMES}
        barr = (f64 * 8)(*bars)
        ins = dict(stats=fc[0], qval=fc[1], hit=fc[2])

        def arr(name, t):
            if name in null_array:
                return None
            return (vp * 1)(None if name in null or t is None else t.data_ptr())

        rc = L.mmt_horizon_score(
            ML.stream_ptr(dev), count, batch, samples, steps, (i32 * 1)(V_) if arrays else None, arr("tok", tok_),
            (c64 * 1)(stride), arr("values", val_), (i32 * 1)(pct), arr("origin", org_) if org_ is not None else None,
            (c64 * 1)(1), arr("real", real_), (c64 * 1)(rstride),
            arr("real_origin", rorg_) if rorg_ is not None else None, (c64 * 1)(1), None, nq,
            (f64 * 16)(*levels) if levels is not None else None, nb,
            (vp * 1)(ctypes.addressof(barr)) if bar_array else None, arr("stats", ins["stats"]),
            arr("qval", ins["qval"]), arr("hit", ins["hit"]), bins, 0, *[arr(k, outs[k]) for k in NAMES],
            scratch.data_ptr() + sc if sc is not None else None, nbytes)
        torch.cuda.synchronize()
        clean = all(bool((t == -7).all()) for t in outs.values())
        return rc, clean

    for kw in (dict(count=-1), dict(batch=-1), dict(steps=-1), dict(samples=0), dict(batch=1 << 20, samples=1 << 11),
               dict(nq=17), dict(nq=-1), dict(nb=9), dict(nb=-1), dict(levels=(0.0, 0.5)), dict(levels=(0.5, 1.0)),
               dict(levels=(nan, 0.5)), dict(levels=None), dict(bars=(0.0, 1.0)), dict(bars=(nan, 1.0)),
               dict(bars=(1.0, -inf)), dict(bins=0), dict(bins=65), dict(V_=0), dict(stride=N - 1),
               dict(rstride=N - 1), dict(arrays=False), dict(tok_=None), dict(real_=None), dict(val_=None),
               dict(org_=None), dict(rorg_=None), dict(bar_array=False), dict(sc=None), dict(sc=8),
               dict(nbytes=need - 1)) + tuple(dict(null=(k,)) for k in ("stats", "qval", "hit") + NAMES[1:]) + tuple(
                   dict(null_array=(k,)) for k in ("tok", "values", "real", "stats", "qval", "hit") + NAMES[1:]):
        rc, clean = call(**kw)
        assert rc == -1 and clean, kw
    for kw in (dict(V_=(1 << 20) + 1), dict(batch=1, samples=4097, nbytes=1 << 40)):
        rc, clean = call(**kw)
        assert rc == -2 and clean, kw
    assert L.mmt_horizon_score_scratch_bytes(1, 1, 4097, N) == -1
    assert L.mmt_horizon_score_scratch_bytes(1, B, S, -1) == -1
    for kw in (dict(count=0), dict(batch=0), dict(steps=0)):
        rc, clean = call(**kw)
        assert rc == 0 and clean, kw
    rc, clean = call(pct=1, org_=None, rorg_=None)  # a percent series needs no origins
    assert rc == 0 and not clean
    rc, clean = call(nq=0, nb=0, bar_array=False, null_array=("qval", "hit", "pin", "bs", "aggq", "aggb"))
    assert rc == 0 and not clean
    rc, clean = call(null=("sc",))  # the records may live in the scratch
    assert rc == 0 and not clean
    rc, clean = call(null_array=("sc",))
    assert rc == 0 and not clean
