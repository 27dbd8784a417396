"""mmt_horizon_joint (csrc/mmt_horizon_joint.hip) on host-made tokens, against horizon_joint_ref (fp64 numpy). No model
runs here, so a failure names these kernels.

Inputs (horizon_joint_ref.case / GRID): three prompts of S paths, 2, 3 or 8 problems (even ones percent series, odd ones
value series), tokens uniform in 0..V-1; no weights, N(0, 0.3^2) and N(0, 8^2) log-weights (prompt 1 shifted by -50,
-inf rows in prompt 2). Per size S an orthogonal array over steps {1, 2, 33} x count {2, 3, 8} x V {1, 5, 900} x the three
weightings, with 8 baskets and every pair, one basket and no pair, or pairs only. Token rows are handed in with a stride
of steps + 3 whose pad holds out-of-range tokens, origins with stride 2, outputs between guard rows.

Bounds: horizon_joint_ref's docstring derives them. Without weights bqrow / bqval (as int64 bits) and min / max equal
the reference's; sums within a relative 1e-12 of their sums of magnitudes; with weights 2 EPS more, EPS = 4 * 2^-24, and
an ambiguous quantile may be the row across its boundary, for at most max(1, 2 %) of a basket's triples
(test_horizon_joint_ref_cpu.py asserts the cap, and which corr cells go uncompared, on these inputs)."""
import ctypes

import numpy as np
import pytest
import torch

import horizon_joint_ref as J
import horizon_ref as H
import mmt_lib as ML
import mmt_sample as MS

pytestmark = pytest.mark.gpu

BIG = 10 ** 9
i32, i64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double


def launch(problems, coefs, barriers, pairs, B, S, N, logw=None, levels=J.LEVELS, pad=3):
    """One raw mmt_horizon_joint call. Returns {"ess", "live" [B], "bstats" [K][B, N, 9], "bqval", "bqrow", "btail" [K][B,
    N, nq], "bhit" [K][B, N, nb], "pstats" [NP][B, N, 22]} as numpy, after checking the guard rows around every output."""
    dev = torch.device("cuda")
    R, P, K, NP, nq = B * S, len(problems), len(coefs), len(pairs), len(levels)
    nb = len(barriers[0]) if barriers else 0
    toks, vals, orgs = [], [], []
    for q in problems:
        t = torch.full((R, N + pad), BIG, dtype=torch.int64, device=dev)
        t[:, :N] = torch.from_numpy(np.ascontiguousarray(q["tok"])).to(dev)
        o = torch.full((R, 2), BIG, dtype=torch.int64, device=dev)  # the odd entries would be out of range
        if not q["pct"]:
            o[:, 0] = torch.from_numpy(np.asarray(q["origin"], dtype=np.int64)).to(dev)
        toks.append(t), orgs.append(o)
        vals.append(torch.from_numpy(np.asarray(q["values"], dtype=np.float64)).to(dev))

    def guarded(n, last, dt=torch.float64):
        return [torch.full((B + 2, N, max(last, 1)), -7, dtype=dt, device=dev) for _ in range(n)]

    g = {"bstats": guarded(K, 9), "bqval": guarded(K, nq), "bqrow": guarded(K, nq, torch.int32),
         "btail": guarded(K, nq), "bhit": guarded(K, nb), "pstats": guarded(NP, 22)}
    ess = torch.full((B + 2,), -7.0, dtype=torch.float64, device=dev)
    live = torch.full((B + 2,), -7, dtype=torch.int32, device=dev)
    ptrs = lambda ts: (vp * max(1, len(ts)))(*[t[1].data_ptr() for t in ts])  # noqa: E731
    lw = None if logw is None else torch.from_numpy(np.asarray(logw, dtype=np.float64)).to(dev)
    L = ML.lib()
    nbytes = L.mmt_horizon_joint_scratch_bytes(P, B, S, N, K)
    assert nbytes >= 0
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    rc = L.mmt_horizon_joint(
        ML.stream_ptr(dev), P, B, S, N, (i32 * P)(*[len(q["values"]) for q in problems]),
        (vp * P)(*[t.data_ptr() for t in toks]), (i64 * P)(*[N + pad] * P), (vp * P)(*[v.data_ptr() for v in vals]),
        (i32 * P)(*[1 if q["pct"] else 0 for q in problems]),
        (vp * P)(*[None if q["pct"] else o.data_ptr() for q, o in zip(problems, orgs)]), (i64 * P)(*[2] * P),
        lw.data_ptr() if lw is not None else None, nq, (f64 * max(1, nq))(*levels), K,
        (f64 * max(1, K * P))(*[a for row in coefs for a in row]), nb,
        (f64 * max(1, K * nb))(*[u for row in barriers for u in row]), NP,
        (i32 * max(1, 2 * NP))(*[i for pq in pairs for i in pq]), ptrs(g["bstats"]),
        ptrs(g["bqval"]) if nq else None, ptrs(g["bqrow"]) if nq else None, ptrs(g["btail"]) if nq else None,
        ptrs(g["bhit"]) if nb else None, ptrs(g["pstats"]), ess[1:].data_ptr(), live[1:].data_ptr(),
        scratch.data_ptr(), nbytes)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, ts in list(g.items()) + [("ess", [ess]), ("live", [live])]:
        for t in ts:
            assert bool((t[0] == -7).all()) and bool((t[-1] == -7).all()), f"wrote outside its {name} rows"
    cut = {"bstats": 9, "bqval": nq, "bqrow": nq, "btail": nq, "bhit": nb, "pstats": 22}
    res = {name: [t[1:-1, :, :cut[name]].cpu().numpy() for t in ts] for name, ts in g.items()}
    res.update(ess=ess[1:-1].cpu().numpy(), live=live[1:-1].cpu().numpy())
    return res


def run_case(c, **kw):
    return launch(c["problems"], c["coefs"], c["barriers"], c["pairs"], J.PROMPTS, c["S"], c["N"], c["logw"], **kw)


def at(res, b):
    return {k: (v[b] if k in ("ess", "live") else [t[b] for t in v]) for k, v in res.items()}


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(x, y):
    """Two results (or two prompts of results) hold the same bits."""
    for k in x:
        xs, ys = (x[k], y[k]) if isinstance(x[k], list) else ([x[k]], [y[k]])
        if len(xs) != len(ys) or not all(np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))) for a, b in zip(xs, ys)):
            return False
    return True


def compare(res, refs, weighted, what):
    """A case's prompts; asserts the cap on ambiguous triples per basket and returns the worst error / bound."""
    worst, amb = 0.0, None
    for b, r in enumerate(refs):
        a, w = J.check(at(res, b), r, weighted, f"{what} prompt {b}")
        amb = a if amb is None else [x + y for x, y in zip(amb, a)]
        worst = max(worst, w)
    for k, n in enumerate(amb if weighted else []):
        assert n <= J.cap(J.ambiguous(refs, k)[1]), (what, k, n)
    return worst


@pytest.mark.parametrize("S", J.SAMPLES)
def test_matches_numpy(S):
    worst = {}
    for N, count, V, sigma, cfg in J.GRID[S]:
        c = J.case(S, N, count, V, sigma, cfg)
        w = compare(run_case(c), c["ref"], sigma is not None, f"S={S} N={N} count={count} V={V} sigma={sigma} {cfg}")
        worst[sigma] = max(worst.get(sigma, 0.0), w)
    print(f"horizon joint S={S}: largest error / bound " + ", ".join(f"sigma {k}: {v:.3f}" for k, v in worst.items()))


def test_a_row_dead_in_one_series_is_dead_everywhere_and_an_all_dead_prompt():
    S, N, count, V = 65, 3, 3, 144
    problems = [dict(q, tok=q["tok"].copy(), origin=q["origin"].copy()) for q in J.problems_for(S, N, count, V, 2)]
    coefs, barriers, pairs = J.config("full", count)
    a = J.F.log_weights(S, 8.0, 2).reshape(-1)
    problems[0]["tok"][5, 1] = V            # prompt 0: a token past the vocabulary in series 0 only
    problems[1]["tok"][7, 2] = -1           # a negative one in series 1 only
    problems[1]["origin"][S + 9] = V        # prompt 1: a bad origin of the value series
    problems[2]["tok"][2 * S:] = BIG        # prompt 2: all dead, through series 2 alone
    res = launch(problems, coefs, barriers, pairs, J.PROMPTS, S, N, a)
    refs = J.reference(problems, S, coefs, barriers, pairs, a)
    assert refs[0]["live"] < S and refs[2]["live"] == 0
    compare(res, refs, True, "dead")
    assert res["live"][2] == 0 and res["ess"][2] == 0
    # a dead row changes nothing else: the same bits as the intact rows with weight zero, in every basket and pair
    intact = J.problems_for(S, N, count, V, 2)
    lw = a.copy()
    lw[[5, 7, S + 9]] = -np.inf
    ref = launch(intact, coefs, barriers, pairs, J.PROMPTS, S, N, lw)
    for b in range(2):
        assert same(at(res, b), at(ref, b)), b
    # a basket that overflows kills its rows for every basket and pair of the call
    # (the last value of series 1 is 1e300: x stays finite, 1e10 x does not; the rows that survive hold ordinary numbers)
    intact[1]["values"] = intact[1]["values"].copy()
    intact[1]["values"][-1] = 1e300
    huge = [[0.0, 1e10, 0.0]] + coefs[:1]
    res = launch(intact, huge, barriers[:2], pairs, J.PROMPTS, S, N, a)
    refs = J.reference(intact, S, huge, barriers[:2], pairs, a)
    with np.errstate(all="ignore"):  # without the basket those rows live, and their 1e300 overflows the pair sums
        assert sum(r["live"] for r in refs) < sum(r["live"] for r in J.reference(intact, S, coefs[:1], barriers[:1], [], a))
    compare(res, refs, True, "overflow")


def test_alone_is_in_company_and_runs_repeat():
    S, N, count, V = 257, 33, 3, 5
    c = J.case(S, N, count, V, 0.3, "full")
    res = run_case(c)
    assert same(res, run_case(c))  # run to run
    for b in range(J.PROMPTS):  # a prompt alone
        sl = slice(b * S, (b + 1) * S)
        one = [dict(q, tok=q["tok"][sl], origin=q["origin"][sl]) for q in c["problems"]]
        alone = launch(one, c["coefs"], c["barriers"], c["pairs"], 1, S, N, c["logw"][sl])
        assert same(at(alone, 0), at(res, b)), b
    for k in (0, 3, 7):  # a basket alone, and with no pair
        alone = launch(c["problems"], [c["coefs"][k]], [c["barriers"][k]], [], J.PROMPTS, S, N, c["logw"])
        for name in ("bstats", "bqval", "bqrow", "btail", "bhit"):
            assert np.array_equal(bits(alone[name][0]), bits(res[name][k])), (k, name)
        assert same({"ess": alone["ess"], "live": alone["live"]}, {"ess": res["ess"], "live": res["live"]})
    for k in (0, 2):  # a pair alone, and with no basket
        alone = launch(c["problems"], [], [], [c["pairs"][k]], J.PROMPTS, S, N, c["logw"])
        assert np.array_equal(bits(alone["pstats"][0]), bits(res["pstats"][k])), k
        assert same({"ess": alone["ess"], "live": alone["live"]}, {"ess": res["ess"], "live": res["live"]})
    # no weights, no quantiles, no barriers: the optional outputs may be absent
    bare = launch(c["problems"], c["coefs"], [[]] * 8, c["pairs"], J.PROMPTS, S, N, None, ())
    compare(bare, J.reference(c["problems"], S, c["coefs"], [[]] * 8, c["pairs"], None, ()), False, "bare")


def test_unit_baskets_and_pair_variances_carry_horizon_stats_bits_and_the_public_wrapper():
    S, N, count, V = 64, 5, 3, 900
    c = J.case(S, N, count, V, 0.3, "full", 1)
    res = run_case(c)
    dev = torch.device("cuda")
    toks = [torch.from_numpy(q["tok"]).to(dev) for q in c["problems"]]
    kw = dict(samples=S, values=[q["values"] for q in c["problems"]], is_percent=[q["pct"] for q in c["problems"]],
              origin=[None if q["pct"] else torch.from_numpy(q["origin"]).to(dev) for q in c["problems"]],
              logw=torch.from_numpy(c["logw"]).to(dev), quantiles=J.LEVELS)
    hz = MS.horizon_stats(toks, barriers=[H.BARRIERS8] * count, **kw)
    units = [[1.0 if i == p else 0.0 for i in range(count)] for p in range(count)]
    jt = MS.horizon_joint(toks, baskets=[{"weights": u, "barriers": H.BARRIERS8} for u in units], pairs="all", **kw)
    eq = lambda x, y: torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,  # noqa: E731
                                  y.view(torch.int64) if y.dtype == torch.float64 else y)
    for p in range(count):
        b, d = jt["baskets"][p], hz[p]
        for name in ("mean", "var", "p_down", "p_flat", "p_up", "mean_high", "mean_low", "min", "max", "hit",
                     "quantile_values"):
            assert eq(b[name].contiguous(), d[name].contiguous()), (p, name)
        assert torch.equal(b["quantile_rows"], d["quantile_paths"])
        assert eq(jt["ess"], d["ess"]) and torch.equal(jt["live"], d["live"])
    assert sorted(jt["pairs"]) == [(0, 1), (0, 2), (1, 2)]
    for (p, q), d in jt["pairs"].items():
        assert eq(d["var_p"].contiguous(), hz[p]["var"].contiguous()), (p, q)
        assert eq(d["var_q"].contiguous(), hz[q]["var"].contiguous()), (p, q)
        assert d["sign_table"].shape == (3, N, 3, 3) and d["step_table"].shape == (3, N, 3, 3)
        # each table's row and column sums are that series' masses, to rounding
        for table, names in ((d["sign_table"], ("p_down", "p_flat", "p_up")),
                             (d["step_table"], ("step_down", "step_flat", "step_up"))):
            mp = torch.stack([hz[p][n] for n in names], dim=-1)
            mq = torch.stack([hz[q][n] for n in names], dim=-1)
            assert torch.allclose(table.sum(dim=3), mp, rtol=0, atol=1e-12)
            assert torch.allclose(table.sum(dim=2), mq, rtol=0, atol=1e-12)
    # the wrapper is the raw call: basket 0 of the case is the unit basket on series 0, its pairs start at (0, 1)
    assert np.array_equal(bits(jt["baskets"][0]["stats"].cpu().numpy()), bits(res["bstats"][0]))
    assert np.array_equal(bits(jt["baskets"][0]["tail_means"].cpu().numpy()), bits(res["btail"][0]))
    assert c["pairs"][0] == (0, 1)
    got = torch.cat([jt["pairs"][(0, 1)][k].reshape(3, N, -1) for k in ("cov", "corr", "var_p", "var_q", "sign_table",
                                                                       "step_table")], dim=-1).cpu().numpy()
    assert np.array_equal(bits(got), bits(res["pstats"][0]))
    # barrier lists of unequal length: padded for the call, their columns cut from the result
    jt2 = MS.horizon_joint(toks, baskets=[{"weights": units[0], "barriers": [0.5]}, {"weights": units[1]}], **kw)
    assert jt2["baskets"][0]["hit"].shape == (3, N, 1) and jt2["baskets"][1]["hit"].shape == (3, N, 0)
    assert eq(jt2["baskets"][0]["hit"][..., 0].contiguous(), hz[0]["hit"][..., 0].contiguous()) and not jt2["pairs"]
    with pytest.raises(ValueError):
        MS.horizon_joint(toks, baskets=[{"weights": [0.0] * count}], **kw)
    with pytest.raises(ValueError):
        MS.horizon_joint(toks, pairs=[(0, 0)], **kw)
    with pytest.raises(ValueError):
        MS.horizon_joint(toks, pairs=[(0, count)], **kw)


def test_refusals_write_nothing():
    B, S, N, V, P = 2, 4, 3, 13, 2
    dev = torch.device("cuda")
    L = ML.lib()
    tok = torch.zeros(B * S, N, dtype=torch.int64, device=dev)
    val = torch.linspace(-1, 1, V, dtype=torch.float64, device=dev)
    org = torch.zeros(B * S, dtype=torch.int64, device=dev)
    need = L.mmt_horizon_joint_scratch_bytes(P, B, S, N, 2)
    assert need > 0
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")

    def call(count=P, batch=B, samples=S, steps=N, V_=V, stride=N, pct=0, nq=2, levels=(0.25, 0.75), nbk=2,
             coef=(1.0, 0.0, 0.5, -0.5), nb=2, bars=(1.0, -1.0, 2.0, -2.0), npair=1, pairs=(0, 1), tok_=tok, val_=val,
             org_=org, arrays=True, with_coef=True, with_bars=True, with_pairs=True, with_ess=True,
             missing=(), null_entry=(), sc=0, nbytes=need):
        outs = {k: torch.full((B * N * 32,), -7.0, dtype=torch.float64, device=dev)
                for k in ("bstats", "bqval", "btail", "bhit", "pstats")}
        outs["bqrow"] = torch.full((B * N * 32,), -7, dtype=torch.int32, device=dev)
        ess = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
        live = torch.full((B,), -7, dtype=torch.int32, device=dev)
        n = max(count, 1)

        def out(name):
            if name in missing:
                return None
            return (vp * 8)(*[None if name in null_entry else outs[name].data_ptr()] * 8)

        rc = L.mmt_horizon_joint(
            ML.stream_ptr(dev), count, batch, samples, steps, (i32 * n)(*[V_] * n) if arrays else None,
            (vp * n)(*[tok_.data_ptr() if tok_ is not None else None] * n), (i64 * n)(*[stride] * n),
            (vp * n)(*[val_.data_ptr() if val_ is not None else None] * n), (i32 * n)(*[pct] * n),
            (vp * n)(*[org_.data_ptr()] * n) if org_ is not None else None, (i64 * n)(*[1] * n), None, nq,
            (f64 * 16)(*levels) if levels is not None else None, nbk, (f64 * 128)(*coef) if with_coef else None, nb,
            (f64 * 64)(*bars) if with_bars else None, npair, (i32 * 56)(*pairs) if with_pairs else None, out("bstats"),
            out("bqval"), out("bqrow"), out("btail"), out("bhit"), out("pstats"), ess.data_ptr() if with_ess else None,
            live.data_ptr() if with_ess else None, scratch.data_ptr() + sc if sc is not None else None, nbytes)
        torch.cuda.synchronize()
        clean = all(bool((t == -7).all()) for t in list(outs.values()) + [ess, live])
        return rc, clean

    for kw in (dict(count=-1), dict(batch=-1), dict(steps=-1), dict(samples=0), dict(batch=1 << 20, samples=1 << 11),
               dict(nq=17), dict(nq=-1), dict(nb=9), dict(nb=-1), dict(levels=(0.0, 0.5)), dict(levels=(0.5, 1.0)),
               dict(levels=(nan, 0.5)), dict(levels=None), dict(bars=(0.0, 1.0, 1.0, 1.0)), dict(bars=(1.0, 1.0, nan, 1.0)),
               dict(bars=(1.0, -inf, 1.0, 1.0)), dict(V_=0), dict(stride=N - 1), dict(arrays=False), dict(tok_=None),
               dict(val_=None), dict(org_=None), dict(sc=None), dict(sc=8), dict(nbytes=need - 1),
               dict(nbk=9), dict(nbk=-1), dict(npair=29), dict(npair=-1), dict(coef=(1.0, nan, 0.5, 0.5)),
               dict(coef=(1.0, 0.0, inf, 0.5)), dict(coef=(1.0, 0.0, 0.0, 0.0)), dict(pairs=(0, 0)), dict(pairs=(0, 2)),
               dict(pairs=(-1, 1)), dict(count=0), dict(with_coef=False), dict(with_bars=False), dict(with_pairs=False),
               dict(missing=("bstats",)), dict(missing=("bqval",)), dict(missing=("bqrow",)), dict(missing=("btail",)),
               dict(missing=("bhit",)), dict(missing=("pstats",)), dict(null_entry=("bstats",)),
               dict(null_entry=("btail",)), dict(null_entry=("bhit",)), dict(null_entry=("pstats",))):
        rc, clean = call(**kw)
        assert rc == -1 and clean, kw
    for kw in (dict(V_=(1 << 20) + 1), dict(batch=1, samples=4097, nbytes=1 << 40),
               dict(count=9, coef=tuple([1.0] * 18), nbytes=1 << 40)):
        rc, clean = call(**kw)
        assert rc == -2 and clean, kw
    assert L.mmt_horizon_joint_scratch_bytes(P, 1, 4097, N, 2) == -1 and L.mmt_horizon_joint_scratch_bytes(P, B, S, -1, 2) == -1
    assert L.mmt_horizon_joint_scratch_bytes(9, B, S, N, 2) == -1 and L.mmt_horizon_joint_scratch_bytes(P, B, S, N, 9) == -1
    for kw in (dict(nbk=0, npair=0), dict(batch=0), dict(steps=0)):
        rc, clean = call(**kw)
        assert rc == 0 and clean, kw
    rc, clean = call(pct=1, org_=None)  # percent series need no origin
    assert rc == 0 and not clean
    rc, clean = call(nq=0, nb=0, missing=("bqval", "bqrow", "btail", "bhit"), with_bars=False, with_ess=False)
    assert rc == 0 and not clean
    rc, clean = call(nbk=0, with_coef=False, with_bars=False, missing=("bstats", "bqval", "bqrow", "btail", "bhit"))
    assert rc == 0 and not clean
    rc, clean = call(npair=0, with_pairs=False, missing=("pstats",))
    assert rc == 0 and not clean
