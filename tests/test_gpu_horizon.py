"""mmt_horizon_stats (csrc/mmt_horizon.hip) on host-made tokens, against horizon_ref (fp64 numpy). No model runs here,
so a failure names these kernels.

Inputs (horizon_ref.case): three prompts of S paths, tokens uniform in 0..V-1, a percent problem and a value problem per
launch, sorted values rounded to 2 decimals; no weights, N(0, 0.3^2) and N(0, 8^2) log-weights (prompt 1 shifted by -50,
-inf rows in prompt 2). S around the powers of two the sort pads to, S = 1 and the cap 4096; 1, 2 and 33 steps; V = 1
(every x equal: the order is that of s), 5 (heavy ties) and 900. Token rows are handed in with a stride of steps + 3
whose pad holds out-of-range tokens, origins with stride 2, outputs between guard rows.

Bounds (derived in horizon_ref's docstring): without weights qrow / qval (as int64 bits) and min / max equal the
reference's, stats and hit within a relative 1e-12 (the mean within 1e-12 sum w |x| / W, the variance with the mean's
allowance squared on top). With weights every entry gains 2 EPS times its sum of magnitudes, EPS = 4 * 2^-24 per weight;
a quantile whose level lies within DELTA = 8 * 2^-24 of a prefix boundary may be the row across it, for at most
max(1, 2 %) of a case's (prompt, step, level) triples (test_horizon_ref_cpu.py asserts the cap on these inputs)."""
import ctypes

import numpy as np
import pytest
import torch

import horizon_ref as H
import mmt_lib as ML
import mmt_sample as MS

pytestmark = pytest.mark.gpu

BIG = 10 ** 9


def launch(problems, B, S, N, logw=None, levels=H.LEVELS, barriers=H.BARRIERS, pad=3):
    """problems: dicts with tok int64 [B S, N], values fp64 [V], pct and (value series) origin int64 [B S]; optional
    bars (else `barriers`). Returns per problem a dict of numpy arrays (stats, qval, qrow, hit, ess, live), after
    checking the guard rows around every output."""
    dev = torch.device("cuda")
    R, nq, nb = B * S, len(levels), len(barriers)
    hl = MS.HorizonLaunch([len(q["values"]) for q in problems], [N + pad] * len(problems),
                          [q["pct"] for q in problems], levels, [q.get("bars", barriers) for q in problems])
    keep, outs = [], []
    for p, q in enumerate(problems):
        t = torch.full((R, N + pad), BIG, dtype=torch.int64, device=dev)
        t[:, :N] = torch.from_numpy(np.ascontiguousarray(q["tok"])).to(dev)
        v = torch.from_numpy(np.asarray(q["values"], dtype=np.float64)).to(dev)
        o = torch.full((R, 2), BIG, dtype=torch.int64, device=dev)  # the odd entries would be out of range
        if not q["pct"]:
            o[:, 0] = torch.from_numpy(np.asarray(q["origin"], dtype=np.int64)).to(dev)
            hl.origin[p], hl.origin_stride[p] = o.data_ptr(), 2
        g = {"stats": torch.full((B + 2, N, 12), -7.0, dtype=torch.float64, device=dev),
             "qval": torch.full((B + 2, N, max(nq, 1)), -7.0, dtype=torch.float64, device=dev),
             "qrow": torch.full((B + 2, N, max(nq, 1)), -7, dtype=torch.int32, device=dev),
             "hit": torch.full((B + 2, N, max(nb, 1)), -7.0, dtype=torch.float64, device=dev),
             "ess": torch.full((B + 2,), -7.0, dtype=torch.float64, device=dev),
             "live": torch.full((B + 2,), -7, dtype=torch.int32, device=dev)}
        keep += [t, v, o]
        hl.tok[p], hl.values[p] = t.data_ptr(), v.data_ptr()
        hl.stats[p], hl.ess[p], hl.live[p] = g["stats"][1].data_ptr(), g["ess"][1:].data_ptr(), g["live"][1:].data_ptr()
        if nq:
            hl.qval[p], hl.qrow[p] = g["qval"][1].data_ptr(), g["qrow"][1].data_ptr()
        if nb:
            hl.hit[p] = g["hit"][1].data_ptr()
        outs.append(g)
    lw = None if logw is None else torch.from_numpy(np.asarray(logw, dtype=np.float64)).to(dev)
    L = ML.lib()
    nbytes = hl.scratch_bytes(L, B, S, N)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    hl.run(L, ML.stream_ptr(dev), B, S, N, lw.data_ptr() if lw is not None else 0, scratch.data_ptr(), nbytes)
    torch.cuda.synchronize()
    res = []
    for g in outs:
        for name, t in g.items():
            assert bool((t[0] == -7).all()) and bool((t[-1] == -7).all()), f"wrote outside its {name} rows"
        res.append({"stats": g["stats"][1:-1].cpu().numpy(), "qval": g["qval"][1:-1, :, :nq].cpu().numpy(),
                    "qrow": g["qrow"][1:-1, :, :nq].cpu().numpy(), "hit": g["hit"][1:-1, :, :nb].cpu().numpy(),
                    "ess": g["ess"][1:-1].cpu().numpy(), "live": g["live"][1:-1].cpu().numpy()})
    return res


def problems_of(c):
    return [dict(tok=c["tok"][0], values=c["values"], pct=True),
            dict(tok=c["tok"][1], values=c["values"], pct=False, origin=c["origin"])]


def at(res, b):
    return {k: v[b] for k, v in res.items()}


def compare(res, refs, weighted, what):
    """One problem's three prompts; returns (ambiguous, triples, worst error / bound)."""
    amb, worst = 0, 0.0
    for b, r in enumerate(refs):
        a, w = H.check(at(res, b), r, weighted, f"{what} prompt {b}")
        amb, worst = amb + a, max(worst, w)
    n = sum(r["margin"].size for r in refs)
    assert amb <= H.cap(n), (what, amb, n)
    return amb, n, worst


def bits(res):
    return [{k: v.view(np.int64) if v.dtype == np.float64 else v for k, v in r.items()} for r in res]


def same(a, b):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(bits(a), bits(b)) for k in x)


@pytest.mark.parametrize("S", H.SAMPLES)
def test_matches_numpy(S):
    amb = n = 0
    worst = {}
    for N in H.steps_for(S):
        for V in H.VS:
            for sigma in H.SIGMAS:
                c = H.case(S, N, V, sigma)
                res = launch(problems_of(c), H.PROMPTS, S, N, c["logw"])
                for p in range(2):
                    a, t, w = compare(res[p], c["ref"][p], sigma is not None, f"S={S} N={N} V={V} sigma={sigma} p={p}")
                    amb, n = amb + a, n + t
                    worst[sigma] = max(worst.get(sigma, 0.0), w)
    print(f"horizon S={S}: ambiguous triples {amb} of {n}; largest error / bound " +
          ", ".join(f"sigma {k}: {v:.3f}" for k, v in worst.items()))


def test_many_levels_eight_barriers_problem_chunks_and_the_public_wrapper():
    S, N, V = 64, 5, 900
    c = H.case(S, N, V, 0.3, 1, H.LEVELS16, H.BARRIERS8)
    two = problems_of(c)
    res = launch([two[p % 2] for p in range(9)], H.PROMPTS, S, N, c["logw"], H.LEVELS16, H.BARRIERS8)  # two launches
    for p in range(9):
        compare(res[p], c["ref"][p % 2], True, f"chunk problem {p}")
        assert same([res[p]], [res[p % 2]])  # a problem's bits do not depend on its place or its company
    dev = torch.device("cuda")
    toks = [torch.from_numpy(t).to(dev) for t in c["tok"]]
    hz = MS.horizon_stats(toks, samples=S, values=[c["values"]] * 2, is_percent=[True, False],
                          origin=[None, torch.from_numpy(c["origin"]).to(dev)], logw=torch.from_numpy(c["logw"]).to(dev),
                          quantiles=H.LEVELS16, barriers=[H.BARRIERS8] * 2)
    for p in range(2):
        d = hz[p]
        assert d["quantile_paths"].shape == (3, N, 16) and d["hit"].shape == (3, N, 8) and d["mean"].shape == (3, N)
        stats = torch.stack([d[k] for k in MS.HORIZON_FIELDS], dim=-1).cpu().numpy()
        got = {"stats": stats, "qval": d["quantile_values"].cpu().numpy(), "qrow": d["quantile_paths"].cpu().numpy(),
               "hit": d["hit"].cpu().numpy(), "ess": d["ess"].cpu().numpy(), "live": d["live"].cpu().numpy()}
        assert same([got], [res[p]])
    with pytest.raises(ValueError):
        MS.horizon_stats(toks, samples=S, values=[c["values"][::-1].copy()] * 2, is_percent=True)
    with pytest.raises(ValueError):
        MS.horizon_stats(toks, samples=S, values=[c["values"]] * 2, is_percent=True, barriers=[[0.0], [1.0]])
    with pytest.raises(ValueError):
        MS.horizon_stats(toks, samples=S, values=[c["values"]] * 2, is_percent=False)  # a value series, no origin
    with pytest.raises(ValueError):
        MS.horizon_stats(toks, samples=S, values=None)


def test_dead_rows_and_an_all_dead_prompt():
    S, N, V = 65, 3, 144
    c = H.case(S, N, V, 8.0, 2)
    tok = [t.copy() for t in c["tok"]]
    origin = c["origin"].copy()
    tok[0][5, 1] = V          # prompt 0: a token past the vocabulary, in the percent problem only
    tok[1][7, 2] = -1         # and a negative one in the value problem
    origin[S + 9] = V         # prompt 1: a bad origin (the value problem; the percent problem does not read it)
    tok[0][2 * S:] = BIG      # prompt 2: all dead in the percent problem
    probs = [dict(tok=tok[0], values=c["values"], pct=True), dict(tok=tok[1], values=c["values"], pct=False, origin=origin)]
    res = launch(probs, H.PROMPTS, S, N, c["logw"])
    for p in range(2):
        pq = H.paths(tok[p], c["values"], p == 0, origin)
        for b in range(H.PROMPTS):
            sl = slice(b * S, (b + 1) * S)
            ref = H.prompt(*[t[sl] for t in pq], c["logw"][sl], H.LEVELS, H.BARRIERS)
            H.check(at(res[p], b), ref, True, f"dead p={p} b={b}")
    assert res[0]["live"][2] == 0 and res[0]["ess"][2] == 0 and (res[0]["qrow"][2] == -1).all()
    assert np.isnan(res[0]["stats"][2]).all() and np.isnan(res[0]["hit"][2]).all() and np.isnan(res[0]["qval"][2]).all()
    # a dead row changes nothing else: the same bits as the intact row with weight zero
    for p, rows in ((0, [5]), (1, [7, S + 9])):
        lw = c["logw"].copy()
        lw[rows] = -np.inf
        ref = launch(problems_of(c), H.PROMPTS, S, N, lw)
        for b in range(2):
            assert same([at(res[p], b)], [at(ref[p], b)]), (p, b)


def test_alone_is_in_company_and_runs_repeat():
    S, N, V = 257, 33, 5
    c = H.case(S, N, V, 0.3)
    probs = problems_of(c)
    res = launch(probs, H.PROMPTS, S, N, c["logw"])
    assert same(res, launch(probs, H.PROMPTS, S, N, c["logw"]))  # run to run
    for b in range(H.PROMPTS):
        sl = slice(b * S, (b + 1) * S)
        one = [dict(q, tok=q["tok"][sl], origin=c["origin"][sl]) for q in probs]
        alone = launch(one, 1, S, N, c["logw"][sl])
        for p in range(2):
            assert same([at(alone[p], 0)], [at(res[p], b)]), (b, p)
    for p in range(2):
        assert same(launch([probs[p]], H.PROMPTS, S, N, c["logw"]), [res[p]])
    # no weights, no quantiles, no barriers: the optional outputs may be absent
    res0 = launch(probs, H.PROMPTS, S, N, None, (), ())
    for p in range(2):
        ref = [H.prompt(*[t[b * S:(b + 1) * S] for t in H.paths(c["tok"][p], c["values"], p == 0, c["origin"])], None,
                        (), ()) for b in range(H.PROMPTS)]
        compare(res0[p], ref, False, f"bare p={p}")


def test_refusals_write_nothing():
    B, S, N, V = 2, 4, 3, 13
    dev = torch.device("cuda")
    L = ML.lib()
    i32, i64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    tok = torch.zeros(B * S, N, dtype=torch.int64, device=dev)
    val = torch.linspace(-1, 1, V, dtype=torch.float64, device=dev)
    org = torch.zeros(B * S, dtype=torch.int64, device=dev)
    need = L.mmt_horizon_scratch_bytes(1, B, S, N)
    assert need > 0
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")

    def call(count=1, batch=B, samples=S, steps=N, V_=V, stride=N, pct=0, nq=2, levels=(0.25, 0.75), nb=2,
             bars=(1.0, -1.0), tok_=tok, val_=val, org_=org, with_stats=True, with_q=True, with_hit=True, arrays=True,
             bar_array=True, sc=0, nbytes=need):
        outs = [torch.full((B * N * 16,), -7.0, dtype=torch.float64, device=dev) for _ in range(4)]
        qrow = torch.full((B * N * 16,), -7, dtype=torch.int32, device=dev)
        live = torch.full((B,), -7, dtype=torch.int32, device=dev)
        barr = (f64 * 8)(*bars)
        rc = L.mmt_horizon_stats(
            ML.stream_ptr(dev), count, batch, samples, steps, (i32 * 1)(V_) if arrays else None,
            (vp * 1)(tok_.data_ptr() if tok_ is not None else None), (i64 * 1)(stride),
            (vp * 1)(val_.data_ptr() if val_ is not None else None), (i32 * 1)(pct),
            (vp * 1)(org_.data_ptr()) if org_ is not None else None, (i64 * 1)(1), None, nq,
            (f64 * 16)(*levels) if levels is not None else None, nb,
            (vp * 1)(ctypes.addressof(barr)) if bar_array else None,
            (vp * 1)(outs[0].data_ptr() if with_stats else None), (vp * 1)(outs[1].data_ptr()) if with_q else None,
            (vp * 1)(qrow.data_ptr()) if with_q else None, (vp * 1)(outs[2].data_ptr()) if with_hit else None,
            (vp * 1)(outs[3].data_ptr()), (vp * 1)(live.data_ptr()),
            scratch.data_ptr() + sc if sc is not None else None, nbytes)
        torch.cuda.synchronize()
        clean = all(bool((t == -7).all()) for t in outs + [qrow, live])
        return rc, clean

    for kw in (dict(count=-1), dict(batch=-1), dict(steps=-1), dict(samples=0), dict(batch=1 << 20, samples=1 << 11),
               dict(nq=17), dict(nq=-1), dict(nb=9), dict(nb=-1), dict(levels=(0.0, 0.5)), dict(levels=(0.5, 1.0)),
               dict(levels=(nan, 0.5)), dict(levels=None), dict(bars=(0.0, 1.0)), dict(bars=(nan, 1.0)),
               dict(bars=(1.0, -inf)), dict(V_=0), dict(stride=N - 1), dict(arrays=False), dict(tok_=None),
               dict(val_=None), dict(org_=None), dict(with_stats=False), dict(with_q=False), dict(with_hit=False),
               dict(bar_array=False), dict(sc=None), dict(sc=8), dict(nbytes=need - 1)):
        rc, clean = call(**kw)
        assert rc == -1 and clean, kw
    for kw in (dict(V_=(1 << 20) + 1), dict(batch=1, samples=4097, nbytes=1 << 40)):
        rc, clean = call(**kw)
        assert rc == -2 and clean, kw
    assert L.mmt_horizon_scratch_bytes(1, 1, 4097, N) == -1 and L.mmt_horizon_scratch_bytes(1, B, S, -1) == -1
    for kw in (dict(count=0), dict(batch=0), dict(steps=0)):
        rc, clean = call(**kw)
        assert rc == 0 and clean, kw
    rc, clean = call(pct=1, org_=None)  # a percent series needs no origin
    assert rc == 0 and not clean
    rc, clean = call(nq=0, nb=0, with_q=False, with_hit=False, bar_array=False)
    assert rc == 0 and not clean
