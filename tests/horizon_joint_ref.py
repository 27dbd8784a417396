"""CPU restatement of the joint horizon rules (include/mmt.h: mmt_horizon_joint), in fp64 numpy, on top of
horizon_ref.paths / horizon_ref.prompt and evidence_ref.weights. Test infrastructure only.

paths(problems, coefs)      rule 1: every problem by horizon_ref.paths, then per basket y = 0.0; t = coef[p] * x^(p); y = y
                            + t for p ascending (one IEEE operation per line), hi^y, lo^y; dead [R]: dead in any problem,
                            or a y that is not finite. Returns xs, ds [P][R, N], ys, his, los [K][R, N], dead.
prompt(xs, ds, ys, his, los, dead, a, levels, barriers, pairs)
                            rules 2 - 8 for one prompt (the arrays sliced to its S rows; a: fp64 [S] log-weights or None;
                            barriers [K][nb]). Returns {"ess", "live", "w", "baskets": [dict], "pairs": [dict]}.
  a basket dict: horizon_ref.prompt's of (y, hi^y, lo^y) with "stats" / "bound" cut to the 9 entries of bstats, plus
    tail, tail_alt [N, nq]     rule 5 at the quantile row and at the row across the nearer boundary
    tail_bound, tail_alt_bound their allowances
  a pair dict: stats, bound [N, 22]; corr_cmp [N] (corr is compared), corr_nan [N] (corr must be NaN); const [N] (a
    series is constant over the rows with weight).

The bounds, derived as horizon_ref derives its own (RTOL = 1e-12 for fp64 sums in another order, EPS = 4 * 2^-24 per
fp32 weight, a ratio of weighted sums moving by 2 EPS times its sum of magnitudes):
  basket stats, quantiles, hits: horizon_ref's, on y. min / max and, without weights, bqrow / bqval are exact.
  tail = (A + rem y_m) / target with A = sum_{i<m} w_i y_i, P = sum_{i<m} w_i, rem = target - P. Without weights P and
    target are exact, so rem is: the error is that of the sum A and of the one addition, RTOL (sum_{i<m} w |y_i| +
    |rem y_m|) / target. With weights tail = y_m + sum_{i<m} w_i (y_i - y_m) / target is a ratio of weighted sums: it
    moves by 2 EPS sum_{i<m} w_i |y_i - y_m| / target <= 2 EPS (sum_{i<m} w |y_i| + P |y_m|) / target, and the fp64
    prefix P in another order adds RTOL P |y_m| / target: (2 EPS + RTOL) (sum_{i<m} w |y_i| + P |y_m|) / target on top.
  pair means as horizon_ref's mean: b_p = (RTOL + 2 EPS) sum w |x_p| / W. var_p as there: (RTOL + 2 EPS) var_p + 2
    b_p^2. cov: about other means m' the sum is cov + (m'_p - m_p) (m'_q - m_q), so (RTOL + 2 EPS) sum w |a c| / W + 2
    b_p b_q. Table cells: (RTOL + 2 EPS) times the cell.
  corr = cov / (sqrt(var_p) sqrt(var_q)) =: cov / den. To first order it moves by b_cov / den + |corr| (b_vp / (2 var_p) +
    b_vq / (2 var_q)); where corr is compared (below) the relative terms stay under 1e-3, so a factor 1.001 covers the
    second order, and RTOL |corr| the two square roots, the product and the division.
  corr is compared only where both reference variances exceed 1e-9 (max |x|)^2, the maximum over both series' rows
    with weight at that step: below that the variance is the rounding of the mean, not a property of the data.
    Elsewhere a series is constant over the rows with weight (the CPU tests assert that on every input), and corr
    must be NaN where the constant's mean is exact in any order of summation, so that every deviation is exactly 0:
    one row with weight (w = 1), or the constant 0. Other constant cells assert nothing on corr (var still has its
    bound).
  Ambiguous quantiles (level within DELTA = 8 * 2^-24 of a prefix boundary, weights only): bqrow / bqval / btail may be
    those of the row across the boundary, for at most max(1, 2 %) of a case's (prompt, step, level) triples per
    basket.

The input family of the GPU tests (case): `count` problems, even ones percent series, odd ones value series, tokens
uniform in 0..V-1, horizon_ref's values and log-weights. GRID[S] lists the cases of one size: an orthogonal array over
steps {1, 2, 33} x count {2, 3, 8} x V {1, 5, 900} x {no weights, sigma 0.3, sigma 8}, the basket / pair configuration
cycling over its rows and shifted with the size."""
import functools
import math

import numpy as np

import forecast_ref as F
import horizon_ref as H

RTOL, EPS, DELTA, PROMPTS = H.RTOL, H.EPS, H.DELTA, H.PROMPTS
LEVELS = H.LEVELS
SAMPLES = [1, 2, 15, 17, 64, 255, 256, 257, 1000, 4096]
STEPS = [1, 2, 33]
COUNTS = [2, 3, 8]
BSTATS = [0, 1, 2, 3, 4, 8, 9, 10, 11]  # horizon_ref.prompt's stats entries that bstats keeps
CONFIGS = ("full", "one_basket", "pairs_only")
# L9(3^4): rows of (steps, count, V, sigma) indices, every pair of columns holding every pair of levels once
L9 = [(0, 0, 0, 0), (0, 1, 1, 1), (0, 2, 2, 2), (1, 0, 1, 2), (1, 1, 2, 0), (1, 2, 0, 1), (2, 0, 2, 1), (2, 1, 0, 2),
      (2, 2, 1, 0)]
GRID = {S: [(STEPS[a], COUNTS[b], H.VS[c], H.SIGMAS[d], CONFIGS[(r + i) % 3]) for r, (a, b, c, d) in enumerate(L9)]
        for i, S in enumerate(SAMPLES)}


def coefs_for(count, nbk, seed=0):
    """nbk baskets over `count` series: the first a unit basket on series 0, the second a long-short pair, the rest
    drawn in {-2, -1.5, .., 2} with zeros (at least one entry non-zero)."""
    rng = np.random.default_rng(4242 + 31 * count + seed)
    out = []
    for k in range(nbk):
        a = np.round(rng.integers(-4, 5, size=count) * 0.5, 1)
        if k == 0:
            a = np.zeros(count)
            a[0] = 1.0
        elif k == 1:
            a = np.zeros(count)
            a[0], a[1] = 1.0, -0.75
        elif not a.any():
            a[k % count] = 0.5
        out.append([float(t) for t in a])
    return out


def config(name, count):
    """(coefs [nbk][count], barriers [nbk][nb], pairs) of a configuration."""
    if name == "full":
        pairs = [(p, q) for p in range(count) for q in range(p + 1, count)]
        pairs = pairs[:-1] + [(pairs[-1][1], pairs[-1][0])]  # one pair the other way round
        return coefs_for(count, 8), [list(H.BARRIERS8)] * 8, pairs
    if name == "one_basket":
        return coefs_for(count, 2)[1:], [list(H.BARRIERS)], []
    return [], [], [(0, 1), (1, 0)] + ([(2, 0)] if count > 2 else [])


def paths(problems, coefs):
    xs, ds, dead = [], [], None
    for q in problems:
        x, _, _, d, dd = H.paths(q["tok"], q["values"], q["pct"], q.get("origin"))
        xs.append(x)
        ds.append(d)
        dead = dd.copy() if dead is None else dead | dd
    ys, his, los = [], [], []
    with np.errstate(all="ignore"):
        for a in coefs:
            y = np.zeros_like(xs[0])
            for p, x in enumerate(xs):
                t = a[p] * x
                y = y + t
            ys.append(y)
            dead = dead | ~np.isfinite(y).all(axis=1)
    for y in ys:
        y[dead] = 0.0
        his.append(np.maximum.accumulate(np.maximum(y, 0.0), axis=1))
        los.append(np.minimum.accumulate(np.minimum(y, 0.0), axis=1))
    return xs, ds, ys, his, los, dead


def tail_at(rows_w, ys, m, target):
    """Rule 5 at place m of the sorted order: (tail, sum_{i<m} w |y_i|, P, rem)."""
    P = rows_w[:m].sum()
    A = (rows_w[:m] * ys[:m]).sum()
    rem = target - P
    t = rem * ys[m]
    return (A + t) / target, (rows_w[:m] * np.abs(ys[:m])).sum(), P, rem


def prompt(xs, ds, ys, his, los, dead, a=None, levels=LEVELS, barriers=(), pairs=()):
    S, N = xs[0].shape
    nq = len(levels)
    weighted = a is not None
    extra = 2 * EPS if weighted else 0.0
    w, ess, live = F.path_weights(np.zeros(S) if a is None else a, dead)
    out = {"ess": ess, "live": live, "w": w, "baskets": [], "pairs": []}
    keep = np.nonzero(w > 0)[0]
    wk = w[keep]
    W = wk.sum()
    zero = np.zeros((S, N), dtype=np.int64)
    for k, y in enumerate(ys):
        r = H.prompt(y, his[k], los[k], zero, dead, a, levels, barriers[k])
        r["stats"], r["bound"] = r["stats"][:, BSTATS], r["bound"][:, BSTATS]
        for name in ("tail", "tail_alt", "tail_bound", "tail_alt_bound"):
            r[name] = np.full((N, nq), np.nan)
        for j in range(N if live else 0):
            yj = y[keep, j]
            order = np.lexsort((keep, yj))
            rows, ysort, wsort = keep[order], yj[order], wk[order]
            place = {int(s): i for i, s in enumerate(rows)}
            for q, lv in enumerate(levels):
                target = lv * W
                for name, row in (("tail", r["qrow"][j, q]), ("tail_alt", r["qalt"][j, q])):
                    m = place[int(row)]
                    t, sabs, P, rem = tail_at(wsort, ysort, m, target)
                    r[name][j, q] = t
                    r[name + "_bound"][j, q] = (RTOL * (sabs + abs(rem * ysort[m])) + (
                        (extra + RTOL) * (sabs + P * abs(ysort[m])) if weighted else 0.0)) / target
        out["baskets"].append(r)
    for p, q in pairs:
        st, bd = np.full((N, 22), np.nan), np.zeros((N, 22))
        cmp_, nan_, const = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
        for j in range(N if live else 0):
            x, z, dx, dz = xs[p][keep, j], xs[q][keep, j], ds[p][keep, j], ds[q][keep, j]
            mp, mq = (wk * x).sum() / W, (wk * z).sum() / W
            bp, bq = (RTOL + extra) * (wk * np.abs(x)).sum() / W, (RTOL + extra) * (wk * np.abs(z)).sum() / W
            da, dc = x - mp, z - mq
            vp, vq, cov = (wk * (da * da)).sum() / W, (wk * (dc * dc)).sum() / W, (wk * (da * dc)).sum() / W
            den = math.sqrt(vp) * math.sqrt(vq)
            st[j, 0], bd[j, 0] = cov, (RTOL + extra) * (wk * np.abs(da * dc)).sum() / W + 2 * bp * bq
            st[j, 2], bd[j, 2] = vp, (RTOL + extra) * vp + 2 * bp * bp
            st[j, 3], bd[j, 3] = vq, (RTOL + extra) * vq + 2 * bq * bq
            st[j, 1] = cov / den if den != 0 else np.nan
            big = max(np.abs(x).max(), np.abs(z).max())
            cmp_[j] = vp > 1e-9 * big * big and vq > 1e-9 * big * big
            if cmp_[j]:
                c = st[j, 1]
                bd[j, 1] = 1.001 * (bd[j, 0] / den + abs(c) * (bd[j, 2] / (2 * vp) + bd[j, 3] / (2 * vq))) + RTOL * abs(c)
            for s, arr in ((x, "x"), (z, "z")):
                if s.max() == s.min():
                    const[j] = True
                    nan_[j] |= len(keep) == 1 or s[0] == 0.0
            sx, sz = H.sign(x), H.sign(z)
            for u in range(3):
                for v in range(3):
                    st[j, 4 + 3 * u + v] = wk[(sx == u - 1) & (sz == v - 1)].sum() / W
                    st[j, 13 + 3 * u + v] = wk[(dx == u - 1) & (dz == v - 1)].sum() / W
            bd[j, 4:] = (RTOL + extra) * st[j, 4:]
        out["pairs"].append({"stats": st, "bound": bd, "corr_cmp": cmp_, "corr_nan": nan_, "const": const})
    return out


def problems_for(S, N, count, V, seed=0):
    rng = np.random.default_rng(700001 * seed + 7919 * S + 131 * N + 17 * V + count)
    R = PROMPTS * S
    return [dict(tok=rng.integers(0, V, size=(R, N)), values=H.values_for(V, seed + p), pct=p % 2 == 0,
                 origin=rng.integers(0, V, size=R)) for p in range(count)]


def reference(problems, S, coefs, barriers, pairs, a, levels=LEVELS):
    """The reference of every prompt of a launch: a list of `prompt` results."""
    pq = paths(problems, coefs)
    B = len(pq[5]) // S
    out = []
    for b in range(B):
        sl = slice(b * S, (b + 1) * S)
        out.append(prompt([x[sl] for x in pq[0]], [d[sl] for d in pq[1]], [y[sl] for y in pq[2]],
                          [h[sl] for h in pq[3]], [lo[sl] for lo in pq[4]], pq[5][sl], None if a is None else a[sl],
                          levels, barriers, pairs))
    return out


@functools.lru_cache(maxsize=None)
def case(S, N, count, V, sigma, cfg, seed=0):
    """One GPU test case, computed once and shared."""
    problems = problems_for(S, N, count, V, seed)
    coefs, barriers, pairs = config(cfg, count)
    a = None if sigma is None else F.log_weights(S, sigma, seed).reshape(-1)
    return {"problems": problems, "coefs": coefs, "barriers": barriers, "pairs": pairs, "logw": a, "S": S, "N": N,
            "ref": reference(problems, S, coefs, barriers, pairs, a)}


def ambiguous(refs, k):
    """(ambiguous, all) (prompt, step, level) triples of basket k over a case's prompts."""
    return (sum(int((r["baskets"][k]["margin"] < DELTA).sum()) for r in refs),
            sum(r["baskets"][k]["margin"].size for r in refs))


def corr_skipped(refs):
    """(cells where corr is not compared, those of them where no series is constant) over a case's prompts."""
    skip = bad = 0
    for r in refs:
        if r["live"] == 0:
            continue
        for pr in r["pairs"]:
            skip += int((~pr["corr_cmp"]).sum())
            bad += int((~pr["corr_cmp"] & ~pr["const"]).sum())
    return skip, bad


def check(got, ref, weighted, what=""):
    """One prompt against `prompt`: got = dict(ess, live, bstats [K][N, 9], bqval, bqrow, btail [K][N, nq], bhit [K][N,
    nb], pstats [NP][N, 22]). Asserts the bounds; returns (ambiguous triples per basket, largest error / bound)."""
    assert int(got["live"]) == ref["live"], (what, got["live"], ref["live"])
    K, NP = len(ref["baskets"]), len(ref["pairs"])
    if ref["live"] == 0:
        assert got["ess"] == 0.0, what
        for k in range(K):
            assert np.isnan(got["bstats"][k]).all() and np.isnan(got["bqval"][k]).all(), what
            assert np.isnan(got["btail"][k]).all() and np.isnan(got["bhit"][k]).all(), what
            assert (got["bqrow"][k] == -1).all(), what
        for k in range(NP):
            assert np.isnan(got["pstats"][k]).all(), what
        return [0] * K, 0.0
    etol = (RTOL + (4 * EPS if weighted else 0.0)) * ref["ess"]
    assert abs(got["ess"] - ref["ess"]) <= etol, (what, got["ess"], ref["ess"])
    worst = 0.0

    def within(g, r, b, name):
        nonlocal worst
        with np.errstate(all="ignore"):
            err = np.where(g == r, 0.0, np.abs(g - r))  # a sum that overflows does so in both: inf equals inf
        bad = ~(err <= b)
        assert not bad.any(), (what, name, np.argwhere(bad)[:4], g[bad][:4], r[bad][:4], b[bad][:4])
        with np.errstate(all="ignore"):
            ratio = np.where(err > 0, err / np.where(b > 0, b, 1.0), 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)

    amb = []
    for k, r in enumerate(ref["baskets"]):
        g = got["bstats"][k]
        assert np.array_equal(g[:, 7:].view(np.int64), r["stats"][:, 7:].view(np.int64)), (what, k, "min/max")
        within(g[:, :7], r["stats"][:, :7], r["bound"][:, :7], f"bstats {k}")
        within(got["bhit"][k], r["hit"], r["hit_bound"], f"bhit {k}")
        clear = r["margin"] >= DELTA if weighted else np.ones_like(r["margin"], dtype=bool)
        qr, qv, tl = got["bqrow"][k], got["bqval"][k], got["btail"][k]
        exact = (qr == r["qrow"]) & (qv.view(np.int64) == r["qval"].view(np.int64))
        other = (qr == r["qalt"]) & (qv.view(np.int64) == r["qalt_val"].view(np.int64)) & ~clear & ~exact
        assert (exact | other).all(), (what, k, "quantiles", np.argwhere(~(exact | other))[:4])
        within(np.where(other, 0.0, tl), np.where(other, 0.0, r["tail"]), r["tail_bound"], f"btail {k}")
        within(np.where(other, tl, 0.0), np.where(other, r["tail_alt"], 0.0), r["tail_alt_bound"], f"btail alt {k}")
        amb.append(int((~clear).sum()))
    for k, r in enumerate(ref["pairs"]):
        g = got["pstats"][k]
        cols = [0] + list(range(2, 22))
        within(g[:, cols], r["stats"][:, cols], r["bound"][:, cols], f"pstats {k}")
        c = r["corr_cmp"]
        within(g[c, 1], r["stats"][c, 1], r["bound"][c, 1], f"corr {k}")
        assert np.isnan(g[r["corr_nan"], 1]).all(), (what, k, "corr is not NaN where a series is exactly constant")
    return amb, worst


def cap(triples):
    return H.cap(triples)


def brute(problems, coefs, barriers, pairs, a, levels):
    """One prompt by brute force in Python floats (problems hold the prompt's rows only): horizon_ref.brute per basket
    cannot be used (it walks tokens), so the walk, the baskets, serial sums and a tuple sort are restated here. Returns
    None without a live row, else (live, baskets [K] of (stats [N][9], qrow, qval, tail [N][nq], hit [N][nb]), pairs
    [NP] of stats [N][22])."""
    S, N = problems[0]["tok"].shape
    P = len(problems)
    rows = []
    for s in range(S):
        ok, xs, ds = True, [], []
        for q in problems:
            v, V = [float(t) for t in q["values"]], len(q["values"])
            good = all(0 <= int(t) < V for t in q["tok"][s]) and (q["pct"] or 0 <= int(q["origin"][s]) < V)
            x, d = [], []
            if good:
                g = 1.0
                prev = None if q["pct"] else v[int(q["origin"][s])]
                for j in range(N):
                    t = v[int(q["tok"][s][j])]
                    if q["pct"]:
                        g = g * (1.0 + t / 100.0)
                        x.append((g - 1.0) * 100.0)
                        d.append((t > 0) - (t < 0))
                    else:
                        x.append(t - v[int(q["origin"][s])])
                        d.append((t - prev > 0) - (t - prev < 0))
                        prev = t
                good = all(math.isfinite(t) for t in x)
            ok = ok and good
            xs.append(x)
            ds.append(d)
        ys, his, los = [], [], []
        if ok:
            for c in coefs:
                y, hi, lo, h, l = [], [], [], 0.0, 0.0
                for j in range(N):
                    t = 0.0
                    for p in range(P):
                        t = t + c[p] * xs[p][j]
                    h, l = max(h, t), min(l, t)
                    y.append(t), hi.append(h), lo.append(l)
                ok = ok and all(math.isfinite(t) for t in y)
                ys.append(y), his.append(hi), los.append(lo)
        rows.append((ok, xs, ds, ys, his, los))
    aa = [0.0 if a is None else (-math.inf if a[s] != a[s] else float(a[s])) for s in range(S)]
    aa = [aa[s] if rows[s][0] else -math.inf for s in range(S)]
    mx = max(aa)
    if mx == -math.inf:
        return None
    w = [math.exp(float(np.float32(t - mx))) if t > -math.inf else 0.0 for t in aa]
    W = math.fsum(w)
    liv = [s for s in range(S) if w[s] > 0]
    sg = lambda t: (t > 0) - (t < 0)  # noqa: E731
    bks = []
    for k in range(len(coefs)):
        stats, qrow, qval, tail, hit = [], [], [], [], []
        for j in range(N):
            y = {s: rows[s][3][k][j] for s in liv}
            mean = math.fsum(w[s] * y[s] for s in liv) / W
            st = [mean, math.fsum(w[s] * (y[s] - mean) ** 2 for s in liv) / W]
            st += [math.fsum(w[s] for s in liv if sg(y[s]) == u) / W for u in (-1, 0, 1)]
            st += [math.fsum(w[s] * rows[s][4][k][j] for s in liv) / W, math.fsum(w[s] * rows[s][5][k][j] for s in liv) / W]
            st += [min(y.values()), max(y.values())]
            stats.append(st)
            hit.append([math.fsum(w[s] for s in liv if (rows[s][4][k][j] >= u if u > 0 else rows[s][5][k][j] <= u)) / W
                        for u in barriers[k]])
            order = sorted((y[s], s) for s in liv)
            qr, qv, tl = [], [], []
            for lv in levels:
                target, acc, m = lv * W, 0.0, len(order) - 1
                for i, (yv, s) in enumerate(order):
                    acc += w[s]
                    if acc >= target:
                        m = i
                        break
                P_ = math.fsum(w[s] for _, s in order[:m])
                A_ = math.fsum(w[s] * yv for yv, s in order[:m])
                qr.append(order[m][1]), qv.append(order[m][0]), tl.append((A_ + (target - P_) * order[m][0]) / target)
            qrow.append(qr), qval.append(qv), tail.append(tl)
        bks.append((stats, qrow, qval, tail, hit))
    prs = []
    for p, q in pairs:
        stats = []
        for j in range(N):
            x, z = {s: rows[s][1][p][j] for s in liv}, {s: rows[s][1][q][j] for s in liv}
            mp, mq = math.fsum(w[s] * x[s] for s in liv) / W, math.fsum(w[s] * z[s] for s in liv) / W
            vp = math.fsum(w[s] * (x[s] - mp) ** 2 for s in liv) / W
            vq = math.fsum(w[s] * (z[s] - mq) ** 2 for s in liv) / W
            cov = math.fsum(w[s] * (x[s] - mp) * (z[s] - mq) for s in liv) / W
            den = math.sqrt(vp) * math.sqrt(vq)
            st = [cov, cov / den if den != 0 else math.nan, vp, vq]
            st += [math.fsum(w[s] for s in liv if sg(x[s]) == u and sg(z[s]) == v) / W for u in (-1, 0, 1)
                   for v in (-1, 0, 1)]
            st += [math.fsum(w[s] for s in liv if rows[s][2][p][j] == u and rows[s][2][q][j] == v) / W
                   for u in (-1, 0, 1) for v in (-1, 0, 1)]
            stats.append(st)
        prs.append(stats)
    return len(liv), bks, prs
