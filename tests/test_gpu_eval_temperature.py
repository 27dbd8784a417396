"""mmt_eval_temperatures (csrc/mmt_evaltemp.hip) against the sampler's and mmt_score_multi's bits, mmt_eval_positions'
bits at temperature 1, the fp64 restatement of both stages (tests/calib_ref.py) and its own contract.

A problem is [3, 5, V] (or [3, 2, V] for the two largest V): N(0, 3^2) rows and the edge rows of `problem`. Every
output buffer lies between guard bands and starts poisoned with one NaN pattern, compared by its bits."""
import ctypes

import numpy as np
import pytest
import torch

import calib_ref as C
import eval_ref as E
import mmt_lib as ML
from test_gpu_eval_positions import launch as positions_launch
from test_gpu_sample import lp_tol
from test_gpu_score import score

pytestmark = pytest.mark.gpu

B0, T0 = 3, 5
VS = [1, 2, 3, 255, 257, 1000, 8192, 8193]
POISON = np.int64(0x7FF8DEAD0000BEEF)  # a NaN
G = 16  # guard doubles on either side of an output
KINDS = ("value", "percent", None)
GRIDS = {1: np.array([1.0], dtype=np.float32), 3: np.array([0.25, 1.0, 1.7], dtype=np.float32),
         32: np.array([2.0 ** ((k - 16) / 8.0) for k in range(32)], dtype=np.float32)}
i32, i64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

_cases = {}


def shape_of(V):
    return (B0, 2) if V >= 8192 else (B0, T0)


def problem(V, kind, seed=0, bad_tokens=True):
    """logits fp32 [B, T, V], xb, yb int64 [B, T], values, is_percent. Edge rows, by flat row index (15 rows; the
    6-row problems of the two largest V hold those marked *): 1* a NaN logit and a target whose logit is -inf, 2* no
    finite logit, 3* a +inf logit, 4* logits of magnitude 80 (at tau 0.25 every weight below the maximum underflows;
    many ties at the maximum), 5* yb = V, 6 xb = -1, 7 xb = V, 8 yb = -1, 9 ties at the maximum among few distinct
    values, 10 a target whose logit is NaN. Cached, read only."""
    key = (V, kind, seed, bad_tokens)
    if key in _cases:
        return _cases[key]
    B, T = shape_of(V)
    rng = np.random.default_rng(4100 + 17 * V + seed)
    x = rng.normal(0.0, 3.0, size=(B * T, V)).astype(np.float32)
    xb, yb = rng.integers(0, V, size=B * T), rng.integers(0, V, size=B * T)
    if V >= 2:
        x[1, (yb[1] + 1) % V] = np.nan
        x[1, yb[1]] = -np.inf
        if V >= 3:
            x[1, (yb[1] + 2) % V] = 0.5  # a finite logit stays
    x[2] = -np.inf
    x[3, int(rng.integers(0, V))] = np.inf
    x[4] = np.where(rng.random(V) < 0.5, np.float32(80.0), np.float32(-80.0))
    if bad_tokens:
        yb[5] = V
    if B * T > 6:
        if bad_tokens:
            xb[6], xb[7], yb[8] = -1, V, -1
        x[9] = rng.integers(-4, 3, size=V).astype(np.float32) * np.float32(0.5)
        x[9, rng.integers(0, V, size=min(V, 3))] = 1.5
        if V >= 2:
            x[10, yb[10]] = np.nan
    values = None if kind is None else E.series(V, "value")
    q = dict(logits=x.reshape(B, T, V), xb=xb.reshape(B, T), yb=yb.reshape(B, T), values=values,
             is_percent=kind == "percent", V=V)
    for a in (q["logits"], q["xb"], q["yb"]):
        a.setflags(write=False)
    _cases[key] = q
    return q


_refs = {}


def ref_records(q, key, temps):
    key = key + (temps.tobytes(),)
    if key not in _refs:
        _refs[key] = C.records(q["logits"], q["xb"], q["yb"], q["values"], q["is_percent"], temps)
        _refs[key].setflags(write=False)
    return _refs[key]


class Guarded:
    """An fp64 device buffer of n doubles between two guard bands, all poisoned (or holding `init`)."""

    def __init__(self, n, dev, init=None):
        self.n = n
        self.t = torch.full((n + 2 * G,), int(POISON), dtype=torch.int64, device=dev).view(torch.float64)
        if init is not None:
            self.t[G:G + n] = torch.from_numpy(np.asarray(init, dtype=np.float64).reshape(-1)).to(dev)

    def ptr(self):
        return self.t.data_ptr() + 8 * G

    def get(self, shape):
        host = self.t.cpu().numpy()
        assert (E.bits(host[:G]) == POISON).all() and (E.bits(host[G + self.n:]) == POISON).all(), "wrote outside"
        return host[G:G + self.n].reshape(shape).copy()


def poisoned(a):
    return (E.bits(a) == POISON).all()


def launch(problems, temps, t_begin=0, bins=10, accumulate=0, with_rec=True, init=None, **over):
    """One mmt_eval_temperatures over `problems`. init: per problem (sum, rel) to start from. `over` replaces raw
    arguments (count, batch, T_, V, K, grid (the temperatures as a list, or None for NULL), scratch, nbytes,
    null=<an array or "entry:<array>" to pass as NULL>). Returns (status, [dict(rec, sum, rel)]); every buffer is
    checked for writes outside it."""
    dev = torch.device("cuda")
    P = len(problems)
    B, T = problems[0]["logits"].shape[:2]
    K = len(temps)
    L = ML.lib()
    bb = min(max(bins, 1), 64)  # the buffers' bins: a refused `bins` still gets buffers to leave untouched
    keep, bufs = [], []
    arr = {k: (vp * max(P, 1))() for k in ("logits", "xb", "yb", "values", "rec", "sum", "rel")}
    for p, q in enumerate(problems):
        d = {k: torch.from_numpy(np.array(q[k])).to(dev) for k in ("logits", "xb", "yb")}
        d["values"] = None if q["values"] is None else torch.from_numpy(q["values"]).to(dev)
        keep.append(d)
        g = dict(rec=Guarded(B * T * K * 4, dev), sum=Guarded(K * 2, dev, init and init[p][0]),
                 rel=Guarded(K * 9 * bb, dev, init and init[p][1]))
        bufs.append(g)
        for k in ("logits", "xb", "yb"):
            arr[k][p] = d[k].data_ptr()
        arr["values"][p] = None if d["values"] is None else d["values"].data_ptr()
        arr["rec"][p] = g["rec"].ptr() if with_rec else None
        arr["sum"][p], arr["rel"][p] = g["sum"].ptr(), g["rel"].ptr()
    null = over.get("null")
    if null in arr:
        arr[null] = None
    elif null is not None and null.startswith("entry:"):
        arr[null.split(":")[1]][0] = None
    V = (i32 * max(P, 1))(*[over.get("V", q["V"]) for q in problems]) if null != "V" else None
    pct = (i32 * max(P, 1))(*[1 if q["is_percent"] else 0 for q in problems])
    tl = over.get("grid", [float(t) for t in temps])
    tarr = None if tl is None else (f32 * max(len(tl), 1))(*tl)
    need = L.mmt_eval_temperatures_scratch_bytes(P, B, T, bb, K)
    assert need >= 0
    scratch = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=dev)
    sp = over.get("scratch", scratch.data_ptr())
    rc = L.mmt_eval_temperatures(ML.stream_ptr(dev), over.get("count", P), over.get("batch", B), over.get("T_", T),
                                 t_begin, bins, accumulate, over.get("K", K), tarr, V, arr["logits"], arr["xb"],
                                 arr["yb"], arr["values"], pct, arr["rec"], arr["sum"], arr["rel"], sp,
                                 over.get("nbytes", need))
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0xAB).all()), "wrote past the scratch"
    out = [dict(rec=g["rec"].get((B, T, K, 4)), sum=g["sum"].get((K, 2)), rel=g["rel"].get((K, 3, bb, 3)))
           for g in bufs]
    return rc, out


def same(a, b):
    return np.array_equal(E.bits(a), E.bits(b))


def check_tables(out, q, t_begin, bins, what):
    """The device's tables are calib_ref.tables of the device's own records, bit for bit."""
    tot, rel = C.tables(out["rec"], t_begin, bins, C.realised(q["xb"], q["yb"], q["values"], q["is_percent"]))
    assert same(out["sum"], tot), (what, "sum", out["sum"], tot)
    assert same(out["rel"], rel), (what, "rel")


def check_records(out, ref, V, t_begin, what):
    rec = out["rec"]
    assert poisoned(rec[:, :t_begin]), (what, "records before t_begin were written")
    got, want = rec[:, t_begin:], ref[:, t_begin:]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want)))
    lp, wlp = got[..., 0], want[..., 0]
    assert np.array_equal(np.isneginf(lp), np.isneginf(wlp)), what
    fin = np.isfinite(wlp)
    err = np.abs(lp[fin] - wlp[fin])
    assert np.all(err <= lp_tol(V, wlp[fin])), (what, float(err.max()))
    worst = 0.0
    for f in (1, 2, 3):
        ok = ~np.isnan(want[..., f])
        err, bound = np.abs(got[..., f][ok] - want[..., f][ok]), E.mass_bound(want[..., f][ok], V)
        if err.size:
            worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (what, f, float(err.max()), np.argwhere(~(err <= bound)))
    return worst


def scores_at(q, temps):
    """mmt_score_multi on logits * inv_t (the fp32 inv_t), one problem per temperature: fp64 [B, T, K]."""
    dev = torch.device("cuda")
    B, T, V = q["logits"].shape
    lg = torch.from_numpy(q["logits"].reshape(B * T, V).copy()).to(dev)
    tok = torch.from_numpy(q["yb"].reshape(B * T).copy()).to(dev)
    probs = [dict(logits=lg * float(C.inv_t(t)), V=V, tok=tok) for t in temps]
    got, rc = score(probs, B * T)
    assert rc == 0
    return np.stack([g.numpy().astype(np.float64).reshape(B, T) for g in got], axis=-1)


def dead_rows(q):
    B, T, V = q["logits"].shape
    x = q["logits"].reshape(B * T, V)
    finite = np.isfinite(np.where(np.isnan(x), -np.inf, x)).any(axis=1) | np.isposinf(x).any(axis=1)
    ok = lambda a: (a.reshape(-1) >= 0) & (a.reshape(-1) < V)
    return ~(finite & ok(q["xb"]) & ok(q["yb"])).reshape(B, T)


@pytest.mark.parametrize("V", VS)
def test_records_and_tables(V):
    """Three problems of one V in one launch (a value series, a percent series, no values), K = 3."""
    temps = GRIDS[3]
    problems = [problem(V, kind) for kind in KINDS]
    rc, outs = launch(problems, temps)
    assert rc == 0
    B, T = shape_of(V)
    dead = dead_rows(problems[0])
    assert dead.reshape(-1)[[2, 5]].all() and not dead.reshape(-1)[[0, 3, 4]].any()
    # 1. rec[..., k, 0]: mmt_score_multi's bits on logits * inv_t
    sc = scores_at(problems[0], temps)
    for p, out in enumerate(outs):
        assert np.isnan(out["rec"][dead]).all(), (V, p)
        assert not np.isnan(out["rec"][~dead][..., 0]).any(), (V, p)
        assert same(out["rec"][~dead][..., 0], sc[~dead]), (V, p)
    if V >= 3:  # a target whose logit is -inf scores -inf at every temperature
        assert np.isneginf(outs[0]["rec"].reshape(B * T, 3, 4)[1, :, 0]).all() and np.isinf(outs[0]["sum"][:, 1]).all()
    # 2. at tau = 1.0 the four fields are mmt_eval_positions' rec[0..3]
    rc, pos = positions_launch(problems)
    assert rc == 0
    for p, out in enumerate(outs):
        assert same(out["rec"][:, :, 1, :], pos[p]["rec"][..., 0:4]), (V, p)
    # 3. the restatement, 4. the tables
    worst = 0.0
    for p, (q, out) in enumerate(zip(problems, outs)):
        worst = max(worst, check_records(out, ref_records(q, (V, KINDS[p]), temps), V, 0, (V, KINDS[p])))
        check_tables(out, q, 0, 10, (V, KINDS[p]))
        assert (out["sum"][:, 0] == (~dead).sum()).all()
        assert (out["rel"][..., 0].sum(axis=(1, 2)) == (0 if q["values"] is None else 3 * (~dead).sum())).all()
    assert np.isnan(outs[2]["rec"][..., 1:]).all() and not outs[2]["rel"].any()
    print(f"eval_temperatures V={V}: worst mass error / bound {worst:.3f}")
    # 5. a second launch gives the same bits; without record buffers the tables are the same
    rc, again = launch(problems, temps)
    rc2, lean = launch(problems, temps, with_rec=False)
    assert rc == 0 and rc2 == 0
    for a, b, c in zip(outs, again, lean):
        assert all(same(a[k], b[k]) for k in ("rec", "sum", "rel"))
        assert all(same(a[k], c[k]) for k in ("sum", "rel")) and poisoned(c["rec"])


@pytest.mark.parametrize("V", [3, 257, 1000, 8193])
def test_score_of_drawn_tokens_is_the_samplers_bits(V):
    """Rows drawn by mmt_sample at tau_k, yb set to the drawn token: rec[..., k, 0] is the sampler's log-probability."""
    import mmt_sample
    dev = torch.device("cuda")
    temps = GRIDS[3]
    q = problem(V, "value", bad_tokens=False)
    B, T = shape_of(V)
    lg = torch.from_numpy(q["logits"].reshape(B * T, V).copy()).to(dev)
    for k, tau in enumerate(temps):
        tok, lp = mmt_sample.sample(lg, temperature=float(tau), seed=99 + k, pos=7, return_logprobs=True)
        tok, lp = tok.cpu().numpy().reshape(B, T), lp.cpu().numpy().astype(np.float64).reshape(B, T)
        drawn = ~np.isnan(lp)  # a row with no finite logit gives token 0 and NaN
        assert drawn.sum() == B * T - 1 - (V == 2)
        rc, (out,) = launch([dict(q, yb=tok)], temps)
        assert rc == 0
        assert same(out["rec"][..., k, 0][drawn], lp[drawn]), (V, k)
        assert np.isnan(out["rec"][~drawn]).all()


@pytest.mark.parametrize("K", [1, 32])
def test_one_and_32_temperatures(K):
    temps = GRIDS[K]
    k_one = int(np.nonzero(temps == 1.0)[0][0])
    for V in (3, 257):
        problems = [problem(V, kind) for kind in ("percent", None)]
        rc, outs = launch(problems, temps)
        assert rc == 0
        dead = dead_rows(problems[0])
        sc = scores_at(problems[0], temps)
        rc, pos = positions_launch(problems)
        for p, (q, out) in enumerate(zip(problems, outs)):
            assert same(out["rec"][~dead][..., 0], sc[~dead]) and np.isnan(out["rec"][dead]).all()
            assert same(out["rec"][:, :, k_one, :], pos[p]["rec"][..., 0:4])
            check_records(out, ref_records(q, (V, p, K), temps), V, 0, (V, p, K))
            check_tables(out, q, 0, 10, (V, p, K))
        if K == 32:  # a temperature gives the bits it gives alone and in the grid of three
            rc, (alone,) = launch(problems[:1], temps[16:17])
            rc2, (three,) = launch(problems[:1], GRIDS[3])
            assert rc == 0 and rc2 == 0
            assert same(alone["rec"][:, :, 0], outs[0]["rec"][:, :, 16]) and same(alone["sum"][0], outs[0]["sum"][16])
            assert same(alone["rel"][0], outs[0]["rel"][16]) and same(three["rec"][:, :, 1], alone["rec"][:, :, 0])
            assert same(three["rec"][:, :, 0], outs[0]["rec"][:, :, 0])  # 0.25 is in both grids


def test_t_begin_and_bins():
    V, temps = 257, GRIDS[3]
    q = problem(V, "percent")
    ref = ref_records(q, (V, "percent"), temps)
    full = None
    for t_begin in (0, 2, 5):
        for bins in (1, 10, 64):
            rc, (out,) = launch([q], temps, t_begin=t_begin, bins=bins)
            assert rc == 0
            if t_begin == T0:  # nothing is launched, nothing written
                assert all(poisoned(out[k]) for k in ("rec", "sum", "rel"))
                continue
            check_records(out, ref, V, t_begin, (t_begin, bins))
            check_tables(out, q, t_begin, bins, (t_begin, bins))
            assert (out["sum"][:, 0] == (~dead_rows(q))[:, t_begin:].sum()).all()
            assert (out["rel"][..., 0].sum(axis=(1, 2)) == 3 * out["sum"][:, 0]).all()
            if t_begin == 0 and bins == 10:
                full = out
            elif bins == 10:  # a later start gives the same records
                assert same(out["rec"][:, t_begin:], full["rec"][:, t_begin:])


def test_problems_alone_and_in_company():
    """Three problems of different V in one call, and nine (two chunks; V on both sides of the LDS threshold cannot
    share B x T with the small ones, so the nine are small): every problem gives the bits it gives alone."""
    temps = GRIDS[3]
    mix = [(257, "value"), (3, "percent"), (1000, None), (1, "value"), (2, "percent"), (255, "value"), (257, "percent"),
           (1000, "value"), (3, None)]
    problems = [problem(V, kind) for V, kind in mix]
    rc, nine = launch(problems, temps)
    assert rc == 0
    rc, three = launch(problems[:3], temps)
    assert rc == 0
    for p, q in enumerate(problems):
        rc, (alone,) = launch([q], temps)
        assert rc == 0
        for k in ("rec", "sum", "rel"):
            assert same(nine[p][k], alone[k]), (p, k)
            if p < 3:
                assert same(three[p][k], alone[k]), (p, k)
    big = [problem(8192, "value"), problem(8193, "percent")]  # both record launches in one call
    rc, both = launch(big, temps)
    assert rc == 0
    for p, q in enumerate(big):
        rc, (alone,) = launch([q], temps)
        assert rc == 0 and all(same(both[p][k], alone[k]) for k in ("rec", "sum", "rel"))


def test_accumulate_adds_once_per_cell():
    V, temps = 257, GRIDS[3]
    a, b = problem(V, "value"), problem(V, "value", seed=1)
    for t_begin in (0, 2):
        rc, (ta,) = launch([a], temps, t_begin=t_begin)
        rc2, (tb,) = launch([b], temps, t_begin=t_begin)
        assert rc == 0 and rc2 == 0 and not same(ta["rel"], tb["rel"])
        rc, (acc,) = launch([b], temps, t_begin=t_begin, accumulate=1, init=[(ta["sum"], ta["rel"])])
        assert rc == 0
        assert same(acc["sum"], ta["sum"] + tb["sum"]) and same(acc["rel"], ta["rel"] + tb["rel"]), t_begin
        rc, (twice,) = launch([b], temps, t_begin=t_begin, accumulate=1, init=[(acc["sum"], acc["rel"])])
        assert rc == 0
        assert same(twice["sum"], (ta["sum"] + tb["sum"]) + tb["sum"]) and same(twice["rel"], (ta["rel"] + tb["rel"]) + tb["rel"])
    init = [(np.full((3, 2), 0.5), np.full((3, 3, 10, 3), 0.25))]
    rc, (acc,) = launch([b], temps, t_begin=2, accumulate=1, init=init)
    assert rc == 0 and same(acc["sum"], init[0][0] + tb["sum"]) and same(acc["rel"], init[0][1] + tb["rel"])


def test_refusals_write_nothing():
    V, temps = 3, GRIDS[3]
    q = problem(V, "percent")
    inf, nan = float("inf"), float("nan")

    def clean(outs):
        return all(poisoned(o[k]) for o in outs for k in ("rec", "sum", "rel"))

    for kw in (dict(count=-1), dict(batch=-1), dict(T_=-1), dict(t_begin=-1), dict(t_begin=T0 + 1), dict(bins=0),
               dict(bins=65), dict(V=0), dict(null="V"), dict(null="logits"), dict(null="xb"), dict(null="yb"),
               dict(null="sum"), dict(null="rel"), dict(null="entry:logits"), dict(null="entry:xb"),
               dict(null="entry:yb"), dict(null="entry:sum"), dict(null="entry:rel"), dict(scratch=None),
               dict(nbytes=15), dict(K=0), dict(K=33), dict(K=-1), dict(grid=None), dict(grid=[0.5, 1.0, inf]),
               dict(grid=[0.5, nan, 2.0]), dict(grid=[0.0, 1.0, 2.0]), dict(grid=[-1.0, 1.0, 2.0]),
               dict(grid=[0.5, 0.5, 2.0]), dict(grid=[0.5, 2.0, 1.0])):
        rc, outs = launch([q], temps, **kw)
        assert rc == -1 and clean(outs), (kw, rc)
    rc, outs = launch([q], temps, V=(1 << 20) + 1)
    assert rc == -2 and clean(outs)
    dev = torch.device("cuda")
    off = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    rc, outs = launch([q], temps, scratch=off.data_ptr() + 8)  # misaligned
    assert rc == -1 and clean(outs)
    rc, outs = launch([q], temps, batch=1 << 16, T_=1 << 15)  # 2^31 rows
    assert rc == -1 and clean(outs)
    L = ML.lib()
    assert L.mmt_eval_temperatures_scratch_bytes(1, 3, 5, 10, 0) == -1
    assert L.mmt_eval_temperatures_scratch_bytes(1, 3, 5, 10, 33) == -1
    assert L.mmt_eval_temperatures_scratch_bytes(1, 3, 5, 65, 3) == -1
    assert L.mmt_eval_temperatures_scratch_bytes(2, 3, 5, 10, 3) >= 2 * (15 * 12 + 5 * 3 * 92) * 8
    for kw in (dict(count=0), dict(batch=0), dict(t_begin=T0)):
        rc, outs = launch([q], temps, **kw)
        assert rc == 0 and clean(outs), kw
    rc, outs = launch([q], temps)
    assert rc == 0 and not clean(outs)


def test_python_layer():
    import mmt_eval as ME
    dev = torch.device("cuda")
    V, temps = 257, GRIDS[3]
    problems = [problem(V, k, bad_tokens=False) for k in KINDS]
    lg = [torch.from_numpy(q["logits"].copy()).to(dev) for q in problems]
    xb = [torch.from_numpy(q["xb"].copy()).to(dev) for q in problems]
    yb = [torch.from_numpy(q["yb"].copy()).to(dev) for q in problems]
    val = [None if q["values"] is None else torch.from_numpy(q["values"]).to(dev) for q in problems]
    pct = [q["is_percent"] for q in problems]
    rc, raw = launch(problems, temps, t_begin=2, bins=8)
    assert rc == 0
    got = ME.temperature_metrics(lg, xb, yb, val, pct, temperatures=temps, t_begin=2, bins=8, records=True)
    one = ME.position_metrics(lg, xb, yb, val, pct, t_begin=2, bins=8, records=True)
    for p in range(3):
        assert same(got[p]["sum"].cpu().numpy(), raw[p]["sum"]) and same(got[p]["rel"].cpu().numpy(), raw[p]["rel"])
        rec = got[p]["rec"].cpu().numpy()
        assert np.isnan(rec[:, :2]).all() and same(rec[:, 2:], raw[p]["rec"][:, 2:])
        assert same(rec[:, 2:, 1, :], one[p]["rec"].cpu().numpy()[:, 2:, 0:4])
        # the reliability table at tau = 1 is mmt_eval_positions'
        assert same(got[p]["rel"].cpu().numpy()[1], one[p]["rel"].cpu().numpy())
    assert "rec" not in ME.temperature_metrics(lg, xb, yb, val, pct)[0]
    assert tuple(ME.temperature_metrics(lg, xb, yb, val, pct)[0]["sum"].shape) == (17, 2)
    for bad in ([], [1.0] * 2, [2.0, 1.0], [0.0, 1.0], [1.0, float("inf")], list(range(1, 34)), [[1.0]], ["a"]):
        with pytest.raises(ValueError, match="temperatures"):
            ME.temperature_metrics(lg, xb, yb, val, pct, temperatures=bad)
    with pytest.raises(ValueError, match=r"yb_list\[1\].*outside"):
        ME.temperature_metrics(lg, xb, [yb[0], torch.full_like(yb[1], V), yb[2]], val, pct)
    with pytest.raises(ValueError, match="t_begin"):
        ME.temperature_metrics(lg, xb, yb, val, pct, t_begin=6)
