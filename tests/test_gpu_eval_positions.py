"""mmt_eval_positions (csrc/mmt_evalpos.hip) against mmt_score_multi's bits, the fp64 restatement of both stages
(tests/eval_ref.py) and mmt_eval_direction's counts.

The rows are the 64 of test_gpu_sample.make_rows(V) as [4, 16, V]: N(0, 3^2) rows, the tie rows, the rows with -inf /
NaN entries, the two rows with no finite logit. Tokens are drawn uniformly; two are put outside the vocabulary (the
entry must not read them). Every output buffer lies between guard bands and starts poisoned.

rec[0] is compared bit for bit with mmt_score_multi on the same buffers; signs and ranks exactly with the restatement;
the masses and the PIT within eval_ref.mass_bound (derived there); the tables bit for bit with eval_ref.tables applied to
the DEVICE's own records, so a probability on a bin edge needs no allowance."""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as E
import mmt_lib as ML
from test_gpu_sample import make_rows
from test_gpu_score import score

pytestmark = pytest.mark.gpu

VS = [1, 5, 13, 64, 65, 900, 8193]
B0, T0 = 4, 16
POISON = -7.0
G = 16  # guard doubles on either side of an output
KINDS = ("value", "percent", "repeated", None)
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

_cases = {}


def family(V, kind, seed=0, bad_tokens=True, B=B0, T=T0):
    """One problem over the family's rows: logits fp32 [B, T, V], xb, yb int64 [B, T], values, is_percent. Cached,
    read only."""
    key = (V, kind, B, T, seed, bad_tokens)
    if key not in _cases:
        rng = np.random.default_rng(77 + 13 * V + seed)
        xb, yb = rng.integers(0, V, size=(B, T)), rng.integers(0, V, size=(B, T))
        rows = make_rows(V)
        for r, hit in ((52, np.isneginf(rows[52])), (53, np.isnan(rows[53]))):  # ask for a token that cannot come
            if hit.any():
                yb.reshape(-1)[r] = int(np.argmax(hit))
        if bad_tokens:
            yb.reshape(-1)[1] = V  # outside the vocabulary: dead rows
            xb.reshape(-1)[18] = -1
        values = None if kind is None else E.series(V, "repeated" if kind == "repeated" else "value")
        q = dict(logits=rows.reshape(B, T, V), xb=xb, yb=yb, values=values, is_percent=kind == "percent", V=V)
        for a in (xb, yb):
            a.setflags(write=False)
        _cases[key] = q
    return _cases[key]


_refs = {}


def ref_records(q, key):
    if key not in _refs:
        _refs[key] = E.records(q["logits"], q["xb"], q["yb"], q["values"], q["is_percent"])
        _refs[key].setflags(write=False)
    return _refs[key]


class Guarded:
    """An fp64 device buffer of n doubles between two guard bands, all poisoned (or holding `init`)."""

    def __init__(self, n, dev, init=None):
        self.n = n
        self.t = torch.full((n + 2 * G,), POISON, dtype=torch.float64, device=dev)
        if init is not None:
            self.t[G:G + n] = torch.from_numpy(np.asarray(init, dtype=np.float64).reshape(-1)).to(dev)

    def ptr(self):
        return self.t.data_ptr() + 8 * G

    def get(self, shape):
        host = self.t.cpu().numpy()
        assert (host[:G] == POISON).all() and (host[G + self.n:] == POISON).all(), "wrote outside its buffer"
        return host[G:G + self.n].reshape(shape).copy()


def launch(problems, t_begin=0, bins=10, accumulate=0, with_rec=True, init=None, B=None, T=None, **over):
    """One mmt_eval_positions over `problems` (family dicts). init: per problem (pos, rel, pit) to start from. `over`
    replaces raw arguments (count, batch, T_, V, scratch, nbytes, null=<name of an array or entry to pass as NULL>).
    Returns (status, [dict(rec, pos, rel, pit)]); every buffer is checked for writes outside it."""
    dev = torch.device("cuda")
    P = len(problems)
    B = problems[0]["logits"].shape[0] if B is None else B
    T = problems[0]["logits"].shape[1] if T is None else T
    L = ML.lib()
    bb = min(max(bins, 1), 64)  # the buffers' bins: a refused `bins` still gets buffers to leave untouched
    keep, bufs = [], []
    arr = {k: (vp * max(P, 1))() for k in ("logits", "xb", "yb", "values", "rec", "pos", "rel", "pit")}
    for p, q in enumerate(problems):
        d = {k: torch.from_numpy(np.array(q[k])).to(dev) for k in ("logits", "xb", "yb")}
        d["values"] = None if q["values"] is None else torch.from_numpy(q["values"]).to(dev)
        keep.append(d)
        g = dict(rec=Guarded(B * T * 8, dev), pos=Guarded(T * 8, dev, init and init[p][0]),
                 rel=Guarded(9 * bb, dev, init and init[p][1]), pit=Guarded(bb, dev, init and init[p][2]))
        bufs.append(g)
        for k in ("logits", "xb", "yb"):
            arr[k][p] = d[k].data_ptr()
        arr["values"][p] = None if d["values"] is None else d["values"].data_ptr()
        arr["rec"][p] = g["rec"].ptr() if with_rec else None
        for k in ("pos", "rel", "pit"):
            arr[k][p] = g[k].ptr()
    null = over.get("null")
    if null in arr:
        arr[null] = None
    elif null is not None and null.startswith("entry:"):
        arr[null.split(":")[1]][0] = None
    V = (i32 * max(P, 1))(*[over.get("V", q["V"]) for q in problems]) if null != "V" else None
    pct = (i32 * max(P, 1))(*[1 if q["is_percent"] else 0 for q in problems])
    need = L.mmt_eval_positions_scratch_bytes(P, B, T, bb)
    assert need >= 0
    scratch = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=dev)
    sp = over.get("scratch", scratch.data_ptr())
    rc = L.mmt_eval_positions(ML.stream_ptr(dev), over.get("count", P), over.get("batch", B), over.get("T_", T), t_begin,
                              bins, accumulate, V, arr["logits"], arr["xb"], arr["yb"], arr["values"], pct, arr["rec"],
                              arr["pos"], arr["rel"], arr["pit"], sp, over.get("nbytes", need))
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0xAB).all()), "wrote past the scratch"
    out = [dict(rec=g["rec"].get((B, T, 8)), pos=g["pos"].get((T, 8)), rel=g["rel"].get((3, bb, 3)),
                pit=g["pit"].get((bb,))) for g in bufs]
    return rc, out


def same(a, b):
    return np.array_equal(E.bits(a), E.bits(b))


def check_tables(out, t_begin, bins, what):
    """The device's tables are eval_ref.tables of the device's own records, bit for bit."""
    pos, rel, pit = E.tables(out["rec"], t_begin, bins)
    for name, want in (("pos", pos), ("rel", rel), ("pit", pit)):
        assert same(out[name], want), (what, name, out[name], want)


def check_records(out, q, ref, V, t_begin, what):
    rec = out["rec"]
    B, T = rec.shape[:2]
    assert (rec[:, :t_begin] == POISON).all(), (what, "records before t_begin were written")
    got, want = rec[:, t_begin:], ref[:, t_begin:]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want)))
    for k in (5, 6, 7):  # rank and signs: exact
        ok = ~np.isnan(want[..., k])
        assert np.array_equal(got[..., k][ok], want[..., k][ok]), (what, k)
    worst = 0.0
    for k in (1, 2, 3, 4):  # masses and the PIT: the derived bound
        ok = ~np.isnan(want[..., k])
        err, bound = np.abs(got[..., k][ok] - want[..., k][ok]), E.mass_bound(want[..., k][ok], V)
        if err.size:
            worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (what, k, float(err.max()), np.argwhere(~(err <= bound)))
    return worst


@pytest.mark.parametrize("V", VS)
def test_records_and_tables(V):
    """Four problems in one launch: a value series, a percent series, a series with repeated values, no values."""
    problems = [family(V, kind) for kind in KINDS]
    rc, outs = launch(problems)
    assert rc == 0
    # rec[0]: mmt_score_multi's bits on the same rows and tokens
    dev = torch.device("cuda")
    q0 = problems[0]
    lg = torch.from_numpy(q0["logits"].reshape(64, V).copy()).to(dev)
    tok = torch.from_numpy(q0["yb"].reshape(64).copy()).to(dev)
    (sc,), src = score([dict(logits=lg, V=V, tok=tok)], 64)
    assert src == 0
    sc = sc.numpy().astype(np.float64).reshape(B0, T0)
    live = ~np.isnan(outs[0]["rec"][..., 5])
    assert live.sum() >= 60 and not live.reshape(-1)[[1, 18, 56, 58]].any()
    for p, out in enumerate(outs):
        assert same(out["rec"][..., 0][live], sc[live]), (V, p)
        assert np.isnan(out["rec"][~live]).all()
    for r, hit in ((52, np.isneginf(make_rows(V)[52])), (53, np.isnan(make_rows(V)[53]))):
        if hit.any():  # a token whose logit is -inf or NaN was asked for: it scores -inf
            assert np.isneginf(outs[0]["rec"].reshape(64, 8)[r, 0]) and np.isinf(outs[0]["pos"][r % T0, 4])
    worst = 0.0
    for p, (q, out) in enumerate(zip(problems, outs)):
        worst = max(worst, check_records(out, q, ref_records(q, (V, KINDS[p])), V, 0, (V, KINDS[p])))
        check_tables(out, 0, 10, (V, KINDS[p]))
        assert out["pos"][:, 0].sum() == live.sum()
    assert np.isnan(outs[3]["rec"][..., [1, 2, 3, 6, 7]]).all() and not outs[3]["pos"][:, [1, 2, 3, 6, 7]].any()
    assert not outs[3]["rel"].any() and outs[3]["pit"].sum() == live.sum()
    if V > 1:
        assert (outs[2]["rec"][..., 2][live] > 0).any(), "the flat class is exercised"
    print(f"eval_positions V={V}: worst mass error / bound {worst:.3f}")
    # a second launch gives the same bits; without record buffers the tables are the same
    rc, again = launch(problems)
    rc2, lean = launch(problems, with_rec=False)
    assert rc == 0 and rc2 == 0
    for a, b, c in zip(outs, again, lean):
        assert all(same(a[k], b[k]) for k in ("rec", "pos", "rel", "pit"))
        assert all(same(a[k], c[k]) for k in ("pos", "rel", "pit")) and (c["rec"] == POISON).all()


@pytest.mark.parametrize("V", [13, 900])
def test_last_position_counts_are_mmt_eval_direction(V):
    """The family without its dead rows as 62 windows of one position (T = 1): wins and losses of position T - 1 are
    the counts mmt_eval_direction gives on the same inputs."""
    dev = torch.device("cuda")
    rows = make_rows(V)[[r for r in range(64) if r not in (56, 58)]]
    B = len(rows)
    rng = np.random.default_rng(5 + V)
    for kind in ("value", "percent", "repeated"):
        q = dict(logits=rows.reshape(B, 1, V), xb=rng.integers(0, V, size=(B, 1)), yb=rng.integers(0, V, size=(B, 1)),
                 values=E.series(V, "repeated" if kind == "repeated" else "value"), is_percent=kind == "percent", V=V)
        rc, (out,) = launch([q])
        assert rc == 0 and out["pos"][0, 0] == B
        check_tables(out, 0, 10, (V, kind))
        acc_i = torch.zeros(2, dtype=torch.int32, device=dev)
        acc_c = torch.zeros(1, dtype=torch.float64, device=dev)
        t = {k: torch.from_numpy(np.array(q[k])).to(dev) for k in ("logits", "xb", "yb", "values")}
        rc = ML.lib().mmt_eval_direction(None, ML.stream_ptr(dev), B, 1, V, ML.ptr(t["logits"]), ML.ptr(t["xb"]),
                                         ML.ptr(t["yb"]), ML.ptr(t["values"]), 1 if q["is_percent"] else 0,
                                         ML.ptr(acc_i), ML.ptr(acc_c))
        assert rc == 0
        assert [int(out["pos"][0, 1]), int(out["pos"][0, 2])] == acc_i.tolist(), (V, kind)


def test_t_begin_and_bins():
    V = 65
    q = family(V, "percent")
    ref = ref_records(q, (V, "percent"))
    full = None
    for t_begin in (0, 5, T0 - 1, T0):
        for bins in (1, 10, 64):
            rc, (out,) = launch([q], t_begin=t_begin, bins=bins)
            assert rc == 0
            if t_begin == T0:  # nothing is launched, nothing written
                assert all((out[k] == POISON).all() for k in ("rec", "pos", "rel", "pit"))
                continue
            check_records(out, q, ref, V, t_begin, (t_begin, bins))
            check_tables(out, t_begin, bins, (t_begin, bins))
            assert not out["pos"][:t_begin].any() and out["pit"].sum() == out["pos"][:, 0].sum()
            assert out["rel"][:, :, 0].sum() == 3 * out["pos"][:, 6].sum()
            if t_begin == 0 and bins == 10:
                full = out
            elif bins == 10:  # a later start gives the same records and the same position rows
                assert same(out["rec"][:, t_begin:], full["rec"][:, t_begin:])
                assert same(out["pos"][t_begin:], full["pos"][t_begin:])


def test_problems_alone_and_in_company():
    """count 1, 3 and 9 (two chunks; V on both sides of the LDS threshold in one call): every problem gives the bits
    it gives alone."""
    mix = [(65, "value"), (13, "percent"), (8193, "repeated"), (5, None), (1, "value"), (900, "percent"),
           (64, "repeated"), (65, "percent"), (8193, "value")]
    problems = [family(V, kind) for V, kind in mix]
    rc, nine = launch(problems)
    assert rc == 0
    rc, three = launch(problems[:3])
    assert rc == 0
    for p, q in enumerate(problems):
        rc, (alone,) = launch([q])
        assert rc == 0
        for k in ("rec", "pos", "rel", "pit"):
            assert same(nine[p][k], alone[k]), (p, k)
            if p < 3:
                assert same(three[p][k], alone[k]), (p, k)
        check_tables(alone, 0, 10, mix[p])


def test_accumulate_adds_in_order():
    V = 65
    a, b = family(V, "repeated"), family(V, "repeated", seed=1)
    for t_begin in (0, 5):
        rc, (ta,) = launch([a], t_begin=t_begin)
        rc2, (tb,) = launch([b], t_begin=t_begin)
        assert rc == 0 and rc2 == 0 and not same(ta["pos"], tb["pos"])
        rc, (acc,) = launch([b], t_begin=t_begin, accumulate=1, init=[(ta["pos"], ta["rel"], ta["pit"])])
        assert rc == 0
        for k in ("pos", "rel", "pit"):
            assert same(acc[k], ta[k] + tb[k]), (t_begin, k)
    # and onto whatever the buffers hold, rows before t_begin included
    init = [(np.full((T0, 8), 0.5), np.full((3, 10, 3), 0.25), np.full(10, 2.0))]
    rc, (acc,) = launch([b], t_begin=5, accumulate=1, init=init)
    assert rc == 0 and same(acc["pos"], init[0][0] + tb["pos"]) and same(acc["rel"], init[0][1] + tb["rel"])
    assert same(acc["pit"], init[0][2] + tb["pit"])


def test_batch_of_one_and_one_position():
    V = 13
    rows = make_rows(V)
    rng = np.random.default_rng(3)
    for B, T in ((1, 64), (64, 1), (1, 1)):
        n = B * T
        q = dict(logits=rows[:n].reshape(B, T, V), xb=rng.integers(0, V, size=(B, T)), yb=rng.integers(0, V, size=(B, T)),
                 values=E.series(V, "repeated"), is_percent=False, V=V)
        rc, (out,) = launch([q], bins=7)
        assert rc == 0
        ref = E.records(q["logits"], q["xb"], q["yb"], q["values"], False)
        check_records(out, q, ref, V, 0, (B, T))
        check_tables(out, 0, 7, (B, T))
        assert out["pos"][:, 0].sum() == n - (2 if n == 64 else 0)


def test_refusals_write_nothing():
    V = 13
    q = family(V, "percent")

    def clean(outs):
        return all((o[k] == POISON).all() for o in outs for k in ("rec", "pos", "rel", "pit"))

    for kw in (dict(count=-1), dict(batch=-1), dict(T_=-1), dict(t_begin=-1), dict(t_begin=T0 + 1), dict(bins=0),
               dict(bins=65), dict(V=0), dict(null="V"), dict(null="logits"), dict(null="xb"), dict(null="yb"),
               dict(null="pos"), dict(null="rel"), dict(null="pit"), dict(null="entry:logits"), dict(null="entry:xb"),
               dict(null="entry:yb"), dict(null="entry:pos"), dict(null="entry:rel"), dict(null="entry:pit"),
               dict(scratch=None), dict(nbytes=15)):
        rc, outs = launch([q], **kw)
        assert rc == -1 and clean(outs), (kw, rc)
    rc, outs = launch([q], V=(1 << 20) + 1)
    assert rc == -2 and clean(outs)
    dev = torch.device("cuda")
    off = torch.empty(4096, dtype=torch.uint8, device=dev)
    rc, outs = launch([q], scratch=off.data_ptr() + 8)  # misaligned
    assert rc == -1 and clean(outs)
    rc, outs = launch([q], batch=1 << 16, T_=1 << 15)  # 2^31 rows
    assert rc == -1 and clean(outs)
    for kw in (dict(count=0), dict(batch=0), dict(t_begin=T0)):
        rc, outs = launch([q], **kw)
        assert rc == 0 and clean(outs), kw
    rc, outs = launch([q])
    assert rc == 0 and not clean(outs)


def test_python_layer():
    import mmt_eval as ME
    dev = torch.device("cuda")
    V = 65
    kinds = ("value", "percent", None)
    problems = [family(V, k, bad_tokens=False) for k in kinds]
    lg = [torch.from_numpy(q["logits"].copy()).to(dev) for q in problems]
    xb = [torch.from_numpy(q["xb"].copy()).to(dev) for q in problems]
    yb = [torch.from_numpy(q["yb"].copy()).to(dev) for q in problems]
    val = [None if q["values"] is None else torch.from_numpy(q["values"]).to(dev) for q in problems]
    pct = [q["is_percent"] for q in problems]
    rc, raw = launch(problems, t_begin=3, bins=8)
    assert rc == 0
    got = ME.position_metrics(lg, xb, yb, val, pct, t_begin=3, bins=8, records=True)
    for p in range(3):
        for k in ("pos", "rel", "pit"):
            assert same(got[p][k].cpu().numpy(), raw[p][k]), (p, k)
        rec = got[p]["rec"].cpu().numpy()
        assert np.isnan(rec[:, :3]).all() and same(rec[:, 3:], raw[p]["rec"][:, 3:])
    assert "rec" not in ME.position_metrics(lg, xb, yb, val, pct)[0]
    # two accumulated batches are the sum of the two; one read at the end
    pm = ME.PositionMetrics(val, pct, t_begin=3, bins=8)
    pm.add(lg, xb, yb)
    pm.add(lg, yb, xb)
    _, swapped = launch([dict(q, xb=q["yb"], yb=q["xb"]) for q in problems], t_begin=3, bins=8)
    res = pm.result()
    assert pm.batches == 2 and len(res) == 3
    for p in range(3):
        for k in ("pos", "rel", "pit"):
            assert same(res[p][k], raw[p][k] + swapped[p][k]), (p, k)
        want = ME.derive(res[p]["pos"], res[p]["rel"], res[p]["pit"], 3)
        assert res[p]["wins"] == want["wins"] == int(res[p]["pos"][:, 1].sum()) and res[p]["rows"] == 2 * (4 * 13 - 2)
    lines = pm.summary_lines(["a", "b", "c"], res)
    assert len(lines) == 3 and lines[2].startswith("  - c" + " " * 29 + "No directional predictions | NLL ")
    assert f"{res[0]['wins']}/{res[0]['wins'] + res[0]['losses']} (" in lines[0] and " | ECE up 0." in lines[0]
    # refusals that need the logits on a GPU to be reached
    with pytest.raises(ValueError, match=r"logits_list\[1\].*contiguous"):
        ME.position_metrics([lg[0], lg[1].transpose(0, 1).contiguous().transpose(0, 1), lg[2]], xb, yb, val, pct)
    with pytest.raises(ValueError, match=r"xb_list\[0\].*int64"):
        ME.position_metrics(lg, [xb[0].int(), xb[1], xb[2]], yb, val, pct)
    with pytest.raises(ValueError, match=r"yb_list\[2\].*int64 \[4, 16\]"):
        ME.position_metrics(lg, xb, [yb[0], yb[1], yb[2][:, :8]], val, pct)
    with pytest.raises(ValueError, match=r"yb_list\[1\].*GPU"):
        ME.position_metrics(lg, xb, [yb[0], yb[1].cpu(), yb[2]], val, pct)
    with pytest.raises(ValueError, match=r"xb_list\[1\].*contiguous"):
        ME.position_metrics(lg, [xb[0], xb[1].t().contiguous().t(), xb[2]], yb, val, pct)
    with pytest.raises(ValueError, match=r"values\[0\].*fp64 \[65\]"):
        ME.position_metrics(lg, xb, yb, [val[0].float(), val[1], None], pct)
    with pytest.raises(ValueError, match=r"values\[1\].*GPU"):
        ME.position_metrics(lg, xb, yb, [val[0], val[1].cpu(), None], pct)
    with pytest.raises(ValueError, match="t_begin"):
        ME.position_metrics(lg, xb, yb, val, pct, t_begin=17)
    bad = yb[1].clone()
    bad[2, 3] = V
    with pytest.raises(ValueError, match=r"yb_list\[1\].*outside 0\.\.64"):
        ME.position_metrics(lg, xb, [yb[0], bad, yb[2]], val, pct)
    bad = xb[0].clone()
    bad[0, 0] = -1
    with pytest.raises(ValueError, match=r"xb_list\[0\].*outside"):
        ME.position_metrics(lg, [bad, xb[1], xb[2]], yb, val, pct)
    with pytest.raises(ValueError, match="first batch"):
        pm.add([t[:2] for t in lg], [t[:2] for t in xb], [t[:2] for t in yb])
