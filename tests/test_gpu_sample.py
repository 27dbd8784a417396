"""mmt_sample (csrc/mmt_sample.hip) against the CPU restatement of its rule (tests/sampling_ref.py).

Tokens are compared under the clear / ambiguous rule: a row whose margins (distance of u * S to the nearest prefix
boundary, of top_p * S to the nearest group mass, both relative to S) are at least delta must give the reference's
token; a closer row may give the reference's token or the neighbour across that boundary. At most 5 % of the rows
of any case may be ambiguous.

delta, from the kernel's summation tree. The weights e_i = exp(z_i - m) are fp32, every sum of them is fp64:
thread t owns c = ceil(V / 256) | 1 consecutive elements, and the prefix the kernel compares with u * S is the thread's
serial total (c additions), a 6-step shift scan over the lanes, the wave totals left to right (3), wave base + lane
offset (1) and the owner's serial walk over its chunk (c); S is the same tree without the walk. That is 2 c + 10 and
c + 9 roundings of 2^-53 each relative to a partial sum that is at most S. A weight carries the error of expf, for
which the bound taken is OpenCL's 3 ulp (of 2^-23), and the rounding of the fp32 subtraction z - m, 2^-24 |z - m|
relative; summed over the row with the weights e_i / S the latter is 2^-24 (H - log S) <= 2^-24 ln V (H the entropy
of the distribution), i.e. ln(V) / 2 ulps. The prefix and S both carry the weight error. u * S and the comparison
are fp64 on the device and exact here. So, as (serial terms + tree depth) roundings plus the exp error in ulps,

    delta(V) = (3 c + 19) * 2^-53 + 2 (3 + ln(V) / 2) * 2^-23        (1.5e-6 at V = 900, 1.8e-6 at V = 8193)

The masses of the top-p search are fp64 sums of the same weights over the interleaved assignment and top_p * S one
more fp64 multiply: the same delta bounds margin_p.

Log-probabilities: the kernel computes (z_tok - m) - log(S), the subtraction z_tok - m in fp32 (2^-24 |z_tok - m|,
and |z_tok - m| <= |lp| + ln V), log and the difference in fp64, rounded to fp32 once (2^-24 |lp|). S is off by at
most delta relative, which log turns into delta absolute: |lp - ref| <= delta + 2^-23 (|ref| + ln V + 1).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import mmt_lib as ML
import sampling_ref as R

pytestmark = pytest.mark.gpu

ONCHIP = 8192  # rows up to this V stay in LDS (csrc/mmt_sample.hip SAMPLE_ONCHIP)
VS = [1, 5, 13, 63, 64, 65, 144, 255, 256, 257, 900, ONCHIP, 8193]
SEED = 0x5EED0123456789AB


def settings(V):
    return [(1.0, 0, 1.0), (0.8, 8, 1.0), (0.8, 0, 0.9), (1.3, 50, 0.5), (1.0, 1, 1.0), (1.0, V + 5, 1.0),
            (1.0, 0, 1e-6), (0.0, 7, 0.3)]


def delta(V):
    c = ((V + 255) // 256) | 1
    return (3 * c + 19) * 2.0 ** -53 + 2 * (3 + math.log(V) / 2) * 2.0 ** -23


def lp_tol(V, ref_lp):
    return delta(V) + 2.0 ** -23 * (np.abs(ref_lp) + math.log(V) + 1)


_rows = {}


def make_rows(V, B=64):
    """[B, V] fp32: N(0, 3^2) rows, and from row 48 on (when B = 64) the edge rows. Cached per shape, read only."""
    if (V, B) in _rows:
        return _rows[(V, B)]
    rng = np.random.default_rng(1000 + V)
    x = rng.normal(0.0, 3.0, size=(B, V)).astype(np.float32)
    if B == 64:
        for b in range(48, 52):  # few distinct values: exact ties at the top-k threshold and at the maximum
            x[b] = rng.integers(-4, 3, size=V).astype(np.float32) * np.float32(0.5)
            x[b, rng.integers(0, V, size=min(V, 3))] = 1.5
        for b in range(52, 56):  # -inf and NaN entries, never chosen
            x[b, rng.integers(0, V, size=max(1, V // 3))] = -np.inf
            x[b, rng.integers(0, V, size=max(1, V // 5))] = np.nan
            x[b, int(rng.integers(0, V))] = 0.25  # at least one finite entry
        x[56] = -np.inf  # no finite logit
        x[57] = 1.25  # all equal
        x[58] = np.nan
    x.setflags(write=False)
    _rows[(V, B)] = x
    return x


def launch(logits, V, B, t, k, p, pos, row0=0, row_stride=None, tok_stride=1, want_lp=True, compact=False, offset=0,
           seed=SEED):
    """One mmt_sample launch on `logits` (a device tensor; row b at element offset + b * row_stride). Returns
    (tokens [B], logprobs [B] | None, compact [B] | None) as CPU tensors, and the raw status."""
    dev = logits.device
    tok = torch.full((B, tok_stride), -7, dtype=torch.int64, device=dev)
    lp = torch.full((B, 3), 123.0, dtype=torch.float32, device=dev) if want_lp else None
    cmp_ = torch.full((B,), -7, dtype=torch.int64, device=dev) if compact else None
    rc = ML.lib().mmt_sample(ML.stream_ptr(dev), B, V, logits.data_ptr() + 4 * offset, row_stride or V, t, k, p, seed,
                             row0, pos, tok.data_ptr() + 8 * (tok_stride - 1), tok_stride, ML.ptr(cmp_),
                             (lp.data_ptr() + 4) if want_lp else None, 3)
    torch.cuda.synchronize()
    if tok_stride > 1:
        assert bool((tok[:, :-1] == -7).all()), "wrote outside its token column"
    if want_lp:
        assert bool((lp[:, 0] == 123.0).all()) and bool((lp[:, 2] == 123.0).all()), "wrote outside its logprob column"
    return tok[:, -1].cpu(), (lp[:, 1].cpu() if want_lp else None), (cmp_.cpu() if compact else None), rc


def compare(V, x, t, k, p, pos, tok, lp, row0=0, seed=SEED, what=""):
    ref = R.sample_rows(x, t, k, p, seed, pos, row0)
    d = delta(V)
    amb, bad = R.check_tokens(ref, tok.numpy(), d)
    print(f"{what} V={V} t={t} k={k} p={p}: ambiguous {amb}/{len(x)} delta {d:.2e}")
    assert not bad, (what, V, t, k, p, bad, tok.numpy()[bad], ref["token"][bad], ref["neighbor"][bad])
    assert amb <= 0.05 * len(x), (what, V, amb)
    clear = (ref["margin_u"] >= d) & (ref["margin_p"] >= d)
    if lp is not None:
        got, want = lp.numpy().astype(np.float64), ref["logprob"]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, V)
        sel = clear & ~nan
        err = np.abs(got[sel] - want[sel])
        assert np.all(err <= lp_tol(V, want[sel])), (what, V, t, k, p, float(err.max()))
    return ref, amb


@pytest.mark.parametrize("V", VS)
def test_sample_matches_rule(V):
    """Every setting at B = 64 (N(0, 3^2) rows, tie rows, rows with -inf / NaN entries, a row without a finite logit,
    an all-equal row), contiguous rows, with the compact copy and a token column of stride 3."""
    x = make_rows(V)
    xd = torch.from_numpy(x.copy()).cuda()
    for j, (t, k, p) in enumerate(settings(V)):
        tok, lp, cmp_, rc = launch(xd, V, 64, t, k, p, pos=11 + j, tok_stride=3, compact=True)
        assert rc == 0
        assert torch.equal(tok, cmp_)
        assert int(tok.min()) >= 0 and int(tok.max()) < V
        ref, _ = compare(V, x, t, k, p, 11 + j, tok, lp, what="rule")
        assert int(tok[56]) == 0 and int(tok[58]) == 0 and math.isnan(float(lp[56])) and math.isnan(float(lp[58]))
        if t == 0.0:  # greedy is exact everywhere, lowest index on ties
            assert np.array_equal(tok.numpy(), ref["token"])
        for b in range(52, 56):
            assert math.isfinite(float(x[b, int(tok[b])])), "chose a -inf / NaN entry"


@pytest.mark.parametrize("V", [13, 257, 900, 8193])
@pytest.mark.parametrize("B", [1, 3])
def test_sample_strides_and_row0(V, B):
    """row_stride V + 7 and 4 V (the last position of a [B, 4, V] tensor, read in place), row0 != 0, small batches."""
    rng = np.random.default_rng(77 + V + B)
    for (t, k, p) in settings(V)[:4] + settings(V)[-1:]:
        full = rng.normal(0.0, 3.0, size=(B, 4, V)).astype(np.float32)
        fd = torch.from_numpy(full).cuda()
        tok, lp, _, rc = launch(fd, V, B, t, k, p, pos=5, row0=1000, row_stride=4 * V, offset=3 * V)
        assert rc == 0
        compare(V, full[:, 3, :], t, k, p, 5, tok, lp, row0=1000, what="[B,4,V]")
        padded = np.full((B, V + 7), np.float32(50.0))  # a huge logit in the pad: reading it would win every draw
        padded[:, :V] = full[:, 0, :]
        pd = torch.from_numpy(padded.astype(np.float32)).cuda()
        tok, lp, _, rc = launch(pd, V, B, t, k, p, pos=6, row0=3, row_stride=V + 7)
        assert rc == 0
        compare(V, full[:, 0, :], t, k, p, 6, tok, lp, row0=3, what="V+7")


def test_sample_top_p_midpoint_family_has_no_ambiguous_row():
    """One multiset of probabilities, permuted per row, top_p at the midpoint between two consecutive cumulative
    masses: margin_p is large by construction, and no row may be ambiguous."""
    rng = np.random.default_rng(5)
    V, B = 144, 64
    probs = np.exp(rng.normal(0.0, 1.5, size=V))
    probs = np.sort(probs / probs.sum())[::-1]
    cum = np.cumsum(probs)
    x = np.stack([np.log(probs)[rng.permutation(V)] for _ in range(B)]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    for j in (0, 3, 10, 40):
        top_p = float(np.float32(0.5 * (cum[j] + cum[j + 1])))
        tok, lp, _, rc = launch(xd, V, B, 1.0, 0, top_p, pos=j)
        assert rc == 0
        ref, amb = compare(V, x, 1.0, 0, top_p, j, tok, lp, what="midpoint")
        assert amb == 0
        assert float(ref["margin_p"].min()) > 0.25 * probs[j + 1]
        assert all(int(r.sum()) == j + 2 for r in ref["kept"])


def test_sample_is_deterministic_and_batch_independent():
    """Two launches give identical bytes; rows of a B = 64 launch equal the same rows launched alone with the matching
    row0, bit for bit (tokens and log-probabilities)."""
    for V in (900, 8193):
        x = make_rows(V)
        xd = torch.from_numpy(x.copy()).cuda()
        for (t, k, p) in ((0.8, 0, 0.9), (1.3, 50, 0.5), (1.0, 0, 1.0)):
            a = launch(xd, V, 64, t, k, p, pos=9)
            b = launch(xd, V, 64, t, k, p, pos=9)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
            for r in (0, 17, 50, 57, 63):
                one = launch(xd, V, 1, t, k, p, pos=9, row0=r, offset=r * V)
                assert int(one[0][0]) == int(a[0][r]), (V, r)
                assert one[1].view(torch.int32)[0] == a[1].view(torch.int32)[r], (V, r)
            part = launch(xd, V, 3, t, k, p, pos=9, row0=40, offset=40 * V)
            assert torch.equal(part[0], a[0][40:43])
            other = launch(xd, V, 64, t, k, p, pos=10)
            assert not torch.equal(other[0], a[0])  # another position draws anew


def test_sample_optional_outputs_and_public_wrapper():
    import mmt_sample
    V = 144
    x = make_rows(V)
    xd = torch.from_numpy(x.copy()).cuda()
    tok, lp, _, rc = launch(xd, V, 64, 0.8, 8, 0.95, pos=3, want_lp=False)
    assert rc == 0 and lp is None
    t2, l2 = mmt_sample.sample(xd, temperature=0.8, top_k=8, top_p=0.95, seed=SEED, pos=3, return_logprobs=True)
    assert torch.equal(t2.cpu(), tok)
    t3 = mmt_sample.sample(xd[8:], temperature=0.8, top_k=8, top_p=0.95, seed=SEED, pos=3, row0=8)
    assert torch.equal(t3.cpu(), tok[8:])
    full = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[:, None, :], (64, 2, V)))).cuda()
    t4 = mmt_sample.sample(full[:, -1, :], temperature=0.8, top_k=8, top_p=0.95, seed=SEED, pos=3)
    assert torch.equal(t4.cpu(), tok)
    with pytest.raises(ValueError):
        mmt_sample.sample(xd, temperature=-1.0, seed=1, pos=0)
    with pytest.raises(ValueError):
        mmt_sample.sample(xd.double(), seed=1, pos=0)


def test_sample_rejects_invalid_arguments_before_launching():
    V, B = 13, 3
    xd = torch.zeros(B, V, dtype=torch.float32, device="cuda")
    L = ML.lib()
    nan = float("nan")

    def call(V_=V, stride=V, t=1.0, k=0, p=1.0, logits=xd, B_=B):
        tok = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        rc = L.mmt_sample(ML.stream_ptr(xd.device), B_, V_, ML.ptr(logits), stride, t, k, p, 1, 0, 0, tok.data_ptr(), 1,
                          None, None, 1)
        torch.cuda.synchronize()
        return rc, tok.cpu()

    for kw in (dict(V_=0), dict(V_=-3), dict(stride=V - 1), dict(t=-0.5), dict(t=nan), dict(k=-1), dict(p=nan),
               dict(logits=None), dict(B_=-1)):
        rc, tok = call(**kw)
        assert rc == -1, kw  # MMT_ERR_INVALID
        assert bool((tok == -7).all()), kw  # nothing launched
    rc, tok = call()
    assert rc == 0 and bool((tok >= 0).all())
