"""mmt_score_multi (csrc/mmt_sample.hip): the log-probability of a given token, against the sampler's own bits and
against the CPU restatement of the rule.

The score of token t is what mmt_sample writes when it draws t at (temperature 1, top_k 0, top_p 1): the same device
code, so the comparison with the sampler is bit for bit. Against the fp64 restatement the bound is the sampler
tests' `lp_tol(V, ref)` (test_gpu_sample.py: S off by delta relative, the fp32 subtraction z_t - m, one rounding of
the result), which holds for any token of the row, not only a likely one: |z_t - m| <= |lp| + ln V."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mmt_lib as ML
from test_gpu_sample import launch as sample_launch, lp_tol, make_rows

pytestmark = pytest.mark.gpu

VS = [1, 5, 13, 64, 65, 900, 8193]
GUARD = 123.0


def score(problems, B):
    """One mmt_score_multi over `problems`: dicts with logits (device tensor), V, tok (device int64) and optionally
    offset (elements), row_stride, tok_stride. Outputs go to column 1 of [B, 3] buffers whose other columns are
    guards. Returns (list of CPU fp32 [B], status)."""
    P = len(problems)
    dev = problems[0]["logits"].device
    outs = [torch.full((B, 3), GUARD, dtype=torch.float32, device=dev) for _ in range(P)]
    V = (ctypes.c_int32 * P)(*[q["V"] for q in problems])
    lg = (ctypes.c_void_p * P)(*[q["logits"].data_ptr() + 4 * q.get("offset", 0) for q in problems])
    rs = (ctypes.c_int64 * P)(*[q.get("row_stride", q["V"]) for q in problems])
    tk = (ctypes.c_void_p * P)(*[q["tok"].data_ptr() for q in problems])
    ts = (ctypes.c_int64 * P)(*[q.get("tok_stride", 1) for q in problems])
    lp = (ctypes.c_void_p * P)(*[o.data_ptr() + 4 for o in outs])
    ls = (ctypes.c_int64 * P)(*[3] * P)
    rc = ML.lib().mmt_score_multi(ML.stream_ptr(dev), P, B, V, lg, rs, tk, ts, lp, ls)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[:, 0] == GUARD).all()) and bool((o[:, 2] == GUARD).all()), "wrote outside its column"
    return [o[:, 1].cpu() for o in outs], rc


def ref_logprob(x, tok):
    """fp64 log-softmax of the raw logits at tok; NaN logits as -inf; a row with no finite logit gives NaN."""
    z = x.astype(np.float64)
    z[np.isnan(z)] = -np.inf
    m = z.max(axis=1)
    out = np.full(len(x), np.nan)
    for b in range(len(x)):
        if m[b] == -np.inf:
            continue
        with np.errstate(all="ignore"):
            e = np.where(z[b] == m[b], 1.0, np.exp(z[b] - m[b]))
        zt = z[b, tok[b]]
        out[b] = -np.inf if zt == -np.inf else (0.0 if zt == m[b] else zt - m[b]) - math.log(e.sum())
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", VS)
def test_score_of_drawn_tokens_is_the_samplers_bits(V):
    x = make_rows(V)
    xd = torch.from_numpy(x.copy()).cuda()
    tok, lp, _, rc = sample_launch(xd, V, 64, 1.0, 0, 1.0, pos=21)
    assert rc == 0
    (got,), rc = score([dict(logits=xd, V=V, tok=tok.cuda())], 64)
    assert rc == 0
    assert torch.equal(bits(got), bits(lp)), (V, got, lp)
    assert math.isnan(float(got[56])) and math.isnan(float(got[58]))  # no finite logit


@pytest.mark.parametrize("V", VS)
def test_score_of_arbitrary_tokens_follows_the_rule(V):
    x = make_rows(V)
    xd = torch.from_numpy(x.copy()).cuda()
    rng = np.random.default_rng(31 + V)
    z = np.where(np.isnan(x), -np.inf, x)
    for name, tok in (("random", rng.integers(0, V, size=64)), ("least likely", z.argmin(axis=1)),
                      ("most likely", z.argmax(axis=1))):
        tok = tok.astype(np.int64)
        (got,), rc = score([dict(logits=xd, V=V, tok=torch.from_numpy(tok).cuda())], 64)
        assert rc == 0
        got, want = got.numpy().astype(np.float64), ref_logprob(x, tok)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (V, name)
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), (V, name)
        fin = np.isfinite(want)
        err = np.abs(got[fin] - want[fin])
        print(f"V={V} {name}: max err {err.max() if fin.any() else 0:.3e}")
        assert np.all(err <= lp_tol(V, want[fin])), (V, name, float(err.max()))
    if V >= 5:
        # -inf and NaN entries score -inf (rows 52..55 hold some of each); all -inf / all NaN rows score NaN
        for b in range(52, 56):
            for kind in (np.isneginf, np.isnan):
                cand = np.nonzero(kind(x[b]))[0]
                if len(cand):
                    tok = np.zeros(64, dtype=np.int64)
                    tok[b] = cand[0]
                    (got,), _ = score([dict(logits=xd, V=V, tok=torch.from_numpy(tok).cuda())], 64)
                    assert float(got[b]) == -math.inf, (V, b)
                    assert math.isnan(float(got[56])) and math.isnan(float(got[58]))


def test_score_reads_a_btv_buffer_in_place_and_strided_tokens():
    V, B = 900, 3
    rng = np.random.default_rng(5)
    full = rng.normal(0.0, 3.0, size=(B, 4, V)).astype(np.float32)
    fd = torch.from_numpy(full).cuda()
    seq = torch.from_numpy(rng.integers(0, V, size=(B, 7))).cuda()
    (got,), rc = score([dict(logits=fd, V=V, tok=seq[:, 4], offset=3 * V, row_stride=4 * V, tok_stride=7)], B)
    assert rc == 0
    (alone,), rc = score([dict(logits=fd[:, 3, :].contiguous(), V=V, tok=seq[:, 4].contiguous())], B)
    assert torch.equal(bits(got), bits(alone))
    want = ref_logprob(full[:, 3, :], seq[:, 4].cpu().numpy())
    assert np.all(np.abs(got.numpy() - want) <= lp_tol(V, want))


def test_score_multi_problem_equals_the_problem_alone():
    """Ten problems (two chunks of the on-chip launch and the re-read launch) of different V in one call."""
    B = 64
    Vs = [900, 13, 8193, 5, 64, 65, 1, 900, 13, 8193]
    probs = []
    for p, V in enumerate(Vs):
        x = make_rows(V)
        rng = np.random.default_rng(p)
        probs.append(dict(logits=torch.from_numpy(x.copy()).cuda(), V=V,
                          tok=torch.from_numpy(rng.integers(0, V, size=B)).cuda()))
    together, rc = score(probs, B)
    assert rc == 0
    again, _ = score(probs, B)
    for p, q in enumerate(probs):
        (alone,), rc = score([q], B)
        assert rc == 0
        assert torch.equal(bits(together[p]), bits(alone)), p
        assert torch.equal(bits(together[p]), bits(again[p])), p


def test_score_token_outside_the_row_is_not_read():
    V, B = 13, 4
    padded = np.full((B, V + 7), np.float32(50.0))
    padded[:, :V] = make_rows(V, B)
    pd = torch.from_numpy(padded).cuda()
    tok = torch.tensor([V, -1, 2 ** 40, 3], dtype=torch.int64).cuda()
    (got,), rc = score([dict(logits=pd, V=V, tok=tok, row_stride=V + 7)], B)
    assert rc == 0
    assert all(math.isnan(float(got[b])) for b in range(3)) and math.isfinite(float(got[3]))


def test_score_rejects_invalid_arguments_before_launching():
    V, B = 13, 3
    xd = torch.zeros(B, V, dtype=torch.float32, device="cuda")
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    good = dict(logits=xd, V=V, tok=tok)
    for bad, status in ((dict(good, V=0), -1), (dict(good, row_stride=V - 1), -1), (dict(good, V=2 ** 20 + 1,
                                                                                         row_stride=2 ** 21), -2)):
        got, rc = score([good, bad], B)
        assert rc == status, bad  # MMT_ERR_INVALID / MMT_ERR_UNSUPPORTED
        assert bool((got[0] == GUARD).all()), "the valid problem ran before the refusal"
    L = ML.lib()
    one = (ctypes.c_int32 * 1)(V)
    assert L.mmt_score_multi(ML.stream_ptr(xd.device), -1, B, one, None, None, None, None, None, None) == -1
    assert L.mmt_score_multi(ML.stream_ptr(xd.device), 1, B, one, None, None, None, None, None, None) == -1
    assert L.mmt_score_multi(ML.stream_ptr(xd.device), 0, B, None, None, None, None, None, None, None) == 0


def test_score_public_wrapper():
    import mmt_sample
    V = 144
    x = make_rows(V)
    xd = torch.from_numpy(x.copy()).cuda()
    tok, lp = mmt_sample.sample(xd, seed=7, pos=3, return_logprobs=True)
    (got,) = mmt_sample.score_multi([xd], [tok])
    assert torch.equal(bits(got.cpu()), bits(lp.cpu()))
    with pytest.raises(ValueError):
        mmt_sample.score_multi([xd], [torch.full((64,), V, dtype=torch.int64, device="cuda")])
