"""mmt_resample (csrc/mmt_evidence.hip) against the numpy restatement of its rule (tests/evidence_ref.py).

Ancestors are compared under the sampler tests' clear / ambiguous rule: a slot whose target (s + u) / S * W is at
least delta * W away from the nearest prefix boundary must take the reference's row; a closer slot may take that row
or the live neighbour across the boundary. At most 5 % of a case's slots may be ambiguous (the restatement alone
leaves at most 1.8 % at S = 4096; tests/test_evidence_ref_cpu.py checks the cap on the CPU for the same inputs).

delta, from the kernel's tree, which is the sampler's with S for V: thread t owns c = ceil(S / 256) | 1 consecutive
weights; the prefix a slot compares with is the thread's serial total (c additions), a 6-step shift scan, the wave
totals left to right (3), wave base + lane offset (1) and the serial walk over the chunk (c); W is the same tree
without the walk: 2 c + 10 and c + 9 roundings of 2^-53 relative to a partial sum of at most W. The target costs
two more fp64 roundings than the sampler's u * S (an addition, a division, a multiplication). A weight e_s = expf(d_s)
carries expf's error (3 ulp of 2^-23 taken, as in test_gpu_sample.py) and the rounding of d_s = (float)(a_s - mx),
2^-24 |d_s| relative, which summed with the weights e_s / W is at most 2^-24 ln S. Hence

    delta(S) = test_gpu_sample.delta(S) + 2 * 2^-53

log_evidence: mx is exact (a maximum of sums the restatement forms in the same order), W is off by at most delta
relative, which the logarithm turns into delta absolute; the fp64 division, logarithm and two additions are taken
as 8 ulp of the result's magnitude: |got - ref| <= delta(S) + 8 * 2^-52 * max(1, |ref|, |mx|)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import evidence_ref as E
import mmt_lib as ML
from test_gpu_sample import delta as sample_delta

pytestmark = pytest.mark.gpu

SEED0 = 0x0E51DE0CE0000000


def delta(S):
    return sample_delta(S) + 2 * 2.0 ** -53


def launch(logw, S, thr, seed, pos=E.POS, lps=(), j0=0, j1=0, log_evidence=None):
    """One mmt_resample over logw (numpy fp64 [B * S]). Returns a dict of CPU arrays and the status; every output
    buffer is preset, so a refusal that wrote nothing leaves the presets."""
    R = len(logw)
    B = R // S
    lw = torch.from_numpy(np.array(logw, dtype=np.float64)).cuda()
    ev = torch.from_numpy(np.array(log_evidence if log_evidence is not None else np.zeros(B), dtype=np.float64)).cuda()
    anc = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    res = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    G = len(lps)
    dl = [torch.from_numpy(np.ascontiguousarray(lp)).cuda() for lp in lps]
    pl = (ctypes.c_void_p * max(G, 1))(*[t.data_ptr() for t in dl])
    st = (ctypes.c_int64 * max(G, 1))(*[t.shape[1] for t in dl])
    rc = ML.lib().mmt_resample(ML.stream_ptr(lw.device), B, S, G, pl, st, j0, j1, lw.data_ptr(), ev.data_ptr(),
                               float(thr), seed, pos, anc.data_ptr(), res.data_ptr())
    torch.cuda.synchronize()
    return dict(logw=lw.cpu().numpy(), ev=ev.cpu().numpy(), anc=anc.cpu().numpy(), res=res.cpu().numpy()), rc


def check_prompt(S, a, b, out, thr, seed, ev0=0.0):
    """Prompt b of a launch against the restatement; returns the number of ambiguous slots."""
    ref = E.resample_prompt(a, thr, seed, b, E.POS)
    loc = out["anc"][b * S:(b + 1) * S] - b * S
    lw = out["logw"][b * S:(b + 1) * S]
    assert int(out["res"][b]) == int(ref["trigger"]), (S, b, thr, ref["ess"] / S)
    if not ref["trigger"]:
        assert np.array_equal(loc, np.arange(S))
        assert np.array_equal(lw.view(np.int64), np.asarray(a, dtype=np.float64).view(np.int64)), "logw not carried"
        assert out["ev"][b] == ev0
        return 0
    assert loc.min() >= 0 and loc.max() < S
    d = delta(S)
    amb, bad = E.check_ancestors(ref, loc, d)
    assert not bad, (S, b, bad[:5], loc[bad[:5]], ref["ancestor"][bad[:5]], ref["neighbor"][bad[:5]])
    assert amb <= 0.05 * S, (S, b, amb)
    assert np.all(ref["e"][loc] > 0), "a dead path is an ancestor"
    want = S * ref["e"] / ref["W"]
    got = np.bincount(loc, minlength=S)
    assert np.all(got >= np.floor(want - 1e-9) - amb) and np.all(got <= np.ceil(want + 1e-9) + amb), (S, b)
    assert np.all(lw == 0.0)
    tol = d + 8 * 2.0 ** -52 * max(1.0, abs(ref["evidence"]), abs(float(np.max(a))))
    assert abs(out["ev"][b] - (ev0 + ref["evidence"])) <= tol, (S, b, out["ev"][b], ref["evidence"])
    return amb


@pytest.mark.parametrize("S", E.SAMPLES)
def test_resample_families(S):
    """Three prompts of different weights per launch, N(0, sigma^2) log-weights, always-on and 0.6 thresholds."""
    worst = 0
    for sigma in E.SIGMAS:
        for seed in E.SEEDS:
            a = E.family(S, sigma, seed)
            for thr in E.THRESHOLDS:
                out, rc = launch(a.reshape(-1), S, thr, seed)  # the seeds the CPU test vetted the families with
                assert rc == 0
                for b in range(3):
                    worst = max(worst, check_prompt(S, a[b], b, out, thr, seed))
            if sigma == 0.0:  # equal weights: the identity, exactly
                out, _ = launch(a.reshape(-1), S, 2.0, seed)
                assert np.array_equal(out["anc"], np.arange(3 * S)) and np.all(out["res"] == 1)
    print(f"S={S}: most ambiguous slots in a prompt {worst} (delta {delta(S):.2e})")


def test_resample_dead_paths_and_dead_prompts():
    S = 257
    a = E.family(S, 2.0, 3)
    a[0, ::3] = -np.inf
    a[1, :] = -np.inf  # no live path
    a[2, :] = -np.inf
    a[2, 100] = -4.0  # one live path
    out, rc = launch(a.reshape(-1), S, 2.0, SEED0, log_evidence=[1.0, 2.0, 3.0])
    assert rc == 0
    check_prompt(S, a[0], 0, out, 2.0, SEED0, ev0=1.0)
    assert np.array_equal(out["anc"][S:2 * S], np.arange(S, 2 * S)) and out["res"][1] == 0 and out["ev"][1] == 2.0
    assert np.all(np.isneginf(out["logw"][S:2 * S]))
    assert np.all(out["anc"][2 * S:] == 2 * S + 100) and out["res"][2] == 1
    assert out["ev"][2] == pytest.approx(3.0 - 4.0 - math.log(S), abs=1e-12)


def test_resample_accumulates_columns_serially():
    """Threshold 0 only folds the columns [j0, j1) of the given matrices into logw: exactly the restated serial fp64
    sum, NaN terms as -inf; the closing fold (a negative threshold) adds mx + log(W / S) to log_evidence."""
    S, B, N = 17, 3, 5
    rng = np.random.default_rng(9)
    lps = [-np.abs(rng.normal(0.0, 2.0, size=(B * S, N))).astype(np.float32) for _ in range(3)]
    lps[1][5, 2] = np.nan
    lps[2][7, 1] = -np.inf
    lw0 = rng.normal(0.0, 1.0, size=B * S)
    for (j0, j1) in ((0, N), (1, 3), (2, 2)):
        want = E.accumulate(lw0, lps, j0, j1)
        out, rc = launch(lw0, S, 0.0, SEED0, lps=lps, j0=j0, j1=j1)
        assert rc == 0
        assert np.array_equal(out["logw"].view(np.int64), want.view(np.int64)), (j0, j1)
        assert np.array_equal(out["anc"], np.arange(B * S)) and np.all(out["res"] == 0) and np.all(out["ev"] == 0.0)
        fold, rc = launch(lw0, S, -1.0, SEED0, lps=lps, j0=j0, j1=j1)
        assert rc == 0
        assert np.array_equal(fold["logw"].view(np.int64), want.view(np.int64))
        assert np.array_equal(fold["anc"], np.arange(B * S)) and np.all(fold["res"] == 0)
        for b in range(B):
            ref = E.resample_prompt(want[b * S:(b + 1) * S], 0.0, 0, b, 0)
            assert abs(fold["ev"][b] - ref["evidence"]) <= delta(S) + 8 * 2.0 ** -52 * max(1.0, abs(ref["evidence"]))
    # the resampling draws on the accumulated weights
    want = E.accumulate(lw0, lps, 0, N)
    out, rc = launch(lw0, S, 2.0, SEED0, lps=lps, j0=0, j1=N)
    assert rc == 0
    for b in range(B):
        check_prompt(S, want[b * S:(b + 1) * S], b, out, 2.0, SEED0)


def test_resample_is_deterministic_and_prompt_independent():
    for S in (17, 1000, 4096):
        a = E.family(S, 2.0, 1)
        x, _ = launch(a.reshape(-1), S, 2.0, SEED0 + 1)
        y, _ = launch(a.reshape(-1), S, 2.0, SEED0 + 1)
        for k in ("logw", "ev", "anc", "res"):
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), (S, k)
        alone, _ = launch(a[0], S, 2.0, SEED0 + 1)
        other = np.concatenate([a[0], E.family(S, 8.0, 5)[2], a[1], a[2]])
        comp, _ = launch(other, S, 2.0, SEED0 + 1)
        for o in (alone, comp):
            assert np.array_equal(o["anc"][:S], x["anc"][:S]) and o["ev"][0].tobytes() == x["ev"][0].tobytes(), S
        moved, _ = launch(a.reshape(-1), S, 2.0, SEED0 + 1, pos=E.POS + 1)
        assert not np.array_equal(moved["anc"], x["anc"])  # another position draws anew


def test_resample_rejects_invalid_arguments_before_launching():
    S = 16
    a = E.family(S, 2.0, 0).reshape(-1)
    lp = [np.zeros((3 * S, 4), dtype=np.float32)]
    for kw, status in ((dict(thr=float("nan")), -1), (dict(j0=3, j1=2, lps=lp), -1), (dict(j0=0, j1=5, lps=lp), -1),
                       (dict(j0=-1, j1=1, lps=lp), -1)):
        kw = dict(dict(thr=2.0), **kw)
        out, rc = launch(a, S, kw.pop("thr"), SEED0, **kw)
        assert rc == status, kw
        assert np.all(out["anc"] == -7) and np.all(out["res"] == -7) and np.array_equal(out["logw"], a)
    big = np.zeros(4097)
    out, rc = launch(big, 4097, 2.0, SEED0)
    assert rc == -2 and np.all(out["anc"] == -7)  # MMT_ERR_UNSUPPORTED above the on-chip fan
    L = ML.lib()
    assert L.mmt_resample(None, 1, 0, 0, None, None, 0, 0, None, None, 0.5, 1, 0, None, None) == -1
    assert L.mmt_resample(None, 1, 4, 0, None, None, 0, 0, None, None, 0.5, 1, 0, None, None) == -1
    assert L.mmt_resample(None, 0, 4, 0, None, None, 0, 0, None, None, 0.5, 1, 0, None, None) == 0


def test_resample_public_wrapper():
    import mmt_sample
    S, B, N = 64, 2, 3
    rng = np.random.default_rng(4)
    lps = [-np.abs(rng.normal(0.0, 2.0, size=(B * S, N))).astype(np.float32) for _ in range(2)]
    want = E.accumulate(np.zeros(B * S), lps, 0, 2)
    logw = torch.zeros(B * S, dtype=torch.float64, device="cuda")
    ev = torch.zeros(B, dtype=torch.float64, device="cuda")
    anc, res = mmt_sample.resample([torch.from_numpy(x).cuda() for x in lps], logw, ev, samples=S, ess_threshold=2.0,
                                   seed=SEED0, pos=E.POS, j0=0, j1=2)
    out = dict(anc=anc.cpu().numpy(), res=res.cpu().numpy(), logw=logw.cpu().numpy(), ev=ev.cpu().numpy())
    for b in range(B):
        check_prompt(S, want[b * S:(b + 1) * S], b, out, 2.0, SEED0)
    with pytest.raises(ValueError):
        mmt_sample.resample([], logw, ev, samples=5, ess_threshold=0.5, seed=1, pos=0)
