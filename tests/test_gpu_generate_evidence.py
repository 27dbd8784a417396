"""generate(..., given=, evidence="weights" | "resample") on the f_small fixture (d64, L2, T32, V = [57, 13, 24, 5],
cross-attention on modalities 0 and 2): prompt 8, 12 new tokens, modalities 1 and 3 generated, 0 and 2 given. The
given modalities are the two with cross-attention, whose heads see the generated tokens (a head without it sees only
its own, given, history: exactly equal weights). Even so the fixture's heads are nearly flat and respond to the other
modalities by 1e-4 in the score, which never moves a resampling slot; the resampling cases that must move rows run
with the given heads peaked and a series per path (test_resample_replays_on_the_cpu).

"weights" must leave the sequences and the sampled log-probabilities bit-identical, report the rule's scores of the
given tokens on the logits the sampler read (logits_hook; bound `lp_tol` of tests/test_gpu_sample.py) and their
serial fp64 sum exactly.

"resample" is replayed on the CPU from what the hook saw. The hook keeps every step's logits and scores the given
tokens on them with the public mmt_sample.score_multi (the kernel generate runs, hence the device's fp32 values for
every row alive at the time, also for rows that leave no descendant). Ancestors: tests/evidence_ref.py on those
values, under the clear / ambiguous rule of tests/test_gpu_resample.py. Tokens: a returned row's token of step j was
drawn by the row its ancestry leads back to at that time, so it is checked against tests/sampling_ref.py on that
row's logits, keyed by that row. The logits the hook saw after the last resampling point must equal one full forward
over the finished rows at the decode-vs-forward bound FWD_BOUND: they can only if sequences, compact tokens and the
fan-out tails all followed the same ancestors. That this check can fail is shown first, from full forwards alone:
swapping two rows' tokens at the last resampled position moves those logits by more than POWER."""
import numpy as np
import pytest
import torch

import evidence_ref as E
import mmt_sample as MS
import sampling_ref as R
from golden_io import model_fixture
from test_gpu_generate_device import build
from test_gpu_generate_joint import FWD_BOUND, POWER, rel
from test_gpu_resample import delta as rs_delta
from test_gpu_sample import delta, lp_tol
from test_gpu_score import ref_logprob

pytestmark = pytest.mark.gpu

SEED = 0xE71DE2CE
N0, N = 8, 12
GEN, GIVEN = [1, 3], [0, 2]
SETTINGS = {1: (0.9, 0, 1.0), 3: (1.0, 3, 1.0)}


@pytest.fixture(scope="module")
def small():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    m = build(meta, sd)
    m.eval()
    return meta, idx, m


@pytest.fixture(scope="module")
def peaked_given():
    """f_small with the output layers of the given modalities' heads scaled by 60 (as the peaked fixture of
    test_gpu_generate_joint.py): the fixture's heads are nearly flat, so every token scores about -ln V; peaked
    heads give different tokens very different scores."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    for i in GIVEN:
        sd[f"post_block.soft_score_layers.{i}.2.weight"] = sd[f"post_block.soft_score_layers.{i}.2.weight"] * 60.0
    m = build(meta, sd)
    m.eval()
    return meta, idx, m


def inputs(meta, idx, B, n_new=N):
    g = torch.Generator().manual_seed(100 + B)
    start = [t[:B, :N0].cuda() for t in idx]
    given = {i: torch.randint(0, meta["V"][i], (B, n_new), generator=g) for i in GIVEN}
    return start, given


def call(m, start, given, n_new=N, **kw):
    return m.generate(start, max_new_tokens=n_new, modality_to_generate=GEN, given=given,
                      temperature={1: 0.9}, top_k={3: 3}, seed=SEED, return_logprobs=True, **kw)


class Recorder:
    """logits_hook: every modality's logits per position, and the device's scores of the given tokens on them."""

    def __init__(self, given, S, score=True):
        self.given, self.S, self.logits, self.glp, self.score = given, S or 1, {}, {}, score

    def __call__(self, n, views):
        j = n - N0
        self.logits[n] = [v.clone() for v in views]
        if not self.score:  # the caller scores afterwards, once it knows which series each row held
            return
        toks = [self.given[i][:, j].repeat_interleave(self.S).cuda() for i in GIVEN]
        self.glp[j] = [x.cpu().numpy() for x in MS.score_multi([views[i] for i in GIVEN], toks)]


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.mark.parametrize("B,S", [(1, 8), (3, 17), (3, None)])
def test_weights_leave_the_run_alone_and_follow_the_rule(small, B, S):
    meta, idx, m = small
    start, given = inputs(meta, idx, B)
    base_seqs, base_lps = call(m, start, given, num_samples=S)
    rec = Recorder(given, S)
    seqs, lps, ev = call(m, start, given, num_samples=S, evidence="weights", logits_hook=rec)
    torch.cuda.synchronize()
    rows = B * (S or 1)
    assert all(torch.equal(a, b) for a, b in zip(seqs, base_seqs))
    assert all(torch.equal(bits(lps[i]), bits(base_lps[i])) for i in GEN)
    assert sorted(ev["given_logprobs"]) == GIVEN and ev["steps"] == []
    assert tuple(ev["ancestors"].shape) == (0, rows) and tuple(ev["resampled"].shape) == (0, B if S else rows)
    glp = {i: ev["given_logprobs"][i].cpu().numpy() for i in GIVEN}
    for p, i in enumerate(GIVEN):
        assert glp[i].shape == (rows, N) and glp[i].dtype == np.float32
        for j in range(N):
            tok = seqs[i][:, N0 + j].cpu().numpy()
            want = ref_logprob(rec.logits[N0 + j][i].cpu().numpy(), tok)
            err = np.abs(glp[i][:, j] - want)
            assert np.all(err <= lp_tol(meta["V"][i], want)), (i, j, float(err.max()))
            assert np.array_equal(glp[i][:, j].view(np.int32), rec.glp[j][p].view(np.int32))
    want = E.accumulate(np.zeros(rows), [glp[i] for i in GIVEN], 0, N)
    lw = ev["log_weights"].cpu().numpy()
    assert lw.dtype == np.float64 and np.array_equal(lw.view(np.int64), want.view(np.int64))
    le = ev["log_evidence"].cpu().numpy()
    Sp = S or 1
    for b in range(len(le)):
        ref = E.resample_prompt(want[b * Sp:(b + 1) * Sp], 0.0, 0, b, 0)
        assert abs(le[b] - ref["evidence"]) <= rs_delta(Sp) + 8 * 2.0 ** -52 * max(1.0, abs(ref["evidence"]))


def test_weights_one_token_evidence_and_cache_modes(small):
    meta, idx, m = small
    B, S = 3, 8
    start, given = inputs(meta, idx, B, 1)
    seqs, lps, ev = call(m, start, given, n_new=1, num_samples=S, evidence="weights")
    # one token: a prompt's rows read one logits row each, so all weights are equal and the evidence is that weight
    glp = [ev["given_logprobs"][i].cpu().numpy().astype(np.float64) for i in GIVEN]
    le = ev["log_evidence"].cpu().numpy()
    for b in range(B):
        assert all(np.all(g[b * S:(b + 1) * S, 0] == g[b * S, 0]) for g in glp)
        assert le[b] == glp[0][b * S, 0] + glp[1][b * S, 0]
    # use_cache=False (tiled re-forwards) and no num_samples: the same keywords run and return the same shapes
    start, given = inputs(meta, idx, B)
    a_seqs, a_lps, a_ev = call(m, start, given, num_samples=S, evidence="weights", use_cache=False)
    assert m.last_generate_path == "tiled"
    b_seqs, b_lps = call(m, start, given, num_samples=S, use_cache=False)
    assert all(torch.equal(x, y) for x, y in zip(a_seqs, b_seqs))
    assert all(torch.equal(bits(a_lps[i]), bits(b_lps[i])) for i in GEN)
    lw = a_ev["log_weights"].cpu().numpy()
    want = E.accumulate(np.zeros(B * S), [a_ev["given_logprobs"][i].cpu().numpy() for i in GIVEN], 0, N)
    assert np.array_equal(lw.view(np.int64), want.view(np.int64)) and np.all(np.isfinite(lw))
    c_seqs, c_ev = m.generate(start, max_new_tokens=N, modality_to_generate=GEN, given=given, seed=SEED,
                              use_cache=False, evidence="weights")
    assert tuple(c_ev["log_weights"].shape) == (B,) and tuple(c_ev["log_evidence"].shape) == (B,)
    assert torch.equal(bits(c_ev["log_weights"]), bits(c_ev["log_evidence"]))  # one path per prompt


def trace(anc, steps, j, rows):
    """The row that, at the sampling of step j, held what the final rows hold: back through the points at >= j."""
    cur = np.arange(rows)
    for k in range(len(steps) - 1, -1, -1):
        if steps[k] >= j:
            cur = anc[k][cur]
    return cur


@pytest.mark.parametrize("B,S,every,per_row", [(1, 8, 1, False), (3, 17, 1, True), (3, 17, 3, True), (1, 17, 3, True)])
def test_resample_replays_on_the_cpu(small, peaked_given, B, S, every, per_row):
    """per_row: every path follows its own given series ([B * S, N]), on the model whose given heads are peaked. On
    f_small the given heads hardly respond to the other modalities' tokens (the scores of a shared series differ by
    1e-4 between the paths of a prompt, measured) and are nearly flat over their vocabulary, so a shared series, or
    flat heads, leave systematic resampling at the identity and the tails unmoved; series of their own under peaked
    heads give the paths weights that differ and rows that move, which the test requires."""
    meta, idx, m = peaked_given if per_row else small
    start, given = inputs(meta, idx, B)
    rows, M = B * S, len(meta["V"])
    if per_row:
        g = torch.Generator().manual_seed(200 + B + every)
        given = {i: torch.randint(0, meta["V"][i], (rows, N), generator=g) for i in GIVEN}
    given_rows = {i: (given[i] if per_row else given[i].repeat_interleave(S, 0)) for i in GIVEN}
    rec = Recorder(given, S, score=False)
    seqs, lps, ev = call(m, start, given, num_samples=S, evidence="resample", resample_every=every,
                         ess_threshold=2.0, logits_hook=rec)
    torch.cuda.synchronize()
    assert m.last_generate_path == "fanout"
    steps = ev["steps"]
    assert steps == [j for j in range(N - 1) if (j + 1) % every == 0]
    anc, res = ev["ancestors"].cpu().numpy(), ev["resampled"].cpu().numpy()
    assert anc.shape == (len(steps), rows) and res.shape == (len(steps), B)
    # the device's scores of the rows alive at each step: the given tokens a row holds at step j are those of the row
    # its ancestry so far leads back to (a path carries its whole series along)
    perm = np.arange(rows)
    for j in range(N):
        toks = [given_rows[i][torch.from_numpy(perm), j].cuda() for i in GIVEN]
        rec.glp[j] = [x.cpu().numpy() for x in MS.score_multi([rec.logits[N0 + j][i] for i in GIVEN], toks)]
        if j in steps:
            perm = perm[anc[steps.index(j)]]
    for i in GIVEN:  # the given series are forced, each path's own
        assert torch.equal(seqs[i][:, N0:].cpu(), given_rows[i][torch.from_numpy(perm)])

    # ancestors, weights and evidence: evidence_ref on the device's scores of the rows alive at each point
    logw, last, le_ref, le_tol, amb_total = np.zeros(rows), 0, np.zeros(B), np.zeros(B), 0
    for k, j in enumerate(steps):
        cols = {c: rec.glp[c] for c in range(last, j + 1)}
        a = logw.copy()
        for c in range(last, j + 1):
            for p in range(len(GIVEN)):
                a = a + cols[c][p].astype(np.float64)
        for b in range(B):
            ref = E.resample_prompt(a[b * S:(b + 1) * S], 2.0, SEED, b, N0 + j)
            assert ref["trigger"] and res[k, b] == 1
            loc = anc[k, b * S:(b + 1) * S] - b * S
            assert loc.min() >= 0 and loc.max() < S
            amb, bad = E.check_ancestors(ref, loc, rs_delta(S))
            assert not bad, (k, j, b, bad, loc, ref["ancestor"], ref["neighbor"])
            amb_total += amb
            le_ref[b] += ref["evidence"]
            le_tol[b] += rs_delta(S) + 8 * 2.0 ** -52 * max(1.0, abs(ref["evidence"]), abs(a[b * S:(b + 1) * S].max()))
        logw, last = np.zeros(rows), j + 1
    assert amb_total <= 0.05 * rows * max(1, len(steps)), amb_total
    want = logw.copy()
    for c in range(last, N):
        for p in range(len(GIVEN)):
            want = want + rec.glp[c][p].astype(np.float64)
    lw = ev["log_weights"].cpu().numpy()
    assert np.array_equal(lw.view(np.int64), want.view(np.int64))
    le = ev["log_evidence"].cpu().numpy()
    for b in range(B):
        ref = E.resample_prompt(want[b * S:(b + 1) * S], 0.0, 0, b, 0)
        tol = le_tol[b] + rs_delta(S) + 8 * 2.0 ** -52 * max(1.0, abs(ref["evidence"]))
        assert abs(le[b] - (le_ref[b] + ref["evidence"])) <= tol, (b, le[b], le_ref[b] + ref["evidence"])

    # tokens, their log-probabilities and the given scores: by the row that drew them
    amb_tok = 0
    for j in range(N):
        n, q = N0 + j, trace(anc, steps, j, rows)
        for p, i in enumerate(GIVEN):
            got = ev["given_logprobs"][i][:, j].cpu().numpy()
            assert np.array_equal(got.view(np.int32), rec.glp[j][p][q].view(np.int32)), (i, j)
        for i, (t, k, pp) in SETTINGS.items():
            V = meta["V"][i]
            ref = R.sample_rows(rec.logits[n][i].cpu().numpy(), t, k, pp, MS.modality_seed(SEED, i), n, 0)
            tok = seqs[i][:, n].cpu().numpy()
            clear = ((ref["margin_u"] >= delta(V)) & (ref["margin_p"] >= delta(V)))[q]
            ok = (tok == ref["token"][q]) | (~clear & (tok == ref["neighbor"][q]))
            assert ok.all(), (i, j, np.nonzero(~ok)[0], tok, ref["token"][q])
            amb_tok += int((~clear).sum())
            err = np.abs(lps[i][:, j].cpu().numpy().astype(np.float64) - ref["logprob"][q])[clear]
            assert np.all(err <= lp_tol(V, ref["logprob"][q][clear])), (i, j)
    assert amb_tok <= 0.05 * rows * N * len(SETTINGS), amb_tok

    # the check below can fail: from full forwards alone, two rows' tokens swapped at the last resampled position
    # move the logits there by more than POWER
    n_last = N0 + steps[-1]
    with torch.no_grad():
        full, _ = m(seqs)
    for i in GEN:
        col = seqs[i][:, n_last]
        assert bool((col != col[0]).any()), "every row holds one token there"
        r1 = int((col != col[0]).nonzero()[0])
        other = [s.clone() for s in seqs]
        other[i][0, n_last], other[i][r1, n_last] = seqs[i][r1, n_last], seqs[i][0, n_last]
        with torch.no_grad():
            moved, _ = m(other)
        e = rel(moved[i][[0, r1], n_last], full[i][[0, r1], n_last])
        print(f"power: modality {i} rows 0/{r1} swapped at position {n_last}: rel-L2 {e:.2f}")
        assert e > POWER, (i, e)
    # the logits the hook saw after the last point against the full forward over the finished rows
    worst = 0.0
    for n in range(n_last + 1, N0 + N):
        for i in range(M):
            e = rel(rec.logits[n][i], full[i][:, n - 1])
            worst = max(worst, e)
            assert e < FWD_BOUND, (i, n, e)
    print(f"B={B} S={S} every={every}: hook logits after the last point vs full forward: worst rel-L2 {worst:.2e}; "
          f"ambiguous slots {amb_total}, ambiguous draws {amb_tok}")
    moved = sum(int((anc[k] != np.arange(rows)).sum()) for k in range(len(steps)))
    print(f"rows that changed their ancestor, over all points: {moved}")
    if per_row:
        assert moved > 0, "no point moved a row: the run exercised no gather"


def test_threshold_zero_is_the_weights_run_and_refusals(small):
    meta, idx, m = small
    B, S = 3, 8
    start, given = inputs(meta, idx, B)
    w_seqs, w_lps, w = call(m, start, given, num_samples=S, evidence="weights")
    r_seqs, r_lps, r = call(m, start, given, num_samples=S, evidence="resample", resample_every=3, ess_threshold=0)
    assert r["steps"] == [2, 5, 8]
    assert torch.equal(r["ancestors"].cpu(), torch.arange(B * S, dtype=torch.int32).expand(3, B * S))
    assert not bool(r["resampled"].any())
    assert all(torch.equal(a, b) for a, b in zip(w_seqs, r_seqs))
    assert all(torch.equal(bits(w_lps[i]), bits(r_lps[i])) for i in GEN)
    assert all(torch.equal(bits(w["given_logprobs"][i]), bits(r["given_logprobs"][i])) for i in GIVEN)
    assert torch.equal(bits(w["log_weights"]), bits(r["log_weights"]))
    assert torch.equal(bits(w["log_evidence"]), bits(r["log_evidence"]))
    twice = call(m, start, given, num_samples=S, evidence="resample", ess_threshold=2.0)
    again = call(m, start, given, num_samples=S, evidence="resample", ess_threshold=2.0)
    assert all(torch.equal(a, b) for a, b in zip(twice[0], again[0]))
    assert torch.equal(twice[2]["ancestors"], again[2]["ancestors"])
    assert torch.equal(bits(twice[2]["log_evidence"]), bits(again[2]["log_evidence"]))
    with pytest.raises(ValueError):
        call(m, start, given, evidence="resample")  # without num_samples
    T = meta["block_size"]
    long_given = {i: torch.zeros(B, T - N0 + 1, dtype=torch.long) for i in GIVEN}
    with pytest.raises(ValueError):
        call(m, start, long_given, n_new=T - N0 + 1, num_samples=S, evidence="resample")  # past the block
    with pytest.raises(ValueError):
        call(m, start, given, num_samples=S, evidence="resample", use_cache=False)
    with pytest.raises(ValueError):
        m.generate(start, max_new_tokens=N, modality_to_generate=GEN, evidence="weights")  # no given modality
