"""Joint rollouts of generate (mmt_rollout.py `rollout`: a list of modalities or "all", `given=`), on the f_small
fixture (d64, L2, T32, B4, V = [57, 13, 24, 5], cross-attention on modalities 0 and 2).

The keying rule is checked as in tests/test_gpu_generate_device.py: the tokens and log-probabilities of modality i
against the CPU restatement of the rule (tests/sampling_ref.py) with the seed modality_seed(seed, i), on exactly the
logits the sampler read (logits_hook), under the clear / ambiguous rule and the bounds of tests/test_gpu_sample.py.

The feedback wiring (which buffer the next step reads for which modality) is checked against one full forward over
the finished sequences: the logits the hook saw before position n must be the full forward's logits at position
n - 1, at the project's decode-vs-forward bound of rel-L2 1e-2 (test_kv_cache_decode_matches_full_forward). The test
first shows, from full forwards alone, that another token of modality i at a position moves that modality's logits
there by more than 1e-1, so a compact buffer wired to the wrong modality, or read one step late, cannot pass."""
import numpy as np
import pytest
import torch

import mmt_sample as MS
import sampling_ref as R
from golden_io import model_fixture
from test_gpu_generate_device import build
from test_gpu_sample import delta, lp_tol

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234
FWD_BOUND = 1e-2  # decode step vs full forward, rel-L2
POWER = 1e-1  # what one other token must move


@pytest.fixture(scope="module")
def small():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    return meta, idx, build(meta, sd)


@pytest.fixture(scope="module")
def peaked():
    """f_small with peaked output heads (argmax stable to bf16 noise), as test_generate_kv_cache_greedy_matches_reforward."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    for k in list(sd):
        if k.startswith("post_block.soft_score_layers.") and k.endswith(".2.weight"):
            sd[k] = sd[k] * 60.0
    return meta, idx, build(meta, sd)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


class Recorder:
    """logits_hook of the list form: keeps a copy of every modality's [rows, V_i] view per position."""

    def __init__(self, meta, rows):
        self.V, self.rows, self.seen = meta["V"], rows, {}

    def __call__(self, n, logits_list):
        assert len(logits_list) == len(self.V)
        for lg, V in zip(logits_list, self.V):
            assert tuple(lg.shape) == (self.rows, V) and lg.dtype == torch.float32
        assert n not in self.seen
        self.seen[n] = [lg.clone() for lg in logits_list]


def check_rule(meta, rec, seqs, lps, settings, seed, n0, N):
    """Every generated modality's tokens and log-probabilities against the rule on the recorded logits."""
    torch.cuda.synchronize()
    assert sorted(rec.seen) == list(range(n0, n0 + N))
    assert sorted(lps) == sorted(settings)
    for i, (t, k, p) in settings.items():
        V, d = meta["V"][i], delta(meta["V"][i])
        out, lp = seqs[i].cpu().numpy(), lps[i].cpu().numpy().astype(np.float64)
        assert lp.shape == (rec.rows, N) and lps[i].dtype == torch.float32
        amb_total = 0
        for j in range(N):
            n = n0 + j
            ref = R.sample_rows(rec.seen[n][i].cpu().numpy(), t, k, p, MS.modality_seed(seed, i), n, 0)
            amb, bad = R.check_tokens(ref, out[:, n], d)
            assert not bad, (i, n, bad, out[:, n], ref["token"], ref["neighbor"])
            amb_total += amb
            clear = (ref["margin_u"] >= d) & (ref["margin_p"] >= d)
            err = np.abs(lp[:, j] - ref["logprob"])[clear]
            assert np.all(err <= lp_tol(V, ref["logprob"][clear])), (i, n, err)
        print(f"modality {i}: ambiguous rows {amb_total}/{rec.rows * N}")
        assert amb_total <= 0.05 * rec.rows * N, (i, amb_total)


def check_against_full_forward(m, rec, seqs, n0, N, modalities):
    """The recorded logits before position n against the full forward's at position n - 1 (seqs are block_size long)."""
    with torch.no_grad():
        full, _ = m(seqs)
    worst = 0.0
    for i in modalities:
        for n in range(n0, n0 + N):
            e = rel(rec.seen[n][i], full[i][:, n - 1])
            worst = max(worst, e)
            assert e < FWD_BOUND, (i, n, e)
    print(f"hook logits vs full forward: worst rel-L2 {worst:.2e}")
    return full


def show_power(m, meta, seqs, full, modalities, positions=(6, 20)):
    """From full forwards alone: another token of modality i at position p moves full[i][:, p] by more than POWER."""
    for i in modalities:
        for p in positions:
            other = [s.clone() for s in seqs]
            other[i][:, p] = (other[i][:, p] + 1) % meta["V"][i]
            with torch.no_grad():
                moved, _ = m(other)
            e = rel(moved[i][:, p], full[i][:, p])
            print(f"power: modality {i} position {p}: rel-L2 {e:.2f}")
            assert e > POWER, (i, p, e)


def test_joint_reproduces_the_rule_on_its_own_logits(small):
    """[0, 2, 3] with per-modality settings, prompt 5, T + 3 - 5 new tokens: the prefill's logits read in place, decode
    steps, and three re-forwards past block_size. Modality 1 is held."""
    meta, idx, m = small
    T, B = meta["block_size"], idx[0].shape[0]
    start = [t[:, :5].cuda() for t in idx]
    N = T + 3 - 5
    rec = Recorder(meta, B)
    seqs, lps = m.generate(start, max_new_tokens=N, modality_to_generate=[0, 2, 3], temperature={0: 0.8, 2: 1.1},
                           top_k={0: 5, 2: 6}, top_p={0: 0.9, 3: 0.8}, seed=SEED, return_logprobs=True,
                           logits_hook=rec)
    settings = {0: (0.8, 5, 0.9), 2: (1.1, 6, 1.0), 3: (1.0, 0, 0.8)}
    check_rule(meta, rec, seqs, lps, settings, SEED, 5, N)
    for i, s in enumerate(seqs):
        assert tuple(s.shape) == (B, T + 3) and s.dtype == start[i].dtype and torch.equal(s[:, :5], start[i]), i
    assert torch.equal(seqs[1][:, 5:], start[1][:, -1:].expand(B, N))
    for i in (0, 2, 3):
        assert int(seqs[i][:, 5:].min()) >= 0 and int(seqs[i][:, 5:].max()) < meta["V"][i]
    # a list of one is the list form: keyed by modality_seed, not by the int form's seed
    one, lp1 = m.generate(start, max_new_tokens=4, modality_to_generate=[2], temperature=1.1, top_k=6, seed=SEED,
                          return_logprobs=True)
    assert torch.equal(one[2][:, 5], seqs[2][:, 5]) and sorted(lp1) == [2]  # the first draw: the same logits and key


def test_joint_feedback_wiring_against_a_full_forward(small):
    meta, idx, m = small
    T, B, M = meta["block_size"], idx[0].shape[0], len(meta["V"])
    start = [t[:, :5].cuda() for t in idx]
    rec = Recorder(meta, B)
    seqs = m.generate(start, max_new_tokens=T - 5, modality_to_generate="all", temperature=1.0, seed=7, logits_hook=rec)
    assert isinstance(seqs, list) and all(tuple(s.shape) == (B, T) for s in seqs)
    full = check_against_full_forward(m, rec, seqs, 5, T - 5, range(M))
    show_power(m, meta, seqs, full, range(M))
    for i in range(M):  # every modality moved: none is held
        assert not torch.equal(seqs[i][:, 5:], start[i][:, -1:].expand(B, T - 5)), i


def test_joint_given_inputs(small):
    meta, idx, m = small
    T, B = meta["block_size"], idx[0].shape[0]
    start = [t[:, :5].cuda() for t in idx]
    N = T - 5
    g = torch.Generator().manual_seed(3)
    path = torch.randint(0, meta["V"][1], (B, N), generator=g)
    rec = Recorder(meta, B)
    seqs, lps = m.generate(start, max_new_tokens=N, modality_to_generate=[0, 2], given={1: path}, temperature=0.9,
                           seed=SEED, return_logprobs=True, logits_hook=rec)
    assert torch.equal(seqs[1][:, 5:].cpu(), path)  # verbatim
    assert torch.equal(seqs[3][:, 5:], start[3][:, -1:].expand(B, N))  # the held pad
    assert all(torch.equal(s[:, :5], start[i]) for i, s in enumerate(seqs))
    check_rule(meta, rec, seqs, lps, {0: (0.9, 0, 1.0), 2: (0.9, 0, 1.0)}, SEED, 5, N)
    full = check_against_full_forward(m, rec, seqs, 5, N, range(4))
    show_power(m, meta, seqs, full, [1])  # modality 1's logits do depend on the given token of the position
    # a given on the device, and another path: modality 1 follows it
    seqs2 = m.generate(start, max_new_tokens=N, modality_to_generate=[0, 2], given={1: ((path + 1) % 13).cuda()},
                       temperature=0.9, seed=SEED)
    assert torch.equal(seqs2[1][:, 5:].cpu(), (path + 1) % 13)


def test_joint_same_call_twice_is_bit_equal(small):
    meta, idx, m = small
    start = [t[:, :7].cuda() for t in idx]
    kw = dict(max_new_tokens=12, modality_to_generate="all", temperature=1.1, top_k={0: 6}, seed=99,
              return_logprobs=True)
    a, la = m.generate(start, **kw)
    b, lb = m.generate(start, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert sorted(la) == [0, 1, 2, 3]
    assert all(torch.equal(la[i].view(torch.int32), lb[i].view(torch.int32)) for i in la)
    c, _ = m.generate(start, **dict(kw, seed=100))
    assert not all(torch.equal(x, y) for x, y in zip(a, c))


def test_joint_greedy_cache_modes_and_the_int_form(peaked):
    meta, idx, m = peaked
    T, B, M = meta["block_size"], idx[0].shape[0], len(meta["V"])
    start = [t[:, :5].cuda() for t in idx]
    N = T + 3 - 5
    a = m.generate(start, max_new_tokens=N, modality_to_generate="all", use_cache=True, temperature=0)
    b = m.generate(start, max_new_tokens=N, modality_to_generate="all", use_cache=False, temperature=0)
    for i in range(M):
        assert tuple(a[i].shape) == (B, T + 3)
        assert torch.equal(a[i], b[i]), i
    for i in range(M):  # each modality's first step: what the int form's argmax path gives for it
        old = m.generate(start, max_new_tokens=1, modality_to_generate=i,
                         sample_fn=lambda probs: probs.argmax(dim=-1, keepdim=True))
        assert torch.equal(old[i][:, 5], a[i][:, 5]), i


@pytest.mark.parametrize("mode", ["cached", "cached_one_row", "reforward", "fanout", "tiled"])
def test_int_form_is_a_list_of_one_under_the_seed_relation(small, mode):
    """generate(modality_to_generate=g, seed=modality_seed(SEED, g)) and generate(modality_to_generate=[g], seed=SEED)
    are the same rollout: every returned sequence equal, the log-probabilities equal as bit patterns. cached crosses
    block_size (the prefill, decode steps and three re-forwards); one row takes the other row-stride branch."""
    meta, idx, m = small
    T, g = meta["block_size"], 2
    B = {"cached_one_row": 1, "fanout": 2, "tiled": 2}.get(mode, idx[0].shape[0])
    start = [t[:B, :5].cuda() for t in idx]
    kw = dict(temperature=0.9, top_k=6, top_p=0.9, return_logprobs=True)
    if mode in ("cached", "cached_one_row"):
        kw.update(max_new_tokens=T + 3 - 5)
    elif mode == "reforward":
        kw.update(max_new_tokens=6, use_cache=False)
    else:
        kw.update(max_new_tokens=9, num_samples=3, use_cache=mode == "fanout")
    m.last_generate_path = None
    seqs, lp = m.generate(start, modality_to_generate=g, seed=MS.modality_seed(SEED, g), **kw)
    path = m.last_generate_path
    m.last_generate_path = None
    seqs1, lps = m.generate(start, modality_to_generate=[g], seed=SEED, **kw)
    assert path == m.last_generate_path == (mode if mode in ("fanout", "tiled") else None)
    rows = B * kw.get("num_samples", 1)
    assert len(seqs) == len(seqs1) == len(meta["V"]) and sorted(lps) == [g]
    for a, b in zip(seqs, seqs1):
        assert tuple(a.shape) == (rows, 5 + kw["max_new_tokens"]) and torch.equal(a, b)
    assert tuple(lp.shape) == (rows, kw["max_new_tokens"]) and lp.dtype == torch.float32
    assert torch.equal(lp.view(torch.int32), lps[g].view(torch.int32))


def test_joint_fanout(small, peaked):
    meta, idx, m = small
    T, B, S = meta["block_size"], 2, 3
    start = [t[:B, :5].cuda() for t in idx]
    N = 9
    g = torch.Generator().manual_seed(4)
    path = torch.randint(0, meta["V"][3], (B, N), generator=g)
    rec = Recorder(meta, B * S)
    kw = dict(modality_to_generate=[0, 1], temperature={0: 0.9}, top_k={1: 4}, seed=SEED, return_logprobs=True)
    seqs, lps = m.generate(start, max_new_tokens=N, given={3: path}, num_samples=S, logits_hook=rec, **kw)
    assert m.last_generate_path == "fanout"
    assert all(tuple(s.shape) == (B * S, 5 + N) for s in seqs)
    assert torch.equal(seqs[3][:, 5:].cpu(), path.repeat_interleave(S, 0))  # shared by a prompt's samples
    assert torch.equal(seqs[2][:, 5:], seqs[2][:, 4:5].expand(B * S, N))
    assert all(torch.equal(s[:, :5], start[i].repeat_interleave(S, 0)) for i, s in enumerate(seqs))
    check_rule(meta, rec, seqs, lps, {0: (0.9, 0, 1.0), 1: (1.0, 4, 1.0)}, SEED, 5, N)
    assert not torch.equal(seqs[0][0], seqs[0][1])  # the samples of a prompt draw apart
    # a [B * S, N] given: one path per sample
    per = torch.randint(0, meta["V"][3], (B * S, N), generator=g)
    s2 = m.generate(start, max_new_tokens=N, given={3: per}, num_samples=S, modality_to_generate=[0, 1], seed=SEED)
    assert m.last_generate_path == "fanout" and torch.equal(s2[3][:, 5:].cpu(), per)
    # past block_size: tiled, and the rule still holds
    N2 = T + 2 - 5
    path2 = torch.randint(0, meta["V"][3], (B, N2), generator=g)
    rec2 = Recorder(meta, B * S)
    seqs, lps = m.generate(start, max_new_tokens=N2, given={3: path2}, num_samples=S, logits_hook=rec2, **kw)
    assert m.last_generate_path == "tiled"
    assert torch.equal(seqs[3][:, 5:].cpu(), path2.repeat_interleave(S, 0))
    check_rule(meta, rec2, seqs, lps, {0: (0.9, 0, 1.0), 1: (1.0, 4, 1.0)}, SEED, 5, N2)
    # peaked greedy: the fan-out equals the tiled call exactly
    meta, idx, mp = peaked
    N3 = T - 5
    path3 = torch.randint(0, meta["V"][3], (B, N3), generator=g)
    gk = dict(max_new_tokens=N3, modality_to_generate=[0, 1, 2], temperature=0)
    fan = mp.generate(start, given={3: path3}, num_samples=S, **gk)
    assert mp.last_generate_path == "fanout"
    tiled = mp.generate(start, given={3: path3}, num_samples=S, use_cache=False, **gk)
    assert mp.last_generate_path == "tiled"
    by_hand = mp.generate([p.repeat_interleave(S, 0) for p in start], given={3: path3.repeat_interleave(S, 0)}, **gk)
    for i in range(4):
        assert torch.equal(fan[i], tiled[i]) and torch.equal(fan[i], by_hand[i]), i
        assert torch.equal(fan[i][0::S].repeat_interleave(S, 0), fan[i]), i  # greedy samples of a prompt coincide


def test_joint_refusals_come_before_any_launch(small, monkeypatch):
    meta, idx, m = small
    B, N = idx[0].shape[0], 4
    start = [t[:, :6].cuda() for t in idx]
    ok = torch.zeros(B, N, dtype=torch.long)

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the forward")

    monkeypatch.setattr(m, "_launch_forward", no_launch)
    bad = [
        dict(modality_to_generate=[0, 1], given={1: ok}),  # generated and given
        dict(modality_to_generate=[0], given={1: ok[:, :-1]}),
        dict(modality_to_generate=[0], given={1: ok[:-1]}),
        dict(modality_to_generate=[0], given={1: ok.int()}),
        dict(modality_to_generate=[0], given={1: torch.full((B, N), 13).cuda()}),  # V_1 = 13
        dict(modality_to_generate=[0], given={3: torch.full((B, N), -1)}),
        dict(modality_to_generate=[0], given={4: ok}),
        dict(modality_to_generate=[0, 0]),
        dict(modality_to_generate=[4]),
        dict(modality_to_generate=[]),
        dict(modality_to_generate="every"),
        dict(modality_to_generate=0, given={1: ok}),  # given needs the list form
        dict(modality_to_generate=[0, 1], sample_fn=lambda probs: probs.argmax(-1, keepdim=True)),
        dict(modality_to_generate=[0, 1], temperature={0: -1.0}),
        dict(modality_to_generate=[0, 1], top_k={2: 5}),  # modality 2 is not generated
        dict(modality_to_generate=[0], given={1: torch.zeros(B * 2, N, dtype=torch.long)}),  # [B * S, N] without S
        dict(modality_to_generate=[0], given={1: ok}, num_samples=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.generate(start, max_new_tokens=N, **kw)
    ragged = [t[:, :6 + (i == 2)].cuda() for i, t in enumerate(idx)]
    assert ragged[2].shape[1] == 7
    with pytest.raises(ValueError):
        m.generate(ragged, max_new_tokens=N, modality_to_generate="all")
    monkeypatch.undo()
    out = m.generate(start, max_new_tokens=N, modality_to_generate=[0], given={1: ok})  # and the valid call runs
    assert tuple(out[0].shape) == (B, 6 + N) and bool((out[1][:, 6:] == 0).all())
