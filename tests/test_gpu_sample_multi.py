"""mmt_sample_multi (csrc/mmt_sample.hip): several sampling problems over the same rows in one launch.

The contract is bit equality with mmt_sample called alone per problem (tokens, compact tokens, log-probability bits),
so most of this file compares with separate mmt_sample launches; two problems are also compared with the CPU
restatement of the rule directly (tests/sampling_ref.py) under the clear / ambiguous rule and the delta of
tests/test_gpu_sample.py. Every output buffer is filled with sentinels and only the addressed column may change."""
import ctypes

import numpy as np
import pytest
import torch

import mmt_lib as ML
import sampling_ref as R
from test_gpu_sample import delta, launch, lp_tol, make_rows

pytestmark = pytest.mark.gpu

B = 33
TOK_SENT, LP_SENT = -7, 123.0
NAN = float("nan")


def problem(V, t, k, p, seed, strided=False, want_lp=True, compact=True, tok_stride=3):
    """A problem over make_rows(V, 33). strided: the rows are the last position of a [B, 4, V] tensor whose other
    positions hold a huge logit (reading them would win every draw)."""
    x = make_rows(V, B)
    if strided:
        full = np.full((B, 4, V), np.float32(50.0))
        full[:, 3, :] = x
        dev, offset, stride = torch.from_numpy(full).cuda(), 3 * V, 4 * V
    else:
        dev, offset, stride = torch.from_numpy(x.copy()).cuda(), 0, V
    return dict(V=V, x=x, dev=dev, offset=offset, stride=stride, t=t, k=k, p=p, seed=seed, want_lp=want_lp,
                compact=compact, tok_stride=tok_stride)


def arr(ctype, values):
    return (ctype * max(1, len(values)))(*values)


def run_multi(probs, pos, row0=0, batch=B, null_lp_array=False, null_compact_array=False, override=None):
    """One mmt_sample_multi call. Token buffers are [B, tok_stride] with the last column addressed, log-probability
    buffers [B, 3] with the middle column addressed, all filled with sentinels; returns the status and per problem
    (tokens, logprobs | None, compact | None) on the CPU after checking that nothing else was written. `override`
    replaces entries of the host arrays: {name: {problem: value}}."""
    toks = [torch.full((B, q["tok_stride"]), TOK_SENT, dtype=torch.int64, device="cuda") for q in probs]
    lps = [torch.full((B, 3), LP_SENT, dtype=torch.float32, device="cuda") for q in probs]
    cmps = [torch.full((B,), TOK_SENT, dtype=torch.int64, device="cuda") for q in probs]
    a = dict(
        V=[q["V"] for q in probs],
        logits=[q["dev"].data_ptr() + 4 * q["offset"] for q in probs],
        row_stride=[q["stride"] for q in probs],
        t=[q["t"] for q in probs], k=[q["k"] for q in probs], p=[q["p"] for q in probs],
        seed=[q["seed"] for q in probs],
        tok=[tk.data_ptr() + 8 * (q["tok_stride"] - 1) for tk, q in zip(toks, probs)],
        tok_stride=[q["tok_stride"] for q in probs],
        compact=[c.data_ptr() if q["compact"] else None for c, q in zip(cmps, probs)],
        lp=[l.data_ptr() + 4 if q["want_lp"] else None for l, q in zip(lps, probs)],
        lp_stride=[3] * len(probs))
    for name, repl in (override or {}).items():
        for i, v in repl.items():
            a[name][i] = v
    rc = ML.lib().mmt_sample_multi(
        ML.stream_ptr(torch.device("cuda")), len(probs), batch, arr(ctypes.c_int32, a["V"]),
        arr(ctypes.c_void_p, a["logits"]), arr(ctypes.c_int64, a["row_stride"]), arr(ctypes.c_float, a["t"]),
        arr(ctypes.c_int32, a["k"]), arr(ctypes.c_float, a["p"]), arr(ctypes.c_uint64, a["seed"]), row0, pos,
        arr(ctypes.c_void_p, a["tok"]), arr(ctypes.c_int64, a["tok_stride"]),
        None if null_compact_array else arr(ctypes.c_void_p, a["compact"]),
        None if null_lp_array else arr(ctypes.c_void_p, a["lp"]), arr(ctypes.c_int64, a["lp_stride"]))
    torch.cuda.synchronize()
    out = []
    for q, tk, l, c in zip(probs, toks, lps, cmps):
        tk, l, c = tk.cpu(), l.cpu(), c.cpu()
        assert bool((tk[:, :-1] == TOK_SENT).all()), "wrote outside its token column"
        assert bool((l[:, 0] == LP_SENT).all()) and bool((l[:, 2] == LP_SENT).all()), "wrote outside its logprob column"
        has_lp, has_c = q["want_lp"] and not null_lp_array, q["compact"] and not null_compact_array
        if not has_lp:
            assert bool((l == LP_SENT).all()), "wrote a log-probability nobody asked for"
        if not has_c:
            assert bool((c == TOK_SENT).all()), "wrote a compact token nobody asked for"
        out.append((tk[:, -1], l[:, 1] if has_lp else None, c if has_c else None))
    return rc, out


def untouched(out):
    return all(bool((tk == TOK_SENT).all()) and (l is None or bool((l == LP_SENT).all()))
               and (c is None or bool((c == TOK_SENT).all())) for tk, l, c in out)


def assert_equals_single(probs, out, pos, row0=0):
    """Problem by problem: the bits of mmt_sample called alone with the problem's arguments."""
    for i, (q, (tk, l, c)) in enumerate(zip(probs, out)):
        s_tok, s_lp, s_c, rc = launch(q["dev"], q["V"], B, q["t"], q["k"], q["p"], pos, row0=row0,
                                      row_stride=q["stride"], tok_stride=q["tok_stride"], compact=True,
                                      offset=q["offset"], seed=q["seed"])
        assert rc == 0
        assert int(tk.min()) >= 0 and int(tk.max()) < q["V"], i
        assert torch.equal(tk, s_tok), (i, q["V"])
        if c is not None:
            assert torch.equal(c, s_c), (i, q["V"])
        if l is not None:
            assert torch.equal(l.view(torch.int32), s_lp.view(torch.int32)), (i, q["V"])


def assert_matches_rule(q, tk, l, pos, row0=0):
    V, d = q["V"], delta(q["V"])
    ref = R.sample_rows(q["x"], q["t"], q["k"], q["p"], q["seed"], pos, row0)
    amb, bad = R.check_tokens(ref, tk.numpy(), d)
    print(f"multi V={V} t={q['t']} k={q['k']} p={q['p']}: ambiguous {amb}/{B} delta {d:.2e}")
    assert not bad, (V, bad, tk.numpy()[bad], ref["token"][bad], ref["neighbor"][bad])
    assert amb <= 0.05 * B, (V, amb)
    clear = (ref["margin_u"] >= d) & (ref["margin_p"] >= d)
    err = np.abs(l.numpy().astype(np.float64) - ref["logprob"])[clear]
    assert np.all(err <= lp_tol(V, ref["logprob"][clear])), (V, float(err.max()))


def mixed():
    """V = 5, 13, 57, 900, 8192: plain, top-k, top-p (read strided from a [B, 4, V] tensor), both, greedy; a seed
    each."""
    return [problem(5, 1.0, 0, 1.0, 0x1111111111111111),
            problem(13, 0.8, 4, 1.0, 0x2222222233333333),
            problem(57, 0.8, 0, 0.9, 0xC0FFEE1234, strided=True),
            problem(900, 1.3, 50, 0.5, 0xFFFFFFFFFFFFFFFF),
            problem(8192, 0.0, 7, 0.3, 5)]


def test_mixed_problems_equal_separate_launches_and_the_rule():
    probs = mixed()
    rc, out = run_multi(probs, pos=17, row0=3)
    assert rc == 0
    assert_equals_single(probs, out, 17, row0=3)
    for i in (2, 3):
        assert_matches_rule(probs[i], out[i][0], out[i][1], 17, row0=3)
    greedy = out[4][0].numpy()
    assert np.array_equal(greedy, np.argmax(probs[4]["x"], axis=1))
    # another position draws anew, and a problem's draw does not depend on its neighbours in the launch
    rc, other = run_multi(probs, pos=18, row0=3)
    assert rc == 0 and not torch.equal(other[3][0], out[3][0])
    rc, alone = run_multi(probs[3:4], pos=17, row0=3)
    assert rc == 0 and torch.equal(alone[0][0], out[3][0])
    assert torch.equal(alone[0][1].view(torch.int32), out[3][1].view(torch.int32))


def test_a_row_too_large_for_lds_joins_the_launch():
    """V = 8200 runs the re-read variant (a second launch); the other five keep their bits."""
    probs = mixed() + [problem(8200, 0.9, 40, 0.8, 77)]
    probs = probs[:2] + probs[5:] + probs[2:5]  # the large one in the middle of the caller's order
    rc, out = run_multi(probs, pos=4)
    assert rc == 0
    assert_equals_single(probs, out, 4)
    assert_matches_rule(probs[2], out[2][0], out[2][1], 4)


def test_nine_problems_run_in_chunks():
    sets = [(1.0, 0, 1.0), (0.8, 3, 1.0), (0.7, 0, 0.8), (1.2, 6, 0.6), (0.0, 0, 1.0)]
    probs = [problem([5, 13, 57, 144, 900][i % 5], *sets[(i * 2) % 5], seed=1000 + 7 * i, strided=i == 8,
                     tok_stride=1 + i % 3) for i in range(9)]
    rc, out = run_multi(probs, pos=9, row0=100)
    assert rc == 0
    assert_equals_single(probs, out, 9, row0=100)
    # same V, same settings, other seed: other draws (problems 0 and 5 share V = 5 and settings)
    assert probs[0]["V"] == probs[5]["V"] and sets[0] == sets[(5 * 2) % 5]
    assert not torch.equal(out[0][0], out[5][0])


def test_optional_outputs_per_problem_and_per_array():
    probs = mixed()[:4]
    probs[1]["want_lp"] = False
    probs[2]["compact"] = False
    probs[3]["want_lp"] = probs[3]["compact"] = False
    rc, out = run_multi(probs, pos=2)  # run_multi checks that absent outputs keep their sentinels
    assert rc == 0
    assert out[1][1] is None and out[2][2] is None and out[3][1] is None and out[3][2] is None
    assert_equals_single(probs, out, 2)
    full = mixed()[:4]
    rc, out2 = run_multi(full, pos=2, null_lp_array=True, null_compact_array=True)
    assert rc == 0 and all(l is None and c is None for _, l, c in out2)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(out, out2))


INVALID = {
    "V = 0": dict(V={2: 0}),
    "V < 0": dict(V={2: -3}),
    "row_stride < V": dict(row_stride={2: 56}),
    "temperature < 0": dict(t={2: -0.5}),
    "temperature NaN": dict(t={2: NAN}),
    "top_k < 0": dict(k={2: -1}),
    "top_p NaN": dict(p={2: NAN}),
    "null logits": dict(logits={2: None}),
    "null tok": dict(tok={2: None}),
}


@pytest.mark.parametrize("what", list(INVALID))
def test_an_invalid_last_problem_stops_the_whole_call(what):
    probs = mixed()[:3]
    rc, out = run_multi(probs, pos=1, override=INVALID[what])
    assert rc == -1, what  # MMT_ERR_INVALID
    assert untouched(out), what


def test_unsupported_and_shared_argument_refusals():
    probs = mixed()[:3]
    rc, out = run_multi(probs, pos=1, override=dict(V={2: 2 ** 20 + 1}, row_stride={2: 2 ** 20 + 1}))
    assert rc == -2 and untouched(out)  # MMT_ERR_UNSUPPORTED
    rc, out = run_multi(probs, pos=1, batch=-1)
    assert rc == -1 and untouched(out)
    L, st = ML.lib(), ML.stream_ptr(torch.device("cuda"))
    assert L.mmt_sample_multi(st, -1, B, *[None] * 7, 0, 0, *[None] * 5) == -1
    assert L.mmt_sample_multi(st, 2, B, *[None] * 7, 0, 0, *[None] * 5) == -1  # null arrays with problems
    rc, out = run_multi(probs, pos=1)  # and the same problems unmodified run
    assert rc == 0 and not untouched(out)


def test_empty_calls_launch_nothing():
    L, st = ML.lib(), ML.stream_ptr(torch.device("cuda"))
    assert L.mmt_sample_multi(st, 0, B, *[None] * 7, 0, 0, *[None] * 5) == 0  # no problems, no arrays
    rc, out = run_multi(mixed()[:3], pos=1, batch=0)
    assert rc == 0 and untouched(out)
    rc, out = run_multi(mixed()[:3], pos=1, batch=0, override=dict(k={1: -1}))
    assert rc == -1  # validated all the same, as mmt_sample


def test_public_wrapper_equals_sample():
    import mmt_sample as MS
    probs = mixed()[:4]
    views = [q["dev"] if q["offset"] == 0 else q["dev"][:, -1, :] for q in probs]
    seeds = [MS.modality_seed(99, i) for i in range(4)]
    toks, lps = MS.sample_multi(views, temperature=[1.0, 0.8, 0.8, 1.3], top_k=[0, 4, 0, 50], top_p=0.9, seeds=seeds,
                                pos=6, row0=2, return_logprobs=True)
    for i, v in enumerate(views):
        t, l = MS.sample(v, temperature=[1.0, 0.8, 0.8, 1.3][i], top_k=[0, 4, 0, 50][i], top_p=0.9, seed=seeds[i],
                         pos=6, row0=2, return_logprobs=True)
        assert torch.equal(toks[i], t) and torch.equal(lps[i].view(torch.int32), l.view(torch.int32)), i
    only = MS.sample_multi(views[:2], seeds=5, pos=0)
    assert len(only) == 2 and tuple(only[0].shape) == (B,) and only[0].dtype == torch.int64
    assert MS.sample_multi([], seeds=[], pos=0) == []
    with pytest.raises(ValueError):
        MS.sample_multi(views, temperature=[1.0, 0.8], seeds=seeds, pos=0)
    with pytest.raises(ValueError):
        MS.sample_multi(views, temperature=-1.0, seeds=seeds, pos=0)
    with pytest.raises(ValueError):
        MS.sample_multi([views[0], views[1][:5]], seeds=[1, 2], pos=0)
