"""The restatement of mmt_eval_positions (tests/eval_ref.py) against the reference's own last-token metric and against
cases worked out by hand. No device."""
import math

import numpy as np
import torch

import eval_ref as E
import mmt_oracle as O
from golden_io import load


def per_position_against_oracle(logits, xb, yb, vocab, pct, bins=10):
    """At every t the restated wins / losses / certainty of position t are mmt_oracle.eval_metrics on the inputs cut to
    [:, :t + 1] (whose last token is position t)."""
    B, T, V = logits.shape
    rec = E.records(logits, xb, yb, np.asarray(vocab, dtype=np.float64), pct)
    pos, rel, pit = E.tables(rec, 0, bins)
    lt, xt, yt = torch.from_numpy(logits), torch.from_numpy(xb), torch.from_numpy(yb)
    for t in range(T):
        w, l, c, p = O.eval_metrics([lt[:, :t + 1]], [xt[:, :t + 1]], [yt[:, :t + 1]], [list(vocab)], [pct])
        if not p[0]:  # a value series needs two tokens of context in the reference (min_len 2): t = 0 is not scored
            assert t == 0 and not pct
            continue
        assert (pos[t, 1], pos[t, 2]) == (w[0], l[0]), (t, pos[t], w, l)
        # the reference's certainty is a sum of fp32 softmax values read one by one
        assert abs(pos[t, 3] - c[0]) <= 1e-5 * B, (t, pos[t, 3], c[0])
        assert pos[t, 0] == B and pos[t, 6] == B
    return rec, pos


def test_every_position_is_the_reference_last_token_rule_on_the_golden_arrays():
    z, meta = load("eval_metrics")
    for i in range(2):
        vocab = [float(v) for v in z[f"vocab.{i}"]]
        per_position_against_oracle(z[f"logits.{i}"].astype(np.float32), z[f"xb.{i}"], z[f"yb.{i}"], vocab,
                                    bool(meta["percent"][i]))
    # the whole-window call is the golden record itself
    for i in range(2):
        vocab = np.array([float(v) for v in z[f"vocab.{i}"]])
        rec = E.records(z[f"logits.{i}"], z[f"xb.{i}"], z[f"yb.{i}"], vocab, bool(meta["percent"][i]))
        T = rec.shape[1]
        pos, _, _ = E.tables(rec, T - 1, 10)
        assert (pos[T - 1, 1], pos[T - 1, 2]) == (z["wins"][i], z["losses"][i])
        assert math.isclose(pos[T - 1, 3], z["certainty"][i], rel_tol=1e-5)
        assert not pos[:T - 1].any()


def synthetic(V, B, T, seed, repeated):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0.0, 2.0, size=(B, T, V)).astype(np.float32)
    logits[0, :, :] = np.float32(0.5)  # all equal: the first index is predicted
    logits[1, :, 3] = logits[1, :, 7] = np.float32(9.0)  # a tie at the maximum
    logits[2, :, :] = np.round(logits[2, :, :])  # many ties
    xb = rng.integers(0, V, size=(B, T))
    yb = rng.integers(0, V, size=(B, T))
    yb[3] = xb[3]  # no change: the flat class of a value series
    return logits, xb, yb, E.series(V, "repeated" if repeated else "value", seed)


def test_every_position_is_the_reference_last_token_rule_on_ties_and_repeated_values():
    for pct in (False, True):
        for repeated in (False, True):
            logits, xb, yb, vocab = synthetic(12, 6, 5, 11 + repeated, repeated)
            rec, pos = per_position_against_oracle(logits, xb, yb, list(vocab), pct)
            if repeated:
                assert (rec[..., 2] > 0).any(), "the flat class is exercised"


def test_direction_masses_sum_to_one():
    for pct in (False, True):
        logits, xb, yb, vocab = synthetic(12, 6, 5, 5, True)
        rec = E.records(logits, xb, yb, vocab, pct)
        assert np.all(np.abs(rec[..., 1:4].sum(axis=-1) - 1.0) <= 4 * 2.0 ** -53)
        assert np.all((rec[..., 4] > 0) & (rec[..., 4] <= 1))


def test_hand_computed_two_by_three():
    """B = 2, T = 3, V = 3, values (-1, 0, 2) read as a percent series, bins = 2. Logits ln of small integers, so the
    law of a row is its integers over their sum:
      (b, t)   weights    yb  law             p_down p_flat p_up  PIT              rank  predicted realised
      (0, 0)   1 1 2      2   1/4 1/4 1/2     1/4    1/4    1/2   1/2 + 1/4 = 3/4  0     +1        +1
      (0, 1)   2 1 1      1   1/2 1/4 1/4     1/2    1/4    1/4   1/2 + 1/8 = 5/8  1     -1        0
      (0, 2)   1 2 1      0   1/4 1/2 1/4     1/4    1/2    1/4   1/8              1     0         -1
      (1, 0)   no finite logit: dead
      (1, 1)   1 1 1      0   1/3 each                            1/6              0     -1 (first) -1
      (1, 2)   1 3 (-inf) 2   1/4 3/4 0       1/4    3/4    0     1 + 0 = 1        2     0         +1
    """
    ln = np.log
    with np.errstate(all="ignore"):
        logits = np.array([[[ln(1), ln(1), ln(2)], [ln(2), ln(1), ln(1)], [ln(1), ln(2), ln(1)]],
                           [[-np.inf, np.nan, -np.inf], [0.0, 0.0, 0.0], [ln(1), ln(3), -np.inf]]], dtype=np.float32)
    yb = np.array([[2, 1, 0], [0, 0, 2]])
    xb = np.zeros((2, 3), dtype=np.int64)
    rec = E.records(logits, xb, yb, np.array([-1.0, 0.0, 2.0]), True)
    want = np.array([[[ln(0.5), .25, .25, .5, .75, 0, 1, 1], [ln(0.25), .5, .25, .25, .625, 1, -1, 0],
                      [ln(0.25), .25, .5, .25, .125, 1, 0, -1]],
                     [[np.nan] * 8, [ln(1 / 3), 1 / 3, 1 / 3, 1 / 3, 1 / 6, 0, -1, -1],
                      [-np.inf, .25, .75, 0, 1, 2, 0, 1]]])
    assert np.array_equal(np.isnan(rec), np.isnan(want))
    ok = ~np.isnan(want) & np.isfinite(want)
    assert np.all(np.abs(rec[ok] - want[ok]) <= 1e-6)  # fp32 logarithms went in
    assert rec[1, 2, 0] == -np.inf
    pos, rel, pit = E.tables(rec, 0, 2)
    #            rows wins losses certainty      nll                 top1 directed realised mass
    tol = dict(rtol=0, atol=1e-6)
    np.testing.assert_allclose(pos[0], [1, 1, 0, .5, -ln(.5), 1, 1, .5], **tol)
    np.testing.assert_allclose(pos[1], [2, 1, 1, .5 + 1 / 3, -ln(.25) - ln(1 / 3), 1, 2, .25 + 1 / 3], **tol)
    assert list(pos[2, :3]) == [2, 0, 2] and pos[2, 4] == np.inf and list(pos[2, 5:7]) == [0, 2]
    np.testing.assert_allclose(pos[2, [3, 7]], [.5 + .75, .25 + 0], **tol)
    # reliability, bins [0, 1/2) and [1/2, 1]: (count, sum of P, realised)
    np.testing.assert_allclose(rel[0], [[4, .25 + .25 + 1 / 3 + .25, 2], [1, .5, 0]], **tol)  # down
    np.testing.assert_allclose(rel[1], [[3, .25 + .25 + 1 / 3, 1], [2, .5 + .75, 0]], **tol)  # flat
    np.testing.assert_allclose(rel[2], [[4, .25 + .25 + 1 / 3 + 0, 1], [1, .5, 1]], **tol)  # up
    assert list(pit) == [2, 3]  # 1/8 and 1/6 below one half; 3/4, 5/8 and 1
    # counts are exact whatever the tolerance above
    assert rel[:, :, 0].sum() == 15 and rel[:, :, 2].sum() == 5 and pit.sum() == 5


def test_t_begin_at_the_last_position_is_the_last_token_metric():
    logits, xb, yb, vocab = synthetic(12, 6, 5, 3, True)
    for pct in (False, True):
        rec_all = E.records(logits, xb, yb, vocab, pct)
        rec = E.records(logits, xb, yb, vocab, pct, t_begin=4)
        assert np.isnan(rec[:, :4]).all() and np.array_equal(E.bits(rec[:, 4]), E.bits(rec_all[:, 4]))
        pos, rel, pit = E.tables(rec, 4, 10)
        w, l, c, p = O.eval_metrics([torch.from_numpy(logits)], [torch.from_numpy(xb)], [torch.from_numpy(yb)],
                                    [list(vocab)], [pct])
        assert (pos[4, 1], pos[4, 2]) == (w[0], l[0]) and abs(pos[4, 3] - c[0]) <= 6e-5
        assert not pos[:4].any() and rel[:, :, 0].sum() == 3 * 6 and pit.sum() == 6
        # the tables of a range are those of the full records restricted to it
        pos2, rel2, pit2 = E.tables(rec_all, 4, 10)
        assert np.array_equal(pos, pos2) and np.array_equal(rel, rel2) and np.array_equal(pit, pit2)
        # t_begin = T: nothing
        pos0, rel0, pit0 = E.tables(rec_all, 5, 10)
        assert not pos0.any() and not rel0.any() and not pit0.any()
