"""Host side of the training objective, no device: the four config getters, mmt_loss.balanced_class_weights,
MultimodalTransformer.set_loss's normalisation and validation (the library's mmt_set_loss replaced by a recorder),
and the C entry points' own refusals (mmt_create needs no device)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import config_utils as CU
import mmt_lib as ML
import mmt_loss


@pytest.fixture
def cfg():
    old = CU._config_cache
    CU._config_cache = {"n_embd": 32, "n_head": 2, "n_layer": 1, "block_size": 8, "dropout": 0.0, "device": "cpu",
                        "batch_size": 2, "eval_iters": 1, "precision": "bf16"}
    yield CU._config_cache
    CU._config_cache = old


# ---------------------------------------------------------------- config getters
def test_getters_default_with_the_keys_absent(cfg):
    assert CU._get_label_smoothing() == 0.0 and CU._get_label_smoothing(3) == 0.0
    assert CU._get_loss_class_weights() is None
    assert CU._get_loss_class_weight_power() == 1.0
    assert CU._get_loss_positions_from() == 0
    flat = CU.load_system_config("/nonexistent/config.yaml")
    assert flat["label_smoothing"] == 0.0 and flat["loss_class_weights"] is None
    assert flat["loss_class_weight_power"] == 1.0 and flat["loss_positions_from"] == 0


def test_getters_valid_forms(cfg):
    cfg.update(label_smoothing=0.1, loss_class_weights="balanced", loss_class_weight_power=0.5, loss_positions_from=7)
    assert CU._get_label_smoothing(2) == 0.1
    assert CU._get_loss_class_weights() == "balanced"
    assert CU._get_loss_class_weight_power() == 0.5
    assert CU._get_loss_positions_from() == 7
    cfg.update(label_smoothing=[0, 0.25], loss_class_weight_power=0, loss_positions_from=0)
    assert CU._get_label_smoothing(2) == [0.0, 0.25] and CU._get_label_smoothing() == [0.0, 0.25]
    assert CU._get_loss_class_weight_power() == 0.0
    cfg.update(loss_class_weight_power=1)
    assert CU._get_loss_class_weight_power() == 1.0


@pytest.mark.parametrize("key,getter,bad", [
    ("label_smoothing", "_get_label_smoothing", [1.0, -0.1, float("nan"), "0.1", True, None, [], [0.1, 1.0], [0.1, "x"]]),
    ("loss_class_weights", "_get_loss_class_weights", ["inverse", True, 1, ["balanced"]]),
    ("loss_class_weight_power", "_get_loss_class_weight_power", [-0.1, 1.5, float("nan"), "1", True, None]),
    ("loss_positions_from", "_get_loss_positions_from", [-1, 8, 1.0, "0", True, None]),
])
def test_getters_reject(cfg, key, getter, bad):
    for v in bad:
        cfg[key] = v
        with pytest.raises(ValueError, match=key):
            getattr(CU, getter)()
    del cfg[key]
    getattr(CU, getter)()


def test_label_smoothing_list_length_is_checked_against_the_modalities(cfg):
    cfg["label_smoothing"] = [0.1, 0.2]
    with pytest.raises(ValueError, match="one value per modality"):
        CU._get_label_smoothing(3)


# ---------------------------------------------------------------- balanced class weights
@pytest.mark.parametrize("power", [1.0, 0.5, 0.0])
def test_balanced_class_weights(power):
    rng = np.random.default_rng(5)
    V = 9
    tokens = rng.choice([0, 1, 2, 4, 7], size=5000, p=[0.6, 0.2, 0.1, 0.07, 0.03])
    w = mmt_loss.balanced_class_weights(tokens, V, power)
    assert w.dtype == torch.float32 and w.shape == (V,)
    count = np.bincount(tokens, minlength=V)
    n = tokens.size
    np.testing.assert_allclose(float((torch.from_numpy(count).double() * w.double()).sum()), n, rtol=1e-6)
    assert (w[count == 0] == 0).all() and (w[count > 0] > 0).all()
    seen = np.flatnonzero(count)
    if power == 0.0:
        assert (w[seen] == 1).all()
    else:  # w_c proportional to (n / count_c) ** power
        ratio = w[seen].double().numpy() / (n / count[seen]) ** power
        np.testing.assert_allclose(ratio, ratio[0], rtol=1e-6)
    # the same from a tensor
    assert torch.equal(mmt_loss.balanced_class_weights(torch.from_numpy(tokens), V, power), w)


def test_balanced_class_weights_reject():
    with pytest.raises(ValueError):
        mmt_loss.balanced_class_weights(np.array([0, 5]), 5)
    with pytest.raises(ValueError):
        mmt_loss.balanced_class_weights(np.array([-1, 2]), 5)
    with pytest.raises(ValueError):
        mmt_loss.balanced_class_weights(np.array([], dtype=np.int64), 5)
    with pytest.raises(ValueError):
        mmt_loss.balanced_class_weights(np.array([0.5, 1.0]), 5)
    for p in (-0.1, 1.1, float("nan"), "1", True):
        with pytest.raises(ValueError):
            mmt_loss.balanced_class_weights(np.array([0, 1]), 5, p)


# ---------------------------------------------------------------- set_loss
V = [5, 9]
T = 8


@pytest.fixture
def model(cfg, monkeypatch):
    """A model on the CPU (no forward is run) whose mmt_set_loss calls are recorded instead of made."""
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(2, V, [[None] * 12, [None] * 12])
    real = ML.lib()
    calls = []

    def fake_set_loss(ctx, arr):
        calls.append(None if arr is None else
                     [(arr[i].label_smoothing, arr[i].class_weight, arr[i].position_weight) for i in range(2)])
        return 0

    stub = types.SimpleNamespace(mmt_set_loss=fake_set_loss, mmt_last_error=real.mmt_last_error,
                                 mmt_destroy=real.mmt_destroy)
    monkeypatch.setattr(ML, "lib", lambda: stub)
    yield m, calls
    monkeypatch.undo()


def test_set_loss_normalises_every_argument_form(model):
    m, calls = model
    assert m.loss_spec is None
    w0, w1, u = torch.rand(5) + 0.1, torch.rand(9) + 0.1, torch.linspace(0, 1, T)
    m.set_loss(0.1, {0: w0, 1: w1.double()}, u.tolist())
    spec = m.loss_spec
    assert [s["label_smoothing"] for s in spec] == [0.1, 0.1]
    assert torch.equal(spec[0]["class_weights"], w0) and torch.equal(spec[1]["class_weights"], w1)
    assert all(torch.equal(s["position_weights"], u) and s["position_weights"].dtype == torch.float32 for s in spec)
    eps, cw, pw = zip(*calls[-1])
    assert eps == (pytest.approx(0.1), pytest.approx(0.1)) and all(cw) and all(pw)
    assert cw[0] == m._loss_dev[1][0][0].data_ptr() and pw[1] == m._loss_dev[1][1][1].data_ptr()  # kept alive
    # dict forms leave the other modalities plain
    m.set_loss({1: 0.2}, {0: w0})
    spec = m.loss_spec
    assert [s["label_smoothing"] for s in spec] == [0.0, 0.2]
    assert spec[1]["class_weights"] is None and spec[0]["position_weights"] is None
    assert calls[-1][0][1] and not calls[-1][1][1] and not calls[-1][0][2]
    # a 0-d tensor is a scalar
    m.set_loss(torch.tensor(0.3))
    assert [s["label_smoothing"] for s in m.loss_spec] == [pytest.approx(0.3)] * 2
    # no arguments, and all-neutral arguments: back to the plain loss (a NULL spec)
    m.set_loss()
    assert m.loss_spec is None and calls[-1] is None and m._loss_dev is None
    m.set_loss(0.0, None, {0: None})
    assert m.loss_spec is None and calls[-1] is None
    # not part of state_dict
    m.set_loss(0.1, None, u)
    assert not any("loss" in k for k in m.state_dict())


@pytest.mark.parametrize("kw", [
    {"label_smoothing": 1.0}, {"label_smoothing": -0.01}, {"label_smoothing": float("nan")},
    {"label_smoothing": "0.1"}, {"label_smoothing": True}, {"label_smoothing": {2: 0.1}},
    {"label_smoothing": torch.tensor([0.1, 0.2])},
    {"class_weights": torch.ones(5)},  # [5] fits modality 0 only
    {"class_weights": {0: torch.ones(4)}}, {"class_weights": {1: torch.ones(3, 3)}},
    {"class_weights": {0: torch.tensor([1, 1, float("inf"), 1, 1])}},
    {"class_weights": {0: torch.tensor([1, 1, float("nan"), 1, 1])}},
    {"class_weights": {0: torch.tensor([1.0, -1, 1, 1, 1])}}, {"class_weights": {0: torch.zeros(5)}},
    {"class_weights": {-1: torch.ones(5)}}, {"class_weights": {"0": torch.ones(5)}},
    {"position_weights": torch.ones(T + 1)}, {"position_weights": torch.zeros(T)},
    {"position_weights": {1: -torch.ones(T)}}, {"position_weights": torch.ones(T, dtype=torch.bool)},
])
def test_set_loss_rejects_before_anything_changes(model, kw):
    m, calls = model
    u = torch.ones(T)
    u[0] = 0
    m.set_loss(0.1, None, u)
    n = len(calls)
    before = m.loss_spec
    with pytest.raises(ValueError):
        m.set_loss(**kw)
    assert len(calls) == n
    after = m.loss_spec
    assert [s["label_smoothing"] for s in after] == [s["label_smoothing"] for s in before]
    assert all(torch.equal(a["position_weights"], b["position_weights"]) for a, b in zip(after, before))


# ---------------------------------------------------------------- the C entry points
def test_c_set_loss_refuses_eps_outside_the_range_and_keeps_its_state(cfg):
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(2, V, [[None] * 12, [None] * 12])
    L = ML.lib()
    arr, out = (ML.MmtLossSpec * 2)(), (ML.MmtLossSpec * 2)()
    keep = torch.ones(9)
    arr[0].label_smoothing, arr[1].label_smoothing, arr[1].class_weight = 0.25, 0.5, keep.data_ptr()
    assert L.mmt_set_loss(m._ctx, arr) == 0
    for bad in (1.0, -0.5, float("nan"), float("inf")):
        arr2 = (ML.MmtLossSpec * 2)()
        arr2[0].label_smoothing, arr2[1].label_smoothing = 0.1, bad
        assert L.mmt_set_loss(m._ctx, arr2) == -1
        assert b"label_smoothing" in L.mmt_last_error(m._ctx)
        assert L.mmt_get_loss(m._ctx, out) == 0
        assert (out[0].label_smoothing, out[1].label_smoothing) == (0.25, 0.5)
        assert out[1].class_weight == keep.data_ptr() and not out[0].class_weight and not out[1].position_weight
    assert L.mmt_set_loss(m._ctx, None) == 0
    assert L.mmt_get_loss(m._ctx, out) == 0
    assert all(o.label_smoothing == 0 and not o.class_weight and not o.position_weight for o in out)
    assert L.mmt_set_loss(None, arr) == -1 and L.mmt_get_loss(m._ctx, None) == -1


def test_c_op_refuses_bad_arguments_before_any_launch():
    L = ML.lib()
    one = ctypes.c_void_p(8)  # never dereferenced: every call below is refused on the host
    args = dict(R=4, T=2, V=5, ld=8, eps=0.1, cw=None, pw=None, denom=None)

    def call(**kw):
        a = dict(args, **kw)
        return L.mmt_op_cross_entropy_spec(None, a["R"], a["T"], a["V"], one, one, one, a["ld"], one, a["eps"], a["cw"],
                                           a["pw"], a["denom"], None, None)

    for kw in ({"R": 0}, {"T": 0}, {"V": 0}, {"ld": 4}, {"eps": 1.0}, {"eps": -0.1}, {"eps": float("nan")},
               {"cw": one}, {"pw": one}):
        assert call(**kw) == -1, kw
