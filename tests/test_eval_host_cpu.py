"""The host side of the evaluation at every position: the two config keys, the ctypes signature and the entry's
refusals, the Python layer's refusals, the formatting of the printed lines, and that estimate_loss with
eval_positions: last never touches mmt_eval. None of it needs a device."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import config_utils as CU
import mmt_lib as ML


@pytest.fixture
def config():
    old = CU._config_cache
    CU._config_cache = {"block_size": 32, "batch_size": 8}
    yield CU._config_cache
    CU._config_cache = old


def test_config_keys_defaults_and_bad_values(config):
    tp = CU._DEFAULTS["training_parameters"]
    assert tp["eval_positions"] == "last" and tp["eval_positions_from"] == 0
    assert CU._get_eval_positions() == "last" and CU._get_eval_positions_from() == 0  # absent keys
    for good in ("last", "all"):
        config["eval_positions"] = good
        assert CU._get_eval_positions() == good
    for bad in ("every", "ALL", "", None, True, 1, ["all"]):
        config["eval_positions"] = bad
        with pytest.raises(ValueError, match="eval_positions"):
            CU._get_eval_positions()
    for good in (0, 5, 31, 32):
        config["eval_positions_from"] = good
        assert CU._get_eval_positions_from() == good
    for bad in (-1, 33, 1.0, "3", None, True):
        config["eval_positions_from"] = bad
        with pytest.raises(ValueError, match="eval_positions_from"):
            CU._get_eval_positions_from()


def test_config_keys_from_yaml(tmp_path):
    p = tmp_path / "config.yaml"
    p.write_text("training_parameters:\n  block_size: 16\n  eval_positions: all\n  eval_positions_from: 4\n")
    flat = CU.load_system_config(str(p))
    assert flat["eval_positions"] == "all" and flat["eval_positions_from"] == 4
    p.write_text("training_parameters:\n  block_size: 16\n")
    flat = CU.load_system_config(str(p))
    assert flat["eval_positions"] == "last" and flat["eval_positions_from"] == 0


def test_ctypes_signature_and_entry_refusals():
    """What mmt_eval_positions refuses is refused before any HIP call; so is what it skips."""
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    res, args = ML._SIGS["mmt_eval_positions"]
    assert res is i32 and len(args) == 19 and args[0] is vp and args[1:7] == [i32] * 6 and args[-2:] == [vp, i64]
    assert ML._SIGS["mmt_eval_positions_scratch_bytes"] == (i64, [i32] * 4)
    L = ML.lib()
    sb = L.mmt_eval_positions_scratch_bytes
    assert sb(2, 4, 16, 10) >= 2 * (4 * 16 * 8 + 16 * 100) * 8 and sb(0, 4, 16, 10) == 0
    for a in ((-1, 4, 16, 10), (1, -4, 16, 10), (1, 4, -16, 10), (1, 4, 16, 0), (1, 4, 16, 65), (1, 1 << 16, 1 << 15, 10)):
        assert sb(*a) == -1, a
    need = sb(1, 4, 16, 10)

    def call(count=1, batch=4, T=16, t_begin=0, bins=10, V_=13, lg=256, xb=256, yb=256, pos=256, rel=256, pit=256,
             scratch=256, nbytes=need, arrays=True):
        one = lambda x: (vp * 1)(x)
        return L.mmt_eval_positions(None, count, batch, T, t_begin, bins, 0, (i32 * 1)(V_) if arrays else None, one(lg),
                                    one(xb), one(yb), None, None, None, one(pos), one(rel), one(pit), scratch, nbytes)

    assert call(count=0) == 0 and call(batch=0) == 0 and call(t_begin=16) == 0
    for kw in (dict(count=-1), dict(batch=-1), dict(T=-1), dict(t_begin=-1), dict(t_begin=17), dict(bins=0),
               dict(bins=65), dict(batch=1 << 16, T=1 << 15, nbytes=1 << 60), dict(V_=0), dict(arrays=False),
               dict(lg=None), dict(xb=None), dict(yb=None), dict(pos=None), dict(rel=None), dict(pit=None),
               dict(scratch=None), dict(scratch=264), dict(nbytes=need - 1)):
        assert call(**kw) == -1, kw
    assert call(V_=(1 << 20) + 1) == -2


def _cpu_inputs(B=2, T=4, V=5):
    return ([torch.zeros(B, T, V)], [torch.zeros(B, T, dtype=torch.int64)], [torch.zeros(B, T, dtype=torch.int64)],
            [torch.zeros(V, dtype=torch.float64)], [False])


def test_python_layer_refusals_name_the_argument():
    import mmt_eval as ME
    lg, xb, yb, val, pct = _cpu_inputs()
    with pytest.raises(ValueError, match=r"logits_list\[0\].*GPU"):  # a CPU tensor
        ME.position_metrics(lg, xb, yb, val, pct)
    with pytest.raises(ValueError, match="bins"):
        ME.position_metrics(lg, xb, yb, val, pct, bins=65)
    with pytest.raises(ValueError, match="bins"):
        ME.position_metrics(lg, xb, yb, val, pct, bins=0)
    with pytest.raises(ValueError, match="t_begin"):
        ME.position_metrics(lg, xb, yb, val, pct, t_begin=-1)
    with pytest.raises(ValueError, match="xb_list"):
        ME.position_metrics(lg, [], yb, val, pct)
    with pytest.raises(ValueError, match="values"):
        ME.position_metrics(lg, xb, yb, None, pct)
    with pytest.raises(ValueError, match=r"logits_list\[0\]"):
        ME.position_metrics([lg[0].double()], xb, yb, val, pct)
    with pytest.raises(ValueError, match=r"logits_list\[0\]"):
        ME.position_metrics([lg[0][0]], xb, yb, val, pct)
    # (what comes after the device check of the logits is refused in tests/test_gpu_eval_positions.py)
    with pytest.raises(ValueError, match=r"PositionMetrics"):
        ME.PositionMetrics(val, [False, True])
    with pytest.raises(ValueError, match="bins"):
        ME.PositionMetrics(val, pct, bins=100)
    pm = ME.PositionMetrics(val, pct)
    with pytest.raises(ValueError, match="logits_list"):
        pm.add([], xb, yb)
    with pytest.raises(ValueError, match=r"logits_list\[0\].*GPU"):
        pm.add(lg, xb, yb)
    assert pm.result() == [] and pm.batches == 0


def test_derived_numbers_and_summary_lines():
    import mmt_eval as ME
    T, bins = 8, 4
    pos = np.zeros((T, 8))
    pos[2:, 0] = 10  # rows
    pos[2:, 1] = [6, 5, 5, 4, 4, 3]  # wins
    pos[2:, 2] = 10 - pos[2:, 1]
    pos[2:, 3] = 4.0
    pos[2:, 4] = 20.0
    pos[2:, 5] = 2
    pos[2:, 6] = 10
    pos[2:, 7] = 3.0
    rel = np.zeros((3, bins, 3))
    rel[2, 1] = [40, 16.0, 10]  # p_up in [1/4, 1/2): mean 0.4, realised 0.25
    rel[2, 2] = [20, 12.0, 14]  # p_up in [1/2, 3/4): mean 0.6, realised 0.7
    rel[0, 0] = [60, 6.0, 6]  # p_down: mean 0.1, realised 0.1
    pit = np.array([15.0, 15.0, 15.0, 15.0])
    r = ME.derive(pos, rel, pit, t_begin=2)
    assert (r["rows"], r["wins"], r["losses"], r["directed"]) == (60, 27, 33, 60)
    assert r["accuracy"] == 27 / 60 and r["nll"] == 2.0 and r["top1"] == 0.2 and r["certainty"] == 0.4
    assert r["realised_mass"] == pytest.approx(0.3)
    assert np.isnan(r["accuracy_per_position"][:2]).all() and list(r["accuracy_per_position"][2:]) == [.6, .5, .5, .4, .4, .3]
    q = r["accuracy_per_quarter"]
    assert np.isnan(q[0]) and q[1:] == [11 / 20, 9 / 20, 7 / 20]
    assert r["ece"]["up"] == pytest.approx((40 * 0.15 + 20 * 0.1) / 60) and r["ece"]["down"] == 0.0
    assert np.isnan(r["ece"]["flat"]) and list(r["pit_hist"]) == [.25] * 4
    text = ME.summary_text(r)
    assert text == ("27/60 (45.0%) | NLL 2.0000 | top-1 20.0% | ECE up 0.1333 down 0.0000 | "
                    "quarters n/a 55.0% 45.0% 35.0%")
    pm = ME.PositionMetrics([None], [False], t_begin=2, bins=bins)
    lines = pm.summary_lines("Close (ranged)", [r])
    assert lines == ["  - " + "Close (ranged)".ljust(30) + text]
    assert pm.summary_lines(["a"], [r])[0].startswith("  - a" + " " * 29 + "27/60")
    with pytest.raises(ValueError, match="name"):
        pm.summary_lines(["a", "b"], [r])
    empty = ME.derive(np.zeros((T, 8)), np.zeros((3, bins, 3)), np.zeros(bins))
    assert ME.summary_text(empty) == ("No directional predictions | NLL n/a | top-1 n/a | ECE up n/a down n/a | "
                                      "quarters n/a n/a n/a n/a")


def test_estimate_loss_with_last_never_touches_mmt_eval(monkeypatch, capsys, tmp_path):
    """eval_positions: last (and an absent key) runs estimate_loss without importing or calling mmt_eval: a sentinel
    module that raises on any attribute stands in for it. The model and the batcher are stand-ins too: the loop itself
    is what is exercised, on the CPU."""
    import training_utils as TU

    class Sentinel(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):  # what the import system itself looks up
                raise AttributeError(name)
            raise AssertionError(f"mmt_eval.{name} touched with eval_positions: last")

    monkeypatch.setitem(sys.modules, "mmt_eval", Sentinel("mmt_eval"))
    calls = []

    class Model:
        training = True

        def eval(self):
            pass

        def train(self):
            pass

        def __call__(self, xb, yb):
            return [torch.zeros(2, 4, 3)], [torch.tensor(1.5)]

    def metrics(logits, xb, yb, *a):
        calls.append(1)
        return [1], [1], [0.5], [1]

    params = [[None] * 12]
    params[0][9] = "Close"
    for k, v in dict(m=Model(), num_modalities=1, all_modality_params=params, all_vocabularies=[[0.0, 1.0, 2.0]],
                     get_batch=lambda s, t: ([torch.zeros(2, 4, dtype=torch.int64)], [torch.zeros(2, 4, dtype=torch.int64)]),
                     calculate_evaluation_metrics=metrics, sync_host_state=lambda: None).items():
        monkeypatch.setattr(TU, k, v, raising=False)
    old = CU._config_cache
    try:
        for extra in ({}, {"eval_positions": "last"}):
            CU._config_cache = dict({"block_size": 4, "batch_size": 2, "eval_iters": 2, "device": "cpu",
                                     "output_file_name": "log.txt", "project_file_path": str(tmp_path) + "/"}, **extra)
            out = TU.estimate_loss()
            assert out == {"train": 1.5, "val": 1.5}
            text = capsys.readouterr().out
            assert "DIRECTIONAL METRICS - Train Set" in text and "POSITION METRICS" not in text
        log = open(tmp_path / "output" / "log.txt").read()
        assert "DIRECTIONAL PREDICTION Val Set - Close: Correct=2 | Incorrect=2" in log and "POSITION" not in log
        assert len(calls) == 8
        CU._config_cache["eval_positions"] = "all"  # and the switch does reach for it
        with pytest.raises(AssertionError, match="mmt_eval"):
            TU.estimate_loss()
        CU._config_cache["eval_positions"] = "some"
        with pytest.raises(ValueError, match="eval_positions"):
            TU.estimate_loss()
    finally:
        CU._config_cache = old
