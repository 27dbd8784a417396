"""The host side of the calibrated temperatures: the config key, the default grid, what temperature="calibrated"
resolves to, the check behind set_calibrated_temperatures, the declarations, the entry's refusals that need no device,
and that estimate_loss with eval_temperature: off never touches mmt_eval. None of it needs a device."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import config_utils as CU
import mmt_lib as ML

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def config():
    old = CU._config_cache
    CU._config_cache = {"block_size": 32, "batch_size": 8}
    yield CU._config_cache
    CU._config_cache = old


def test_config_key_default_and_bad_values(config, tmp_path):
    assert CU._DEFAULTS["training_parameters"]["eval_temperature"] == "off"
    assert CU._get_eval_temperature() == "off"  # an absent key
    for good in ("off", "fit"):
        config["eval_temperature"] = good
        assert CU._get_eval_temperature() == good
    config["eval_temperature"] = False  # YAML's reading of a bare `off`
    assert CU._get_eval_temperature() == "off"
    for bad in ("on", "FIT", "", None, True, 1, ["fit"]):
        config["eval_temperature"] = bad
        with pytest.raises(ValueError, match="eval_temperature"):
            CU._get_eval_temperature()
    p = tmp_path / "config.yaml"
    p.write_text("training_parameters:\n  block_size: 16\n  eval_temperature: fit\n")
    assert CU.load_system_config(str(p))["eval_temperature"] == "fit"
    p.write_text("training_parameters:\n  block_size: 16\n")
    assert CU.load_system_config(str(p))["eval_temperature"] == "off"


def test_default_temperatures():
    import mmt_eval as ME
    t = ME.default_temperatures()
    assert t.dtype == np.float32 and t.shape == (17,) and (np.diff(t) > 0).all()
    assert t[8] == 1.0 and t[0] == 0.25 and t[16] == 4.0 and t[4] == 0.5 and t[12] == 2.0
    assert np.array_equal(t, np.array([2.0 ** ((k - 8) / 4) for k in range(17)]).astype(np.float32))
    tf = ME.TemperatureFit([None], [False])
    assert np.array_equal(tf.temperatures(), t) and tf.result() == [] and tf.batches == 0
    assert np.array_equal(ME.TemperatureFit([None], [False], temperatures=[0.5, 1.5]).temperatures(),
                          np.array([0.5, 1.5], dtype=np.float32))
    for bad in ([], [2.0, 1.0], [0.0, 1.0], [float("nan")], list(range(1, 34))):
        with pytest.raises(ValueError, match="temperatures"):
            ME.TemperatureFit([None], [False], temperatures=bad)
    with pytest.raises(ValueError, match="TemperatureFit"):
        ME.TemperatureFit([None], [False, True])
    with pytest.raises(ValueError, match="bins"):
        ME.TemperatureFit([None], [False], bins=65)
    with pytest.raises(ValueError, match=r"logits_list\[0\].*GPU"):  # a CPU tensor
        tf.add([torch.zeros(2, 4, 5)], [torch.zeros(2, 4, dtype=torch.int64)], [torch.zeros(2, 4, dtype=torch.int64)])
    with pytest.raises(ValueError, match=r"logits_list\[0\].*GPU"):
        ME.temperature_metrics([torch.zeros(2, 4, 5)], [torch.zeros(2, 4, dtype=torch.int64)],
                               [torch.zeros(2, 4, dtype=torch.int64)], [None], [False])


def test_calibrated_resolves_to_the_stored_numbers():
    import mmt_rollout as MR
    store = {0: 1.25, 2: 0.8}
    res = lambda g, s=store: MR.resolve_calibrated("calibrated", s, g, 3)
    assert res(0) == 1.25 and res(2) == 0.8  # the int form: the number
    assert res([0]) == {0: 1.25} and res([2, 0]) == {2: 0.8, 0: 1.25} and res((0, 2)) == {0: 1.25, 2: 0.8}
    with pytest.raises(ValueError, match="modality 1 has no calibrated temperature"):
        res(1)
    with pytest.raises(ValueError, match="modality 1 has no calibrated temperature"):
        res([0, 1, 2])
    with pytest.raises(ValueError, match="modality 1 has no calibrated temperature"):
        res("all")
    assert res("all", {0: 1.0, 1: 2.0, 2: 3.0}) == {0: 1.0, 1: 2.0, 2: 3.0}
    for g in (0, [0], "all"):
        with pytest.raises(ValueError, match="modality 0 has no calibrated temperature"):
            res(g, {})  # an empty store
    # anything else passes through untouched, and so does a modality_to_generate that is refused later anyway
    for t in (None, 0.7, {0: 0.7}, "Calibrated"):
        assert MR.resolve_calibrated(t, {}, 0, 3) is t
    for g in ("every", True, [True], [0.5], 1.5):
        assert MR.resolve_calibrated("calibrated", store, g, 3) == "calibrated"


def test_set_calibrated_temperatures_validation():
    import mmt_rollout as MR
    chk = MR.check_calibrated_temperatures
    assert chk(None, 3) == {} and chk({}, 3) == {}
    given = {0: 1, 2: np.float32(0.5)}
    got = chk(given, 3)
    assert got == {0: 1.0, 2: 0.5} and got is not given and all(type(v) is float for v in got.values())
    for bad in ({3: 1.0}, {-1: 1.0}, {"0": 1.0}, {True: 1.0}, {0.0: 1.0}, {0: 0.0}, {0: -1.0}, {0: float("inf")},
                {0: float("nan")}, {0: "1"}, {0: None}, {0: True}, [1.0], 1.0, "calibrated"):
        with pytest.raises(ValueError, match="set_calibrated_temperatures"):
            chk(bad, 3)
    # the model's method is this check on a plain attribute
    import inspect
    import model
    src = inspect.getsource(model.MultimodalTransformer.set_calibrated_temperatures)
    assert "check_calibrated_temperatures(mapping, self.num_modalities)" in src

    class Stub:
        num_modalities = 2
        set_calibrated_temperatures = model.MultimodalTransformer.set_calibrated_temperatures

    s = Stub()
    s.set_calibrated_temperatures({1: 2})
    assert s.calibrated_temperatures == {1: 2.0}
    s.set_calibrated_temperatures(None)
    assert s.calibrated_temperatures == {}
    with pytest.raises(ValueError):
        s.set_calibrated_temperatures({2: 1.0})


def test_declared_bound_and_built():
    import mmt_build
    hdr = open(os.path.join(REPO, "include", "mmt.h")).read()
    assert "int mmt_eval_temperatures(void* stream," in hdr
    assert "int64_t mmt_eval_temperatures_scratch_bytes(int32_t count, int32_t batch, int32_t T, int32_t bins, int32_t K);" in hdr
    assert "mmt_evaltemp.hip" in mmt_build.SOURCES
    assert os.path.exists(os.path.join(mmt_build.CSRC, "mmt_evaltemp.hip"))
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    res, args = ML._SIGS["mmt_eval_temperatures"]
    assert res is i32 and len(args) == 20 and args[0] is vp and args[1:8] == [i32] * 7 and args[-2:] == [vp, i64]
    assert args[8] == ctypes.POINTER(ctypes.c_float)
    assert ML._SIGS["mmt_eval_temperatures_scratch_bytes"] == (i64, [i32] * 5)
    L = ML.lib()
    assert hasattr(L, "mmt_eval_temperatures") and hasattr(L, "mmt_eval_temperatures_scratch_bytes")


def test_entry_refusals_before_any_hip_call():
    i32, vp, f32 = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float
    L = ML.lib()
    sb = L.mmt_eval_temperatures_scratch_bytes
    assert sb(2, 4, 16, 10, 3) == 2 * (4 * 16 * 3 * 4 + 16 * 3 * 92) * 8 and sb(0, 4, 16, 10, 3) == 0
    for a in ((-1, 4, 16, 10, 3), (1, -4, 16, 10, 3), (1, 4, -16, 10, 3), (1, 4, 16, 0, 3), (1, 4, 16, 65, 3),
              (1, 1 << 16, 1 << 15, 10, 3), (1, 4, 16, 10, 0), (1, 4, 16, 10, 33)):
        assert sb(*a) == -1, a
    need = sb(1, 4, 16, 10, 3)

    def call(count=1, batch=4, T=16, t_begin=0, bins=10, K=3, temps=(0.5, 1.0, 2.0), V_=13, lg=256, xb=256, yb=256,
             tot=256, rel=256, scratch=256, nbytes=need, arrays=True):
        one = lambda x: (vp * 1)(x)
        t = None if temps is None else (f32 * len(temps))(*temps)
        return L.mmt_eval_temperatures(None, count, batch, T, t_begin, bins, 0, K, t, (i32 * 1)(V_) if arrays else None,
                                       one(lg), one(xb), one(yb), None, None, None, one(tot), one(rel), scratch, nbytes)

    assert call(count=0) == 0 and call(batch=0) == 0 and call(t_begin=16) == 0
    inf, nan = float("inf"), float("nan")
    for kw in (dict(count=-1), dict(batch=-1), dict(T=-1), dict(t_begin=-1), dict(t_begin=17), dict(bins=0),
               dict(bins=65), dict(batch=1 << 16, T=1 << 15, nbytes=1 << 60), dict(V_=0), dict(arrays=False),
               dict(lg=None), dict(xb=None), dict(yb=None), dict(tot=None), dict(rel=None), dict(scratch=None),
               dict(scratch=264), dict(nbytes=need - 1), dict(K=0), dict(K=33), dict(temps=None),
               dict(temps=(0.5, 1.0, inf)), dict(temps=(0.5, nan, 2.0)), dict(temps=(0.0, 1.0, 2.0)),
               dict(temps=(-0.5, 1.0, 2.0)), dict(temps=(0.5, 0.5, 2.0)), dict(temps=(0.5, 2.0, 1.0)),
               dict(count=0, temps=None), dict(count=0, K=0), dict(batch=0, temps=(1.0, 1.0, 2.0))):
        assert call(**kw) == -1, kw
    assert call(V_=(1 << 20) + 1) == -2


def test_estimate_loss_with_off_never_touches_mmt_eval(monkeypatch, capsys, tmp_path):
    """eval_temperature: off (and an absent key) runs estimate_loss without importing or calling mmt_eval, and prints
    and logs byte for byte the same: a sentinel module that raises on any attribute stands in for it; the model and
    the batcher are stand-ins too."""
    import training_utils as TU

    class Sentinel(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            raise AssertionError(f"mmt_eval.{name} touched with eval_temperature: off")

    monkeypatch.setitem(sys.modules, "mmt_eval", Sentinel("mmt_eval"))

    class Model:
        training = True

        def eval(self):
            pass

        def train(self):
            pass

        def __call__(self, xb, yb):
            return [torch.zeros(2, 4, 3)], [torch.tensor(1.5)]

    params = [[None] * 12]
    params[0][9] = "Close"
    for k, v in dict(m=Model(), num_modalities=1, all_modality_params=params, all_vocabularies=[[0.0, 1.0, 2.0]],
                     get_batch=lambda s, t: ([torch.zeros(2, 4, dtype=torch.int64)], [torch.zeros(2, 4, dtype=torch.int64)]),
                     calculate_evaluation_metrics=lambda *a: ([1], [1], [0.5], [1]),
                     sync_host_state=lambda: None).items():
        monkeypatch.setattr(TU, k, v, raising=False)
    monkeypatch.setattr(TU, "datetime", type("Clock", (), {"now": staticmethod(lambda: __import__("datetime").datetime(2025, 1, 1))}))
    old = CU._config_cache
    try:
        texts, logs = [], []
        for n, extra in enumerate(({}, {"eval_temperature": "off"}, {"eval_temperature": False})):
            CU._config_cache = dict({"block_size": 4, "batch_size": 2, "eval_iters": 2, "device": "cpu",
                                     "output_file_name": f"log{n}.txt", "project_file_path": str(tmp_path) + "/"}, **extra)
            assert TU.estimate_loss() == {"train": 1.5, "val": 1.5}
            texts.append(capsys.readouterr().out)
            logs.append(open(tmp_path / "output" / f"log{n}.txt").read())
        assert texts[0] == texts[1] == texts[2] and logs[0] == logs[1] == logs[2]
        assert "TEMPERATURE" not in texts[0] + logs[0] and not TU.last_temperature_fit
        CU._config_cache["eval_temperature"] = "fit"  # and the switch does reach for it
        with pytest.raises(AssertionError, match="mmt_eval"):
            TU.estimate_loss()
        CU._config_cache["eval_temperature"] = "sometimes"
        with pytest.raises(ValueError, match="eval_temperature"):
            TU.estimate_loss()
    finally:
        CU._config_cache = old
        TU.last_temperature_fit.clear()
