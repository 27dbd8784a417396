"""Host-side checks of the deterministic training mode (no compute calls): the `deterministic` config
key and its MMT_DETERMINISTIC override, the ctypes binding table, and the per-context switch of the
C ABI (mmt_create needs no device)."""
import ctypes
import os
import re

import pytest

import config_utils
import mmt_lib as ML

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def clean_config(monkeypatch):
    monkeypatch.delenv("MMT_DETERMINISTIC", raising=False)
    old = config_utils._config_cache
    yield
    config_utils._config_cache = old


def test_config_key_defaults_to_false(clean_config, tmp_path, monkeypatch):
    config_utils._config_cache = {"n_embd": 64}
    assert config_utils._get_deterministic() is False
    # the key sits next to `precision` in the model_architecture section of config.yaml
    assert config_utils._DEFAULTS["model_architecture"]["deterministic"] is False
    assert "precision" in config_utils._DEFAULTS["model_architecture"]
    monkeypatch.chdir(tmp_path)
    assert config_utils.load_system_config()["deterministic"] is False
    (tmp_path / "config.yaml").write_text("model_architecture:\n  deterministic: true\n")
    assert config_utils.load_system_config()["deterministic"] is True


@pytest.mark.parametrize("value,want", [(True, True), (False, False), (1, True), (0, False), ("true", True),
                                        ("off", False)])
def test_config_key_values(clean_config, value, want):
    config_utils._config_cache = {"deterministic": value}
    assert config_utils._get_deterministic() is want


@pytest.mark.parametrize("env,want", [("1", True), ("0", False), ("true", True), ("False", False), ("on", True),
                                      ("no", False)])
def test_environment_overrides_config(clean_config, monkeypatch, env, want):
    config_utils._config_cache = {"deterministic": not want}
    monkeypatch.setenv("MMT_DETERMINISTIC", env)
    assert config_utils._get_deterministic() is want


def test_empty_environment_value_keeps_the_config(clean_config, monkeypatch):
    config_utils._config_cache = {"deterministic": True}
    monkeypatch.setenv("MMT_DETERMINISTIC", "")
    assert config_utils._get_deterministic() is True


@pytest.mark.parametrize("bad", ["maybe", "2", 2, -1, 0.5, None, [1]])
def test_bad_values_are_rejected(clean_config, monkeypatch, bad):
    config_utils._config_cache = {"deterministic": bad}
    with pytest.raises(ValueError, match="deterministic"):
        config_utils._get_deterministic()
    if isinstance(bad, str):
        config_utils._config_cache = {"deterministic": False}
        monkeypatch.setenv("MMT_DETERMINISTIC", bad)
        with pytest.raises(ValueError, match="deterministic"):
            config_utils._get_deterministic()


def test_binding_table():
    for name in ("mmt_set_deterministic", "mmt_get_deterministic", "mmt_op_ordered_sum"):
        assert name in ML._SIGS, name
        assert name in ML.EXPORTED
    assert ML._SIGS["mmt_set_deterministic"] == (ML.c_i32, [ML.c_vp, ML.c_i32])
    assert ML._SIGS["mmt_get_deterministic"] == (ML.c_i32, [ML.c_vp])
    assert ML._SIGS["mmt_op_ordered_sum"] == (ML.c_i32, [ML.c_vp, ML.c_i32, ML.c_i32, ML.c_vp, ML.c_i64, ML.c_vp])
    # and the header declares them with those argument lists
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mmt.h")).read(), flags=re.S)
    assert re.search(r"int\s+mmt_set_deterministic\(mmt_ctx\*\s*ctx,\s*int32_t\s+on\)", src)
    assert re.search(r"int32_t\s+mmt_get_deterministic\(const\s+mmt_ctx\*\s*ctx\)", src)
    L = ML.lib()
    for name in ("mmt_set_deterministic", "mmt_get_deterministic", "mmt_op_ordered_sum"):
        assert hasattr(L, name), name


def _ctx(C=64, H=4, L_=1, T=32, V=(11, 7), cross=(True, False)):
    cfg = ML.MmtConfig()
    cfg.num_modalities = len(V)
    cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.block_size = C, H, L_, T
    for i, v in enumerate(V):
        cfg.vocab_sizes[i] = v
        cfg.cross_attention[i] = int(cross[i])
    ctx = ML.lib().mmt_create(ctypes.byref(cfg))
    assert ctx, ML.lib().mmt_create_error()
    return ctypes.c_void_p(ctx)


def test_switch_is_per_context_and_off_by_default():
    L = ML.lib()
    a, b = _ctx(), _ctx()
    try:
        assert L.mmt_get_deterministic(a) == 0 and L.mmt_get_deterministic(b) == 0
        assert L.mmt_set_deterministic(a, 1) == 0
        assert L.mmt_get_deterministic(a) == 1
        assert L.mmt_get_deterministic(b) == 0  # not process-global
        assert L.mmt_set_deterministic(a, 7) == 0  # any non-zero value is "on"
        assert L.mmt_get_deterministic(a) == 1
        assert L.mmt_set_deterministic(a, 0) == 0
        assert L.mmt_get_deterministic(a) == 0
        assert L.mmt_set_deterministic(None, 1) == -1  # MMT_ERR_INVALID
        assert L.mmt_get_deterministic(None) == 0
    finally:
        L.mmt_destroy(a)
        L.mmt_destroy(b)


@pytest.mark.parametrize("shape", [dict(), dict(C=256, H=8, L_=2, T=256, V=(900, 13, 144, 5), cross=(1, 1, 0, 0)),
                                   dict(C=128, H=2, L_=1, T=64, V=(5,), cross=(0,))])
def test_workspace_bytes_do_not_depend_on_the_switch(shape):
    """The partial-sum scratch is part of every plan, so sizes cached by the Python side stay valid
    when the mode is toggled."""
    L = ML.lib()
    ctx = _ctx(**shape)
    try:
        off = [L.mmt_workspace_bytes(ctx, B) for B in (1, 3, 8)]
        L.mmt_set_deterministic(ctx, 1)
        on = [L.mmt_workspace_bytes(ctx, B) for B in (1, 3, 8)]
        assert on == off and all(x > 0 for x in on)
    finally:
        L.mmt_destroy(ctx)
