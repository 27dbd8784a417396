"""Host-side checks of the guarded optimizer step and in-place gradient accumulation (no compute calls):
the config keys `grad_clip`, `grad_accum_steps` and `skip_nonfinite_steps`, the AdamW constructor's
arguments, the guard-state size and header layout, the ctypes binding table, and the per-context
accumulation switch of the C ABI (mmt_create needs no device)."""
import ctypes
import os
import re

import pytest
import torch

import config_utils
import mmt_lib as ML
import mmt_optim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def clean_config():
    old = config_utils._config_cache
    yield
    config_utils._config_cache = old


# ------------------------------------------------------------------------------------------------ config
def test_config_keys_default(clean_config, tmp_path, monkeypatch):
    config_utils._config_cache = {"n_embd": 64}  # an injected dict without the keys gets the defaults
    assert config_utils._get_grad_clip() is None
    assert config_utils._get_grad_accum_steps() == 1
    assert config_utils._get_skip_nonfinite_steps() is False
    tp = config_utils._DEFAULTS["training_parameters"]
    assert tp["grad_clip"] is None and tp["grad_accum_steps"] == 1 and tp["skip_nonfinite_steps"] is False
    monkeypatch.chdir(tmp_path)
    cfg = config_utils.load_system_config()
    assert cfg["grad_clip"] is None and cfg["grad_accum_steps"] == 1 and cfg["skip_nonfinite_steps"] is False
    (tmp_path / "config.yaml").write_text(
        "training_parameters:\n  grad_clip: 0.5\n  grad_accum_steps: 4\n  skip_nonfinite_steps: true\n")
    config_utils._config_cache = config_utils.load_system_config()
    assert config_utils._get_grad_clip() == 0.5
    assert config_utils._get_grad_accum_steps() == 4
    assert config_utils._get_skip_nonfinite_steps() is True
    (tmp_path / "config.yaml").write_text("training_parameters:\n  grad_clip: null\n")
    config_utils._config_cache = config_utils.load_system_config()
    assert config_utils._get_grad_clip() is None


@pytest.mark.parametrize("value,want", [(1, 1.0), (0.25, 0.25), (1e9, 1e9), (None, None)])
def test_grad_clip_values(clean_config, value, want):
    config_utils._config_cache = {"grad_clip": value}
    got = config_utils._get_grad_clip()
    assert got == want and (got is None or isinstance(got, float))


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), "1.0", True, [1.0]])
def test_grad_clip_bad_values(clean_config, bad):
    config_utils._config_cache = {"grad_clip": bad}
    with pytest.raises(ValueError, match="grad_clip"):
        config_utils._get_grad_clip()


@pytest.mark.parametrize("bad", [0, -2, 1.5, 2.0, "2", None, True])
def test_grad_accum_steps_bad_values(clean_config, bad):
    config_utils._config_cache = {"grad_accum_steps": bad}
    with pytest.raises(ValueError, match="grad_accum_steps"):
        config_utils._get_grad_accum_steps()


@pytest.mark.parametrize("value,want", [(True, True), (False, False), (1, True), (0, False)])
def test_skip_nonfinite_steps_values(clean_config, value, want):
    config_utils._config_cache = {"skip_nonfinite_steps": value}
    assert config_utils._get_skip_nonfinite_steps() is want


@pytest.mark.parametrize("bad", [2, "yes", None, 0.5])
def test_skip_nonfinite_steps_bad_values(clean_config, bad):
    config_utils._config_cache = {"skip_nonfinite_steps": bad}
    with pytest.raises(ValueError, match="skip_nonfinite_steps"):
        config_utils._get_skip_nonfinite_steps()


# ------------------------------------------------------------------------------------------------ optimizer
def _params():
    return [torch.nn.Parameter(torch.zeros(8))]


def test_adamw_defaults_are_the_plain_optimizer():
    opt = mmt_optim.AdamW(_params(), lr=1e-3)
    assert opt.guarded is False and opt.max_grad_norm is None and opt.skip_nonfinite is False
    assert opt.last_grad_norm is None and opt.counters() == (0, 0, 0)
    assert set(opt.state_dict()) == {"state", "param_groups"}


def test_adamw_guard_arguments():
    assert mmt_optim.AdamW(_params(), max_grad_norm=1.0).guarded is True
    assert mmt_optim.AdamW(_params(), max_grad_norm=2).max_grad_norm == 2.0
    assert mmt_optim.AdamW(_params(), max_grad_norm=float("inf")).guarded is True  # the norm alone, never clips
    assert mmt_optim.AdamW(_params(), skip_nonfinite=True).guarded is True
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            mmt_optim.AdamW(_params(), max_grad_norm=bad)
    for bad in ("1", True, [1.0]):
        with pytest.raises(TypeError, match="max_grad_norm"):
            mmt_optim.AdamW(_params(), max_grad_norm=bad)
    for bad in (1, 0, None, "true"):
        with pytest.raises(TypeError, match="skip_nonfinite"):
            mmt_optim.AdamW(_params(), skip_nonfinite=bad)
    with pytest.raises(ValueError, match="learning rate"):
        mmt_optim.AdamW(_params(), lr=-1.0, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="betas"):  # one device step count, one pair of bias corrections
        mmt_optim.AdamW([{"params": _params()}, {"params": _params(), "betas": (0.8, 0.9)}], max_grad_norm=1.0)


def test_betas_are_checked_again_at_every_guarded_step():
    """Groups can be edited or added after construction; the check runs before anything is launched."""
    opt = mmt_optim.AdamW([{"params": _params()}, {"params": _params()}], max_grad_norm=1.0)
    opt.step()  # no gradients: nothing to do
    opt.param_groups[1]["betas"] = (0.8, 0.9)
    with pytest.raises(ValueError, match="betas"):
        opt.step()
    opt.param_groups[1]["betas"] = opt.param_groups[0]["betas"]
    opt.add_param_group({"params": _params(), "betas": (0.5, 0.9)})
    with pytest.raises(ValueError, match="betas"):
        opt.step()
    plain = mmt_optim.AdamW([{"params": _params()}, {"params": _params(), "betas": (0.8, 0.9)}])
    plain.step()  # the plain optimizer keeps a step count per parameter: any betas per group


def test_guarded_state_dict_step_is_an_int_and_loads_back():
    p = _params()
    opt = mmt_optim.AdamW(p, max_grad_norm=1.0)
    sd = {"state": {0: {"step": 7, "exp_avg": torch.ones(8), "exp_avg_sq": torch.ones(8)}},
          "param_groups": opt.state_dict()["param_groups"]}
    opt.load_state_dict(sd)
    assert opt.counters() == (7, 0, 0)  # kept for the guard state the first step allocates
    out = opt.state_dict()
    assert out["state"][0]["step"] == 7 and isinstance(out["state"][0]["step"], int)


# ------------------------------------------------------------------------------------------------ C ABI
def test_guard_state_size_and_header_layout():
    n = ML.lib().mmt_guard_state_bytes()
    assert n > 0
    assert ctypes.sizeof(ML.MmtGuardHeader) == 64
    assert n == 64 + 8 * ML.GUARD_SLOTS
    H = ML.MmtGuardHeader
    assert (H.norm.offset, H.coef.offset, H.ok.offset) == (0, 4, 8)
    assert (H.applied_steps.offset, H.skipped_steps.offset, H.clipped_steps.offset) == (16, 24, 32)
    assert (H.bias_correction1.offset, H.bias_correction2_sqrt.offset) == (40, 44)
    src = open(os.path.join(REPO, "include", "mmt.h")).read()
    assert re.search(r"#define\s+MMT_GUARD_SLOTS\s+%d\b" % ML.GUARD_SLOTS, src)
    body = re.search(r"struct mmt_guard_header \{(.*?)\};", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert names == [f[0] for f in H._fields_]


def test_binding_table():
    want = {
        "mmt_guard_state_bytes": (ML.c_i64, []),
        "mmt_grad_sqsum": (ML.c_i32, [ML.c_vp, ML.c_vp, ML.c_i64, ML.c_i32, ML.c_vp]),
        "mmt_guard_finalize": (ML.c_i32, [ML.c_vp, ML.c_f32, ML.c_i32, ML.c_f32, ML.c_f32, ML.c_vp]),
        "mmt_adamw_step_guarded": (ML.c_i32, [ML.c_vp] * 6 + [ML.c_i64] + [ML.c_f32] * 5 + [ML.c_vp]),
        "mmt_set_grad_accumulate": (ML.c_i32, [ML.c_vp, ML.c_i32]),
        "mmt_get_grad_accumulate": (ML.c_i32, [ML.c_vp]),
    }
    L = ML.lib()
    for name, sig in want.items():
        assert ML._SIGS[name] == sig, name
        assert name in ML.EXPORTED and hasattr(L, name), name
    # the plain step's entry point is as it was
    assert ML._SIGS["mmt_adamw_step"] == (ML.c_i32, [ML.c_vp] * 6 + [ML.c_i64, ML.c_i64] + [ML.c_f32] * 5)


def test_bad_arguments_are_refused_before_any_launch():
    """Null guard, n < 0 and misaligned pointers return MMT_ERR_INVALID on the host (no device needed:
    nothing is launched; the addresses are never dereferenced)."""
    L = ML.lib()
    a = ctypes.c_void_p(0x10000)  # a 16-byte aligned address
    odd = ctypes.c_void_p(0x10004)
    assert L.mmt_grad_sqsum(None, a, 4, 0, None) == -1
    assert L.mmt_grad_sqsum(None, a, -1, 0, a) == -1
    assert L.mmt_grad_sqsum(None, odd, 4, 0, a) == -1
    assert L.mmt_grad_sqsum(None, a, 4, 0, odd) == -1
    assert L.mmt_guard_finalize(None, 1.0, 0, 0.9, 0.999, None) == -1
    assert L.mmt_guard_finalize(None, 1.0, 0, 0.9, 0.999, odd) == -1
    args = (4, 1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert L.mmt_adamw_step_guarded(None, None, a, a, a, a, *args, None) == -1
    assert L.mmt_adamw_step_guarded(None, None, a, a, a, a, -1, *args[1:], a) == -1
    for k in range(4):
        ptrs = [a] * 4
        ptrs[k] = odd
        assert L.mmt_adamw_step_guarded(None, None, *ptrs, *args, a) == -1, k
    assert L.mmt_adamw_step_guarded(None, None, a, a, a, a, *args, odd) == -1


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


def test_grad_accumulate_switch_is_per_context_and_off_by_default():
    L = ML.lib()
    a, b = _ctx(), _ctx()
    try:
        assert L.mmt_get_grad_accumulate(a) == 0 and L.mmt_get_grad_accumulate(b) == 0
        assert L.mmt_set_grad_accumulate(a, 1) == 0
        assert L.mmt_get_grad_accumulate(a) == 1
        assert L.mmt_get_grad_accumulate(b) == 0  # not process-global
        assert L.mmt_set_grad_accumulate(a, 5) == 0  # any non-zero value is "on"
        assert L.mmt_get_grad_accumulate(a) == 1
        assert L.mmt_set_grad_accumulate(a, 0) == 0
        assert L.mmt_get_grad_accumulate(a) == 0
        assert L.mmt_set_grad_accumulate(None, 1) == -1  # MMT_ERR_INVALID
        assert L.mmt_get_grad_accumulate(None) == 0
    finally:
        L.mmt_destroy(a)
        L.mmt_destroy(b)
