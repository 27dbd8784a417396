"""Configuration accessors — same names and cache hook as the reference's config_utils.py:8-69.

`_config_cache` is the injection point (tests and the bench set it directly, as the reference's
own model import does). When empty it is filled from `config.yaml` in the current directory
with the defaults of the reference's SystemConfig.from_dict (config_manager.py:110-147) and the
`device: auto` resolution of compatibility_layer.py:124-126.
"""
import os

_config_cache = None

_DEFAULTS = {
    "project_settings": {"project_file_path": "", "output_file_name": "training_log.txt",
                         "model_file_name": "model.pth", "create_new_model": 1, "save_model": 1, "device": "cpu"},
    "data_splitting": {"validation_size": 0.1, "num_validation_files": 0},
    "training_parameters": {"batch_size": 32, "block_size": 64, "max_iters": 5000, "eval_interval": 500,
                            "eval_iters": 40, "learning_rate": 3e-4,
                            # build-only keys (the reference ignores unknown keys): the guarded optimizer step
                            # (mmt_optim.AdamW max_grad_norm / skip_nonfinite) and in-place gradient accumulation
                            "grad_clip": None, "grad_accum_steps": 1, "skip_nonfinite_steps": False,
                            # build-only key: per-tensor gradient statistics (mmt_stats.TensorStats)
                            "grad_stats": "off",
                            # build-only keys: evaluation at every position (mmt_eval.PositionMetrics in estimate_loss)
                            "eval_positions": "last", "eval_positions_from": 0,
                            # build-only keys: scored rollouts (mmt_eval.RolloutMetrics in estimate_loss); 0 paths: off
                            "eval_rollout_paths": 0, "eval_rollout_steps": 16, "eval_rollout_seed": 0,
                            # build-only key: fit each head's temperature (mmt_eval.TemperatureFit in estimate_loss)
                            "eval_temperature": "off",
                            # build-only keys: the training objective (MultimodalTransformer.set_loss, mmt_loss)
                            "label_smoothing": 0.0, "loss_class_weights": None, "loss_class_weight_power": 1.0,
                            "loss_positions_from": 0},
    "model_architecture": {"n_embd": 384, "n_head": 6, "n_layer": 6, "dropout": 0.2,
                           "fixed_values": [-0.5, -0.2, -0.1, 0, 0.1, 0.2, 0.5],
                           # build-only key (the reference ignores unknown keys): "bf16" | "fp8"
                           "precision": "bf16",
                           # build-only key: bitwise-reproducible gradients (mmt_set_deterministic)
                           "deterministic": False},
}


def load_system_config(path="config.yaml"):
    """Flattened system configuration dict from a reference-format config.yaml."""
    import yaml
    raw = {}
    if os.path.exists(path):
        with open(path, "r", encoding="utf-8") as f:
            raw = yaml.safe_load(f) or {}
    flat = {}
    for section, defaults in _DEFAULTS.items():
        sec = raw.get(section, {}) or {}
        for k, v in defaults.items():
            flat[k] = sec.get(k, v)
    flat["create_new_model"] = int(bool(flat["create_new_model"]))
    flat["save_model"] = int(bool(flat["save_model"]))
    if flat["device"] == "auto":
        import torch
        flat["device"] = "cuda" if torch.cuda.is_available() else "cpu"
    return flat


def _get_config():
    global _config_cache
    if _config_cache is None:
        _config_cache = load_system_config()
    return _config_cache


def _get_device():
    return _get_config()["device"]


def _get_block_size():
    return _get_config()["block_size"]


def _get_batch_size():
    return _get_config()["batch_size"]


def _get_eval_iters():
    return _get_config()["eval_iters"]


def _get_n_embd():
    return _get_config()["n_embd"]


def _get_n_head():
    return _get_config()["n_head"]


def _get_n_layer():
    return _get_config()["n_layer"]


def _get_dropout():
    return _get_config()["dropout"]


def _get_fixed_values():
    return _get_config()["fixed_values"]


def _get_precision():
    """Build-only knob (no reference counterpart): "bf16" (default) or "fp8" (MX-fp8 forward
    GEMMs, BASELINE configs[4]); the MMT_PRECISION environment variable overrides the config."""
    p = os.environ.get("MMT_PRECISION") or _get_config().get("precision", "bf16")
    if p not in ("bf16", "fp8"):
        raise ValueError(f"precision must be 'bf16' or 'fp8', got {p!r}")
    return p


def _get_deterministic():
    """Build-only knob (the counterpart of torch.use_deterministic_algorithms): True makes every
    backward write bit-identical gradients for identical inputs (include/mmt.h, mmt_set_deterministic).
    Default False; the MMT_DETERMINISTIC environment variable (0/1, false/true, off/on, no/yes)
    overrides the config."""
    env = os.environ.get("MMT_DETERMINISTIC")
    v = env if env else _get_config().get("deterministic", False)
    if isinstance(v, bool):
        return v
    if isinstance(v, int) and v in (0, 1):
        return bool(v)
    if isinstance(v, str):
        t = v.strip().lower()
        if t in ("1", "true", "on", "yes"):
            return True
        if t in ("0", "false", "off", "no"):
            return False
    raise ValueError(f"deterministic must be a boolean (0/1, false/true, off/on, no/yes), got {v!r}")


def _get_grad_clip():
    """Build-only knob: the global gradient-norm bound of the guarded optimizer step (torch's
    clip_grad_norm_ formula, on the device; mmt_optim.AdamW max_grad_norm). A positive float, or None
    (default, also when the key is absent): no clipping."""
    v = _get_config().get("grad_clip", None)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v <= 0:
        raise ValueError(f"grad_clip must be a positive number or null, got {v!r}")
    return float(v)


def _get_grad_accum_steps():
    """Build-only knob: micro-batches per optimizer step (in-place gradient accumulation,
    MultimodalTransformer.set_grad_accumulation). An integer >= 1; default 1 (also when the key is absent)."""
    v = _get_config().get("grad_accum_steps", 1)
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"grad_accum_steps must be an integer >= 1, got {v!r}")
    return v


def _get_skip_nonfinite_steps():
    """Build-only knob: True skips, on the device, an optimizer step whose gradient norm is NaN / Inf
    (mmt_optim.AdamW skip_nonfinite). Default False (also when the key is absent)."""
    v = _get_config().get("skip_nonfinite_steps", False)
    if isinstance(v, bool):
        return v
    if isinstance(v, int) and v in (0, 1):
        return bool(v)
    raise ValueError(f"skip_nonfinite_steps must be a boolean, got {v!r}")


def _get_grad_stats():
    """Build-only knob: per-tensor gradient statistics on the device (mmt_stats.TensorStats handed to
    mmt_optim.AdamW). "off" (default, also when the key is absent), "skipped" (the first skipped step since the
    last evaluation is kept; main.run turns skip_nonfinite_steps on with it) or "every" (the latest step)."""
    v = _get_config().get("grad_stats", "off")
    if v is False:  # YAML reads a bare `off` as a boolean
        return "off"
    if not isinstance(v, str) or v not in ("off", "skipped", "every"):
        raise ValueError(f"grad_stats must be 'off', 'skipped' or 'every', got {v!r}")
    return v


def _get_eval_positions():
    """Build-only knob: which positions estimate_loss evaluates. "last" (default, also when the key is absent): the
    reference's directional metric on the last position of every window, nothing else. "all": in addition the
    position metrics of mmt_eval.PositionMetrics over every position from eval_positions_from on."""
    v = _get_config().get("eval_positions", "last")
    if not isinstance(v, str) or v not in ("last", "all"):
        raise ValueError(f"eval_positions must be 'last' or 'all', got {v!r}")
    return v


def _get_eval_positions_from():
    """Build-only knob: the first position (t_begin) of the position metrics, an integer in 0..block_size; default 0
    (also when the key is absent). Read only with eval_positions: all."""
    v = _get_config().get("eval_positions_from", 0)
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v > _get_block_size():
        raise ValueError(f"eval_positions_from must be an integer in 0..block_size, got {v!r}")
    return v


def _get_eval_temperature():
    """Build-only knob: "off" (default, also when the key is absent): nothing runs. "fit": estimate_loss also hands
    every iteration's logits to a mmt_eval.TemperatureFit, prints the fitted temperature of each scored head and,
    after the val state, stores it in the model for generate(temperature="calibrated"). Independent of
    eval_positions (it only shares eval_positions_from)."""
    v = _get_config().get("eval_temperature", "off")
    if v is False:  # YAML reads a bare `off` as a boolean
        return "off"
    if not isinstance(v, str) or v not in ("off", "fit"):
        raise ValueError(f"eval_temperature must be 'off' or 'fit', got {v!r}")
    return v


def _get_eval_rollout_paths():
    """Build-only knob: how many paths estimate_loss rolls from the head of every evaluation window to score the
    horizon forecast against the window's own tail (mmt_eval.RolloutMetrics). 0 (default, also when the key is
    absent): off, nothing runs. At most 4096 (the paths of a prompt are sorted on chip)."""
    v = _get_config().get("eval_rollout_paths", 0)
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v > 4096:
        raise ValueError(f"eval_rollout_paths must be an integer in 0..4096, got {v!r}")
    return v


def _get_eval_rollout_steps():
    """Build-only knob: H, the steps of a scored rollout: the last H tokens of a window are the realised series, the
    first block_size - H the prompt. An integer with 1 <= H < block_size; default 16. Read only with
    eval_rollout_paths > 0."""
    v = _get_config().get("eval_rollout_steps", 16)
    if isinstance(v, bool) or not isinstance(v, int) or v < 1 or v >= _get_block_size():
        raise ValueError(f"eval_rollout_steps must be an integer with 1 <= H < block_size, got {v!r}")
    return v


def _get_eval_rollout_seed():
    """Build-only knob: the seed the scored rollouts derive theirs from, an integer >= 0; default 0. Read only with
    eval_rollout_paths > 0."""
    v = _get_config().get("eval_rollout_seed", 0)
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"eval_rollout_seed must be an integer >= 0, got {v!r}")
    return v


def _get_label_smoothing(num_modalities=None):
    """Build-only knob: the label smoothing of the training objective (MultimodalTransformer.set_loss), a number in
    [0, 1) for every modality or a list of one per modality (its length is checked when num_modalities is given).
    Default 0.0 (also when the key is absent): the plain cross-entropy."""
    v = _get_config().get("label_smoothing", 0.0)

    def one(e):
        if isinstance(e, bool) or not isinstance(e, (int, float)) or e != e or e < 0 or e >= 1:
            raise ValueError(f"label_smoothing must be a number in [0, 1) or a list of them, got {v!r}")
        return float(e)

    if isinstance(v, (list, tuple)):
        if not v or (num_modalities is not None and len(v) != num_modalities):
            raise ValueError(f"label_smoothing as a list needs one value per modality, got {v!r}")
        return [one(e) for e in v]
    return one(v)


def _get_loss_class_weights():
    """Build-only knob: the class weights of the training objective. None (default, also when the key is absent):
    none. "balanced": mmt_loss.balanced_class_weights over the training tokens of every modality."""
    v = _get_config().get("loss_class_weights", None)
    if v is None:
        return None
    if not isinstance(v, str) or v != "balanced":
        raise ValueError(f"loss_class_weights must be null or 'balanced', got {v!r}")
    return v


def _get_loss_class_weight_power():
    """Build-only knob: alpha of the balanced class weights, w_c ~ (n / count_c) ** alpha: a number in [0, 1],
    default 1 (also when the key is absent). Read only with loss_class_weights: balanced."""
    v = _get_config().get("loss_class_weight_power", 1.0)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v < 0 or v > 1:
        raise ValueError(f"loss_class_weight_power must be a number in [0, 1], got {v!r}")
    return float(v)


def _get_loss_positions_from():
    """Build-only knob: the first position of a window that counts in the training loss, an integer in
    0..block_size - 1; the positions below it get weight 0, the rest 1. Default 0 (also when the key is absent):
    every position."""
    v = _get_config().get("loss_positions_from", 0)
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v >= _get_block_size():
        raise ValueError(f"loss_positions_from must be an integer in 0..block_size - 1, got {v!r}")
    return v
