"""mmt_loss.py — host side of the training objective (include/mmt.h, mmt_set_loss): label smoothing, class
weights and position weights of the cross-entropy.

    row_r = (1 - eps) w[t_r] (lse_r - x[r, t_r]) + eps / V * sum_c w[c] (lse_r - x[r, c])
    loss  = sum_r u[r mod T] row_r / sum_r u[r mod T] w[t_r]

Nothing here touches the device: `normalize_spec` turns the arguments of MultimodalTransformer.set_loss into one
checked (eps, class weights, position weights) triple per modality, `balanced_class_weights` counts the training
tokens once at start-up, `spec_from_config` reads the build-only config keys for main.run.
"""
import numpy as np
import torch


def _per_modality(value, M, what):
    """value for every modality, or a {modality: value} dict (absent modalities: None)."""
    if isinstance(value, dict):
        for k in value:
            if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < M:
                raise ValueError(f"{what}: modality {k!r} is not an integer in 0..{M - 1}")
        return [value.get(i) for i in range(M)]
    return [value] * M


def _weights(value, n, what):
    """None, or a checked fp32 host vector [n]: finite, >= 0, not all zero."""
    if value is None:
        return None
    w = torch.as_tensor(value).detach().to("cpu")
    if w.dim() != 1 or w.numel() != n:
        raise ValueError(f"{what} must have shape [{n}], got {list(w.shape)}")
    if w.dtype == torch.bool or w.is_complex():
        raise ValueError(f"{what} must be real numbers")
    w = w.to(torch.float32).contiguous()
    if not bool(torch.isfinite(w).all()):
        raise ValueError(f"{what} must be finite")
    if bool((w < 0).any()):
        raise ValueError(f"{what} must be >= 0")
    if not bool((w > 0).any()):
        raise ValueError(f"{what} must not be all zero")
    return w.clone()


def _eps(value, what):
    if value is None:
        return 0.0
    if isinstance(value, torch.Tensor):
        if value.numel() != 1:
            raise ValueError(f"{what} must be a scalar, got shape {list(value.shape)}")
        value = value.item()
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"{what} must be a number in [0, 1), got {value!r}")
    e = float(value)
    if not (0.0 <= e < 1.0):  # also refuses NaN
        raise ValueError(f"{what} must be in [0, 1), got {value!r}")
    if np.float32(e) >= 1.0:
        raise ValueError(f"{what} must be below 1 in fp32, got {value!r}")
    return e


def normalize_spec(label_smoothing, class_weights, position_weights, vocab_sizes, block_size):
    """[(eps, class weights [V_i] or None, position weights [block_size] or None)] * M, checked on the host; None
    when every entry is the plain loss. Each argument is one value for all modalities or a {modality: value} dict;
    one class-weight tensor for all modalities needs equal vocabulary sizes (its shape is checked per modality)."""
    M = len(vocab_sizes)
    eps = [_eps(e, f"label_smoothing[{i}]") for i, e in enumerate(_per_modality(label_smoothing, M, "label_smoothing"))]
    cw = [_weights(w, vocab_sizes[i], f"class_weights[{i}]")
          for i, w in enumerate(_per_modality(class_weights, M, "class_weights"))]
    pw = [_weights(u, block_size, f"position_weights[{i}]")
          for i, u in enumerate(_per_modality(position_weights, M, "position_weights"))]
    if all(e == 0.0 for e in eps) and all(w is None for w in cw) and all(u is None for u in pw):
        return None
    return list(zip(eps, cw, pw))


def balanced_class_weights(tokens, V, power=1.0):
    """Class weights against the imbalance of one modality's training tokens, fp32 [V]: w_c ~ (n / count_c) ** power
    for the classes that occur and 0 for those that do not, scaled so that sum_c count_c w_c = n: the weighted
    loss keeps the plain loss's scale and its denominator stays near the row count. power = 0: all ones on the
    classes that occur."""
    if isinstance(power, bool) or not isinstance(power, (int, float)) or not (0.0 <= power <= 1.0):
        raise ValueError(f"power must be a number in [0, 1], got {power!r}")
    t = np.asarray(tokens.cpu() if isinstance(tokens, torch.Tensor) else tokens).reshape(-1)
    if t.size == 0:
        raise ValueError("balanced_class_weights: no tokens")
    if not np.issubdtype(t.dtype, np.integer):
        raise ValueError("balanced_class_weights: tokens must be integers")
    if int(t.min()) < 0 or int(t.max()) >= V:
        raise ValueError(f"balanced_class_weights: tokens outside 0..{V - 1}")
    count = np.bincount(t.astype(np.int64), minlength=V).astype(np.float64)
    n = float(t.size)
    w = np.zeros(V, dtype=np.float64)
    seen = count > 0
    w[seen] = (n / count[seen]) ** float(power)
    w *= n / float((count * w).sum())
    return torch.from_numpy(w).to(torch.float32)


def spec_from_config(train_tokens, vocab_sizes, block_size):
    """(set_loss keyword arguments, the LOSS OBJECTIVE line) from the build-only config keys label_smoothing,
    loss_class_weights, loss_class_weight_power and loss_positions_from; (None, None) when all are off."""
    import config_utils as CU
    M = len(vocab_sizes)
    eps = CU._get_label_smoothing(M)
    mode = CU._get_loss_class_weights()
    t0 = CU._get_loss_positions_from()
    eps_list = eps if isinstance(eps, list) else [eps] * M
    if all(e == 0.0 for e in eps_list) and mode is None and t0 == 0:
        return None, None
    kw = {"label_smoothing": {i: e for i, e in enumerate(eps_list)}, "class_weights": None, "position_weights": None}
    parts = ["label_smoothing " + (f"{eps:g}" if not isinstance(eps, list) else "[" + ", ".join(f"{e:g}" for e in eps) + "]")]
    if mode == "balanced":
        power = CU._get_loss_class_weight_power()
        kw["class_weights"] = {i: balanced_class_weights(train_tokens[i], vocab_sizes[i], power) for i in range(M)}
        spans = []
        for i in range(M):
            w = kw["class_weights"][i]
            pos = w[w > 0]
            spans.append(f"{float(pos.min()):.3g}..{float(pos.max()):.3g}")
        parts.append(f"class weights balanced (power {power:g}; per modality {', '.join(spans)})")
    else:
        parts.append("class weights none")
    if t0 > 0:
        u = torch.ones(block_size, dtype=torch.float32)
        u[:t0] = 0.0
        kw["position_weights"] = u
    parts.append(f"positions from {t0} of {block_size}")
    return kw, "LOSS OBJECTIVE: " + " | ".join(parts)
