"""mmt_rollout.py — the rollouts behind `MultimodalTransformer.generate` (model.py): the host-side checks of its
keywords, the one reference loop and the one device loop.

A device rollout is described by a JointPlan (which modality is GENERATED, GIVEN or HELD, the checked shape, the
evidence / forecast / horizon settings). `rollout` runs it: per new token it asks a logits source for the [rows, V_i]
views of the step and runs the stages on them, in this order: sample (mmt_sample_multi), score the given tokens
(evidence, mmt_score_multi), forecast (mmt_forecast_multi), then the resampling point. There are two sources and they
are all that differs between the paths: CachedSource (mmt_decode_step while the KV cache holds the position before,
else the re-forward over the cropped buffers) and FanoutSource (one prefill over the prompts, then
mmt_decode_fanout_step over the samples' rows; RollingSource carries it past the block: a forward over the prompts'
shared rows and one mmt_rolling_step over each path's own). The int form of generate is a plan of one generated modality keyed by
the raw seed (`rollout_int`). `reference_loop` is the reference's per-token loop with the choice of the next token
passed in: torch.multinomial / sample_fn for the default path, mmt_sample for device calls with prompts of unequal
lengths."""
import numbers

import torch

import mmt_lib as ML
import mmt_sample as MS

NO_GPU = ("MultimodalTransformer (libmmt_hip) runs only on a ROCm GPU: call .to('cuda') "
          "(there is no CPU path)")


def check_num_samples(num_samples):
    """generate's num_samples: an integer >= 1 (a bool is none)."""
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
        raise ValueError(f"generate: num_samples must be an integer >= 1 or None, got {num_samples!r}")
    return num_samples


CALIBRATED = "calibrated"


def check_calibrated_temperatures(mapping, num_modalities):
    """set_calibrated_temperatures' argument as a fresh {modality: float}: None clears ({}); otherwise a dict whose
    keys are ints 0..M - 1 and whose values are finite numbers > 0."""
    if mapping is None:
        return {}
    if not isinstance(mapping, dict):
        raise ValueError("set_calibrated_temperatures: pass {modality: temperature} or None")
    out = {}
    for i, tau in mapping.items():
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < num_modalities:
            raise ValueError(f"set_calibrated_temperatures: {i!r} is no modality; modalities are the ints "
                             f"0..{num_modalities - 1}")
        if isinstance(tau, bool) or not isinstance(tau, numbers.Real) or not 0.0 < float(tau) < float("inf"):
            raise ValueError(f"set_calibrated_temperatures: the temperature of modality {i} must be a finite number "
                             f"> 0, got {tau!r}")
        out[i] = float(tau)
    return out


def resolve_calibrated(temperature, stored, modality_to_generate, num_modalities):
    """generate's temperature="calibrated" as the numbers it stands for, from `stored` ({modality: tau}, what
    set_calibrated_temperatures holds): the stored tau in the int form, {modality: tau} over the generated modalities
    in the list form. ValueError names the first generated modality without a stored value. Any other temperature,
    and a modality_to_generate that plan_joint will refuse anyway, pass through unchanged."""
    if not (isinstance(temperature, str) and temperature == CALIBRATED):
        return temperature
    g = modality_to_generate
    if isinstance(g, bool):
        return temperature
    if isinstance(g, int):
        gen, as_int = [g], True
    elif isinstance(g, str):
        if g != "all":
            return temperature
        gen, as_int = list(range(num_modalities)), False
    else:
        try:
            gen, as_int = list(g), False
        except TypeError:
            return temperature
        if any(isinstance(i, bool) or not isinstance(i, int) for i in gen):
            return temperature
    for i in gen:
        if i not in stored:
            raise ValueError(f"generate: temperature=\"calibrated\" but modality {i} has no calibrated temperature "
                             "(estimate_loss with eval_temperature: fit, or set_calibrated_temperatures, stores one)")
    return stored[gen[0]] if as_int else {i: stored[i] for i in gen}


def tile_prompts(idx_list, num_samples):
    """The row order of generate(num_samples=S): row b*S + s of every returned tensor is sample s of prompt b,
    i.e. each prompt repeated S times in place."""
    return [p.repeat_interleave(num_samples, 0) for p in idx_list]


GENERATED, GIVEN, HELD = "generated", "given", "held"


class JointPlan:
    """What plan_joint returns for the list form of generate: `roles[i]` in (GENERATED, GIVEN, HELD), `generated`
    the generated modalities in ascending order, `given` {modality: the caller's int64 tensor}, and the checked
    shape: B prompts of n0 tokens, N new tokens. `evidence` is None, "weights" or "resample", with it
    `resample_every`, `ess_threshold` and `points`, the new-token indices j after whose sampling the paths are
    resampled (resample_points; empty unless evidence == "resample")."""

    def __init__(self, roles, generated, given, B, n0, N, evidence=None, resample_every=1, ess_threshold=0.5):
        self.roles, self.generated, self.given, self.B, self.n0, self.N = roles, generated, given, B, n0, N
        self.evidence, self.resample_every, self.ess_threshold = evidence, resample_every, ess_threshold
        self.points = resample_points(N, resample_every) if evidence == "resample" else []
        self.forecast = None  # check_forecast's result: the forecast settings, None when off
        self.horizon = None  # check_horizon's result: the horizon settings, None when off
        self.realised = None  # check_realised's result: the realised series to score the horizon against, or None


EVIDENCE_MODES = (None, "weights", "resample")


def resample_points(N, resample_every):
    """The fixed schedule of generate(evidence="resample"): the paths are resampled after the sampling of new token
    j whenever (j + 1) % resample_every == 0 and j < N - 1 (after the last token nothing is left to steer)."""
    return [j for j in range(N - 1) if (j + 1) % resample_every == 0]


DEFAULT_QUANTILES = (0.05, 0.5, 0.95)


def check_forecast(forecast, generated, vocab_sizes):
    """generate's forecast= for the generated modalities: None / False (off), True, or a dict with the optional keys
    "quantiles" (at most 16 levels in (0, 1)), "values" {i: V_i non-decreasing numbers} and "is_percent" {i: bool},
    i generated. Returns None or {"quantiles": [floats], "values": {i: CPU fp64 [V_i]}, "is_percent": {i: bool}};
    ValueError for anything else (checked on the host, once)."""
    if forecast is None or forecast is False:
        return None
    if forecast is True:
        forecast = {}
    if not isinstance(forecast, dict):
        raise ValueError(f"generate: forecast must be True or a dict, got {forecast!r}")
    for k in forecast:
        if k not in ("quantiles", "values", "is_percent"):
            raise ValueError(f"generate: forecast has no key {k!r} (quantiles, values, is_percent)")
    out = {"quantiles": MS.check_quantiles(forecast.get("quantiles", DEFAULT_QUANTILES)), "values": {},
           "is_percent": {}}
    for name in ("values", "is_percent"):
        d = forecast.get(name) or {}
        if not isinstance(d, dict):
            raise ValueError(f"generate: forecast[{name!r}] must be a dict {{modality: ...}}")
        for i, x in d.items():
            if i not in generated:
                raise ValueError(f"generate: forecast[{name!r}] names modality {i!r}, which is not generated")
            out[name][i] = (MS.check_values(x, vocab_sizes[i], f"forecast['values'][{i}]") if name == "values"
                            else bool(x))
    return out


def check_horizon(horizon, generated, vocab_sizes, forecast=None):
    """generate's horizon= for the generated modalities: None / False (off), True, or a dict with the optional keys
    "quantiles" (at most 16 levels in (0, 1)), "values" {i: V_i non-decreasing numbers}, "is_percent" {i: bool} and
    "barriers" {i: at most 8 finite non-zero numbers}, i generated, and the joint keys "baskets" / "pairs"
    (check_joint). values and is_percent default to those of `forecast` (check_forecast's result) where it is given.
    Returns None or {"quantiles", "values" {i: CPU fp64 [V_i]}, "is_percent" {i: bool}, "barriers" {i: [floats]},
    "modalities": the generated modalities with values, ascending}, with check_joint's entries where a joint key is given;
    ValueError for anything else, and when no generated modality has values (a horizon has no meaning on token
    indices)."""
    if horizon is None or horizon is False:
        return None
    if horizon is True:
        horizon = {}
    if not isinstance(horizon, dict):
        raise ValueError(f"generate: horizon must be True or a dict, got {horizon!r}")
    for k in horizon:
        if k not in ("quantiles", "values", "is_percent", "barriers", "baskets", "pairs"):
            raise ValueError(f"generate: horizon has no key {k!r} (quantiles, values, is_percent, barriers, baskets, "
                             "pairs)")
    out = {"quantiles": MS.check_quantiles(horizon.get("quantiles", DEFAULT_QUANTILES)),
           "values": dict(forecast["values"]) if forecast else {},
           "is_percent": dict(forecast["is_percent"]) if forecast else {}, "barriers": {}}
    for name in ("values", "is_percent", "barriers"):
        d = horizon.get(name) or {}
        if not isinstance(d, dict):
            raise ValueError(f"generate: horizon[{name!r}] must be a dict {{modality: ...}}")
        for i, x in d.items():
            if i not in generated:
                raise ValueError(f"generate: horizon[{name!r}] names modality {i!r}, which is not generated")
            out[name][i] = (MS.check_values(x, vocab_sizes[i], f"horizon['values'][{i}]") if name == "values"
                            else MS.check_barriers(x) if name == "barriers" else bool(x))
    out["modalities"] = [i for i in generated if i in out["values"]]
    if not out["modalities"]:
        raise ValueError("generate: horizon= needs the values of a generated modality (horizon={\"values\": {i: ...}} "
                         "or forecast's): a horizon has no meaning on token indices")
    if "baskets" in horizon or "pairs" in horizon:
        out.update(check_joint(horizon.get("baskets"), horizon.get("pairs"), out["modalities"]))
    return out


def check_joint(baskets, pairs, modalities):
    """horizon's "baskets" and "pairs" against the generated modalities with values: baskets None or a list of at most
    8 dicts {"weights": {i: a_i}, "barriers": [...]} (a modality that is not named has coefficient 0; the a_i finite,
    not all zero), pairs None, "all" or a list of distinct (i, k), i != k. Returns {"baskets": [{"weights": {i: float},
    "barriers": [floats]}], "pairs": [(i, k)], "joint_modalities": the modalities a basket or a pair names, ascending};
    ValueError for anything else: a modality without values, a list that is too long, more than 8 modalities named,
    and both keys empty."""
    def modality(i, where):
        if isinstance(i, bool) or not isinstance(i, int) or i not in modalities:
            raise ValueError(f"generate: horizon[{where}] names modality {i!r}, which is not a generated modality with "
                             f"values (horizon covers {modalities})")
        return i

    bk = []
    if baskets is not None:
        if not isinstance(baskets, (list, tuple)) or not all(isinstance(b, dict) for b in baskets):
            raise ValueError("generate: horizon[\"baskets\"] must be a list of dicts {\"weights\": {modality: a}, "
                             "\"barriers\": [...]}")
        if len(baskets) > MS.JOINT_MAX_BASKETS:
            raise ValueError(f"generate: horizon[\"baskets\"] holds at most {MS.JOINT_MAX_BASKETS} baskets, got "
                             f"{len(baskets)}")
        for n, b in enumerate(baskets):
            for name in b:
                if name not in ("weights", "barriers"):
                    raise ValueError(f"generate: basket {n} has no key {name!r} (weights, barriers)")
            w = b.get("weights")
            if not isinstance(w, dict) or not w:
                raise ValueError(f"generate: basket {n} needs \"weights\": a dict {{modality: coefficient}}")
            try:
                a = {modality(i, "'baskets'"): float(x) for i, x in w.items()}
            except TypeError:
                raise ValueError(f"generate: the weights of basket {n} must be numbers, got {w!r}") from None
            if any(x != x or x in (float("inf"), float("-inf")) for x in a.values()):
                raise ValueError(f"generate: the weights of basket {n} must be finite, got {w!r}")
            if not any(x != 0.0 for x in a.values()):
                raise ValueError(f"generate: basket {n} has no non-zero weight")
            bk.append({"weights": {i: a[i] for i in sorted(a)}, "barriers": MS.check_barriers(b.get("barriers"))})
    pr = []
    if isinstance(pairs, str):
        if pairs != "all":
            raise ValueError(f"generate: horizon[\"pairs\"] must be \"all\" or a list of (i, k), got {pairs!r}")
        pr = [(i, k) for n, i in enumerate(modalities) for k in modalities[n + 1:]]
    elif pairs is not None:
        try:
            pr = [(modality(i, "'pairs'"), modality(k, "'pairs'")) for i, k in pairs]
        except TypeError:
            raise ValueError(f"generate: horizon[\"pairs\"] must be \"all\" or a list of (i, k), got {pairs!r}") from None
        if any(i == k for i, k in pr) or len(set(pr)) != len(pr):
            raise ValueError(f"generate: horizon[\"pairs\"] needs distinct pairs of two different modalities, got {pr}")
    if len(pr) > MS.JOINT_MAX_PAIRS:
        raise ValueError(f"generate: horizon[\"pairs\"] holds at most {MS.JOINT_MAX_PAIRS} pairs, got {len(pr)}")
    if not bk and not pr:
        raise ValueError("generate: horizon[\"baskets\"] / [\"pairs\"] name no basket and no pair")
    named = sorted({i for b in bk for i in b["weights"]} | {i for pq in pr for i in pq})
    if len(named) > MS.JOINT_MAX_PROBLEMS:
        raise ValueError(f"generate: the baskets and pairs of one call name at most {MS.JOINT_MAX_PROBLEMS} modalities, "
                         f"got {named}")
    return {"baskets": bk, "pairs": pr, "joint_modalities": named}


def check_realised(realised, horizon, B, N):
    """generate's realised= against the plan's horizon (check_horizon's result): None (off), or a dict {i: int64 [B, N]
    tokens}, i a generated modality with values, the series that followed each prompt. Returns None or the dict, its
    keys ascending; ValueError for anything else, and without horizon= (the scores are those of the horizon forecast).
    The tokens' range is not read back: a row with a token outside the vocabulary is dead on the device."""
    if realised is None:
        return None
    if horizon is None:
        raise ValueError("generate: realised= scores the horizon forecast: pass horizon= (with the values of the "
                         "modalities to score)")
    if not isinstance(realised, dict) or not realised:
        raise ValueError("generate: realised must be a dict {modality: int64 [B, N] tokens}")
    for i, t in realised.items():
        if isinstance(i, bool) or not isinstance(i, int) or i not in horizon["modalities"]:
            raise ValueError(f"generate: realised names modality {i!r}, which is not a generated modality with values "
                             f"(horizon covers {horizon['modalities']})")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.long:
            raise ValueError(f"generate: realised[{i}] must be an int64 tensor")
        if tuple(t.shape) != (B, N):
            raise ValueError(f"generate: realised[{i}] must be [{B}, {N}], got {tuple(t.shape)}")
    return {i: realised[i] for i in sorted(realised)}


def plan_joint(modality_to_generate, given, vocab_sizes, prompt_shapes, max_new_tokens, num_samples=None,
               evidence=None, resample_every=1, ess_threshold=0.5, forecast=None, horizon=None, realised=None):
    """generate's `modality_to_generate` and `given` as per-modality roles, every refusal of the list form that
    needs no device in one place. An int (the int form: one modality sampled, generate as it always ran) returns
    None, and refuses `given`. A sequence of distinct ints, even of one, or "all" is the list form (a joint
    rollout): those modalities are GENERATED, the keys of `given` are GIVEN (tokens supplied by the caller,
    int64 [B, N] or [B * num_samples, N] with N = max_new_tokens), every other modality is HELD at its last prompt
    token. ValueError for: a modality named twice, out of range or not an int; an empty list; a modality both
    generated and given; a given tensor of another dtype or shape, or with a token outside 0..V_i - 1; a wrong
    number of prompts; prompts that are not [B, n0 >= 1] of one shape (the reference's pad / crop rule is defined
    around one generated modality). `evidence` ("weights" or "resample": the importance weights of the given series,
    generate's docstring) is refused without a given modality, with an unknown value, with resample_every < 1
    or no integer, with a negative or NaN ess_threshold, and as "resample" without num_samples. `horizon`
    (check_horizon) is refused in the int form and with num_samples > 4096 (the paths of a prompt are sorted on
    chip)."""
    M = len(vocab_sizes)
    g = modality_to_generate
    if evidence not in EVIDENCE_MODES:
        raise ValueError(f"generate: evidence must be None, \"weights\" or \"resample\", got {evidence!r}")
    if evidence is not None:
        if not given:
            raise ValueError("generate: evidence= needs a given modality (given={modality: tokens}): the weights are "
                             "the probabilities of the given tokens")
        if isinstance(resample_every, bool) or not isinstance(resample_every, int) or resample_every < 1:
            raise ValueError(f"generate: resample_every must be an integer >= 1, got {resample_every!r}")
        try:
            thr_ok = float(ess_threshold) >= 0.0
        except (TypeError, ValueError):
            thr_ok = False
        if not thr_ok:
            raise ValueError(f"generate: ess_threshold must be a number >= 0, got {ess_threshold!r}")
        if evidence == "resample" and num_samples is None:
            raise ValueError("generate: evidence=\"resample\" resamples the num_samples paths of each prompt: pass "
                             "num_samples")
    if isinstance(g, int) and not isinstance(g, bool):
        if given is not None:
            raise ValueError("generate: given= needs the list form of modality_to_generate (a sequence or \"all\")")
        if forecast is not None and forecast is not False:
            raise ValueError(f"generate: forecast= needs the list form of modality_to_generate: pass [{g}] (a "
                             "sequence, even of one, or \"all\")")
        if horizon is not None and horizon is not False:
            raise ValueError(f"generate: horizon= needs the list form of modality_to_generate: pass [{g}] (a "
                             "sequence, even of one, or \"all\")")
        if realised is not None:
            raise ValueError(f"generate: realised= needs the list form of modality_to_generate: pass [{g}] (a "
                             "sequence, even of one, or \"all\") and horizon=")
        return None
    if isinstance(g, str):
        if g != "all":
            raise ValueError(f"generate: modality_to_generate must be an int, a sequence of ints or \"all\", got {g!r}")
        gen = list(range(M))
    else:
        try:
            gen = list(g)
        except TypeError:
            raise ValueError(f"generate: modality_to_generate must be an int, a sequence of ints or \"all\", "
                             f"got {g!r}") from None
    for i in gen:
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < M:
            raise ValueError(f"generate: modality_to_generate names {i!r}; modalities are the ints 0..{M - 1}")
    if len(set(gen)) != len(gen):
        raise ValueError(f"generate: modality_to_generate names a modality twice: {gen}")
    if not gen:
        raise ValueError("generate: modality_to_generate is empty")
    N = int(max_new_tokens)
    if N < 0:
        raise ValueError(f"generate: max_new_tokens must be >= 0, got {max_new_tokens!r}")
    shapes = [tuple(int(x) for x in s) for s in prompt_shapes]
    if len(shapes) != M:
        raise ValueError(f"expected {M} index tensors, got {len(shapes)}")
    if any(len(s) != 2 for s in shapes) or len(set(shapes)) != 1:
        raise ValueError(f"generate: a joint rollout needs [B, n0] prompts of one shape, got {shapes}")
    B, n0 = shapes[0]
    if n0 < 1:
        raise ValueError("generate: the prompt must hold at least one token")
    given = {} if given is None else given
    if not isinstance(given, dict):
        raise ValueError("generate: given must be a dict {modality: int64 [B, N] tokens}")
    rows = (B,) if num_samples is None else (B, B * num_samples)
    for i, t in given.items():
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < M:
            raise ValueError(f"generate: given names {i!r}; modalities are the ints 0..{M - 1}")
        if i in gen:
            raise ValueError(f"generate: modality {i} is both generated and given")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.long:
            raise ValueError(f"generate: given[{i}] must be an int64 tensor")
        if t.dim() != 2 or t.shape[1] != N or t.shape[0] not in rows:
            raise ValueError(f"generate: given[{i}] must be [{' or '.join(str(r) for r in rows)}, {N}], "
                             f"got {tuple(t.shape)}")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= vocab_sizes[i]):
            raise ValueError(f"generate: given[{i}] holds tokens outside 0..{vocab_sizes[i] - 1}")
    roles = [GENERATED if i in gen else GIVEN if i in given else HELD for i in range(M)]
    plan = JointPlan(roles, sorted(gen), dict(given), B, n0, N, evidence, resample_every,
                     0.5 if evidence is None else float(ess_threshold))
    plan.forecast = check_forecast(forecast, plan.generated, vocab_sizes)
    plan.horizon = check_horizon(horizon, plan.generated, vocab_sizes, plan.forecast)
    if plan.horizon is not None and num_samples is not None:
        if num_samples > MS.HORIZON_MAX_SAMPLES:
            raise ValueError(f"generate: horizon= sorts at most {MS.HORIZON_MAX_SAMPLES} samples per prompt, got "
                             f"num_samples={num_samples}")
    plan.realised = check_realised(realised, plan.horizon, B, N)
    return plan


def joint_setting(value, generated, name):
    """A sampling setting of the list form per generated modality: a scalar (or None) for all, or a dict
    {modality: value} whose keys are generated modalities (the others take the default)."""
    if not isinstance(value, dict):
        return {i: value for i in generated}
    for i in value:
        if i not in generated:
            raise ValueError(f"generate: {name} names modality {i!r}, which is not generated")
    return {i: value.get(i) for i in generated}


def cache_rule(model, use_cache):
    """Whether generate may use the KV cache: not in training mode with dropout (the reference's forward samples
    dropout there) and not at fp8 (whose forward GEMMs the bf16 decode would not reproduce)."""
    return bool(use_cache) and not (model.training and model.dropout_p > 0.0) and model.precision == "bf16"


def fans_out(cache, shapes, N, S, T):
    """Whether generate(num_samples=S) runs the fan-out engine: the cache rule, [B, n0 >= 1] prompts of one shape and
    1 <= N new tokens that fit the block. Otherwise the prompts are tiled."""
    return (S is not None and cache and all(len(sh) == 2 for sh in shapes) and len(set(shapes)) == 1
            and shapes[0][1] >= 1 and shapes[0][1] + N <= T and N >= 1)


def rolls(cache, shapes, N, S, T, rolling=False):
    """Whether generate(num_samples=S, rolling=True) runs the rolling-window engine: `rolling` is given, the fans_out
    conditions hold with the bound n0 + N <= T lifted (the cache rule, [B, n0 >= 1] prompts of one shape, N >= 1),
    the prompt fits the block (n0 <= T), N <= T (so the shared prefix of the last step keeps a row) and the call
    leaves the block at all: the last step reads a sequence of n0 + N - 1 > T tokens. A call that stays inside the
    block is fans_out's (bit for bit the call without the keyword); everything else is tiled."""
    return (bool(rolling) and S is not None and bool(cache) and all(len(sh) == 2 for sh in shapes)
            and len(set(shapes)) == 1 and 1 <= shapes[0][1] <= T and 1 <= N <= T and shapes[0][1] + N - 1 > T)


def generate_path(cache, shapes, N, S, T, rolling=False):
    """model.last_generate_path of a call with num_samples: "fanout" where fans_out holds (whatever `rolling`
    says), "rolling" where rolls holds, else "tiled"."""
    if fans_out(cache, shapes, N, S, T):
        return "fanout"
    return "rolling" if rolls(cache, shapes, N, S, T, rolling) else "tiled"


def rolling_step(n0, j, T):
    """What new token j of a rolling call runs. The step reads a sequence of n = n0 + j tokens. While n <= T the
    existing steps apply (None): the prefill at j == 0, then mmt_decode_fanout_step at position n - 1. Past the block
    every position shifts: (k, m, p) with k = n - T the window's first column, m = j the path's own last rows and
    p = T - m the rows of the prompt, shifted, that all paths of a prompt share."""
    n = n0 + j
    return None if n <= T else (n - T, j, T - j)


def rolling_schedule(n0, N, T):
    """rolling_step for j = 0..N-1."""
    return [rolling_step(n0, j, T) for j in range(N)]


@torch.no_grad()
def reference_loop(model, seqs, N, g, use_cache, pick):
    """The reference's loop (its model.py:404-446) over `seqs`, a list the loop extends: per new token the logits of
    the last position of the block_size cropped context, `pick(j, n, last) -> [B, 1]` tokens of modality g for
    position n, appended; the other modalities are padded with their last token or cropped to the same length. While
    the cache rule holds, the prompts share one length and the sequence fits the block, the first step is the
    prefill and every later one a decode step."""
    T = model.block_size
    cache = (cache_rule(model, use_cache) and len({int(s.shape[1]) for s in seqs}) == 1
             and all(s.dim() == 2 for s in seqs))
    cached_pos = None  # the last position whose keys / values the workspace holds
    for j in range(N):
        n = seqs[g].shape[1]
        if cache and cached_pos == n - 2 and n <= T:
            last = model._decode_step([s[:, n - 1] for s in seqs], n - 1)[g]
            cached_pos = n - 1
        else:
            logits, _ = model([s[:, -T:] for s in seqs])
            last = logits[g][:, -1, :]
            cached_pos = n - 1 if (cache and n <= T) else None
        nxt = pick(j, n, last).to(seqs[g].dtype)
        seqs[g] = torch.cat((seqs[g].to(nxt.device), nxt), dim=1)
        for i in range(model.num_modalities):
            if i != g and seqs[i].shape[1] < n + 1:
                seqs[i] = torch.cat((seqs[i], seqs[i][:, -1:]), dim=1)
            elif i != g and seqs[i].shape[1] > n + 1:
                seqs[i] = seqs[i][:, :n + 1]
    return seqs


class DecodeArgs:
    """The arguments of the decode launches, one set for both logits sources, made at first use: the [rows, V_i]
    logits buffers and the token pointers. idx[i] points at the compact buffer of a generated modality, at the held
    token, or at row j of a given modality's [N, rows] `steps`: the engine reads the pointer array on the host per
    call, so the host moves a pointer and no kernel copies a token."""

    def __init__(self, model, rows, compact, held, steps):
        self.model, self.rows, self.compact, self.held, self.steps = model, rows, compact, held, steps
        self.logits = None

    def at(self, j):
        """The arguments of the step that reads the tokens of new position j."""
        if self.logits is None:
            m, flat = self.model, self.model.flat_params
            self.logits = [torch.empty(self.rows, V, dtype=torch.float32, device=flat.device) for V in m.vocab_sizes]
            self.idx = ML.ptr_array([self.compact[i] if i in self.compact else self.held.get(i)
                                     for i in range(m.num_modalities)])
            self.out, self.flat = ML.ptr_array(self.logits), ML.ptr(flat)
        for i, st in self.steps.items():
            self.idx[i] = st.data_ptr() + 8 * self.rows * j
        return self


class CachedSource:
    """Step j's views from the KV cache or a re-forward: one position through mmt_decode_step while the cache rule
    holds, the workspace holds the position before and the sequence fits the block (the first step is the prefill),
    else the forward over the block_size cropped buffers, whose last position is read in place."""

    def __init__(self, model, bufs, dec, cache):
        self.model, self.bufs, self.dec, self.cache = model, bufs, dec, cache
        self.cached_pos = None  # the last position whose keys / values the workspace holds

    def views(self, j, n, stream):
        m, T = self.model, self.model.block_size
        if self.cache and self.cached_pos == n - 2 and n <= T:
            d = self.dec.at(j - 1)
            rc = ML.lib().mmt_decode_step(m._ctx, stream, d.rows, n - 1, d.idx, d.flat, d.out, ML.ptr(m._ws))
            ML.check(rc, m._ctx, "mmt_decode_step")
            m._gen += 1
            self.cached_pos = n - 1
            return d.logits
        logits, _ = m([buf[:, max(0, n - T):n] for buf in self.bufs])
        self.cached_pos = n - 1 if (self.cache and n <= T) else None
        return [lg[:, -1, :] for lg in logits]


class FanoutSource:
    """Step j's views for S samples per prompt from one prefill (mmt_decode_fanout_step, include/mmt.h). The prefill
    runs over the B prompts; its last-position logits, one row per prompt, are expanded to [B*S, V_i] once, for the
    modalities in `need` (row r = b*S + s). From then on a token costs one fan-out decode step over B*S rows, which
    reads the prompts' keys / values from the prefill's workspace and keeps the samples' own in the fan buffer. With
    `two`, a second fan buffer: at a resampling point `gather` moves the tails into it behind their ancestors
    (mmt_fanout_gather) and the two swap."""

    def __init__(self, model, prompts, shape, dec, need, nbytes, two):
        self.model, self.prompts, self.shape, self.dec, self.need = model, prompts, shape, dec, need
        dev = prompts[0].device
        self.bufs = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2 if two else 1)]
        self.fan, self.fan2 = ML.ptr(self.bufs[0]), ML.ptr(self.bufs[-1])

    def views(self, j, n, stream):
        m = self.model
        B, S, n0, N = self.shape
        if j == 0:
            logits, _ = m(self.prompts)  # the prefill: leaves every prompt position's keys / values in the workspace
            self.ws = ML.ptr(m._ws)
            sel = torch.arange(B, device=self.prompts[0].device).repeat_interleave(S)
            return [lg[:, -1, :].index_select(0, sel) if i in self.need else None for i, lg in enumerate(logits)]
        d = self.dec.at(j - 1)
        rc = ML.lib().mmt_decode_fanout_step(m._ctx, stream, B, S, n0, N, n - 1, d.idx, d.flat, d.out, self.ws,
                                             self.fan)
        ML.check(rc, m._ctx, "mmt_decode_fanout_step")
        return d.logits

    def gather(self, j, anc_ptr, stream):
        m = self.model
        B, S, n0, N = self.shape
        rc = ML.lib().mmt_fanout_gather(m._ctx, stream, B, S, n0, N, j, anc_ptr, self.fan, self.fan2)
        ML.check(rc, m._ctx, "mmt_fanout_gather")
        self.fan, self.fan2 = self.fan2, self.fan


class RollingSource(FanoutSource):
    """FanoutSource for a call that leaves the block (rolls, rolling_step). While the sequence read fits the block
    the steps are FanoutSource's, with a fan buffer for the block_size - n0 positions left. Past it, step j runs one
    ordinary forward over the B prompts' columns k..n0-1 (the p = block_size - j rows every path of a prompt shares,
    at their shifted positions), which leaves their keys / values in the workspace, then ONE mmt_rolling_step over
    the paths' own m = j tokens, read in place from columns n0..n-1 of the [rows, cap] sequence buffers (generated,
    given and held modalities alike). No torch op per token beyond that forward, and no sync."""

    def __init__(self, model, prompts, shape, dec, need, nbytes, seqs, cap, roll_bytes):
        B, S, n0, N = shape
        super().__init__(model, prompts, (B, S, n0, model.block_size - n0), dec, need, nbytes, False)
        self.seqs, self.cap = seqs, cap
        self.roll_buf = torch.empty(roll_bytes, dtype=torch.uint8, device=prompts[0].device)
        self.roll, self.tail = ML.ptr(self.roll_buf), ML.ptr_array(seqs)

    def views(self, j, n, stream):
        m = self.model
        B, S, n0, _ = self.shape
        step = rolling_step(n0, j, m.block_size)
        if step is None:
            return super().views(j, n, stream)
        k, mt, p = step
        m([pr[:, k:n0] for pr in self.prompts])
        d = self.dec.at(j - 1)
        for i, buf in enumerate(self.seqs):
            self.tail[i] = buf.data_ptr() + 8 * (n - mt)
        rc = ML.lib().mmt_rolling_step(m._ctx, stream, B, S, p, mt, self.tail, self.cap, d.flat, d.out, ML.ptr(m._ws),
                                       self.roll)
        ML.check(rc, m._ctx, "mmt_rolling_step")
        return d.logits


@torch.no_grad()
def rollout(model, idx_list, plan, use_cache, temperature, top_k, top_p, seed, return_logprobs, logits_hook, S,
            seed_of=MS.modality_seed, rolling=False):
    """The device loop of generate. Every GENERATED modality i of the plan is sampled per step from its own head, all
    of them in one mmt_sample_multi launch, with the seed seed_of(seed, i); GIVEN modalities follow the caller's
    tokens; HELD ones stay at their last prompt token. The sequences live in preallocated [rows, n0 + N] buffers,
    given columns and held pads are written once before the loop (what the reference's pad / crop rule amounts to
    for prompts of one length), the sampler writes column n of a generated modality's buffer and the compact [rows]
    token buffer the next decode step reads (DecodeArgs). Per token the host asks the logits source for the step's
    views (CachedSource; with num_samples where fans_out holds, FanoutSource over B*S rows, where rolls holds (`rolling`,
    a call that leaves the block) RollingSource, else the tiled prompts)
    and runs the stages: no torch op, no sync. The draw of row r at sequence position n is keyed by (seed_of(seed,
    i), r, n): the same seed and the same logits give the same tokens whatever the cache mode and whatever else is in
    the batch. seed=None takes one from the device generator (never torch's CPU generator). `logits_hook(n, views)`
    sees the [rows, V_i] views the sampler is about to read (the decode steps reuse one buffer: clone to keep).
    With plan.evidence a step also issues one mmt_score_multi over the given modalities' views and the given tokens
    of column n, which the sequence buffers hold; "resample" adds, at the plan's points, mmt_resample, an
    index_select of every per-row buffer and the source's gather; a closing mmt_resample folds the remaining
    columns. With plan.forecast a step also issues one mmt_forecast_multi over the generated modalities' views, after
    the sampling and scoring and before a resampling, into column j of preallocated [Bp, N, V_i] buffers; one
    mmt_sample.pmf_stats follows the loop. With plan.horizon one mmt_sample.horizon_stats follows the loop too, over
    the sequence buffers' new columns (and, with the joint keys of horizon=, one mmt_sample.horizon_joint on the same
    buffers, origins and weights), and with plan.realised one mmt_sample.horizon_score after it, on the same
    buffers. Returns seqs, or the tuple (seqs[, {i: logprobs}][, ev][, fc][, hz][, sc])."""
    flat = model.flat_params
    dev = flat.device
    M, T, N, n0, gen, Vs = model.num_modalities, model.block_size, plan.N, plan.n0, plan.generated, model.vocab_sizes
    ts, ks, ps = (joint_setting(temperature, gen, "temperature"), joint_setting(top_k, gen, "top_k"),
                  joint_setting(top_p, gen, "top_p"))
    settings = [MS.check_settings(ts[i], ks[i], ps[i]) for i in gen]
    if dev.type != "cuda":
        raise RuntimeError(NO_GPU)
    seed = MS.device_seed(dev) if seed is None else int(seed) & MS.MASK64
    L = ML.lib()
    cache = cache_rule(model, use_cache)
    shapes = [tuple(s.shape) for s in idx_list]
    fan = fans_out(cache, shapes, N, S, T)
    roll = not fan and rolls(cache, shapes, N, S, T, rolling)
    nbytes = L.mmt_fanout_bytes(model._ctx, plan.B, S, N) if fan else 0
    roll_bytes = 0
    if roll:  # the fan buffer of the positions left in the block, the roll buffer of the longest tail (N - 1 rows)
        nbytes = L.mmt_fanout_bytes(model._ctx, plan.B, S, T - n0) if n0 < T else 0
        roll_bytes = L.mmt_rolling_bytes(model._ctx, plan.B, S, N - 1)
    if nbytes < 0 or roll_bytes < 0:
        raise ValueError(f"generate: {plan.B} prompts x {S} samples are more rows than the decode launches address")
    if plan.evidence == "resample" and not (fan and S <= MS.RESAMPLE_MAX_SAMPLES):
        raise ValueError(
            "generate: evidence=\"resample\" runs on the fan-out engine only: it needs num_samples (at most "
            f"{MS.RESAMPLE_MAX_SAMPLES}), use_cache, eval mode or no dropout, precision bf16, max_new_tokens >= 1 and "
            "n0 + max_new_tokens <= block_size (rolling= does not lift that for it)")
    if plan.evidence is not None and S is not None and S > MS.RESAMPLE_MAX_SAMPLES:
        raise ValueError(f"generate: evidence= folds the weights of at most {MS.RESAMPLE_MAX_SAMPLES} samples per "
                         f"prompt, got num_samples={S}")
    if S is not None:
        model.last_generate_path = "fanout" if fan else "rolling" if roll else "tiled"
    prompts = [s.to(device=dev, dtype=torch.long).contiguous() for s in idx_list]
    rows = prompts if S is None else tile_prompts(prompts, S)
    R, cap = rows[0].shape[0], n0 + N
    bufs, steps = [], {}
    for i, s in enumerate(rows):
        buf = torch.zeros(R, cap, dtype=torch.long, device=dev)
        buf[:, :n0] = s
        if plan.roles[i] == GIVEN and N > 0:
            g = plan.given[i].to(dev)
            buf[:, n0:] = g if g.shape[0] == R else g.repeat_interleave(S, 0)
            steps[i] = buf[:, n0:].t().contiguous()  # [N, R]: row j is what a decode step of new position j reads
        elif plan.roles[i] == HELD and N > 0:
            buf[:, n0:] = s[:, -1:]
        bufs.append(buf)
    compact = {i: torch.zeros(R, dtype=torch.long, device=dev) for i in gen}
    held = {i: rows[i][:, -1].contiguous() for i in range(M) if plan.roles[i] == HELD}
    lps = {i: torch.empty(R, N, dtype=torch.float32, device=dev) for i in gen} if return_logprobs else None
    ml = MS.MultiLaunch([Vs[i] for i in gen], settings, [seed_of(seed, i) for i in gen], [cap] * len(gen),
                        [N] * len(gen))
    for p, i in enumerate(gen):
        ml.compact[p] = compact[i].data_ptr()
    # evidence: one scoring problem per given modality, over the views the sampler reads and the given token of
    # column n, which the sequence buffers already hold; the fp64 weights per row and evidence per prompt
    giv = sorted(plan.given) if plan.evidence is not None else []
    Bp, Sp = (plan.B, S) if S is not None else (R, 1)  # without num_samples every row is a prompt of one path
    if giv:
        glp = {i: torch.zeros(R, N, dtype=torch.float32, device=dev) for i in giv}
        sl = MS.ScoreLaunch([Vs[i] for i in giv], [cap] * len(giv), [N] * len(giv))
        logw = torch.zeros(R, dtype=torch.float64, device=dev)
        logev = torch.zeros(Bp, dtype=torch.float64, device=dev)
        npts = len(plan.points)
        anc = torch.empty(npts + 1, R, dtype=torch.int32, device=dev)  # the last row: the closing fold's identity
        res = torch.empty(npts + 1, Bp, dtype=torch.int32, device=dev)
        rl = MS.ResampleLaunch([glp[i].data_ptr() for i in giv], [N] * len(giv))
    # forecast: per generated modality the pmf of every (prompt, new token), ESS and live count as [N, Bp] (a
    # step writes one contiguous row); the weights are those the evidence carries: logw and the given columns
    fc = plan.forecast
    if fc is not None:
        fpmf = {i: torch.zeros(Bp, N, Vs[i], dtype=torch.float32, device=dev) for i in gen}
        fess = {i: torch.zeros(N, Bp, dtype=torch.float64, device=dev) for i in gen}
        flive = {i: torch.zeros(N, Bp, dtype=torch.int32, device=dev) for i in gen}
        fl = MS.ForecastLaunch([Vs[i] for i in gen], settings, [max(N, 1) * Vs[i] for i in gen],
                               [glp[i].data_ptr() for i in giv], [N] * len(giv))
        fbytes = fl.scratch_bytes(L, Bp, Sp)
        fscratch = torch.empty(max(fbytes, 16), dtype=torch.uint8, device=dev)
        # with evidence the forecast carries rule 2's a_s itself, from one buffer into the other, and folds ONE
        # column per step: the serial fp64 sum over the columns since the last point, bit for bit, at O(1) a step
        facc = torch.zeros(2, R, dtype=torch.float64, device=dev) if giv else None
        fcur = 0

    def stages(n, j, views):
        """Sample, then score the given tokens, then forecast: each binds its problems to the step's views."""
        nonlocal fcur
        if logits_hook is not None:
            logits_hook(n, views)
        for p, i in enumerate(gen):
            MS.bind_view(ml, p, views[i], R)
            ml.tok[p] = bufs[i].data_ptr() + 8 * n
            ml.logprob[p] = lps[i].data_ptr() + 4 * j if lps is not None else None
        ml.run(L, stream, R, 0, n)
        if giv:
            for p, i in enumerate(giv):
                MS.bind_view(sl, p, views[i], R)
                sl.tok[p] = bufs[i].data_ptr() + 8 * n
                sl.logprob[p] = glp[i].data_ptr() + 4 * j
            sl.run(L, stream, R)
        if fc is not None:  # the mixture of the laws just drawn from, weighted by the given columns since..j
            for p, i in enumerate(gen):
                MS.bind_view(fl, p, views[i], R)
                fl.pmf[p] = fpmf[i].data_ptr() + 4 * Vs[i] * j
                fl.ess[p] = fess[i].data_ptr() + 8 * Bp * j
                fl.live[p] = flive[i].data_ptr() + 4 * Bp * j
            if giv:
                fl.run(L, stream, Bp, Sp, j, j + 1, facc[fcur].data_ptr(), fscratch.data_ptr(), fbytes,
                       facc[1 - fcur].data_ptr())
                fcur = 1 - fcur
            else:
                fl.run(L, stream, Bp, Sp, 0, 0, 0, fscratch.data_ptr(), fbytes)

    def fold(j0, j1, threshold, pos, point):
        """mmt_resample over the given log-probabilities of the new tokens j0..j1-1 into row `point` of the
        ancestors / resampled records."""
        rl.run(L, stream, Bp, Sp, j0, j1, logw.data_ptr(), logev.data_ptr(), threshold, seed, pos,
               anc.data_ptr() + 4 * R * point, res.data_ptr() + 4 * Bp * point)

    def follow(a):
        """Every per-row buffer follows its ancestor (in place: the launch arrays keep their addresses)."""
        a = a.long()
        for t in bufs + list(compact.values()) + list(glp.values()) + (list(lps.values()) if lps else []):
            t.copy_(t.index_select(0, a))
        for st in steps.values():
            st.copy_(st.index_select(1, a))

    dec = DecodeArgs(model, R, compact, held, steps)
    if fan or roll:  # the prefill's first rows: only of the modalities a stage (or the hook) reads
        need = range(M) if logits_hook is not None else gen + giv
        if fan:
            source = FanoutSource(model, prompts, (plan.B, S, n0, N), dec, need, nbytes, bool(plan.points))
        else:
            source = RollingSource(model, prompts, (plan.B, S, n0, N), dec, need, nbytes, bufs, cap, roll_bytes)
    else:
        source = CachedSource(model, bufs, dec, cache)
    with torch.cuda.device(dev):
        stream = ML.stream_ptr(dev)
        last_point, point = 0, 0
        for j in range(N):
            n = n0 + j
            stages(n, j, source.views(j, n, stream))
            if point < len(plan.points) and plan.points[point] == j:
                # the fixed schedule: weights of the columns since the last point, ancestors (the identity for a
                # prompt that did not trigger), then every per-row buffer and the fan-out tails follow them
                fold(last_point, j + 1, plan.ess_threshold, n, point)
                follow(anc[point])
                if fc is not None:  # the forecast's carried sums restart from the folded weights
                    facc[fcur].copy_(logw)
                if j >= 1:
                    source.gather(j, anc.data_ptr() + 4 * R * point, stream)
                last_point, point = j + 1, point + 1
        if giv:
            fold(last_point, N, -1.0, n0 + N - 1, point)  # the closing fold: no resampling
    seqs = [buf.to(idx_list[i].dtype) for i, buf in enumerate(bufs)]
    out = [seqs] + ([lps] if return_logprobs else [])
    if giv:
        out.append({"given_logprobs": glp, "log_weights": logw, "log_evidence": logev, "ancestors": anc[:npts],
                    "resampled": res[:npts], "steps": list(plan.points)})
    if fc is not None:
        # the summaries of every (prompt, new token) pmf row; the origin of a value series' direction is the
        # prompt's last token of that modality
        stats, qtok = MS.pmf_stats([fpmf[i] for i in gen], values=[fc["values"].get(i) for i in gen],
                                   is_percent=[fc["is_percent"].get(i, False) for i in gen],
                                   origin=[prompts[i][:, -1:].expand(Bp, N).contiguous() for i in gen],
                                   quantiles=fc["quantiles"])
        res_fc = {}
        for i, s, qt in zip(gen, stats, qtok):
            if i in fc["values"]:
                qv = torch.where(qt >= 0, fc["values"][i].to(dev)[qt.clamp_min(0).long()], float("nan"))
            else:
                qv = torch.full(qt.shape, float("nan"), dtype=torch.float64, device=dev)
            res_fc[i] = {"pmf": fpmf[i], "ess": fess[i].t().contiguous(), "live": flive[i].t().contiguous(),
                         "entropy": s[..., 1], "mean": s[..., 2], "var": s[..., 3], "p_down": s[..., 4],
                         "p_flat": s[..., 5], "p_up": s[..., 6], "quantile_tokens": qt, "quantile_values": qv}
        out.append(res_fc)
    hz = plan.horizon
    if hz is not None:
        # the final paths: the new columns of the sequence buffers, the origin of a value series the column before
        # them, the weights the final log_weights. One number of barriers per call: shorter lists are padded (with
        # 1.0) and their columns cut from the result.
        mods = hz["modalities"]
        bars = [list(hz["barriers"].get(i, [])) for i in mods]
        nbar = max(len(b) for b in bars)
        res_hz = MS.horizon_stats([bufs[i][:, n0:] for i in mods], samples=Sp, values=[hz["values"][i] for i in mods],
                                  is_percent=[hz["is_percent"].get(i, False) for i in mods],
                                  origin=[bufs[i][:, n0 - 1] for i in mods], logw=logw if giv else None,
                                  quantiles=hz["quantiles"], barriers=[b + [1.0] * (nbar - len(b)) for b in bars])
        rz = plan.realised
        if rz is not None:
            # the scores of that forecast against the series that followed each prompt: the same buffers, weights,
            # levels and padded barriers, the origin of the realised row the prompt's last token
            at = [mods.index(i) for i in rz]
            res_sc = MS.horizon_score([bufs[i][:, n0:] for i in rz], [rz[i].to(dev).contiguous() for i in rz],
                                      samples=Sp, values=[hz["values"][i] for i in rz],
                                      is_percent=[hz["is_percent"].get(i, False) for i in rz],
                                      origin=[bufs[i][:, n0 - 1] for i in rz],
                                      realised_origin=[prompts[i][:, -1] for i in rz], logw=logw if giv else None,
                                      forecast=[res_hz[k] for k in at], quantiles=hz["quantiles"],
                                      barriers=[bars[k] + [1.0] * (nbar - len(bars[k])) for k in at])
            for d, k in zip(res_sc, at):
                d["brier"], d["aggb"] = d["brier"][..., :len(bars[k])], d["aggb"][:, :len(bars[k])]
        for d, b in zip(res_hz, bars):
            d["hit"] = d["hit"][..., :len(b)]
        res_hz = dict(zip(mods, res_hz))
        if "joint_modalities" in hz:
            # the cross-series statistics of the same paths, origins and weights, over the modalities that a basket or a
            # pair names: series p of the call is modality jm[p]
            jm = hz["joint_modalities"]
            res_j = MS.horizon_joint([bufs[i][:, n0:] for i in jm], samples=Sp, values=[hz["values"][i] for i in jm],
                                     is_percent=[hz["is_percent"].get(i, False) for i in jm],
                                     origin=[bufs[i][:, n0 - 1] for i in jm], logw=logw if giv else None,
                                     quantiles=hz["quantiles"],
                                     baskets=[{"weights": [b["weights"].get(i, 0.0) for i in jm],
                                               "barriers": b["barriers"]} for b in hz["baskets"]],
                                     pairs=[(jm.index(i), jm.index(k)) for i, k in hz["pairs"]])
            res_j["pairs"] = {ik: res_j["pairs"][(jm.index(ik[0]), jm.index(ik[1]))] for ik in hz["pairs"]}
            res_j["modalities"] = list(jm)
            res_hz["joint"] = res_j
        out.append(res_hz)
        if rz is not None:
            out.append(dict(zip(rz, res_sc)))
    return out[0] if len(out) == 1 else tuple(out)


@torch.no_grad()
def rollout_int(model, idx_list, max_new_tokens, g, use_cache, temperature, top_k, top_p, seed, return_logprobs,
                logits_hook, S, rolling=False):
    """The int form of generate on the device: the plan with modality g GENERATED and the others HELD, its one
    sampling problem keyed by the raw seed, and the results unwrapped to the int form's shapes (the hook sees the one
    [rows, V_g] view, the log-probabilities are a tensor). With num_samples the fan-out engine runs where fans_out
    holds, the rolling engine where rolls holds; otherwise, invalid input included, the prompts are tiled, which is the
    definition of the result. Prompts
    of unequal lengths run the reference's loop (re-forward, pad / crop per step) around mmt_sample."""
    M, N, dev = model.num_modalities, int(max_new_tokens), model.flat_params.device
    if S is not None:
        path = "tiled"
        if len(idx_list) == M and 0 <= g < M and dev.type == "cuda":
            path = generate_path(cache_rule(model, use_cache), [tuple(s.shape) for s in idx_list], N, S,
                                 model.block_size, rolling)
        model.last_generate_path = path
        if path == "tiled":
            idx_list, S = tile_prompts(idx_list, S), None
    t, k, p = MS.check_settings(temperature, top_k, top_p)
    if len(idx_list) != M:
        raise ValueError(f"expected {M} index tensors, got {len(idx_list)}")
    if not 0 <= g < M:
        raise ValueError(f"modality_to_generate must be 0..{M - 1}, got {g}")
    if dev.type != "cuda":
        raise RuntimeError(NO_GPU)
    seed = MS.device_seed(dev) if seed is None else int(seed) & MS.MASK64
    B = idx_list[0].shape[0]
    if len({int(s.shape[1]) for s in idx_list}) != 1 or any(s.dim() != 2 for s in idx_list):
        lp = torch.empty(B, max(N, 0), dtype=torch.float32, device=dev) if return_logprobs else None

        def pick(j, n, last):
            if logits_hook is not None:
                logits_hook(n, last)
            nxt, l = MS.sample(last, temperature=t, top_k=k, top_p=p, seed=seed, pos=n, return_logprobs=True)
            if lp is not None:
                lp[:, j] = l
            return nxt[:, None]

        seqs = reference_loop(model, [s.to(device=dev, dtype=torch.long).clone() for s in idx_list], N, g, use_cache,
                              pick)
        seqs = [s.to(idx_list[i].dtype) for i, s in enumerate(seqs)]
        return (seqs, lp) if return_logprobs else seqs
    n0 = int(idx_list[0].shape[1])
    if n0 < 1:
        raise ValueError("generate: the prompt must hold at least one token")
    plan = JointPlan([GENERATED if i == g else HELD for i in range(M)], [g], {}, int(B), n0, max(N, 0))
    hook = None if logits_hook is None else (lambda n, views: logits_hook(n, views[g]))
    out = rollout(model, idx_list, plan, use_cache, t, k, p, seed, return_logprobs, hook, S,
                  seed_of=lambda seed, i: seed, rolling=rolling)
    return (out[0], out[1][g]) if return_logprobs else out
