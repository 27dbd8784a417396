"""Evaluation at every position (include/mmt.h: mmt_eval_positions): direction, log score and calibration of the
heads over all B x T rows an evaluation forward has written, not only the last position of each window.

    position_metrics(logits_list, xb_list, yb_list, values, is_percent, ...)   one call, the device tables
    PositionMetrics(values, is_percent, ...).add(...) / .result() / .summary_lines(names)
                                                                               tables accumulated over many batches

Calibrated temperatures (include/mmt.h: mmt_eval_temperatures): the same rows under a grid of temperatures, the
temperature that minimises the NLL:

    temperature_metrics(logits_list, xb_list, yb_list, values, is_percent, temperatures=None, ...)
    TemperatureFit(values, is_percent, temperatures=None, ...).add(...) / .result() / .summary_lines(names)
    fit_temperature(temperatures, rows, nll_sum) / derive_temperature(sum, rel, temperatures)      host fp64

Scores of horizon forecasts against the realised series (include/mmt.h: mmt_horizon_score), accumulated the same way:

    RolloutMetrics().add(scores) / .result() / .summary_lines(names)            scores: what generate(realised=) returns

Everything runs in the library's kernels; there is no torch formulation behind it. `add` launches and returns: the
one device-to-host read is in `result`."""
import ctypes

import numpy as np
import torch

import mmt_lib as ML

POS_FIELDS = ("rows", "wins", "losses", "certainty", "nll", "top1", "directed", "realised_mass")  # pos[t, k]
REC_FIELDS = ("logprob", "p_down", "p_flat", "p_up", "pit", "rank", "predicted", "realised")  # rec[b, t, k]
DIRECTIONS = ("down", "flat", "up")  # rel[d]
MAX_BINS = 64
MAX_V = 1 << 20


def _check_settings(t_begin, bins, T=None):
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"position_metrics: bins must be an integer in 1..{MAX_BINS}, got {bins!r}")
    if isinstance(t_begin, bool) or not isinstance(t_begin, int) or t_begin < 0 or (T is not None and t_begin > T):
        raise ValueError(f"position_metrics: t_begin must be an integer in 0..T{'' if T is None else f' (T = {T})'}, "
                         f"got {t_begin!r}")


def _check_inputs(logits_list, xb_list, yb_list, values, is_percent, token_range):
    """The shapes, dtypes, layout and device of one call's inputs; ValueError names the argument. Returns
    (device, B, T, [V])."""
    P = len(logits_list)
    for name, lst in (("xb_list", xb_list), ("yb_list", yb_list), ("values", values), ("is_percent", is_percent)):
        if not isinstance(lst, (list, tuple)) or len(lst) != P:
            raise ValueError(f"position_metrics: {name} must be a list of {P} entries, one per logits tensor")
    if P == 0:
        return None, 0, 0, []
    lg0 = logits_list[0]
    if not isinstance(lg0, torch.Tensor) or lg0.dim() != 3:
        raise ValueError("position_metrics: logits_list[0] must be an fp32 [B, T, V] tensor")
    dev, B, T = lg0.device, int(lg0.shape[0]), int(lg0.shape[1])
    Vs = []
    for p in range(P):
        lg = logits_list[p]
        if not isinstance(lg, torch.Tensor) or lg.dim() != 3 or lg.dtype != torch.float32 or (
                tuple(lg.shape[:2]) != (B, T)) or lg.shape[2] < 1:
            raise ValueError(f"position_metrics: logits_list[{p}] must be an fp32 [{B}, {T}, V] tensor")
        if lg.device.type != "cuda" or lg.device != dev:
            raise ValueError(f"position_metrics: logits_list[{p}] must be on the GPU of logits_list[0] (the metrics run "
                             "in HIP kernels; there is no CPU path)")
        if not lg.is_contiguous():
            raise ValueError(f"position_metrics: logits_list[{p}] must be contiguous")
        V = int(lg.shape[2])
        if V > MAX_V:
            raise ValueError(f"position_metrics: logits_list[{p}] has V = {V}, above {MAX_V}")
        Vs.append(V)
        for name, t in (("xb_list", xb_list[p]), ("yb_list", yb_list[p])):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != (B, T):
                raise ValueError(f"position_metrics: {name}[{p}] must be an int64 [{B}, {T}] tensor")
            if t.device != dev:
                raise ValueError(f"position_metrics: {name}[{p}] must be on the GPU of the logits")
            if not t.is_contiguous():
                raise ValueError(f"position_metrics: {name}[{p}] must be contiguous")
            if token_range and t.numel() and (int(t.min()) < 0 or int(t.max()) >= V):
                raise ValueError(f"position_metrics: {name}[{p}] holds tokens outside 0..{V - 1}")
        v = values[p]
        if v is not None:
            if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or tuple(v.shape) != (V,):
                raise ValueError(f"position_metrics: values[{p}] must be None or an fp64 [{V}] tensor")
            if v.device != dev:
                raise ValueError(f"position_metrics: values[{p}] must be on the GPU of the logits")
            if not v.is_contiguous():
                raise ValueError(f"position_metrics: values[{p}] must be contiguous")
    if B * T >= 2 ** 31:
        raise ValueError(f"position_metrics: logits_list holds {B} x {T} rows, 2^31 or more")
    return dev, B, T, Vs


class EvalLaunch:
    """The host arrays of mmt_eval_positions over P problems (raw addresses; values / rec 0 = absent), made once."""

    def __init__(self, V, is_percent):
        P = self.P = len(V)
        n = max(1, P)
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.is_percent = (ctypes.c_int32 * n)(*[1 if x else 0 for x in is_percent])
        self.logits = (ctypes.c_void_p * n)()
        self.xb = (ctypes.c_void_p * n)()
        self.yb = (ctypes.c_void_p * n)()
        self.values = (ctypes.c_void_p * n)()
        self.rec = (ctypes.c_void_p * n)()
        self.pos = (ctypes.c_void_p * n)()
        self.rel = (ctypes.c_void_p * n)()
        self.pit = (ctypes.c_void_p * n)()

    def scratch_bytes(self, L, batch, T, bins):
        n = L.mmt_eval_positions_scratch_bytes(self.P, int(batch), int(T), int(bins))
        if n < 0:
            raise ValueError(f"position_metrics: {batch} x {T} rows with {bins} bins is a shape the entry refuses")
        return int(n)

    def run(self, L, stream, batch, T, t_begin, bins, accumulate, scratch_ptr, scratch_bytes):
        rc = L.mmt_eval_positions(stream, self.P, batch, T, t_begin, bins, 1 if accumulate else 0, self.V, self.logits,
                                  self.xb, self.yb, self.values, self.is_percent, self.rec, self.pos, self.rel,
                                  self.pit, scratch_ptr, scratch_bytes)
        if rc != 0:
            raise ML.MmtError(f"mmt_eval_positions failed (status {rc})")


def _table_views(flat, P, T, bins):
    """The tables of P problems as views of one flat fp64 buffer: per problem pos [T, 8], rel [3, bins, 3], pit
    [bins], in that order."""
    each = T * 8 + 10 * bins
    out = []
    for p in range(P):
        o = p * each
        out.append((flat[o:o + T * 8].view(T, 8), flat[o + T * 8:o + T * 8 + 9 * bins].view(3, bins, 3),
                    flat[o + T * 8 + 9 * bins:o + each].view(bins)))
    return out


def position_metrics(logits_list, xb_list, yb_list, values, is_percent, t_begin=0, bins=10, records=False):
    """One mmt_eval_positions call over P modalities: logits_list holds P contiguous fp32 [B, T, V_p] tensors on one
    GPU, xb_list / yb_list P contiguous int64 [B, T] tensors (the token at position t and the one that followed it),
    values P entries, each an fp64 [V_p] device tensor or None (a non-numeric vocabulary: no direction), is_percent P
    bools. Rows with t >= t_begin are scored. Returns a list of P dicts of device tensors: "pos" fp64 [T, 8]
    (POS_FIELDS), "rel" fp64 [3, bins, 3] (per direction and bin: count, sum of the probability, realised), "pit" fp64
    [bins], and with records=True "rec" fp64 [B, T, 8] (REC_FIELDS; rows before t_begin hold NaN). ValueError, naming
    the argument, for shapes or dtypes that do not match, non-contiguous inputs, CPU tensors and tokens outside the
    vocabulary (this check reads the tokens' extremes back; PositionMetrics.add leaves it out)."""
    _check_settings(t_begin, bins)
    dev, B, T, Vs = _check_inputs(logits_list, xb_list, yb_list, values, is_percent, token_range=True)
    _check_settings(t_begin, bins, T)
    P = len(Vs)
    if P == 0:
        return []
    flat = torch.zeros(P * (T * 8 + 10 * bins), dtype=torch.float64, device=dev)  # zeros: B == 0 launches nothing
    views = _table_views(flat, P, T, bins)
    el = EvalLaunch(Vs, is_percent)
    recs = [torch.full((B, T, 8), float("nan"), dtype=torch.float64, device=dev) if records else None
            for _ in range(P)]
    for p in range(P):
        el.logits[p], el.xb[p], el.yb[p] = logits_list[p].data_ptr(), xb_list[p].data_ptr(), yb_list[p].data_ptr()
        el.values[p] = values[p].data_ptr() if values[p] is not None else None
        el.rec[p] = recs[p].data_ptr() if records and recs[p].numel() else None
        el.pos[p], el.rel[p], el.pit[p] = (x.data_ptr() for x in views[p])
    L = ML.lib()
    nbytes = el.scratch_bytes(L, B, T, bins)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        el.run(L, ML.stream_ptr(dev), B, T, t_begin, bins, False, scratch.data_ptr(), nbytes)
    out = []
    for p in range(P):
        d = {"pos": views[p][0], "rel": views[p][1], "pit": views[p][2]}
        if records:
            d["rec"] = recs[p]
        out.append(d)
    return out


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def derive(pos, rel, pit, t_begin=0):
    """The numbers of one modality from its tables (numpy fp64: pos [T, 8], rel [3, bins, 3], pit [bins]). Returns a
    dict: the tables; rows, directed, wins, losses; accuracy (wins / (wins + losses)) overall, per position [T] (NaN
    where a position holds no row with a direction) and per quarter of the context length [4]; nll (mean -log p of
    the token that came); top1 (rate of rank 0); certainty (mean mass on the predicted direction); realised_mass;
    ece, per direction sum_k n_k / N |mean P_d - realised rate| over the bins; pit_hist (the PIT counts over their
    sum). A mean over nothing is NaN."""
    pos, rel, pit = np.asarray(pos, np.float64), np.asarray(rel, np.float64), np.asarray(pit, np.float64)
    T = pos.shape[0]
    tot = pos.sum(axis=0) if T else np.zeros(8)
    rows, wins, losses, directed = int(tot[0]), int(tot[1]), int(tot[2]), int(tot[6])
    with np.errstate(all="ignore"):
        acc_t = np.where(pos[:, 1] + pos[:, 2] > 0, pos[:, 1] / (pos[:, 1] + pos[:, 2]), np.nan)
    quarters = []
    for k in range(4):
        lo, hi = max((k * T) // 4, t_begin), ((k + 1) * T) // 4
        seg = pos[lo:hi] if hi > lo else pos[:0]
        quarters.append(_ratio(seg[:, 1].sum(), seg[:, 1].sum() + seg[:, 2].sum()))
    ece = {}
    for d, name in enumerate(DIRECTIONS):
        n = rel[d, :, 0].sum()
        ece[name] = _ratio(np.abs(rel[d, :, 1] - rel[d, :, 2]).sum(), n)
    return {"pos": pos, "rel": rel, "pit": pit, "t_begin": t_begin, "rows": rows, "directed": directed, "wins": wins,
            "losses": losses, "accuracy": _ratio(wins, wins + losses), "accuracy_per_position": acc_t,
            "accuracy_per_quarter": quarters, "nll": _ratio(tot[4], rows), "top1": _ratio(tot[5], rows),
            "certainty": _ratio(tot[3], directed), "realised_mass": _ratio(tot[7], directed), "ece": ece,
            "pit_hist": pit / pit.sum() if pit.sum() > 0 else np.full(pit.shape, np.nan)}


def _pct(x, digits=1):
    return "n/a" if x != x else f"{round(x * 100, digits)}%"


def summary_text(r):
    """One modality's line, without its name: correct/total and accuracy over all positions, mean NLL, top-1 rate,
    ECE of p_up and p_down, accuracy per quarter of the context length."""
    total = r["wins"] + r["losses"]
    head = f"{r['wins']}/{total} ({_pct(r['accuracy'])})" if total > 0 else "No directional predictions"
    nll = "n/a" if r["nll"] != r["nll"] else f"{r['nll']:.4f}"
    ece = " ".join(f"{k} {'n/a' if r['ece'][k] != r['ece'][k] else format(r['ece'][k], '.4f')}" for k in ("up", "down"))
    quarters = " ".join(_pct(q) for q in r["accuracy_per_quarter"])
    return f"{head} | NLL {nll} | top-1 {_pct(r['top1'])} | ECE {ece} | quarters {quarters}"


class PositionMetrics:
    """Tables accumulated on the device over many evaluation batches. values: P entries, each an fp64 [V_p] device
    tensor or None; is_percent: P bools. `add` checks its inputs on the host (shapes, dtypes, layout, device; not the
    tokens' range: a row with a token outside the vocabulary is dead on the device), launches with accumulate = 1 and
    does not sync; the first `add` fixes B, T and the V_p. `result` is one device-to-host read."""

    def __init__(self, values, is_percent, t_begin=0, bins=10):
        _check_settings(t_begin, bins)
        if not isinstance(values, (list, tuple)) or not isinstance(is_percent, (list, tuple)) or (
                len(values) != len(is_percent)):
            raise ValueError("PositionMetrics: values and is_percent must be lists of one length")
        self.values, self.is_percent = list(values), [bool(x) for x in is_percent]
        self.t_begin, self.bins = t_begin, bins
        self.P = len(self.values)
        self.batches = 0
        self._shape = None

    def _setup(self, dev, B, T, Vs):
        _check_settings(self.t_begin, self.bins, T)
        self._shape = (dev, B, T, tuple(Vs))
        self._flat = torch.zeros(self.P * (T * 8 + 10 * self.bins), dtype=torch.float64, device=dev)
        self._views = _table_views(self._flat, self.P, T, self.bins)
        self._launch = el = EvalLaunch(Vs, self.is_percent)
        for p in range(self.P):
            el.values[p] = self.values[p].data_ptr() if self.values[p] is not None else None
            el.pos[p], el.rel[p], el.pit[p] = (x.data_ptr() for x in self._views[p])
        self._lib = ML.lib()
        self._nbytes = el.scratch_bytes(self._lib, B, T, self.bins)
        self._scratch = torch.empty(max(self._nbytes, 16), dtype=torch.uint8, device=dev)

    def add(self, logits_list, xb_list, yb_list):
        if len(logits_list) != self.P:
            raise ValueError(f"PositionMetrics.add: logits_list must hold {self.P} tensors")
        dev, B, T, Vs = _check_inputs(logits_list, xb_list, yb_list, self.values, self.is_percent, token_range=False)
        if self.P == 0:
            return
        if self._shape is None:
            self._setup(dev, B, T, Vs)
        elif self._shape != (dev, B, T, tuple(Vs)):
            raise ValueError(f"PositionMetrics.add: logits_list does not match the first batch's device and shapes "
                             f"(B {self._shape[1]}, T {self._shape[2]}, V {list(self._shape[3])})")
        el = self._launch
        for p in range(self.P):
            el.logits[p], el.xb[p], el.yb[p] = logits_list[p].data_ptr(), xb_list[p].data_ptr(), yb_list[p].data_ptr()
        with torch.cuda.device(dev):
            el.run(self._lib, ML.stream_ptr(dev), B, T, self.t_begin, self.bins, True, self._scratch.data_ptr(),
                   self._nbytes)
        self.batches += 1

    def result(self):
        """A list of P dicts (`derive`), from one device-to-host read of all tables. Before any `add`: []."""
        if self._shape is None:
            return []
        T = self._shape[2]
        host = self._flat.cpu()
        return [derive(pos.numpy(), rel.numpy(), pit.numpy(), self.t_begin)
                for pos, rel, pit in _table_views(host, self.P, T, self.bins)]

    def summary_lines(self, name, result=None):
        """The lines to print, one per modality: `name` is a list of P names (or one string when P == 1)."""
        names = [name] if isinstance(name, str) else list(name)
        res = self.result() if result is None else result
        if len(names) != len(res):
            raise ValueError(f"PositionMetrics.summary_lines: name must hold {len(res)} names, got {len(names)}")
        return [f"  - {n:<30}{summary_text(r)}" for n, r in zip(names, res)]


# ------------------------------------------------------------------------------------------
# Calibrated temperatures (mmt_eval_temperatures): NLL and reliability on a grid of temperatures, the fit
# ------------------------------------------------------------------------------------------
MAX_TEMPERATURES = 32
TEMP_REC_FIELDS = ("logprob", "p_down", "p_flat", "p_up")  # rec[b, t, k, f]


def default_temperatures():
    """The default grid: the 17 fp32 values 2^((k - 8) / 4), k = 0..16 (0.25 .. 4, 1.0 exactly at k = 8)."""
    return np.array([2.0 ** ((k - 8) / 4.0) for k in range(17)], dtype=np.float32)


def _check_temperatures(temperatures):
    """The grid as an fp32 numpy array: 1..32 finite values > 0, strictly ascending (as fp32)."""
    t = default_temperatures() if temperatures is None else np.asarray(temperatures)
    if t.ndim != 1 or not 1 <= t.size <= MAX_TEMPERATURES or t.dtype.kind not in "fiu":
        raise ValueError(f"temperature_metrics: temperatures must hold 1..{MAX_TEMPERATURES} numbers")
    with np.errstate(all="ignore"):
        t = t.astype(np.float32)
    if not (np.isfinite(t).all() and (t > 0).all() and (np.diff(t) > 0).all()):
        raise ValueError("temperature_metrics: temperatures must be finite, > 0 and strictly ascending in fp32")
    return t


class TempLaunch:
    """The host arrays of mmt_eval_temperatures over P problems (raw addresses; values / rec 0 = absent), made once."""

    def __init__(self, V, is_percent, temperatures):
        P = self.P = len(V)
        n = max(1, P)
        self.K = len(temperatures)
        self.temperatures = (ctypes.c_float * self.K)(*[float(t) for t in temperatures])
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.is_percent = (ctypes.c_int32 * n)(*[1 if x else 0 for x in is_percent])
        self.logits, self.xb, self.yb, self.values, self.rec, self.sum, self.rel = (
            (ctypes.c_void_p * n)() for _ in range(7))

    def scratch_bytes(self, L, batch, T, bins):
        n = L.mmt_eval_temperatures_scratch_bytes(self.P, int(batch), int(T), int(bins), self.K)
        if n < 0:
            raise ValueError(f"temperature_metrics: {batch} x {T} rows with {bins} bins is a shape the entry refuses")
        return int(n)

    def run(self, L, stream, batch, T, t_begin, bins, accumulate, scratch_ptr, scratch_bytes):
        rc = L.mmt_eval_temperatures(stream, self.P, batch, T, t_begin, bins, 1 if accumulate else 0, self.K,
                                     self.temperatures, self.V, self.logits, self.xb, self.yb, self.values,
                                     self.is_percent, self.rec, self.sum, self.rel, scratch_ptr, scratch_bytes)
        if rc != 0:
            raise ML.MmtError(f"mmt_eval_temperatures failed (status {rc})")


def _temp_views(flat, P, K, bins):
    """The tables of P problems as views of one flat fp64 buffer: per problem sum [K, 2], rel [K, 3, bins, 3]."""
    each = K * (2 + 9 * bins)
    return [(flat[p * each:p * each + 2 * K].view(K, 2), flat[p * each + 2 * K:(p + 1) * each].view(K, 3, bins, 3))
            for p in range(P)]


def temperature_metrics(logits_list, xb_list, yb_list, values, is_percent, temperatures=None, t_begin=0, bins=10,
                        records=False):
    """One mmt_eval_temperatures call over P modalities; the inputs are position_metrics' (and checked as there),
    temperatures 1..32 finite values > 0, strictly ascending (default: default_temperatures()). Returns a list of P
    dicts of device tensors: "sum" fp64 [K, 2] (per temperature: live rows, the sum of -log p of the token that came),
    "rel" fp64 [K, 3, bins, 3] (per temperature, direction and bin: count, sum of the probability, realised), and
    with records=True "rec" fp64 [B, T, K, 4] (TEMP_REC_FIELDS; rows before t_begin hold NaN)."""
    temps = _check_temperatures(temperatures)
    _check_settings(t_begin, bins)
    dev, B, T, Vs = _check_inputs(logits_list, xb_list, yb_list, values, is_percent, token_range=True)
    _check_settings(t_begin, bins, T)
    P, K = len(Vs), len(temps)
    if P == 0:
        return []
    flat = torch.zeros(P * K * (2 + 9 * bins), dtype=torch.float64, device=dev)  # zeros: B == 0 launches nothing
    views = _temp_views(flat, P, K, bins)
    tl = TempLaunch(Vs, is_percent, temps)
    recs = [torch.full((B, T, K, 4), float("nan"), dtype=torch.float64, device=dev) if records else None
            for _ in range(P)]
    for p in range(P):
        tl.logits[p], tl.xb[p], tl.yb[p] = logits_list[p].data_ptr(), xb_list[p].data_ptr(), yb_list[p].data_ptr()
        tl.values[p] = values[p].data_ptr() if values[p] is not None else None
        tl.rec[p] = recs[p].data_ptr() if records and recs[p].numel() else None
        tl.sum[p], tl.rel[p] = (x.data_ptr() for x in views[p])
    L = ML.lib()
    nbytes = tl.scratch_bytes(L, B, T, bins)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        tl.run(L, ML.stream_ptr(dev), B, T, t_begin, bins, False, scratch.data_ptr(), nbytes)
    out = []
    for p in range(P):
        d = {"sum": views[p][0], "rel": views[p][1]}
        if records:
            d["rec"] = recs[p]
        out.append(d)
    return out


def fit_temperature(temperatures, rows, nll_sum):
    """The temperature that minimises the mean NLL measured on a grid, in host fp64: (tau, k_star, at_bound).
    mean_k = nll_sum[k] / rows, a non-finite mean counting as +inf; no rows or no finite mean: (nan, -1, True). k* is
    the lowest index of the minimum. K == 1 or k* at either end of the grid: (tau_k*, k*, True): the minimum may lie
    outside. A neighbour without a finite mean: (tau_k*, k*, False). Otherwise the vertex of the parabola through
    (ln tau, mean) at k* - 1, k*, k* + 1 (NLL is convex in 1 / tau and smooth in ln tau); ln tau_k* instead when the
    denominator is 0 or the vertex is not finite or leaves [ln tau_{k*-1}, ln tau_{k*+1}]."""
    tau = [float(t) for t in temperatures]
    K = len(tau)
    rows = float(rows)
    if not rows > 0:
        return float("nan"), -1, True
    with np.errstate(all="ignore"):
        mean = [float(s) / rows for s in nll_sum]
    mean = [m if np.isfinite(m) else float("inf") for m in mean]
    if not any(np.isfinite(m) for m in mean):
        return float("nan"), -1, True
    ks = min(range(K), key=lambda k: (mean[k], k))
    if K == 1 or ks == 0 or ks == K - 1:
        return tau[ks], ks, True
    if not (np.isfinite(mean[ks - 1]) and np.isfinite(mean[ks + 1])):
        return tau[ks], ks, False
    x0, x1, x2 = (float(np.log(tau[k])) for k in (ks - 1, ks, ks + 1))
    y0, y1, y2 = mean[ks - 1], mean[ks], mean[ks + 1]
    den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
    xs = x1
    if den != 0.0:
        with np.errstate(all="ignore"):
            v = x1 - 0.5 * ((x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)) / den
        if np.isfinite(v) and x0 <= v <= x2:
            xs = float(v)
    return float(np.exp(xs)), ks, False


def derive_temperature(sum, rel, temperatures):
    """The numbers of one modality from its tables (numpy fp64: sum [K, 2], rel [K, 3, bins, 3]). Returns a dict: the
    tables and the grid; rows; nll [K] (the mean per temperature, NaN without rows); ece {direction: [K]} (`derive`'s
    formula per temperature); tau, k_star, at_bound (`fit_temperature`); k_one (the index of the grid point equal to
    1.0, None if absent)."""
    sum, rel = np.asarray(sum, np.float64), np.asarray(rel, np.float64)
    temps = np.asarray(temperatures, np.float32)
    K = len(temps)
    rows = float(sum[0, 0]) if K else 0.0
    nll = np.array([_ratio(sum[k, 1], sum[k, 0]) for k in range(K)])
    ece = {name: np.array([_ratio(np.abs(rel[k, d, :, 1] - rel[k, d, :, 2]).sum(), rel[k, d, :, 0].sum())
                           for k in range(K)]) for d, name in enumerate(DIRECTIONS)}
    tau, ks, at_bound = fit_temperature(temps, rows, sum[:, 1])
    one = np.nonzero(temps == np.float32(1.0))[0]
    return {"sum": sum, "rel": rel, "temperatures": temps, "rows": int(rows), "nll": nll, "ece": ece, "tau": tau,
            "k_star": ks, "at_bound": at_bound, "k_one": int(one[0]) if len(one) else None}


def temperature_summary_text(r):
    """One modality's line, without its name: the fitted temperature (marked when the minimum sits on the grid's
    edge), then NLL and the ECE of p_up / p_down at temperature 1 -> at the grid point of the minimum."""
    if r["k_star"] < 0:
        return "no fit (no scored row)"

    def pair(a):
        f = lambda k: "n/a" if k is None or a[k] != a[k] else f"{a[k]:.4f}"
        return f"{f(r['k_one'])} -> {f(r['k_star'])}"

    mark = " (at the grid's edge)" if r["at_bound"] else ""
    return (f"tau* {r['tau']:.4f}{mark} | NLL {pair(r['nll'])} | ECE up {pair(r['ece']['up'])} "
            f"down {pair(r['ece']['down'])}")


class TemperatureFit:
    """The tables of mmt_eval_temperatures accumulated on the device over many evaluation batches. values, is_percent
    as PositionMetrics'; temperatures as temperature_metrics'. `add` checks its inputs on the host (not the tokens'
    range), launches with accumulate = 1 and does not sync; the first `add` fixes B, T and the V_p. `result` is one
    device-to-host read."""

    def __init__(self, values, is_percent, temperatures=None, t_begin=0, bins=10):
        _check_settings(t_begin, bins)
        if not isinstance(values, (list, tuple)) or not isinstance(is_percent, (list, tuple)) or (
                len(values) != len(is_percent)):
            raise ValueError("TemperatureFit: values and is_percent must be lists of one length")
        self._temps = _check_temperatures(temperatures)
        self.values, self.is_percent = list(values), [bool(x) for x in is_percent]
        self.t_begin, self.bins = t_begin, bins
        self.P = len(self.values)
        self.batches = 0
        self._shape = None

    def temperatures(self):
        """The grid, fp32 numpy [K]."""
        return self._temps.copy()

    def _setup(self, dev, B, T, Vs):
        _check_settings(self.t_begin, self.bins, T)
        self._shape = (dev, B, T, tuple(Vs))
        K = len(self._temps)
        self._flat = torch.zeros(self.P * K * (2 + 9 * self.bins), dtype=torch.float64, device=dev)
        self._views = _temp_views(self._flat, self.P, K, self.bins)
        self._launch = tl = TempLaunch(Vs, self.is_percent, self._temps)
        for p in range(self.P):
            tl.values[p] = self.values[p].data_ptr() if self.values[p] is not None else None
            tl.sum[p], tl.rel[p] = (x.data_ptr() for x in self._views[p])
        self._lib = ML.lib()
        self._nbytes = tl.scratch_bytes(self._lib, B, T, self.bins)
        self._scratch = torch.empty(max(self._nbytes, 16), dtype=torch.uint8, device=dev)

    def add(self, logits_list, xb_list, yb_list):
        if len(logits_list) != self.P:
            raise ValueError(f"TemperatureFit.add: logits_list must hold {self.P} tensors")
        dev, B, T, Vs = _check_inputs(logits_list, xb_list, yb_list, self.values, self.is_percent, token_range=False)
        if self.P == 0:
            return
        if self._shape is None:
            self._setup(dev, B, T, Vs)
        elif self._shape != (dev, B, T, tuple(Vs)):
            raise ValueError(f"TemperatureFit.add: logits_list does not match the first batch's device and shapes "
                             f"(B {self._shape[1]}, T {self._shape[2]}, V {list(self._shape[3])})")
        tl = self._launch
        for p in range(self.P):
            tl.logits[p], tl.xb[p], tl.yb[p] = logits_list[p].data_ptr(), xb_list[p].data_ptr(), yb_list[p].data_ptr()
        with torch.cuda.device(dev):
            tl.run(self._lib, ML.stream_ptr(dev), B, T, self.t_begin, self.bins, True, self._scratch.data_ptr(),
                   self._nbytes)
        self.batches += 1

    def result(self):
        """A list of P dicts (`derive_temperature`), from one device-to-host read of all tables. Before any `add`:
        []."""
        if self._shape is None:
            return []
        host = self._flat.cpu()
        return [derive_temperature(s.numpy(), r.numpy(), self._temps)
                for s, r in _temp_views(host, self.P, len(self._temps), self.bins)]

    def summary_lines(self, name, result=None):
        """The lines to print, one per modality: `name` is a list of P names (or one string when P == 1)."""
        names = [name] if isinstance(name, str) else list(name)
        res = self.result() if result is None else result
        if len(names) != len(res):
            raise ValueError(f"TemperatureFit.summary_lines: name must hold {len(res)} names, got {len(names)}")
        return [f"  - {n:<30}{temperature_summary_text(r)}" for n, r in zip(names, res)]


# ------------------------------------------------------------------------------------------
# Scores of horizon forecasts (mmt_horizon_score) over many evaluation batches
# ------------------------------------------------------------------------------------------
ROLLOUT_TABLES = ("agg", "aggq", "aggb", "pit_hist")


def _div(a, n):
    with np.errstate(all="ignore"):
        return np.where(n > 0, a / np.where(n > 0, n, 1.0), np.nan)


def derive_rollout(agg, aggq, aggb, pit, quantiles, barriers=()):
    """The numbers of one modality per step from its tables (numpy fp64: agg [N, 10], aggq [N, Q, 2], aggb [N, nb, 3],
    pit [N, bins]; include/mmt.h, rule 8 of mmt_horizon_score). Returns a dict of arrays over the N steps: count;
    crps (mean) and skill = 1 - sum CRPS / sum |x*| (against a forecast of no change; NaN where nothing moved); mae
    and rmse of the forecast mean, spread (the root of the mean forecast variance, to set against rmse); coverage [N,
    Q] (the rate of x* <= q_k, to set against quantiles[k]) and pinball [N, Q]; brier, hit_forecast, hit_observed [N,
    nb] (the mean Brier score and the two sides of the reliability of a barrier's probability); sign_accuracy and
    step_accuracy (hits of the most likely sign of the cumulative change / of the step), sign_mass and step_mass (the
    mean mass on what came); pit_hist [N, bins] (the counts over their sum) and pit_deviation (half the L1 distance of
    pit_hist from uniform: 0 for a calibrated forecast, towards 1 for a useless one). A mean over nothing is NaN."""
    agg, aggq = np.asarray(agg, np.float64), np.asarray(aggq, np.float64)
    aggb, pit = np.asarray(aggb, np.float64), np.asarray(pit, np.float64)
    n = agg[:, 0]
    bins = pit.shape[1]
    hist = _div(pit, pit.sum(axis=1, keepdims=True))
    return {"agg": agg, "aggq": aggq, "aggb": aggb, "pit": pit, "quantiles": [float(q) for q in quantiles],
            "barriers": [float(u) for u in barriers], "count": n, "crps": _div(agg[:, 1], n),
            "skill": 1.0 - _div(agg[:, 1], agg[:, 2]), "mae": _div(agg[:, 3], n), "rmse": np.sqrt(_div(agg[:, 4], n)),
            "spread": np.sqrt(_div(agg[:, 9], n)), "coverage": _div(aggq[:, :, 1], n[:, None]),
            "pinball": _div(aggq[:, :, 0], n[:, None]), "brier": _div(aggb[:, :, 0], n[:, None]),
            "hit_forecast": _div(aggb[:, :, 1], n[:, None]), "hit_observed": _div(aggb[:, :, 2], n[:, None]),
            "sign_mass": _div(agg[:, 5], n), "sign_accuracy": _div(agg[:, 6], n), "step_mass": _div(agg[:, 7], n),
            "step_accuracy": _div(agg[:, 8], n), "pit_hist": hist,
            "pit_deviation": 0.5 * np.abs(hist - 1.0 / bins).sum(axis=1)}


def rollout_steps(N):
    """The steps a summary shows: 1, N / 2 and N (as indices 0, N // 2 - 1, N - 1; fewer where they coincide)."""
    return sorted({0, max(N // 2 - 1, 0), N - 1}) if N > 0 else []


def rollout_summary_text(r, steps=None):
    """One modality's line, without its name: per shown step the CRPS skill against no change, the coverage of every
    quantile level and the accuracy of the most likely sign of the cumulative change."""
    N = len(r["count"])
    parts = []
    for j in (rollout_steps(N) if steps is None else steps):
        if not r["count"][j] > 0:
            parts.append(f"step {j + 1}: no scored prompt")
            continue
        sk = r["skill"][j]
        cov = " ".join(f"{_pct(q, 2)}:{_pct(float(c))}" for q, c in zip(r["quantiles"], r["coverage"][j]))
        parts.append(f"step {j + 1}: skill {'n/a' if sk != sk else format(sk, '.3f')} | coverage {cov} | "
                     f"direction {_pct(float(r['sign_accuracy'][j]))} | PIT dev {r['pit_deviation'][j]:.3f}")
    return " || ".join(parts) if parts else "no steps"


class RolloutMetrics:
    """The tables of mmt_horizon_score accumulated on the device over many evaluation batches. `add` takes what
    generate(realised=) returned last, {modality: score dict}, and adds each modality's four tables to its own, which
    the first `add` allocates (one fp64 addition per cell, on the device, no sync); every later `add` must bring the
    same modalities and table shapes. quantiles / barriers: the levels and {modality: barriers} the scores were made
    with, for the report. `result` is one device-to-host read."""

    def __init__(self, quantiles=(0.05, 0.5, 0.95), barriers=None):
        self.quantiles = [float(q) for q in quantiles]
        self.barriers = dict(barriers or {})
        self.batches = 0
        self._keys = None

    def add(self, scores):
        if not isinstance(scores, dict) or not scores or any(
                not isinstance(d, dict) or any(k not in d for k in ROLLOUT_TABLES) for d in scores.values()):
            raise ValueError("RolloutMetrics.add: scores must be the {modality: dict} generate(realised=) returns")
        keys = sorted(scores)
        shapes = [tuple(tuple(scores[i][k].shape) for k in ROLLOUT_TABLES) for i in keys]
        if any(s[1][1] != len(self.quantiles) for s in shapes):
            raise ValueError(f"RolloutMetrics.add: the scores hold {shapes[0][1][1]} quantile levels, this object "
                             f"{len(self.quantiles)}")
        if self._keys is None:
            self._keys, self._shapes = keys, shapes
            sizes = [[int(np.prod(s)) for s in sh] for sh in shapes]
            dev = scores[keys[0]]["agg"].device
            self._flat = torch.zeros(sum(sum(s) for s in sizes), dtype=torch.float64, device=dev)
            self._views, o = [], 0
            for sh, sz in zip(shapes, sizes):
                row = []
                for s, n in zip(sh, sz):
                    row.append(self._flat[o:o + n].view(s))
                    o += n
                self._views.append(row)
        elif keys != self._keys or shapes != self._shapes:
            raise ValueError("RolloutMetrics.add: the scores do not match the first batch's modalities and shapes")
        for row, i in zip(self._views, keys):
            for dst, k in zip(row, ROLLOUT_TABLES):
                dst.add_(scores[i][k])
        self.batches += 1

    def result(self):
        """{modality: derive_rollout(...)} from one device-to-host read of all tables. Before any `add`: {}."""
        if self._keys is None:
            return {}
        host = self._flat.cpu()
        out, o = {}, 0
        for i, sh in zip(self._keys, self._shapes):
            tabs = []
            for s in sh:
                n = int(np.prod(s))
                tabs.append(host[o:o + n].view(s).numpy())
                o += n
            out[i] = derive_rollout(*tabs, self.quantiles, self.barriers.get(i, ()))
        return out

    def summary_lines(self, names, result=None):
        """The lines to print, one per modality: `names` is {modality: name} or a list in ascending modality order."""
        res = self.result() if result is None else result
        if not isinstance(names, dict):
            names = list(names)
            if len(names) != len(res):
                raise ValueError(f"RolloutMetrics.summary_lines: names must hold {len(res)} names, got {len(names)}")
            names = dict(zip(sorted(res), names))
        return [f"  - {names[i]:<30}{rollout_summary_text(res[i])}" for i in sorted(res)]
