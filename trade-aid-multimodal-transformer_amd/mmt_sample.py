"""Device-side sampling (include/mmt.h: mmt_sample): temperature, top-k, top-p, draws keyed by
(seed, row, position) and the log-probability of what was drawn, one launch for all rows, no sync.

    tok = mmt_sample.sample(logits, temperature=0.8, top_k=50, top_p=0.9, seed=1234, pos=n)
    tok, lp = mmt_sample.sample(logits, ..., return_logprobs=True)

`model.generate(..., temperature=..., top_k=..., top_p=..., seed=...)` runs on `MultiLaunch` below (one problem:
bit for bit mmt_sample); `sample` is the entry for users with their own decode loop. The rule is stated in include/mmt.h and INTEGRATION.md.

Several heads of one step in one launch (mmt_sample_multi), as the joint rollouts of generate use it:

    toks = mmt_sample.sample_multi([logits_0, logits_2], temperature=[0.8, 1.0], top_k=50,
                                   seeds=[mmt_sample.modality_seed(1234, i) for i in (0, 2)], pos=n)

Evidence of given tokens (generate's evidence=): the score of a token under a head (mmt_score_multi) and one
particle-filter step over the S paths of each prompt (mmt_resample):

    lps = mmt_sample.score_multi([logits_1], [tokens_1])
    ancestors, resampled = mmt_sample.resample(lps_list, logw, log_evidence, samples=S, ess_threshold=0.5,
                                               seed=1234, pos=n)

Forecast distributions (generate's forecast=): per prompt the mixture of the laws its paths draw their next token from,
weighted as mmt_resample weighs them (mmt_forecast_multi), and the summaries of stored pmf rows (mmt_pmf_stats):

    pmfs, ess, live = mmt_sample.forecast_multi([logits_0], samples=S, temperature=0.8, top_k=50, logprobs=lps_list)
    stats, qtok = mmt_sample.pmf_stats(pmfs, values=[vocab_values_0], is_percent=True, quantiles=(0.05, 0.5, 0.95))

Horizon forecasts (generate's horizon=): where a series stands after j new steps, from the finished paths and their
log-weights (mmt_horizon_stats): cumulative change per path, its weighted moments, quantiles and barrier hits:

    hz = mmt_sample.horizon_stats([seqs_0[:, n0:]], samples=S, values=[vocab_values_0], is_percent=True,
                                  logw=ev["log_weights"], barriers=[[-2.0, 2.0]])
"""
import ctypes

import torch

import mmt_lib as ML

MASK64 = 2 ** 64 - 1


def check_settings(temperature, top_k, top_p):
    """The three settings as the C entry takes them (None: 1.0 / off / off); ValueError for what it would refuse."""
    t = 1.0 if temperature is None else float(temperature)
    k = 0 if top_k is None else int(top_k)
    p = 1.0 if top_p is None else float(top_p)
    if not t >= 0.0:
        raise ValueError(f"temperature must be >= 0 (0 = greedy), got {temperature!r}")
    if k < 0:
        raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k!r}")
    if p != p:
        raise ValueError("top_p must not be NaN")
    return t, k, p


def device_seed(dev):
    """A 64-bit seed from the device generator's seed and Philox offset (the offset is advanced by 4, as the
    dropout seeds of model.py do); torch's CPU generator is never touched."""
    seed, off = 0, 0
    try:
        gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        seed = int(gen.initial_seed())
        off = int(gen.get_offset())
        gen.set_offset(off + 4)
    except (AttributeError, RuntimeError, IndexError):
        pass
    x = (seed * 0x9E3779B97F4A7C15 + off * 0xBF58476D1CE4E5B9 + 0x53414D50) & MASK64
    x ^= x >> 31
    x = (x * 0x94D049BB133111EB) & MASK64
    return int(x ^ (x >> 29)) & MASK64


def launch(L, stream, batch, V, logits_ptr, row_stride, t, k, p, seed, row0, pos, tok_ptr, tok_stride, compact_ptr,
           lp_ptr, lp_stride):
    """mmt_sample with raw addresses (ints; 0 = absent). Raises MmtError on a non-zero status."""
    rc = L.mmt_sample(stream, batch, V, logits_ptr, row_stride, t, k, p, seed & MASK64, row0, pos, tok_ptr, tok_stride,
                      compact_ptr or None, lp_ptr or None, lp_stride)
    if rc != 0:
        raise ML.MmtError(f"mmt_sample failed (status {rc})")


def sample(logits, *, temperature=1.0, top_k=0, top_p=1.0, seed, pos, row0=0, return_logprobs=False):
    """One token per row of `logits` (fp32 [B, V] on the GPU; rows may be strided, e.g. `full[:, -1, :]` of a
    [B, T, V] tensor, but elements of a row must be contiguous). Returns int64 [B], with return_logprobs also
    fp32 [B]. `pos` is the sequence position being written and `row0` the index of the first row (for callers
    that split a batch): the draw of row b depends on (seed, row0 + b, pos) and on that row's logits alone."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.device.type != "cuda":
        raise ValueError("sample: logits must be an fp32 [B, V] tensor on the GPU")
    B, V = logits.shape
    if V < 1 or (V > 1 and logits.stride(1) != 1) or (B > 1 and logits.stride(0) < V):
        raise ValueError("sample: the elements of a row must be contiguous and rows must not overlap")
    t, k, p = check_settings(temperature, top_k, top_p)
    dev = logits.device
    tok = torch.empty(B, dtype=torch.int64, device=dev)
    lp = torch.empty(B, dtype=torch.float32, device=dev) if return_logprobs else None
    with torch.cuda.device(dev):
        launch(ML.lib(), ML.stream_ptr(dev), B, V, logits.data_ptr(), max(int(logits.stride(0)), V) if B > 1 else V,
               t, k, p, int(seed), int(row0), int(pos), tok.data_ptr(), 1, 0, lp.data_ptr() if lp is not None else 0, 1)
    return (tok, lp) if return_logprobs else tok


def modality_seed(seed, i):
    """The keying rule of joint rollouts (generate with a list of modalities or "all"): the draw of modality i, row r,
    position n is mmt_sample's draw with this seed, whatever other modalities are generated. One splitmix64 step on
    seed + (i + 1) * 0x9E3779B97F4A7C15, all arithmetic modulo 2^64."""
    x = (int(seed) + (int(i) + 1) * 0x9E3779B97F4A7C15) & MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


class MultiLaunch:
    """The host arrays of one mmt_sample_multi call over P problems (include/mmt.h), made once and updated in place
    between launches: a decode loop changes `logits[p]` / `row_stride[p]` / `tok[p]` / `logprob[p]` (raw addresses,
    0 = absent) and calls `run`. settings: P triples from check_settings; seeds: P ints."""

    def __init__(self, V, settings, seeds, tok_stride, lp_stride):
        P = self.P = len(V)
        n = max(1, P)
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.temperature = (ctypes.c_float * n)(*[s[0] for s in settings])
        self.top_k = (ctypes.c_int32 * n)(*[s[1] for s in settings])
        self.top_p = (ctypes.c_float * n)(*[s[2] for s in settings])
        self.seed = (ctypes.c_uint64 * n)(*[int(s) & MASK64 for s in seeds])
        self.logits = (ctypes.c_void_p * n)()
        self.row_stride = (ctypes.c_int64 * n)(*[int(v) for v in V])
        self.tok = (ctypes.c_void_p * n)()
        self.tok_stride = (ctypes.c_int64 * n)(*[int(x) for x in tok_stride])
        self.compact = (ctypes.c_void_p * n)()
        self.logprob = (ctypes.c_void_p * n)()
        self.lp_stride = (ctypes.c_int64 * n)(*[int(x) for x in lp_stride])

    def run(self, L, stream, batch, row0, pos):
        """One mmt_sample_multi. Raises MmtError on a non-zero status."""
        rc = L.mmt_sample_multi(stream, self.P, batch, self.V, self.logits, self.row_stride, self.temperature,
                                self.top_k, self.top_p, self.seed, row0, pos, self.tok, self.tok_stride, self.compact,
                                self.logprob, self.lp_stride)
        if rc != 0:
            raise ML.MmtError(f"mmt_sample_multi failed (status {rc})")


def bind_view(launch, p, view, rows):
    """Point problem p of a launch object (MultiLaunch, ScoreLaunch, ForecastLaunch) at a [rows, V_p] logits view:
    its address and its row stride in elements (V_p for one row, whatever the view's stride says)."""
    V = int(launch.V[p])
    launch.logits[p] = view.data_ptr()
    launch.row_stride[p] = max(int(view.stride(0)), V) if rows > 1 else V


def _per_problem(value, P, name):
    if isinstance(value, (list, tuple)):
        if len(value) != P:
            raise ValueError(f"sample_multi: {name} has {len(value)} entries for {P} problems")
        return list(value)
    return [value] * P


def sample_multi(logits_list, *, temperature=1.0, top_k=0, top_p=1.0, seeds, pos, row0=0, return_logprobs=False):
    """`sample` for P problems over the same rows in one launch (mmt_sample_multi): logits_list holds P fp32 [B, V_p]
    tensors on one GPU (rows may be strided, as for `sample`); temperature / top_k / top_p are scalars or sequences
    of P; seeds is a sequence of P 64-bit seeds (for the modalities of a joint rollout: modality_seed(seed, i)), or
    one int for all. Returns a list of P int64 [B] tensors, with return_logprobs also a list of P fp32 [B]. Problem p
    gives exactly what sample(logits_list[p], ..., seed=seeds[p]) gives."""
    P = len(logits_list)
    ts, ks, ps = (_per_problem(temperature, P, "temperature"), _per_problem(top_k, P, "top_k"),
                  _per_problem(top_p, P, "top_p"))
    seeds = [int(s) for s in _per_problem(seeds, P, "seeds")]
    settings = [check_settings(t, k, p) for t, k, p in zip(ts, ks, ps)]
    if P == 0:
        return ([], []) if return_logprobs else []
    B, dev = logits_list[0].shape[0], logits_list[0].device
    for lg in logits_list:
        if lg.dim() != 2 or lg.dtype != torch.float32 or lg.device.type != "cuda" or lg.device != dev:
            raise ValueError("sample_multi: every logits must be an fp32 [B, V] tensor on the same GPU")
        if lg.shape[0] != B:
            raise ValueError("sample_multi: the problems must share the number of rows")
        V = lg.shape[1]
        if V < 1 or (V > 1 and lg.stride(1) != 1) or (B > 1 and lg.stride(0) < V):
            raise ValueError("sample_multi: the elements of a row must be contiguous and rows must not overlap")
    toks = [torch.empty(B, dtype=torch.int64, device=dev) for _ in range(P)]
    lps = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(P)] if return_logprobs else None
    ml = MultiLaunch([lg.shape[1] for lg in logits_list], settings, seeds, [1] * P, [1] * P)
    for p, lg in enumerate(logits_list):
        bind_view(ml, p, lg, B)
        ml.tok[p] = toks[p].data_ptr()
        ml.logprob[p] = lps[p].data_ptr() if lps is not None else None
    with torch.cuda.device(dev):
        ml.run(ML.lib(), ML.stream_ptr(dev), B, int(row0), int(pos))
    return (toks, lps) if return_logprobs else toks


class ScoreLaunch:
    """The host arrays of one mmt_score_multi call over P problems (include/mmt.h), made once and updated in place
    between launches, as MultiLaunch: a decode loop changes `logits[p]` / `row_stride[p]` / `tok[p]` / `logprob[p]`
    (raw addresses) and calls `run`."""

    def __init__(self, V, tok_stride, lp_stride):
        P = self.P = len(V)
        n = max(1, P)
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.logits = (ctypes.c_void_p * n)()
        self.row_stride = (ctypes.c_int64 * n)(*[int(v) for v in V])
        self.tok = (ctypes.c_void_p * n)()
        self.tok_stride = (ctypes.c_int64 * n)(*[int(x) for x in tok_stride])
        self.logprob = (ctypes.c_void_p * n)()
        self.lp_stride = (ctypes.c_int64 * n)(*[int(x) for x in lp_stride])

    def run(self, L, stream, batch):
        """One mmt_score_multi. Raises MmtError on a non-zero status."""
        rc = L.mmt_score_multi(stream, self.P, batch, self.V, self.logits, self.row_stride, self.tok, self.tok_stride,
                               self.logprob, self.lp_stride)
        if rc != 0:
            raise ML.MmtError(f"mmt_score_multi failed (status {rc})")


def score_multi(logits_list, tokens_list):
    """The log-probability of given tokens, P problems over the same rows in one launch (mmt_score_multi):
    logits_list holds P fp32 [B, V_p] tensors on one GPU (rows may be strided, as for `sample`), tokens_list P int64
    [B] tensors (any stride). Returns a list of P fp32 [B]: for a token that `sample(logits, temperature=1.0)` drew,
    bit for bit the log-probability it reported. ValueError for a token outside 0..V_p - 1 (this check reads the
    tokens on the host; a loop that must not sync validates its tokens once and uses ScoreLaunch)."""
    P = len(logits_list)
    if len(tokens_list) != P:
        raise ValueError(f"score_multi: {len(tokens_list)} token tensors for {P} problems")
    if P == 0:
        return []
    B, dev = logits_list[0].shape[0], logits_list[0].device
    for lg, tk in zip(logits_list, tokens_list):
        if lg.dim() != 2 or lg.dtype != torch.float32 or lg.device.type != "cuda" or lg.device != dev:
            raise ValueError("score_multi: every logits must be an fp32 [B, V] tensor on the same GPU")
        if lg.shape[0] != B:
            raise ValueError("score_multi: the problems must share the number of rows")
        V = lg.shape[1]
        if V < 1 or (V > 1 and lg.stride(1) != 1) or (B > 1 and lg.stride(0) < V):
            raise ValueError("score_multi: the elements of a row must be contiguous and rows must not overlap")
        if tk.dim() != 1 or tk.dtype != torch.int64 or tk.device != dev or tk.shape[0] != B:
            raise ValueError("score_multi: every tokens must be an int64 [B] tensor on the logits' GPU")
        if B and (int(tk.min()) < 0 or int(tk.max()) >= V):
            raise ValueError(f"score_multi: tokens outside 0..{V - 1}")
    lps = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(P)]
    sl = ScoreLaunch([lg.shape[1] for lg in logits_list], [max(int(tk.stride(0)), 1) for tk in tokens_list], [1] * P)
    for p, (lg, tk) in enumerate(zip(logits_list, tokens_list)):
        bind_view(sl, p, lg, B)
        sl.tok[p] = tk.data_ptr()
        sl.logprob[p] = lps[p].data_ptr()
    with torch.cuda.device(dev):
        sl.run(ML.lib(), ML.stream_ptr(dev), B)
    return lps


class ForecastLaunch:
    """The host arrays of one mmt_forecast_multi call over P problems (include/mmt.h), made once and updated in place
    between launches, as MultiLaunch: a decode loop changes `logits[p]` / `row_stride[p]` / `pmf[p]` / `ess[p]` /
    `live[p]` (raw addresses; ess / live 0 = absent) and calls `run`. settings: P triples from check_settings;
    lp_ptrs / lp_strides: the G <= 8 log-probability matrices of the weights (none: unweighted unless `run` gets a
    logw)."""

    def __init__(self, V, settings, pmf_stride, lp_ptrs=(), lp_strides=()):
        P = self.P = len(V)
        G = self.G = len(lp_ptrs)
        if G > 8:
            raise ValueError("forecast: at most 8 log-probability matrices")
        if len(lp_strides) != G or len(settings) != P or len(pmf_stride) != P:
            raise ValueError("forecast: one setting and pmf stride per problem, one stride per log-probability matrix")
        n, g = max(1, P), max(1, G)
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.temperature = (ctypes.c_float * n)(*[s[0] for s in settings])
        self.top_k = (ctypes.c_int32 * n)(*[s[1] for s in settings])
        self.top_p = (ctypes.c_float * n)(*[s[2] for s in settings])
        self.logits = (ctypes.c_void_p * n)()
        self.row_stride = (ctypes.c_int64 * n)(*[int(v) for v in V])
        self.pmf = (ctypes.c_void_p * n)()
        self.pmf_stride = (ctypes.c_int64 * n)(*[int(x) for x in pmf_stride])
        self.ess = (ctypes.c_void_p * n)()
        self.live = (ctypes.c_void_p * n)()
        self.lp = (ctypes.c_void_p * g)(*[int(x) for x in lp_ptrs])
        self.lp_stride = (ctypes.c_int64 * g)(*[int(x) for x in lp_strides])

    def scratch_bytes(self, L, batch, samples):
        """mmt_forecast_scratch_bytes for this launch's problems; ValueError for a shape the entry refuses."""
        n = L.mmt_forecast_scratch_bytes(self.P, int(batch), int(samples))
        if n < 0:
            raise ValueError(f"forecast: {batch} prompts x {samples} samples are more rows than a launch addresses")
        return int(n)

    def run(self, L, stream, batch, samples, j0, j1, logw_ptr, scratch_ptr, scratch_bytes, logw_out_ptr=0):
        """One mmt_forecast_multi (logw_ptr / logw_out_ptr: raw addresses, 0 = absent). Raises MmtError on a non-zero
        status."""
        rc = L.mmt_forecast_multi(stream, self.P, batch, samples, self.V, self.logits, self.row_stride,
                                  self.temperature, self.top_k, self.top_p, self.pmf, self.pmf_stride, self.G, self.lp,
                                  self.lp_stride, j0, j1, logw_ptr or None, logw_out_ptr or None, self.ess, self.live,
                                  scratch_ptr, scratch_bytes)
        if rc != 0:
            raise ML.MmtError(f"mmt_forecast_multi failed (status {rc})")


def forecast_multi(logits_list, *, samples, temperature=1.0, top_k=0, top_p=1.0, logprobs=None, logw=None, j0=0,
                   j1=None):
    """The forecast distribution of one step (mmt_forecast_multi, include/mmt.h): logits_list holds P fp32
    [B * samples, V_p] tensors on one GPU (rows may be strided, as for `sample`), row b * samples + s being path s of
    prompt b; temperature / top_k / top_p are scalars or sequences of P, the settings the sampler draws with. Returns
    (pmfs, ess, live): lists of P fp32 [B, V_p], fp64 [B] and int32 [B]. pmfs[p][b] is the mixture of the laws the
    prompt's rows draw their token from; with logprobs (up to 8 fp32 [B * samples, N], columns [j0, j1), default all)
    and / or logw (fp64 [B * samples]) the rows are weighted as mmt_resample weighs them (samples <= 4096). No sync."""
    P = len(logits_list)
    ts, ks, ps = (_per_problem(temperature, P, "temperature"), _per_problem(top_k, P, "top_k"),
                  _per_problem(top_p, P, "top_p"))
    settings = [check_settings(t, k, p) for t, k, p in zip(ts, ks, ps)]
    S = int(samples)
    if S < 1:
        raise ValueError(f"forecast_multi: samples must be >= 1, got {samples!r}")
    if P == 0:
        return [], [], []
    R, dev = logits_list[0].shape[0], logits_list[0].device
    if R % S:
        raise ValueError(f"forecast_multi: {R} rows are no multiple of samples={samples}")
    B = R // S
    for lg in logits_list:
        if lg.dim() != 2 or lg.dtype != torch.float32 or lg.device.type != "cuda" or lg.device != dev:
            raise ValueError("forecast_multi: every logits must be an fp32 [rows, V] tensor on the same GPU")
        if lg.shape[0] != R:
            raise ValueError("forecast_multi: the problems must share the number of rows")
        V = lg.shape[1]
        if V < 1 or (V > 1 and lg.stride(1) != 1) or (R > 1 and lg.stride(0) < V):
            raise ValueError("forecast_multi: the elements of a row must be contiguous and rows must not overlap")
    logprobs = [] if logprobs is None else list(logprobs)
    N = None
    for lp in logprobs:
        if lp.dtype != torch.float32 or lp.dim() != 2 or lp.shape[0] != R or lp.device != dev or (
                lp.shape[1] > 1 and lp.stride(1) != 1):
            raise ValueError(f"forecast_multi: every logprobs must be an fp32 [{R}, N] tensor on the GPU, rows "
                             "contiguous")
        if N is not None and lp.shape[1] != N:
            raise ValueError("forecast_multi: the logprobs must share N")
        N = lp.shape[1]
    N = 0 if N is None else N
    j1 = N if j1 is None else int(j1)
    if not 0 <= int(j0) <= j1 <= N:
        raise ValueError(f"forecast_multi: columns [{j0}, {j1}) outside 0..{N}")
    if logw is not None and (logw.dtype != torch.float64 or logw.shape != (R,) or not logw.is_contiguous()
                             or logw.device != dev):
        raise ValueError(f"forecast_multi: logw must be a contiguous fp64 [{R}] tensor on the GPU")
    if (logprobs or logw is not None) and S > RESAMPLE_MAX_SAMPLES:
        raise ValueError(f"forecast_multi: weights are folded over at most {RESAMPLE_MAX_SAMPLES} samples, got {S}")
    pmfs = [torch.empty(B, lg.shape[1], dtype=torch.float32, device=dev) for lg in logits_list]
    ess = [torch.empty(B, dtype=torch.float64, device=dev) for _ in range(P)]
    live = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(P)]
    fl = ForecastLaunch([lg.shape[1] for lg in logits_list], settings, [lg.shape[1] for lg in logits_list],
                        [lp.data_ptr() for lp in logprobs], [max(int(lp.stride(0)), N) for lp in logprobs])
    for p, lg in enumerate(logits_list):
        bind_view(fl, p, lg, R)
        fl.pmf[p], fl.ess[p], fl.live[p] = pmfs[p].data_ptr(), ess[p].data_ptr(), live[p].data_ptr()
    L = ML.lib()
    nbytes = fl.scratch_bytes(L, B, S)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        fl.run(L, ML.stream_ptr(dev), B, S, int(j0), j1, logw.data_ptr() if logw is not None else 0,
               scratch.data_ptr(), nbytes)
    return pmfs, ess, live


STATS_FIELDS = ("total", "entropy", "mean", "var", "p_down", "p_flat", "p_up", "p_max")  # stats[..., k] of mmt_pmf_stats
PMF_MAX_QUANTILES = 16


def check_quantiles(quantiles):
    """The quantile levels as mmt_pmf_stats takes them: at most 16 floats in (0, 1); ValueError otherwise."""
    try:
        q = [float(x) for x in quantiles]
    except (TypeError, ValueError):
        raise ValueError(f"forecast: quantiles must be a sequence of numbers in (0, 1), got {quantiles!r}") from None
    if len(q) > PMF_MAX_QUANTILES:
        raise ValueError(f"forecast: at most {PMF_MAX_QUANTILES} quantile levels, got {len(q)}")
    for x in q:
        if not 0.0 < x < 1.0:
            raise ValueError(f"forecast: a quantile level must lie in (0, 1), got {x!r}")
    return q


def check_values(values, V, name="values"):
    """A vocabulary's values as mmt_pmf_stats takes them: V numbers, none NaN, non-decreasing in token order (the
    reference's vocabulary is sorted(set(...))). Returns a CPU fp64 tensor; checked once on the host. ValueError
    otherwise."""
    v = torch.as_tensor(values, dtype=torch.float64).detach().cpu().reshape(-1)
    if v.shape[0] != V:
        raise ValueError(f"forecast: {name} must hold {V} numbers, got {v.shape[0]}")
    if bool(torch.isnan(v).any()) or (V > 1 and bool((v[1:] < v[:-1]).any())):
        raise ValueError(f"forecast: {name} must be non-decreasing in token order, without NaN")
    return v


class StatsLaunch:
    """The host arrays of one mmt_pmf_stats call over P problems (raw addresses; values / origin 0 = absent)."""

    def __init__(self, V, pmf_stride, is_percent, quantiles):
        P = self.P = len(V)
        n = max(1, P)
        q = check_quantiles(quantiles)
        self.nq = len(q)
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.pmf = (ctypes.c_void_p * n)()
        self.pmf_stride = (ctypes.c_int64 * n)(*[int(x) for x in pmf_stride])
        self.values = (ctypes.c_void_p * n)()
        self.is_percent = (ctypes.c_int32 * n)(*[1 if x else 0 for x in is_percent])
        self.origin = (ctypes.c_void_p * n)()
        self.origin_stride = (ctypes.c_int64 * n)(*([1] * P))
        self.levels = (ctypes.c_double * max(1, self.nq))(*q)
        self.stats = (ctypes.c_void_p * n)()
        self.qtok = (ctypes.c_void_p * n)()

    def run(self, L, stream, rows):
        rc = L.mmt_pmf_stats(stream, self.P, rows, self.V, self.pmf, self.pmf_stride, self.values, self.is_percent,
                             self.origin, self.origin_stride, self.nq, self.levels, self.stats, self.qtok)
        if rc != 0:
            raise ML.MmtError(f"mmt_pmf_stats failed (status {rc})")


def pmf_stats(pmf_list, *, values=None, is_percent=False, origin=None, quantiles=(0.05, 0.5, 0.95)):
    """Summaries of pmf rows (mmt_pmf_stats, include/mmt.h): pmf_list holds P fp32 [..., V_p] tensors on one GPU with
    the same leading shape (contiguous; e.g. generate's [B, N, V]). values: None or a list of P entries, each None or
    V_p non-decreasing numbers (checked on the host); is_percent: a bool or P bools; origin: None or a list of P
    entries, each None or an int64 tensor of the leading shape (the token a value series' direction is measured
    from). Returns (stats, qtok): lists of P fp64 [..., 8] (STATS_FIELDS) and int32 [..., Q]."""
    P = len(pmf_list)
    q = check_quantiles(quantiles)
    if P == 0:
        return [], []
    dev, lead = pmf_list[0].device, tuple(pmf_list[0].shape[:-1])
    vals = _per_problem(values, P, "values") if isinstance(values, (list, tuple)) else [values] * P
    pct = _per_problem(is_percent, P, "is_percent")
    org = _per_problem(origin, P, "origin") if isinstance(origin, (list, tuple)) else [origin] * P
    rows = 1
    for d in lead:
        rows *= int(d)
    keep = []
    sl = StatsLaunch([t.shape[-1] for t in pmf_list], [t.shape[-1] for t in pmf_list], pct, q)
    stats = [torch.empty(*lead, 8, dtype=torch.float64, device=dev) for _ in range(P)]
    qtok = [torch.empty(*lead, len(q), dtype=torch.int32, device=dev) for _ in range(P)]
    for p, t in enumerate(pmf_list):
        if t.dim() < 1 or t.dtype != torch.float32 or t.device.type != "cuda" or t.device != dev or (
                tuple(t.shape[:-1]) != lead) or not t.is_contiguous() or t.shape[-1] < 1:
            raise ValueError("pmf_stats: every pmf must be a contiguous fp32 [..., V] tensor on the same GPU, the "
                             "leading shapes equal")
        sl.pmf[p], sl.stats[p], sl.qtok[p] = t.data_ptr(), stats[p].data_ptr(), qtok[p].data_ptr()
        if vals[p] is not None:
            keep.append(check_values(vals[p], t.shape[-1]).to(dev))
            sl.values[p] = keep[-1].data_ptr()
        if org[p] is not None:
            o = org[p]
            if o.dtype != torch.int64 or tuple(o.shape) != lead or o.device != dev:
                raise ValueError("pmf_stats: an origin must be an int64 tensor of the pmf's leading shape on its GPU")
            keep.append(o.contiguous())
            sl.origin[p] = keep[-1].data_ptr()
    with torch.cuda.device(dev):
        sl.run(ML.lib(), ML.stream_ptr(dev), rows)
    return stats, qtok


HORIZON_FIELDS = ("mean", "var", "p_down", "p_flat", "p_up", "step_down", "step_flat", "step_up", "mean_high",
                  "mean_low", "min", "max")  # stats[..., k] of mmt_horizon_stats
HORIZON_MAX_BARRIERS = 8
HORIZON_MAX_SAMPLES = 4096  # csrc/mmt_horizon.hip HZ_MAX_S: the rows of a (prompt, step) are sorted in LDS


def check_barriers(barriers):
    """The barriers of one problem as mmt_horizon_stats takes them: at most 8 finite non-zero numbers (None: none);
    ValueError otherwise."""
    if barriers is None:
        return []
    try:
        u = [float(x) for x in barriers]
    except (TypeError, ValueError):
        raise ValueError(f"horizon: barriers must be a sequence of numbers, got {barriers!r}") from None
    if len(u) > HORIZON_MAX_BARRIERS:
        raise ValueError(f"horizon: at most {HORIZON_MAX_BARRIERS} barriers, got {len(u)}")
    for x in u:
        if x != x or x in (float("inf"), float("-inf")) or x == 0.0:
            raise ValueError(f"horizon: a barrier must be finite and non-zero, got {x!r}")
    return u


class HorizonLaunch:
    """The host arrays of one mmt_horizon_stats call over P problems (include/mmt.h), made once: the caller fills
    `tok[p]` / `values[p]` / `origin[p]` / `stats[p]` / `qval[p]` / `qrow[p]` / `hit[p]` / `ess[p]` / `live[p]` (raw
    addresses; ess / live 0 = absent) and the strides, and calls `run`. barriers: P lists of the same length."""

    def __init__(self, V, tok_stride, is_percent, quantiles, barriers):
        P = self.P = len(V)
        n = max(1, P)
        q = check_quantiles(quantiles)
        bars = [check_barriers(b) for b in barriers]
        if len(bars) != P or len({len(b) for b in bars}) > 1:
            raise ValueError("horizon: one list of barriers per problem, all of one length")
        self.nq, self.nb = len(q), len(bars[0]) if bars else 0
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.tok = (ctypes.c_void_p * n)()
        self.tok_stride = (ctypes.c_int64 * n)(*[int(x) for x in tok_stride])
        self.values = (ctypes.c_void_p * n)()
        self.is_percent = (ctypes.c_int32 * n)(*[1 if x else 0 for x in is_percent])
        self.origin = (ctypes.c_void_p * n)()
        self.origin_stride = (ctypes.c_int64 * n)(*([1] * P))
        self.levels = (ctypes.c_double * max(1, self.nq))(*q)
        self._bars = [(ctypes.c_double * max(1, self.nb))(*b) for b in bars]  # kept alive: `barriers` points at them
        self.barriers = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in self._bars])
        self.stats = (ctypes.c_void_p * n)()
        self.qval = (ctypes.c_void_p * n)()
        self.qrow = (ctypes.c_void_p * n)()
        self.hit = (ctypes.c_void_p * n)()
        self.ess = (ctypes.c_void_p * n)()
        self.live = (ctypes.c_void_p * n)()

    def scratch_bytes(self, L, batch, samples, steps):
        """mmt_horizon_scratch_bytes for this launch's problems; ValueError for a shape the entry refuses."""
        n = L.mmt_horizon_scratch_bytes(self.P, int(batch), int(samples), int(steps))
        if n < 0:
            raise ValueError(f"horizon: {batch} prompts x {samples} samples x {steps} steps is a shape the entry "
                             f"refuses (at most {HORIZON_MAX_SAMPLES} samples per prompt)")
        return int(n)

    def run(self, L, stream, batch, samples, steps, logw_ptr, scratch_ptr, scratch_bytes):
        """One mmt_horizon_stats (logw_ptr: a raw address, 0 = absent). Raises MmtError on a non-zero status."""
        rc = L.mmt_horizon_stats(stream, self.P, batch, samples, steps, self.V, self.tok, self.tok_stride, self.values,
                                 self.is_percent, self.origin, self.origin_stride, logw_ptr or None, self.nq,
                                 self.levels, self.nb, self.barriers, self.stats, self.qval, self.qrow, self.hit,
                                 self.ess, self.live, scratch_ptr, scratch_bytes)
        if rc != 0:
            raise ML.MmtError(f"mmt_horizon_stats failed (status {rc})")


def horizon_outputs(P, batch, steps, nq, nb, dev):
    """The output tensors of one mmt_horizon_stats call, per problem: (stats, qval, qrow, hit, ess, live)."""
    return [(torch.empty(batch, steps, 12, dtype=torch.float64, device=dev),
             torch.empty(batch, steps, nq, dtype=torch.float64, device=dev),
             torch.empty(batch, steps, nq, dtype=torch.int32, device=dev),
             torch.empty(batch, steps, nb, dtype=torch.float64, device=dev),
             torch.zeros(batch, dtype=torch.float64, device=dev),  # zeros: steps == 0 launches nothing
             torch.zeros(batch, dtype=torch.int32, device=dev)) for _ in range(P)]


def horizon_dict(outs):
    """One problem's outputs as the dict generate(horizon=) and horizon_stats return: the HORIZON_FIELDS as fp64
    [B, N], "quantile_values" fp64 and "quantile_paths" int32 [B, N, Q], "hit" fp64 [B, N, nb], "ess", "live" [B]."""
    stats, qval, qrow, hit, ess, live = outs
    d = {name: stats[..., k] for k, name in enumerate(HORIZON_FIELDS)}
    d.update(quantile_values=qval, quantile_paths=qrow, hit=hit, ess=ess, live=live)
    return d


def horizon_stats(tokens_list, *, samples, values, is_percent=False, origin=None, logw=None,
                  quantiles=(0.05, 0.5, 0.95), barriers=None):
    """Horizon forecasts of finished paths (mmt_horizon_stats, include/mmt.h): tokens_list holds P int64 [B * samples,
    N] tensors on one GPU (the new tokens of each path; rows may be strided, e.g. `seqs[i][:, n0:]`), row b * samples
    + s being path s of prompt b. values: a list of P vocabularies (V_p non-decreasing numbers each, required);
    is_percent: a bool or P bools; origin: None or a list of P entries, each None (a percent series) or an int64
    [B * samples] tensor (the token a value series' change is measured from: the column before the new ones); logw:
    None or fp64 [B * samples] log-weights, weighed as mmt_resample weighs them; quantiles: at most 16 levels;
    barriers: None or a list of P lists (one length) of at most 8 finite non-zero numbers. Returns a list of P dicts
    (horizon_dict): per (prompt, step) the weighted moments of the cumulative change x, the masses of its sign and of
    the step direction, the means of the running high and low, min / max, quantiles with the path that carries each,
    the probability of having touched each barrier; per prompt ess and live. No sync."""
    P = len(tokens_list)
    q = check_quantiles(quantiles)
    S = int(samples)
    if S < 1:
        raise ValueError(f"horizon_stats: samples must be >= 1, got {samples!r}")
    if S > HORIZON_MAX_SAMPLES:
        raise ValueError(f"horizon_stats: at most {HORIZON_MAX_SAMPLES} samples per prompt, got {S}")
    if not isinstance(values, (list, tuple)) or len(values) != P:
        raise ValueError(f"horizon_stats: values must be a list of {P} vocabularies (a horizon has no meaning on "
                         "token indices)")
    pct = _per_problem(is_percent, P, "is_percent")
    org = _per_problem(origin, P, "origin") if isinstance(origin, (list, tuple)) else [origin] * P
    bars = [[] for _ in range(P)] if barriers is None else [check_barriers(b) for b in barriers]
    if len(bars) != P:
        raise ValueError(f"horizon_stats: barriers must be a list of {P} lists")
    if P == 0:
        return []
    R, N = tokens_list[0].shape[0], tokens_list[0].shape[1] if tokens_list[0].dim() == 2 else -1
    dev = tokens_list[0].device
    if R % S:
        raise ValueError(f"horizon_stats: {R} rows are no multiple of samples={samples}")
    B = R // S
    if logw is not None and (logw.dtype != torch.float64 or logw.shape != (R,) or not logw.is_contiguous()
                             or logw.device != dev):
        raise ValueError(f"horizon_stats: logw must be a contiguous fp64 [{R}] tensor on the GPU")
    keep = []
    for p, t in enumerate(tokens_list):
        if t.dim() != 2 or t.dtype != torch.int64 or t.device.type != "cuda" or t.device != dev or (
                tuple(t.shape) != (R, N)) or (N > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < N):
            raise ValueError("horizon_stats: every tokens must be an int64 [rows, N] tensor on the same GPU, the "
                             "elements of a row contiguous")
        if values[p] is None:
            raise ValueError(f"horizon_stats: problem {p} has no values")
        if not pct[p]:
            o = org[p]
            if o is None or o.dtype != torch.int64 or tuple(o.shape) != (R,) or o.device != dev:
                raise ValueError(f"horizon_stats: a value series needs an int64 [{R}] origin on the GPU (problem {p})")
    hl = HorizonLaunch([len(torch.as_tensor(v).reshape(-1)) for v in values],
                       [max(int(t.stride(0)), N) if R > 1 else max(N, 1) for t in tokens_list], pct, q, bars)
    outs = horizon_outputs(P, B, N, hl.nq, hl.nb, dev)
    for p, t in enumerate(tokens_list):
        keep.append(check_values(values[p], hl.V[p]).to(dev))
        hl.tok[p], hl.values[p] = t.data_ptr(), keep[-1].data_ptr()
        if not pct[p]:
            hl.origin[p] = org[p].data_ptr()
            hl.origin_stride[p] = max(int(org[p].stride(0)), 1)
        (hl.stats[p], hl.qval[p], hl.qrow[p], hl.hit[p], hl.ess[p],
         hl.live[p]) = [x.data_ptr() if x.numel() else None for x in outs[p]]
    L = ML.lib()
    nbytes = hl.scratch_bytes(L, B, S, N)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        hl.run(L, ML.stream_ptr(dev), B, S, N, logw.data_ptr() if logw is not None else 0, scratch.data_ptr(), nbytes)
    return [horizon_dict(o) for o in outs]


JOINT_FIELDS = ("mean", "var", "p_down", "p_flat", "p_up", "mean_high", "mean_low", "min", "max")  # bstats[..., k]
JOINT_MAX_PROBLEMS = 8
JOINT_MAX_BASKETS = 8
JOINT_MAX_PAIRS = 28


def check_baskets(baskets, P):
    """The baskets of one mmt_horizon_joint call over P problems: None (none) or at most 8 dicts {"weights": P finite
    numbers, not all zero, "barriers": at most 8 finite non-zero numbers (optional)}. Returns (coefficients [nbk][P],
    barriers [nbk][...]); ValueError otherwise."""
    if baskets is None:
        return [], []
    if not isinstance(baskets, (list, tuple)) or not all(isinstance(b, dict) for b in baskets):
        raise ValueError("horizon_joint: baskets must be a list of dicts {\"weights\": [...], \"barriers\": [...]}")
    if len(baskets) > JOINT_MAX_BASKETS:
        raise ValueError(f"horizon_joint: at most {JOINT_MAX_BASKETS} baskets, got {len(baskets)}")
    coef, bars = [], []
    for k, b in enumerate(baskets):
        for name in b:
            if name not in ("weights", "barriers"):
                raise ValueError(f"horizon_joint: basket {k} has no key {name!r} (weights, barriers)")
        try:
            a = [float(x) for x in b["weights"]]
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"horizon_joint: basket {k} needs \"weights\": a sequence of {P} numbers") from None
        if len(a) != P:
            raise ValueError(f"horizon_joint: basket {k} has {len(a)} weights for {P} series")
        if any(x != x or x in (float("inf"), float("-inf")) for x in a):
            raise ValueError(f"horizon_joint: the weights of basket {k} must be finite, got {a!r}")
        if not any(x != 0.0 for x in a):
            raise ValueError(f"horizon_joint: basket {k} has no non-zero weight")
        coef.append(a)
        bars.append(check_barriers(b.get("barriers")))
    return coef, bars


def check_pairs(pairs, P):
    """The pairs of one mmt_horizon_joint call over P problems: None (none), "all" (every p < q) or a sequence of
    distinct (p, q), p != q in 0..P-1. Returns a list of tuples; ValueError otherwise."""
    if pairs is None:
        return []
    if isinstance(pairs, str):
        if pairs != "all":
            raise ValueError(f"horizon_joint: pairs must be \"all\" or a list of (p, q), got {pairs!r}")
        return [(p, q) for p in range(P) for q in range(p + 1, P)]
    out = []
    try:
        for pq in pairs:
            p, q = pq
            if any(isinstance(i, bool) or not isinstance(i, int) for i in (p, q)):
                raise TypeError
            out.append((p, q))
    except (TypeError, ValueError):
        raise ValueError(f"horizon_joint: pairs must be \"all\" or a list of (p, q) ints, got {pairs!r}") from None
    for p, q in out:
        if not (0 <= p < P and 0 <= q < P) or p == q:
            raise ValueError(f"horizon_joint: pair {(p, q)} must name two different series in 0..{P - 1}")
    if len(set(out)) != len(out):
        raise ValueError(f"horizon_joint: a pair is named twice: {out}")
    if len(out) > JOINT_MAX_PAIRS:
        raise ValueError(f"horizon_joint: at most {JOINT_MAX_PAIRS} pairs, got {len(out)}")
    return out


def horizon_joint(tokens_list, *, samples, values, is_percent=False, origin=None, logw=None,
                  quantiles=(0.05, 0.5, 0.95), baskets=None, pairs=None):
    """Joint horizon forecasts of finished paths (mmt_horizon_joint, include/mmt.h). tokens_list, samples, values,
    is_percent, origin, logw, quantiles: as horizon_stats takes them, for the P <= 8 series that take part. baskets: a
    list of at most 8 dicts {"weights": [a_0..a_{P-1}], "barriers": [...]}: the position sum_p a_p x^(p) in the series'
    cumulative changes (barrier lists of unequal length are padded for the call and their columns cut from the result).
    pairs: "all" or a list of (p, q). Returns {"ess", "live" [B], "baskets": a list of dicts, "pairs": {(p, q): dict}}.
    A basket dict: "stats" fp64 [B, N, 9] and its columns by name (JOINT_FIELDS: "mean", "var", ...),
    "quantile_values" fp64, "quantile_rows" int32 (the path that carries each quantile) and "tail_means" fp64 (the mean
    of the basket below each quantile: the expected shortfall; mirror the weights for the upper tail) [B, N, Q], "hit"
    fp64 [B, N, nb]. A pair dict: "cov", "corr", "var_p", "var_q" fp64 [B, N], "sign_table" and "step_table" fp64 [B, N,
    3, 3] (the mass of (sign x_p, sign x_q) / of the step directions at [s_p + 1, s_q + 1]). A path that is dead in
    one series is dead in all. No sync."""
    P = len(tokens_list)
    q = check_quantiles(quantiles)
    S = int(samples)
    if S < 1:
        raise ValueError(f"horizon_joint: samples must be >= 1, got {samples!r}")
    if S > HORIZON_MAX_SAMPLES:
        raise ValueError(f"horizon_joint: at most {HORIZON_MAX_SAMPLES} samples per prompt, got {S}")
    if not 1 <= P <= JOINT_MAX_PROBLEMS:
        raise ValueError(f"horizon_joint: 1..{JOINT_MAX_PROBLEMS} series per call, got {P}")
    if not isinstance(values, (list, tuple)) or len(values) != P:
        raise ValueError(f"horizon_joint: values must be a list of {P} vocabularies (a horizon has no meaning on "
                         "token indices)")
    pct = _per_problem(is_percent, P, "is_percent")
    org = _per_problem(origin, P, "origin") if isinstance(origin, (list, tuple)) else [origin] * P
    coef, bars = check_baskets(baskets, P)
    prs = check_pairs(pairs, P)
    nbk, npair, nq = len(coef), len(prs), len(q)
    nb = max([len(b) for b in bars], default=0)
    R, N = tokens_list[0].shape[0], tokens_list[0].shape[1] if tokens_list[0].dim() == 2 else -1
    dev = tokens_list[0].device
    if R % S:
        raise ValueError(f"horizon_joint: {R} rows are no multiple of samples={samples}")
    B = R // S
    if logw is not None and (logw.dtype != torch.float64 or logw.shape != (R,) or not logw.is_contiguous()
                             or logw.device != dev):
        raise ValueError(f"horizon_joint: logw must be a contiguous fp64 [{R}] tensor on the GPU")
    for p, t in enumerate(tokens_list):
        if t.dim() != 2 or t.dtype != torch.int64 or t.device.type != "cuda" or t.device != dev or (
                tuple(t.shape) != (R, N)) or (N > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < N):
            raise ValueError("horizon_joint: every tokens must be an int64 [rows, N] tensor on the same GPU, the "
                             "elements of a row contiguous")
        if values[p] is None:
            raise ValueError(f"horizon_joint: problem {p} has no values")
        if not pct[p]:
            o = org[p]
            if o is None or o.dtype != torch.int64 or tuple(o.shape) != (R,) or o.device != dev:
                raise ValueError(f"horizon_joint: a value series needs an int64 [{R}] origin on the GPU (problem {p})")
    Vs = [len(torch.as_tensor(v).reshape(-1)) for v in values]
    vals = [check_values(values[p], Vs[p]).to(dev) for p in range(P)]
    f64, i32, i64, vp = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    new = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)  # noqa: E731
    bst = [new(B, N, 9) for _ in range(nbk)]
    bqv, btl = [new(B, N, nq) for _ in range(nbk)], [new(B, N, nq) for _ in range(nbk)]
    bqr = [new(B, N, nq, dt=torch.int32) for _ in range(nbk)]
    bht = [new(B, N, nb) for _ in range(nbk)]
    pst = [new(B, N, 22) for _ in range(npair)]
    ess = torch.zeros(B, dtype=torch.float64, device=dev)  # zeros: steps == 0 launches nothing
    live = torch.zeros(B, dtype=torch.int32, device=dev)
    if nbk or npair:
        L = ML.lib()
        nbytes = int(L.mmt_horizon_joint_scratch_bytes(P, B, S, N, nbk))
        if nbytes < 0:
            raise ValueError(f"horizon_joint: {B} prompts x {S} samples x {N} steps is a shape the entry refuses")
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        ptrs = lambda ts: (vp * max(1, len(ts)))(*[t.data_ptr() if t.numel() else None for t in ts])  # noqa: E731
        with torch.cuda.device(dev):
            rc = L.mmt_horizon_joint(
                ML.stream_ptr(dev), P, B, S, N, (i32 * P)(*Vs), (vp * P)(*[t.data_ptr() for t in tokens_list]),
                (i64 * P)(*[max(int(t.stride(0)), N) if R > 1 else max(N, 1) for t in tokens_list]),
                (vp * P)(*[v.data_ptr() for v in vals]), (i32 * P)(*[1 if x else 0 for x in pct]),
                (vp * P)(*[None if pct[p] else org[p].data_ptr() for p in range(P)]),
                (i64 * P)(*[1 if pct[p] else max(int(org[p].stride(0)), 1) for p in range(P)]),
                logw.data_ptr() if logw is not None else None, nq, (f64 * max(1, nq))(*q), nbk,
                (f64 * max(1, nbk * P))(*[a for row in coef for a in row]), nb,
                (f64 * max(1, nbk * nb))(*[u for b in bars for u in b + [1.0] * (nb - len(b))]), npair,
                (i32 * max(1, 2 * npair))(*[i for pq in prs for i in pq]), ptrs(bst), ptrs(bqv), ptrs(bqr), ptrs(btl),
                ptrs(bht), ptrs(pst), ess.data_ptr() if B else None, live.data_ptr() if B else None,
                scratch.data_ptr(), nbytes)
        if rc != 0:
            raise ML.MmtError(f"mmt_horizon_joint failed (status {rc})")
    out = {"ess": ess, "live": live, "baskets": [], "pairs": {}}
    for k in range(nbk):
        d = {name: bst[k][..., i] for i, name in enumerate(JOINT_FIELDS)}
        d.update(stats=bst[k], quantile_values=bqv[k], quantile_rows=bqr[k], tail_means=btl[k],
                 hit=bht[k][..., :len(bars[k])])
        out["baskets"].append(d)
    for k, pq in enumerate(prs):
        s = pst[k]
        out["pairs"][pq] = {"cov": s[..., 0], "corr": s[..., 1], "var_p": s[..., 2], "var_q": s[..., 3],
                            "sign_table": s[..., 4:13].reshape(B, N, 3, 3), "step_table": s[..., 13:22].reshape(B, N, 3, 3)}
    return out


SCORE_FIELDS = ("realised", "crps", "pit", "mean_error", "p_realised_sign", "p_realised_step", "realised_high",
                "realised_low")  # sc[..., k] of mmt_horizon_score
SCORE_AGG_FIELDS = ("count", "crps", "abs_realised", "abs_error", "sq_error", "p_realised_sign", "sign_hits",
                    "p_realised_step", "step_hits", "var")  # agg[..., k]
SCORE_MAX_BINS = 64


def check_bins(bins):
    """The PIT bins as mmt_horizon_score takes them: an int in 1..64; ValueError otherwise."""
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= SCORE_MAX_BINS:
        raise ValueError(f"horizon score: bins must be an int in 1..{SCORE_MAX_BINS}, got {bins!r}")
    return bins


class HorizonScoreLaunch:
    """The host arrays of one mmt_horizon_score call over P problems (include/mmt.h), made once: the caller fills the
    raw addresses `tok` / `values` / `origin` / `real` / `real_origin` (inputs), `stats` / `qval` / `hit` (the
    forecast of a mmt_horizon_stats call on the same inputs), `sc` (0 = in the scratch) / `pin` / `bs` / `agg` /
    `aggq` / `aggb` / `pit` (outputs) and the strides, and calls `run`. barriers: P lists of the same length."""

    def __init__(self, V, tok_stride, real_stride, is_percent, quantiles, barriers, bins=10):
        P = self.P = len(V)
        n = max(1, P)
        q = check_quantiles(quantiles)
        bars = [check_barriers(b) for b in barriers]
        if len(bars) != P or len({len(b) for b in bars}) > 1:
            raise ValueError("horizon score: one list of barriers per problem, all of one length")
        self.nq, self.nb, self.bins = len(q), len(bars[0]) if bars else 0, check_bins(bins)
        self.V = (ctypes.c_int32 * n)(*[int(v) for v in V])
        self.tok = (ctypes.c_void_p * n)()
        self.tok_stride = (ctypes.c_int64 * n)(*[int(x) for x in tok_stride])
        self.values = (ctypes.c_void_p * n)()
        self.is_percent = (ctypes.c_int32 * n)(*[1 if x else 0 for x in is_percent])
        self.origin = (ctypes.c_void_p * n)()
        self.origin_stride = (ctypes.c_int64 * n)(*([1] * P))
        self.real = (ctypes.c_void_p * n)()
        self.real_stride = (ctypes.c_int64 * n)(*[int(x) for x in real_stride])
        self.real_origin = (ctypes.c_void_p * n)()
        self.real_origin_stride = (ctypes.c_int64 * n)(*([1] * P))
        self.levels = (ctypes.c_double * max(1, self.nq))(*q)
        self._bars = [(ctypes.c_double * max(1, self.nb))(*b) for b in bars]  # kept alive: `barriers` points at them
        self.barriers = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in self._bars])
        for name in ("stats", "qval", "hit", "sc", "pin", "bs", "agg", "aggq", "aggb", "pit"):
            setattr(self, name, (ctypes.c_void_p * n)())

    def scratch_bytes(self, L, batch, samples, steps):
        """mmt_horizon_score_scratch_bytes for this launch's problems; ValueError for a shape the entry refuses."""
        n = L.mmt_horizon_score_scratch_bytes(self.P, int(batch), int(samples), int(steps))
        if n < 0:
            raise ValueError(f"horizon score: {batch} prompts x {samples} samples x {steps} steps is a shape the "
                             f"entry refuses (at most {HORIZON_MAX_SAMPLES} samples per prompt)")
        return int(n)

    def run(self, L, stream, batch, samples, steps, logw_ptr, scratch_ptr, scratch_bytes, accumulate=False):
        """One mmt_horizon_score (logw_ptr: a raw address, 0 = absent). Raises MmtError on a non-zero status."""
        rc = L.mmt_horizon_score(stream, self.P, batch, samples, steps, self.V, self.tok, self.tok_stride, self.values,
                                 self.is_percent, self.origin, self.origin_stride, self.real, self.real_stride,
                                 self.real_origin, self.real_origin_stride, logw_ptr or None, self.nq, self.levels,
                                 self.nb, self.barriers, self.stats, self.qval, self.hit, self.bins,
                                 1 if accumulate else 0, self.sc, self.pin, self.bs, self.agg, self.aggq, self.aggb,
                                 self.pit, scratch_ptr, scratch_bytes)
        if rc != 0:
            raise ML.MmtError(f"mmt_horizon_score failed (status {rc})")


def horizon_score_outputs(P, batch, steps, nq, nb, bins, dev):
    """The output tensors of one mmt_horizon_score call, per problem: (sc, pin, bs, agg, aggq, aggb, pit). The tables
    start at zero: a call with no step or no prompt launches nothing."""
    f64 = dict(dtype=torch.float64, device=dev)
    return [(torch.empty(batch, steps, 8, **f64), torch.empty(batch, steps, nq, **f64),
             torch.empty(batch, steps, nb, **f64), torch.zeros(steps, 10, **f64), torch.zeros(steps, nq, 2, **f64),
             torch.zeros(steps, nb, 3, **f64), torch.zeros(steps, bins, **f64)) for _ in range(P)]


def horizon_score_dict(outs):
    """One problem's outputs as the dict generate(realised=) and horizon_score return: the SCORE_FIELDS as fp64 [B, N],
    "pinball" fp64 [B, N, Q], "brier" fp64 [B, N, nb], and the tables "agg" [N, 10] (SCORE_AGG_FIELDS), "aggq" [N, Q,
    2], "aggb" [N, nb, 3], "pit_hist" [N, bins]."""
    sc, pin, bs, agg, aggq, aggb, pit = outs
    d = {name: sc[..., k] for k, name in enumerate(SCORE_FIELDS)}
    d.update(pinball=pin, brier=bs, agg=agg, aggq=aggq, aggb=aggb, pit_hist=pit)
    return d


def bind_score_forecast(sl, p, stats, qval, hit):
    """Point problem p of a HorizonScoreLaunch at the forecast tensors of a mmt_horizon_stats call."""
    sl.stats[p] = stats.data_ptr() if stats.numel() else None
    sl.qval[p] = qval.data_ptr() if qval.numel() else None
    sl.hit[p] = hit.data_ptr() if hit.numel() else None


def bind_score_outputs(sl, p, outs):
    (sl.sc[p], sl.pin[p], sl.bs[p], sl.agg[p], sl.aggq[p], sl.aggb[p],
     sl.pit[p]) = [x.data_ptr() if x.numel() else None for x in outs]


def horizon_score(tokens_list, realised_list, *, samples, values, is_percent=False, origin=None, realised_origin=None,
                  logw=None, forecast, quantiles=(0.05, 0.5, 0.95), barriers=None, bins=10):
    """Scores of horizon forecasts against the realised series (mmt_horizon_score, include/mmt.h). tokens_list, samples,
    values, is_percent, origin, logw, quantiles and barriers: what horizon_stats was given. realised_list: P int64 [B,
    N] tensors, the tokens that followed prompt b (rows may be strided); realised_origin: None or a list of P entries,
    each None (a percent series) or an int64 [B] tensor (the token before the realised ones). forecast: the list of
    P dicts horizon_stats returned for these inputs; it is read, never recomputed. bins: the cells of the PIT histogram,
    1..64. Returns a list of P dicts (horizon_score_dict): per (prompt, step) the realised change, the CRPS and
    mid-PIT of the weighted paths, the error of the mean, the mass the forecast gave the realised sign and step
    direction, the realised running high and low, the pinball loss per level and the Brier score per barrier; per
    step the tables RolloutMetrics accumulates. No sync."""
    P = len(tokens_list)
    q = check_quantiles(quantiles)
    check_bins(bins)
    S = int(samples)
    if S < 1:
        raise ValueError(f"horizon_score: samples must be >= 1, got {samples!r}")
    if S > HORIZON_MAX_SAMPLES:
        raise ValueError(f"horizon_score: at most {HORIZON_MAX_SAMPLES} samples per prompt, got {S}")
    if not isinstance(values, (list, tuple)) or len(values) != P:
        raise ValueError(f"horizon_score: values must be a list of {P} vocabularies")
    if not isinstance(realised_list, (list, tuple)) or len(realised_list) != P:
        raise ValueError(f"horizon_score: realised_list must hold {P} tensors")
    if not isinstance(forecast, (list, tuple)) or len(forecast) != P:
        raise ValueError(f"horizon_score: forecast must be the list of {P} dicts horizon_stats returned")
    pct = _per_problem(is_percent, P, "is_percent")
    org = _per_problem(origin, P, "origin") if isinstance(origin, (list, tuple)) else [origin] * P
    rorg = (_per_problem(realised_origin, P, "realised_origin") if isinstance(realised_origin, (list, tuple))
            else [realised_origin] * P)
    bars = [[] for _ in range(P)] if barriers is None else [check_barriers(b) for b in barriers]
    if len(bars) != P:
        raise ValueError(f"horizon_score: barriers must be a list of {P} lists")
    if P == 0:
        return []
    R, N = tokens_list[0].shape[0], tokens_list[0].shape[1] if tokens_list[0].dim() == 2 else -1
    dev = tokens_list[0].device
    if R % S:
        raise ValueError(f"horizon_score: {R} rows are no multiple of samples={samples}")
    B = R // S
    if logw is not None and (logw.dtype != torch.float64 or logw.shape != (R,) or not logw.is_contiguous()
                             or logw.device != dev):
        raise ValueError(f"horizon_score: logw must be a contiguous fp64 [{R}] tensor on the GPU")
    nq, nb = len(q), len(bars[0])
    fc = []
    for p, t in enumerate(tokens_list):
        if t.dim() != 2 or t.dtype != torch.int64 or t.device.type != "cuda" or t.device != dev or (
                tuple(t.shape) != (R, N)) or (N > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < N):
            raise ValueError("horizon_score: every tokens must be an int64 [rows, N] tensor on the same GPU, the "
                             "elements of a row contiguous")
        y = realised_list[p]
        if not torch.is_tensor(y) or y.dim() != 2 or y.dtype != torch.int64 or y.device != dev or (
                tuple(y.shape) != (B, N)) or (N > 1 and y.stride(1) != 1) or (B > 1 and y.stride(0) < N):
            raise ValueError(f"horizon_score: every realised must be an int64 [{B}, {N}] tensor on the same GPU, the "
                             "elements of a row contiguous")
        if values[p] is None:
            raise ValueError(f"horizon_score: problem {p} has no values")
        if not pct[p]:
            o, ro = org[p], rorg[p]
            if o is None or o.dtype != torch.int64 or tuple(o.shape) != (R,) or o.device != dev:
                raise ValueError(f"horizon_score: a value series needs an int64 [{R}] origin on the GPU (problem {p})")
            if ro is None or ro.dtype != torch.int64 or tuple(ro.shape) != (B,) or ro.device != dev:
                raise ValueError(f"horizon_score: a value series needs an int64 [{B}] realised_origin on the GPU "
                                 f"(problem {p})")
        f = forecast[p]
        try:
            st = torch.stack([f[k] for k in HORIZON_FIELDS], dim=-1).contiguous()
            qv, ht = f["quantile_values"].contiguous(), f["hit"].contiguous()
        except (KeyError, TypeError, RuntimeError):
            raise ValueError(f"horizon_score: forecast[{p}] is not a dict horizon_stats returned") from None
        if tuple(st.shape) != (B, N, 12) or tuple(qv.shape) != (B, N, nq) or tuple(ht.shape) != (B, N, nb) or any(
                x.dtype != torch.float64 or x.device != dev for x in (st, qv, ht)):
            raise ValueError(f"horizon_score: forecast[{p}] does not have the shapes of {B} prompts, {N} steps, "
                             f"{nq} quantiles and {nb} barriers")
        fc.append((st, qv, ht))
    sl = HorizonScoreLaunch([len(torch.as_tensor(v).reshape(-1)) for v in values],
                            [max(int(t.stride(0)), N) if R > 1 else max(N, 1) for t in tokens_list],
                            [max(int(y.stride(0)), N) if B > 1 else max(N, 1) for y in realised_list], pct, q, bars,
                            bins)
    outs = horizon_score_outputs(P, B, N, nq, nb, bins, dev)
    keep = []
    for p, t in enumerate(tokens_list):
        keep.append(check_values(values[p], sl.V[p]).to(dev))
        sl.tok[p], sl.values[p], sl.real[p] = t.data_ptr(), keep[-1].data_ptr(), realised_list[p].data_ptr()
        if not pct[p]:
            sl.origin[p], sl.origin_stride[p] = org[p].data_ptr(), max(int(org[p].stride(0)), 1)
            sl.real_origin[p], sl.real_origin_stride[p] = rorg[p].data_ptr(), max(int(rorg[p].stride(0)), 1)
        bind_score_forecast(sl, p, *fc[p])
        bind_score_outputs(sl, p, outs[p])
    L = ML.lib()
    nbytes = sl.scratch_bytes(L, B, S, N)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        sl.run(L, ML.stream_ptr(dev), B, S, N, logw.data_ptr() if logw is not None else 0, scratch.data_ptr(), nbytes)
    return [horizon_score_dict(o) for o in outs]


RESAMPLE_MAX_SAMPLES = 4096  # csrc/mmt_evidence.hip RS_MAX_S: the S weights of a prompt stay in LDS


class ResampleLaunch:
    """The host arrays of mmt_resample over G log-probability matrices (raw addresses and row strides in elements),
    made once; `run` is one launch over the columns [j0, j1)."""

    def __init__(self, lp_ptrs, lp_strides):
        G = self.G = len(lp_ptrs)
        n = max(1, G)
        self.lp = (ctypes.c_void_p * n)(*[int(x) for x in lp_ptrs])
        self.stride = (ctypes.c_int64 * n)(*[int(x) for x in lp_strides])

    def run(self, L, stream, batch, samples, j0, j1, logw_ptr, log_evidence_ptr, ess_threshold, seed, pos, anc_ptr,
            resampled_ptr):
        rc = L.mmt_resample(stream, batch, samples, self.G, self.lp, self.stride, j0, j1, logw_ptr, log_evidence_ptr,
                            float(ess_threshold), int(seed) & MASK64, int(pos), anc_ptr, resampled_ptr)
        if rc != 0:
            raise ML.MmtError(f"mmt_resample failed (status {rc})")


def resample(logprobs, logw, log_evidence, *, samples, ess_threshold, seed, pos, j0=0, j1=None):
    """One particle-filter step over the S = samples paths of each prompt (mmt_resample, include/mmt.h): logprobs is
    a list of up to 8 fp32 [B * S, N] tensors (the given modalities' log-probabilities, ascending modality; the
    elements of a row contiguous), logw fp64 [B * S] and log_evidence fp64 [B] are updated IN PLACE, the columns
    [j0, j1) (default: all) are folded in. Returns (ancestors int32 [B * S] as global row indices, resampled int32
    [B]). ess_threshold 0 only accumulates; a negative one is the closing fold (log_evidence gains the estimate of
    the carried weights, nothing is resampled). No sync."""
    dev = logw.device
    if logw.dtype != torch.float64 or logw.dim() != 1 or not logw.is_contiguous() or dev.type != "cuda":
        raise ValueError("resample: logw must be a contiguous fp64 [B * S] tensor on the GPU")
    R, S = logw.shape[0], int(samples)
    if S < 1 or R % S:
        raise ValueError(f"resample: {R} rows are no multiple of samples={samples}")
    B = R // S
    if (log_evidence.dtype != torch.float64 or log_evidence.shape != (B,) or not log_evidence.is_contiguous()
            or log_evidence.device != dev):
        raise ValueError(f"resample: log_evidence must be a contiguous fp64 [{B}] tensor on the GPU")
    if len(logprobs) > 8:
        raise ValueError("resample: at most 8 log-probability matrices")
    N = None
    for lp in logprobs:
        if lp.dtype != torch.float32 or lp.dim() != 2 or lp.shape[0] != R or lp.device != dev or (
                lp.shape[1] > 1 and lp.stride(1) != 1):
            raise ValueError(f"resample: every logprobs must be an fp32 [{R}, N] tensor on the GPU, rows contiguous")
        if N is not None and lp.shape[1] != N:
            raise ValueError("resample: the logprobs must share N")
        N = lp.shape[1]
    N = 0 if N is None else N
    j1 = N if j1 is None else int(j1)
    if not 0 <= int(j0) <= j1 <= N:
        raise ValueError(f"resample: columns [{j0}, {j1}) outside 0..{N}")
    if ess_threshold != ess_threshold:
        raise ValueError("resample: ess_threshold must not be NaN")
    if S > RESAMPLE_MAX_SAMPLES:
        raise ValueError(f"resample: samples={S} exceeds {RESAMPLE_MAX_SAMPLES}")
    anc = torch.empty(R, dtype=torch.int32, device=dev)
    res = torch.empty(B, dtype=torch.int32, device=dev)
    rl = ResampleLaunch([lp.data_ptr() for lp in logprobs], [max(int(lp.stride(0)), N) for lp in logprobs])
    with torch.cuda.device(dev):
        rl.run(ML.lib(), ML.stream_ptr(dev), B, S, int(j0), j1, logw.data_ptr(), log_evidence.data_ptr(),
               ess_threshold, seed, pos, anc.data_ptr(), res.data_ptr())
    return anc, res
