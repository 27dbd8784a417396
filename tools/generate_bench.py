"""Tokens per second of `model.generate`: the default path (host loop: torch.softmax, torch.multinomial, a
torch.cat per modality per token) and the device path (mmt_sample: temperature / top-k / top-p on the GPU, sequences
in preallocated buffers, per token mmt_decode_step + mmt_sample and nothing else).

C1 dimensions (d256, 8 heads, 6 layers, block 256, vocabularies 900 / 13 / 144 / 5, cross-attention on modality 0),
B = 64, a 128-token prompt, 128 new tokens of modality 0, eval mode, freshly initialised weights. Each timed call is
one generate with one synchronisation at its end; tokens per second counts B * new tokens.

    python tools/generate_bench.py [--paths default,device] [--rounds 3] [--warmup 1] [--tree DIR] [--sampler]

--tree DIR takes the package (and its built library) of another checkout of this repository, e.g. the parent
commit, whose generate has the default path only (--paths default). --sampler adds the time of mmt_sample on its
own per vocabulary size and setting. One JSON line per run.

    python tools/generate_bench.py --samples S --batch B [--paths fanout,tiled] [--attn]

Joint rollouts (every modality sampled per step from its own head, one mmt_sample_multi per token): --paths
joint,joint_topk_topp beside device,device_topk_topp; with --samples, --paths fanout_joint beside fanout.
--sampler-multi adds the time of one mmt_sample_multi launch over the four heads against four mmt_sample launches.

--samples S measures S continuations per prompt instead: `fanout` is generate(prompts, num_samples=S) and `tiled`
the same call over the prompts repeated S times by the caller (what a checkout without the keyword can do: with
--tree, --paths tiled). Per round it records paths per second (B * S / wall time), tokens per second and the peak
of torch.cuda.max_memory_allocated over the call; a path that runs out of memory is reported as such. --attn adds
the fan-out attention kernel alone against attn_decode_kernel at B * S rows (this tree only).

Evidence of a given series (modalities 0..2 sampled, modality 3 given): --paths joint_given,joint_weights without
--samples; with --samples, --paths fanout_given,fanout_weights,fanout_resample1,fanout_resample8,fanout_resample32
(evidence="resample" with ess_threshold 0.5 at resample_every 1 / 8 / 32). --gather adds mmt_fanout_gather alone
after half the new tokens: its bytes (read plus written) and us per call.

Forecast distributions (--forecast): without --samples the paths joint,joint_forecast,joint_hook and
joint_weights,joint_weights_forecast; with --samples fanout_joint,fanout_joint_forecast,fanout_joint_hook and
fanout_weights,fanout_weights_forecast. `_forecast` is the same call with forecast=True; `_hook` is what a caller can
write without it: a logits_hook that computes the unfiltered, unweighted mixture per step with torch (softmax, mean over
a prompt's paths, a copy into a [B, N, V] tensor). --forecast also adds the two entries alone: us per
mmt_forecast_multi call over the four heads at 64 rows (64 prompts of one path), 512 and 4096 rows (one prompt),
without and with weights, and us per mmt_pmf_stats launch over the four heads at 64 / 512 / 4096 pmf rows.

Horizon forecasts (--horizon): without --samples the paths joint,joint_horizon and joint_weights,joint_weights_horizon;
with --samples fanout_joint,fanout_joint_horizon and fanout_weights,fanout_weights_horizon. `_horizon` is the same call
with horizon={"values": ..., "is_percent": {0: True}, "barriers": ...} over every generated head. --horizon also adds
the entry alone: us per mmt_horizon_stats call over the four heads and 128 steps at 64 rows (64 prompts of one path),
512 and 4096 rows (one prompt), without and with log-weights, beside the torch formulation a caller can write on the
same device (value gather, cumprod, sort, cumsum of the sorted weights, searchsorted).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C1 = dict(n_embd=256, n_head=8, n_layer=6, block_size=256, V=[900, 13, 144, 5], cross=[True, False, False, False])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="default,device")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--label", default="")
    ap.add_argument("--sampler", action="store_true", help="also time mmt_sample alone (this tree only)")
    ap.add_argument("--sampler-multi", action="store_true",
                    help="also time mmt_sample_multi over the four heads against four mmt_sample launches")
    ap.add_argument("--samples", type=int, default=0, help="continuations per prompt (0: the single-path benchmark)")
    ap.add_argument("--attn", action="store_true", help="with --samples: the two decode attention kernels alone")
    ap.add_argument("--gather", action="store_true", help="with --samples: mmt_fanout_gather alone (this tree only)")
    ap.add_argument("--forecast", action="store_true",
                    help="the forecast paths by default, and the two forecast entries alone (this tree only)")
    ap.add_argument("--horizon", action="store_true",
                    help="the horizon paths by default, and mmt_horizon_stats alone against torch (this tree only)")
    a = ap.parse_args()
    if a.horizon and a.paths == "default,device":
        a.paths = ("fanout_joint,fanout_joint_horizon,fanout_weights,fanout_weights_horizon"
                   if a.samples else "joint,joint_horizon,joint_weights,joint_weights_horizon")
    if a.forecast and a.paths == "default,device":
        a.paths = ("fanout_joint,fanout_joint_forecast,fanout_joint_hook,fanout_weights,fanout_weights_forecast"
                   if a.samples else "joint,joint_forecast,joint_hook,joint_weights,joint_weights_forecast")
    if a.samples and a.paths == "default,device":
        a.paths = "fanout,tiled"
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "trade-aid-multimodal-transformer_amd"))
    import torch
    import config_utils
    from model import MultimodalTransformer
    dev = torch.device("cuda", 0)
    config_utils._config_cache = {"n_embd": C1["n_embd"], "n_head": C1["n_head"], "n_layer": C1["n_layer"],
                                  "block_size": C1["block_size"], "dropout": 0.0, "device": str(dev),
                                  "batch_size": a.batch, "eval_iters": 1}
    params = []
    for c in C1["cross"]:
        p = [None] * 12
        p[8] = c
        params.append(p)
    torch.manual_seed(1234)
    model = MultimodalTransformer(len(C1["V"]), C1["V"], params).to(dev)
    model.eval()
    g = torch.Generator().manual_seed(7)
    prompt = [torch.randint(0, v, (a.batch, a.prompt), generator=g).to(dev) for v in C1["V"]]
    calls = {
        "default": lambda: model.generate(prompt, max_new_tokens=a.new, modality_to_generate=0),
        "device": lambda: model.generate(prompt, max_new_tokens=a.new, modality_to_generate=0, temperature=1.0, seed=11),
        "device_topk_topp": lambda: model.generate(prompt, max_new_tokens=a.new, modality_to_generate=0, temperature=0.8,
                                                   top_k=50, top_p=0.9, seed=11),
        # joint rollouts: every modality sampled per step from its own head (one mmt_sample_multi per token)
        "joint": lambda: model.generate(prompt, max_new_tokens=a.new, modality_to_generate="all", temperature=1.0,
                                        seed=11),
        "joint_topk_topp": lambda: model.generate(prompt, max_new_tokens=a.new, modality_to_generate="all",
                                                  temperature=0.8, top_k=50, top_p=0.9, seed=11),
    }
    # evidence of a given series: modalities 0..2 sampled, modality 3 follows the caller's tokens
    scen = {3: torch.randint(0, C1["V"][3], (a.batch, a.new), generator=g)}
    gkw = dict(max_new_tokens=a.new, modality_to_generate=[0, 1, 2], given=scen, temperature=1.0, seed=11)
    calls["joint_given"] = lambda: model.generate(prompt, **gkw)
    calls["joint_weights"] = lambda: model.generate(prompt, evidence="weights", **gkw)[0]
    jkw = dict(max_new_tokens=a.new, modality_to_generate="all", temperature=1.0, seed=11)
    calls["joint_forecast"] = lambda: model.generate(prompt, forecast=True, **jkw)[0]
    calls["joint_hook"] = lambda: model.generate(prompt, logits_hook=mixture_hook(torch, dev, a, 1), **jkw)
    calls["joint_weights_forecast"] = lambda: model.generate(prompt, evidence="weights", forecast=True, **gkw)[0]
    calls["joint_horizon"] = lambda: model.generate(prompt, horizon=horizon_arg(torch, range(4)), **jkw)[0]
    calls["joint_weights_horizon"] = lambda: model.generate(prompt, evidence="weights",
                                                            horizon=horizon_arg(torch, range(3)), **gkw)[0]
    paths = [p for p in a.paths.split(",") if p]
    if a.samples:
        return fanout_bench(a, torch, dev, model, prompt, paths)
    out = {p: [] for p in paths}
    for p in paths:
        for _ in range(a.warmup):
            calls[p]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):  # the paths alternate: each round brackets the others
        for p in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seqs = calls[p]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert tuple(seqs[0].shape) == (a.batch, a.prompt + a.new)
            out[p].append(round(a.batch * a.new / dt, 1))
    res = {"tool": "generate_bench", "label": a.label, "device": torch.cuda.get_device_name(0),
           "batch": a.batch, "prompt": a.prompt, "new_tokens": a.new,
           "tokens_per_s": out, "best_tokens_per_s": {p: max(v) for p, v in out.items()}}
    if a.sampler:
        res["sampler_us"] = sampler_alone(torch, dev, a.batch, a.rounds)
    if a.sampler_multi:
        res["sampler_multi_us"] = sampler_multi_alone(torch, dev, a.rounds)
    if a.forecast:
        res["forecast_us"] = forecast_alone(torch, dev, a.rounds)
    if a.horizon:
        res["horizon_us"] = horizon_alone(torch, dev, a.new, a.rounds)
    print(json.dumps(res), flush=True)


def horizon_arg(torch, mods):
    """generate's horizon= over the heads `mods`: a sorted vocabulary of percent changes per head (modality 0 a percent
    series, the others value series), two barriers each."""
    return {"values": {i: torch.linspace(-2.0, 2.0, C1["V"][i], dtype=torch.float64) for i in mods},
            "is_percent": {0: True}, "barriers": {i: [1.0, -1.0] for i in mods}}


def horizon_alone(torch, dev, steps, rounds, reps=20):
    """us per mmt_horizon_stats call (its two launches) over the four C1 heads and `steps` new tokens at 64 rows (64
    prompts of one path), 512 and 4096 rows (one prompt of as many paths), without and with log-weights, three
    levels and two barriers; and the torch formulation of one head's quantiles a caller could write: gather the
    values, cumprod, sort every (prompt, step) column, cumsum of the gathered weights, searchsorted (times four for
    the four heads; no moments, directions, extremes or barriers). HIP events around `reps` calls, best of `rounds`."""
    import mmt_lib as ML
    import mmt_sample as MS
    L, st = ML.lib(), ML.stream_ptr(dev)
    Vs = C1["V"]
    out = {}

    def timed(fn):
        best = None
        for _ in range(rounds):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _k in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            best = us if best is None else min(best, us)
        return round(best, 2)

    g = torch.Generator().manual_seed(9)
    for rows in (64, 512, 4096):
        B, S = (64, 1) if rows == 64 else (1, rows)
        toks = [torch.randint(0, V, (rows, steps), generator=g).to(dev) for V in Vs]
        org = [torch.randint(0, V, (rows,), generator=g).to(dev) for V in Vs]
        vals = [torch.linspace(-2.0, 2.0, V, dtype=torch.float64, device=dev) for V in Vs]
        logw = (torch.randn(rows, generator=g, dtype=torch.float64) * 2.0).to(dev)
        hl = MS.HorizonLaunch(Vs, [steps] * 4, [True, False, False, False], (0.05, 0.5, 0.95), [[1.0, -1.0]] * 4)
        outs = MS.horizon_outputs(4, B, steps, hl.nq, hl.nb, dev)
        for i in range(4):
            hl.tok[i], hl.values[i], hl.origin[i] = toks[i].data_ptr(), vals[i].data_ptr(), org[i].data_ptr()
            hl.stats[i], hl.qval[i], hl.qrow[i], hl.hit[i], hl.ess[i], hl.live[i] = [x.data_ptr() for x in outs[i]]
        nbytes = hl.scratch_bytes(L, B, S, steps)
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        levels = torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device=dev)

        def torch_form(weighted):
            for i in range(4):
                v = vals[i][toks[i]]                                        # [rows, steps]
                x = ((1.0 + v / 100.0).cumprod(1) - 1.0) * 100.0 if i == 0 else v - vals[i][org[i]][:, None]
                xs, order = x.view(B, S, steps).sort(dim=1)                 # every (prompt, step) column
                w = torch.exp(logw - logw.max()) if weighted else torch.ones_like(logw)
                cw = w.view(B, S, 1).expand(B, S, steps).gather(1, order).cumsum(1)
                tgt = levels.view(1, 1, 3) * cw[:, -1:, :].transpose(1, 2)  # [B, steps, 3]
                pos = torch.searchsorted(cw.transpose(1, 2).contiguous(), tgt.contiguous()).clamp_(max=S - 1)
                xs.transpose(1, 2).gather(2, pos)

        for name, weighted in (("plain", False), ("weights", True)):
            lw = logw.data_ptr() if weighted else 0
            out[f"horizon_rows{rows}_{name}"] = timed(lambda: hl.run(L, st, B, S, steps, lw, scratch.data_ptr(), nbytes))
            out[f"torch_rows{rows}_{name}"] = timed(lambda: torch_form(weighted))
    return out


def mixture_hook(torch, dev, a, S):
    """The logits_hook a caller can write without forecast=: per step and head the softmax of the [B * S, V] logits,
    averaged over each prompt's S paths, copied into column j of a [B, N, V] tensor (no top-k / top-p law, no evidence
    weights: those are not available to a hook)."""
    store = {}

    def hook(n, views):
        j = n - a.prompt
        for i, v in enumerate(views):
            if i not in store:
                store[i] = torch.zeros(a.batch, a.new, v.shape[1], dtype=torch.float32, device=dev)
            p = torch.softmax(v, dim=-1)
            store[i][:, j] = p.view(a.batch, S, -1).mean(1) if S > 1 else p

    return hook


def forecast_alone(torch, dev, rounds, reps=100):
    """us per mmt_forecast_multi call (its two launches, three with weights) over the four C1 heads at 64 rows (64
    prompts of one path), 512 and 4096 rows (one prompt of as many paths), without weights and with 32 columns of one
    log-probability matrix plus logw; and us per mmt_pmf_stats launch over the four heads at as many pmf rows. HIP
    events around `reps` back-to-back calls over rotating N(0, 3^2) logits, best of `rounds`."""
    import mmt_lib as ML
    import mmt_sample as MS
    L, st = ML.lib(), ML.stream_ptr(dev)
    Vs = C1["V"]
    out = {}

    def timed(fn):
        best = None
        for _ in range(rounds):
            for k in range(8):
                fn(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for k in range(reps):
                fn(k)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            best = us if best is None else min(best, us)
        return round(best, 2)

    for rows in (64, 512, 4096):
        B, S = (64, 1) if rows == 64 else (1, rows)
        bufs = [[torch.randn(rows, V, device=dev) * 3.0 for V in Vs] for _ in range(8)]
        pmf = [torch.zeros(B, V, device=dev) for V in Vs]
        ess = [torch.zeros(B, dtype=torch.float64, device=dev) for _ in Vs]
        live = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in Vs]
        glp = -torch.rand(rows, 32, device=dev)
        logw = torch.zeros(rows, dtype=torch.float64, device=dev)
        for name, weighted in (("plain", False), ("weights", True)):
            fl = MS.ForecastLaunch(Vs, [(1.0, 0, 1.0)] * 4, Vs, [glp.data_ptr()] if weighted else [],
                                   [32] if weighted else [])
            for i in range(4):
                fl.pmf[i], fl.ess[i], fl.live[i] = pmf[i].data_ptr(), ess[i].data_ptr(), live[i].data_ptr()
            nbytes = fl.scratch_bytes(L, B, S)
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)

            def one(k):
                for i in range(4):
                    fl.logits[i] = bufs[k % 8][i].data_ptr()
                fl.run(L, st, B, S, 0, 32 if weighted else 0, logw.data_ptr() if weighted else 0, scratch.data_ptr(),
                       nbytes)

            out[f"forecast_rows{rows}_{name}"] = timed(one)
        rowsets = [torch.softmax(torch.randn(rows, V, device=dev) * 3.0, dim=-1) for V in Vs]
        sl = MS.StatsLaunch(Vs, Vs, [False] * 4, (0.05, 0.5, 0.95))
        vals = [torch.linspace(-1.0, 1.0, V, dtype=torch.float64, device=dev) for V in Vs]
        org = torch.zeros(rows, dtype=torch.int64, device=dev)
        stats = [torch.zeros(rows, 8, dtype=torch.float64, device=dev) for _ in Vs]
        qtok = [torch.zeros(rows, 3, dtype=torch.int32, device=dev) for _ in Vs]
        for i in range(4):
            sl.pmf[i], sl.values[i], sl.origin[i] = rowsets[i].data_ptr(), vals[i].data_ptr(), org.data_ptr()
            sl.stats[i], sl.qtok[i] = stats[i].data_ptr(), qtok[i].data_ptr()
        out[f"pmf_stats_rows{rows}"] = timed(lambda k: sl.run(L, st, rows))
    return out


def fanout_bench(a, torch, dev, model, prompt, paths):
    """--samples: the paths alternate, one sync per call, per round paths/s, tokens/s and the call's peak memory."""
    S, B = a.samples, a.batch
    tiled = [p.repeat_interleave(S, 0) for p in prompt]
    kw = dict(max_new_tokens=a.new, modality_to_generate=0, temperature=1.0, seed=11)
    calls = {"fanout": lambda: model.generate(prompt, num_samples=S, **kw),
             "tiled": lambda: model.generate(tiled, **kw),
             "fanout_joint": lambda: model.generate(prompt, num_samples=S, **dict(kw, modality_to_generate="all"))}
    g = torch.Generator().manual_seed(8)
    scen = {3: torch.randint(0, C1["V"][3], (B, a.new), generator=g)}
    gkw = dict(kw, modality_to_generate=[0, 1, 2], given=scen, num_samples=S)
    calls["fanout_given"] = lambda: model.generate(prompt, **gkw)
    calls["fanout_weights"] = lambda: model.generate(prompt, evidence="weights", **gkw)[0]
    for every in (1, 8, 32):
        calls[f"fanout_resample{every}"] = lambda every=every: model.generate(
            prompt, evidence="resample", resample_every=every, ess_threshold=0.5, **gkw)[0]
    jkw = dict(kw, modality_to_generate="all", num_samples=S)
    calls["fanout_joint_forecast"] = lambda: model.generate(prompt, forecast=True, **jkw)[0]
    calls["fanout_joint_hook"] = lambda: model.generate(prompt, logits_hook=mixture_hook(torch, dev, a, S), **jkw)
    calls["fanout_weights_forecast"] = lambda: model.generate(prompt, evidence="weights", forecast=True, **gkw)[0]
    calls["fanout_joint_horizon"] = lambda: model.generate(prompt, horizon=horizon_arg(torch, range(4)), **jkw)[0]
    calls["fanout_weights_horizon"] = lambda: model.generate(prompt, evidence="weights",
                                                             horizon=horizon_arg(torch, range(3)), **gkw)[0]
    rec = {p: {"paths_per_s": [], "tokens_per_s": [], "peak_bytes": []} for p in paths}

    def one(p, timed):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        try:
            seqs = calls[p]()
        except torch.OutOfMemoryError as e:
            rec[p]["error"] = "out of memory: " + str(e).splitlines()[0][:160]
            return False
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(seqs[0].shape) == (B * S, a.prompt + a.new)
        if timed:
            rec[p]["paths_per_s"].append(round(B * S / dt, 1))
            rec[p]["tokens_per_s"].append(round(B * S * a.new / dt, 1))
            rec[p]["peak_bytes"].append(int(torch.cuda.max_memory_allocated(dev)))
        return True

    live = [p for p in paths if all(one(p, False) for _ in range(a.warmup))]
    for _ in range(a.rounds):
        live = [p for p in live if one(p, True)]
    res = {"tool": "generate_bench", "label": a.label, "device": torch.cuda.get_device_name(0), "batch": B,
           "samples": S, "prompt": a.prompt, "new_tokens": a.new, "paths": rec}
    if "fanout" in paths:
        res["fanout_path"] = getattr(model, "last_generate_path", None) if "fanout" in live else None
    if a.attn:
        res["attn_us"] = attention_alone(torch, dev, B, S, a.prompt, a.prompt + a.new, a.rounds)
    if a.gather:
        res["gather"] = gather_alone(torch, dev, model, prompt, B, S, a.prompt, a.new, a.rounds)
    if a.forecast:
        res["forecast_us"] = forecast_alone(torch, dev, a.rounds)
    if a.horizon:
        res["horizon_us"] = horizon_alone(torch, dev, a.new, a.rounds)
    print(json.dumps(res), flush=True)


def gather_alone(torch, dev, model, prompt, B, S, n0, N, rounds, reps=20):
    """mmt_fanout_gather on its own after N // 2 fan-out steps (identity ancestors, a second fan buffer): the bytes it
    moves (read plus written: whole K | Q | V and cross K | V rows of the positions written so far) and us per call
    (HIP events around `reps` back-to-back calls, best of `rounds`)."""
    import mmt_lib as ML
    L, st = ML.lib(), ML.stream_ptr(dev)
    R, npos = B * S, max(1, N // 2)
    with torch.no_grad():
        model(prompt)
        for k in range(npos):
            model._decode_fanout_step([torch.zeros(R, dtype=torch.long, device=dev) for _ in C1["V"]], n0 + k, S, n0, N)
    src = model._fan
    dst = torch.empty_like(src)
    anc = torch.arange(R, dtype=torch.int32, device=dev)
    C, M, ncross = C1["n_embd"], len(C1["V"]), sum(C1["cross"])
    moved = 2 * R * npos * 2 * C1["n_layer"] * (M * 3 * C + ncross * (M - 1) * 2 * C)

    def one():
        return L.mmt_fanout_gather(model._ctx, st, B, S, n0, N, npos, ML.ptr(anc), ML.ptr(src), ML.ptr(dst))

    best = None
    for _ in range(rounds):
        assert one() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _k in range(reps):
            one()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        best = us if best is None else min(best, us)
    return {"npos": npos, "bytes": moved, "us": round(best, 2), "GB_per_s": round(moved / best / 1e3, 1)}


def attention_alone(torch, dev, B, S, n0, T, rounds, reps=50):
    """us per launch (HIP events around `reps` back-to-back launches, best of `rounds`) of the self-attention decode
    of one modality at C1's heads: the fan-out kernel over B prompts x S samples with a shared prefix of n0 keys,
    and attn_decode_kernel over B * S rows with a cache row each, at the middle and the last position."""
    import ctypes

    import mmt_lib as ML
    L, st = ML.lib(), ML.stream_ptr(dev)
    H, hs = C1["n_head"], C1["n_embd"] // C1["n_head"]
    C, R, cap = H * hs, B * S, T - n0
    bf = torch.bfloat16
    q = torch.randn(R, 3 * C, device=dev).to(bf)
    o = torch.empty(R, C, device=dev, dtype=bf)
    cache = torch.randn(B * T, 3 * C, device=dev).to(bf)
    tail = torch.randn(R * cap, 3 * C, device=dev).to(bf)
    one = lambda x: (ctypes.c_void_p * 1)(x.data_ptr())  # noqa: E731
    out = {}
    try:
        big = torch.randn(R * T, 3 * C, device=dev).to(bf)
    except torch.OutOfMemoryError:
        big = None
    for t in (n0 + cap // 2 - 1, T - 1):
        def fan():
            return L.mmt_op_attention_decode_fanout(st, B, S, n0, t, T, H, hs, 1, ML.ptr(q[:, C:]), 3 * C, one(cache),
                                                    one(cache[:, 2 * C:]), 3 * C, hs, one(tail), one(tail[:, 2 * C:]),
                                                    3 * C, cap, ML.ptr(o), C)

        def plain():
            return L.mmt_op_attention_decode(st, R, t, T, H, hs, 1, ML.ptr(q[:, C:]), 3 * C, one(big),
                                             one(big[:, 2 * C:]), 3 * C, hs, ML.ptr(o), C)

        for name, fn in (("fanout", fan), ("decode", plain)):
            if name == "decode" and big is None:
                out[f"decode_t{t}"] = "out of memory"
                continue
            best = None
            for _ in range(rounds):
                assert fn() == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _k in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / reps * 1e3
                best = us if best is None else min(best, us)
            out[f"{name}_t{t}"] = round(best, 2)
    return out


def sampler_alone(torch, dev, batch, rounds, reps=200):
    """us per mmt_sample launch on its own (HIP events around `reps` back-to-back launches over rotating N(0, 3^2)
    logits), per vocabulary size and setting."""
    import mmt_lib as ML
    import mmt_sample
    L, st = ML.lib(), ML.stream_ptr(dev)
    tok = torch.zeros(batch, dtype=torch.int64, device=dev)
    lp = torch.zeros(batch, dtype=torch.float32, device=dev)
    out = {}
    for V in C1["V"] + [8192, 32768]:
        bufs = [torch.randn(batch, V, device=dev) * 3.0 for _ in range(8)]
        ptrs = [b.data_ptr() for b in bufs]
        for name, (t, k_, p) in (("plain", (1.0, 0, 1.0)), ("top_k50", (0.8, 50, 1.0)),
                                 ("top_k50_top_p0.9", (0.8, 50, 0.9)), ("greedy", (0.0, 0, 1.0))):
            def one(k):
                mmt_sample.launch(L, st, batch, V, ptrs[k % 8], V, t, k_, p, 3, 0, k, tok.data_ptr(), 1, 0, lp.data_ptr(), 1)

            best = None
            for _ in range(rounds):
                for k in range(8):
                    one(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for k in range(reps):
                    one(k)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / reps * 1e3
                best = us if best is None else min(best, us)
            out[f"V{V}_{name}"] = round(best, 2)
    return out


def sampler_multi_alone(torch, dev, rounds, reps=200):
    """us per step of sampling all four C1 heads (V 900 / 13 / 144 / 5) over the same rows: one mmt_sample_multi
    launch against four back-to-back mmt_sample launches, at 64 and 4096 rows, plain and with top_k=50, top_p=0.9
    (HIP events around `reps` steps over rotating N(0, 3^2) logits, best of `rounds`; the two alternate)."""
    import mmt_lib as ML
    import mmt_sample
    L, st = ML.lib(), ML.stream_ptr(dev)
    Vs = C1["V"]
    out = {}
    for rows in (64, 4096):
        toks = [torch.zeros(rows, dtype=torch.int64, device=dev) for _ in Vs]
        lps = [torch.zeros(rows, dtype=torch.float32, device=dev) for _ in Vs]
        bufs = [[torch.randn(rows, V, device=dev) * 3.0 for V in Vs] for _ in range(8)]
        for name, (t, k_, p) in (("plain", (1.0, 0, 1.0)), ("top_k50_top_p0.9", (0.8, 50, 0.9))):
            ml = mmt_sample.MultiLaunch(Vs, [(t, k_, p)] * 4, [mmt_sample.modality_seed(3, i) for i in range(4)],
                                        [1] * 4, [1] * 4)
            for i in range(4):
                ml.tok[i], ml.logprob[i] = toks[i].data_ptr(), lps[i].data_ptr()

            def multi(k):
                for i in range(4):
                    ml.logits[i] = bufs[k % 8][i].data_ptr()
                ml.run(L, st, rows, 0, k)

            def four(k):
                for i, V in enumerate(Vs):
                    mmt_sample.launch(L, st, rows, V, bufs[k % 8][i].data_ptr(), V, t, k_, p, int(ml.seed[i]), 0, k,
                                      toks[i].data_ptr(), 1, 0, lps[i].data_ptr(), 1)

            best = {"multi": None, "four_launches": None}
            for _ in range(rounds):
                for which, fn in (("multi", multi), ("four_launches", four)):
                    for k in range(8):
                        fn(k)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for k in range(reps):
                        fn(k)
                    e1.record()
                    torch.cuda.synchronize()
                    us = e0.elapsed_time(e1) / reps * 1e3
                    best[which] = us if best[which] is None else min(best[which], us)
            for which, us in best.items():
                out[f"rows{rows}_{name}_{which}"] = round(us, 2)
    return out


if __name__ == "__main__":
    main()
