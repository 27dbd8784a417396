"""Cost of the guarded optimizer step (mmt_optim.AdamW max_grad_norm / skip_nonfinite), on one box in one
process, interleaved:

  * optimizer alone at a config's parameter count: plain mmt_adamw_step against mmt_grad_sqsum +
    mmt_guard_finalize + mmt_adamw_step_guarded, HIP events around batches of calls on gradients that change
    between calls (a rotating set of buffers larger than the 256 MiB Infinity Cache together), plus the two
    added kernels on their own. From the bytes alone the guarded step moves 8 n floats against 7 n
    (sqsum reads g once more);
  * the whole training step, timed the way bench.py times its headline (same model, synthetic data, device
    batcher, warm-up and step count, wall clock around the timed steps), with grad_clip off and on.

    python tools/guard_cost.py [--config c1] [--steps 200] [--warmup 20] [--rounds 2] [--clip 1.0]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))

import torch  # noqa: E402

import bench  # noqa: E402


def optimizer_alone(n, dev, reps, rounds, clip):
    """us per call of the plain step and of the guarded triple over n fp32 elements."""
    import mmt_lib as ML
    L = ML.lib()
    nbuf = max(2, (320 << 20) // (16 * n) + 1)  # p, g, m, v sets: together past the Infinity Cache
    sets = [[torch.randn(n, device=dev) * s for s in (0.02, 1e-3, 1e-4, 1e-8)] for _ in range(nbuf)]
    for s in sets:
        s[3].abs_()
    guard = torch.zeros(L.mmt_guard_state_bytes(), dtype=torch.uint8, device=dev)
    st = ML.stream_ptr(dev)
    args = (1e-5, 0.9, 0.999, 1e-8, 0.01)  # a small lr: thousands of timed steps leave the buffers finite

    def plain(k):
        p, g, m, v = sets[k % nbuf]
        ML.check(L.mmt_adamw_step(None, st, ML.ptr(p), ML.ptr(g), ML.ptr(m), ML.ptr(v), n, 1000 + k, *args), None, "adamw")

    def sqsum(k):
        ML.check(L.mmt_grad_sqsum(st, ML.ptr(sets[k % nbuf][1]), n, 0, ML.ptr(guard)), None, "sqsum")

    def finalize(k):
        ML.check(L.mmt_guard_finalize(st, clip, 1, 0.9, 0.999, ML.ptr(guard)), None, "finalize")

    def guarded(k):
        p, g, m, v = sets[k % nbuf]
        sqsum(k)
        finalize(k)
        ML.check(L.mmt_adamw_step_guarded(None, st, ML.ptr(p), ML.ptr(g), ML.ptr(m), ML.ptr(v), n, *args, ML.ptr(guard)),
                 None, "adamw_guarded")

    def timed(fn):
        for k in range(nbuf):
            fn(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for k in range(reps):
            fn(k)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    out = {"plain": [], "guarded": [], "sqsum": [], "finalize": []}
    for _ in range(rounds):  # plain, guarded, plain, guarded: the two bracket each other
        for name, fn in (("plain", plain), ("guarded", guarded), ("sqsum", sqsum), ("finalize", finalize)):
            out[name].append(round(timed(fn), 3))
    return out


def run(config, steps, warmup, rounds, clip, reps):
    import config_utils
    import mmt_data
    import mmt_optim
    import training_utils as TU
    from model import MultimodalTransformer
    cfg = bench.CONFIGS[config]
    M, C, H, L, T, B = cfg["M"], cfg["C"], cfg["H"], cfg["L"], cfg["T"], cfg["B"]
    dev = torch.device("cuda", 0)
    config_utils._config_cache = {"n_embd": C, "n_head": H, "n_layer": L, "block_size": T, "dropout": 0.1,
                                  "device": str(dev), "batch_size": B, "eval_iters": 1, "learning_rate": 3e-4,
                                  "precision": "fp8" if config == "c4" else "bf16"}
    data = mmt_data.make_synthetic(n_modalities=M)
    V = data["vocab_sizes"]
    torch.manual_seed(1234)
    model = MultimodalTransformer(M, V, data["params"]).to(dev)
    n = model.flat_params.numel()
    alone = optimizer_alone(n, dev, reps, rounds, clip)
    batcher = TU.DeviceBatcher(data["train"], data["val"], V, [p[2] for p in data["params"]], data["file_lengths"],
                               data["is_percents"], T, B, dev, seed=1000)
    # two optimizers over the same parameters; each keeps its own moments
    opts = {False: mmt_optim.AdamW(model.parameters(), lr=3e-4),
            True: mmt_optim.AdamW(model.parameters(), lr=3e-4, max_grad_norm=clip, skip_nonfinite=True)}

    def timed(on):
        opt = opts[on]

        def step():
            xb, yb = batcher.next("train", 1)
            _, losses = model(xb, yb)
            opt.zero_grad(set_to_none=True)
            sum(losses).backward()
            opt.step()

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    ms = {False: [], True: []}
    for _ in range(rounds):  # off, on, off, on
        for on in (False, True):
            ms[on].append(round(timed(on), 4))
    applied, skipped, clipped = opts[True].counters()
    best = {k: min(v) for k, v in alone.items()}
    return {"config": config, "device": torch.cuda.get_device_name(0), "n_params": n, "steps": steps, "warmup": warmup,
            "optimizer_us": alone,
            "optimizer_guarded_over_plain": round(best["guarded"] / best["plain"], 4), "bytes_expectation": round(8 / 7, 4),
            "plain_GBps": round(7 * 4 * n / best["plain"] / 1e3, 1), "guarded_GBps": round(8 * 4 * n / best["guarded"] / 1e3, 1),
            "sqsum_GBps": round(4 * n / best["sqsum"] / 1e3, 1),
            "ms_per_step_clip_off": ms[False], "ms_per_step_clip_on": ms[True],
            "step_cost_pct": round((min(ms[True]) / min(ms[False]) - 1.0) * 100.0, 3),
            "clip": clip, "last_grad_norm": float(opts[True].last_grad_norm),
            "applied_skipped_clipped": [applied, skipped, clipped]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--clip", type=float, default=1.0)
    a = ap.parse_args()
    for config in a.config.split(","):
        print(json.dumps(run(config, a.steps, a.warmup, a.rounds, a.clip, a.reps)), flush=True)


if __name__ == "__main__":
    main()
