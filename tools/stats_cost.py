"""Cost of the per-tensor gradient statistics (mmt_stats.TensorStats / mmt_tensor_stats), on one box in one
visit, interleaved:

  * `python bench.py` (the default headline) from a checkout of the parent commit and from this tree, in
    fresh child processes, alternating (--parent DIR; skipped without it): the default path must not move;
  * mmt_tensor_stats alone over the model's gradient layout: mode ALWAYS (one streaming read of the buffer)
    and mode ON_SKIP on a clean step (three launches that return after one load each), HIP events around
    batches of calls on a rotating set of buffers larger than the 256 MiB Infinity Cache together;
  * the whole training step, timed the way bench.py times its headline (same model, synthetic data, device
    batcher, warm-up and step count, wall clock around the timed steps), with four optimizers over the same
    parameters: plain (grad_stats off), guarded without statistics (what `skipped` / `every` switch on
    first), guarded + mode "skipped", guarded + mode "every".

    python tools/stats_cost.py [--config c1] [--steps 200] [--warmup 20] [--rounds 2] [--parent DIR]
                               [--out profiles/stats_cost.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))


def bench_lines(parent, config, steps, warmup, rounds):
    """bench.py's headline from `parent` and from this tree, alternating, one fresh process each."""
    out = {"parent": [], "tree": []}
    for _ in range(rounds):
        for name, root in (("parent", parent), ("tree", REPO)):
            cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", config, "--steps", str(steps),
                   "--warmup", str(warmup)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py failed in {root}:\n{r.stderr[-2000:]}")
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            out[name].append({"ms_per_step": line["ms_per_step"], "tokens_per_s": line["value"],
                              "final_loss": line["final_loss"]})
            print(f"bench {name}: {line['ms_per_step']} ms/step", file=sys.stderr, flush=True)
    return out


def stats_alone(model, dev, reps, rounds):
    """us per mmt_tensor_stats call over the model's gradient layout."""
    import torch

    import mmt_lib as ML
    import mmt_stats
    L = ML.lib()
    n = model.flat_params.numel()
    nbuf = max(2, (320 << 20) // (4 * n) + 1)
    bufs = [torch.randn(n, device=dev) * 1e-3 for _ in range(nbuf)]
    st = mmt_stats.TensorStats(model, "every")
    guard = torch.zeros(L.mmt_guard_state_bytes(), dtype=torch.uint8, device=dev)
    ML.check(L.mmt_grad_sqsum(ML.stream_ptr(dev), ML.ptr(bufs[0]), n, 0, ML.ptr(guard)), None, "sqsum")
    ML.check(L.mmt_guard_finalize(ML.stream_ptr(dev), 0.0, 1, 0.9, 0.999, ML.ptr(guard)), None, "finalize")  # ok = 1
    s = ML.stream_ptr(dev)
    table = model.tensor_segments()["device"]

    def call(mode):
        def fn(k):
            ML.check(L.mmt_tensor_stats(s, ML.ptr(bufs[k % nbuf]), n, ML.ptr(table), st._nseg, mode, ML.ptr(guard),
                                        ML.ptr(st._scratch), ML.ptr(st._rec)), None, "mmt_tensor_stats")
        return fn

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

    out = {"always": [], "on_skip_clean": []}
    for _ in range(rounds):
        out["always"].append(round(timed(call(ML.STATS_ALWAYS)), 3))
        out["on_skip_clean"].append(round(timed(call(ML.STATS_ON_SKIP)), 3))
    return out, n, st._nseg


def run(config, steps, warmup, rounds, reps):
    import torch

    import bench
    import config_utils
    import mmt_data
    import mmt_optim
    import mmt_stats
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
    alone, n, nseg = stats_alone(model, dev, reps, rounds)
    batcher = TU.DeviceBatcher(data["train"], data["val"], V, [p[2] for p in data["params"]], data["file_lengths"],
                               data["is_percents"], T, B, dev, seed=1000)
    # four optimizers over the same parameters; each keeps its own moments
    legs = ("off", "guarded", "skipped", "every")
    opts = {"off": mmt_optim.AdamW(model.parameters(), lr=3e-4),
            "guarded": mmt_optim.AdamW(model.parameters(), lr=3e-4, skip_nonfinite=True),
            "skipped": mmt_optim.AdamW(model.parameters(), lr=3e-4, skip_nonfinite=True,
                                       stats=mmt_stats.TensorStats(model, "skipped")),
            "every": mmt_optim.AdamW(model.parameters(), lr=3e-4, skip_nonfinite=True,
                                     stats=mmt_stats.TensorStats(model, "every"))}

    def timed(leg):
        opt = opts[leg]

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

    ms = {leg: [] for leg in legs}
    for _ in range(rounds):  # off, guarded, skipped, every, off, ...
        for leg in legs:
            ms[leg].append(round(timed(leg), 4))
            print(f"step {leg}: {ms[leg][-1]} ms", file=sys.stderr, flush=True)
    best = {leg: min(v) for leg, v in ms.items()}
    rep = opts["every"].stats.read()
    return {"config": config, "device": torch.cuda.get_device_name(0), "n_params": n, "segments": nseg, "steps": steps,
            "warmup": warmup, "stats_us": alone, "stats_always_GBps": round(4 * n / min(alone["always"]) / 1e3, 1),
            "ms_per_step": ms,
            "step_cost_pct_vs_off": {leg: round((best[leg] / best["off"] - 1.0) * 100.0, 3) for leg in legs[1:]},
            "step_cost_pct_vs_guarded": {leg: round((best[leg] / best["guarded"] - 1.0) * 100.0, 3) for leg in legs[2:]},
            "skipped_record_is_empty": opts["skipped"].stats.read() is None,
            "every_global_norm": rep.global_norm, "every_vs_guard_norm": float(opts["every"].last_grad_norm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py from there and "
                                                   "from this tree, alternating")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stats_cost.txt"))
    a = ap.parse_args()
    lines = []
    if a.parent:  # first: this process has not opened the GPU yet
        b = bench_lines(os.path.abspath(a.parent), a.config.split(",")[0], a.steps, a.warmup, a.bench_rounds)
        p, t = [x["ms_per_step"] for x in b["parent"]], [x["ms_per_step"] for x in b["tree"]]
        b["tree_best_no_slower_than_parent_worst"] = min(t) <= max(p)
        lines.append(json.dumps({"bench_default": b}))
    for config in a.config.split(","):
        lines.append(json.dumps(run(config, a.steps, a.warmup, a.rounds, a.reps)))
    for l in lines:
        print(l, flush=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
