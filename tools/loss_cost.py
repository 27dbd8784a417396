"""Cost of the training objective (MultimodalTransformer.set_loss) at the C1 dimensions.

Three steps, each its own command:

    python tools/loss_cost.py prepare [--rev HEAD~1]
        git-archives the parent commit into ab_variants/parent/ and builds its library there (no GPU needed; the
        directory is git-ignored and travels with the tree).
    python tools/loss_cost.py steps [--steps 200] [--warmup 20] [--passes 3] [--out FILE]
        the training step, timed as bench.py times its headline (same model, synthetic data, device batcher, AdamW,
        warm-up, host clock around steps that end in a synchronise, no profiler, no probe events): one fresh
        process per measurement, alternating parent, plain (this tree, no spec), eps (label smoothing alone) and
        full (smoothing, class and position weights), `passes` times over, the order rotated by one each pass (a
        fixed order gives every variant one place in the sequence, and the places differ by about as much as the
        parent's passes: profiles/r23_loss_objective.txt, first run). The one condition: the mean of `plain`
        lies inside the parent's pass-to-pass spread [min, max] of the same run. Exit status 1 when it does not.
    python tools/loss_cost.py trace --variant plain|eps|full --dir output/loss_trace_V
        a few steps under `rocprofv3 --kernel-trace --stats` (a run of its own), then the loss launch's kernels
        (ce_fwd_kernel / ce_spec_kernel, ce_denom_kernel, ce_loss_kernel) read from the kernel statistics.

`steps` and `trace` append what they print to --out (default profiles/r23_loss_objective.txt).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(REPO, "ab_variants", "parent")
PKG = "trade-aid-multimodal-transformer_amd"
OUT = os.path.join(REPO, "profiles", "r23_loss_objective.txt")
KERNELS = ("ce_fwd_kernel", "ce_spec_kernel", "ce_denom_kernel", "ce_loss_kernel")


def prepare(rev):
    os.makedirs(PARENT, exist_ok=True)
    tar = subprocess.run(["git", "-C", REPO, "archive", rev], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", PARENT], input=tar, check=True)
    subprocess.run([sys.executable, os.path.join(PARENT, PKG, "mmt_build.py")], check=True)
    print(f"parent tree of {rev} built in {PARENT}")


def child(tree, variant, steps, warmup):
    """One measurement in this process: ms per training step of `tree`'s code under `variant`."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, PKG))
    import torch
    import bench
    import config_utils
    import mmt_data
    import mmt_optim
    import training_utils as TU
    from model import MultimodalTransformer
    if not torch.cuda.is_available():
        raise SystemExit("loss_cost: no GPU (there is nothing to time without one)")
    cfg = bench.CONFIGS["c1"]
    M, C, H, L, T, B = cfg["M"], cfg["C"], cfg["H"], cfg["L"], cfg["T"], cfg["B"]
    dev = torch.device("cuda", 0)
    config_utils._config_cache = {"n_embd": C, "n_head": H, "n_layer": L, "block_size": T, "dropout": 0.1,
                                  "device": str(dev), "batch_size": B, "eval_iters": 1, "learning_rate": 3e-4,
                                  "precision": "bf16"}
    data = mmt_data.make_synthetic(n_modalities=M)
    V = data["vocab_sizes"]
    torch.manual_seed(1234)
    model = MultimodalTransformer(M, V, data["params"]).to(dev)
    if variant == "eps":
        model.set_loss(0.1)
    elif variant == "full":
        import mmt_loss
        u = torch.ones(T)
        u[: T // 4] = 0
        model.set_loss(0.1, {i: mmt_loss.balanced_class_weights(data["train"][i], V[i]) for i in range(M)}, u)
    opt = mmt_optim.AdamW(model.parameters(), lr=3e-4)
    batcher = TU.DeviceBatcher(data["train"], data["val"], V, [p[2] for p in data["params"]], data["file_lengths"],
                               data["is_percents"], T, B, dev, seed=1000)

    def step():
        xb, yb = batcher.next("train", 1)
        _, losses = model(xb, yb)
        opt.zero_grad(set_to_none=True)
        sum(losses).backward()
        opt.step()
        return losses

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print("RESULT " + json.dumps({"variant": variant, "ms_per_step": round(ms, 4), "steps": steps, "V": V, "R": B * T,
                                  "last_losses": [round(float(l), 4) for l in losses],
                                  "device": torch.cuda.get_device_name(0)}), flush=True)


def _spawn(tree, variant, steps, warmup, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "child", "--tree", tree, "--variant", variant,
                          "--steps", str(steps), "--warmup", str(warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode or not got:
        raise SystemExit(f"loss_cost: the {variant} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(got[-1][len("RESULT "):])


def _emit(lines, out):
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write(text + "\n")


def steps_cmd(a):
    if not os.path.exists(os.path.join(PARENT, PKG, "libmmt_hip.so")):
        raise SystemExit("loss_cost: no parent build; run `python tools/loss_cost.py prepare` first")
    order = [("parent", PARENT, "plain"), ("plain", REPO, "plain"), ("eps", REPO, "eps"), ("full", REPO, "full")]
    ms = {name: [] for name, _, _ in order}
    info = None
    for k in range(a.passes):  # the order rotates by one each pass: no variant keeps one place in the sequence
        for name, tree, variant in order[k % len(order):] + order[:k % len(order)]:
            r = _spawn(tree, variant, a.steps, a.warmup)
            ms[name].append(r["ms_per_step"])
            info = r
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    lo, hi = min(ms["parent"]), max(ms["parent"])
    ok = lo <= mean["plain"] <= hi
    lines = [f"# training step at C1 (R = {info['R']}, V = {info['V']}), {info['device']}: {a.passes} passes of "
             f"{a.steps} steps after {a.warmup} warm-up steps, one fresh process each, alternating",
             json.dumps({"ms_per_step": ms, "mean": {k: round(v, 4) for k, v in mean.items()},
                         "parent_spread": [lo, hi], "plain_inside_parent_spread": ok,
                         "eps_over_plain_pct": round((mean["eps"] / mean["plain"] - 1) * 100, 3),
                         "full_over_plain_pct": round((mean["full"] / mean["plain"] - 1) * 100, 3)})]
    _emit(lines, a.out)
    return 0 if ok else 1


def trace_cmd(a):
    os.makedirs(a.dir, exist_ok=True)
    _spawn(REPO, a.variant, a.steps, a.warmup,
           prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.dir, "-o", "run", "--"))
    found = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise SystemExit(f"loss_cost: no kernel statistics under {a.dir}")
    rows = []
    with open(found[-1], newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in KERNELS):
                rows.append({"kernel": row["Name"][:70], "calls": int(row["Calls"]),
                             "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)})
    lines = [f"# loss launch at C1, variant {a.variant}: rocprofv3 --kernel-trace --stats over {a.warmup + a.steps} steps"]
    lines += [json.dumps(r) for r in rows]
    lines.append(json.dumps({"variant": a.variant, "loss_launch_avg_us": round(sum(r["avg_us"] for r in rows), 2)}))
    _emit(lines, a.out)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("cmd", choices=["prepare", "steps", "trace", "child"])
    ap.add_argument("--rev", default="HEAD~1")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--variant", default="plain", choices=["plain", "eps", "full"])
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--dir", default=os.path.join(REPO, "output", "loss_trace"))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    trace = a.cmd == "trace"
    a.steps = a.steps if a.steps is not None else (10 if trace else 200)
    a.warmup = a.warmup if a.warmup is not None else (3 if trace else 20)
    if a.cmd == "prepare":
        return prepare(a.rev)
    if a.cmd == "child":
        return child(a.tree, a.variant, a.steps, a.warmup)
    return steps_cmd(a) if a.cmd == "steps" else trace_cmd(a)


if __name__ == "__main__":
    sys.exit(main())
