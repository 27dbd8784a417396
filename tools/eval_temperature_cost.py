"""Cost of the temperature sweep (mmt_eval.TemperatureFit / mmt_eval_temperatures), on one box in one visit,
interleaved, after a warm-up, min - max over the passes:

  * the entry alone at a config's dimensions (C1: B 64, T 256, the four heads' V, K 17, bins 10) on random logits,
    with accumulate = 1 as estimate_loss calls it, against
      (a) mmt_eval_positions alone on the same inputs (one temperature, eight fields), and
      (b) a torch formulation of the same tables (K x log_softmax, gathers, masked sums, bucketize),
    HIP events around batches of calls on a rotating set of inputs larger than the 256 MiB Infinity Cache together;
  * estimate_loss with eval_temperature fit against off: same model, synthetic data and device batcher as bench.py's
    headline, stdout discarded, wall clock around calls that end in a device synchronise, alternating;
  * with --parent DIR (a built checkout of the parent commit) the parent's estimate_loss in fresh child processes,
    alternating with this tree's `off` in fresh child processes of the same script, the order inside a pair
    alternating too (a first run with the parent always first put the tree 0.1 - 0.2 ms above the parent's spread;
    with the order mixed it lies inside it).

    python tools/eval_temperature_cost.py [--config c1] [--reps 30] [--rounds 3] [--eval-iters 20] [--parent DIR]
                                          [--out profiles/r21_eval_temperature.txt]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from eval_positions_cost import CHILD  # noqa: E402  (estimate_loss with the default keys, timed in a child process)


def child_lines(parent, config, iters, rounds, procs):
    """`procs` pairs of fresh child processes, the parent checkout and this tree; the order inside a pair alternates
    (tree, parent, parent, tree, ...), so neither side always runs second."""
    import subprocess
    out = {"parent": [], "tree_last": [], "order": []}
    for k in range(procs):
        pair = (("tree_last", REPO), ("parent", parent))
        for name, root in (pair if k % 2 == 0 else pair[::-1]):
            r = subprocess.run([sys.executable, "-c", CHILD, config, str(iters), str(rounds)], cwd=root,
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"estimate_loss child failed in {root}:\n{r.stderr[-2000:]}")
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            out["order"].append("tree_off" if name == "tree_last" else "parent")
            print(f"child {name}: {out[name][-1]} ms", file=sys.stderr, flush=True)
    return out


def torch_tables(lg, xb, yb, values, is_pct, temps, bins):
    """The same tables in torch ops: (sum [K, 2], rel [K, 3, bins, 3]) of one modality, fp32 softmax, fp64 sums. Not
    bit-compatible with the entry (other rounding, atomics in the scatter-adds): a timing yardstick."""
    import torch
    B, T, V = lg.shape
    K = len(temps)
    if is_pct:
        sg = torch.sign(values).expand(B, T, V)
    else:
        sg = torch.sign(values.view(1, 1, V) - values[xb].unsqueeze(-1))
    rs = sg.gather(-1, yb.unsqueeze(-1)).squeeze(-1).long()
    one = torch.ones(B * T, dtype=torch.float64, device=lg.device)
    edges = torch.arange(1, bins, device=lg.device, dtype=torch.float64) / bins
    tot = torch.zeros(K, 2, dtype=torch.float64, device=lg.device)
    rel = torch.zeros(K, 3, bins, 3, dtype=torch.float64, device=lg.device)
    for k, tau in enumerate(temps):
        lp = torch.log_softmax(lg * (1.0 / float(tau)), dim=-1)
        P = lp.exp()
        tot[k, 0] = B * T
        tot[k, 1] = -lp.gather(-1, yb.unsqueeze(-1)).sum(dtype=torch.float64)
        for d in range(3):
            mass = (P * (sg == d - 1)).sum(-1, dtype=torch.float64)
            j = torch.bucketize(mass.contiguous(), edges, right=True).reshape(-1)
            rel[k, d, :, 0].index_add_(0, j, one)
            rel[k, d, :, 1].index_add_(0, j, mass.reshape(-1))
            rel[k, d, :, 2].index_add_(0, j, (rs == d - 1).double().reshape(-1))
    return tot, rel


def entry_alone(Vs, values, pcts, B, T, dev, reps, rounds, bins=10):
    """us per call over all modalities: the entry, mmt_eval_positions, the torch formulation."""
    import torch

    import mmt_eval
    per_set = sum(B * T * V * 4 for V in Vs)
    nset = max(2, (320 << 20) // per_set + 1)
    g = torch.Generator(device=dev).manual_seed(7)
    sets = []
    for _ in range(nset):
        lg = [torch.randn(B, T, V, device=dev, generator=g) * 2 for V in Vs]
        xb = [torch.randint(0, V, (B, T), device=dev, generator=g) for V in Vs]
        yb = [torch.randint(0, V, (B, T), device=dev, generator=g) for V in Vs]
        sets.append((lg, xb, yb))
    tf = mmt_eval.TemperatureFit(values, pcts, t_begin=0, bins=bins)
    pm = mmt_eval.PositionMetrics(values, pcts, t_begin=0, bins=bins)
    temps = tf.temperatures()

    def entry(k):
        tf.add(*sets[k % nset])

    def positions(k):
        pm.add(*sets[k % nset])

    def torch_form(k):
        lg, xb, yb = sets[k % nset]
        for i in range(len(Vs)):
            torch_tables(lg[i], xb[i], yb[i], values[i], pcts[i], temps, bins)

    def timed(fn, n):
        for k in range(min(nset, 4)):
            fn(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for k in range(n):
            fn(k)
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / n * 1e3, 2)

    out = {"entry": [], "eval_positions": [], "torch": []}
    for _ in range(rounds):  # alternating
        out["entry"].append(timed(entry, reps))
        out["eval_positions"].append(timed(positions, reps))
        out["torch"].append(timed(torch_form, max(3, reps // 8)))
    out["entry_over_eval_positions"] = round(min(out["entry"]) / min(out["eval_positions"]), 3)
    out["torch_over_entry"] = round(min(out["torch"]) / min(out["entry"]), 3)
    out["K"] = len(temps)
    out["logit_MB_per_call"] = round(per_set / 1e6, 1)
    out["input_sets"] = nset
    out["rows_checked"] = [r["rows"] for r in tf.result()]
    return out


def run(config, reps, rounds, iters):
    import torch

    import bench
    import config_utils
    import mmt_data
    import training_utils as TU
    from model import MultimodalTransformer
    cfg = bench.CONFIGS[config]
    M, C, H, L, T, B = cfg["M"], cfg["C"], cfg["H"], cfg["L"], cfg["T"], cfg["B"]
    dev = torch.device("cuda", 0)
    conf = {"n_embd": C, "n_head": H, "n_layer": L, "block_size": T, "dropout": 0.1, "device": str(dev),
            "batch_size": B, "eval_iters": iters, "output_file_name": "", "project_file_path": ""}
    config_utils._config_cache = conf
    data = mmt_data.make_synthetic(n_modalities=M)
    Vs = data["vocab_sizes"]
    torch.manual_seed(1234)
    model = MultimodalTransformer(M, Vs, data["params"]).to(dev)
    mmt_data.install(TU, data, model)
    numeric = [TU._numeric_vocab(v, dev) for v in data["vocabs"]]
    idx = [i for i in range(M) if numeric[i][0]]
    alone = entry_alone([Vs[i] for i in idx], [numeric[i][1] for i in idx],
                        [bool(data["params"][i][3]) for i in idx], B, T, dev, reps, rounds)

    def timed(mode):
        conf["eval_temperature"] = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            TU.estimate_loss()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 3)

    for mode in ("off", "fit"):
        timed(mode)
    ms = {"off": [], "fit": []}
    for _ in range(rounds):
        for mode in ("off", "fit"):
            ms[mode].append(timed(mode))
            print(f"estimate_loss {mode}: {ms[mode][-1]} ms", file=sys.stderr, flush=True)
    calls = 2 * iters  # train and val
    fits = {s: [round(r["tau"], 4) for r in TU.last_temperature_fit[s]["results"]] for s in TU.last_temperature_fit}
    return {"config": config, "device": torch.cuda.get_device_name(0), "B": B, "T": T, "V": [Vs[i] for i in idx],
            "alone_us_per_call": alone, "eval_iters": iters, "estimate_loss_ms": ms,
            "fit_over_off": round(min(ms["fit"]) / min(ms["off"]), 4),
            "added_us_per_iteration": round((min(ms["fit"]) - min(ms["off"])) / calls * 1e3, 1),
            "fitted_tau_untrained_model": fits}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eval-iters", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its estimate_loss and this "
                                                   "tree's `off`, in fresh child processes, alternating")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r21_eval_temperature.txt"))
    a = ap.parse_args()
    lines = []
    if a.parent:  # first: this process has not opened the GPU yet
        c = child_lines(os.path.abspath(a.parent), a.config, a.eval_iters, a.rounds, a.procs)
        c = {"parent": c["parent"], "tree_off": c["tree_last"], "order": c["order"]}
        flat = {k: [x for run_ in c[k] for x in run_] for k in ("parent", "tree_off")}
        c["parent_spread_ms"] = [min(flat["parent"]), max(flat["parent"])]
        c["tree_off_spread_ms"] = [min(flat["tree_off"]), max(flat["tree_off"])]
        c["tree_off_over_parent"] = round(min(flat["tree_off"]) / min(flat["parent"]), 4)
        lines.append(json.dumps({"estimate_loss_ms_fresh_processes": c, "eval_iters": a.eval_iters}))
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))
    lines.append(json.dumps(run(a.config, a.reps, a.rounds, a.eval_iters)))
    for l in lines:
        print(l, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
