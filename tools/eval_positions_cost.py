"""Cost of the evaluation at every position (mmt_eval.PositionMetrics / mmt_eval_positions), on one box in one
visit, interleaved:

  * the entry alone at a config's dimensions (C1: B 64, T 256, the four heads' V) on random logits, with accumulate
    = 1 as estimate_loss calls it, against
      (a) a torch formulation of the same tables (log-softmax, gather, masked sums, bucketize), and
      (b) the four mmt_eval_direction launches estimate_loss makes anyway (the last position only),
    HIP events around batches of calls on a rotating set of inputs larger than the 256 MiB Infinity Cache together;
  * estimate_loss with eval_positions all against last: same model, synthetic data and device batcher as bench.py's
    headline, stdout discarded, wall clock around calls that end in a device synchronise (the loss read-back),
    alternating;
  * with --parent DIR (a built checkout of the parent commit) the parent's estimate_loss in fresh child processes,
    alternating with this tree's `last` in fresh child processes of the same script.

    python tools/eval_positions_cost.py [--config c1] [--reps 50] [--rounds 3] [--eval-iters 20] [--parent DIR]
                                        [--out profiles/r16_eval_positions.txt]
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a child process runs, in the checkout given as its working directory: estimate_loss (the default, last-position
# metric) timed as below. Only names the parent commit has.
CHILD = r"""
import contextlib, io, json, os, sys, time
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "trade-aid-multimodal-transformer_amd"))
import torch, bench, config_utils, mmt_data, training_utils as TU
from model import MultimodalTransformer
config, iters, rounds = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
cfg = bench.CONFIGS[config]
config_utils._config_cache = {"n_embd": cfg["C"], "n_head": cfg["H"], "n_layer": cfg["L"], "block_size": cfg["T"],
                              "dropout": 0.1, "device": "cuda:0", "batch_size": cfg["B"], "eval_iters": iters,
                              "output_file_name": "", "project_file_path": ""}
data = mmt_data.make_synthetic(n_modalities=cfg["M"])
torch.manual_seed(1234)
m = MultimodalTransformer(cfg["M"], data["vocab_sizes"], data["params"]).to("cuda:0")
mmt_data.install(TU, data, m)
ms = []
for r in range(rounds + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        TU.estimate_loss()
    torch.cuda.synchronize()
    if r:  # the first call warms up
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
print(json.dumps(ms))
"""


def child_lines(parent, config, iters, rounds, procs):
    out = {"parent": [], "tree_last": []}
    for _ in range(procs):
        for name, root in (("parent", parent), ("tree_last", REPO)):
            r = subprocess.run([sys.executable, "-c", CHILD, config, str(iters), str(rounds)], cwd=root,
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"estimate_loss child failed in {root}:\n{r.stderr[-2000:]}")
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"child {name}: {out[name][-1]} ms", file=sys.stderr, flush=True)
    return out


def torch_tables(lg, xb, yb, values, is_pct, bins):
    """The same tables in torch ops: (pos [T, 8], rel [3, bins, 3], pit [bins]) of one modality, fp32 softmax, fp64
    sums. Not bit-compatible with the entry (other rounding, atomics in the scatter-adds): a timing yardstick."""
    import torch
    B, T, V = lg.shape
    lp = torch.log_softmax(lg, dim=-1)
    P = lp.exp()
    lpy = lp.gather(-1, yb.unsqueeze(-1)).squeeze(-1)
    zy = lg.gather(-1, yb.unsqueeze(-1))
    rank = (lg > zy).sum(-1)
    pred = lg.argmax(-1)
    if is_pct:
        sg = torch.sign(values).expand(B, T, V)
    else:
        sg = torch.sign(values.view(1, 1, V) - values[xb].unsqueeze(-1))
    masses = torch.stack([(P * (sg == s)).sum(-1, dtype=torch.float64) for s in (-1, 0, 1)], dim=-1)  # [B, T, 3]
    cum = P.cumsum(-1)
    py = P.gather(-1, yb.unsqueeze(-1)).squeeze(-1)
    pit_v = (cum.gather(-1, yb.unsqueeze(-1)).squeeze(-1) - 0.5 * py).double()
    ps = sg.gather(-1, pred.unsqueeze(-1)).squeeze(-1).long()
    rs = sg.gather(-1, yb.unsqueeze(-1)).squeeze(-1).long()
    cert = masses.gather(-1, (ps + 1).unsqueeze(-1)).squeeze(-1)
    real = masses.gather(-1, (rs + 1).unsqueeze(-1)).squeeze(-1)
    one = torch.ones(B, T, dtype=torch.float64, device=lg.device)
    pos = torch.stack([one, (ps == rs).double(), (ps != rs).double(), cert, -lpy.double(), (rank == 0).double(), one,
                       real], dim=-1).sum(0)
    edges = torch.arange(1, bins, device=lg.device, dtype=torch.float64) / bins
    rel = torch.zeros(3, bins, 3, dtype=torch.float64, device=lg.device)
    for d in range(3):
        k = torch.bucketize(masses[..., d].contiguous(), edges, right=True).reshape(-1)
        rel[d, :, 0].index_add_(0, k, one.reshape(-1))
        rel[d, :, 1].index_add_(0, k, masses[..., d].reshape(-1))
        rel[d, :, 2].index_add_(0, k, (rs == d - 1).double().reshape(-1))
    pit = torch.zeros(bins, dtype=torch.float64, device=lg.device)
    pit.index_add_(0, torch.bucketize(pit_v, edges, right=True).reshape(-1), one.reshape(-1))
    return pos, rel, pit


def entry_alone(Vs, values, pcts, B, T, dev, reps, rounds, bins=10):
    """us per call: the entry over all modalities, the torch formulation over all modalities, the mmt_eval_direction
    launches over all modalities."""
    import torch

    import mmt_eval
    import mmt_lib as ML
    per_set = sum(B * T * V * 4 for V in Vs)
    nset = max(2, (320 << 20) // per_set + 1)
    g = torch.Generator(device=dev).manual_seed(7)
    sets = []
    for _ in range(nset):
        lg = [torch.randn(B, T, V, device=dev, generator=g) * 2 for V in Vs]
        xb = [torch.randint(0, V, (B, T), device=dev, generator=g) for V in Vs]
        yb = [torch.randint(0, V, (B, T), device=dev, generator=g) for V in Vs]
        sets.append((lg, xb, yb))
    pm = mmt_eval.PositionMetrics(values, pcts, t_begin=0, bins=bins)
    L, s = ML.lib(), ML.stream_ptr(dev)
    acc_i = torch.zeros(2, dtype=torch.int32, device=dev)
    acc_c = torch.zeros(1, dtype=torch.float64, device=dev)

    def entry(k):
        pm.add(*sets[k % nset])

    def torch_form(k):
        lg, xb, yb = sets[k % nset]
        for i in range(len(Vs)):
            torch_tables(lg[i], xb[i], yb[i], values[i], pcts[i], bins)

    def direction(k):
        lg, xb, yb = sets[k % nset]
        for i, V in enumerate(Vs):
            ML.check(L.mmt_eval_direction(None, s, B, T, V, ML.ptr(lg[i]), ML.ptr(xb[i]), ML.ptr(yb[i]),
                                          ML.ptr(values[i]), 1 if pcts[i] else 0, ML.ptr(acc_i), ML.ptr(acc_c)), None,
                     "mmt_eval_direction")

    def timed(fn, n):
        for k in range(nset):
            fn(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for k in range(n):
            fn(k)
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / n * 1e3, 2)

    out = {"entry": [], "torch": [], "eval_direction": []}
    for _ in range(rounds):  # alternating
        out["entry"].append(timed(entry, reps))
        out["torch"].append(timed(torch_form, max(4, reps // 4)))
        out["eval_direction"].append(timed(direction, reps))
    # the entry alone is one stream of the logits: the bytes it must read over its time
    out["entry_logit_GBps"] = round(per_set / min(out["entry"]) / 1e3, 1)
    out["logit_MB_per_call"] = round(per_set / 1e6, 1)
    out["input_sets"] = nset
    res = pm.result()
    out["rows_checked"] = [r["rows"] for r in res]
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
        conf["eval_positions"] = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            TU.estimate_loss()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 3)

    for mode in ("last", "all"):
        timed(mode)
    ms = {"last": [], "all": []}
    for _ in range(rounds):
        for mode in ("last", "all"):
            ms[mode].append(timed(mode))
            print(f"estimate_loss {mode}: {ms[mode][-1]} ms", file=sys.stderr, flush=True)
    calls = 2 * iters  # train and val
    return {"config": config, "device": torch.cuda.get_device_name(0), "B": B, "T": T, "V": [Vs[i] for i in idx],
            "alone_us_per_call": alone, "eval_iters": iters, "estimate_loss_ms": ms,
            "all_over_last": round(min(ms["all"]) / min(ms["last"]), 4),
            "added_us_per_iteration": round((min(ms["all"]) - min(ms["last"])) / calls * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eval-iters", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its estimate_loss and this "
                                                   "tree's, in fresh child processes, alternating")
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16_eval_positions.txt"))
    a = ap.parse_args()
    lines = []
    if a.parent:  # first: this process has not opened the GPU yet
        c = child_lines(os.path.abspath(a.parent), a.config, a.eval_iters, a.rounds, a.procs)
        best = {k: min(min(v) for v in c[k]) for k in c}
        c["tree_last_over_parent"] = round(best["tree_last"] / best["parent"], 4)
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
