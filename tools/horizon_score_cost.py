"""Cost of scoring horizon forecasts (mmt_horizon_score, generate(realised=), estimate_loss with eval_rollout_paths),
on one box in one visit, alternating:

  * the entry alone over the four C1 heads and 128 steps at 64 prompts x 1 path, 1 x 512 and 1 x 4096, on the outputs
    of a mmt_horizon_stats call on the same inputs, against a torch formulation of CRPS + PIT + coverage (value
    gather, cumprod, sort of every (prompt, step) column, gather + cumsum of the weights, the gap sum, two masked
    sums, a comparison per level). HIP events around batches of calls, min - max over alternating passes;
  * generate at C1 dimensions, prompt 128, 128 new tokens, "all" four heads with horizon=, without and with realised=
    on this tree, and with --parent DIR (a built checkout of the parent commit) the parent's call without it: fresh
    child processes, alternating;
  * estimate_loss at bench.py's C1 setup with eval_rollout_paths 0 and 64 (16 steps) on this tree, and with --parent
    the parent's: fresh child processes, alternating.

    python tools/horizon_score_cost.py [--reps 20] [--passes 3] [--eval-iters 5] [--parent DIR]
                                       [--out profiles/r17_horizon_score.txt]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_C1 = [900, 13, 144, 5]

# what a child process runs in the checkout given as its working directory. mode "generate": argv = B, S (0: none),
# realised (0 / 1), rounds -> ms per call; mode "eval": argv = paths, steps, iters, rounds -> ms per estimate_loss.
# Without realised / with paths 0 it uses only names the parent commit has.
CHILD = r"""
import contextlib, io, json, os, sys, time
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "trade-aid-multimodal-transformer_amd"))
import torch, bench, config_utils, mmt_data, training_utils as TU
from model import MultimodalTransformer
mode, a = sys.argv[1], [int(x) for x in sys.argv[2:]]
cfg = bench.CONFIGS["c1"]
conf = {"n_embd": cfg["C"], "n_head": cfg["H"], "n_layer": cfg["L"], "block_size": cfg["T"], "dropout": 0.1,
        "device": "cuda:0", "batch_size": cfg["B"], "eval_iters": 1, "output_file_name": "", "project_file_path": ""}
config_utils._config_cache = conf
data = mmt_data.make_synthetic(n_modalities=cfg["M"])
torch.manual_seed(1234)
m = MultimodalTransformer(cfg["M"], data["vocab_sizes"], data["params"]).to("cuda:0")
mmt_data.install(TU, data, m)
m.eval()
ms = []
if mode == "generate":
    B, S, realised, rounds = a
    g = torch.Generator().manual_seed(3)
    Vs = data["vocab_sizes"]
    prompt = [torch.randint(0, V, (B, 128), generator=g).cuda() for V in Vs]
    kw = dict(max_new_tokens=128, modality_to_generate="all", seed=11, num_samples=S or None,
              horizon={"values": {i: torch.linspace(-2.0, 2.0, Vs[i], dtype=torch.float64) for i in range(4)},
                       "is_percent": {0: True}, "barriers": {i: [1.0, -1.0] for i in range(4)}})
    if realised:
        kw["realised"] = {i: torch.randint(0, Vs[i], (B, 128), generator=g).cuda() for i in range(4)}
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate(prompt, **kw)
        torch.cuda.synchronize()
        if r:
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
else:
    paths, steps, iters, rounds = a
    conf["eval_iters"] = iters
    if paths:
        conf.update(eval_rollout_paths=paths, eval_rollout_steps=steps)
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            TU.estimate_loss()
        torch.cuda.synchronize()
        if r:
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
print(json.dumps(ms))
"""


def child(root, mode, *args):
    r = subprocess.run([sys.executable, "-c", CHILD, mode] + [str(x) for x in args], cwd=root, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{mode} child failed in {root}:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def span(xs):
    return f"{min(xs):10.2f} - {max(xs):10.2f}"


def children(parent, passes, rounds, iters):
    """The lines of the generate and estimate_loss comparisons, fresh processes alternating."""
    lines = ["", f"generate, C1, prompt 128, 128 new tokens, horizon= over the four heads; ms per call, {rounds} calls "
                 f"after a warm-up in each of {passes} fresh processes per cell, alternating, min - max"]
    for B, S in ((64, 0), (1, 512), (1, 4096)):
        cells = {"tree   horizon": (REPO, 0), "tree   horizon + realised": (REPO, 1)}
        if parent:
            cells = dict({"parent horizon": (parent, 0)}, **cells)
        got = {k: [] for k in cells}
        for _ in range(passes):
            for k, (root, realised) in cells.items():
                got[k] += child(root, "generate", B, S, realised, rounds)
                print(f"generate B={B} S={S} {k}: {got[k][-rounds:]}", file=sys.stderr, flush=True)
        lines.append(f"  {B} prompt(s) x {S or 1} path(s)")
        lines += [f"    {k:<28}{span(v)}" for k, v in got.items()]
    lines += ["", f"estimate_loss, bench.py's C1 setup (B 64, T 256), eval_iters {iters} (train and val: {2 * iters} "
                  f"iterations a call); ms per call, {rounds} calls after a warm-up in each of {passes} fresh processes "
                  "per cell, alternating, min - max"]
    cells = {"tree   eval_rollout_paths 0": (REPO, 0), "tree   eval_rollout_paths 64, 16 steps": (REPO, 64)}
    if parent:
        cells = dict({"parent": (parent, 0)}, **cells)
    got = {k: [] for k in cells}
    for _ in range(passes):
        for k, (root, paths) in cells.items():
            got[k] += child(root, "eval", paths, 16, iters, rounds)
            print(f"estimate_loss {k}: {got[k][-rounds:]}", file=sys.stderr, flush=True)
    lines += [f"    {k:<42}{span(v)}" for k, v in got.items()]
    off, on = min(got["tree   eval_rollout_paths 0"]), min(got["tree   eval_rollout_paths 64, 16 steps"])
    lines.append(f"    64 paths x 16 steps per window add {(on - off) / (2 * iters):.2f} ms per iteration of 64 windows "
                 f"(best against best), {on / off:.2f}x the call")
    return lines


def entry_alone(reps, passes, steps=128):
    """The lines of the entry against the torch formulation."""
    sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))
    import torch

    import mmt_lib as ML
    import mmt_sample as MS
    dev = torch.device("cuda", 0)
    L, st = ML.lib(), ML.stream_ptr(dev)
    Vs, levels, bars = V_C1, (0.05, 0.5, 0.95), [[1.0, -1.0]] * 4

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    lines = ["mmt_horizon_score alone, us per call (three launches) over the four C1 heads x 128 steps, three levels, "
             "two barriers, 10 bins, accumulate = 1, against a torch formulation of CRPS + PIT + coverage on the same "
             f"device. HIP events around {reps} calls, {passes} alternating passes, min - max."]
    g = torch.Generator().manual_seed(9)
    for rows in (64, 512, 4096):
        B, S = (64, 1) if rows == 64 else (1, rows)
        toks = [torch.randint(0, V, (rows, steps), generator=g).to(dev) for V in Vs]
        real = [torch.randint(0, V, (B, steps), generator=g).to(dev) for V in Vs]
        org = [torch.randint(0, V, (rows,), generator=g).to(dev) for V in Vs]
        rorg = [torch.randint(0, V, (B,), generator=g).to(dev) for V in Vs]
        vals = [torch.linspace(-2.0, 2.0, V, dtype=torch.float64, device=dev) for V in Vs]
        logw = (torch.randn(rows, generator=g, dtype=torch.float64) * 2.0).to(dev)
        pct = [True, False, False, False]
        hl = MS.HorizonLaunch(Vs, [steps] * 4, pct, levels, bars)
        sl = MS.HorizonScoreLaunch(Vs, [steps] * 4, [steps] * 4, pct, levels, bars, 10)
        houts = MS.horizon_outputs(4, B, steps, hl.nq, hl.nb, dev)
        souts = MS.horizon_score_outputs(4, B, steps, sl.nq, sl.nb, 10, dev)
        for i in range(4):
            hl.tok[i], hl.values[i], hl.origin[i] = toks[i].data_ptr(), vals[i].data_ptr(), org[i].data_ptr()
            hl.stats[i], hl.qval[i], hl.qrow[i], hl.hit[i], hl.ess[i], hl.live[i] = [x.data_ptr() for x in houts[i]]
            sl.tok[i], sl.values[i], sl.origin[i] = toks[i].data_ptr(), vals[i].data_ptr(), org[i].data_ptr()
            sl.real[i], sl.real_origin[i] = real[i].data_ptr(), rorg[i].data_ptr()
            MS.bind_score_forecast(sl, i, houts[i][0], houts[i][1], houts[i][3])
            MS.bind_score_outputs(sl, i, souts[i])
        hbytes, sbytes = hl.scratch_bytes(L, B, S, steps), sl.scratch_bytes(L, B, S, steps)
        scratch = torch.empty(max(hbytes, sbytes, 16), dtype=torch.uint8, device=dev)
        lv = torch.tensor(levels, dtype=torch.float64, device=dev)

        def torch_form(weighted):
            for i in range(4):
                v, vr = vals[i][toks[i]], vals[i][real[i]]                  # [rows, steps], [B, steps]
                if i == 0:
                    x = ((1.0 + v / 100.0).cumprod(1) - 1.0) * 100.0
                    xr = ((1.0 + vr / 100.0).cumprod(1) - 1.0) * 100.0
                else:
                    x, xr = v - vals[i][org[i]][:, None], vr - vals[i][rorg[i]][:, None]
                x = x.view(B, S, steps)
                xs, order = x.sort(dim=1)                                   # every (prompt, step) column
                w = (torch.exp(logw - logw.max()) if weighted else torch.ones_like(logw)).view(B, S, 1)
                W = w.sum(1, keepdim=True)
                F = w.expand(B, S, steps).gather(1, order).cumsum(1) / W
                t = xr.view(B, 1, steps)
                lo_x, hi_x, Fm = xs[:, :-1], xs[:, 1:], F[:, :-1]
                s = torch.minimum(hi_x, torch.maximum(lo_x, t))
                crps = ((s - lo_x) * Fm * Fm + (hi_x - s) * (1 - Fm) * (1 - Fm)).sum(1)
                crps = crps + (xs[:, 0] - xr).clamp_min(0) + (xr - xs[:, -1]).clamp_min(0)
                pit = ((w * (x < t)).sum(1) + 0.5 * (w * (x == t)).sum(1)) / W[:, 0]
                pos = torch.searchsorted(F.transpose(1, 2).contiguous(), lv.view(1, 1, 3).expand(B, steps, 3).contiguous())
                q = xs.transpose(1, 2).gather(2, pos.clamp_(max=S - 1))
                cover = (xr.unsqueeze(-1) <= q).sum(0)
                crps.sum(0), torch.histc(pit, 10, 0.0, 1.0), cover

        for name, weighted in (("plain", False), ("weights", True)):
            lw = logw.data_ptr() if weighted else 0
            hl.run(L, st, B, S, steps, lw, scratch.data_ptr(), hbytes)  # the forecast the entry scores
            ent, tor = [], []
            for _ in range(passes):
                ent.append(timed(lambda: sl.run(L, st, B, S, steps, lw, scratch.data_ptr(), sbytes, accumulate=True)))
                tor.append(timed(lambda: torch_form(weighted)))
            lines.append(f"  rows {rows:5d} {name:<8} entry {span(ent)}   torch {span(tor)}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eval-iters", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--skip-children", action="store_true", help="the entry alone only")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17_horizon_score.txt"))
    a = ap.parse_args()
    lines = ["Scores of horizon forecasts: mmt_horizon_score, generate(realised=), estimate_loss(eval_rollout_paths), one "
             "MI355X.", "C1 dimensions (d256, 8 heads, 6 layers, block 256, V 900 / 13 / 144 / 5).", ""]
    tail = []
    if not a.skip_children:  # first: this process has not opened the GPU yet
        tail = children(os.path.abspath(a.parent) if a.parent else None, a.passes, a.rounds, a.eval_iters)
    lines += entry_alone(a.reps, a.passes) + tail
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
