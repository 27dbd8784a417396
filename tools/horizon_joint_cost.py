"""Cost of joint horizon forecasts (mmt_horizon_joint, generate(horizon={"baskets", "pairs"})), on one box in one visit,
alternating:

  * the entry alone over the four C1 heads and 128 steps at 64 prompts x 1 path, 1 x 512 and 1 x 4096, with 2 baskets, 6
    pairs, three levels and two barriers, against a torch formulation of the same outputs (value gather, cumprod, the
    baskets as a matrix product, weighted sums for moments, masses, covariances and the 3 x 3 tables, sort + cumsum per
    basket for quantiles and tail means, cummax / cummin for the barriers). HIP events around batches of calls, min -
    max over alternating passes;
  * generate at C1 dimensions, prompt 128, 128 new tokens, "all" four heads with horizon=, without and with the two
    keys on this tree, and with --parent DIR (a built checkout of the parent commit) the parent's call without them:
    fresh child processes, alternating.

    python tools/horizon_joint_cost.py [--reps 20] [--passes 3] [--parent DIR] [--out profiles/r22_horizon_joint.txt]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_C1 = [900, 13, 144, 5]
COEFS = [[1.0, -0.5, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25]]
BARS = [[1.0, -1.0], [1.0, -1.0]]
PAIRS = [(p, q) for p in range(4) for q in range(p + 1, 4)]

# what a child process runs in the checkout given as its working directory: argv = B, S (0: none), joint (0 / 1), rounds
# -> ms per call. Without joint it uses only names the parent commit has.
CHILD = r"""
import json, os, sys, time
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "trade-aid-multimodal-transformer_amd"))
import torch, bench, config_utils, mmt_data, training_utils as TU
from model import MultimodalTransformer
B, S, joint, rounds = [int(x) for x in sys.argv[1:]]
cfg = bench.CONFIGS["c1"]
conf = {"n_embd": cfg["C"], "n_head": cfg["H"], "n_layer": cfg["L"], "block_size": cfg["T"], "dropout": 0.1,
        "device": "cuda:0", "batch_size": cfg["B"], "eval_iters": 1, "output_file_name": "", "project_file_path": ""}
config_utils._config_cache = conf
data = mmt_data.make_synthetic(n_modalities=cfg["M"])
torch.manual_seed(1234)
m = MultimodalTransformer(cfg["M"], data["vocab_sizes"], data["params"]).to("cuda:0")
mmt_data.install(TU, data, m)
m.eval()
g = torch.Generator().manual_seed(3)
Vs = data["vocab_sizes"]
prompt = [torch.randint(0, V, (B, 128), generator=g).cuda() for V in Vs]
hz = {"values": {i: torch.linspace(-2.0, 2.0, Vs[i], dtype=torch.float64) for i in range(4)},
      "is_percent": {0: True}, "barriers": {i: [1.0, -1.0] for i in range(4)}}
if joint:
    hz.update(baskets=[{"weights": {0: 1.0, 1: -0.5}, "barriers": [1.0, -1.0]},
                       {"weights": {i: 0.25 for i in range(4)}, "barriers": [1.0, -1.0]}], pairs="all")
kw = dict(max_new_tokens=128, modality_to_generate="all", seed=11, num_samples=S or None, horizon=hz)
ms = []
for r in range(rounds + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.generate(prompt, **kw)
    torch.cuda.synchronize()
    if r:
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
print(json.dumps(ms))
"""


def child(root, *args):
    r = subprocess.run([sys.executable, "-c", CHILD] + [str(x) for x in args], cwd=root, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed in {root}:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def span(xs):
    return f"{min(xs):10.2f} - {max(xs):10.2f}"


def children(parent, passes, rounds):
    """The lines of the generate comparison, fresh processes alternating."""
    lines = ["", f"generate, C1, prompt 128, 128 new tokens, horizon= over the four heads; ms per call, {rounds} calls "
                 f"after a warm-up in each of {passes} fresh processes per cell, alternating, min - max"]
    for B, S in ((64, 0), (1, 512), (1, 4096)):
        cells = {"tree   horizon": (REPO, 0), "tree   horizon + baskets + pairs": (REPO, 1)}
        if parent:
            cells = dict({"parent horizon": (parent, 0)}, **cells)
        got = {k: [] for k in cells}
        for _ in range(passes):
            for k, (root, joint) in cells.items():
                got[k] += child(root, B, S, joint, rounds)
                print(f"generate B={B} S={S} {k}: {got[k][-rounds:]}", file=sys.stderr, flush=True)
        lines.append(f"  {B} prompt(s) x {S or 1} path(s)")
        lines += [f"    {k:<36}{span(v)}" for k, v in got.items()]
        if parent:
            lo, hi = min(got["parent horizon"]), max(got["parent horizon"])
            t = got["tree   horizon"]
            inside = lo <= min(t) <= hi or lo <= max(t) <= hi or (min(t) <= lo and hi <= max(t))
            lines.append(f"    without the keys the tree's range {'overlaps' if inside else 'DOES NOT overlap'} the parent's")
    return lines


def entry_alone(reps, passes, steps=128):
    """The lines of the entry against the torch formulation."""
    sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))
    import torch

    import mmt_lib as ML
    dev = torch.device("cuda", 0)
    L, st = ML.lib(), ML.stream_ptr(dev)
    Vs, levels = V_C1, (0.05, 0.5, 0.95)

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

    lines = ["mmt_horizon_joint alone, us per call (three launches) over the four C1 heads x 128 steps, 2 baskets, 6 pairs, three levels, two barriers, against a "
             f"torch formulation of the same outputs on the same device. HIP events around {reps} calls, {passes} "
             "alternating passes, min - max."]
    g = torch.Generator().manual_seed(9)
    lv = torch.tensor(levels, dtype=torch.float64, device=dev)
    coef = torch.tensor(COEFS, dtype=torch.float64, device=dev)
    for rows in (64, 512, 4096):
        B, S = (64, 1) if rows == 64 else (1, rows)
        toks = [torch.randint(0, V, (rows, steps), generator=g).to(dev) for V in Vs]
        org = [torch.randint(0, V, (rows,), generator=g).to(dev) for V in Vs]
        vals = [torch.linspace(-2.0, 2.0, V, dtype=torch.float64, device=dev) for V in Vs]
        logw = (torch.randn(rows, generator=g, dtype=torch.float64) * 2.0).to(dev)
        pct = [True, False, False, False]

        # the raw call on preallocated outputs and scratch, as the horizon tools time theirs
        i32, i64, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
        new = lambda n, last, dt=torch.float64: [torch.empty(B, steps, last, dtype=dt, device=dev)  # noqa: E731
                                                 for _ in range(n)]
        outs = [new(2, 9), new(2, 3), new(2, 3, torch.int32), new(2, 3), new(2, 2), new(6, 22)]
        ess, live = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        nbytes = L.mmt_horizon_joint_scratch_bytes(4, B, S, steps, 2)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        host = [(i32 * 4)(*Vs), (vp * 4)(*[t.data_ptr() for t in toks]), (i64 * 4)(*[steps] * 4),
                (vp * 4)(*[v.data_ptr() for v in vals]), (i32 * 4)(*[int(x) for x in pct]),
                (vp * 4)(*[o.data_ptr() for o in org]), (i64 * 4)(*[1] * 4)]
        tail = [3, (f64 * 3)(*levels), 2, (f64 * 8)(*[a for c in COEFS for a in c]), 2,
                (f64 * 4)(*[u for b in BARS for u in b]), 6, (i32 * 12)(*[i for pq in PAIRS for i in pq])]
        tail += [(vp * len(ts))(*[t.data_ptr() for t in ts]) for ts in outs]
        tail += [ess.data_ptr(), live.data_ptr(), scratch.data_ptr(), nbytes]

        def entry(weighted):
            rc = L.mmt_horizon_joint(st, 4, B, S, steps, *host, logw.data_ptr() if weighted else None, *tail)
            assert rc == 0, rc

        def torch_form(weighted):
            xs, ds = [], []
            for i in range(4):
                v = vals[i][toks[i]]                                            # [rows, steps]
                if i == 0:
                    xs.append(((1.0 + v / 100.0).cumprod(1) - 1.0) * 100.0)
                    ds.append(torch.sign(v))
                else:
                    v0 = vals[i][org[i]][:, None]
                    xs.append(v - v0)
                    ds.append(torch.sign(v - torch.cat([v0, v[:, :-1]], dim=1)))
            x = torch.stack(xs).view(4, B, S, steps)
            d = torch.stack(ds).view(4, B, S, steps)
            w = (torch.exp(logw - logw.max()) if weighted else torch.ones_like(logw)).view(B, S, 1)
            W = w.sum(1, keepdim=True)
            (w * w).sum(1)
            y = torch.einsum("kp,pbsn->kbsn", coef, x)                          # the baskets
            hi, lo = y.clamp_min(0).cummax(3).values, y.clamp_max(0).cummin(3).values
            mean = (w * y).sum(2) / W[:, 0]
            (w * (y - mean.unsqueeze(2)) ** 2).sum(2), (w * (y < 0)).sum(2), (w * (y == 0)).sum(2), (w * (y > 0)).sum(2)
            (w * hi).sum(2), (w * lo).sum(2), y.amin(2), y.amax(2)
            for u in (1.0, -1.0):
                (w * ((hi >= u) if u > 0 else (lo <= u))).sum(2)
            ys, order = y.sort(dim=2)                                           # every (basket, prompt, step) column
            ws = w.expand(2, B, S, steps).gather(2, order)
            P, A = ws.cumsum(2), (ws * ys).cumsum(2)
            target = (lv.view(1, 1, 3, 1) * W.view(1, B, 1, 1)).expand(2, B, 3, steps)
            pos = torch.searchsorted(P.transpose(2, 3).contiguous(), target.transpose(2, 3).contiguous()).clamp_(max=S - 1)
            q = ys.transpose(2, 3).gather(3, pos)
            prev = (pos - 1).clamp_min(0)
            Pm = torch.where(pos > 0, P.transpose(2, 3).gather(3, prev), 0.0)
            Am = torch.where(pos > 0, A.transpose(2, 3).gather(3, prev), 0.0)
            tt = target.transpose(2, 3)
            (Am + (tt - Pm) * q) / tt
            mx = (w * x).sum(2) / W[:, 0]                                       # the pairs
            a = x - mx.unsqueeze(2)
            var = (w * a * a).sum(2) / W[:, 0]
            sx, sd = torch.sign(x).long() + 1, d.long() + 1
            for p, r in PAIRS:
                cov = (w * a[p] * a[r]).sum(1) / W[:, 0]
                cov / (var[p].sqrt() * var[r].sqrt())
                for s in (sx, sd):
                    cell = 3 * s[p] + s[r]
                    torch.zeros(B, 9, steps, dtype=torch.float64, device=dev).scatter_add_(
                        1, cell, w.expand(B, S, steps).contiguous()) / W

        for name, weighted in (("plain", False), ("weights", True)):
            ent, tor = [], []
            for _ in range(passes):
                ent.append(timed(lambda: entry(weighted)))
                tor.append(timed(lambda: torch_form(weighted)))
            lines.append(f"  rows {rows:5d} {name:<8} entry {span(ent)}   torch {span(tor)}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--skip-children", action="store_true", help="the entry alone only")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_horizon_joint.txt"))
    a = ap.parse_args()
    lines = ["Joint horizon forecasts: mmt_horizon_joint, generate(horizon={\"baskets\", \"pairs\"}), one MI355X.",
             "C1 dimensions (d256, 8 heads, 6 layers, block 256, V 900 / 13 / 144 / 5).", ""]
    tail = []
    if not a.skip_children:  # first: this process has not opened the GPU yet
        tail = children(os.path.abspath(a.parent) if a.parent else None, a.passes, a.rounds)
    lines += entry_alone(a.reps, a.passes) + tail
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
