"""Cost of rollouts from a full context window: generate(num_samples=S, rolling=True) against the same call without
the keyword, which past block_size tiles the prompts and re-runs the whole forward over B*S windows per token.

C1 dimensions (d256, 8 heads, 6 layers, block 256, vocabularies 900 / 13 / 144 / 5, cross-attention on modality 0),
ONE prompt of n0 = block_size = 256 tokens, N new tokens of modality 0, temperature 1, seed 11, eval mode, freshly
initialised weights. Each timed call is one generate with one synchronisation at its end; the two calls alternate,
three passes after one warm-up each; paths per second is S / wall time, peak memory torch.cuda.max_memory_allocated
over one further call of each kind that starts without the model's workspace of the call before.

    python tools/rolling_cost.py [--passes 3] [--out FILE] [--shapes 64x16,64x64,512x16,512x64] [--big 4096x16]

--big runs rolling only: the tiled call needs a workspace of B*S sequences, whose size the tool reports
(mmt_workspace_bytes) instead of attempting it. The tool also times mmt_rolling_step alone by tail length m at S = 512
(HIP events around back-to-back calls after one prefix forward, best of the passes), beside the prefix forward every
rolling step also runs. One JSON line on stdout; --out also writes the table as text.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1 = dict(n_embd=256, n_head=8, n_layer=6, block_size=256, V=[900, 13, 144, 5], cross=[True, False, False, False])


def pairs(text):
    return [tuple(int(x) for x in p.split("x")) for p in text.split(",") if p]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--shapes", default="64x16,64x64,512x16,512x64", help="SxN pairs measured on both calls")
    ap.add_argument("--big", default="4096x16", help="SxN pairs measured on the rolling call only")
    ap.add_argument("--step-samples", type=int, default=512)
    ap.add_argument("--step-tails", default="1,2,4,8,16,32,63")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))
    import torch
    import config_utils
    import mmt_lib as ML
    from model import MultimodalTransformer
    dev = torch.device("cuda", 0)
    T = C1["block_size"]
    config_utils._config_cache = {"n_embd": C1["n_embd"], "n_head": C1["n_head"], "n_layer": C1["n_layer"],
                                  "block_size": T, "dropout": 0.0, "device": str(dev), "batch_size": 1, "eval_iters": 1}
    params = []
    for c in C1["cross"]:
        p = [None] * 12
        p[8] = c
        params.append(p)
    torch.manual_seed(1234)
    model = MultimodalTransformer(len(C1["V"]), C1["V"], params).to(dev)
    model.eval()
    g = torch.Generator().manual_seed(7)
    prompt = [torch.randint(0, v, (1, T), generator=g).to(dev) for v in C1["V"]]

    def one(S, N, rolling):
        kw = dict(max_new_tokens=N, modality_to_generate=0, temperature=1.0, seed=11, num_samples=S)
        if rolling:
            kw["rolling"] = True
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        seqs = model.generate(prompt, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(seqs[0].shape) == (S, T + N)
        assert model.last_generate_path == ("rolling" if rolling else "tiled"), model.last_generate_path
        return S / dt, int(torch.cuda.max_memory_allocated(dev))

    rows = []
    for S, N in pairs(a.shapes):
        rec = {"samples": S, "new_tokens": N, "rolling": [], "tiled": [], "peak_rolling": 0, "peak_tiled": 0}
        for name in ("rolling", "tiled"):
            one(S, N, name == "rolling")  # warm-up
        for _ in range(a.passes):  # the two calls alternate: each pass brackets the other
            for name in ("rolling", "tiled"):
                rec[name].append(round(one(S, N, name == "rolling")[0], 1))
        for name in ("rolling", "tiled"):  # the peak of one call that starts without the other call's workspace
            model._ws = None
            torch.cuda.empty_cache()
            rec["peak_" + name] = one(S, N, name == "rolling")[1]
        model._ws = None
        torch.cuda.empty_cache()
        rows.append(rec)
    for S, N in pairs(a.big):
        rec = {"samples": S, "new_tokens": N, "rolling": [], "tiled": None, "peak_rolling": 0,
               "tiled_workspace_bytes": int(ML.lib().mmt_workspace_bytes(model._ctx, S))}
        model._ws_bytes.clear()
        one(S, N, True)
        for _ in range(a.passes):
            pps, peak = one(S, N, True)
            rec["rolling"].append(round(pps, 1))
            rec["peak_rolling"] = max(rec["peak_rolling"], peak)
        rows.append(rec)
    steps = step_alone(torch, dev, model, prompt, a.step_samples, [int(x) for x in a.step_tails.split(",")], a.passes)
    res = {"tool": "rolling_cost", "device": torch.cuda.get_device_name(0), "prompt": T, "block_size": T,
           "passes": a.passes, "shapes": rows, "step_samples": a.step_samples, "step_us": steps}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(res))


def step_alone(torch, dev, model, prompt, S, tails, passes, reps=10):
    """us per mmt_rolling_step over S paths by tail length m (p = block_size - m), and per prefix forward (one
    sequence of block_size rows), which every rolling step of generate also runs."""
    T = C1["block_size"]
    g = torch.Generator().manual_seed(3)
    seqs = [torch.cat([p.repeat_interleave(S, 0), torch.randint(0, v, (S, T), generator=g).to(dev)], dim=1)
            for p, v in zip(prompt, C1["V"])]

    def timed(fn):
        best = None
        for _ in range(passes):
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
        return round(best, 1)

    out = {}
    with torch.no_grad():
        out["prefix_forward"] = timed(lambda: model(prompt))
        for m in tails:
            p = T - m
            # the sequences' columns p..p+m-1 stand for the paths' own tokens; the workspace holds the prompt's rows
            out[f"m{m}"] = timed(lambda: model._rolling_step(seqs, S, p, m))
    return out


def table(res):
    gb = lambda b: f"{b / 1e9:.2f} GB"  # noqa: E731
    span = lambda v: f"{min(v):.1f} - {max(v):.1f}"  # noqa: E731
    lines = [f"tools/rolling_cost.py on {res['device']}: C1 dimensions, one prompt of n0 = block_size = {res['prompt']} "
             f"tokens, modality 0, temperature 1, seed 11;", f"rolling=True and the tiled call alternating, "
             f"{res['passes']} passes after a warm-up each, min - max, one sync per call", "",
             "| S x N | tiled: paths/s | rolling: paths/s | rolling / tiled (worst / best) | peak, tiled | peak, rolling |",
             "|---|---|---|---|---|---|"]
    for r in res["shapes"]:
        if r["tiled"]:
            ratio = f"{min(r['rolling']) / max(r['tiled']):.2f} / {max(r['rolling']) / min(r['tiled']):.2f}"
            lines.append(f"| {r['samples']} x {r['new_tokens']} | {span(r['tiled'])} | {span(r['rolling'])} | {ratio} | "
                         f"{gb(r['peak_tiled'])} | {gb(r['peak_rolling'])} |")
        else:
            lines.append(f"| {r['samples']} x {r['new_tokens']} | does not fit: the workspace alone is "
                         f"{r['tiled_workspace_bytes'] / 2 ** 30:.1f} GiB | {span(r['rolling'])} | - | - | "
                         f"{gb(r['peak_rolling'])} |")
    lines += ["", f"mmt_rolling_step alone, S = {res['step_samples']} paths, us per call by tail length m (p = "
              f"{res['block_size']} - m), best of {res['passes']} x 10 back-to-back calls (the host wrapper's buffer "
              "allocation included); prefix_forward: the forward over the one prompt that every rolling step also runs",
              "", "| " + " | ".join(res["step_us"]) + " |", "|" + "---|" * len(res["step_us"]),
              "| " + " | ".join(str(v) for v in res["step_us"].values()) + " |", "", json.dumps(res), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
