"""Cost of the deterministic training mode (mmt_set_deterministic): ms/step with the mode off and on, on
one box in one process, timed the way bench.py times its headline (same model, synthetic data, device
batcher, AdamW, warm-up and step count, wall clock around the timed steps, no probe events in them).
Then, from separate probed steps, the `det_sum` total (the ordered-sum launches) and the per-label time
of every converted producer with the mode off and on (in the mode a producer's events also bracket its
ordered sum), sorted by what the mode adds.

    python tools/det_cost.py [--config c1,target] [--steps 200] [--warmup 20] [--rounds 2]
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "trade-aid-multimodal-transformer_amd"))

import torch  # noqa: E402

import bench  # noqa: E402

# launches that carry a converted sum (the engine's probe labels)
SITES = ["head2_db", "head2_dx", "head0_dx", "lnf_bwd", "ca_proj_dx", "ca_proj2_dx", "ca_q_dx", "lnc_bwd", "ca_kv_dx",
         "dres16", "ffn2_dx", "ffn0_dx", "ln2_bwd", "proj_dx", "proj2_dx", "attn_bwd", "qkv2_bwd", "qkv1_dx", "ln1_bwd"]


def run(config, steps, warmup, rounds, probe_steps):
    import config_utils
    import mmt_data
    import mmt_lib as ML
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
    opt = mmt_optim.AdamW(model.parameters(), lr=3e-4)
    batcher = TU.DeviceBatcher(data["train"], data["val"], V, [p[2] for p in data["params"]], data["file_lengths"],
                               data["is_percents"], T, B, dev, seed=1000)
    L_ = ML.lib()

    def step():
        xb, yb = batcher.next("train", 1)
        _, losses = model(xb, yb)
        opt.zero_grad(set_to_none=True)
        sum(losses).backward()
        opt.step()

    def timed(on):
        model.set_deterministic(on)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    ms = {False: [], True: []}
    for _ in range(rounds):  # off, on, off, on: the two modes bracket each other
        for on in (False, True):
            ms[on].append(timed(on))

    def probed(on, labels):
        model.set_deterministic(on)
        step()
        torch.cuda.synchronize()
        L_.mmt_probe_set(model._ctx, ",".join(labels).encode())
        L_.mmt_probe_enable(model._ctx, 1)
        for _ in range(probe_steps):
            step()
        torch.cuda.synchronize()
        out = {}
        tot, n = ctypes.c_double(), ctypes.c_int64()
        for i, lb in enumerate(labels):
            ML.check(L_.mmt_probe_read_at(model._ctx, i, ctypes.byref(tot), ctypes.byref(n), None, None), model._ctx,
                     "mmt_probe_read_at")
            out[lb] = (tot.value / probe_steps, n.value // probe_steps)
        L_.mmt_probe_set(model._ctx, None)
        return out

    ws = L_.mmt_workspace_bytes(model._ctx, B)
    det_sum = probed(True, ["det_sum"])["det_sum"]
    off, on = probed(False, SITES), probed(True, SITES)
    sites = sorted(({"label": lb, "off_ms": round(off[lb][0], 4), "on_ms": round(on[lb][0], 4),
                     "added_ms": round(on[lb][0] - off[lb][0], 4), "launches": on[lb][1]} for lb in SITES if on[lb][1]),
                   key=lambda d: -d["added_ms"])
    model.set_deterministic(False)
    return {"config": config, "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup,
            "ms_per_step_off": [round(x, 4) for x in ms[False]], "ms_per_step_on": [round(x, 4) for x in ms[True]],
            "cost_pct": round((min(ms[True]) / min(ms[False]) - 1.0) * 100.0, 3), "workspace_bytes": ws,
            "det_sum_ms_per_step": round(det_sum[0], 4), "det_sum_launches_per_step": det_sum[1], "sites": sites}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1,target")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--probe-steps", type=int, default=8)
    a = ap.parse_args()
    for config in a.config.split(","):
        print(json.dumps(run(config, a.steps, a.warmup, a.rounds, a.probe_steps)), flush=True)


if __name__ == "__main__":
    main()
