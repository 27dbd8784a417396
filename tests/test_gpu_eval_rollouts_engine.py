"""estimate_loss with eval_rollout_paths: 8 against eval_rollout_paths: 0 (and against the key being absent), on the tiny
synthetic setup of test_gpu_eval_positions_engine.py and from the same seeds: what was there stays byte for byte
(losses, every printed and written line, the next training batch), the new block and log lines have their form, every
window is scored, and two runs give identical tables."""
import datetime as real_datetime
import os
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, B, ITERS, H, PATHS = 32, 8, 3, 4, 8
BLOCK = re.compile(r"\nROLLOUT METRICS - (Train|Val) Set \((\d+) paths, (\d+) steps from position (\d+)\)\n"
                   r"((?:  - [^\n]*\n)*)")
PCT = r"(?:-?\d+\.\d+%|n/a)"
STEP = (rf"step \d+: skill (?:-?\d+\.\d{{3}}|n/a) \| coverage 5\.0%:{PCT} 50\.0%:{PCT} 95\.0%:{PCT} \| "
        rf"direction {PCT} \| PIT dev \d\.\d{{3}}")
LINE = re.compile(rf"^  - .{{30,}}?{STEP} \|\| {STEP} \|\| {STEP}$")


class Clock:
    @staticmethod
    def now():
        return real_datetime.datetime(2025, 1, 1, 12, 0, 0)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import config_utils
    import mmt_data
    import training_utils as TU
    from model import MultimodalTransformer
    tmp = tmp_path_factory.mktemp("evalroll")
    data = mmt_data.make_synthetic(n_rows=40_000, n_files=10)
    old = config_utils._config_cache
    cfg = {"n_embd": 64, "n_head": 2, "n_layer": 1, "block_size": T, "dropout": 0.1, "device": "cuda",
           "batch_size": B, "eval_iters": ITERS, "output_file_name": "log.txt", "project_file_path": str(tmp) + "/"}
    config_utils._config_cache = cfg
    torch.manual_seed(0)
    m = MultimodalTransformer(4, data["vocab_sizes"], data["params"]).to("cuda")
    mmt_data.install(TU, data, m)
    yield TU, cfg, str(tmp)
    config_utils._config_cache = old
    TU._device_batcher[0] = None


def run(setup, capsys, monkeypatch, name, **keys):
    """One estimate_loss from fixed seeds with the given config keys, then the next training batch: (losses, stdout,
    log text, batch)."""
    TU, cfg, tmp = setup
    monkeypatch.setattr(TU, "datetime", Clock)
    for k in ("eval_rollout_paths", "eval_rollout_steps", "eval_rollout_seed"):
        cfg.pop(k, None)
    cfg.update(keys, output_file_name=name)
    random.seed(0)
    torch.manual_seed(0)
    TU._device_batcher[0] = None
    TU.last_rollout_metrics.clear()
    capsys.readouterr()
    out = TU.estimate_loss(3, 10)
    text = capsys.readouterr().out
    xb, yb = TU.get_batch("train", 1)
    batch = [t.cpu().clone() for t in list(xb) + list(yb)]
    return out, text, open(os.path.join(tmp, "output", name)).read(), batch


def test_rollouts_add_their_block_and_change_nothing_else(setup, capsys, monkeypatch):
    TU = setup[0]
    base_out, base_text, base_log, base_batch = run(setup, capsys, monkeypatch, "absent.txt")
    assert "ROLLOUT METRICS" not in base_text + base_log and not TU.last_rollout_metrics
    off = run(setup, capsys, monkeypatch, "off.txt", eval_rollout_paths=0, eval_rollout_steps=H)
    assert off[:3] == (base_out, base_text, base_log) and not TU.last_rollout_metrics
    assert all(torch.equal(a, b) for a, b in zip(off[3], base_batch))

    out, text, log, batch = run(setup, capsys, monkeypatch, "on.txt", eval_rollout_paths=PATHS, eval_rollout_steps=H)
    assert out == base_out, (out, base_out)
    assert BLOCK.sub("", text) == base_text
    assert "".join(l for l in log.splitlines(True) if not l.startswith("   ROLLOUT METRICS ")) == base_log
    assert len(batch) == len(base_batch) and all(torch.equal(a, b) for a, b in zip(batch, base_batch))
    blocks = BLOCK.findall(text)
    assert [b[:4] for b in blocks] == [("Train", str(PATHS), str(H), str(T - H)), ("Val", str(PATHS), str(H), str(T - H))]
    for (state, _, _, _, body), key in zip(blocks, ("train", "val")):
        rec = TU.last_rollout_metrics[key]
        lines = body.splitlines()
        assert len(lines) == len(rec["names"]) >= 1 and rec["batches"] == ITERS
        assert (rec["paths"], rec["steps"]) == (PATHS, H) and rec["indices"] == sorted(rec["results"])
        for line, i in zip(lines, rec["indices"]):
            name, r = rec["names"][i], rec["results"][i]
            assert LINE.match(line), line
            assert line.startswith(f"  - {name:<30}step 1: skill ")
            assert f"   ROLLOUT METRICS {state} Set - {name}: {line[4 + max(30, len(name)):]}\n" in log
            # a clean vocabulary: every window of every iteration is scored at every step
            assert r["agg"].shape == (H, 10) and r["agg"][:, 0].tolist() == [ITERS * B] * H
            assert r["pit"].sum(axis=1).tolist() == [ITERS * B] * H and r["aggq"].shape == (H, 3, 2)
            assert np.isfinite(r["crps"]).all() and (r["crps"] >= 0).all()
            assert ((r["coverage"] >= 0) & (r["coverage"] <= 1)).all()
            assert (np.diff(r["coverage"], axis=1) >= 0).all()  # a higher level covers no less
    # in the log the new lines follow the directional ones of their state
    order = [l.split(" - ")[0].strip() for l in log.splitlines() if l.strip()]
    n = len(TU.last_rollout_metrics["val"]["names"])
    assert order[-n:] == ["ROLLOUT METRICS Val Set"] * n and order[-n - 1] == "DIRECTIONAL PREDICTION Val Set"
    first = {k: {i: {t: r[t].copy() for t in ("agg", "aggq", "aggb", "pit")} for i, r in v["results"].items()}
             for k, v in TU.last_rollout_metrics.items()}

    # run to run: the same seeds give the same tables, bit for bit
    again = run(setup, capsys, monkeypatch, "on2.txt", eval_rollout_paths=PATHS, eval_rollout_steps=H)
    assert again[:2] == (out, text) and again[2] == log
    for k, v in TU.last_rollout_metrics.items():
        for i, r in v["results"].items():
            for t in ("agg", "aggq", "aggb", "pit"):
                assert np.array_equal(r[t].view(np.int64), first[k][i][t].view(np.int64)), (k, i, t)
    # another seed moves the paths, not what was there before
    other = run(setup, capsys, monkeypatch, "seed.txt", eval_rollout_paths=PATHS, eval_rollout_steps=H,
                eval_rollout_seed=5)
    assert other[0] == base_out and BLOCK.sub("", other[1]) == base_text
    assert any(not np.array_equal(r["agg"], first[k][i]["agg"]) for k, v in TU.last_rollout_metrics.items()
               for i, r in v["results"].items())


def test_bad_keys_are_refused_before_anything_runs(setup, capsys, monkeypatch):
    TU = setup[0]
    for keys, match in ((dict(eval_rollout_paths=-1), "eval_rollout_paths"),
                        (dict(eval_rollout_paths=4097), "eval_rollout_paths"),
                        (dict(eval_rollout_paths=8, eval_rollout_steps=T), "eval_rollout_steps"),
                        (dict(eval_rollout_paths=8, eval_rollout_steps=0), "eval_rollout_steps"),
                        (dict(eval_rollout_paths=8, eval_rollout_steps=H, eval_rollout_seed=-1), "eval_rollout_seed")):
        TU.m.train()
        with pytest.raises(ValueError, match=match):
            run(setup, capsys, monkeypatch, "bad.txt", **keys)
        assert TU.m.training  # refused before the model changes mode
