"""estimate_loss with eval_positions: all against eval_positions: last, on the tiny synthetic setup of
test_gpu_train_utils.test_estimate_loss_end_to_end and from the same seeds: what was there stays byte for byte, the
new block and log lines have their form, and the position table at T - 1 is the directional metric that is printed."""
import datetime as real_datetime
import os
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, B, ITERS = 32, 8, 3
BLOCK = re.compile(r"\nPOSITION METRICS - (Train|Val) Set \(positions (\d+)\.\.(\d+)\)\n((?:  - [^\n]*\n)*)")
PCT = r"(?:\d+\.\d%|n/a)"
LINE = re.compile(r"^  - .{30,}?\d+/\d+ \(\d+\.\d%\) \| NLL \d+\.\d{4} \| top-1 \d+\.\d% \| ECE up \d\.\d{4} down "
                  rf"\d\.\d{{4}} \| quarters {PCT} {PCT} {PCT} {PCT}$")
DIRLOG = re.compile(r"   DIRECTIONAL PREDICTION (Train|Val) Set - (.*): Correct=([\d,]+) \| Incorrect=([\d,]+) \|")


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
    tmp = tmp_path_factory.mktemp("evalpos")
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
    """One estimate_loss from fixed seeds with the given config keys: (losses, stdout, log text)."""
    TU, cfg, tmp = setup
    monkeypatch.setattr(TU, "datetime", Clock)
    for k in ("eval_positions", "eval_positions_from"):
        cfg.pop(k, None)
    cfg.update(keys, output_file_name=name)
    random.seed(0)
    torch.manual_seed(0)
    TU._device_batcher[0] = None
    TU.last_position_metrics.clear()
    capsys.readouterr()
    out = TU.estimate_loss(3, 10)
    text = capsys.readouterr().out
    return out, text, open(os.path.join(tmp, "output", name)).read()


def test_all_adds_its_block_and_changes_nothing_else(setup, capsys, monkeypatch):
    TU = setup[0]
    base_out, base_text, base_log = run(setup, capsys, monkeypatch, "last.txt")
    assert "POSITION METRICS" not in base_text + base_log and not TU.last_position_metrics
    assert run(setup, capsys, monkeypatch, "last2.txt", eval_positions="last")[:2] == (base_out, base_text)
    out, text, log = run(setup, capsys, monkeypatch, "all.txt", eval_positions="all")
    assert out == base_out, (out, base_out)
    assert BLOCK.sub("", text) == base_text
    assert "".join(l for l in log.splitlines(True) if not l.startswith("   POSITION METRICS ")) == base_log
    blocks = BLOCK.findall(text)
    assert [(b[0], b[1], b[2]) for b in blocks] == [("Train", "0", str(T - 1)), ("Val", "0", str(T - 1))]
    directional = {}
    for state, name, ok, bad in DIRLOG.findall(log):
        directional[(state, name)] = (int(ok.replace(",", "")), int(bad.replace(",", "")))
    for (state, _, _, body), key in zip(blocks, ("train", "val")):
        rec = TU.last_position_metrics[key]
        lines = body.splitlines()
        assert len(lines) == len(rec["names"]) >= 1 and rec["batches"] == ITERS and rec["t_begin"] == 0
        for line, name, r in zip(lines, rec["names"], rec["results"]):
            assert LINE.match(line), line
            assert line.startswith(f"  - {name:<30}{r['wins']}/{r['wins'] + r['losses']} (")
            assert f"   POSITION METRICS {state} Set - {name}: {line[4 + max(30, len(name)):]}\n" in log
            # the last position, summed over the iterations, is the directional metric of the reference
            assert (int(r["pos"][T - 1, 1]), int(r["pos"][T - 1, 2])) == directional[(state, name)], (state, name)
            assert r["pos"][:, 0].tolist() == [ITERS * B] * T and r["rows"] == ITERS * B * T
            assert r["pit"].sum() == r["rows"] and np.isfinite(r["nll"]) and 0 <= r["ece"]["up"] <= 1
        # every scored modality has its line, in the order of the directional block
        assert [n for (s, n) in directional if s == state and sum(directional[(s, n)]) > 0] == rec["names"]
    # in the log the new lines follow the directional ones of their state
    order = [l.split(" - ")[0].strip() for l in log.splitlines() if l.strip()]
    n = len(TU.last_position_metrics["train"]["names"])
    assert order[-n:] == ["POSITION METRICS Val Set"] * n and order[-n - 1] == "DIRECTIONAL PREDICTION Val Set"
    full = {k: [r["pos"].copy() for r in v["results"]] for k, v in TU.last_position_metrics.items()}

    # eval_positions_from moves the range and nothing else
    out2, text2, log2 = run(setup, capsys, monkeypatch, "from.txt", eval_positions="all", eval_positions_from=T // 2)
    assert out2 == base_out and BLOCK.sub("", text2) == base_text
    assert [(b[1], b[2]) for b in BLOCK.findall(text2)] == [(str(T // 2), str(T - 1))] * 2
    for key in ("train", "val"):
        rec = TU.last_position_metrics[key]
        assert rec["t_begin"] == T // 2
        for r, pos in zip(rec["results"], full[key]):
            assert not r["pos"][:T // 2].any() and np.array_equal(r["pos"][T // 2:], pos[T // 2:])
            assert r["rows"] == ITERS * B * (T // 2) and np.isnan(r["accuracy_per_quarter"][:2]).all()
    for line in BLOCK.findall(text2)[0][3].splitlines():
        assert LINE.match(line) and "quarters n/a n/a " in line, line


def test_bad_keys_are_refused_before_anything_runs(setup, capsys, monkeypatch):
    with pytest.raises(ValueError, match="eval_positions"):
        run(setup, capsys, monkeypatch, "bad.txt", eval_positions="every")
    with pytest.raises(ValueError, match="eval_positions_from"):
        run(setup, capsys, monkeypatch, "bad.txt", eval_positions="all", eval_positions_from=T + 1)
