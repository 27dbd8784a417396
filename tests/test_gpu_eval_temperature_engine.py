"""The calibrated temperatures end to end: TemperatureFit over batches, the fit on device tables against the
restatement, the bracket property on the device, estimate_loss with eval_temperature: fit on the tiny synthetic setup
of test_gpu_eval_positions_engine.py (same seeds: what was there stays byte for byte), and
generate(temperature="calibrated") against the call with the stored numbers."""
import datetime as real_datetime
import os
import random
import re

import numpy as np
import pytest
import torch

import calib_ref as C
import eval_ref as E

pytestmark = pytest.mark.gpu

T, B, ITERS = 32, 8, 3
BLOCK = re.compile(r"\nTEMPERATURE FIT - (Train|Val) Set\n((?:  - [^\n]*\n)*)")
NUM = r"(?:\d+\.\d{4}|n/a)"
LINE = re.compile(rf"^  - .{{30,}}?tau\* \d+\.\d{{4}}(?: \(at the grid's edge\))? \| NLL {NUM} -> {NUM} \| "
                  rf"ECE up {NUM} -> {NUM} down {NUM} -> {NUM}$")


def same(a, b):
    return np.array_equal(E.bits(a), E.bits(b))


def batches(n=3, Bn=4, Tn=6, Vs=(13, 40)):
    dev = torch.device("cuda")
    rng = np.random.default_rng(11)
    out = []
    for _ in range(n):
        lg = [torch.from_numpy(rng.normal(0.0, 2.0, size=(Bn, Tn, V)).astype(np.float32)).to(dev) for V in Vs]
        xb = [torch.from_numpy(rng.integers(0, V, size=(Bn, Tn))).to(dev) for V in Vs]
        yb = [torch.from_numpy(rng.integers(0, V, size=(Bn, Tn))).to(dev) for V in Vs]
        out.append((lg, xb, yb))
    values = [torch.from_numpy(E.series(V, "value")).to(dev) for V in Vs]
    return out, values, [False, True]


def test_fit_over_batches_and_derive():
    import mmt_eval as ME
    bs, values, pct = batches()
    tf = ME.TemperatureFit(values, pct, t_begin=1, bins=10)
    for lg, xb, yb in bs:
        tf.add(lg, xb, yb)
    res = tf.result()
    assert tf.batches == 3 and len(res) == 2
    each = [ME.temperature_metrics(lg, xb, yb, values, pct, t_begin=1) for lg, xb, yb in bs]
    cat = ME.temperature_metrics(*[[torch.cat([b[j][p] for b in bs]) for p in range(2)] for j in range(3)], values, pct,
                                 t_begin=1)
    temps = tf.temperatures()
    for p in range(2):
        tot, rel = res[p]["sum"], res[p]["rel"]
        ctot, crel = cat[p]["sum"].cpu().numpy(), cat[p]["rel"].cpu().numpy()
        # the exact counts are those of the concatenated batch
        assert np.array_equal(tot[:, 0], ctot[:, 0]) and (tot[:, 0] == 3 * 4 * 5).all()
        assert np.array_equal(rel[..., 0], crel[..., 0]) and np.array_equal(rel[..., 2], crel[..., 2])
        assert np.allclose(tot[:, 1], ctot[:, 1], rtol=1e-12) and np.allclose(rel[..., 1], crel[..., 1], rtol=1e-12)
        # every cell is the per-batch tables added in order, one fp64 addition each
        wtot, wrel = np.zeros_like(tot), np.zeros_like(rel)
        for e in each:
            wtot, wrel = wtot + e[p]["sum"].cpu().numpy(), wrel + e[p]["rel"].cpu().numpy()
        assert same(tot, wtot) and same(rel, wrel)
        # the derived numbers are the restatement's on the same tables
        want = C.derive(tot, rel, temps)
        got = res[p]
        assert (got["tau"], got["k_star"], got["at_bound"], got["k_one"], got["rows"]) == (
            want["tau"], want["k_star"], want["at_bound"], want["k_one"], want["rows"])
        assert same(got["nll"], want["nll"])
        for name in ("down", "flat", "up"):
            assert np.allclose(got["ece"][name], want["ece"][name], rtol=1e-15, atol=0, equal_nan=True)
        assert got["k_one"] == 8 and got["at_bound"] and got["k_star"] == 16  # random targets: the flatter the better
    lines = tf.summary_lines(["a", "b"], res)
    assert len(lines) == 2 and lines[0].startswith("  - a" + " " * 29 + "tau* 4.0000 (at the grid's edge) | NLL ")
    with pytest.raises(ValueError, match="first batch"):
        tf.add([t[:2] for t in bs[0][0]], [t[:2] for t in bs[0][1]], [t[:2] for t in bs[0][2]])


def test_bracket_property_on_the_device():
    """The input of test_calib_ref_cpu's bracket test: the minimiser of the true NLL and the fitted tau* both lie
    strictly between the grid neighbours of the device's k*."""
    import mmt_eval as ME
    dev = torch.device("cuda")
    x, yb = C.bracket_input()
    lg = torch.from_numpy(x[:, None, :].copy()).to(dev)
    tok = torch.from_numpy(yb[:, None].copy()).to(dev)
    (got,) = ME.temperature_metrics([lg], [tok], [tok], [None], [False])
    r = ME.derive_temperature(got["sum"].cpu().numpy(), got["rel"].cpu().numpy(), ME.default_temperatures())
    grid, ks = ME.default_temperatures(), r["k_star"]
    assert r["rows"] == 4096 and 0 < ks < 16 and not r["at_bound"]
    tau_hat = C.newton_tau(x, yb)
    assert grid[ks - 1] < tau_hat < grid[ks + 1] and grid[ks - 1] < r["tau"] < grid[ks + 1]
    assert r["nll"][ks] < r["nll"][8]  # the targets came from tau = 1.7: tau = 1 is over-confident
    print(f"device fit {r['tau']:.5f}, newton {tau_hat:.5f}, NLL {r['nll'][8]:.5f} -> {r['nll'][ks]:.5f}")


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
    tmp = tmp_path_factory.mktemp("evaltemp")
    data = mmt_data.make_synthetic(n_rows=40_000, n_files=10)
    old = config_utils._config_cache
    cfg = {"n_embd": 64, "n_head": 2, "n_layer": 1, "block_size": T, "dropout": 0.1, "device": "cuda",
           "batch_size": B, "eval_iters": ITERS, "output_file_name": "log.txt", "project_file_path": str(tmp) + "/"}
    config_utils._config_cache = cfg
    torch.manual_seed(0)
    m = MultimodalTransformer(4, data["vocab_sizes"], data["params"]).to("cuda")
    mmt_data.install(TU, data, m)
    yield TU, cfg, str(tmp), m
    config_utils._config_cache = old
    TU._device_batcher[0] = None


def run(setup, capsys, monkeypatch, name, **keys):
    """One estimate_loss from fixed seeds with the given config keys: (losses, stdout, log text)."""
    TU, cfg, tmp, m = setup
    monkeypatch.setattr(TU, "datetime", Clock)
    for k in ("eval_positions", "eval_positions_from", "eval_temperature"):
        cfg.pop(k, None)
    cfg.update(keys, output_file_name=name)
    random.seed(0)
    torch.manual_seed(0)
    TU._device_batcher[0] = None
    TU.last_temperature_fit.clear()
    capsys.readouterr()
    out = TU.estimate_loss(3, 10)
    text = capsys.readouterr().out
    return out, text, open(os.path.join(tmp, "output", name)).read()


def test_estimate_loss_fit_adds_its_block_and_changes_nothing_else(setup, capsys, monkeypatch):
    TU, cfg, tmp, m = setup
    m.set_calibrated_temperatures(None)
    base_out, base_text, base_log = run(setup, capsys, monkeypatch, "absent.txt")
    assert "TEMPERATURE FIT" not in base_text + base_log and not TU.last_temperature_fit
    assert m.calibrated_temperatures == {}
    off = run(setup, capsys, monkeypatch, "off.txt", eval_temperature="off")
    assert off == (base_out, base_text, base_log) and not TU.last_temperature_fit and m.calibrated_temperatures == {}
    out, text, log = run(setup, capsys, monkeypatch, "fit.txt", eval_temperature="fit")
    assert out == base_out, (out, base_out)
    assert BLOCK.sub("", text) == base_text
    assert "".join(l for l in log.splitlines(True) if not l.startswith("   TEMPERATURE FIT ")) == base_log
    blocks = BLOCK.findall(text)
    assert [b[0] for b in blocks] == ["Train", "Val"]
    for (state, body), key in zip(blocks, ("train", "val")):
        rec = TU.last_temperature_fit[key]
        lines = body.splitlines()
        assert len(lines) == len(rec["names"]) == len(rec["indices"]) >= 2 and rec["batches"] == ITERS
        assert rec["t_begin"] == 0 and len(rec["temperatures"]) == 17
        for line, name, r in zip(lines, rec["names"], rec["results"]):
            assert LINE.match(line), line
            assert f"   TEMPERATURE FIT {state} Set - {name}: {line[4 + max(30, len(name)):]}\n" in log
            assert r["rows"] == ITERS * B * T and r["sum"].shape == (17, 2) and r["rel"].shape == (17, 3, 10, 3)
            assert np.isfinite(r["nll"]).all() and r["k_star"] >= 0 and r["nll"][r["k_star"]] <= r["nll"][8]
    # the block follows the directional one of its state, and in the log the new lines close the state's lines
    assert text.index("DIRECTIONAL METRICS - Train Set") < text.index("TEMPERATURE FIT - Train Set") < text.index(
        "DIRECTIONAL METRICS - Val Set") < text.index("TEMPERATURE FIT - Val Set")
    order = [l.split(" - ")[0].strip() for l in log.splitlines() if l.strip()]
    n = len(TU.last_temperature_fit["val"]["names"])
    assert order[-n:] == ["TEMPERATURE FIT Val Set"] * n and order[-n - 1] == "DIRECTIONAL PREDICTION Val Set"
    # the val fit is what the model holds from here on
    val = TU.last_temperature_fit["val"]
    assert m.calibrated_temperatures == {i: r["tau"] for i, r in zip(val["indices"], val["results"])}
    assert all(math_ok(t) for t in m.calibrated_temperatures.values())

    # with the position metrics on, the block comes after theirs; eval_positions_from moves both
    out2, text2, log2 = run(setup, capsys, monkeypatch, "both.txt", eval_temperature="fit", eval_positions="all",
                            eval_positions_from=T // 2)
    assert out2 == base_out
    assert text2.index("POSITION METRICS - Train Set") < text2.index("TEMPERATURE FIT - Train Set") < text2.index(
        "POSITION METRICS - Val Set") < text2.index("TEMPERATURE FIT - Val Set")
    for key in ("train", "val"):
        rec = TU.last_temperature_fit[key]
        assert rec["t_begin"] == T // 2 and all(r["rows"] == ITERS * B * (T // 2) for r in rec["results"])
        # at tau = 1 the fit's NLL and reliability tables are the position metrics' own
        for r, pr in zip(rec["results"], TU.last_position_metrics[key]["results"]):
            assert same(r["rel"][8], pr["rel"]) and r["nll"][8] == pytest.approx(pr["nll"], rel=1e-12)
    with pytest.raises(ValueError, match="eval_temperature"):
        run(setup, capsys, monkeypatch, "bad.txt", eval_temperature="always")


def math_ok(t):
    return isinstance(t, float) and 0.0 < t < float("inf")


def test_generate_calibrated_is_the_call_with_the_stored_numbers(setup):
    TU, cfg, tmp, m = setup
    m.eval()
    m.set_calibrated_temperatures(None)
    xb, _ = TU.get_batch("val", 0)
    prompts = [x[:2, :10].contiguous() for x in xb]
    full = [x[:2].contiguous() for x in xb]
    with pytest.raises(ValueError, match="modality 0 has no calibrated temperature"):
        m.generate(prompts, 3, 0, temperature="calibrated", seed=5)
    m.set_calibrated_temperatures({0: 1.3, 1: 0.7})
    with pytest.raises(ValueError, match="modality 2 has no calibrated temperature"):
        m.generate(prompts, 3, "all", temperature="calibrated", seed=5)
    with pytest.raises(ValueError, match="sample_fn"):
        m.generate(prompts, 3, 0, temperature="calibrated", sample_fn=lambda p: p.argmax(-1, keepdim=True))

    def equal(a, b):
        if isinstance(a, torch.Tensor):
            return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
                a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
        return a == b

    cases = [
        ("int", prompts, dict(modality_to_generate=0), 1.3, None),
        ("list", prompts, dict(modality_to_generate=[0, 1], forecast=True), {0: 1.3, 1: 0.7}, None),
        ("samples", prompts, dict(modality_to_generate=[1, 0], num_samples=4, forecast=True), {0: 1.3, 1: 0.7},
         "fanout"),
        ("int samples", prompts, dict(modality_to_generate=1, num_samples=4), 0.7, "fanout"),
        ("rolling", full, dict(modality_to_generate=[0, 1], num_samples=4, rolling=True, forecast=True),
         {0: 1.3, 1: 0.7}, "rolling"),
    ]
    for what, idx, kw, numbers, path in cases:
        a = m.generate(idx, 3, temperature="calibrated", seed=17, return_logprobs=True, **kw)
        pa = m.last_generate_path
        b = m.generate(idx, 3, temperature=numbers, seed=17, return_logprobs=True, **kw)
        assert equal(a, b), what
        assert pa == m.last_generate_path and (path is None or pa == path), (what, pa)
        c = m.generate(idx, 3, temperature=1.0, seed=17, return_logprobs=True, **kw)
        assert not equal(a, c), (what, "the temperature has no effect")
    assert m.calibrated_temperatures == {0: 1.3, 1: 0.7}
    assert "calibrated_temperatures" not in m.state_dict() and not any("calibrated" in k for k in m.state_dict())
    m.set_calibrated_temperatures(None)
    assert m.calibrated_temperatures == {}
