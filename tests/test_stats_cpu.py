"""Host-side checks of the per-tensor statistics (no compute calls): the config key `grad_stats`, the ctypes
mirrors of mmt_tensor_stat / mmt_stats_header and the size queries of the C ABI, the segment builder,
StatsReport's rollups and its log line on a hand-made record, and the `stats=` argument of mmt_optim.AdamW."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import config_utils
import mmt_lib as ML
import mmt_optim
import mmt_stats


@pytest.fixture
def clean_config():
    old = config_utils._config_cache
    yield
    config_utils._config_cache = old


# ------------------------------------------------------------------------------------------------ config
def test_grad_stats_key(clean_config, tmp_path, monkeypatch):
    config_utils._config_cache = {"n_embd": 64}  # the key absent
    assert config_utils._get_grad_stats() == "off"
    assert config_utils._DEFAULTS["training_parameters"]["grad_stats"] == "off"
    for v in ("off", "skipped", "every"):
        config_utils._config_cache = {"grad_stats": v}
        assert config_utils._get_grad_stats() == v
    monkeypatch.chdir(tmp_path)
    assert config_utils.load_system_config()["grad_stats"] == "off"  # no config.yaml at all
    for text, want in (("skipped", "skipped"), ("every", "every"), ("off", "off"), ("'off'", "off")):
        (tmp_path / "config.yaml").write_text(f"training_parameters:\n  grad_stats: {text}\n")
        config_utils._config_cache = config_utils.load_system_config()
        assert config_utils._get_grad_stats() == want, text  # YAML reads a bare off as false: still "off"


@pytest.mark.parametrize("bad", [True, 0, 1, None, "on", "Every", "skip", "", ["every"], 2.5])
def test_grad_stats_bad_values(clean_config, bad):
    config_utils._config_cache = {"grad_stats": bad}
    with pytest.raises(ValueError, match="grad_stats"):
        config_utils._get_grad_stats()


# ------------------------------------------------------------------------------------------------ ABI mirrors
def test_struct_mirrors_and_size_queries():
    assert ctypes.sizeof(ML.MmtTensorStat) == 40
    assert ctypes.sizeof(ML.MmtStatsHeader) == 32
    assert [(f[0], getattr(ML.MmtTensorStat, f[0]).offset) for f in ML.MmtTensorStat._fields_] == [
        ("sqsum", 0), ("nan_count", 8), ("inf_count", 16), ("first_bad", 24), ("absmax", 32), ("reserved", 36)]
    assert [(f[0], getattr(ML.MmtStatsHeader, f[0]).offset) for f in ML.MmtStatsHeader._fields_] == [
        ("valid", 0), ("nseg", 4), ("applied_steps", 8), ("skipped_steps", 16), ("reserved", 24)]
    L = ML.lib()
    assert L.mmt_stats_chunk() == ML.STATS_CHUNK and ML.STATS_CHUNK % 1024 == 0
    assert (ML.STATS_ALWAYS, ML.STATS_ON_SKIP) == (0, 1)
    assert L.mmt_stats_record_bytes(0) == 32
    assert L.mmt_stats_record_bytes(7) == 32 + 7 * 40
    assert L.mmt_stats_record_bytes(-1) == -1
    # one 32-byte slot per (chunk, segment) pair index c + s < chunks + segments
    assert L.mmt_stats_scratch_bytes(3 * ML.STATS_CHUNK + 1, 5) == 32 * (4 + 5)
    assert L.mmt_stats_scratch_bytes(0, 0) >= 16
    assert L.mmt_stats_scratch_bytes(-1, 0) == -1 and L.mmt_stats_scratch_bytes(0, -1) == -1
    for name in ("mmt_tensor_stats", "mmt_stats_record_bytes", "mmt_stats_scratch_bytes", "mmt_stats_chunk"):
        assert name in ML.EXPORTED and hasattr(L, name)


def test_invalid_arguments_are_rejected_before_any_launch():
    """Runs without a device: every one of these returns before the first launch."""
    L = ML.lib()
    ok = ctypes.c_void_p(4096)  # non-null, 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(4096 + 8)
    good = dict(stream=None, x=ok, n=64, seg=ok, nseg=1, mode=ML.STATS_ALWAYS, guard=None, scratch=ok, record=ok)

    def call(**change):
        return L.mmt_tensor_stats(*{**good, **change}.values())  # the dict keeps the argument order

    for bad in (dict(x=None), dict(seg=None), dict(scratch=None), dict(record=None), dict(nseg=-1), dict(n=-1),
                dict(x=odd), dict(scratch=odd), dict(record=odd), dict(guard=odd), dict(mode=ML.STATS_ON_SKIP),
                dict(mode=2)):
        assert call(**bad) == -1, bad  # MMT_ERR_INVALID


# ------------------------------------------------------------------------------------------------ segments
def test_build_segments_names_the_gaps():
    bounds, named = mmt_stats.build_segments(["a", "b", "c", "d"], [4, 10, 16, 16], [10, 13, 16, 20])
    assert bounds == [4, 10, 13, 16, 16, 20]  # a, b, the gap 13..16, c (empty), d
    assert named == [0, 1, 3, 4]
    assert mmt_stats.build_segments([], [], []) == ([0], [])
    assert mmt_stats.build_segments(["x"], [0], [5]) == ([0, 5], [0])


@pytest.mark.parametrize("begins,ends", [([0, 8], [9, 12]),      # overlap
                                          ([8, 0], [12, 4]),      # unsorted
                                          ([0, 4], [4, 3]),       # end < begin
                                          ([-1], [3])])
def test_build_segments_rejects_overlapping_or_unsorted(begins, ends):
    with pytest.raises(ValueError):
        mmt_stats.build_segments([f"t{i}" for i in range(len(begins))], begins, ends)


# ------------------------------------------------------------------------------------------------ report
def _record(stats, applied, skipped, valid=1):
    hdr = ML.MmtStatsHeader(valid, len(stats), applied, skipped, 0)
    return bytes(hdr) + b"".join(bytes(ML.MmtTensorStat(*s, 0.0)) for s in stats)


def _hand_made():
    """Five table segments: post.w, a gap, l1.w, l0.w, emb.w; stages post [0, 10), layer 1 [10, 20),
    layer 0 [20, 30), embeddings [30, 40) in backward order."""
    stats = [(9.0, 0, 0, -1, 2.0),        # post.w      [0, 6)
             (0.0, 7, 0, 0, 0.0),         # the gap     [6, 10): its NaNs must not show anywhere
             (16.0, 0, 0, -1, 4.0),       # l1.w        [10, 18)
             (1.0, 2, 1, 5, 1.0),         # l0.w        [20, 28)   (table: the gap 18..20 is folded for brevity)
             (4.0, 0, 1, 3, 2.0)]         # emb.w       [30, 36)
    names, named, begins = ["post.w", "l1.w", "l0.w", "emb.w"], [0, 2, 3, 4], [0, 10, 20, 30]
    stages = [(0, 10), (10, 20), (20, 30), (30, 40)]
    return stats, names, named, begins, stages


def test_report_from_record_and_rollups():
    stats, names, named, begins, stages = _hand_made()
    assert mmt_stats.StatsReport.from_record(_record(stats, 5, 1, valid=0), names, named, begins, stages) is None
    r = mmt_stats.StatsReport.from_record(_record(stats, 5, 1), names, named, begins, stages)
    assert r.names == names and (r.applied_steps, r.skipped_steps) == (5, 1)
    assert r.sqsum.tolist() == [9.0, 16.0, 1.0, 4.0] and r.absmax.tolist() == [2.0, 4.0, 1.0, 2.0]
    assert r.nan_count.tolist() == [0, 0, 2, 0] and r.inf_count.tolist() == [0, 0, 1, 1]
    assert r.first_bad.tolist() == [-1, -1, 5, 3]
    assert r.norm("l1.w") == 4.0 and r.norm("post.w") == 3.0
    assert math.isnan(r.global_norm)
    assert r.nonfinite() == [("l0.w", 2, 1, 5), ("emb.w", 0, 1, 3)]
    st = r.by_stage()
    assert [s["tensors"] for s in st] == [1, 1, 1, 1] and [s["nonfinite"] for s in st] == [0, 0, 1, 1]
    assert [s["norm"] for s in st] == [3.0, 4.0, 1.0, 2.0]
    assert r.first_poisoned_stage == 2  # layer 0 runs before the embeddings in the backward
    line = r.format()
    assert "applied 5 skipped 1" in line and "non-finite tensors: 2/4" in line and "first poisoned stage: 2/4" in line
    assert "l0.w (nan 2, inf 1, first at 5)" in line and "emb.w (nan 0, inf 1, first at 3)" in line
    assert "\n" not in line
    assert r.format(max_names=1).count("first at") == 1 and "+1 more" in r.format(max_names=1)


def test_report_of_a_healthy_record():
    stats, names, named, begins, stages = _hand_made()
    stats = [(s[0], 0, 0, -1, s[4]) for s in stats]
    r = mmt_stats.StatsReport.from_record(_record(stats, 3, 0), names, named, begins, stages)
    assert r.nonfinite() == [] and r.first_poisoned_stage is None
    assert r.global_norm == math.sqrt(9.0 + 16.0 + 1.0 + 4.0)
    assert r.largest(3) == [("l1.w", 4.0), ("post.w", 3.0), ("emb.w", 2.0)]
    line = r.format()
    assert f"norm: {r.global_norm:.4f}" in line and "largest: l1.w 4, post.w 3, emb.w 2" in line
    bare = mmt_stats.StatsReport(names, r.sqsum, r.absmax, r.nan_count, r.inf_count, r.first_bad)
    with pytest.raises(ValueError):
        bare.by_stage()
    assert "norm:" in bare.format()


# ------------------------------------------------------------------------------------------------ optimizer
def _fake_stats(mode):
    return types.SimpleNamespace(mode=mode, record=lambda *a, **k: None, model=None)


def test_adamw_stats_argument():
    p = [torch.nn.Parameter(torch.zeros(4))]
    assert mmt_optim.AdamW(p).stats is None
    with pytest.raises(ValueError, match="skipped"):
        mmt_optim.AdamW(p, stats=_fake_stats("skipped"))  # unguarded: nothing ever skips
    assert mmt_optim.AdamW(p, stats=_fake_stats("every")).stats.mode == "every"
    assert mmt_optim.AdamW(p, skip_nonfinite=True, stats=_fake_stats("skipped")).guarded
    assert mmt_optim.AdamW(p, max_grad_norm=1.0, stats=_fake_stats("every")).guarded
    for bad in ("every", 3, types.SimpleNamespace(mode="sometimes", record=print), types.SimpleNamespace(mode="every")):
        with pytest.raises(TypeError, match="stats"):
            mmt_optim.AdamW(p, stats=bad)


def test_tensor_stats_mode_is_validated():
    class M:
        flat_params = torch.zeros(4)
    assert mmt_stats.TensorStats(M(), "every").read() is None  # no device: nothing allocated, nothing recorded
    with pytest.raises(ValueError, match="mode"):
        mmt_stats.TensorStats(M(), "always")
