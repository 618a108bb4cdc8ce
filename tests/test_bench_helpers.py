"""CPU: the pieces of bench.py that turn the committed rocprofv3 summaries (profiles/) into the roofline fields of the
JSON line -- they must keep reading the files the profile scripts write."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_profile_summaries_feed_the_roofline_fields():
    b = _bench()
    traffic, src = b.pmc_traffic("unwrap_median_gray_kernel", 256)
    assert src and src.startswith("profiles/") and 4e8 < traffic < 1.5e9          # ~700 MB per launch of 256 pairs
    t2, _ = b.pmc_traffic("unwrap_median_gray_kernel", 128)
    assert abs(t2 * 2 - traffic) < 1e-6 * traffic                                 # scales with the pairs per launch
    assert b.pmc_traffic("no_such_kernel", 256) == (None, None)
    vi = b.valu_issue("unwrap_median_gray_kernel", 256, 2.42e-3)       # round-2 launch time
    assert vi["mix_source"] and 3.0 < vi["issue_cycles_per_inst"] < 4.4 and 0.8 < vi["frac"] < 1.05
    step = b.valu_issue_step(768, 14.1)
    assert 0.55 < step["dominant_kernel_share"] < 0.75 and 0.7 < step["frac"] < 1.05
    assert 0.4 < step["frac_vs_guide_2cyc"] < step["frac"] and step["per_kernel"] and step["mix_source"]   # priced per kernel
    meta = b.profile_meta(os.path.join(ROOT, step["source"]), {"detector": "GFT"})
    assert "stale" in meta
    assert b.b_alg_c2(480, 640, 2000) == 1943296                                   # algorithmic bytes per pair
    assert b.host_cores() >= 1


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    """--dump-outputs: float64 .npy per array, float32 kept; over the budget every array keeps the same seeded rows."""
    import numpy as np
    b = _bench()
    rec = np.arange(64 * 16, dtype=np.float64).reshape(64, 16)
    kept = b.write_outputs(str(tmp_path / "a"), {"records": rec, "counts": np.arange(64, dtype=np.int32),
                                                  "resp": np.ones((64, 3), np.float32)})
    assert kept == {"records": 64, "counts": 64, "resp": 64}
    got = np.load(str(tmp_path / "a" / "records.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, rec)
    assert np.load(str(tmp_path / "a" / "counts.npy")).dtype == np.float64
    assert np.load(str(tmp_path / "a" / "resp.npy")).dtype == np.float32
    budget = rec.nbytes // 4
    for d in ("b", "c"):
        kept = b.write_outputs(str(tmp_path / d), {"records": rec}, budget_bytes=budget)
        assert kept == {"records": 16}
    s1, s2 = np.load(str(tmp_path / "b" / "records.npy")), np.load(str(tmp_path / "c" / "records.npy"))
    assert s1.nbytes <= budget and np.array_equal(s1, s2)                          # fixed sample, run to run
    rows = s1[:, 0] / 16
    assert np.all(np.diff(rows) > 0) and np.array_equal(s1, rec[rows.astype(int)])   # whole rows, in order
    assert b.OUTPUT_BUDGET == 64 << 20


def test_steps_and_dump_outputs_arguments(monkeypatch):
    import sys
    import pytest
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    args = b.parse()
    assert (args.steps, args.warmup, args.dump_outputs) == (7, 2, "out")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        b.parse()


def test_plain_run_leaves_everything_beyond_the_headline_to_full(monkeypatch):
    """Without --full a run skips the CPU baselines, the PCIe leg, the isolated launches and the sub-records; with --full
    it runs them, and the --no-* options still leave single parts out."""
    import sys
    b = _bench()
    gated = ("no_cpu", "no_h2d", "no_isolated", "no_sub")
    for argv, expect in ((["--gpus", "1", "--steps", "7", "--warmup", "2"], (True, True, True, True)),
                         (["--full"], (False, False, False, False)),
                         (["--full", "--no-sub", "--no-h2d"], (False, True, False, True))):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        args = b.parse()
        assert tuple(getattr(args, k) for k in gated) == expect, argv
        assert args.full == ("--full" in argv)
