"""bench.py's run modes on the CPU: a plain run keeps only the headline measurement (`--full`
brings the comparisons back, each still behind its own --no-... switch), and --dump-outputs
writes float32 arrays within its size limit, the same row sample every time."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_rocsparse and a.no_cpu and a.no_north_star


def test_full_run_keeps_the_single_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_rocsparse or a.no_cpu or a.no_north_star)
    a = _parse(monkeypatch, "--full", "--no-cpu", "--dump-outputs", "d")
    assert a.no_cpu and not a.no_rocsparse and a.dump_outputs == "d"


def test_dump_outputs_whole_arrays(tmp_path):
    c = torch.arange(12, dtype=torch.float16).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "o"), {"C": c})
    got = np.load(tmp_path / "o" / "C.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, c.float().numpy())
    bench.dump_outputs(str(tmp_path / "o"), {"C": c}, rank=1, world=2)
    assert os.path.exists(tmp_path / "o" / "rank1_C.npy")


def test_dump_outputs_samples_rows_past_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    a = torch.arange(300 * 4, dtype=torch.float32).reshape(300, 4)
    b = torch.arange(100 * 4, dtype=torch.float32).reshape(100, 4).neg()
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"A": a, "B": b})
    ga, gb = np.load(tmp_path / "x" / "A.npy"), np.load(tmp_path / "x" / "B.npy")
    assert ga.nbytes + gb.nbytes <= 4000 and ga.shape[0] > gb.shape[0] > 0
    rows = (ga[:, 0] / 4).astype(int)
    assert np.all(np.diff(rows) > 0)                      # distinct rows, in order
    np.testing.assert_array_equal(ga, a.numpy()[rows])    # whole rows of the array
    np.testing.assert_array_equal(ga, np.load(tmp_path / "y" / "A.npy"))  # the same sample again
    np.testing.assert_array_equal(gb, np.load(tmp_path / "y" / "B.npy"))
