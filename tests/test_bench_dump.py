"""CPU tier: bench.py's --full / --dump-outputs options and its output writer (bench.dump_outputs).

The writer must store float32 .npy files, keep the whole set under its byte budget by keeping a seeded sample of the rows
of the large arrays (the same rows on every run), and leave small outputs whole."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_whole_when_small(tmp_path):
    lp = np.random.default_rng(1).standard_normal((64, 10))
    bench.dump_outputs(str(tmp_path / "d"), {"log_probs": lp, "kl": np.float64(2.5)})
    got = np.load(tmp_path / "d" / "log_probs.npy")
    assert got.dtype == np.float32 and np.array_equal(got, lp.astype(np.float32))
    kl = np.load(tmp_path / "d" / "kl.npy")
    assert kl.dtype == np.float32 and kl.shape == () and float(kl) == 2.5


def test_dump_outputs_samples_the_same_rows_under_the_budget(tmp_path):
    lp = np.arange(5000 * 10, dtype=np.float32).reshape(5000, 10)
    budget = 40000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"log_probs": lp, "kl": np.float32(1.0)}, max_bytes=budget)
    a, b = np.load(tmp_path / "a" / "log_probs.npy"), np.load(tmp_path / "b" / "log_probs.npy")
    assert np.array_equal(a, b) and a.dtype == np.float32
    assert a.nbytes + 4 <= budget and a.shape[0] >= 900
    rows = a[:, 0].astype(np.int64) // 10
    assert (np.diff(rows) > 0).all() and np.array_equal(a, lp[rows])          # whole rows of the output, in order
