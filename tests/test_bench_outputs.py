"""CPU tests of bench.py's `--dump-outputs` writer and of its argument checks - no GPU."""

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_every_array_whole_in_float64(tmp_path):
    lnl = np.linspace(-3.0, 290.0, 1000)
    chi2 = np.arange(1000, dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), {"lnl": lnl, "chi2": chi2})
    got_l, got_c = np.load(tmp_path / "out" / "lnl.npy"), np.load(tmp_path / "out" / "chi2.npy")
    assert got_l.dtype == got_c.dtype == np.float64
    assert np.array_equal(got_l, lnl) and np.array_equal(got_c, chi2)


def test_dump_outputs_samples_the_same_rows_of_every_array_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1600)
    n = 10_000
    idx = np.arange(n, dtype=np.float64)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"lnl": idx, "chi2": 2 * idx})
    a_l, a_c = np.load(tmp_path / "a" / "lnl.npy"), np.load(tmp_path / "a" / "chi2.npy")
    assert a_l.nbytes + a_c.nbytes <= 1600 and len(a_l) == 100
    assert np.all(np.diff(a_l) > 0) and np.array_equal(a_c, 2 * a_l)            # sorted rows, the same rows in both arrays
    assert np.array_equal(a_l, np.load(tmp_path / "b" / "lnl.npy"))              # the sample is fixed: run to run identical


def test_bench_rejects_zero_steps():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 2 and "--steps" in res.stderr and res.stdout == ""


def test_bench_takes_full_and_documents_it():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "0"], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 2 and "--steps must be at least 1" in res.stderr and res.stdout == ""
    helped = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert helped.returncode == 0 and "--full" in helped.stdout
