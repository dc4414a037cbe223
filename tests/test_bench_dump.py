"""bench.py --dump-outputs on the CPU: dump_outputs writes the buffer of the
last timed step (the two output buffers rotate), whole when it is small and
as the same seeded sample on every call when it is large; the argument parser
knows --full and --dump-outputs."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _wl(rows):
    a = torch.arange(rows + 3, dtype=torch.int32)  # (buffers may be longer than the column)
    return SimpleNamespace(rows=rows, outs=[(a, None), (-a, None)])


def test_dump_whole_column_of_last_step(tmp_path):
    assert bench.DUMP_ROWS * 8 <= 64 << 20  # the largest dump, in bytes
    wl = _wl(1000)
    for steps, sign in ((4, -1), (5, 1)):  # step k decodes into buffer k & 1
        info = bench.dump_outputs(torch, wl, steps, str(tmp_path), 1, 0)
        got = np.load(tmp_path / "values.npy")
        assert got.dtype == np.float64 and info["rows"] == 1000 and not info["sampled"]
        assert np.array_equal(got, sign * np.arange(1000, dtype=np.float64))


def test_dump_sample_is_fixed_and_stratified(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 64)
    wl = _wl(1001)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(torch, wl, 1, str(a), 1, 0)
    bench.dump_outputs(torch, wl, 1, str(b), 1, 0)
    got = np.load(a / "values.npy")
    assert info["sampled"] and got.shape == (64,)
    assert np.array_equal(got, np.load(b / "values.npy"))
    edges = np.arange(65) * 1001 // 64  # the values are the row numbers: one row of every stratum
    assert ((got >= edges[:-1]) & (got < edges[1:])).all()


def test_dump_names_ranks(tmp_path):
    info = bench.dump_outputs(torch, _wl(10), 1, str(tmp_path), 2, 1)
    assert info["file"] == "values_rank1.npy" and (tmp_path / "values_rank1.npy").exists()


def test_cli_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
