"""bench.py's options and its output dump, without a GPU: `--full` / `--dump-outputs` are declared, and dump_outputs() writes float64
arrays, all games of a batch that fits its budget and a fixed sample of one that does not."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from algames_jl_amd._abi import game_stats_dtype  # noqa: E402


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


class _FakeBatch:
    """What dump_outputs() reads from an alg Batch: the trajectory and the constraint duals of every game."""

    def __init__(self, G, L, C):
        g = np.arange(G, dtype=np.float64)[:, None]
        self.z = g + np.arange(L) / L
        self.lam, self.mu = g + np.arange(C) / C, -g - np.arange(C) / C

    def get_traj(self):
        return self.z.copy()

    def get_con_duals(self):
        return self.lam.copy(), self.mu.copy()


def _stats(G):
    st = np.zeros(G, dtype=game_stats_dtype)
    st["newton_iters"] = np.arange(G) % 7 + 3
    st["converged"] = 1
    st["last"]["res"] = np.linspace(1e-12, 1e-9, G)
    st["last"]["t_elap"] = 123.0
    return st


def test_dump_writes_every_game_of_a_small_batch(tmp_path):
    G, ids = 16, np.arange(100, 116)
    info = bench.dump_outputs(str(tmp_path), _FakeBatch(G, 30, 5), ids, _stats(G), (np.full(G, 9), np.ones(G)))
    assert info["games"] == G
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 and a.shape[0] == G for a in files.values())
    assert np.array_equal(files["game_ids"], ids) and files["pdtraj"].shape == (G, 30) and files["con_mu"].shape == (G, 5)
    assert np.array_equal(files["stats_newton_iters"], np.arange(G) % 7 + 3) and np.array_equal(files["mpc_newton_iters"], np.full(G, 9.0))
    assert "last_t_elap" not in files                                    # wall time is not an output of the computation


def test_dump_samples_a_large_batch_within_the_budget_and_the_same_rows_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    G = 4096
    fb, st = _FakeBatch(G, 40, 6), _stats(G)
    a = bench.dump_outputs(str(tmp_path / "a"), fb, np.arange(G), st)
    b = bench.dump_outputs(str(tmp_path / "b"), fb, np.arange(G), st)
    assert 0 < a["games"] < G and a == {**b, "dir": a["dir"]} and a["bytes"] <= 200_000
    ids = np.load(tmp_path / "a" / "game_ids.npy")
    assert np.array_equal(ids, np.load(tmp_path / "b" / "game_ids.npy")) and np.all(np.diff(ids) > 0)
    z = np.load(tmp_path / "a" / "pdtraj.npy")
    assert np.array_equal(z, fb.z[ids.astype(int)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 200_000 + 128 * len(os.listdir(tmp_path / "a"))


def test_dump_budget_stays_below_64_mb():
    assert bench.DUMP_BYTES + 128 * 64 <= 64_000_000
