"""bench.py's `--full` / `--dump-outputs` plumbing that needs no device: the options exist and
default to a plain run, and dump_outputs writes the result a step returned as float32 / float64
.npy files at a fixed column sample within its size bound.  CPU only."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Result:
    def __init__(self, K, m, n, B, with_t=True, with_loss=True):
        g = torch.Generator().manual_seed(5)
        self.Z = torch.randn(K, n, B, generator=g)
        self.E = torch.randn(K, m, B, generator=g)
        self.L = torch.randn(K, m, B, generator=g)
        self.T = torch.randn(K + 1, m, B, generator=g) if with_t else None
        self.loss_sums = torch.rand(K, 2, generator=g, dtype=torch.float64) if with_loss else None


def test_plain_run_is_default(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_sample(tmp_path):
    b = _bench()
    K, m, n, B = 3, 4, 8, 1000
    r = _Result(K, m, n, B)
    obj = torch.arange(K, dtype=torch.float64)
    b.dump_outputs(str(tmp_path / "a"), r, obj, 0)
    b.dump_outputs(str(tmp_path / "b"), r, obj, 0)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["E.npy", "L.npy", "T.npy", "Z.npy", "loss_sums.npy", "objective.npy"]
    cols = np.sort(np.random.default_rng(1126).choice(B, b.DUMP_COLS, replace=False))
    for nm in names:
        x = np.load(tmp_path / "a" / nm)
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, np.load(tmp_path / "b" / nm))   # the same sample every time
    for nm in ("Z", "E", "L", "T"):
        x = np.load(tmp_path / "a" / f"{nm}.npy")
        assert x.dtype == np.float32
        assert np.array_equal(x, getattr(r, nm).numpy()[:, :, cols])
    assert np.array_equal(np.load(tmp_path / "a" / "loss_sums.npy"), r.loss_sums.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "objective.npy"), obj.numpy())


def test_dump_outputs_small_batch_rank_and_bound(tmp_path, monkeypatch):
    b = _bench()
    # a batch below the sample size is written whole; no T / objective for the variants without
    r = _Result(2, 3, 5, 7, with_t=False, with_loss=False)
    b.dump_outputs(str(tmp_path), r, torch.zeros(1, dtype=torch.float64), 2)
    assert sorted(os.listdir(tmp_path)) == ["E.rank2.npy", "L.rank2.npy", "Z.rank2.npy"]
    assert np.array_equal(np.load(tmp_path / "Z.rank2.npy"), r.Z.numpy())
    # the byte bound caps the sample: 4 * (3*8 + 2*3*4 + 4*4) = 256 B per column
    monkeypatch.setattr(b, "DUMP_BYTES", 256 * 10 + 100)
    r = _Result(3, 4, 8, 1000)
    out = tmp_path / "capped"
    b.dump_outputs(str(out), r, torch.zeros(3, dtype=torch.float64), 0)
    assert np.load(out / "Z.npy").shape == (3, 8, 10)
    assert sum(np.load(out / f"{nm}.npy").nbytes for nm in "ZELT") <= b.DUMP_BYTES
