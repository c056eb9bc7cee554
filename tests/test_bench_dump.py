"""bench.py --dump-outputs on CPU tensors: what bench.dump_outputs writes (whole maps, or one fixed seeded pixel sample shared by
every map and rank), the 64 MB bound at the default sample size, and --steps below 1 refused before anything runs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _maps(h, w, ranks, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"depth": [torch.rand((h, w), generator=g) for _ in range(ranks)],
            "normal": [torch.rand((h, w, 3), generator=g) for _ in range(ranks)],
            "cost": [torch.rand((h, w), generator=g) for _ in range(ranks)]}


def test_small_maps_are_written_whole(tmp_path):
    maps = _maps(12, 20, 1)
    bench.dump_outputs(str(tmp_path), maps, 12, 20)
    assert sorted(os.listdir(tmp_path)) == ["cost.npy", "depth.npy", "normal.npy"]
    for name, (t,) in maps.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.numpy())


def test_several_ranks_are_stacked(tmp_path):
    maps = _maps(8, 10, 3)
    bench.dump_outputs(str(tmp_path), maps, 8, 10)
    a = np.load(tmp_path / "normal.npy")
    assert a.shape == (3, 8, 10, 3)
    assert all(np.array_equal(a[r], maps["normal"][r].numpy()) for r in range(3))


def test_large_maps_are_one_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 1000)
    h, w, ranks = 48, 64, 2
    maps = _maps(h, w, ranks)
    n = 1000 // ranks
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(h * w, size=n, replace=False))   # the recipe the docstring states
    bench.dump_outputs(str(tmp_path / "a"), maps, h, w)
    bench.dump_outputs(str(tmp_path / "b"), _maps(h, w, ranks), h, w)        # a second run on equal inputs
    for name, per_rank in maps.items():
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (ranks, n) + tuple(per_rank[0].shape[2:])
        for r, t in enumerate(per_rank):
            assert np.array_equal(a[r], t.numpy().reshape(h * w, *t.shape[2:])[idx])
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))


def test_default_sample_stays_under_64_mb():
    per_pixel = (1 + 3 + 1) * 4                       # depth + normal + cost, float32
    assert bench.DUMP_MAX_PIXELS * per_pixel + 3 * 1024 <= 64 * 10 ** 6
    assert 6048 * 4032 > bench.DUMP_MAX_PIXELS       # the default workload is the sampled case


def test_steps_below_one_are_refused(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
