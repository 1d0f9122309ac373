"""bench.py's --dump-outputs writer on the host: a stand-in output pool in host memory, the device calls replaced by no-ops.
The sample must be the same rows for the same path count, hold the pool's values at those rows, and stay under 64 MB for all
ranks' files together."""
import os
import sys
import types

import numpy as np
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

HOST_TORCH = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda: None), from_numpy=torch.from_numpy,
                                   int64=torch.int64, float64=torch.float64)


class HostPool:
    """What dump_outputs reads of binding.OutputPool: L, D and torch views of the ids (int32) and pde (float64) rows."""

    def __init__(self, rows, L, D, seed):
        g = torch.Generator().manual_seed(seed)
        self.L, self.D = L, D
        self.ids = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, L), dtype=torch.int32, generator=g)
        self.pde = torch.randn(rows, D, dtype=torch.float64, generator=g)

    def ids_tensor(self, device):
        return self.ids

    def pde_tensor(self, device):
        return self.pde


def _dump(tmp, pool, total, suffix="", ranks=1):
    bench.dump_outputs(str(tmp), HOST_TORCH, "cpu", pool, total, total * ranks, suffix, ranks)
    return {k: np.load(os.path.join(tmp, f"{k}{suffix}.npy")) for k in ("ids", "pde", "rows", "paths")}


def test_dump_is_a_fixed_sample_of_the_pool_rows(tmp_path):
    total = 3_000_000
    a = _dump(tmp_path / "a", HostPool(total, 3, 6, 1), total)
    b = _dump(tmp_path / "b", HostPool(total, 3, 6, 2), total)
    rows = a["rows"].astype(np.int64)
    assert all(x.dtype == np.float64 for x in a.values())
    assert len(rows) == 1 << 18 and np.array_equal(a["rows"], b["rows"]) and np.all(np.diff(rows) > 0) and rows[-1] < total
    pool = HostPool(total, 3, 6, 1)
    assert np.array_equal(a["ids"], pool.ids.numpy()[rows].view(np.uint32).astype(np.float64))
    assert np.array_equal(a["pde"], pool.pde.numpy()[rows]) and a["paths"].tolist() == [total, total]
    small = _dump(tmp_path / "c", HostPool(1000, 3, 6, 3), 1000)
    assert np.array_equal(small["rows"], np.arange(1000.0))


def test_dump_of_all_ranks_stays_under_64_mb(tmp_path):
    for ranks, L, D in ((1, 4, 32), (4, 3, 6), (8, 4, 32)):
        d = tmp_path / f"r{ranks}"
        for r in range(ranks):
            _dump(d, HostPool(1 << 20, L, D, r), 1 << 20, f"_rank{r}", ranks)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) < 64 << 20, (ranks, L, D)
