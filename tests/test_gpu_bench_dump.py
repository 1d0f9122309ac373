"""bench.py's plain run (no --full) and its --dump-outputs files: the headline fields only, the legs left out, and the sampled
rows of the last timed step equal to the oracle's paths and embeddings at those rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gnnpe_amd import synth

pytestmark = pytest.mark.gpu


def test_plain_bench_dumps_the_oracle_rows(tmp_path, oracle):
    n, m, labels = 20000, 100000, 16
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--vertices", str(n), "--edges", str(m), "--labels", str(labels), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "paths/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u32 ids + f64 embeddings" and d["value"] > 0
    assert not {"index_build", "online_filter", "config2", "gnn_pge", "config5", "e2e"} & set(d) and d["cpu_baseline"] is None
    assert d["phases_ms"]["per_step"] == {}

    g = synth.gnm_graph(n, m, n_labels=labels)
    sn = synth.degree_order(g["offsets"])
    paths = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    x, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], 2)
    pde, _, _, _ = oracle.gen_pde(paths, 2, g["offsets"], g["labels"], x, vde)
    total = len(paths)
    assert d["config"]["paths"] == total
    files = {f: np.load(out / f"{f}.npy") for f in ("ids", "pde", "rows", "paths")}
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(os.path.getsize(out / f"{f}.npy") for f in files) < 64 << 20
    assert files["paths"].tolist() == [total, total]
    rows = files["rows"].astype(np.int64)
    assert len(rows) == min(total, 1 << 18) and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < total
    assert np.array_equal(files["ids"], paths[rows].astype(np.float64))
    assert np.array_equal(files["pde"].view(np.uint64), pde[rows].view(np.uint64))
