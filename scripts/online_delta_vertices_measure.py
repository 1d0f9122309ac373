#!/usr/bin/env python3
"""What the matches through a set of data vertices and a vertex relabel cost ("Matches through a set of
data vertices"; profiles/online_delta_vertices.txt).

1. gnnpe_refine_sets_delta_vertices beside its emulation by existing code, gnnpe_refine_sets_delta over E(S) (every edge with an
   endpoint in S), count only, for the same query on the same graph and bitmap.
   Graph: powerlaw_graph(n, m, max_degree=600) of section 3.7 (default 20 000 / 80 000) with every label 0, the graph of
   profiles/online_delta.txt.  Queries: wedge, triangle, C4, diamond, K4, mode 0, limit 2^64 - 1, no rows.  S: the first 1, 100 and
   10 000 vertices of a shuffle with seed 1, and the vertex with the longest row alone ("hub").
   Per query one JSON line: per S its size, |E(S)|, DeltaV, then the device ms of the vertex form (nq launches) and of the
   emulation (nqe launches) -- the best of the warm runs with their spread (--rounds runs, the first dropped; the two calls
   alternate in one process) -- and their ratio.  The two answers must be equal (asserted).
2. gnnpe_set_vertex_labels of 100 and 10 000 vertices, device ms, beside gnnpe_load_csr of the whole graph with the new labels,
   wall-clock, on gnm_graph(1 000 000, 10 000 000) (the graph of profiles/online_entry_map.txt): one JSON line ("relabel").

Every query and the relabel part run in a child process of their own under a time limit of their own (--time-limit seconds); a
child that passes it is ended, a "timed_out" row follows and nothing is run again: the chain stops at the first failure.
Usage: python scripts/online_delta_vertices_measure.py [--n 20000] [--m 80000] [--rounds 4] [--time-limit 300]
       [--queries wedge,triangle,...] [--relabel-n 1000000] [--relabel-m 10000000] [--no-relabel]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from online_delta_measure import FULL, SHAPES, ld_bitmap, write_query  # noqa: E402

SIZES = (1, 100, 10000)
RELABEL_SIZES = (100, 10000)


def child(name, a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    g = synth.powerlaw_graph(a.n, a.m, max_degree=600)
    g = dict(g, labels=np.zeros(g["n"], np.uint32))
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    nq, edges = SHAPES[name]
    qp = os.path.join(a.out, f"{name}.graph")
    write_query(qp, nq, edges, [0] * nq)
    bm = ld_bitmap(g, binding.host_load_graph(qp))
    deg = np.diff(g["offsets"].astype(np.int64))
    src = np.repeat(np.arange(g["n"], dtype=np.int64), deg)
    E = np.stack([src, g["nbrs"].astype(np.int64)], axis=1)
    E = E[E[:, 0] < E[:, 1]]
    shuffled = np.random.default_rng(1).permutation(g["n"])
    sets = [(str(k), shuffled[:k]) for k in SIZES if k <= g["n"]] + [("hub", np.array([int(np.argmax(deg))]))]
    at = {key: E[np.isin(E[:, 0], S) | np.isin(E[:, 1], S)] for key, S in sets}
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, nq=nq, nqe=len(edges), max_degree=int(deg.max()))
    v_runs, e_runs = {key: [] for key, _ in sets}, {key: [] for key, _ in sets}
    for _ in range(a.rounds):  # alternately: the vertex form, then the emulation, for every S
        for key, S in sets:
            ans, _, ms = eng.refine_sets_delta_vertices(qp, bm, S)
            v_runs[key].append((ans, ms))
            ans, _, ms = eng.refine_sets_delta(qp, bm, at[key])
            e_runs[key].append((ans, ms))
    for key, S in sets:
        assert len({r[0] for r in v_runs[key] + e_runs[key]}) == 1, (key, v_runs[key], e_runs[key])
        v, e = [r[1] for r in v_runs[key][1:]], [r[1] for r in e_runs[key][1:]]
        row[f"S_{key}"] = dict(size=len(S), edges_at=len(at[key]), delta_v=v_runs[key][0][0], vertices_ms=round(min(v), 3),
                               vertices_spread_ms=round(max(v) - min(v), 3), emulation_ms=round(min(e), 3),
                               emulation_spread_ms=round(max(e) - min(e), 3), vertices_over_emulation=round(min(v) / max(min(e), 1e-6), 3))
    eng.close()
    print(json.dumps(row), flush=True)


def relabel_child(a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    g = synth.gnm_graph(a.relabel_n, a.relabel_m, n_labels=16, seed=1)
    labels = g["labels"].astype(np.uint32)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], labels)
    rng = np.random.default_rng(2)
    row = dict(relabel=True, graph=f"gnm_{a.relabel_n}_{a.relabel_m}", entries=int(g["offsets"][-1]))
    for k in RELABEL_SIZES:
        dev, wall, load = [], [], []
        for _ in range(a.rounds):
            S = rng.choice(g["n"], k, replace=False)
            new = ((labels[S] + 1 + rng.integers(0, 15, k)) % 16).astype(np.uint32)
            t0 = time.perf_counter()
            dev.append(eng.set_vertex_labels(S, new, timing=True))
            wall.append((time.perf_counter() - t0) * 1e3)
            labels[S] = new
            assert np.array_equal(eng.download_labels(), labels)
            t0 = time.perf_counter()
            eng.load_csr(g["offsets"], g["nbrs"], labels)  # what the parent has: the whole graph again
            load.append((time.perf_counter() - t0) * 1e3)
        row[f"k_{k}"] = dict(set_labels_device_ms=round(min(dev[1:]), 4), set_labels_spread_ms=round(max(dev[1:]) - min(dev[1:]), 4),
                             set_labels_wall_ms=round(min(wall[1:]), 3), load_csr_wall_ms=round(min(load[1:]), 2),
                             load_csr_spread_ms=round(max(load[1:]) - min(load[1:]), 2))
    eng.close()
    print(json.dumps(row), flush=True)


def run_child(cmd, what, limit):
    p = subprocess.Popen(cmd)  # a fresh process per part: its row goes straight to this stdout
    try:
        rc = p.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        print(json.dumps(dict(query=what, timed_out=True, time_limit_s=limit)), flush=True)
        return 1  # nothing more is started after a run that had to be ended
    if rc != 0:
        print(json.dumps(dict(query=what, failed=True, returncode=rc)), flush=True)
        return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--queries", default="wedge,triangle,C4,diamond,K4")
    ap.add_argument("--relabel-n", type=int, default=1_000_000)
    ap.add_argument("--relabel-m", type=int, default=10_000_000)
    ap.add_argument("--no-relabel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_delta_vertices"))
    ap.add_argument("--time-limit", type=float, default=300.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child == "relabel":
        return relabel_child(a)
    if a.child:
        return child(a.child, a)
    common = ["--n", str(a.n), "--m", str(a.m), "--rounds", str(a.rounds), "--out", a.out, "--relabel-n", str(a.relabel_n), "--relabel-m",
              str(a.relabel_m)]
    for name in (k for k in a.queries.split(",") if k):
        if run_child([sys.executable, os.path.abspath(__file__), "--child", name] + common, name, a.time_limit):
            return 1
    if not a.no_relabel and run_child([sys.executable, os.path.abspath(__file__), "--child", "relabel"] + common, "relabel", a.time_limit):
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
