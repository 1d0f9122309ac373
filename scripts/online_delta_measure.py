#!/usr/bin/env python3
"""What the matches through a set of data edges cost ("Matches through a set of data edges"):
gnnpe_refine_sets_delta for F of 1, 100 and 10 000 random edges and for F = E(G), beside gnnpe_refine_sets_mode, count only, for
the same query on the same graph and bitmap.

Graph: powerlaw_graph(n, m, max_degree=600) of section 3.7 (default 20 000 / 80 000) with every label 0 -- the motif setting and
the graph of profiles/online_edge_counts.txt.  Queries: wedge, triangle, C4, diamond, K4 and C5, mode 0, limit 2^64 - 1, no rows.
Per query one JSON line: the count and its device ms, then per F its size, Delta, the device ms and the launches (one per query
edge); every ms is the best of the warm runs, with their spread (--rounds runs, the first dropped; the calls alternate in one
process).  For F = E(G), where Delta must equal the count (asserted), the ratio to the plain call: what the nqe launches and the
key searches cost.  The random edges are drawn with seed 1 and the smaller F are prefixes of the larger.
Every query runs in a child process under a time limit of its own (--time-limit seconds); a child that passes it is ended, a
"timed_out" row follows and nothing is run again.
Usage: python scripts/online_delta_measure.py [--n 20000] [--m 80000] [--rounds 4] [--time-limit 300] [--queries wedge,triangle,...]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = (1 << 64) - 1
SHAPES = {
    "wedge": (3, ((0, 1), (1, 2))),
    "triangle": (3, ((0, 1), (0, 2), (1, 2))),
    "C4": (4, ((0, 1), (1, 2), (2, 3), (0, 3))),
    "diamond": (4, ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3))),
    "K4": (4, tuple((a, b) for a in range(4) for b in range(a + 1, 4))),
    "C5": (5, ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4))),
}
SIZES = (1, 100, 10000)


def write_query(path, n, edges, labels):
    deg = [0] * n
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
    with open(path, "w") as f:
        f.write(f"t {n} {len(edges)}\n")
        for v in range(n):
            f.write(f"v {v} {labels[v]} {deg[v]}\n")
        for a, b in sorted(edges):
            f.write(f"e {a} {b}\n")


def ld_bitmap(g, q):
    """bit v of row u: label(v) = label(u) and degree(v) >= degree(u)"""
    n = g["n"]
    deg = np.diff(g["offsets"].astype(np.int64))
    qd = np.diff(q["offsets"].astype(np.int64))
    bm = np.zeros((q["n"], (n + 31) // 32), np.uint32)
    for u in range(q["n"]):
        ids = np.nonzero((g["labels"] == q["labels"][u]) & (deg >= qd[u]))[0]
        np.bitwise_or.at(bm[u], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return bm


def child(name, a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    g = synth.powerlaw_graph(a.n, a.m, max_degree=600)
    g = dict(g, labels=np.zeros(g["n"], np.uint32))
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(synth.degree_order(g["offsets"]), np.zeros(g["n"], np.uint32), 1)
    eng.set_label_table(binding.host_label_table(1, 2))
    eng.vde(want=False)
    nq, edges = SHAPES[name]
    qp = os.path.join(a.out, f"{name}.graph")
    write_query(qp, nq, edges, [0] * nq)
    bm = ld_bitmap(g, binding.host_load_graph(qp))
    src = np.repeat(np.arange(g["n"], dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    E = np.stack([src, g["nbrs"].astype(np.int64)], axis=1)
    E = E[E[:, 0] < E[:, 1]]
    shuffled = E[np.random.default_rng(1).permutation(len(E))]
    sets = [(str(k), shuffled[:k]) for k in SIZES if k < len(E)] + [("all", E)]
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, edges=len(E), launches=len(edges))
    count_runs, delta_runs = [], {key: [] for key, _ in sets}
    for _ in range(a.rounds):  # alternately: count only, then every F
        count_runs.append(eng.refine_sets(qp, bm, limit=FULL)[:2])
        for key, F in sets:
            ans, _, ms = eng.refine_sets_delta(qp, bm, F)
            delta_runs[key].append((ans, ms))
    assert len({r[0] for r in count_runs}) == 1
    row["answers"] = count_runs[0][0]
    ms = [r[1] for r in count_runs[1:]]
    row.update(count_ms=round(min(ms), 3), count_spread_ms=round(max(ms) - min(ms), 3), count_first_ms=round(count_runs[0][1], 3))
    for key, F in sets:
        runs = delta_runs[key]
        assert len({r[0] for r in runs}) == 1, (key, runs)
        ms = [r[1] for r in runs[1:]]
        row[f"F_{key}"] = dict(size=len(F), delta=runs[0][0], ms=round(min(ms), 3), spread_ms=round(max(ms) - min(ms), 3),
                               first_ms=round(runs[0][1], 3), over_count=round(min(ms) / max(row["count_ms"], 1e-6), 3))
    assert row["F_all"]["delta"] == row["answers"], (row["F_all"], row["answers"])
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--queries", default="wedge,triangle,C4,diamond,K4,C5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_delta"))
    ap.add_argument("--time-limit", type=float, default=300.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for name in (k for k in a.queries.split(",") if k):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--n", str(a.n), "--m", str(a.m), "--rounds", str(a.rounds),
               "--out", a.out]
        p = subprocess.Popen(cmd)  # a fresh process per query: its row goes straight to this stdout
        try:
            rc = p.wait(timeout=a.time_limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            print(json.dumps(dict(query=name, timed_out=True, time_limit_s=a.time_limit)), flush=True)
            return 1  # nothing more is started after a run that had to be ended
        if rc != 0:
            print(json.dumps(dict(query=name, failed=True, returncode=rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
