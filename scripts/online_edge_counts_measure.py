#!/usr/bin/env python3
"""What the per-edge table costs ("Per-edge match counts"): gnnpe_refine_sets_mode, count only,
gnnpe_refine_sets_vertex_counts and gnnpe_refine_sets_edge_counts on the same label/degree bitmap, alternating in one process.

Graph: powerlaw_graph(n, m, max_degree=600) of section 3.7 (default 20 000 / 80 000) with every label 0 -- the motif setting.
Queries: wedge, triangle, C4, diamond, K4 and C5, mode 0, limit 2^64 - 1 (the whole search: the tables are exact only then).
Per query one JSON line: the count, the three device ms (best of three warm runs and the spread of the three; a table's ms covers
its zeroing), edge table / count and edge table / vertex table, and the atomics on the edge table per find -- deg_Q(last position)
leaf adds per find plus the adds of the flushes the kernel counts (GNNPE_DEBUG=1 makes the library print both; the child keeps its
own stderr in a file and reads the last such line).  The edge table is checked once on the host: every row sums to the count, its
marginals are the vertex table's rows, and the wedge's rows are their closed forms.
Every query runs in a child process under a time limit of its own (--time-limit seconds); a child that passes it is ended, a
"timed_out" row follows and nothing is run again.
Usage: python scripts/online_edge_counts_measure.py [--n 20000] [--m 80000] [--out DIR] [--time-limit 300]
       [--queries wedge,triangle,...]"""
import argparse
import json
import os
import re
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
    # the library's GNNPE_DEBUG lines go to this process's stderr: keep it in a file of the child's own
    err_path = os.path.join(a.out, f"{name}.stderr")
    err = open(err_path, "w")
    os.dup2(err.fileno(), 2)
    os.environ["GNNPE_DEBUG"] = "1"  # read when the context is created
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
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name)
    # alternately: count only, vertex table, edge table, count only, ...
    count_runs, vertex_runs, edge_runs = [], [], []
    for _ in range(4):
        count_runs.append(eng.refine_sets(qp, bm, limit=FULL, induced=True)[:2] if a.induced else eng.refine_sets(qp, bm, limit=FULL)[:2])
        ans, complete, _, ms = eng.refine_sets_vertex_counts(qp, bm, induced=a.induced, device=True)
        assert complete
        vertex_runs.append((ans, ms))
        ans, complete, _, ms = eng.refine_sets_edge_counts(qp, bm, induced=a.induced, device=True)
        assert complete
        edge_runs.append((ans, ms))
    ans = {r[0] for r in count_runs + vertex_runs + edge_runs}
    assert len(ans) == 1, ans
    row["answers"] = ans.pop()
    for key, runs in (("count", count_runs), ("vertex", vertex_runs), ("edge", edge_runs)):
        ms = [r[1] for r in runs[1:]]
        row.update({f"{key}_ms": round(min(ms), 3), f"{key}_spread_ms": round(max(ms) - min(ms), 3), f"{key}_first_ms": round(runs[0][1], 3)})
    row["edge_over_count"] = round(row["edge_ms"] / max(row["count_ms"], 1e-6), 2)
    row["edge_over_vertex"] = round(row["edge_ms"] / max(row["vertex_ms"], 1e-6), 2)
    # the edge table once on the host: every row sums to the count, and its marginals are rows of the vertex table
    vtable = eng.refine_sets_vertex_counts(qp, bm, induced=a.induced)[2]
    etable = eng.refine_sets_edge_counts(qp, bm, induced=a.induced)[2]
    qedges = binding.host_query_edges(qp)
    assert etable.shape == (len(qedges), len(g["nbrs"])) and (etable.sum(axis=1) == row["answers"]).all()
    src = np.repeat(np.arange(g["n"], dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    dst = g["nbrs"].astype(np.int64)
    for k, (qa, qb) in enumerate(qedges.tolist()):
        for u, idx in ((qa, src), (qb, dst)):
            m = np.zeros(g["n"], np.uint64)
            np.add.at(m, idx, etable[k])
            assert np.array_equal(m, vtable[u]), (k, u)
    d = np.diff(g["offsets"].astype(np.int64)).astype(np.uint64)
    if name == "wedge" and not a.induced:
        assert np.array_equal(etable[0], d[dst] - 1) and np.array_equal(etable[1], d[src] - 1)
    row["largest_cell"] = int(etable.max())
    row["entries_in_a_match"] = int((etable.sum(axis=0) > 0).sum())
    eng.close()
    err.flush()
    said = [ln for ln in open(err_path) if ln.startswith("[refine_ecount] finds=")]
    m = re.search(r"finds=(\d+) flush_adds=(\d+) leaf_adds=(\d+)", said[-1])
    finds, flushes, leaves = int(m.group(1)), int(m.group(2)), int(m.group(3))
    assert finds == row["answers"]
    row.update(flush_adds=flushes, leaf_adds=leaves, atomics_per_find=round((leaves + flushes) / max(finds, 1), 4))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--queries", default="wedge,triangle,C4,diamond,K4,C5")
    ap.add_argument("--induced", action="store_true", help="the three calls with GNNPE_MATCH_INDUCED")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_edge_counts"))
    ap.add_argument("--time-limit", type=float, default=300.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for name in (k for k in a.queries.split(",") if k):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--n", str(a.n), "--m", str(a.m), "--out", a.out]
        if a.induced:
            cmd.append("--induced")
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
