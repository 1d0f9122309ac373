#!/usr/bin/env python3
"""What symmetry breaking buys ("Distinct subgraphs"): gnnpe_refine_sets against
gnnpe_refine_sets_distinct on the same label/degree bitmap, alternating in one process, limit 2^64 - 1.

Graph: powerlaw_graph(n, m, max_degree=600) of section 3.7 (default 20 000 / 80 000) with every label 0 -- the motif setting,
where the whole cost is the size of the search tree.  Queries: triangle, C4, diamond, K4, C5.  Per query one JSON line: R, D,
|Aut|, both device ms (best of three warm runs and the spread of the three) and plain / distinct next to |Aut|.  Every query is
run twice, with the row trim and with GNNPE_TESTING=sets_trim=0 (the bounds are then compared only), each in a child process of
its own since the switch is read when a context is created.
Fixed cost: the diamond with labels 0, 1, 0, 1 (no symmetry: both calls run the same kernel) on a copy of the graph with labels
alternating by vertex id.
Every child runs under a time limit of its own (--time-limit seconds); a child that passes it is ended, its finished rows stay, a
"timed_out" row follows and nothing is run again.
Usage: python scripts/online_distinct_measure.py [--n 20000] [--m 80000] [--out DIR] [--time-limit 400] [--queries triangle,C4,...]"""
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
    "triangle": (3, ((0, 1), (0, 2), (1, 2))),
    "C4": (4, ((0, 1), (1, 2), (2, 3), (0, 3))),
    "diamond": (4, ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3))),
    "K4": (4, tuple((a, b) for a in range(4) for b in range(a + 1, 4))),
    "C5": (5, ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4))),
}
CHILDREN = ("two_labels", "one_label_trim", "one_label_no_trim")


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


def child(kind, a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    g = synth.powerlaw_graph(a.n, a.m, max_degree=600)
    two = kind == "two_labels"
    g = dict(g, labels=(np.arange(g["n"]) % 2 if two else np.zeros(g["n"])).astype(np.uint32))
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(synth.degree_order(g["offsets"]), np.zeros(g["n"], np.uint32), 1)
    eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
    eng.vde(want=False)
    names = ["diamond"] if two else [k for k in a.queries.split(",") if k]
    for name in names:
        nq, edges = SHAPES[name]
        qp = os.path.join(a.out, f"{name}_{kind}.graph")
        write_query(qp, nq, edges, [i % 2 for i in range(nq)] if two else [0] * nq)
        print(f"{kind} {name}", file=sys.stderr, flush=True)
        aut, pairs = binding.host_query_symmetry(qp)
        bm = ld_bitmap(g, binding.host_load_graph(qp))
        row = dict(graph=f"powerlaw_{a.n}_{a.m}", labels=2 if two else 1, query=name, trim=kind != "one_label_no_trim", aut=aut,
                   pairs=len(pairs))
        # alternately: plain, distinct, plain, distinct, ...
        runs = {False: [], True: []}
        for _ in range(4):
            for distinct in (False, True):
                runs[distinct].append(eng.refine_sets(qp, bm, limit=FULL, distinct=distinct))
        for distinct, key in ((False, "plain"), (True, "distinct")):
            ans = {r[0] for r in runs[distinct]}
            assert len(ans) == 1, ans
            ms = [r[1] for r in runs[distinct][1:]]
            row.update({f"{key}_answers": ans.pop(), f"{key}_ms": round(min(ms), 3), f"{key}_spread_ms": round(max(ms) - min(ms), 3),
                        f"{key}_first_ms": round(runs[distinct][0][1], 3)})
        row["ratio"] = round(row["plain_ms"] / max(row["distinct_ms"], 1e-6), 2)
        row["counts_agree"] = row["distinct_answers"] * aut == row["plain_answers"]
        print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--queries", default="triangle,C4,diamond,K4,C5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_distinct"))
    ap.add_argument("--time-limit", type=float, default=400.0)
    ap.add_argument("--children", default=",".join(CHILDREN))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for kind in CHILDREN:
        if kind not in a.children.split(","):
            continue
        env = dict(os.environ)
        if kind == "one_label_no_trim":
            env["GNNPE_TESTING"] = "sets_trim=0"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(a.n), "--m", str(a.m), "--queries", a.queries,
               "--out", a.out]
        p = subprocess.Popen(cmd, env=env)  # a fresh process per run: its rows go straight to this stdout
        try:
            rc = p.wait(timeout=a.time_limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            print(json.dumps(dict(child=kind, timed_out=True, time_limit_s=a.time_limit)), flush=True)
            return 1  # nothing more is started after a run that had to be ended
        if rc != 0:
            print(json.dumps(dict(child=kind, failed=True, returncode=rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
