#!/usr/bin/env python3
"""What the induced test costs and what it cuts ("Induced matching"): gnnpe_refine_sets against
gnnpe_refine_sets_mode with GNNPE_MATCH_INDUCED on the same label/degree bitmap, alternating in one process.

Graph: powerlaw_graph(n, m, max_degree=600) of section 3.7 (default 20 000 / 80 000) with every label 0 -- the motif setting.
Queries: wedge, C4, diamond, C5, star5 (a centre and four leaves) and the 6-vertex path.  Per query one JSON line: R, I, the
non-adjacent pairs, both device ms (best of three warm runs and the spread of the three) and plain / induced.  The induced call
does extra binary searches per surviving lane and cuts the subtrees below an image that is adjacent to one it must not be adjacent
to; which of the two wins on which query is what the line says.
--limit (default 2^64 - 1) bounds both calls alike.  Under a limit below the counts both answers are the limit and the line compares
the time to reach it, not the time to walk the whole tree: star5 and path6 hold 3.6 x 10^12 and up to 1.5 x 10^13 monomorphisms
on the default graph (sum d(d-1)(d-2)(d-3); the 5-walks), which is what the option is for.
Every query runs in a child process under a time limit of its own (--time-limit seconds); a child that passes it is ended, a
"timed_out" row follows and nothing is run again.
Usage: python scripts/online_induced_measure.py [--n 20000] [--m 80000] [--out DIR] [--time-limit 300] [--limit L]
       [--queries wedge,C4,...]"""
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
    "C4": (4, ((0, 1), (1, 2), (2, 3), (0, 3))),
    "diamond": (4, ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3))),
    "C5": (5, ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4))),
    "star5": (5, ((0, 1), (0, 2), (0, 3), (0, 4))),
    "path6": (6, ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5))),
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
    print(f"{name}", file=sys.stderr, flush=True)
    bm = ld_bitmap(g, binding.host_load_graph(qp))
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, nonedges=nq * (nq - 1) // 2 - len(edges),
               limit=None if a.limit == FULL else a.limit)
    # alternately: plain, induced, plain, induced, ...
    runs = {False: [], True: []}
    for _ in range(4):
        for induced in (False, True):
            runs[induced].append(eng.refine_sets(qp, bm, limit=a.limit, induced=induced))
    for induced, key in ((False, "plain"), (True, "induced")):
        ans = {r[0] for r in runs[induced]}
        assert len(ans) == 1, ans
        ms = [r[1] for r in runs[induced][1:]]
        row.update({f"{key}_answers": ans.pop(), f"{key}_ms": round(min(ms), 3), f"{key}_spread_ms": round(max(ms) - min(ms), 3),
                    f"{key}_first_ms": round(runs[induced][0][1], 3)})
    row["ratio"] = round(row["plain_ms"] / max(row["induced_ms"], 1e-6), 2)
    print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--queries", default="wedge,C4,diamond,C5,star5,path6")
    ap.add_argument("--limit", type=int, default=FULL)
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_induced"))
    ap.add_argument("--time-limit", type=float, default=300.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for name in (k for k in a.queries.split(",") if k):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--n", str(a.n), "--m", str(a.m), "--limit", str(a.limit),
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
