#!/usr/bin/env python3
"""What the count tables of the induced matches on a set of non-edges cost ("Count tables of the induced
matches on a set of non-edges"): gnnpe_refine_sets_delta_nonedges_vertex_counts / _edge_counts beside the count-only call on the
same F and beside the full induced tables they keep up to date.

Graph, bitmap and method are those of scripts/online_delta_nonedges_measure.py: powerlaw_graph(n, m, max_degree=600) with every
label 0, the label/degree bitmap, mode INDUCED, limit 2^64 - 1; the calls alternate in ONE process (this one, no children),
--rounds runs, the first dropped, the best of the warm runs with their spread.  F is drawn from the non-adjacent pairs that share a
neighbour (a random vertex with two random neighbours that are not adjacent, seed 1, by rejection; the smaller F are prefixes of the
larger) -- random non-edges of this graph carry next to no match (profiles/online_delta_nonedges.txt) -- in sizes 1, 100 and
10 000, and `hub` is the one pair of the two highest-degree vertices that are not adjacent: one item per direction, each a single
wave's work.  Per query one JSON line; per F, device ms of
  (a) plain        gnnpe_refine_sets_delta_nonedges, count only: the floor, the search is the same;
  (b) v_own/e_own  the two new calls with the context-owned table (zeroed inside the timed span), and
      v_acc/e_acc  the same calls accumulating with sign +1 into a caller's table (no zeroing; the table just wraps);
and per query
  (d) v_full/e_full  gnnpe_refine_sets_vertex_counts / _edge_counts in the induced mode: what keeping the table costs without them.
The tables of (b) are checked in the run: every row sums to N, and N is the count-only call's.  Every step says on stderr when it
ended, so that a run that is ended at its time limit shows how far it came; --sizes leaves some F out (C5 with all four did not end
inside 420 s).
Run one query per invocation under a time limit (`timeout 300 python scripts/online_delta_nonedges_counts_measure.py --queries
wedge && ...`): a run that had to be ended is not repeated.
Usage: python scripts/online_delta_nonedges_counts_measure.py [--n 20000] [--m 80000] [--rounds 4] [--queries wedge,C4,diamond,C5]
       [--sizes 1,100,10000,hub]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from online_delta_measure import FULL, SHAPES, SIZES, ld_bitmap, write_query  # noqa: E402

QUERIES = "wedge,C4,diamond,C5"


def best(ms):
    return dict(ms=round(min(ms[1:]), 3), spread_ms=round(max(ms[1:]) - min(ms[1:]), 3), first_ms=round(ms[0], 3))


def adjacent(g, x, y):
    o = g["offsets"]
    row = g["nbrs"][o[x]:o[x + 1]]
    i = np.searchsorted(row, y)
    return i < len(row) and row[i] == y


def wedge_ends(g, k, seed):
    """k different pairs x < y that are no edges of g and have a common neighbour, in the order they were drawn"""
    n = g["n"]
    o = g["offsets"].astype(np.int64)
    mids = np.nonzero(np.diff(o) >= 2)[0]
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < k:
        z = int(mids[rng.integers(0, len(mids))])
        x, y = sorted(int(g["nbrs"][o[z] + i]) for i in rng.choice(o[z + 1] - o[z], 2, replace=False))
        if not adjacent(g, x, y) and x * n + y not in seen:
            seen.add(x * n + y)
            out.append((x, y))
    return np.array(out, np.int64)


def hub_pair(g):
    """the first non-adjacent pair among the vertices in descending order of degree"""
    order = np.argsort(-np.diff(g["offsets"].astype(np.int64)), kind="stable")[:50]
    return next(np.array([[min(x, y), max(x, y)]], np.int64) for i, x in enumerate(order) for y in order[i + 1:] if not adjacent(g, x, y))


def measure(name, a, g, eng, torch):
    from gnnpe_amd import binding
    nq, edges = SHAPES[name]
    qp = os.path.join(a.out, f"{name}.graph")
    write_query(qp, nq, edges, [0] * nq)
    bm = ld_bitmap(g, binding.host_load_graph(qp))
    drawn = wedge_ends(g, max(SIZES), 1)
    hub = hub_pair(g)
    deg = np.diff(g["offsets"].astype(np.int64))
    sets = [(key, F) for key, F in [(str(k), drawn[:k]) for k in SIZES] + [("hub", hub)] if key in a.sizes.split(",")]
    nqe, entries = len(edges), len(g["nbrs"])
    acc_v = torch.zeros((nq, g["n"]), dtype=torch.int64, device="cuda:0")
    acc_e = torch.zeros((nqe, entries), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, edges=entries // 2, launches=len(binding.host_query_nonedges(qp)),
               hub_degrees=[int(deg[hub[0, 0]]), int(deg[hub[0, 1]])], table_bytes=dict(vertex=nq * g["n"] * 8, edge=nqe * entries * 8))
    full = dict(v_full=[], e_full=[])
    runs = {key: dict(plain=[], v_own=[], e_own=[], v_acc=[], e_acc=[]) for key, _ in sets}
    found = {}
    said = lambda *what: print(f"[{time.perf_counter() - t0:8.2f} s]", name, *what, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    for rnd in range(a.rounds):  # alternately: every F in every form, then the full induced tables
        for key, F in sets:
            r = runs[key]
            N, _, ms = eng.refine_sets_delta_nonedges(qp, bm, F, limit=FULL)
            r["plain"].append(ms)
            nv = eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, F)
            ne = eng.refine_sets_delta_nonedges_edge_counts(qp, bm, F)
            assert nv[1] and ne[1] and nv[0] == ne[0] == N and (nv[2].sum(axis=1) == N).all() and (ne[2].sum(axis=1) == N).all()
            r["v_own"].append(nv[3])
            r["e_own"].append(ne[3])
            for kind, fn, acc in (("v_acc", eng.refine_sets_delta_nonedges_vertex_counts, acc_v),
                                  ("e_acc", eng.refine_sets_delta_nonedges_edge_counts, acc_e)):
                got = fn(qp, bm, F, accum=acc.data_ptr(), sign=1)
                assert got[:2] == (N, True)
                r[kind].append(got[3])
            found[key] = N
            said("round", rnd, "F", key, "N", N, "ms", [round(r[k][-1], 3) for k in ("plain", "v_own", "e_own", "v_acc", "e_acc")])
        fv = eng.refine_sets_vertex_counts(qp, bm, induced=True, device=True)
        fe = eng.refine_sets_edge_counts(qp, bm, induced=True, device=True)
        assert fv[1] and fe[1] and fv[0] == fe[0]
        full["v_full"].append(fv[3])
        full["e_full"].append(fe[3])
        said("round", rnd, "full tables", fv[0], "ms", round(fv[3], 3), round(fe[3], 3))
    row["induced_answers"] = fv[0]
    row["v_full"], row["e_full"] = best(full["v_full"]), best(full["e_full"])
    for key, F in sets:
        out = dict(size=len(F), N=found[key], **{k: best(v) for k, v in runs[key].items()})
        for k in ("v_own", "e_own", "v_acc", "e_acc"):
            out[k]["over_plain"] = round(out[k]["ms"] / max(out["plain"]["ms"], 1e-6), 3)
        out["v_own"]["over_full"] = round(out["v_own"]["ms"] / max(row["v_full"]["ms"], 1e-6), 4)
        out["e_own"]["over_full"] = round(out["e_own"]["ms"] / max(row["e_full"]["ms"], 1e-6), 4)
        row[f"F_{key}"] = out
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--queries", default=QUERIES)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)) + ",hub", help="which F to run: sizes, and `hub`")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_delta_nonedges_counts"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import gnnpe_amd  # noqa: F401
    import torch
    from gnnpe_amd import binding, synth
    g = synth.powerlaw_graph(a.n, a.m, max_degree=600)
    g = dict(g, labels=np.zeros(g["n"], np.uint32))
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(synth.degree_order(g["offsets"]), np.zeros(g["n"], np.uint32), 1)
    eng.set_label_table(binding.host_label_table(1, 2))
    eng.vde(want=False)
    for name in (k for k in a.queries.split(",") if k):
        measure(name, a, g, eng, torch)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
