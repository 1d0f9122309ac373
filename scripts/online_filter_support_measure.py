#!/usr/bin/env python3
"""The exact filter's support table measured: what a standing exact query pays per edge batch with the table
(a) against what the loop costs without it (b), on the graphs and queries of scripts/online_exact_measure.py -- G(n,m) 1M / 10M and
the power-law graph of the same size, 64 labels, e = 2, the same five cut queries of 8 vertices, l = 2 exact and l = 3.

Per (graph, query, l, batch size in 1, 64, 4096), one JSON line on stdout:
  (a) delta_minus_ms + delta_plus_ms + bitmap_ms: filter_support_delta(-1) on G, apply_edges, vde, filter_support_delta(+1) on G',
      support_bitmap -- device ms, best of three warm batches.  A batch is half deletions of random edges, half insertions of random
      non-edges (a batch of 1: an insertion); batches alternate with their inverses, so the graph returns to G.
  (b) set_order + filter_candidates_exact on the updated graph: order_filter_wall_ms (host clock around both calls) and
      filter_ms (device), best of three warm runs.
  (c) full_table_ms: filter_support_exact once per (query, l), best of three warm runs.
After the batches the carried table is compared with a recomputed one on the device (table_ok).
Usage: python scripts/online_filter_support_measure.py [--queries 5] [--graphs gnm,powerlaw] [--batches 1,64,4096] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gnnpe_amd  # noqa: E402,F401
from gnnpe_amd import binding, synth  # noqa: E402
from make_golden_online import cut_query  # noqa: E402


def draw_batch(g, k, rng):
    """(insertions, deletions): k // 2 random edges to delete, the rest random non-edges to insert"""
    n, offs, nbrs = g["n"], g["offsets"].astype(np.int64), g["nbrs"]
    dele = set()
    while len(dele) < k // 2:
        j = int(rng.integers(len(nbrs)))
        a = int(np.searchsorted(offs, j, side="right")) - 1
        dele.add((min(a, int(nbrs[j])), max(a, int(nbrs[j]))))
    ins = set()
    while len(ins) < k - k // 2:
        a, b = sorted(int(x) for x in rng.integers(0, n, 2))
        if a != b and b not in nbrs[offs[a]:offs[a + 1]]:
            ins.add((a, b))
    return sorted(ins), sorted(dele)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=5)
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--lengths", default="2,3")
    a = ap.parse_args()
    graphs = []
    if "gnm" in a.graphs:
        graphs.append(("gnm_1m_10m", lambda: synth.gnm_graph(1_000_000, 10_000_000)))
    if "powerlaw" in a.graphs:
        graphs.append(("powerlaw_1m_10m", lambda: synth.powerlaw_graph(1_000_000, 10_000_000)))
    qdir = a.out or os.path.join(ROOT, "profile_out", "online_filter_support")
    os.makedirs(qdir, exist_ok=True)
    for gname, make in graphs:
        g = make()
        n = g["n"]
        sn, member = synth.degree_order(g["offsets"]), np.zeros(n, np.uint32)
        eng = binding.Engine(0)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
        eng.vde(want=False)
        rng = np.random.default_rng(2026)
        brng = np.random.default_rng(2027)
        batches = {k: draw_batch(g, k, brng) for k in (int(x) for x in a.batches.split(","))}
        for q in range(a.queries):
            qp = os.path.join(qdir, f"{gname}_q{q}.graph")
            open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], a.size, rng))
            for l in (int(x) for x in a.lengths.split(",")):
                plan = binding.host_query_plan_exact(qp, 2, l)
                nq = int(plan["n_vertices"])
                table, _ = eng.filter_support_exact(plan)
                full_ms = min(eng.filter_support_exact(plan, table=table)[1] for _ in range(3))
                for k, (ins, dele) in batches.items():
                    print(f"{gname} q{q} l={l} batch={k}", file=sys.stderr, flush=True)
                    T = np.unique(np.array(ins + dele, np.int64))
                    runs, today = [], []
                    for i in range(4):  # forwards, backwards, ...: the first one is the warm-up
                        fwd = i % 2 == 0
                        minus = eng.filter_support_delta(plan, T, -1, table)
                        eng.apply_edges(insert=ins if fwd else dele, delete=dele if fwd else ins)
                        eng.vde(want=False)
                        plus = eng.filter_support_delta(plan, T, +1, table)
                        bm, bms = eng.support_bitmap(table, nq)
                        runs.append((minus + plus + bms, minus, plus, bms))
                        if i == 0:  # (b) on the updated graph: what every batch costs without the table
                            for _ in range(4):
                                t0 = time.perf_counter()
                                eng.set_order(sn, member, 1)
                                bm_b, fms = eng.filter_candidates_exact(plan)
                                today.append(((time.perf_counter() - t0) * 1e3, fms))
                            same = bool(np.array_equal(bm, bm_b))
                    best, today_best = min(runs[1:]), min(today[1:])
                    check = eng.filter_support_exact(plan)[0]
                    print(json.dumps(dict(graph=gname, query=q, l=l, batch=k, touched=len(T), plan=[len(plan[p]["vids"]) for p in ("main", "tri", "single")],
                                          incremental_ms=round(best[0], 3), delta_minus_ms=round(best[1], 3), delta_plus_ms=round(best[2], 3),
                                          bitmap_ms=round(best[3], 3), order_filter_wall_ms=round(today_best[0], 3),
                                          filter_ms=round(min(t[1] for t in today[1:]), 3), full_table_ms=round(full_ms, 3),
                                          bitmap_equals_filter=same, table_ok=bool(torch.equal(table, check)))), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
