#!/usr/bin/env python3
"""Exact online queries measured (DESIGN.md "Exact online queries"): the 1M-vertex / 10M-edge G(n,m) graph with 64 labels (and
the power-law graph of the same size), cut queries of 8 vertices; per query and mode -- l = 2 reference, l = 2 exact, l = 3 --
the filter's device time (best of three warm runs), total candidates, the start vertex' candidates (the refinement starts from
the query vertex with the fewest) and the device refinement's time.  One JSON line per (graph, query, mode) on stdout.
The refinement runs on the G(n,m) graph only: on the power-law graph the first query's reference-mode step did not finish in
seven minutes, and the filter alone takes milliseconds there.  The query graphs go to --out
(default profile_out/online_exact/ in the repository, which git ignores).
Usage: python scripts/online_exact_measure.py [--queries 5] [--out DIR] [--graphs gnm,powerlaw]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gnnpe_amd  # noqa: E402,F401
from gnnpe_amd import binding, synth  # noqa: E402
from make_golden_online import cut_query  # noqa: E402


def popcounts(bm):
    return [int(np.unpackbits(row.view(np.uint8)).sum()) for row in bm]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=5)
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", default="gnm,powerlaw")
    a = ap.parse_args()
    graphs = []
    if "gnm" in a.graphs:
        graphs.append(("gnm_1m_10m", lambda: synth.gnm_graph(1_000_000, 10_000_000), True))
    if "powerlaw" in a.graphs:
        graphs.append(("powerlaw_1m_10m", lambda: synth.powerlaw_graph(1_000_000, 10_000_000), False))
    qdir = a.out or os.path.join(ROOT, "profile_out", "online_exact")
    os.makedirs(qdir, exist_ok=True)
    for gname, make, with_refine in graphs:
        g = make()
        sn = synth.degree_order(g["offsets"])
        eng = binding.Engine(0)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
        eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
        eng.vde(want=False)
        rng = np.random.default_rng(2026)
        for k in range(a.queries):
            qp = os.path.join(qdir, f"{gname}_q{k}.graph")
            open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], a.size, rng))
            for mode in ("l2_reference", "l2_exact", "l3"):
                print(f"{gname} q{k} {mode}", file=sys.stderr, flush=True)
                if mode == "l2_reference":
                    plan = binding.host_query_plan(qp, 2)
                    run = lambda: eng.filter_candidates(plan)  # noqa: E731
                    sizes = [len(plan["vids"])]
                else:
                    plan = binding.host_query_plan_exact(qp, 2, 2 if mode == "l2_exact" else 3)
                    run = lambda: eng.filter_candidates_exact(plan)  # noqa: E731
                    sizes = [len(plan[p]["vids"]) for p in ("main", "tri", "single")]
                ms = []
                for _ in range(4):
                    bm, t = run()
                    ms.append(t)
                cand = popcounts(bm)
                answers, rms = eng.refine(qp, bm) if with_refine else (None, None)
                print(json.dumps(dict(graph=gname, query=k, mode=mode, plan=sizes, filter_ms=round(min(ms[1:]), 3),
                                      filter_ms_first=round(ms[0], 3), candidates=sum(cand), start_candidates=min(cand),
                                      refine_ms=None if rms is None else round(rms, 3), answers=answers)), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
