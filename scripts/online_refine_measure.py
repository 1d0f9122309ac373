#!/usr/bin/env python3
"""The two device refinements measured side by side: the graphs and queries of
scripts/online_exact_measure.py -- 1M vertices / 10M edges, G(n,m) and power-law, 64 labels, cut queries of 8 vertices, query rng
2026 -- in its two exact modes (l = 2 exact, l = 3; the reference-mode sets are incomplete, so the two refinements answer
different questions there).  Per (graph, query, mode) one JSON line on stdout: the frozen refinement's (gnnpe_refine) and the
set-restricted one's (gnnpe_refine_sets) device ms, best of three warm runs, the spread of those three, and both answers.

On the power-law graph the frozen refinement is not run (it did not finish there: DESIGN.md section 3.7); the set-restricted one
runs with limit = 10^9 and the row records time, answer and whether the limit was reached.  Every graph is measured in a child
process under a time limit of its own (--time-limit seconds); a child that passes it is ended, its finished rows stay, a
"timed_out" row follows and nothing is run again.
Usage: python scripts/online_refine_measure.py [--queries 5] [--out DIR] [--graphs gnm,powerlaw] [--time-limit 600]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

GRAPHS = {"gnm": "gnm_1m_10m", "powerlaw": "powerlaw_1m_10m"}
POWERLAW_LIMIT = 10 ** 9


def popcounts(bm):
    return [int(np.unpackbits(row.view(np.uint8)).sum()) for row in bm]


def warm_best(run, warm=3, slow_ms=5000.0):
    """(result, best ms of `warm` warm runs, their spread, ms of the first run); a first run above slow_ms is not repeated"""
    res, first = run()
    if first > slow_ms:
        return res, first, 0.0, first
    ms = [run()[1] for _ in range(warm)]
    return res, min(ms), max(ms) - min(ms), first


def child(kind, a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    from make_golden_online import cut_query
    gname = GRAPHS[kind]
    g = synth.gnm_graph(1_000_000, 10_000_000) if kind == "gnm" else synth.powerlaw_graph(1_000_000, 10_000_000)
    sn = synth.degree_order(g["offsets"])
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
    eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
    eng.vde(want=False)
    rng = np.random.default_rng(2026)
    limit = 0xFFFFFFFF if kind == "gnm" else POWERLAW_LIMIT
    for k in range(a.queries):
        qp = os.path.join(a.out, f"{gname}_q{k}.graph")
        open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], a.size, rng))
        for mode, l in (("l2_exact", 2), ("l3", 3)):
            print(f"{gname} q{k} {mode}", file=sys.stderr, flush=True)
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            cand = popcounts(bm)
            row = dict(graph=gname, query=k, mode=mode, candidates=sum(cand), start_candidates=min(cand), limit=limit)
            if kind == "gnm":
                ans, ms, spread, first = warm_best(lambda: eng.refine(qp, bm, limit))
                row.update(frozen_ms=round(ms, 3), frozen_spread_ms=round(spread, 3), frozen_first_ms=round(first, 3),
                           frozen_answers=ans)
            ans, ms, spread, first = warm_best(lambda: eng.refine_sets(qp, bm, limit))
            row.update(sets_ms=round(ms, 3), sets_spread_ms=round(spread, 3), sets_first_ms=round(first, 3), sets_answers=ans,
                       limit_reached=ans >= limit)
            print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=5)
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_refine"))
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--time-limit", type=float, default=600.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for kind in GRAPHS:
        if kind not in a.graphs.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--queries", str(a.queries), "--size", str(a.size),
               "--out", a.out]
        p = subprocess.Popen(cmd)  # a fresh process per graph: its rows go straight to this stdout
        try:
            rc = p.wait(timeout=a.time_limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            print(json.dumps(dict(graph=GRAPHS[kind], timed_out=True, time_limit_s=a.time_limit)), flush=True)
            return 1  # nothing more is started after a run that had to be ended
        if rc != 0:
            print(json.dumps(dict(graph=GRAPHS[kind], failed=True, returncode=rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
