#!/usr/bin/env python3
"""What the induced matches on a set of non-edges cost ("Induced matches on a set of non-edges"):
gnnpe_refine_sets_delta_nonedges for F of 1, 100 and 10 000 random non-edges, beside the whole induced count
(gnnpe_refine_sets_mode, GNNPE_MATCH_INDUCED, count only) for the same query on the same graph and bitmap, in the same process.

Graph: powerlaw_graph(n, m, max_degree=600) of section 3.7 (default 20 000 / 80 000) with every label 0 -- the motif setting and
the graph of profiles/online_delta.txt.  Queries: wedge, C4, diamond and C5, mode INDUCED, the label/degree bitmap, limit 2^64 - 1,
no rows.  Per query one JSON line: the induced count and its device ms, the launches of a call (one per non-adjacent query pair),
then per F its size, N and the device ms; every ms is the best of the warm runs, with their spread (--rounds runs, the first
dropped; the calls alternate in one process).  The random non-edges are drawn with seed 1 by rejection and the smaller F are
prefixes of the larger.
Every query runs in a child process under a time limit of its own (--time-limit seconds); a child that passes it is ended, a
"timed_out" row follows and nothing is run again.
Usage: python scripts/online_delta_nonedges_measure.py [--n 20000] [--m 80000] [--rounds 4] [--time-limit 300] [--queries wedge,C4,...]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from online_delta_measure import FULL, SHAPES, SIZES, ld_bitmap, write_query  # noqa: E402

QUERIES = "wedge,C4,diamond,C5"


def random_non_edges(g, k, seed):
    """k different pairs x < y that are no edges of g, in the order they were drawn"""
    n = g["n"]
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    have = set((src * n + g["nbrs"].astype(np.int64)).tolist())
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < k:
        x, y = sorted(int(v) for v in rng.integers(0, n, 2))
        if x != y and x * n + y not in have and x * n + y not in seen:
            seen.add(x * n + y)
            out.append((x, y))
    return np.array(out, np.int64)


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
    drawn = random_non_edges(g, max(SIZES), 1)
    sets = [(str(k), drawn[:k]) for k in SIZES]
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, edges=len(g["nbrs"]) // 2, launches=len(binding.host_query_nonedges(qp)))
    count_runs, non_runs = [], {key: [] for key, _ in sets}
    for _ in range(a.rounds):  # alternately: the whole induced count, then every F
        count_runs.append(eng.refine_sets(qp, bm, limit=FULL, induced=True)[:2])
        for key, F in sets:
            ans, _, ms = eng.refine_sets_delta_nonedges(qp, bm, F)
            non_runs[key].append((ans, ms))
    assert len({r[0] for r in count_runs}) == 1
    row["induced_answers"] = count_runs[0][0]
    ms = [r[1] for r in count_runs[1:]]
    row.update(count_ms=round(min(ms), 3), count_spread_ms=round(max(ms) - min(ms), 3), count_first_ms=round(count_runs[0][1], 3))
    for key, F in sets:
        runs = non_runs[key]
        assert len({r[0] for r in runs}) == 1, (key, runs)
        ms = [r[1] for r in runs[1:]]
        row[f"F_{key}"] = dict(size=len(F), N=runs[0][0], ms=round(min(ms), 3), spread_ms=round(max(ms) - min(ms), 3),
                               first_ms=round(runs[0][1], 3), over_count=round(min(ms) / max(row["count_ms"], 1e-6), 4))
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--queries", default=QUERIES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_delta_nonedges"))
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
