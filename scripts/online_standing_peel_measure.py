#!/usr/bin/env python3
"""Peeling the resident graph by edge support measured: gnnpe_csr_edges_below on its own, one round of
gnnpe_standing_peel against the loop a user writes without it, and gnnpe_standing_truss_levels.

Setup as scripts/online_standing_counts_measure.py: G(n,m) 1M / 10M and the power-law graph of the same size, 64 labels, e = 2,
l = 2; a triangle and a 4-cycle cut from the graph, DISTINCT mode, the handle keeping E.

select   gnnpe_csr_edges_below alone on a table of nqe x entries random cells (0 .. 999) in device memory, thresholds found by
         bisection on the call's own n_selected so that no edge, about 1 % and about 50 % of the edges are selected; cap = every
         edge.  Device ms, best of `runs` warm calls with the spread, and the gather requests per second: per entry one adj_start[y]
         and one nbrs[r], per edge nqe cells at r, in pass 1 and again in the tiles pass 2 does not skip; and the bytes per second
         over what a pass has to read (16 per entry: nbrs, revpos, adj_start[y], nbrs[r]; 16 nqe per edge: the cells at j and r).
round    one round at threshold 1 on the handle's own E, warm, (a) and (b) ALTERNATING in one process, best of `runs`, wall and
         device ms; the removed edges are inserted again after every round (not timed):
  (a) StandingQuery.peel(1, max_rounds=1)
  (b) the loop without it: StandingQuery.counts("edge") to the host, Engine.download_csr(), the select in numpy (keys, the
      reverse entry by searchsorted, the two directions added, the pairs below the threshold), Engine.standing_apply_edges(delete).
      The parts are reported next to the sum.
levels   StandingQuery.truss_levels with and without restore: rounds, levels, wall and device ms (once each: the call is its own
         repeat, it peels until nothing is left).
One JSON line per measurement on stdout.
Usage: python scripts/online_standing_peel_measure.py [--graphs gnm,powerlaw] [--queries triangle,c4] [--runs 6] [--n N --m M]
       [--skip select,round,levels] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gnnpe_amd  # noqa: E402,F401
from gnnpe_amd import binding, synth  # noqa: E402
from online_standing_measure import find_cycle, write_cycle  # noqa: E402

FULL = 2 ** 64 - 1


def spread(xs):
    return (round(min(xs), 4), round(max(xs) - min(xs), 4))


def measure_select(eng, nqe, entries, runs, tag):
    import torch
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    table = torch.randint(0, 1000, (nqe, entries), dtype=torch.int64, device="cuda:0", generator=gen)
    edges = entries // 2
    pairs = torch.zeros((edges, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def threshold_for(share):  # the smallest threshold that selects at least share * edges
        lo, hi = 0, 2 * nqe * 1000
        while lo < hi:
            mid = (lo + hi) // 2
            if eng.edges_below(table, nqe, mid)[0] >= share * edges:
                hi = mid
            else:
                lo = mid + 1
        return lo

    for what, t in (("none", 0), ("1 %", threshold_for(0.01)), ("50 %", threshold_for(0.5))):
        ms = []
        for i in range(runs + 1):
            n_sel, low, m = eng.edges_below(table, nqe, t, pairs, edges, timing=True)
            if i:
                ms.append(m)
        tiles = (entries + 2047) // 2048
        passes = 1 + (1 if n_sel else 0)  # at 1 % and 50 % no tile of random cells is without a selected edge
        requests = passes * (2 * entries + edges * nqe)
        print(json.dumps(dict(select=tag, rows=nqe, entries=entries, tiles=tiles, pattern=what, threshold=t, selected=n_sel,
                              device_ms=spread(ms), gather_requests=requests, g_requests_per_s=round(requests / (min(ms) * 1e-3) / 1e9, 2),
                              gb_per_s=round(passes * (entries * 16 + edges * nqe * 16) / (min(ms) * 1e-3) / 1e9, 1))), flush=True)


def numpy_select(off, nb, table, t):
    n = len(off) - 1
    x = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))
    y = nb.astype(np.int64)
    rev = np.searchsorted(x * n + y, y * n + x)
    col = table.sum(axis=0, dtype=np.uint64)
    sel = (x < y) & (col + col[rev] < np.uint64(t))
    return np.column_stack([x[sel], y[sel]])


def measure_round(eng, sq, runs, tag):
    a_runs, b_runs, parts, same = [], [], [], True
    for i in range(runs + 1):
        t0 = time.perf_counter()
        removed, _, out, ms = sq.peel(1, max_rounds=1, timing=True)
        wall_a = (time.perf_counter() - t0) * 1e3
        count_a = sq.count
        if len(removed):
            eng.standing_apply_edges(insert=removed)
        t0 = time.perf_counter()
        table = sq.counts("edge")
        t1 = time.perf_counter()
        off, nb = eng.download_csr()
        t2 = time.perf_counter()
        pairs = numpy_select(off, nb, table, 1)
        t3 = time.perf_counter()
        ms_b = eng.standing_apply_edges(delete=pairs, timing=True) if len(pairs) else 0.0
        t4 = time.perf_counter()
        same = same and np.array_equal(pairs, removed.astype(np.int64)) and sq.count == count_a
        if len(pairs):
            eng.standing_apply_edges(insert=pairs)
        if i:
            a_runs.append((wall_a, ms))
            b_runs.append(((t4 - t0) * 1e3, ms_b))
            parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))
    best = min(range(len(b_runs)), key=lambda k: b_runs[k][0])
    print(json.dumps(dict(round=tag, threshold=1, edges=int(out[1] + out[2]), removed=int(out[1]), same_edges_and_count=bool(same),
                          peel_wall_ms=spread([r[0] for r in a_runs]), peel_device_ms=spread([r[1] for r in a_runs]),
                          loop_wall_ms=spread([r[0] for r in b_runs]), loop_apply_device_ms=spread([r[1] for r in b_runs]),
                          loop_parts_ms=dict(zip(("counts_to_host", "download_csr", "numpy_select", "apply"), (round(v, 3) for v in parts[best]))))),
          flush=True)


def measure_levels(eng, sq, tag):
    for restore in (True, False):
        t0 = time.perf_counter()
        edges, levels, out, ms = sq.truss_levels(restore=restore, timing=True)
        wall = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(levels=tag, restore=restore, edges=out[0], distinct_levels=out[1], largest_level=out[2], rounds=out[3],
                              wall_ms=round(wall, 3), device_ms=round(ms, 3), count_after=sq.count)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--queries", default="triangle,c4")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--skip", default="")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=10_000_000)
    a = ap.parse_args()
    graphs = []
    if "gnm" in a.graphs:
        graphs.append((f"gnm_{a.n}_{a.m}", lambda: synth.gnm_graph(a.n, a.m)))
    if "powerlaw" in a.graphs:
        graphs.append((f"powerlaw_{a.n}_{a.m}", lambda: synth.powerlaw_graph(a.n, a.m)))
    qdir = a.out or os.path.join(ROOT, "profile_out", "online_standing_peel")
    os.makedirs(qdir, exist_ok=True)
    for gname, make in graphs:
        g = make()
        rng = np.random.default_rng(2026)
        eng = binding.Engine(0)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
        eng.vde(want=False)
        for qname, k in (("triangle", 3), ("c4", 4)):
            qp = os.path.join(qdir, f"{gname}_{qname}.graph")
            write_cycle(qp, g["labels"][find_cycle(g, k, rng)])
            if qname not in a.queries:
                continue
            tag = f"{gname} {qname}"
            print(tag, file=sys.stderr, flush=True)
            if "select" not in a.skip:
                measure_select(eng, k, len(g["nbrs"]), a.runs, tag)
            sq = eng.standing_open(qp, l=2, distinct=True)
            sq.keep_counts(vertex=False, edge=True)
            if "round" not in a.skip:
                measure_round(eng, sq, a.runs, tag)
            if "levels" not in a.skip:
                measure_levels(eng, sq, tag)
            sq.close()
            # (the levels without restore leave the empty graph: the next query starts from the loaded one)
            eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
            eng.vde(want=False)
        eng.close()


if __name__ == "__main__":
    main()
