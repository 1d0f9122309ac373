#!/usr/bin/env python3
"""The standing exact query measured: what one edge batch costs through gnnpe_standing_apply_edges (a) against
the same loop composed from the entry points that take the candidate sets as a host bitmap (b), on G(n,m) 1M / 10M and the power-law
graph of the same size, 64 labels, e = 2, l = 2.

Queries: a triangle and a 4-cycle cut from the graph (found by joining rows; their labels are the graph's), in mode 0 and induced.
Batches of 1, 100 and 10 000 edges, half deletions of random edges, half insertions of random non-edges (a batch of 1: an insertion);
a batch alternates with its inverse, so the graph returns to G.

(a) and (b) run in one process on two engines that hold the same graph and ALTERNATE batch by batch, warm; per configuration the best
of three with the spread (max - min), wall clock around the whole batch and the device ms the calls report:
  (a) Engine.standing_apply_edges(insert, delete)
  (b) filter_support_delta(-1), refine_sets_delta on the host bitmap (and refine_sets_delta_nonedges for an induced query),
      apply_edges, vde, filter_support_delta(+1), support_bitmap, refine_sets_delta (and _nonedges); an induced mixed batch in two
      such steps, deletions first, as the handle applies it.
The counts of (a) and (b) are compared after every batch (counts_ok).  One JSON line per configuration on stdout.
Usage: python scripts/online_standing_measure.py [--graphs gnm,powerlaw] [--batches 1,100,10000] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnnpe_amd  # noqa: E402,F401
from gnnpe_amd import binding, synth  # noqa: E402
from online_filter_support_measure import draw_batch  # noqa: E402

FULL = 2 ** 64 - 1


def row(g, v):
    return g["nbrs"][g["offsets"][v]:g["offsets"][v + 1]].astype(np.int64)


def find_cycle(g, k, rng):
    """the vertices of a triangle (k = 3) or of a 4-cycle (k = 4) of the graph, in cycle order"""
    while True:
        a = int(rng.integers(g["n"]))
        for b in row(g, a):
            if k == 3:
                common = np.intersect1d(row(g, a), row(g, int(b)))
                if len(common):
                    return [a, int(b), int(common[0])]
            else:
                for c in row(g, int(b)):
                    common = np.setdiff1d(np.intersect1d(row(g, a), row(g, int(c))), [int(b)])
                    if int(c) != a and len(common):
                        return [a, int(b), int(c), int(common[0])]


def write_cycle(path, labels):
    k = len(labels)
    lines = [f"t {k} {k}"] + [f"v {i} {int(labels[i])} 2" for i in range(k)]
    lines += [f"e {a} {b}" for a, b in sorted((min(i, (i + 1) % k), max(i, (i + 1) % k)) for i in range(k))]
    open(path, "w").write("\n".join(lines) + "\n")


def composed_step(eng, qp, plan, table, ins, dele, induced):
    """one apply of the hand-written loop: (created, destroyed, device ms)"""
    nq = int(plan["n_vertices"])
    T = np.unique(np.array(list(ins) + list(dele), np.int64))
    ms = eng.filter_support_delta(plan, T, -1, table)
    bm = composed_step.bitmap
    destroyed = created = 0
    if len(dele):
        r = eng.refine_sets_delta(qp, bm, dele, induced=induced)
        destroyed, ms = destroyed + r[0], ms + r[2]
    if induced and len(ins):
        r = eng.refine_sets_delta_nonedges(qp, bm, ins)
        destroyed, ms = destroyed + r[0], ms + r[2]
    ms += eng.apply_edges(insert=ins, delete=dele, timing=True)[1]
    eng.vde(want=False)
    ms += eng.filter_support_delta(plan, T, +1, table)
    bm, bms = eng.support_bitmap(table, nq)
    composed_step.bitmap = bm
    ms += bms
    if len(ins):
        r = eng.refine_sets_delta(qp, bm, ins, induced=induced)
        created, ms = created + r[0], ms + r[2]
    if induced and len(dele):
        r = eng.refine_sets_delta_nonedges(qp, bm, dele)
        created, ms = created + r[0], ms + r[2]
    return created, destroyed, ms


def composed_batch(eng, qp, plan, table, ins, dele, induced):
    if induced and len(ins) and len(dele):
        c1, d1, m1 = composed_step(eng, qp, plan, table, [], dele, induced)
        c2, d2, m2 = composed_step(eng, qp, plan, table, ins, [], induced)
        return c1 + c2, d1 + d2, m1 + m2
    return composed_step(eng, qp, plan, table, ins, dele, induced)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--batches", default="1,100,10000")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=10_000_000)
    a = ap.parse_args()
    graphs = []
    if "gnm" in a.graphs:
        graphs.append((f"gnm_{a.n}_{a.m}", lambda: synth.gnm_graph(a.n, a.m)))
    if "powerlaw" in a.graphs:
        graphs.append((f"powerlaw_{a.n}_{a.m}", lambda: synth.powerlaw_graph(a.n, a.m)))
    qdir = a.out or os.path.join(ROOT, "profile_out", "online_standing")
    os.makedirs(qdir, exist_ok=True)
    for gname, make in graphs:
        g = make()
        rng = np.random.default_rng(2026)
        brng = np.random.default_rng(2027)
        batches = {k: draw_batch(g, k, brng) for k in (int(x) for x in a.batches.split(","))}
        engines = []
        for _ in range(2):
            eng = binding.Engine(0)
            eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
            eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
            eng.vde(want=False)
            engines.append(eng)
        ea, eb = engines
        for qname, k in (("triangle", 3), ("c4", 4)):
            qp = os.path.join(qdir, f"{gname}_{qname}.graph")
            write_cycle(qp, g["labels"][find_cycle(g, k, rng)])
            plan = binding.host_query_plan_exact(qp, 2, 2)
            for induced in (False, True):
                t0 = time.perf_counter()
                sq = ea.standing_open(qp, l=2, induced=induced)
                open_wall = (time.perf_counter() - t0) * 1e3
                table, _ = eb.filter_support_exact(plan)
                composed_step.bitmap = eb.support_bitmap(table, int(plan["n_vertices"]))[0]
                count_b = eb.refine_sets(qp, composed_step.bitmap, limit=FULL, induced=induced)[0]
                for size, (ins, dele) in batches.items():
                    print(f"{gname} {qname} induced={induced} batch={size}", file=sys.stderr, flush=True)
                    runs_a, runs_b, ok = [], [], True
                    for i in range(8):  # forwards, backwards, ...: the first pair is the warm-up
                        bi, bd = (ins, dele) if i % 2 == 0 else (dele, ins)
                        t0 = time.perf_counter()
                        ms_a = ea.standing_apply_edges(insert=bi, delete=bd, timing=True)
                        wall_a = (time.perf_counter() - t0) * 1e3
                        t0 = time.perf_counter()
                        created, destroyed, ms_b = composed_batch(eb, qp, plan, table, bi, bd, induced)
                        wall_b = (time.perf_counter() - t0) * 1e3
                        count_b += created - destroyed
                        res = sq.result()
                        ok = ok and res[:3] == (count_b, created, destroyed)
                        if i >= 2:
                            runs_a.append((wall_a, ms_a))
                            runs_b.append((wall_b, ms_b))
                    pick = lambda runs, j: (round(min(r[j] for r in runs), 3), round(max(r[j] for r in runs) - min(r[j] for r in runs), 3))
                    print(json.dumps(dict(graph=gname, query=qname, induced=induced, batch=size, applies=2 if induced and len(ins) and len(dele) else 1,
                                          count=res[0], created=res[1], destroyed=res[2], counts_ok=ok, open_wall_ms=round(open_wall, 3),
                                          standing_wall_ms=pick(runs_a, 0), standing_device_ms=pick(runs_a, 1),
                                          composed_wall_ms=pick(runs_b, 0), composed_device_ms=pick(runs_b, 1))), flush=True)
                sq.close()
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    main()
