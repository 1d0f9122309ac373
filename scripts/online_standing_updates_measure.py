#!/usr/bin/env python3
"""Relabels and vertex batches through a standing exact query measured: what one batch costs through
gnnpe_standing_set_labels / gnnpe_standing_apply_vertices (a), against the loop of include/gnnpe_hip.h composed by hand with a host
mirror of the rows -- the recipe of `gnnpe_main --incremental`, its gnnpe_csr_download after a vertex batch included -- (b), and
against the plain update followed by gnnpe_vde and gnnpe_standing_refresh (c).

Setup as scripts/online_standing_counts_measure.py: G(n,m) 1M / 10M and the power-law graph of the same size, 64 labels, e = 2; a
triangle and a 4-cycle cut from the graph, mode 0, l = 2 (--l 3 for the other path length); batches of 1, 100 and 10 000 vertices:
  relabel  R random vertices to the next label, the following batch back to the labels of before
  remove   R random vertices leave (every batch another R: the graph shrinks by 7 batches' worth over a configuration)
  add      as many vertices arrive, labels drawn at random
With --hub the relabel batches contain the vertex of the largest degree: the case in which T = R u N(R) is a hub's whole
neighbourhood and recomputing may win.

(a), (b) and (c) run in one process on three engines that hold the same graph and take the same batches in turn, warm; per
configuration the best of six with the spread (max - min) after one warm-up batch, wall clock around the whole batch and the
device ms the calls report ((c): wall clock only for the update and vde, the refresh's device ms):
  (a) Engine.standing_set_labels / Engine.standing_apply_vertices, rows_cap 0, no kept table
  (b) T = R u N(R) from the host copy of the CSR; filter_support_delta(-1); refine_sets_delta_vertices on the host bitmap;
      set_vertex_labels, or apply_vertices + carry_vertices + download_csr; vde; filter_support_delta(+1) over T or T';
      support_bitmap; refine_sets_delta_vertices on the new bitmap
  (c) set_vertex_labels or apply_vertices; vde; StandingQuery.refresh
The counts of the three are compared after every batch (counts_ok).  One JSON line per configuration on stdout; the last line
names, per (graph, query, kind), the smallest measured batch at which (c) was cheaper than (a) in wall clock, or null.
Usage: python scripts/online_standing_updates_measure.py [--graphs gnm,powerlaw] [--batches 1,100,10000] [--queries triangle,c4]
       [--kinds relabel,remove,add] [--l 2] [--hub] [--n N --m M] [--out DIR]
The output this repository keeps is profiles/online_standing_updates.txt."""
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


def with_neighbours(offs, nbrs, R):
    R = np.asarray(R, np.int64)
    rows = [nbrs[offs[v]:offs[v + 1]].astype(np.int64) for v in R]
    return np.unique(np.concatenate([R] + rows)) if len(R) else R


class Composed:
    """the hand-written loops on an engine of its own: S as a torch tensor, the bitmap and a copy of the CSR on the host"""

    def __init__(self, eng, g, qp, plan):
        import torch
        self.torch, self.eng, self.qp, self.plan = torch, eng, qp, plan
        self.nq = int(plan["n_vertices"])
        self.offs, self.nbrs = g["offsets"].astype(np.int64), g["nbrs"]
        self.table, _ = eng.filter_support_exact(plan)
        self.bm = eng.support_bitmap(self.table, self.nq)[0]
        self.count = eng.refine_sets(qp, self.bm, limit=FULL)[0]

    def relabel(self, R, labels):
        eng = self.eng
        T = with_neighbours(self.offs, self.nbrs, R)
        ms = eng.filter_support_delta(self.plan, T, -1, self.table)
        lost, _, m = eng.refine_sets_delta_vertices(self.qp, self.bm, R)
        ms += m + eng.set_vertex_labels(R, labels, timing=True)
        eng.vde(want=False)
        ms += eng.filter_support_delta(self.plan, T, +1, self.table)
        self.bm, m2 = eng.support_bitmap(self.table, self.nq)
        gained, _, m3 = eng.refine_sets_delta_vertices(self.qp, self.bm, R)
        self.count += gained - lost
        return gained, lost, ms + m2 + m3

    def vertices(self, rem, add):
        eng, torch = self.eng, self.torch
        rem = np.unique(np.asarray(rem, np.int64))
        T = with_neighbours(self.offs, self.nbrs, rem)
        ms, lost = 0.0, 0
        if len(T):
            ms += eng.filter_support_delta(self.plan, T, -1, self.table)
            lost, _, m = eng.refine_sets_delta_vertices(self.qp, self.bm, rem)
            ms += m
        n2, _, _, _, _, m = eng.apply_vertices(rem, add, timing=True)
        ms += m
        dst = torch.empty((self.nq, n2), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ms += eng.carry_vertices(self.table, dst, self.nq, timing=True)
        self.table = dst
        eng.vde(want=False)
        keep = np.setdiff1d(T, rem)
        T2 = np.concatenate([keep - np.searchsorted(rem, keep), np.arange(n2 - len(add), n2)])  # the new ids of N(R) \\ R, and A
        if len(T2):
            ms += eng.filter_support_delta(self.plan, T2, +1, self.table)
        self.bm, m = eng.support_bitmap(self.table, self.nq)
        ms += m
        gained = 0
        if len(add):
            gained, _, m = eng.refine_sets_delta_vertices(self.qp, self.bm, np.arange(n2 - len(add), n2))
            ms += m
        offs, self.nbrs = eng.download_csr()  # the host mirror of the next batch
        self.offs = offs.astype(np.int64)
        self.count += gained - lost
        return gained, lost, ms


def pick(runs, j):
    return (round(min(r[j] for r in runs), 3), round(max(r[j] for r in runs) - min(r[j] for r in runs), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--batches", default="1,100,10000")
    ap.add_argument("--queries", default="triangle,c4")
    ap.add_argument("--kinds", default="relabel,remove,add")
    ap.add_argument("--l", type=int, default=2)
    ap.add_argument("--hub", action="store_true")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=10_000_000)
    a = ap.parse_args()
    graphs = []
    if "gnm" in a.graphs:
        graphs.append((f"gnm_{a.n}_{a.m}", lambda: synth.gnm_graph(a.n, a.m)))
    if "powerlaw" in a.graphs:
        graphs.append((f"powerlaw_{a.n}_{a.m}", lambda: synth.powerlaw_graph(a.n, a.m)))
    qdir = a.out or os.path.join(ROOT, "profile_out", "online_standing_updates")
    os.makedirs(qdir, exist_ok=True)
    sizes = [int(x) for x in a.batches.split(",")]
    cheaper = {}
    for gname, make in graphs:
        g = make()
        n_labels = int(g["labels"].max()) + 1
        rng = np.random.default_rng(2026)
        for qname, k in (("triangle", 3), ("c4", 4)):
            qp = os.path.join(qdir, f"{gname}_{qname}.graph")
            write_cycle(qp, g["labels"][find_cycle(g, k, rng)])
            if qname not in a.queries:
                continue
            plan = binding.host_query_plan_exact(qp, 2, a.l)
            for kind in a.kinds.split(","):
                # three engines on the graph as made: every kind starts from the same graph
                engines = []
                for _ in range(3):
                    eng = binding.Engine(0)
                    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
                    eng.set_label_table(binding.host_label_table(n_labels, 2))
                    eng.vde(want=False)
                    engines.append(eng)
                ea, eb, ec = engines
                sq = ea.standing_open(qp, l=a.l)
                comp = Composed(eb, g, qp, plan)
                sr = ec.standing_open(qp, l=a.l)
                brng = np.random.default_rng(2027)
                labels = g["labels"].astype(np.int64).copy()  # of the graph as the engines hold it (relabel batches only)
                n = g["n"]
                hub = int(np.argmax(np.diff(g["offsets"].astype(np.int64))))
                for size in sizes:
                    print(f"{gname} {qname} l={a.l} {kind} batch={size}", file=sys.stderr, flush=True)
                    runs = {"a": [], "b": [], "c": []}
                    ok, touched = True, 0
                    R = None
                    for i in range(a.runs + 1 + (kind == "relabel" and (a.runs + 1) % 2)):  # the first batch is the warm-up
                        if kind == "relabel":
                            if i % 2 == 0:  # forwards, then back
                                R = np.sort(brng.choice(n, size, replace=False))
                                if a.hub and hub not in R:
                                    R[0] = hub
                                    R = np.unique(R)
                                new = (labels[R] + 1) % n_labels
                            else:
                                new = (labels[R] + n_labels - 1) % n_labels
                            labels[R] = new
                            if i == 0:
                                touched = len(with_neighbours(comp.offs, comp.nbrs, R))
                            t0 = time.perf_counter()
                            ms_a = ea.standing_set_labels(R, new, timing=True)
                            wall_a = (time.perf_counter() - t0) * 1e3
                            t0 = time.perf_counter()
                            created, destroyed, ms_b = comp.relabel(R, new)
                            wall_b = (time.perf_counter() - t0) * 1e3
                            t0 = time.perf_counter()
                            ec.set_vertex_labels(R, new)
                        else:
                            rem = np.sort(brng.choice(n, size, replace=False)) if kind == "remove" else np.zeros(0, np.int64)
                            add = brng.integers(0, n_labels, size) if kind == "add" else np.zeros(0, np.int64)
                            if i == 0:
                                touched = len(with_neighbours(comp.offs, comp.nbrs, rem)) + len(add)
                            t0 = time.perf_counter()
                            n2, ms_a = ea.standing_apply_vertices(rem, add, timing=True)
                            wall_a = (time.perf_counter() - t0) * 1e3
                            t0 = time.perf_counter()
                            created, destroyed, ms_b = comp.vertices(rem, add)
                            wall_b = (time.perf_counter() - t0) * 1e3
                            t0 = time.perf_counter()
                            ec.apply_vertices(rem, add)
                            n = n2
                        ec.vde(want=False)
                        count_c, ms_c = sr.refresh(timing=True)
                        wall_c = (time.perf_counter() - t0) * 1e3
                        res = sq.result()
                        ok = ok and res[:3] == (comp.count, created, destroyed) and res[0] == count_c
                        if i:
                            runs["a"].append((wall_a, ms_a))
                            runs["b"].append((wall_b, ms_b))
                            runs["c"].append((wall_c, ms_c))
                    line = dict(graph=gname, query=qname, l=a.l, kind=kind, hub=bool(a.hub and kind == "relabel"), batch=size, touched=touched,
                                count=res[0], created=res[1], destroyed=res[2], counts_ok=bool(ok),
                                standing_wall_ms=pick(runs["a"], 0), standing_device_ms=pick(runs["a"], 1),
                                composed_wall_ms=pick(runs["b"], 0), composed_device_ms=pick(runs["b"], 1),
                                refresh_wall_ms=pick(runs["c"], 0), refresh_device_ms=pick(runs["c"], 1))
                    print(json.dumps(line), flush=True)
                    key = f"{gname} {qname} {kind}"
                    if cheaper.get(key) is None:
                        cheaper[key] = size if line["refresh_wall_ms"][0] < line["standing_wall_ms"][0] else None
                sq.close()
                sr.close()
                del comp
                for eng in engines:
                    eng.close()
    print(json.dumps(dict(refresh_cheaper_from_batch=cheaper, hub=bool(a.hub), l=a.l)), flush=True)


if __name__ == "__main__":
    main()
