#!/usr/bin/env python3
"""The count tables of a standing exact query measured: what one edge batch costs through
gnnpe_standing_apply_edges with V, with E and with both kept (a), against the same loop composed by hand from the public calls
that were there before the handle kept tables (b), and gnnpe_table_fold on its own.

Setup as scripts/online_standing_measure.py: G(n,m) 1M / 10M and the power-law graph of the same size, 64 labels, e = 2, l = 2; a
triangle and a 4-cycle cut from the graph, mode 0 and induced; batches of 1, 100 and 10 000 edges, half deletions, half insertions
(a batch of 1: an insertion), a batch alternating with its inverse.

(a) and (b) run in one process on two engines that hold the same graph and ALTERNATE batch by batch, warm; per configuration the
best of three with the spread (max - min), wall clock around the whole batch and the device ms the calls report:
  (a) Engine.standing_apply_edges(insert, delete), rows_cap 0, changes_cap 0
  (b) per apply: filter_support_delta(-1); per kept table refine_sets_delta_{vertex,edge}_counts(accum=T, sign=-1) on the host
      bitmap (and the _nonedges_ forms for an induced query); apply_edges_map; vde; carry_entries of T for E;
      filter_support_delta(+1); support_bitmap; the count calls with sign=+1.  created / destroyed are the count calls' answers.
The counts of (a) and (b) are compared after every batch, and at the end of a configuration V cell by cell and every row sum of E
(tables_ok).  One JSON line per configuration on stdout; with --fold one line per fold measurement.
Usage: python scripts/online_standing_counts_measure.py [--graphs gnm,powerlaw] [--batches 1,100,10000] [--kept V,E,VE]
       [--queries triangle,c4] [--fold] [--out DIR]"""
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
from online_filter_support_measure import draw_batch  # noqa: E402
from online_standing_measure import find_cycle, write_cycle  # noqa: E402

FULL = 2 ** 64 - 1


class Composed:
    """the hand-written loop on an engine of its own: S, the host bitmap and the caller's tables as torch tensors"""

    def __init__(self, eng, qp, plan, induced, kept):
        import torch
        self.torch, self.eng, self.qp, self.plan, self.induced = torch, eng, qp, plan, induced
        self.nq = int(plan["n_vertices"])
        self.table, _ = eng.filter_support_exact(plan)
        self.bm = eng.support_bitmap(self.table, self.nq)[0]
        self.count = eng.refine_sets(qp, self.bm, limit=FULL, induced=induced)[0]
        self.V = self.E = None
        if "V" in kept:
            v = eng.refine_sets_vertex_counts(qp, self.bm, induced=induced)[2]
            self.V = torch.from_numpy(v.view(np.int64)).cuda()
        if "E" in kept:
            e = eng.refine_sets_edge_counts(qp, self.bm, induced=induced)[2]
            self.E = torch.from_numpy(np.ascontiguousarray(e).view(np.int64)).cuda()
        torch.cuda.synchronize()

    def counts(self, edges, nonedges, sign):
        """sign * the tables of the matches through `edges` (and, induced, on `nonedges`) into the kept tables: (matches, ms)"""
        eng, found, ms = self.eng, 0, 0.0
        for T, vertex in ((self.V, True), (self.E, False)):
            if T is None:
                continue
            got = 0
            if len(edges):
                fn = eng.refine_sets_delta_vertex_counts if vertex else eng.refine_sets_delta_edge_counts
                r = fn(self.qp, self.bm, edges, induced=self.induced, accum=T.data_ptr(), sign=sign)
                got, ms = got + r[0], ms + r[3]
            if self.induced and len(nonedges):
                fn = eng.refine_sets_delta_nonedges_vertex_counts if vertex else eng.refine_sets_delta_nonedges_edge_counts
                r = fn(self.qp, self.bm, nonedges, accum=T.data_ptr(), sign=sign)
                got, ms = got + r[0], ms + r[3]
            found = got
        return found, ms

    def step(self, ins, dele):
        eng, torch = self.eng, self.torch
        T = np.unique(np.array(list(ins) + list(dele), np.int64))
        ms = eng.filter_support_delta(self.plan, T, -1, self.table)
        destroyed, m = self.counts(dele, ins, -1)
        ms += m
        if self.E is not None:
            before, after, _, m = eng.apply_edges_map(insert=ins, delete=dele, timing=True)
            ms += m
            dst = torch.empty((self.E.shape[0], after), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ms += eng.carry_entries(self.E, dst, self.E.shape[0], timing=True)
            self.E = dst
        else:
            ms += eng.apply_edges(insert=ins, delete=dele, timing=True)[1]
        eng.vde(want=False)
        ms += eng.filter_support_delta(self.plan, T, +1, self.table)
        self.bm, m = eng.support_bitmap(self.table, self.nq)
        ms += m
        created, m = self.counts(ins, dele, +1)
        return created, destroyed, ms + m

    def batch(self, ins, dele):
        if self.induced and len(ins) and len(dele):
            c1, d1, m1 = self.step([], dele)
            c2, d2, m2 = self.step(ins, [])
            c, d, m = c1 + c2, d1 + d2, m1 + m2
        else:
            c, d, m = self.step(ins, dele)
        self.count += c - d
        return c, d, m


def measure_fold(eng, shapes):
    """gnnpe_table_fold alone: device ms (best of three, spread) at `cells` cells with 0, 100 and 10^6 nonzero cells, next to the
    bytes it has to move: 8 per cell for pass 1 over D; pass 2 reads 8 per tile and, in a tile with a nonzero cell, 16 per cell
    and writes 8 per cell of D; per nonzero cell 8 of T written and a 16-byte pair"""
    import torch
    for what, cells in shapes:
        for nz in (0, 100, 1_000_000):
            t = torch.zeros(cells, dtype=torch.int64, device="cuda:0")
            d = torch.zeros(cells, dtype=torch.int64, device="cuda:0")
            cc, cd = torch.zeros(max(nz, 1), dtype=torch.int64, device="cuda:0"), torch.zeros(max(nz, 1), dtype=torch.int64, device="cuda:0")
            idx = torch.from_numpy(np.random.default_rng(nz).choice(cells, nz, replace=False)).cuda() if nz else None
            runs = []
            for i in range(4):
                if nz:
                    d[idx] = 1
                torch.cuda.synchronize()
                n, ms = eng.table_fold(t, d, cells, cc, cd, nz, timing=True)
                assert n == nz
                if i:
                    runs.append(ms)
            tiles = (cells + 2047) // 2048
            dirty = min(tiles, nz)  # at most
            print(json.dumps(dict(fold=what, cells=cells, nonzero=nz, device_ms=(round(min(runs), 4), round(max(runs) - min(runs), 4)),
                                  bytes_pass1=cells * 8 + tiles * 8, bytes_pass2_at_most=tiles * 16 + dirty * 2048 * 24 + nz * 24)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--batches", default="1,100,10000")
    ap.add_argument("--kept", default="V,E,VE")
    ap.add_argument("--queries", default="triangle,c4")
    ap.add_argument("--fold", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=10_000_000)
    a = ap.parse_args()
    graphs = []
    if "gnm" in a.graphs:
        graphs.append((f"gnm_{a.n}_{a.m}", lambda: synth.gnm_graph(a.n, a.m)))
    if "powerlaw" in a.graphs:
        graphs.append((f"powerlaw_{a.n}_{a.m}", lambda: synth.powerlaw_graph(a.n, a.m)))
    qdir = a.out or os.path.join(ROOT, "profile_out", "online_standing_counts")
    os.makedirs(qdir, exist_ok=True)
    if a.fold:
        eng = binding.Engine(0)
        measure_fold(eng, (("V triangle nq x n", 3 * a.n), ("V c4 nq x n", 4 * a.n), ("E triangle nqe x entries", 3 * 2 * a.m),
                           ("E c4 nqe x entries", 4 * 2 * a.m)))
        eng.close()
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
            if qname not in a.queries:
                continue
            plan = binding.host_query_plan_exact(qp, 2, 2)
            for induced in (False, True):
                for kept in a.kept.split(","):
                    sq = ea.standing_open(qp, l=2, induced=induced)
                    t0 = time.perf_counter()
                    keep_ms = sq.keep_counts(vertex="V" in kept, edge="E" in kept, changes_cap=0, timing=True)
                    keep_wall = (time.perf_counter() - t0) * 1e3
                    comp = Composed(eb, qp, plan, induced, kept)
                    for size, (ins, dele) in batches.items():
                        print(f"{gname} {qname} induced={induced} kept={kept} batch={size}", file=sys.stderr, flush=True)
                        runs_a, runs_b, ok, changes = [], [], True, {}
                        for i in range(8):  # forwards, backwards, ...: the first pair is the warm-up
                            bi, bd = (ins, dele) if i % 2 == 0 else (dele, ins)
                            t0 = time.perf_counter()
                            ms_a = ea.standing_apply_edges(insert=bi, delete=bd, timing=True)
                            wall_a = (time.perf_counter() - t0) * 1e3
                            t0 = time.perf_counter()
                            created, destroyed, ms_b = comp.batch(bi, bd)
                            wall_b = (time.perf_counter() - t0) * 1e3
                            res = sq.result()
                            ok = ok and res[:3] == (comp.count, created, destroyed)
                            if i == 2:
                                changes = {w: sq.n_changes(w) for w, c in (("vertex", "V"), ("edge", "E")) if c in kept}
                            if i >= 2:
                                runs_a.append((wall_a, ms_a))
                                runs_b.append((wall_b, ms_b))
                        pick = lambda runs, j: (round(min(r[j] for r in runs), 3), round(max(r[j] for r in runs) - min(r[j] for r in runs), 3))
                        print(json.dumps(dict(graph=gname, query=qname, induced=induced, kept=kept, batch=size,
                                              applies=2 if induced and len(ins) and len(dele) else 1, count=res[0], created=res[1],
                                              destroyed=res[2], changes=changes, counts_ok=ok, keep_counts_ms=(round(keep_wall, 3), round(keep_ms, 3)),
                                              standing_wall_ms=pick(runs_a, 0), standing_device_ms=pick(runs_a, 1),
                                              composed_wall_ms=pick(runs_b, 0), composed_device_ms=pick(runs_b, 1))), flush=True)
                    tables_ok = True
                    if comp.V is not None:
                        tables_ok = tables_ok and np.array_equal(sq.counts("vertex"), comp.V.cpu().numpy().view(np.uint64))
                    if comp.E is not None:
                        tables_ok = tables_ok and bool((comp.E.sum(dim=1).cpu().numpy().view(np.uint64) == np.uint64(sq.count)).all())
                    print(json.dumps(dict(graph=gname, query=qname, induced=induced, kept=kept, tables_ok=bool(tables_ok))), flush=True)
                    sq.close()
                    del comp
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    main()
