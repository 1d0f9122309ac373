#!/usr/bin/env python3
"""What the count tables of the matches through a set of data vertices cost ("Count tables of the matches
through a set of data vertices"; profiles/online_delta_vertices_counts.txt).

1. gnnpe_refine_sets_delta_vertices_vertex_counts / _edge_counts beside two things the parent commit has, for the same query on the
   same graph and bitmap: the emulation, gnnpe_refine_sets_delta_vertex_counts / _edge_counts over E(S) (every edge with an endpoint
   in S), whose answers and tables must be equal (asserted), and the full recount, gnnpe_refine_sets_vertex_counts / _edge_counts.
   Graph, queries and S are those of scripts/online_delta_vertices_measure.py: powerlaw_graph(n, m, max_degree=600) (default
   20 000 / 80 000) with every label 0; wedge, triangle, C4, diamond, K4, mode 0, limit 2^64 - 1; S = the first 1, 100 and 10 000
   vertices of a shuffle with seed 1, and the vertex with the longest row alone ("hub").
   Per query one JSON line: per S and per table ("v", "e") the device ms of the vertex form, of the emulation and of the recount --
   the best of the warm runs with their spread (--rounds runs, the first dropped; the calls alternate in one process) -- and the
   ratios.
2. The relabel loop on the same graph, per query, S = the 100 and the 10 000 vertices: T holds V(G, C) in caller memory;
   T -= VV(G, C, S); gnnpe_set_vertex_labels(S -> label 1); T += VV(G', C', S) -- device ms of the three steps summed -- beside the
   recount gnnpe_refine_sets_vertex_counts on G'; then the same loop back to label 0, where the matches return.  T must equal the
   recount after both (asserted); the same for the edge table.  C and C' are the label/degree bitmaps of the two graphs.

Every query runs in a child process of its own under a time limit of its own (--time-limit seconds); a child that passes it is
ended, a "timed_out" row follows and nothing is run again: the chain stops at the first failure.
Usage: python scripts/online_delta_vertices_counts_measure.py [--n 20000] [--m 80000] [--rounds 4] [--time-limit 300]
       [--queries wedge,triangle,...] [--no-loop]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from online_delta_measure import SHAPES, ld_bitmap, write_query  # noqa: E402
from online_delta_vertices_measure import SIZES, run_child  # noqa: E402

LOOP_SIZES = (100, 10000)


def best(ms):
    return round(min(ms), 3), round(max(ms) - min(ms), 3)


def child(name, a):
    import torch
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    g = synth.powerlaw_graph(a.n, a.m, max_degree=600)
    g = dict(g, labels=np.zeros(g["n"], np.uint32))
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    nq, edges = SHAPES[name]
    qp = os.path.join(a.out, f"{name}.graph")
    write_query(qp, nq, edges, [0] * nq)
    q = binding.host_load_graph(qp)
    bm = ld_bitmap(g, q)
    deg = np.diff(g["offsets"].astype(np.int64))
    src = np.repeat(np.arange(g["n"], dtype=np.int64), deg)
    E = np.stack([src, g["nbrs"].astype(np.int64)], axis=1)
    E = E[E[:, 0] < E[:, 1]]
    shuffled = np.random.default_rng(1).permutation(g["n"])
    sets = [(str(k), shuffled[:k]) for k in SIZES if k <= g["n"]] + [("hub", np.array([int(np.argmax(deg))]))]
    at = {key: E[np.isin(E[:, 0], S) | np.isin(E[:, 1], S)] for key, S in sets}
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, nq=nq, nqe=len(edges), max_degree=int(deg.max()))
    calls = dict(v=(eng.refine_sets_delta_vertices_vertex_counts, eng.refine_sets_delta_vertex_counts, eng.refine_sets_vertex_counts),
                 e=(eng.refine_sets_delta_vertices_edge_counts, eng.refine_sets_delta_edge_counts, eng.refine_sets_edge_counts))
    for t, (new, emu, full) in calls.items():
        runs = {key: ([], []) for key, _ in sets}
        recount = []
        for _ in range(a.rounds):  # alternately: the vertex form, then the emulation, for every S; then the recount
            for key, S in sets:
                ans, done, table, ms = new(qp, bm, S)
                ans2, done2, table2, ms2 = emu(qp, bm, at[key])
                assert done and done2 and ans == ans2 and np.array_equal(table, table2), (t, key, ans, ans2)
                runs[key][0].append(ms)
                runs[key][1].append(ms2)
                row.setdefault(f"S_{key}", dict(size=len(S), edges_at=len(at[key]), delta_v=ans))
            total, done, _, ms = full(qp, bm)
            assert done
            recount.append(ms)
        r_ms, r_spread = best(recount[1:])
        row[f"recount_{t}"] = dict(matches=total, ms=r_ms, spread_ms=r_spread)
        for key, _ in sets:
            (v_ms, v_spread), (e_ms, e_spread) = best(runs[key][0][1:]), best(runs[key][1][1:])
            row[f"S_{key}"][t] = dict(vertices_ms=v_ms, vertices_spread_ms=v_spread, emulation_ms=e_ms, emulation_spread_ms=e_spread,
                                      vertices_over_emulation=round(v_ms / max(e_ms, 1e-6), 3),
                                      vertices_over_recount=round(v_ms / max(r_ms, 1e-6), 4))
    print(json.dumps(row), flush=True)
    if a.no_loop:
        eng.close()
        return

    # the relabel loop: S to label 1 (its matches go), then back to label 0 (they return)
    def dev(arr):
        t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        return t

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint64)

    loop = dict(graph=row["graph"], query=name, relabel_loop=True)
    for k in (k for k in LOOP_SIZES if k <= g["n"]):
        S = shuffled[:k]
        out = {}
        for t, (new, _, full) in calls.items():
            labels = g["labels"].copy()
            T = dev(full(qp, bm)[2])
            steps = []
            for lab in (1, 0, 1, 0)[:max(2, 2 * (a.rounds // 2))]:
                cur = ld_bitmap(dict(g, labels=labels), q)
                gone, done, _, ms_minus = new(qp, cur, S, accum=T.data_ptr(), sign=-1)
                assert done
                ms_set = eng.set_vertex_labels(S, np.full(k, lab, np.uint32), timing=True)
                labels[S] = lab
                nxt = ld_bitmap(dict(g, labels=labels), q)
                came, done, _, ms_plus = new(qp, nxt, S, accum=T.data_ptr(), sign=1)
                assert done
                total, done, want, ms_full = full(qp, nxt)
                assert done and np.array_equal(host(T), want), (t, k, lab)
                steps.append(dict(to_label=lab, lost=gone, gained=came, matches_after=total, loop_ms=round(ms_minus + ms_set + ms_plus, 3),
                                  minus_ms=round(ms_minus, 3), set_labels_ms=round(ms_set, 4), plus_ms=round(ms_plus, 3),
                                  recount_ms=round(ms_full, 3)))
            out[t] = steps[2:] if len(steps) > 2 else steps  # the first pass warms the kernels
        loop[f"S_{k}"] = out
    eng.close()
    print(json.dumps(loop), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--queries", default="wedge,triangle,C4,diamond,K4")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_delta_vertices_counts"))
    ap.add_argument("--time-limit", type=float, default=300.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    common = ["--n", str(a.n), "--m", str(a.m), "--rounds", str(a.rounds), "--out", a.out] + (["--no-loop"] if a.no_loop else [])
    for name in (k for k in a.queries.split(",") if k):
        if run_child([sys.executable, os.path.abspath(__file__), "--child", name] + common, name, a.time_limit):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
