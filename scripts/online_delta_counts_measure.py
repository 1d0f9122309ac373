#!/usr/bin/env python3
"""What the count tables of the matches through a set of data edges cost ("Count tables of the matches
through a set of data edges"): gnnpe_refine_sets_delta_vertex_counts / _edge_counts for F of 1, 100 and 10 000 random edges and
for F = E(G), beside what the same search costs without a table and beside what maintaining a table costs without them.

Graph, bitmap, queries and method are those of scripts/online_delta_measure.py: powerlaw_graph(n, m, max_degree=600) with every
label 0, the label/degree bitmap, mode 0, limit 2^64 - 1; the calls alternate in one process, --rounds runs, the first dropped, the
best of the warm runs with their spread.  C5 runs |F| = 1 only.  Per query one JSON line; per F, device ms of
  (a) plain       gnnpe_refine_sets_delta, count only: the floor, the search is the same;
  (b) v_own/e_own the two new calls with the context-owned table (zeroed inside the timed span);
  (c) v_acc/e_acc the same calls accumulating into a caller's table (no zeroing; sign +1, then -1 outside the timing restores it);
and per query
  (d) v_full/e_full  gnnpe_refine_sets_vertex_counts / _edge_counts of the whole graph: what the loop costs today;
  (e) rows_wall_ms   today's other route, once per F, wall time: the delta rows with matches_cap = Delta to the host and a numpy
                     tally of the vertex table (np.bincount); "not feasible" where the rows pass --rows-limit bytes.
The atomics on the table per find come from the flush_adds of the GNNPE_DEBUG line (the child keeps its stderr in a file): for the
vertex table 1 + flush_adds / finds, for the edge table deg_Q(last position) + flush_adds / finds, the last position being each
launch's own, so the figure reported for the edge table is flush_adds / finds alone.
The tables of (b) are checked in the run: every row sums to Delta, and for F = E(G) they equal the tables of (d).
Every query runs in a child process under a time limit of its own; a child that passes it is ended and nothing is run again.
Usage: python scripts/online_delta_counts_measure.py [--n 20000] [--m 80000] [--rounds 4] [--time-limit 400] [--queries ...]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from online_delta_measure import SHAPES, SIZES, ld_bitmap, write_query  # noqa: E402


def best(ms):
    return dict(ms=round(min(ms[1:]), 3), spread_ms=round(max(ms[1:]) - min(ms[1:]), 3), first_ms=round(ms[0], 3))


def child(name, a):
    err_path = os.path.join(a.out, f"{name}.stderr")
    err = open(err_path, "w")
    os.dup2(err.fileno(), 2)
    os.environ["GNNPE_DEBUG"] = "1"  # read when the context is created
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
    nq, edges = SHAPES[name]
    qp = os.path.join(a.out, f"{name}.graph")
    write_query(qp, nq, edges, [0] * nq)
    bm = ld_bitmap(g, binding.host_load_graph(qp))
    src = np.repeat(np.arange(g["n"], dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    E = np.stack([src, g["nbrs"].astype(np.int64)], axis=1)
    E = E[E[:, 0] < E[:, 1]]
    shuffled = E[np.random.default_rng(1).permutation(len(E))]
    sets = [(str(k), shuffled[:k]) for k in SIZES if k < len(E)] + [("all", E)]
    if name == "C5":
        sets = sets[:1]
    nqe, entries = len(edges), len(g["nbrs"])
    acc_v = torch.zeros((nq, g["n"]), dtype=torch.int64, device="cuda:0")
    acc_e = torch.zeros((nqe, entries), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    row = dict(graph=f"powerlaw_{a.n}_{a.m}", query=name, edges=len(E), launches=nqe, table_bytes=dict(vertex=nq * g["n"] * 8, edge=nqe * entries * 8))
    full = dict(v_full=[], e_full=[])
    runs = {key: dict(plain=[], v_own=[], e_own=[], v_acc=[], e_acc=[]) for key, _ in sets}
    deltas = {}
    for _ in range(a.rounds):  # alternately: the full tables, then every F in every form
        fv = eng.refine_sets_vertex_counts(qp, bm)
        fe = eng.refine_sets_edge_counts(qp, bm)
        assert fv[1] and fe[1] and fv[0] == fe[0]
        full["v_full"].append(fv[3])
        full["e_full"].append(fe[3])
        for key, F in sets:
            r = runs[key]
            d, _, ms = eng.refine_sets_delta(qp, bm, F)
            r["plain"].append(ms)
            dv = eng.refine_sets_delta_vertex_counts(qp, bm, F)
            de = eng.refine_sets_delta_edge_counts(qp, bm, F)
            assert dv[1] and de[1] and dv[0] == de[0] == d and (dv[2].sum(axis=1) == d).all() and (de[2].sum(axis=1) == d).all()
            if key == "all":
                assert d == fv[0] and np.array_equal(dv[2], fv[2]) and np.array_equal(de[2], fe[2])
            r["v_own"].append(dv[3])
            r["e_own"].append(de[3])
            for kind, fn, acc in (("v_acc", eng.refine_sets_delta_vertex_counts, acc_v), ("e_acc", eng.refine_sets_delta_edge_counts, acc_e)):
                got = fn(qp, bm, F, accum=acc.data_ptr(), sign=1)
                assert got[:2] == (d, True)
                r[kind].append(got[3])
                fn(qp, bm, F, accum=acc.data_ptr(), sign=-1)
            deltas[key] = d
    assert not acc_v.any().item() and not acc_e.any().item()  # +1 and -1 cancelled
    row["answers"] = fv[0]
    row["v_full"], row["e_full"] = best(full["v_full"]), best(full["e_full"])
    err.flush()
    said = [ln for ln in open(err_path) if re.match(r"\[refine_delta_[ve]count\] finds=", ln)]
    for i, (key, F) in enumerate(sets):
        d = deltas[key]
        out = dict(size=len(F), delta=d, **{k: best(v) for k, v in runs[key].items()})
        # the last round's lines of this F: vertex own, edge own, then the accumulating calls
        per_round = 6 * len(sets)
        mine = said[len(said) - per_round + 6 * i:][:2]
        fl = [int(re.search(r"flush_adds=(\d+)", ln).group(1)) for ln in mine]
        assert all(int(re.search(r"finds=(\d+)", ln).group(1)) == d for ln in mine)
        out["v_atomics_per_find"] = round(1 + fl[0] / max(d, 1), 4)
        out["e_flush_adds_per_find"] = round(fl[1] / max(d, 1), 4)
        for k in ("v_own", "e_own", "v_acc", "e_acc"):
            out[k]["over_plain"] = round(out[k]["ms"] / max(out["plain"]["ms"], 1e-6), 3)
        out["v_own"]["over_full"] = round(out["v_own"]["ms"] / max(row["v_full"]["ms"], 1e-6), 3)
        out["e_own"]["over_full"] = round(out["e_own"]["ms"] / max(row["e_full"]["ms"], 1e-6), 3)
        if d * nq * 4 > a.rows_limit:
            out["rows_wall_ms"] = "not feasible"
            out["rows_bytes"] = d * nq * 4
        else:
            t0 = time.perf_counter()
            got, rows, _ = eng.refine_sets_delta(qp, bm, F, matches_cap=d)
            tally = np.stack([np.bincount(rows[:, u], minlength=g["n"]) for u in range(nq)]) if d else np.zeros((nq, g["n"]), np.int64)
            out["rows_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            assert got == d and (tally.sum(axis=1) == d).all()
        row[f"F_{key}"] = out
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=80000)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--queries", default="wedge,triangle,C4,diamond,K4,C5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_delta_counts"))
    ap.add_argument("--time-limit", type=float, default=400.0)
    ap.add_argument("--rows-limit", type=int, default=1 << 30, help="bytes of delta rows route (e) may bring to the host")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for name in (k for k in a.queries.split(",") if k):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--n", str(a.n), "--m", str(a.m), "--rounds", str(a.rounds),
               "--out", a.out, "--rows-limit", str(a.rows_limit)]
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
