#!/usr/bin/env python3
"""What applying an edge batch to the resident graph costs ("Updating the resident graph"):
gnnpe_csr_apply_edges beside the only alternative, gnnpe_load_csr of the finished host arrays of G' (the host-side rebuild of
those arrays is not even charged to it).

Graphs: powerlaw_graph(20000, 80000, max_degree=600) of section 3.7 and gnm_graph(1_000_000, 10_000_000) of the README figures.
Batches of 1, 100, 10 000 and 1 000 000 edges (sizes the graph does not allow are skipped), half non-edge inserts and half existing
deletes, seed 1.  Per graph one child process under its own time limit; inside it the warm runs alternate: apply (I, D), load_csr of
G', load_csr of G, ... (--rounds rounds, the first dropped).  Per case one JSON line: device_ms and wall ms of the apply, wall ms
of the load, each the best of the warm runs with their spread; the bytes the merge kernel has to move, 4 * (entries + entries');
and the shares of device_ms spent before the wait (keys to merge), in the wait (the counters' read-back and the host's decision)
and in the rebuild of the derived structure (device events right around the owned copy, finish_rows and the neighbour labels).
The shares come from a pass of their own on a second context created with GNNPE_DEBUG=1, which makes the library print them;
the timed runs are made without it.
--rocprof GRAPH:SIZE runs that one case under `rocprofv3 --kernel-trace --stats` in a run of its own and prints k_csr_merge's row
of the kernel statistics with its bytes/s (HBM peak of the MI355X: 8 TB/s).
Usage: python scripts/online_apply_edges_measure.py [--graphs powerlaw,gnm] [--rounds 4] [--time-limit 400] [--rocprof gnm:10000]"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 100, 10_000, 1_000_000)
HBM_PEAK = 8.0e12  # bytes/s


def make_graph(name):
    from gnnpe_amd import synth
    g = synth.powerlaw_graph(20000, 80000, max_degree=600) if name == "powerlaw" else synth.gnm_graph(1_000_000, 10_000_000)
    return dict(n=g["n"], offsets=g["offsets"], nbrs=g["nbrs"], labels=np.zeros(g["n"], np.uint32))


def und_edges(g):
    src = np.repeat(np.arange(g["n"], dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    dst = g["nbrs"].astype(np.int64)
    keep = src < dst
    return src[keep] * g["n"] + dst[keep]  # ascending codes


def batch(g, codes, k, rng):
    """(inserts, deletes): (k + 1) // 2 non-edges and k // 2 edges, as (x, y) arrays"""
    n, ni, nd = g["n"], (k + 1) // 2, k // 2
    ins = np.zeros(0, np.int64)
    while len(ins) < ni:
        x, y = rng.integers(0, n, 2 * ni + 64), rng.integers(0, n, 2 * ni + 64)
        c = np.minimum(x, y) * n + np.maximum(x, y)
        c = c[(x != y) & ~np.isin(c, codes)]
        ins = np.unique(np.concatenate([ins, c]))
    ins = rng.permutation(ins)[:ni]
    dele = codes[rng.choice(len(codes), nd, replace=False)]
    return np.stack([ins // n, ins % n], axis=1), np.stack([dele // n, dele % n], axis=1)


def updated(g, codes, ins, dele):
    from gnnpe_amd import synth
    n = g["n"]
    keep = np.union1d(np.setdiff1d(codes, dele[:, 0] * n + dele[:, 1]), ins[:, 0] * n + ins[:, 1])
    offs, nbrs = synth._csr_from_edges(n, keep // n, keep % n)
    return dict(g, offsets=offs, nbrs=nbrs)


def child(name, a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding
    g = make_graph(name)
    codes = und_edges(g)
    os.environ.pop("GNNPE_DEBUG", None)
    eng = binding.Engine(0)  # the timed context
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    # the context of the share pass: GNNPE_DEBUG is read when a context is created; its [apply_edges] lines go to a file
    log = tempfile.NamedTemporaryFile(prefix="apply_edges_", suffix=".log", dir=a.out, delete=False)
    os.dup2(log.fileno(), 2)
    os.environ["GNNPE_DEBUG"] = "1"
    dbg = binding.Engine(0)
    os.environ.pop("GNNPE_DEBUG")
    dbg.load_csr(g["offsets"], g["nbrs"], g["labels"])
    rng = np.random.default_rng(1)
    for k in (int(s) for s in a.sizes.split(",")):
        if k // 2 > len(codes) // 2:
            print(json.dumps(dict(graph=name, batch=k, skipped="the graph has %d edges" % len(codes))), flush=True)
            continue
        ins, dele = batch(g, codes, k, rng)
        g2 = updated(g, codes, ins, dele)
        dev, wall, load, parts = [], [], [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            entries, ms = eng.apply_edges(ins, dele, timing=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ms)
            assert entries == len(g2["nbrs"])
            t0 = time.perf_counter()
            eng.load_csr(g2["offsets"], g2["nbrs"], g2["labels"])
            eng.sync()
            load.append((time.perf_counter() - t0) * 1e3)
            eng.load_csr(g["offsets"], g["nbrs"], g["labels"])  # back to G for the next round
        offs, nbrs = eng.download_csr()
        assert np.array_equal(offs, g["offsets"]) and np.array_equal(nbrs, g["nbrs"])
        for _ in range(a.rounds):  # the share pass
            mark = os.path.getsize(log.name)
            dbg.apply_edges(ins, dele)
            line = [ln for ln in open(log.name).read()[mark:].splitlines() if ln.startswith("[apply_edges]")][-1]
            f = {k: float(v) for k, v in (p.split("=") for p in line.split()[1:]) if k.endswith("_ms")}
            parts.append([f[k] / max(f["device_ms"], 1e-9) for k in ("build_ms", "wait_ms", "rebuild_ms")])
            dbg.apply_edges(dele, ins)  # back to G
        med = np.median(np.array(parts[1:]), axis=0)
        stat = lambda v: dict(best=round(min(v[1:]), 4), spread=round(max(v[1:]) - min(v[1:]), 4), first=round(v[0], 4))
        row = dict(graph=name, n=g["n"], entries=len(g["nbrs"]), batch=k, inserts=len(ins), deletes=len(dele), device_ms=stat(dev),
                   apply_wall_ms=stat(wall), load_csr_wall_ms=stat(load), build_share=round(float(med[0]), 3),
                   wait_share=round(float(med[1]), 3), rebuild_share=round(float(med[2]), 3),
                   merge_bytes=4 * (len(g["nbrs"]) + len(g2["nbrs"])))
        row["apply_beats_load"] = bool(max(wall[1:]) < min(load[1:]))  # by more than the spread of the two
        print(json.dumps(row), flush=True)
    eng.close()
    dbg.close()


def rocprof(case, a):
    name, size = case.split(":")
    out = os.path.join(a.out, f"rocprof_{name}_{size}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--child", name,
           "--sizes", size, "--rounds", str(a.rounds), "--out", a.out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.time_limit)
    rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not rows or "merge_bytes" not in rows[0]:
        print(json.dumps(dict(case=case, failed=True, returncode=p.returncode, tail=p.stderr[-400:])), flush=True)
        return 1
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_csr_merge" in (r.get("Name") or ""):
                avg_ns = next((float(v) for k, v in r.items() if re.fullmatch(r"Average(Ns| \(ns\))?", k or "", re.I)), None)
                row = dict(case=case, kernel="k_csr_merge", stats=r, merge_bytes=rows[0]["merge_bytes"])
                if avg_ns:
                    row.update(bytes_per_s=round(rows[0]["merge_bytes"] / (avg_ns * 1e-9), 0),
                               of_hbm_peak=round(rows[0]["merge_bytes"] / (avg_ns * 1e-9) / HBM_PEAK, 4))
                print(json.dumps(row), flush=True)
                return 0
    print(json.dumps(dict(case=case, failed=True, no_kernel_row_in=sorted(glob.glob(os.path.join(out, "**", "*"), recursive=True))[:40])),
          flush=True)
    return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="powerlaw,gnm")
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_apply_edges"))
    ap.add_argument("--time-limit", type=float, default=400.0)
    ap.add_argument("--rocprof", default=None, help="GRAPH:SIZE, one case under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        try:
            return child(a.child, a)
        except Exception:  # (the child's stderr is the library's log)
            import traceback
            print(json.dumps(dict(graph=a.child, failed=True, error=traceback.format_exc()[-600:])), flush=True)
            return 1
    if a.rocprof:
        return rocprof(a.rocprof, a)
    for name in (k for k in a.graphs.split(",") if k):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--sizes", a.sizes, "--rounds", str(a.rounds), "--out", a.out]
        p = subprocess.Popen(cmd)  # a fresh process per graph: its rows go straight to this stdout
        try:
            rc = p.wait(timeout=a.time_limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            print(json.dumps(dict(graph=name, timed_out=True, time_limit_s=a.time_limit)), flush=True)
            return 1  # nothing more is started after a run that had to be ended
        if rc != 0:
            print(json.dumps(dict(graph=name, failed=True, returncode=rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
