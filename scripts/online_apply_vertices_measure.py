#!/usr/bin/env python3
"""What a vertex batch on the resident graph costs ("Adding and removing vertices").

Graph: gnm_graph(1_000_000, 10_000_000) of the relabel figures, 2 x 10^7 adjacency entries, one label.  Batches: R = 1, 100 and
10 000 random vertices (seed 1); R = the highest-degree vertex alone; A = 1 and 10 000 added vertices.  One child process under a time
limit; per batch, --rounds rounds of apply / reload, the first dropped, best and spread:

  gnnpe_csr_apply_vertices without and with the entry map: device_ms, the rebuild tail's part of it (the [apply_vertices] line the
  library prints under GNNPE_DEBUG=1, read back from the child's own stderr) and the wall clock;
  (a) gnnpe_load_csr of G' (the host form's arrays), wall clock: what a caller did before this call existed;
  (b) for the removals, gnnpe_csr_apply_edges_map deleting the edges at R, device_ms: the emulation that leaves the ids in place.

Writes the rows as JSON lines behind a header with the recorded resource figures of the kernels (gfx950, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks; nothing here reads them from a binary).

Usage: python scripts/online_apply_vertices_measure.py [--out profiles/online_apply_vertices.txt] [--rounds 4] [--time-limit 420]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import online_apply_edges_measure as base  # noqa: E402  (make_graph)

KERNELS = """kernels of csrc/gnnpe_update_vertices.hip (gfx950, -O3; VGPRs / SGPRs / LDS bytes per block / scratch bytes per lane / waves per SIMD)
  k_vert_mark             14 /  32 /    0 / 0 / 8   one wave per removed vertex: the bitmap bit, the row's flags, the mirrored flags
  k_vert_tile_counts      22 /  34 /   16 / 0 / 8   kept entries of every tile of 2048
  k_vert_compact<true>    37 / 106 / 4384 / 0 / 7   the compaction with the entry map, and the new starts of the tile's rows
  k_vert_compact<false>   30 / 106 / 4384 / 0 / 7   ... without the map
  k_vert_map               8 /  22 /    0 / 0 / 8   vertex_map[newid(v)] = v
  k_vert_tail             30 /  40 /    0 / 0 / 8   degrees, labels, presence, the constant tail of the added vertices
  (gnnpe_csr_carry_vertices launches k_carry_entries of csrc/gnnpe_update.hip, unchanged)
not measured: a plain table of new ids (4 n bytes) against the bitmap and its scan (n / 4 bytes); a decoupled look-back against
the two-pass kept-prefix."""


def stat(v):
    return dict(best=round(min(v[1:]), 4), spread=round(max(v[1:]) - min(v[1:]), 4), first=round(v[0], 4))


class DebugLines:
    """the library's GNNPE_DEBUG lines: fd 2 of this process appended to a file, read through a second descriptor"""

    def __init__(self):
        self.path = tempfile.NamedTemporaryFile(delete=False).name
        os.dup2(os.open(self.path, os.O_WRONLY | os.O_APPEND), 2)
        self.f = open(self.path, "rb")

    def new(self, tag):
        return [ln for ln in self.f.read().decode(errors="replace").splitlines() if ln.startswith(tag)]


def child(a):
    os.environ["GNNPE_DEBUG"] = "1"
    dbg = DebugLines()
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding
    g = base.make_graph("gnm")
    n = g["n"]
    o = g["offsets"].astype(np.int64)
    deg = np.diff(o)
    rng = np.random.default_rng(1)
    batches = [(f"R = {k} random", rng.choice(n, k, replace=False), []) for k in (1, 100, 10_000)]
    batches += [(f"R = the highest-degree vertex (degree {int(deg.max())})", [int(np.argmax(deg))], [])]
    batches += [(f"A = {k}", [], np.zeros(k, np.uint32)) for k in (1, 10_000)]
    eng = binding.Engine(0)
    load = lambda x: (eng.load_csr(x["offsets"], x["nbrs"], x["labels"]), eng.sync())
    load(g)
    for name, rem, add in batches:
        rem = np.asarray(rem, np.int64)
        g2, _ = binding.host_apply_vertices(g, rem, add)
        row = dict(batch=name, n_after=g2["n"], entries_before=len(g["nbrs"]), entries_after=len(g2["nbrs"]))
        for key, want_map in (("apply_vertices", False), ("apply_vertices_entry_map", True)):
            dev, wall, tail = [], [], []
            for _ in range(a.rounds):
                dbg.new("[")
                t0 = time.perf_counter()
                out = eng.apply_vertices(rem, add, entry_map=want_map, timing=True)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(out[-1])
                line = dbg.new("[apply_vertices]")[-1]
                tail.append(float(line.split("rebuild_ms=")[1].split()[0]))
                assert (out[0], out[2]) == (g2["n"], len(g2["nbrs"]))
                load(g)
            row[key] = dict(device_ms=stat(dev), rebuild_tail_ms=stat(tail), tail_share=round(min(tail[1:]) / min(dev[1:]), 3), wall_ms=stat(wall))
        wall = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            load(g2)
            wall.append((time.perf_counter() - t0) * 1e3)
            load(g)
        row["a_load_csr_of_G2_wall_ms"] = stat(wall)
        if len(rem):
            src = np.concatenate([np.full(deg[v], v, np.int64) for v in rem])
            dst = np.concatenate([g["nbrs"][o[v]:o[v + 1]].astype(np.int64) for v in rem])
            dele = np.stack([src, dst], axis=1)
            dev = []
            for _ in range(a.rounds):
                out = eng.apply_edges_map(None, dele, timing=True)
                dev.append(out[-1])
                load(g)
            row["b_apply_edges_map_deleting_the_edges_at_R_device_ms"] = stat(dev)
            row["b_edges_deleted"] = int(len(np.unique(np.minimum(src, dst) * n + np.maximum(src, dst))))
        print(json.dumps(row), flush=True)
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_apply_vertices.txt"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--time-limit", type=float, default=420.0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        try:
            return child(a)
        except Exception:
            import traceback
            print(json.dumps(dict(failed=True, error=traceback.format_exc()[-800:])), flush=True)  # (stderr goes to the debug file)
            return 1
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)], stdout=subprocess.PIPE, text=True)
    try:
        rows, _ = p.communicate(timeout=a.time_limit)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        print(json.dumps(dict(timed_out=True, time_limit_s=a.time_limit)), flush=True)
        return 1  # nothing more is started after a run that had to be ended
    print(rows, end="")
    if p.returncode != 0:
        print(json.dumps(dict(failed=True, returncode=p.returncode)), flush=True)
        return 1
    head = ("gnnpe_csr_apply_vertices on gnm_graph(1_000_000, 10_000_000), one MI355X; times in ms; best / spread over the warm rounds\n"
            f"(rounds = {a.rounds}, the first dropped); scripts/online_apply_vertices_measure.py\n\n" + KERNELS + "\n\n")
    with open(a.out, "w") as f:
        f.write(head + rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
