#!/usr/bin/env python3
"""What the entry map and the carry of a per-entry table cost ("Carrying per-entry tables"; ABI 20).

Graph: gnm_graph(1_000_000, 10_000_000) of the README figures, 2 x 10^7 adjacency entries; batches of half non-edge inserts and
half existing deletes, seed 1, as scripts/online_apply_edges_measure.py draws them.  Three parts, each a child process under its
own time limit, one JSON line per case:

  apply   gnnpe_csr_apply_edges in the process pattern of the ABI 16 table -- apply (I, D), load_csr of G', load_csr of G, ...,
          --rounds rounds, the first dropped, best and spread of device_ms and of the wall clock -- and, where the library has it,
          gnnpe_csr_apply_edges_map in the same pattern.  The child talks to the library through ctypes alone, so --lib may name a
          libgnnpe_hip.so of ANOTHER commit (the parent's: the plain call must lie within its spread); --label tags its rows.
  carry   after a batch of 10 000: gnnpe_csr_carry_entries of 3 rows of 8 bytes (480 MB in, 480 MB out) beside a device-to-device
          hipMemcpyAsync of the same bytes between the same two buffers (gnnpe_copy_device on the context's stream), alternating,
          wall clock between two stream synchronisations, at least twenty warm pairs; the carry's device_ms too; the same with
          4-byte cells.
  trip    the carry on the device (one run, wall clock) beside the host round trip it replaces: download the CSR of G (before the apply) and of G',
          copy the table to the host, carry it in numpy by the key (x, y), copy it back (one run, wall clock, its parts listed).

Usage: python scripts/online_entry_map_measure.py [--parts apply,carry,trip] [--lib PATH --label NAME] [--rounds 4]
                                                  [--sizes 100,10000] [--time-limit 300]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import online_apply_edges_measure as base  # noqa: E402  (make_graph, und_edges, batch, updated)


def stat(v):
    return dict(best=round(min(v[1:]), 4), spread=round(max(v[1:]) - min(v[1:]), 4), first=round(v[0], 4))


def child_apply(a):
    """ctypes alone: the entries used here have had these signatures since ABI 16"""
    import torch  # noqa: F401  (its libamdhip64 first, as binding.load does)
    lib = C.CDLL(a.lib)
    u32p, u64p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    lib.gnnpe_create.restype = C.c_void_p
    lib.gnnpe_create.argtypes = [C.c_int]
    lib.gnnpe_destroy.argtypes = [C.c_void_p]
    lib.gnnpe_last_error.restype = C.c_char_p
    lib.gnnpe_sync.argtypes = [C.c_void_p]
    lib.gnnpe_load_csr.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, u32p]
    lib.gnnpe_csr_apply_edges.argtypes = [C.c_void_p, u32p, C.c_uint64, u32p, C.c_uint64, u64p, f64p]
    has_map = hasattr(lib, "gnnpe_csr_apply_edges_map")
    if has_map:
        lib.gnnpe_csr_apply_edges_map.argtypes = [C.c_void_p, u32p, C.c_uint64, u32p, C.c_uint64, u64p, u64p, C.POINTER(C.c_void_p), f64p]
    g = base.make_graph("gnm")
    codes = base.und_edges(g)
    ctx = lib.gnnpe_create(0)
    assert ctx, lib.gnnpe_last_error()
    p = lambda arr: arr.ctypes.data_as(u32p)

    def ck(rc):
        assert rc == 0, lib.gnnpe_last_error()

    def load(x):
        o, nb, lb = (np.ascontiguousarray(x[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
        ck(lib.gnnpe_load_csr(ctx, x["n"], p(o), p(nb), p(lb)))
        ck(lib.gnnpe_sync(ctx))

    load(g)
    rng = np.random.default_rng(1)
    for k in (int(s) for s in a.sizes.split(",")):
        ins, dele = base.batch(g, codes, k, rng)
        g2 = base.updated(g, codes, ins, dele)
        i32, d32 = np.ascontiguousarray(ins, np.uint32), np.ascontiguousarray(dele, np.uint32)
        for call in ("gnnpe_csr_apply_edges",) + (("gnnpe_csr_apply_edges_map",) if has_map else ()):
            dev, wall = [], []
            for _ in range(a.rounds):
                after, before, ms, ptr = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_void_p()
                t0 = time.perf_counter()
                if call.endswith("_map"):
                    ck(lib.gnnpe_csr_apply_edges_map(ctx, p(i32), len(i32), p(d32), len(d32), C.byref(before), C.byref(after), C.byref(ptr), C.byref(ms)))
                else:
                    ck(lib.gnnpe_csr_apply_edges(ctx, p(i32), len(i32), p(d32), len(d32), C.byref(after), C.byref(ms)))
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(ms.value)
                assert after.value == len(g2["nbrs"])
                load(g2)
                load(g)
            print(json.dumps(dict(part="apply", lib=a.label, call=call, entries=len(g["nbrs"]), batch=k, device_ms=stat(dev), wall_ms=stat(wall))),
                  flush=True)
    lib.gnnpe_destroy(ctx)


def _carry_np(n, g_from, g_to, table):
    """the host's carry: by the key x * n + y of an entry"""
    keys = lambda x: np.repeat(np.arange(n, dtype=np.int64), np.diff(x["offsets"].astype(np.int64))) * n + x["nbrs"].astype(np.int64)
    k_from, k_to = keys(g_from), keys(g_to)
    out = np.zeros((table.shape[0], len(k_to)), table.dtype)
    there = np.isin(k_from, k_to, assume_unique=True)
    out[:, np.searchsorted(k_to, k_from[there])] = table[:, there]
    return out


def child_carry(a, trip):
    import torch
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding
    g = base.make_graph("gnm")
    codes = base.und_edges(g)
    ins, dele = base.batch(g, codes, 10_000, np.random.default_rng(1))
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    t0 = time.perf_counter()
    off0, nb0 = eng.download_csr() if trip else (None, None)
    t_old = (time.perf_counter() - t0) * 1e3  # the round trip's download of G: it has to be made before the apply
    before, after, view = eng.apply_edges_map(ins, dele)
    rows = 3
    if not trip:
        for eb, dt in ((8, torch.int64), (4, torch.int32)):
            src = torch.randint(1, 1 << 30, (rows, before), dtype=dt, device="cuda:0")
            dst = torch.empty((rows, after), dtype=dt, device="cuda:0")
            torch.cuda.synchronize()
            nbytes = rows * before * eb
            assert before == after  # (as many inserts as deletes: the copy moves the same bytes)
            carry, copy, dev = [], [], []
            for _ in range(max(a.rounds, 21)):  # (a call takes 0.1 to 0.2 ms: twenty warm pairs)
                eng.sync()
                t0 = time.perf_counter()
                ms = eng.carry_entries(src, dst, rows, elem_bytes=eb, timing=True)
                eng.sync()
                carry.append((time.perf_counter() - t0) * 1e3)
                dev.append(ms)
                t0 = time.perf_counter()
                eng._ck(eng.lib.gnnpe_copy_device(eng.ctx, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes))
                eng.sync()
                copy.append((time.perf_counter() - t0) * 1e3)
            row = dict(part="carry", rows=rows, elem_bytes=eb, entries_before=before, entries_after=after, bytes_in=nbytes, bytes_out=rows * after * eb,
                       carry_wall_ms=stat(carry), carry_device_ms=stat(dev), copy_wall_ms=stat(copy))
            row["carry_over_copy"] = round(min(carry[1:]) / min(copy[1:]), 3)
            row["carry_bytes_per_s"] = round((nbytes + rows * after * eb + 4 * after) / (min(dev[1:]) * 1e-3), 0)
            print(json.dumps(row), flush=True)
            del src, dst
    else:
        m = eng.entry_map_to_host(view)
        src = torch.randint(1, 1 << 30, (rows, before), dtype=torch.int64, device="cuda:0")
        gone = np.ones(before, bool)
        gone[m[m != 0xFFFFFFFF]] = False
        src[:, torch.as_tensor(np.nonzero(gone)[0], device="cuda:0")] = 0  # the entries of D hold zero by the time of the carry
        dst = torch.empty((rows, after), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        eng.carry_entries(src, dst, rows)  # warm
        eng.sync()
        t0 = time.perf_counter()
        eng.carry_entries(src, dst, rows)
        eng.sync()
        t_dev = (time.perf_counter() - t0) * 1e3
        t = [time.perf_counter()]
        off1, nb1 = eng.download_csr()
        t.append(time.perf_counter())
        table = src.cpu().numpy()
        t.append(time.perf_counter())
        moved = _carry_np(g["n"], dict(offsets=off0, nbrs=nb0), dict(offsets=off1, nbrs=nb1), table)
        t.append(time.perf_counter())
        back = torch.from_numpy(moved).to("cuda:0")
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        assert torch.equal(back, dst)
        parts = [round((t[k + 1] - t[k]) * 1e3, 2) for k in range(4)]
        parts[0] = round(parts[0] + t_old, 2)
        print(json.dumps(dict(part="trip", rows=rows, elem_bytes=8, entries=after, device_carry_wall_ms=round(t_dev, 4),
                              host_round_trip_wall_ms=round(sum(parts), 2), download_csr_ms=parts[0], table_to_host_ms=parts[1],
                              numpy_carry_ms=parts[2], table_to_device_ms=parts[3], ratio=round(sum(parts) / t_dev, 1))), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="apply,carry,trip")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gnn-pe_amd", "libgnnpe_hip.so"))
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--sizes", default="100,10000")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--time-limit", type=float, default=300.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        try:
            return child_apply(a) if a.child == "apply" else child_carry(a, a.child == "trip")
        except Exception:
            import traceback
            print(json.dumps(dict(part=a.child, failed=True, error=traceback.format_exc()[-600:])), flush=True)
            return 1
    for part in (k for k in a.parts.split(",") if k):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--lib", a.lib, "--label", a.label, "--sizes", a.sizes, "--rounds", str(a.rounds)]
        p = subprocess.Popen(cmd)  # a fresh process per part: its rows go straight to this stdout
        try:
            rc = p.wait(timeout=a.time_limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            print(json.dumps(dict(part=part, timed_out=True, time_limit_s=a.time_limit)), flush=True)
            return 1  # nothing more is started after a run that had to be ended
        if rc != 0:
            print(json.dumps(dict(part=part, failed=True, returncode=rc)), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
