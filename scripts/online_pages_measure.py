#!/usr/bin/env python3
"""The match cursor (gnnpe_refine_pages_*) measured against the one-shot gnnpe_refine_sets: the graphs
and queries of scripts/online_refine_measure.py -- 1M vertices / 10M edges, G(n,m) and power-law, 64 labels, cut queries of 8
vertices, query rng 2026 -- on the exact bitmaps of the modes given (--modes, default l3; l2_exact costs another 15-19 s of
filter per power-law query).  One JSON line per measurement on stdout.

power-law, limit 10^7, per query:
  "protocol": device ms of gnnpe_refine_sets with matches_cap = limit (the baseline) and of a cursor with ONE page of `limit`
      rows, the two alternating in one process on one bitmap, one run of each to warm up, then best of three and the spread;
  "paging":   the cursor with pages of 2^16, 2^20 and 2^22 rows: total device ms, launches, mean suspended waves per page,
      end-to-end seconds with every page copied to the host (open and close included).
  "full" (query --full-query, default 2): every embedding through 2^22-row device pages, rows discarded.
G(n,m), limit 2^32 - 1, per query:
  "fixed_cost": wall-clock of one gnnpe_refine_sets call with matches against open + one next + close of a cursor.

Every graph is measured in a child process under a time limit of its own (--time-limit seconds); a child that passes it is
ended, its finished rows stay, a "timed_out" row follows and nothing is run again.
Usage: python scripts/online_pages_measure.py [--queries 5] [--out DIR] [--graphs gnm,powerlaw] [--modes l3] [--time-limit 600]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

GRAPHS = {"gnm": "gnm_1m_10m", "powerlaw": "powerlaw_1m_10m"}
MODES = {"l2_exact": 2, "l3": 3}
LIMIT = 10 ** 7
PAGE_SIZES = (1 << 16, 1 << 20, 1 << 22)


def emit(**row):
    print(json.dumps(row), flush=True)


def cursor_run(eng, qp, bm, page_rows, limit, device):
    """every page of one cursor: rows, launches, device ms, mean suspended waves per page, seconds from open to close"""
    t0 = time.perf_counter()
    rows = ms = susp = 0
    with eng.open_match_cursor(qp, bm, page_rows, limit=limit, device=device) as cur:
        done = False
        while not done:
            page, done = cur.next()
            rows += page.shape[0]
            ms += cur.device_ms
            susp += cur.info()["suspended_waves"]
        info = cur.info()
    pages = max(info["pages"], 1)
    return dict(rows=rows, launches=info["pages"], device_ms=round(ms, 3), mean_suspended=round(susp / pages, 1),
                slots=info["slots"], seconds=round(time.perf_counter() - t0, 4))


def child(kind, a):
    import gnnpe_amd  # noqa: F401
    from gnnpe_amd import binding, synth
    from make_golden_online import cut_query
    gname = GRAPHS[kind]
    g = synth.gnm_graph(1_000_000, 10_000_000) if kind == "gnm" else synth.powerlaw_graph(1_000_000, 10_000_000)
    sn = synth.degree_order(g["offsets"])
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
    eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, 2))
    eng.vde(want=False)
    rng = np.random.default_rng(2026)
    for k in range(a.queries):
        qp = os.path.join(a.out, f"{gname}_q{k}.graph")
        open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], a.size, rng))
        for mode in a.modes.split(","):
            print(f"{gname} q{k} {mode}", file=sys.stderr, flush=True)
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, MODES[mode]))
            base = dict(graph=gname, query=k, mode=mode)
            if kind == "gnm":
                limit = 0xFFFFFFFF
                for rep in range(2):  # the first pair warms up
                    t0 = time.perf_counter()
                    ans, sets_ms, rows = eng.refine_sets(qp, bm, limit, matches_cap=1 << 16)
                    t1 = time.perf_counter()
                    c = cursor_run(eng, qp, bm, 1 << 16, limit, device=False)
                assert c["rows"] == ans == len(rows)
                emit(kind="fixed_cost", answers=ans, sets_call_s=round(t1 - t0, 5), sets_device_ms=round(sets_ms, 3),
                     cursor_open_next_close_s=c["seconds"], cursor_device_ms=c["device_ms"], cursor_launches=c["launches"], **base)
                continue
            sets_ms, page_ms = [], []
            for rep in range(4):  # alternating; the first pair warms up
                ans, ms, rows = eng.refine_sets(qp, bm, LIMIT, matches_cap=LIMIT)
                del rows
                c = cursor_run(eng, qp, bm, LIMIT, LIMIT, device=True)
                assert c["rows"] == ans, (c, ans)
                if rep:
                    sets_ms.append(ms)
                    page_ms.append(c["device_ms"])
            emit(kind="protocol", answers=ans, limit=LIMIT, sets_ms=round(min(sets_ms), 3),
                 sets_spread_ms=round(max(sets_ms) - min(sets_ms), 3), cursor_one_page_ms=round(min(page_ms), 3),
                 cursor_spread_ms=round(max(page_ms) - min(page_ms), 3), cursor_launches=c["launches"], **base)
            for page_rows in PAGE_SIZES:
                c = cursor_run(eng, qp, bm, page_rows, LIMIT, device=False)
                assert c["rows"] == ans, (c, ans)
                emit(kind="paging", page_rows=page_rows, limit=LIMIT, **c, **base)
            if k == a.full_query:
                c = cursor_run(eng, qp, bm, 1 << 22, 2 ** 64 - 1, device=True)
                emit(kind="full", page_rows=1 << 22, **c, **base)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=5)
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profile_out", "online_pages"))
    ap.add_argument("--graphs", default="gnm,powerlaw")
    ap.add_argument("--modes", default="l3")
    ap.add_argument("--full-query", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=600.0)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        return child(a.child, a)
    for kind in GRAPHS:
        if kind not in a.graphs.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--queries", str(a.queries), "--size", str(a.size),
               "--out", a.out, "--modes", a.modes, "--full-query", str(a.full_query)]
        p = subprocess.Popen(cmd)  # a fresh process per graph: its rows go straight to this stdout
        try:
            rc = p.wait(timeout=a.time_limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            emit(graph=GRAPHS[kind], timed_out=True, time_limit_s=a.time_limit)
            return 1  # nothing more is started after a run that had to be ended
        if rc != 0:
            emit(graph=GRAPHS[kind], failed=True, returncode=rc)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
