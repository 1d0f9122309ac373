"""Same-process A/B of the count phase with and without the reuse of the count's structure at config 3:
G(1M, 10M), e = 2, one context, one pair of output buffers, the cases alternating within the process.
    off     GNNPE_COUNT_REUSE=0: every count builds pair records, record order, start records and the total (the code path of the
            releases before the reuse: k_rows_rank_multi + k_start_scan)
    on      the default: counts after the first refresh the embeddings (k_rows_refresh), nothing else
(The block-driven refresh that profiles/count_reuse_ab.txt compares -- a lane per record in block order -- lost and is gone with its knob.)
Per round and case: device time (events) of vde + count alone and of whole enqueued steps (vde, enqueue-only count, capped fill), ten
each.  Diagnostic build (scripts/_diag.py).
    python scripts/count_reuse_ab.py [off on]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _diag  # noqa: F401  (the diagnostic build: the knobs of this script live there)
import numpy as np, torch
import gnnpe_amd  # noqa: F401
from gnnpe_amd import binding, synth

CASES = {"off": {"GNNPE_COUNT_REUSE": "0"}, "on": {}}
KEYS = ["GNNPE_COUNT_REUSE"]
cases = sys.argv[1:] or ["off", "on"]
ROUNDS, ITERS = int(os.environ.get("GNNPE_AB_ROUNDS", "3")), int(os.environ.get("GNNPE_AB_ITERS", "10"))  # keep both small under --pmc

g = synth.gnm_graph(1_000_000, 10_000_000)
sn = synth.degree_order(g["offsets"])
stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
eng = binding.Engine(0, stream=stream.cuda_stream)
eng.load_csr(g["offsets"], g["nbrs"], g["labels"]); eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
eng.set_label_table(binding.host_label_table(64, 2)); eng.vde(want=False)
want = synth.expected_paths_l2(g["offsets"])
assert eng.count_paths(2) == want
dev = torch.device("cuda:0")
ids = torch.empty((want, 3), dtype=torch.int32, device=dev)
pde = torch.empty((want, 6), dtype=torch.float64, device=dev)


def timed(fn):
    ts = []
    for _ in range(ITERS):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), sorted(ts)[len(ts) // 2]


def count_only():
    eng.vde(want=False); eng.count_paths_enqueue(2)


def whole_step():
    eng.vde(want=False); eng.count_paths_enqueue(2); eng.fill_paths_capped_device(want, ids, pde)


def vde_only():
    eng.vde(want=False)


check = None
for rnd in range(ROUNDS):
    for case in cases:
        for k in KEYS: os.environ.pop(k, None)
        os.environ.update(CASES[case])
        whole_step(); eng.sync()  # (a step of this case first: its structure, its code in the caches)
        assert eng.count_total() == want
        v = timed(vde_only)
        c = timed(count_only)
        s = timed(whole_step)
        # the rows of every case are the same rows
        sums = (int(ids[:, 2].to(torch.int64).sum()), float(pde.sum()))
        check = check or sums
        assert sums == check, (case, sums, check)
        print(f"round {rnd} {case:6s}: vde {v[0]:.3f}  vde+count min {c[0]:.3f} median {c[1]:.3f}  count alone {c[0] - v[0]:.3f}  "
              f"whole step min {s[0]:.3f} median {s[1]:.3f} ms", flush=True)
eng.close()
