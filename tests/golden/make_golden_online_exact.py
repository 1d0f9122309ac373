#!/usr/bin/env python3
"""exact_answers.json: for the golden queries q0-q4 on the Test graph, the reference's answer (answers.json) beside the true
embedding count -- what exact mode answers (INTEGRATION.md "Exact mode").  The true count is the library's host refinement on
candidate sets that test label and degree only: the refinement restricts only its start vertex to its set, so those sets let
every embedding through.  CPU only.  Re-run: python tests/golden/make_golden_online_exact.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import gnnpe_amd  # noqa: E402,F401
from gnnpe_amd import binding  # noqa: E402


def main():
    g = binding.host_load_graph(os.path.join(HERE, "test_graph", "data_graph.graph"))
    deg = np.diff(g["offsets"].astype(np.int64))
    n = g["n"]
    ref = json.load(open(os.path.join(HERE, "online", "answers.json")))
    out = {}
    for name in sorted(ref):
        qp = os.path.join(HERE, "online", f"{name}.graph")
        q = binding.host_load_graph(qp)
        qd = np.diff(q["offsets"].astype(np.int64))
        bm = np.zeros((q["n"], (n + 31) // 32), np.uint32)
        for u in range(q["n"]):
            ids = np.nonzero((g["labels"] == q["labels"][u]) & (deg >= qd[u]))[0]
            np.bitwise_or.at(bm[u], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
        out[name] = dict(reference=ref[name], exact=binding.host_refine(g, qp, bm))
    with open(os.path.join(HERE, "online", "exact_answers.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
