#!/usr/bin/env python3
"""Golden answers for the GNN-PGE online row, printed by the COMPILED reference (oracle/_ref/ref_main_pge = unmodified
GNN-PGE/src/main.cpp + libsrc, built by oracle/Makefile): `-m offline`, then `-m online -q <query>` on the Test graph for
the sample query and the five online queries, at p = 1 and 2, plus one run capped by `-n`.  Stores data only (the
answer counts).  Re-run: python tests/golden/make_golden_pge_online.py"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import gnnpe_amd  # noqa: E402,F401
from gnnpe_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_main_pge")
# query name -> path relative to tests/golden
QUERIES = {"qg": "test_graph/query_graph.graph", **{f"q{i}": f"online/q{i}.graph" for i in range(5)}}
CAPPED = ("q0", 1000)


def answer(wd, graph, p, query, limit=None):
    cmd = [REF, "-f", wd + "/", "-d", graph, "-q", os.path.join(HERE, query), "-m", "online", "-p", str(p)]
    if limit is not None:
        cmd += ["-n", str(limit)]
    out = subprocess.check_output(cmd, text=True)
    return int(re.search(r"Answer Num: (\d+)", out).group(1))


def main():
    graph = os.path.join(HERE, "test_graph", "data_graph.graph")
    deg = np.array([int(l.split()[3]) for l in open(graph) if l.startswith("v")])
    n = len(deg)
    order = np.argsort(deg, kind="stable").astype(np.uint32)  # the prep step's degree order (make_golden_pge.py)
    gold = dict(queries=QUERIES)
    for p, mem in ((1, np.zeros(n, np.uint32)), (2, (np.arange(n) % 2).astype(np.uint32))):
        with tempfile.TemporaryDirectory() as wd:
            for i in range(p):
                os.makedirs(os.path.join(wd, "gnn-pge", "partitions", f"partition-{i}"))
            synth.write_membership(os.path.join(wd, "gnn-pge", "membership.txt"), order, mem)
            subprocess.check_call([REF, "-f", wd + "/", "-d", graph, "-m", "offline", "-p", str(p)], stdout=subprocess.DEVNULL)
            gold[f"p{p}"] = {name: answer(wd, graph, p, q) for name, q in QUERIES.items()}
            if p == 1:
                gold["capped"] = dict(query=CAPPED[0], n=CAPPED[1], p=1,
                                      answer_num=answer(wd, graph, p, QUERIES[CAPPED[0]], CAPPED[1]))
    json.dump(gold, open(os.path.join(HERE, "pge_online.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(gold, indent=1))


if __name__ == "__main__":
    main()
