"""Exact online queries (INTEGRATION.md "Exact mode"): the orientation-complete filter at l = 2 and the 4-vertex (l = 3) filter.

Contract: C(u) = the union over the plan paths through u of the data vertices at u's position in every simple data path that
passes the reference's leaf test in EITHER orientation; a query vertex on no plan path gets label, degree and vde dominance.
Oracles: the oracle's width-generic leaf test (orc_filter_candidates) over enumerate_closed(..., L) stacked with its
column-reversed copy, a numpy restatement of the vertex test, and a Python restatement of the planner.  Answers: the true
embedding count, from networkx and from the frozen host refinement on a label/degree-only bitmap (the refinement restricts
only its start vertex to its set, so that bitmap counts every embedding)."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

ONLINE = os.path.join(GOLDEN, "online")
QUERIES = ["q0", "q1", "q2", "q3", "q4"]
CLI = os.path.join(ROOT, "gnn-pe_amd", "gnnpe_main")
EPS = 1e-6


def _cut_query():
    sys.path.insert(0, GOLDEN)
    from make_golden_online import cut_query
    return cut_query


def _write_query(path, n, edges, labels):
    deg = np.zeros(n, np.int64)
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
    lines = [f"t {n} {len(edges)}"] + [f"v {i} {int(labels[i])} {int(deg[i])}" for i in range(n)]
    lines += [f"e {a} {b}" for a, b in sorted(edges)]
    open(path, "w").write("\n".join(lines) + "\n")


# ---- Python restatement of the exact planner (host/query_plan.cpp build_query_plan_exact) ------------------------------------

def _dfs_paths(offs, nbrs, n, length):
    """dfs_query (custom.h:94-119) at `length` vertices: from every vertex in id order, neighbours in row order, a path is kept
    unless it or its reverse was kept before"""
    seen, out = set(), []

    def rec(path):
        if len(path) == length:
            t = tuple(path)
            if t in seen or t[::-1] in seen:
                return
            out.append(t)
            seen.add(t)
            return
        for nb in nbrs[offs[path[-1]]:offs[path[-1] + 1]]:
            nb = int(nb)
            if nb in path:
                continue
            path.append(nb)
            rec(path)
            path.pop()

    for v in range(n):
        rec([v])
    return out


def py_plan_exact(qpath, e, l):
    """(main, tri, single) vertex tuples of the exact plan"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qpath)
    n, offs, nbrs = q["n"], q["offsets"].astype(np.int64), q["nbrs"]
    deg = np.diff(offs)
    ref = [tuple(int(v) for v in p) for p in binding.host_query_plan(qpath, e)["vids"]]
    covered, main, tri = set(), [], []

    def take(p, dst):  # gen_query_pde (custom.h:606-626)
        if len(covered) == n or all(v in covered for v in p):
            return
        covered.update(p)
        dst.append(p)

    if l == 2:
        main = list(ref)
        for p in ref:
            covered.update(p)
    else:
        all4 = _dfs_paths(offs, nbrs, n, 4)
        for p in sorted(all4, key=lambda p: -int(sum(deg[v] for v in p))):  # stable, descending weight
            take(p, main)
        for p in ref:
            take(p, tri)
    single = [(u,) for u in range(n) if u not in covered]
    return main, tri, single


# ---- oracle candidate sets ------------------------------------------------------------------------------------------------

def oracle_exact_sets(oracle, g, sn, vde, plan, paths_cache=None):
    """reference sets of the exact contract for `plan` (host_query_plan_exact's dict), both orientations of every data path"""
    offs, labels = g["offsets"], g["labels"]
    nq = plan["n_vertices"]
    n = len(offs) - 1
    deg = np.diff(offs.astype(np.int64))
    sets = [set() for _ in range(nq)]
    cache = {} if paths_cache is None else paths_cache
    for part in ("main", "tri"):
        p = plan[part]
        if len(p["vids"]) == 0:
            continue
        W = p["vids"].shape[1]
        if W not in cache:
            fwd = oracle.enumerate_closed(offs, g["nbrs"], sn, W)
            cache[W] = (fwd, np.ascontiguousarray(fwd[:, ::-1]))
        for paths in cache[W]:
            got = oracle.filter_candidates(paths, offs, labels, vde, p["vids"], p["labels"], p["degrees"], p["pde"], nq)
            for u in range(nq):
                sets[u].update(int(v) for v in got[u])
    s = plan["single"]
    for i in range(len(s["vids"])):
        q = s["pde"][i]
        ok = (labels == s["labels"][i, 0]) & (deg >= s["degrees"][i, 0])
        ok &= ~np.any((q[None, :] > vde) & (np.abs(q[None, :] - vde) > EPS), axis=1)
        sets[int(s["vids"][i, 0])].update(int(v) for v in np.nonzero(ok)[0])
    assert all(v < n for st in sets for v in st)
    return [np.array(sorted(st), np.uint32) for st in sets]


def _ld_bitmap(g, qpath):
    """label + degree only: every embedding's image passes"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qpath)
    qd = np.diff(q["offsets"].astype(np.int64))
    deg = np.diff(g["offsets"].astype(np.int64))
    n = len(g["labels"])
    bm = np.zeros((q["n"], (n + 31) // 32), np.uint32)
    for u in range(q["n"]):
        ids = np.nonzero((g["labels"] == q["labels"][u]) & (deg >= qd[u]))[0]
        np.bitwise_or.at(bm[u], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return bm


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def _random_queries(tmp_path, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(2, 10))
        kind = i % 5
        if kind == 0:  # star: no 4-vertex path
            edges = {(0, j) for j in range(1, n)}
        elif kind == 1 and n >= 3:  # a path plus a pendant isolated vertex
            edges = {(j, j + 1) for j in range(n - 2)}
        else:
            m = int(rng.integers(1, n * (n - 1) // 2 + 1))
            edges = set()
            while len(edges) < m:
                a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False))
                edges.add((a, b))
        p = str(tmp_path / f"rq{i}.graph")
        _write_query(p, n, edges, rng.integers(0, 3, n))
        out.append(p)
    return out


@pytest.mark.parametrize("l", [2, 3])
def test_exact_planner_equals_the_python_restatement(tmp_path, oracle, l):
    """>= 50 random small query graphs (stars, isolated vertices, dense ones): the library's exact plan == the restatement,
    every query vertex covered exactly by the three parts, pde = the query vde at every position"""
    from gnnpe_amd import binding
    widths = {"main": l + 1, "tri": 3, "single": 1}
    seen_parts = {"main": 0, "tri": 0, "single": 0}
    for qpath in _random_queries(tmp_path, 60, 40 + l):
        plan = binding.host_query_plan_exact(qpath, 2, l)
        want = dict(zip(("main", "tri", "single"), py_plan_exact(qpath, 2, l)))
        q = binding.host_load_graph(qpath)
        qdeg = np.diff(q["offsets"].astype(np.int64))
        _, _, vde = oracle.gen_vde(q["offsets"], q["nbrs"], q["labels"], 2)
        covered = set()
        for part, w in widths.items():
            got = plan[part]
            assert [tuple(int(v) for v in p) for p in got["vids"]] == want[part], (qpath, part)
            assert got["vids"].shape[1:] == (w,) and got["pde"].shape[1:] == (2 * w,)
            v = got["vids"].astype(np.int64)
            assert np.array_equal(got["labels"], q["labels"][v]) and np.array_equal(got["degrees"], qdeg[v])
            assert np.array_equal(got["pde"], vde[v].reshape(len(v), 2 * w))
            covered.update(int(x) for x in v.ravel())
            seen_parts[part] += len(v)
        assert covered == set(range(plan["n_vertices"]))
        if l == 2:
            assert len(plan["tri"]["vids"]) == 0
            assert np.array_equal(plan["main"]["vids"], binding.host_query_plan(qpath, 2)["vids"])
    assert seen_parts["main"] and seen_parts["single"] and (l == 2 or seen_parts["tri"])


def test_exact_planner_refuses_other_lengths():
    from gnnpe_amd import binding
    with pytest.raises(binding.GnnpeError):
        binding.host_query_plan_exact(os.path.join(ONLINE, "q0.graph"), 2, 4)
    with pytest.raises(FileNotFoundError):
        binding.host_query_plan_exact("/nonexistent/q.graph", 2, 3)


def _orientation_case(tmp_path):
    """data graph: the path a(0) - b(1) - c(2), labels A B C, c first in the processing order; query: the same labelled path"""
    from gnnpe_amd import synth
    g = dict(n=3, m=2, offsets=np.array([0, 1, 3, 4], np.uint32), nbrs=np.array([1, 0, 2, 1], np.uint32),
             labels=np.array([0, 1, 2], np.uint32), eu=np.array([0, 1]), ev=np.array([1, 2]))
    gp = str(tmp_path / "abc.graph")
    synth.write_graph_file(gp, g)
    qp = str(tmp_path / "q_abc.graph")
    _write_query(qp, 3, {(0, 1), (1, 2)}, [0, 1, 2])
    return g, gp, qp, np.array([2, 0, 1], np.uint32)


def test_orientation_example_reference_misses_exact_finds(oracle, tmp_path):
    """the issue's smallest case: the reference-style set of u0 is empty (answer 0), the exact set holds a (answer 1)"""
    from gnnpe_amd import binding
    g, gp, qp, sn = _orientation_case(tmp_path)
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], 2)
    paths = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    assert paths.tolist() == [[2, 1, 0]]  # the data side keeps (c, b, a) only
    ref_plan = binding.host_query_plan(qp, 2)
    ref = oracle.filter_candidates(paths, g["offsets"], g["labels"], vde, ref_plan["vids"], ref_plan["labels"],
                                   ref_plan["degrees"], ref_plan["pde"], 3)
    assert len(ref[0]) == 0
    exact = oracle_exact_sets(oracle, g, sn, vde, binding.host_query_plan_exact(qp, 2, 2))
    assert [list(s) for s in exact] == [[0], [1], [2]]
    from test_online_filter import _sets_to_bitmap
    assert binding.host_refine(g, qp, _sets_to_bitmap(ref, 3)) == 0
    assert binding.host_refine(g, qp, _sets_to_bitmap(exact, 3)) == 1


def test_golden_exact_answers_are_the_true_counts(test_graph):
    """tests/golden/online/exact_answers.json: the true count of q0-q4 (host refinement on the label/degree bitmap), at least
    the reference's answer"""
    from gnnpe_amd import binding
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    ref = json.load(open(os.path.join(ONLINE, "answers.json")))
    for name in QUERIES:
        qpath = os.path.join(ONLINE, f"{name}.graph")
        assert rec[name]["reference"] == ref[name]
        assert rec[name]["exact"] == binding.host_refine(test_graph, qpath, _ld_bitmap(test_graph, qpath)) >= ref[name]
    assert any(rec[q]["exact"] > rec[q]["reference"] for q in QUERIES)


def _dataset(tmp_path, graph):
    from gnnpe_amd import synth
    deg = np.array([int(l.split()[3]) for l in open(graph) if l.startswith("v")])
    tmp = str(tmp_path)
    synth.make_dataset_dir(tmp, 2)
    synth.write_membership(os.path.join(tmp, "gnn-pe", "membership.txt"), np.argsort(deg, kind="stable").astype(np.uint32),
                           (np.arange(len(deg)) % 2).astype(np.uint32))
    return tmp + "/"


def test_cli_l3_and_exact_get_past_the_old_refusal_and_refuse_multigraphs_first(tmp_path):
    """-m online -l 3 used to die ("only -l 2"); now it plans and goes to the device.  A file with a repeated edge is refused by
    exact -m online before any GPU work; reference mode and -m filter still take it"""
    import torch
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = _dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    for extra in (["-l", "3"], ["--exact"]):
        r = subprocess.run([CLI, "-f", root, "-d", graph, "-q", q, "-m", "online", "-p", "2"] + extra, capture_output=True,
                           text=True, timeout=300)
        if torch.cuda.is_available():
            assert r.returncode == 0 and "Answer Number:" in r.stdout, r.stderr
        else:
            assert r.returncode == 1 and "no HIP device" in r.stderr, r.stderr
    txt = open(graph).read().splitlines()
    e = [l for l in txt if l.startswith("e")][0]
    u, v = e.split()[1:]
    out = []
    for l in txt:
        f = l.split()
        if f[0] == "t":
            l = f"t {f[1]} {int(f[2]) + 1}"
        if f[0] == "v" and f[1] in (u, v):
            l = f"v {f[1]} {f[2]} {int(f[3]) + 1}"
        out.append(l)
    multi = str(tmp_path / "multi.graph")
    open(multi, "w").write("\n".join(out + [e]) + "\n")
    for extra in (["-l", "3"], ["--exact"]):
        r = subprocess.run([CLI, "-f", root, "-d", multi, "-q", q, "-m", "online", "-p", "2"] + extra, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1 and "needs a simple graph" in r.stderr, r.stderr
    if not torch.cuda.is_available():
        for extra in ([], ["--exact"]):
            mode = "filter" if extra else "online"
            r = subprocess.run([CLI, "-f", root, "-d", multi, "-q", q, "-m", mode, "-p", "2"] + extra, capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 1 and "no HIP device" in r.stderr, r.stderr


# ---- GPU: bitmaps ---------------------------------------------------------------------------------------------------------

def _engine(binding, g, sn, e, slab=None):
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, np.zeros(len(g["labels"]), np.uint32), 1)
    if slab is not None:
        eng.set_slab(*slab)
    eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, e))
    eng.vde(want=False)
    return eng


def _check_sets(bm, want, n, what):
    from oracle import bitmap_to_sets
    got = bitmap_to_sets(bm, n)
    for u in range(len(want)):
        assert np.array_equal(got[u], want[u]), (what, u, len(got[u]), len(want[u]))


@pytest.mark.gpu
@pytest.mark.parametrize("e", [2, 8])
def test_gpu_exact_bitmaps_random_graphs(oracle, tmp_path, e):
    """>= 20 random G(n,m) graphs, random orders, cut queries plus stars and single edges: bitmaps == oracle, l = 2 and l = 3"""
    from gnnpe_amd import binding, synth
    cut_query = _cut_query()
    rng = np.random.default_rng(100 + e)
    nonempty = 0
    for trial in range(20):
        n = int(rng.integers(150, 500))
        g = synth.gnm_graph(n, int(n * rng.uniform(2.5, 5)), n_labels=int(rng.integers(2, 5)), seed=int(rng.integers(1 << 30)))
        sn = rng.permutation(n).astype(np.uint32)
        _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
        eng = _engine(binding, g, sn, e)
        cache = {}
        qpaths = []
        for k in range(2):
            qp = str(tmp_path / f"q{trial}_{k}.graph")
            open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], int(rng.integers(3, 8)), rng))
            qpaths.append(qp)
        qp = str(tmp_path / f"q{trial}_x.graph")  # star or single edge: single-vertex tests
        k = int(rng.integers(1, 4))
        _write_query(qp, k + 1, {(0, j) for j in range(1, k + 1)}, rng.integers(0, int(g["labels"].max()) + 1, k + 1))
        qpaths.append(qp)
        for qp in qpaths:
            for l in (2, 3):
                plan = binding.host_query_plan_exact(qp, e, l)
                want = oracle_exact_sets(oracle, g, sn, vde, plan, cache)
                bm, ms = eng.filter_candidates_exact(plan)
                _check_sets(bm, want, n, (trial, qp, l))
                nonempty += sum(len(w) > 0 for w in want)
        eng.close()
    assert nonempty > 100


@pytest.mark.gpu
@pytest.mark.parametrize("e", [2, 8])
def test_gpu_exact_bitmaps_powerlaw_hub_rows(oracle, tmp_path, e):
    """rows of degree > 64 at every level of the 4-vertex walk"""
    from gnnpe_amd import binding, synth
    cut_query = _cut_query()
    g = synth.powerlaw_graph(2000, 6000, exponent=2.1, max_degree=150, n_labels=4, seed=5)
    deg = np.diff(g["offsets"].astype(np.int64))
    assert (deg > 64).sum() >= 10
    sn = synth.degree_order(g["offsets"])
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    eng = _engine(binding, g, sn, e)
    rng = np.random.default_rng(7)
    cache = {}
    hubs = np.nonzero(deg > 64)[0]
    hit_hub = False
    for k in range(4):
        qp = str(tmp_path / f"pq{k}.graph")
        open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], 4 + k, rng))
        for l in (2, 3):
            plan = binding.host_query_plan_exact(qp, e, l)
            want = oracle_exact_sets(oracle, g, sn, vde, plan, cache)
            hit_hub |= any(np.isin(w, hubs).any() for w in want)
            _check_sets(eng.filter_candidates_exact(plan)[0], want, g["n"], (qp, l))
    eng.close()
    assert hit_hub


@pytest.mark.gpu
@pytest.mark.parametrize("e", [2, 8])
def test_gpu_exact_bitmaps_test_graph_golden_queries(oracle, test_graph, e):
    from gnnpe_amd import binding
    g, sn = test_graph, test_graph["sorted_nodes"]
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    eng = _engine(binding, g, sn, e)
    cache = {}
    for name in QUERIES:
        for l in (2, 3):
            plan = binding.host_query_plan_exact(os.path.join(ONLINE, f"{name}.graph"), e, l)
            _check_sets(eng.filter_candidates_exact(plan)[0], oracle_exact_sets(oracle, g, sn, vde, plan, cache),
                        len(g["labels"]), (name, l))
    eng.close()


@pytest.mark.gpu
def test_gpu_exact_bitmaps_slab_contexts(oracle, tmp_path):
    """three slabs of a whole-graph context, and a rows-only context holding a slab and its halo: OR of the slabs == oracle"""
    from gnnpe_amd import binding, synth
    cut_query = _cut_query()
    e = 2
    g = synth.gnm_graph(600, 2400, n_labels=3, seed=77)
    n = g["n"]
    sn = synth.degree_order(g["offsets"])
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    rng = np.random.default_rng(3)
    offs = g["offsets"].astype(np.int64)
    bounds = [0, 150, 420, n]
    deg = np.diff(offs)
    for k in range(3):
        qp = str(tmp_path / f"sq{k}.graph")
        if k < 2:
            open(qp, "w").write(cut_query(offs, g["nbrs"], g["labels"], 5 + k, rng))
        else:
            _write_query(qp, 2, {(0, 1)}, [0, 1])  # single edge: vertex-level tests only
        for l in (2, 3):
            plan = binding.host_query_plan_exact(qp, e, l)
            want = oracle_exact_sets(oracle, g, sn, vde, plan)
            acc = acc_rows = None
            for r in range(3):
                eng = _engine(binding, g, sn, e, slab=(bounds[r], bounds[r + 1]))
                bm = eng.filter_candidates_exact(plan)[0]
                acc = bm if acc is None else acc | bm
                eng.close()
                # rows-only context: the slab's rows and every row within three hops (the filter reads rows two hops out and
                # the vde of the vertices three hops out; gnnpe_vde computes it for the rows held)
                held = set(int(v) for v in sn[bounds[r]:bounds[r + 1]])
                front = set(held)
                for _ in range(3):
                    front = {int(w) for v in front for w in g["nbrs"][offs[v]:offs[v + 1]]} - held
                    held |= front
                rows = np.array(sorted(held), np.uint32)
                roff = np.zeros(len(rows) + 1, np.uint64)
                np.cumsum(deg[rows.astype(np.int64)], out=roff[1:])
                rnbr = np.concatenate([g["nbrs"][offs[v]:offs[v + 1]] for v in rows]).astype(np.uint32) \
                    if len(rows) else np.zeros(0, np.uint32)
                eng = binding.Engine(0)
                eng.load_rows(n, g["labels"], rows, roff, rnbr)
                eng.set_order(sn, np.zeros(n, np.uint32), 1)
                eng.set_slab(bounds[r], bounds[r + 1])
                eng.set_label_table(binding.host_label_table(int(g["labels"].max()) + 1, e))
                eng.vde(want=False)
                eng.set_degrees(deg)
                bm = eng.filter_candidates_exact(plan)[0]
                acc_rows = bm if acc_rows is None else acc_rows | bm
                eng.close()
            _check_sets(acc, want, n, ("slabs", qp, l))
            _check_sets(acc_rows, want, n, ("rows", qp, l))


@pytest.mark.gpu
def test_gpu_exact_filter_argument_checks(test_graph):
    from gnnpe_amd import binding
    g = test_graph
    eng = _engine(binding, g, g["sorted_nodes"], 2)
    plan = binding.host_query_plan_exact(os.path.join(ONLINE, "q0.graph"), 2, 3)
    big = dict(plan)
    big["main"] = {k: np.repeat(v, 257 // max(len(v), 1) + 1, axis=0)[:257] for k, v in plan["main"].items()}
    with pytest.raises(binding.GnnpeError, match="limit 512"):
        eng.filter_candidates_exact(big)  # 257 paths, 514 with their reverses
    with pytest.raises(binding.GnnpeError, match="l = 4"):
        eng.filter_candidates_exact(dict(plan, l=4))
    eng.close()


# ---- GPU: answers ---------------------------------------------------------------------------------------------------------

def _nx_count(g, qpath):
    import networkx as nx
    from networkx.algorithms import isomorphism as iso
    from gnnpe_amd import binding

    def G(offs, nbrs, labels):
        H = nx.Graph()
        for v in range(len(labels)):
            H.add_node(v, l=int(labels[v]))
        for v in range(len(labels)):
            for w in nbrs[offs[v]:offs[v + 1]]:
                H.add_edge(v, int(w))
        return H
    q = binding.host_load_graph(qpath)
    D, Q = G(g["offsets"], g["nbrs"], g["labels"]), G(q["offsets"], q["nbrs"], q["labels"])
    return sum(1 for _ in iso.GraphMatcher(D, Q, node_match=lambda a, b: a["l"] == b["l"]).subgraph_monomorphisms_iter())


@pytest.mark.gpu
def test_gpu_exact_answers_equal_networkx(tmp_path):
    """>= 10 small random labelled graphs, cut queries: device refinement on the exact sets == networkx monomorphism count"""
    from gnnpe_amd import binding, synth
    cut_query = _cut_query()
    rng = np.random.default_rng(21)
    total = 0
    for trial in range(12):
        g = synth.gnm_graph(60, int(rng.integers(90, 160)), n_labels=3, seed=500 + trial)
        sn = rng.permutation(g["n"]).astype(np.uint32)
        qp = str(tmp_path / f"nq{trial}.graph")
        open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], int(rng.integers(3, 7)), rng))
        want = _nx_count(g, qp)
        eng = _engine(binding, g, sn, 2)
        for l in (2, 3):
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            assert eng.refine(qp, bm)[0] == want, (trial, l)
            assert binding.host_refine(g, qp, bm) == want, (trial, l)
        eng.close()
        total += want
    assert total > 0


@pytest.mark.gpu
def test_gpu_exact_answers_test_graph(test_graph):
    """q0-q4: l = 2 exact and l = 3 answer the true count (host refinement on the label/degree bitmap), recorded beside the
    reference's answer in tests/golden/online/exact_answers.json"""
    from gnnpe_amd import binding
    g = test_graph
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    eng = _engine(binding, g, g["sorted_nodes"], 2)
    for name in QUERIES:
        qp = os.path.join(ONLINE, f"{name}.graph")
        truth = binding.host_refine(g, qp, _ld_bitmap(g, qp))
        assert truth == rec[name]["exact"] >= rec[name]["reference"]
        for l in (2, 3):
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            assert eng.refine(qp, bm)[0] == truth, (name, l)
    eng.close()


def _cut_with_sources(offs, nbrs, labels, size, rng):
    """make_golden_online.cut_query, also returning the data vertex every query vertex was cut from"""
    n = len(offs) - 1
    while True:
        v = int(rng.integers(n))
        if offs[v + 1] > offs[v]:
            break
    chosen = [v]
    while len(chosen) < size:
        u = chosen[int(rng.integers(len(chosen)))]
        w = int(nbrs[int(rng.integers(offs[u], offs[u + 1]))])
        if w not in chosen:
            chosen.append(w)
    idx = {v: i for i, v in enumerate(chosen)}
    edges = {(idx[v], idx[int(w)]) for v in chosen for w in nbrs[offs[v]:offs[v + 1]] if int(w) in idx and idx[v] < idx[int(w)]}
    return edges, [int(labels[v]) for v in chosen], chosen


@pytest.mark.gpu
def test_gpu_exact_scale_cut_sources_are_candidates(tmp_path):
    """1M vertices / 10M edges, cut queries of 6-10 vertices: every cut source vertex is in its query vertex's set"""
    from gnnpe_amd import binding, synth
    g = synth.gnm_graph(1_000_000, 10_000_000)
    sn = synth.degree_order(g["offsets"])
    eng = _engine(binding, g, sn, 2)
    rng = np.random.default_rng(11)
    offs = g["offsets"].astype(np.int64)
    for k, size in enumerate((6, 8, 10)):
        edges, labels, src = _cut_with_sources(offs, g["nbrs"], g["labels"], size, rng)
        qp = str(tmp_path / f"big{k}.graph")
        _write_query(qp, size, edges, labels)
        for l in (2, 3):
            bm, ms = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            assert ms > 0
            for u, v in enumerate(src):
                assert (bm[u, v >> 5] >> (v & 31)) & 1, (size, l, u, v)
    eng.close()


# ---- GPU: CLI -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_cli_exact_online_and_filter(tmp_path, test_graph):
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = _dataset(tmp_path, graph)
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    for name in ("q0", "q3"):
        qp = os.path.join(ONLINE, f"{name}.graph")
        base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2"]
        r = subprocess.run(base + ["-m", "online"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"Answer Number: {rec[name]['reference']} " in r.stdout, r.stderr  # -l 2: unchanged
        for extra in (["--exact"], ["-l", "3"], ["-l", "3", "--exact"]):
            r = subprocess.run(base + ["-m", "online", "--timing"] + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            assert f"Answer Number: {rec[name]['exact']} " in r.stdout, (extra, r.stdout)
            t = json.loads(r.stderr.strip().splitlines()[-1])
            l = 3 if "3" in extra else 2
            plan = binding.host_query_plan_exact(qp, 2, l)
            assert t["exact"] is True and t["l"] == l
            assert t["plan_paths_by_width"][str(l + 1)] == len(plan["main"]["vids"])
            assert t["plan_paths_by_width"]["1"] == len(plan["single"]["vids"])
            assert len(t["candidates"]) == plan["n_vertices"] and min(t["candidates"]) > 0
        # -m filter -l 3: candidates.bin == the library's bitmap
        r = subprocess.run(base + ["-m", "filter", "-l", "3"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        eng = _engine(binding, test_graph, test_graph["sorted_nodes"], 2)
        bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, 3))
        eng.close()
        from oracle import bitmap_to_sets
        want = bitmap_to_sets(bm, len(test_graph["labels"]))
        b = open(os.path.join(root, "gnn-pe", "candidates.bin"), "rb").read()
        assert struct.unpack_from("<I", b, 0)[0] == len(want)
        off = 4
        for u in range(len(want)):
            c, = struct.unpack_from("<I", b, off)
            assert np.array_equal(np.frombuffer(b, np.uint32, c, off + 4), want[u]), (name, u)
            off += 4 + 4 * c
        assert off == len(b)


def test_cli_refuses_exact_outside_online_and_filter(tmp_path):
    """--exact means nothing to -m offline: refused before the graph is read, not ignored"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = _dataset(tmp_path, graph)
    r = subprocess.run([CLI, "-f", root, "-d", graph, "-m", "offline", "-p", "2", "--exact"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "--exact applies to -m online and -m filter only" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(root, "gnn-pe", "all_paths.txt"))
