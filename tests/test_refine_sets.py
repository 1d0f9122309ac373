"""Set-restricted refinement (include/gnnpe_online.h "ABI version 9"): R(C, limit) = min(limit, number of embeddings f with
f(u) in C(u) for EVERY query vertex u).

Yardsticks: networkx's monomorphisms (all of them, then filtered by the sets), the frozen refinements on complete sets
(gnnpe_host_refine / gnnpe_refine restrict the start vertex only, so they agree exactly where every set is complete), and the
host form gnnpe_host_refine_sets for the device kernel on graphs networkx is too slow for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import test_online_exact as ex

ONLINE = os.path.join(GOLDEN, "online")
QUERIES = ["q0", "q1", "q2", "q3", "q4"]
CLI = os.path.join(ROOT, "gnn-pe_amd", "gnnpe_main")
N_TRIALS = 12
KEEP = 0.75


# ---- yardsticks -----------------------------------------------------------------------------------------------------------

def _nx_embeddings(g, qpath):
    """every monomorphism of the query into the data graph as a row: column u = image of query vertex u"""
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
    rows = []
    for m in iso.GraphMatcher(D, Q, node_match=lambda a, b: a["l"] == b["l"]).subgraph_monomorphisms_iter():
        inv = {u: v for v, u in m.items()}
        rows.append([inv[u] for u in range(q["n"])])
    return np.array(rows, np.int64).reshape(len(rows), q["n"])


def _in_sets(bm, rows):
    """mask of the rows whose every image lies in its query vertex's set"""
    if len(rows) == 0:
        return np.zeros(0, bool)
    u = np.arange(rows.shape[1])[None, :]
    return (((bm[u, rows >> 5] >> (rows & 31).astype(np.uint32)) & 1) != 0).all(axis=1)


def _subset(bm, n, seed, keep=KEEP):
    """each C(u) thinned to a seeded random subset: every vertex kept with probability `keep`"""
    rng = np.random.default_rng(seed)
    drop = rng.random((bm.shape[0], n)) >= keep
    out = bm.copy()
    for u in range(bm.shape[0]):
        ids = np.nonzero(drop[u])[0]
        np.bitwise_and.at(out[u], ids >> 5, ~(np.uint32(1) << (ids & 31).astype(np.uint32)))
    return out


def _clear(bm, u, v):
    out = bm.copy()
    out[u, v >> 5] &= ~(np.uint32(1) << np.uint32(v & 31))
    return out


_CASES = {}


def _small_cases(tmp_path_factory):
    """the generator of test_gpu_exact_answers_equal_networkx: 12 G(60, 90..160) graphs with 3 labels, cut queries of 3-6
    vertices (query rng seed 21, graph seeds 500 + trial); with every case networkx's embeddings, the label/degree-only bitmap
    and its thinned copy (subset seeds 900 + trial)"""
    if "small" in _CASES:
        return _CASES["small"]
    from gnnpe_amd import synth
    cut_query = ex._cut_query()
    tmp = tmp_path_factory.mktemp("refine_sets")
    rng = np.random.default_rng(21)
    cases = []
    for trial in range(N_TRIALS):
        g = synth.gnm_graph(60, int(rng.integers(90, 160)), n_labels=3, seed=500 + trial)
        sn = rng.permutation(g["n"]).astype(np.uint32)
        qp = str(tmp / f"nq{trial}.graph")
        open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], int(rng.integers(3, 7)), rng))
        bm = ex._ld_bitmap(g, qp)
        cases.append(dict(g=g, sn=sn, qp=qp, emb=_nx_embeddings(g, qp), bm=bm, sub=_subset(bm, g["n"], 900 + trial)))
    _CASES["small"] = cases
    return cases


def _start_vertex(qpath, bm):
    """fewest candidates, ties to the larger degree, then the smaller id (host/refine.h)"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qpath)
    qd = np.diff(q["offsets"].astype(np.int64))
    cnt = np.array([sum(bin(int(w)).count("1") for w in bm[u]) for u in range(q["n"])])
    return min(range(q["n"]), key=lambda u: (cnt[u], -qd[u], u)), cnt


def _assert_rows_are_embeddings(g, qpath, bm, rows):
    """labels, degrees, edges, injective, inside the sets, pairwise different"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qpath)
    rows = np.asarray(rows, np.int64)
    assert rows.ndim == 2 and rows.shape[1] == q["n"]
    if len(rows) == 0:
        return
    n = len(g["labels"])
    assert rows.min() >= 0 and rows.max() < n
    deg = np.diff(g["offsets"].astype(np.int64))
    qd = np.diff(q["offsets"].astype(np.int64))
    assert (g["labels"][rows] == q["labels"][None, :]).all()
    assert (deg[rows] >= qd[None, :]).all()
    srt = np.sort(rows, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a row maps two query vertices onto one data vertex"
    assert _in_sets(bm, rows).all()
    offs = g["offsets"].astype(np.int64)
    keys = np.repeat(np.arange(n, dtype=np.int64), deg) * n + g["nbrs"].astype(np.int64)  # ascending: rows sorted by id
    for a in range(q["n"]):
        for b in q["nbrs"][q["offsets"][a]:q["offsets"][a + 1]]:
            if a < int(b):
                k = rows[:, a] * n + rows[:, int(b)]
                pos = np.searchsorted(keys, k)
                assert (pos < len(keys)).all() and (keys[np.minimum(pos, len(keys) - 1)] == k).all(), (a, int(b))
    assert len(np.unique(rows, axis=0)) == len(rows), "a row comes back twice"
    assert len(offs) == n + 1


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_complete_sets_equal_the_frozen_refinement_and_networkx(tmp_path_factory):
    """1. on the label/degree-only bitmap host_refine_sets == host_refine == the networkx monomorphism count"""
    from gnnpe_amd import binding
    counts = []
    for t, c in enumerate(_small_cases(tmp_path_factory)):
        want = len(c["emb"])
        assert binding.host_refine_sets(c["g"], c["qp"], c["bm"]) == want, t
        assert binding.host_refine(c["g"], c["qp"], c["bm"]) == want, t
        counts.append(want)
    assert len(counts) >= 12 and sum(counts) > 0 and sum(k > 0 for k in counts) * 2 >= len(counts), counts


def test_arbitrary_sets_count_the_embeddings_inside_them(tmp_path_factory):
    """2. each C(u) a random 3/4 subset of the label/degree set: host_refine_sets == the networkx monomorphisms whose every image
    lies in its set; in at least half of the trials that is non-zero and below the unrestricted count"""
    from gnnpe_amd import binding
    telling = 0
    for t, c in enumerate(_small_cases(tmp_path_factory)):
        want = int(_in_sets(c["sub"], c["emb"]).sum())
        assert binding.host_refine_sets(c["g"], c["qp"], c["sub"]) == want, t
        telling += 0 < want < len(c["emb"])
    assert telling * 2 >= N_TRIALS, telling


def test_limit_and_arguments(tmp_path_factory, tmp_path):
    """3. limit below, at and above the count, limit 0; a cleared image of a vertex that is not the start vertex lowers
    host_refine_sets and leaves host_refine alone; an empty set gives 0; a disconnected query and null arguments are refused"""
    from gnnpe_amd import binding
    cases = _small_cases(tmp_path_factory)
    c = max(cases, key=lambda c: len(c["emb"]))
    g, qp, bm, k = c["g"], c["qp"], c["bm"], len(c["emb"])
    assert k > 3
    for limit, want in ((1, 1), (k - 1, k - 1), (k, k), (k + 1, k), (10 * k, k), (0, 0)):
        assert binding.host_refine_sets(g, qp, bm, limit) == want, limit
    cleared = 0
    for c in cases:
        if len(c["emb"]) == 0:
            continue
        start, cnt = _start_vertex(c["qp"], c["bm"])
        f = c["emb"][0]
        for u in range(len(f)):
            if u == start or cnt[u] - 1 <= cnt[start]:
                continue
            bm2 = _clear(c["bm"], u, int(f[u]))
            assert _start_vertex(c["qp"], bm2)[0] == start
            lost = int((c["emb"][:, u] == f[u]).sum())
            assert lost >= 1
            assert binding.host_refine_sets(c["g"], c["qp"], bm2) == len(c["emb"]) - lost
            assert binding.host_refine(c["g"], c["qp"], bm2) == len(c["emb"])
            cleared += 1
            break
    assert cleared >= 3, cleared
    empty = bm.copy()
    empty[bm.shape[0] - 1] = 0
    assert binding.host_refine_sets(g, qp, empty) == 0
    disc = str(tmp_path / "disconnected.graph")
    ex._write_query(disc, 4, {(0, 1), (2, 3)}, [0, 0, 0, 0])
    with pytest.raises(binding.GnnpeError, match="not connected"):
        binding.host_refine_sets(g, disc, np.full((4, 2), 0xFFFFFFFF, np.uint32))
    import ctypes as C
    lib, out = binding.load_online(), C.c_uint64()
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.gnnpe_host_refine_sets(g["n"], p(o), p(nb), p(lb), qp.encode(), None, 10, C.byref(out)) != 0
    assert lib.gnnpe_host_refine_sets(g["n"], p(o), p(nb), p(lb), None, p(bm), 10, C.byref(out)) != 0
    assert lib.gnnpe_host_refine_sets(g["n"], p(o), p(nb), p(lb), qp.encode(), p(bm), 10, None) != 0
    assert lib.gnnpe_refine_sets(None, qp.encode(), p(bm), 10, C.byref(out), None, 0, None) != 0


def test_cli_refuses_refine_sets_where_the_sets_are_incomplete(tmp_path):
    """4. each refusal exits non-zero with its message before the graph is read or a GPU is touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2"]
    for extra, msg in ((["-m", "online", "--refine", "sets"], "--refine sets needs complete candidate sets"),
                       (["-m", "online", "-l", "2", "--refine", "sets"], "--refine sets needs complete candidate sets"),
                       (["-m", "online", "--exact", "--matches", str(tmp_path / "m.txt")], "--matches needs --refine sets"),
                       (["-m", "online", "--exact", "--refine", "start", "--matches", str(tmp_path / "m.txt")],
                        "--matches needs --refine sets"),
                       (["-m", "online", "--exact", "--refine", "waves"], "--refine must be start or sets"),
                       (["-m", "offline", "--refine", "sets"], "--refine sets applies to -m online only"),
                       (["-m", "filter", "--exact", "--refine", "sets"], "--refine sets applies to -m online only")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra
    assert not os.path.exists(str(tmp_path / "m.txt"))
    assert not os.path.exists(os.path.join(root, "gnn-pe", "all_paths.txt"))


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_small_graphs_equal_the_host_form_the_frozen_kernel_and_networkx(tmp_path_factory):
    """5. complete and thinned bitmaps: device == host form == networkx; exact filter output (l = 2, l = 3): == Engine.refine ==
    networkx"""
    from gnnpe_amd import binding
    for t, c in enumerate(_small_cases(tmp_path_factory)):
        g, qp = c["g"], c["qp"]
        eng = ex._engine(binding, g, c["sn"], 2)
        for name in ("bm", "sub"):
            want = int(_in_sets(c[name], c["emb"]).sum())
            assert binding.host_refine_sets(g, qp, c[name]) == want, (t, name)
            got, ms = eng.refine_sets(qp, c[name])
            assert got == want and ms >= 0, (t, name, got, want)
        for l in (2, 3):
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            assert eng.refine_sets(qp, bm)[0] == eng.refine(qp, bm)[0] == len(c["emb"]), (t, l)
        eng.close()


HUB_GRAPHS = (dict(n=2000, m=6000, max_degree=150, n_labels=4, seed=5),
              dict(n=20000, m=80000, max_degree=600, n_labels=8, seed=6))
HUB_LIMIT = 10 ** 7


def _hub_cases(tmp_path):
    """(graph, query path, bitmap) of test 6: five cut queries of 4-8 vertices per graph (query rng seeds 31, 32), each on the
    label/degree bitmap and on its 3/4 subset"""
    from gnnpe_amd import synth
    cut_query = ex._cut_query()
    for gi, spec in enumerate(HUB_GRAPHS):
        g = synth.powerlaw_graph(spec["n"], spec["m"], exponent=2.1, max_degree=spec["max_degree"], n_labels=spec["n_labels"],
                                 seed=spec["seed"])
        rng = np.random.default_rng(31 + gi)
        for k in range(5):
            qp = str(tmp_path / f"hq{gi}_{k}.graph")
            open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], 4 + k, rng))
            bm = ex._ld_bitmap(g, qp)
            yield gi, g, qp, bm, _subset(bm, g["n"], 900 + k)


@pytest.mark.gpu
def test_gpu_hub_rows_at_every_depth(tmp_path):
    """6. power-law graphs, rows longer than 64 at every level of the search: powerlaw_graph(2000, 6000, max_degree=150,
    n_labels=4, seed=5) (23 rows longer than 64) and powerlaw_graph(20000, 80000, max_degree=600, n_labels=8, seed=6) (300 such
    rows, the longest 628).  Cut queries of 4-8 vertices, limit 10^7: on one core the host form takes at most 0.2 s per query on
    the first graph and at most 7.4 s on the second (its 8-vertex query; every other one below 0.6 s); 7 of the 10 complete-set
    counts and 8 of the 10 subset counts stay below the limit.  Device == host form, and some query's matches hold a vertex of
    degree > 64."""
    from gnnpe_amd import binding
    eng, at, below, hub_in_matches = None, -1, 0, False
    for gi, g, qp, bm, sub in _hub_cases(tmp_path):
        deg = np.diff(g["offsets"].astype(np.int64))
        if gi != at:
            assert (deg > 64).sum() >= 10
            if eng:
                eng.close()
            from gnnpe_amd import synth
            eng, at = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2), gi
        for name, b in (("complete", bm), ("subset", sub)):
            want = binding.host_refine_sets(g, qp, b, HUB_LIMIT)
            got, ms, rows = eng.refine_sets(qp, b, limit=HUB_LIMIT, matches_cap=1 << 16)
            print(f"hub graph {gi} {os.path.basename(qp)} {name}: {got} embeddings, {ms:.3f} ms")
            assert got == want, (gi, qp, name, got, want)
            assert len(rows) == min(got, 1 << 16)
            _assert_rows_are_embeddings(g, qp, b, rows)
            hub_in_matches |= bool(len(rows)) and bool((deg[rows.astype(np.int64)] > 64).any())
            below += want < HUB_LIMIT
    eng.close()
    assert hub_in_matches and below >= 10


@pytest.mark.gpu
def test_gpu_matches_are_the_embeddings(tmp_path_factory):
    """7. matches_cap above the count: the rows are networkx's set; below it: exactly matches_cap valid, different rows and the
    full count"""
    from gnnpe_amd import binding
    capped = 0
    for t, c in enumerate(_small_cases(tmp_path_factory)):
        g, qp = c["g"], c["qp"]
        eng = ex._engine(binding, g, c["sn"], 2)
        for name in ("bm", "sub"):
            emb = c["emb"][_in_sets(c[name], c["emb"])]
            got, _, rows = eng.refine_sets(qp, c[name], matches_cap=len(emb) + 7)
            assert got == len(emb) == len(rows), (t, name)
            _assert_rows_are_embeddings(g, qp, c[name], rows)
            assert set(map(tuple, rows.tolist())) == set(map(tuple, emb.tolist())), (t, name)
            if len(emb) >= 2:
                cap = len(emb) // 2
                got, _, rows = eng.refine_sets(qp, c[name], matches_cap=cap)
                assert got == len(emb) and len(rows) == cap, (t, name, got, len(rows))
                _assert_rows_are_embeddings(g, qp, c[name], rows)
                assert set(map(tuple, rows.tolist())) <= set(map(tuple, emb.tolist())), (t, name)
                capped += 1
        eng.close()
    assert capped >= N_TRIALS


@pytest.mark.gpu
def test_gpu_limit_and_repeated_calls(tmp_path_factory):
    """8. a limit below the count returns exactly the limit (matches_cap above the limit is the limit); a repeated call on the
    same context returns the same answer"""
    from gnnpe_amd import binding
    cases = _small_cases(tmp_path_factory)
    c = max(cases, key=lambda c: len(c["emb"]))
    g, qp, bm, k = c["g"], c["qp"], c["bm"], len(c["emb"])
    assert k > 3
    eng = ex._engine(binding, g, c["sn"], 2)
    for limit, want in ((1, 1), (k - 1, k - 1), (k, k), (k + 1, k), (0, 0)):
        for _ in range(2):
            assert eng.refine_sets(qp, bm, limit=limit)[0] == want, limit
    got, _, rows = eng.refine_sets(qp, bm, limit=3, matches_cap=100)
    assert got == 3 and len(rows) == 3
    _assert_rows_are_embeddings(g, qp, bm, rows)
    for _ in range(3):
        assert eng.refine_sets(qp, bm)[0] == k
        assert eng.refine_sets(qp, c["sub"])[0] == int(_in_sets(c["sub"], c["emb"]).sum())
    empty = bm.copy()
    empty[bm.shape[0] - 1] = 0
    assert eng.refine_sets(qp, empty)[0] == 0
    eng.close()
    # a power-law graph and a count of 435 924, where waves pass 1024 finds inside one item: still exactly the limit, twice
    from gnnpe_amd import synth
    spec = HUB_GRAPHS[0]
    g = synth.powerlaw_graph(spec["n"], spec["m"], exponent=2.1, max_degree=spec["max_degree"], n_labels=spec["n_labels"],
                             seed=spec["seed"])
    tmp = tmp_path_factory.mktemp("limit")
    qp = str(tmp / "hq.graph")
    open(qp, "w").write(ex._cut_query()(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], 5, np.random.default_rng(31)))
    bm = ex._ld_bitmap(g, qp)
    full = binding.host_refine_sets(g, qp, bm, HUB_LIMIT)
    assert full > 5000
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    for _ in range(2):
        assert eng.refine_sets(qp, bm, limit=5000)[0] == 5000
        assert eng.refine_sets(qp, bm, limit=HUB_LIMIT)[0] == full
    eng.close()


@pytest.mark.gpu
def test_gpu_test_graph_golden_exact_answers(test_graph):
    """9. q0-q4, l = 2 exact and l = 3: refine_sets == the "exact" value of tests/golden/online/exact_answers.json"""
    from gnnpe_amd import binding
    g = test_graph
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    eng = ex._engine(binding, g, g["sorted_nodes"], 2)
    for name in QUERIES:
        qp = os.path.join(ONLINE, f"{name}.graph")
        for l in (2, 3):
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            assert eng.refine_sets(qp, bm)[0] == rec[name]["exact"], (name, l)
    eng.close()


@pytest.mark.gpu
def test_gpu_scale_equals_the_frozen_kernel_and_finds_the_cut(tmp_path):
    """10. 1M vertices / 10M edges, the three cut queries of test_gpu_exact_scale_cut_sources_are_candidates: on the exact bitmaps
    refine_sets == refine (both under a finite limit), and the tuple the query was cut from is among the matches"""
    from gnnpe_amd import binding, synth
    g = synth.gnm_graph(1_000_000, 10_000_000)
    sn = synth.degree_order(g["offsets"])
    eng = ex._engine(binding, g, sn, 2)
    rng = np.random.default_rng(11)
    offs = g["offsets"].astype(np.int64)
    limit, cap, found_src = 10 ** 7, 1 << 16, 0
    for k, size in enumerate((6, 8, 10)):
        edges, labels, src = ex._cut_with_sources(offs, g["nbrs"], g["labels"], size, rng)
        qp = str(tmp_path / f"big{k}.graph")
        ex._write_query(qp, size, edges, labels)
        for l in (2, 3):
            bm, _ = eng.filter_candidates_exact(binding.host_query_plan_exact(qp, 2, l))
            got, ms, rows = eng.refine_sets(qp, bm, limit=limit, matches_cap=cap)
            want, ms0 = eng.refine(qp, bm, limit=limit)
            print(f"scale query {size} l={l}: {got} embeddings, sets {ms:.3f} ms, start {ms0:.3f} ms")
            assert got == want >= 1, (size, l, got, want)
            if got < cap:
                assert tuple(src) in set(map(tuple, rows.tolist())), (size, l)
                found_src += 1
    eng.close()
    assert found_src >= 1


@pytest.mark.gpu
def test_gpu_cli_refine_sets_and_matches(tmp_path, test_graph):
    """11. gnnpe_main -m online --exact / -l 3 with --refine sets: the golden exact count, --matches writes that many distinct
    valid lines, --refine start prints the same count and its old JSON line"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    for name in ("q0", "q3"):
        qp = os.path.join(ONLINE, f"{name}.graph")
        want = rec[name]["exact"]
        base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--timing"]
        for extra in (["--exact"], ["-l", "3"]):
            mf = str(tmp_path / f"{name}_{len(extra)}.txt")
            r = subprocess.run(base + extra + ["--refine", "sets", "--matches", mf], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            assert f"Answer Number: {want} " in r.stdout, (extra, r.stdout)
            t = json.loads(r.stderr.strip().splitlines()[-1])
            assert t["refine"] == "sets" and t["matches_written"] == min(want, 1 << 20) and t["exact"] is True
            rows = np.loadtxt(mf, dtype=np.int64, ndmin=2) if want else np.zeros((0, 1), np.int64)
            assert len(rows) == min(want, 1 << 20)
            if want:
                _assert_rows_are_embeddings(test_graph, qp, ex._ld_bitmap(test_graph, qp), rows)
            r = subprocess.run(base + extra + ["--refine", "start"], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and f"Answer Number: {want} " in r.stdout, (extra, r.stdout, r.stderr)
            t = json.loads(r.stderr.strip().splitlines()[-1])
            assert "refine" not in t and "matches_written" not in t
        # -n below the count: the answer and the file stop at it
        if want > 2:
            mf = str(tmp_path / f"{name}_n.txt")
            r = subprocess.run(base + ["--exact", "--refine", "sets", "--matches", mf, "-n", "2"], capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0 and "Answer Number: 2 " in r.stdout, r.stderr
            assert len(open(mf).read().splitlines()) == 2
