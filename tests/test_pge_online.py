"""GNN-PGE online (GNN-PGE/src/main.cpp:197-361): the query vertices' path groups on the host, the leaf test of
Partition::query (custom.h:327-374) over every data vertex on the GPU, and `gnnpge_main -m online / -m filter`.

The numpy leaf test below is the restatement everything is checked against; it is pinned to the reference by running the
reference's own refinement (oracle/_ref/ref_online ... refine) on the sets it gives for the reference's own data."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gnnpe_amd import binding, synth
from oracle import bitmap_to_sets, ref_online_path

CLI = os.path.join(ROOT, "gnn-pe_amd", "gnnpge_main")
DATA_GRAPH = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
GOLD = json.load(open(os.path.join(GOLDEN, "pge_online.json")))
QUERIES = {name: os.path.join(GOLDEN, rel) for name, rel in GOLD["queries"].items()}


def leaf_bitmap(labels, degrees, pg, plg, q):
    """custom.h:335-367 applied to every data vertex: bitmap [n_query_vertices x ceil(n/32)] uint32, bit v of row u = v is a
    candidate of u.  Exact comparisons, inclusive bounds, written as the reference's rejections."""
    n = len(labels)
    words = (n + 31) // 32
    out = np.zeros((len(q["labels"]), words), np.uint32)
    shifts = np.arange(32, dtype=np.uint64)
    for u in range(len(q["labels"])):
        idx = np.flatnonzero((labels == q["labels"][u]) & (degrees >= q["degrees"][u]))
        g, lg = pg[idx], plg[idx]
        qg, qlg = q["pg"][u], q["plg"][u]
        bad = (lg[:, 1::2] < qlg[0::2]).any(1) | (lg[:, 0::2] > qlg[1::2]).any(1) | (g[:, 1::2] < qg[0::2]).any(1)
        mask = np.zeros(words * 32, bool)
        mask[idx[~bad]] = True
        out[u] = (mask.reshape(words, 32).astype(np.uint64) << shifts).sum(1).astype(np.uint32)
    return out


def write_candidates(path, sets):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(sets)))
        for s in sets:
            f.write(struct.pack("<I", len(s)))
            f.write(np.asarray(s, "<u4").tobytes())


def read_candidates(path):
    b = open(path, "rb").read()
    nq, off, out = struct.unpack_from("<I", b, 0)[0], 4, []
    for _ in range(nq):
        c = struct.unpack_from("<I", b, off)[0]
        out.append(np.frombuffer(b, "<u4", c, off + 4).copy())
        off += 4 + 4 * c
    assert off == len(b)
    return out


def cut_query(g, seed_vertex, k, path):
    """A connected query of up to k vertices cut from data graph g (BFS from seed_vertex, induced edges), written to path.
    Returns the data vertex behind every query vertex."""
    offs, nbrs = g["offsets"], g["nbrs"]
    picked, frontier = [int(seed_vertex)], [int(seed_vertex)]
    while frontier and len(picked) < k:
        v = frontier.pop(0)
        for w in nbrs[offs[v]:offs[v + 1]][:3]:
            if int(w) not in picked and len(picked) < k:
                picked.append(int(w))
                frontier.append(int(w))
    pos = {v: i for i, v in enumerate(picked)}
    edges = sorted({(min(pos[v], pos[int(w)]), max(pos[v], pos[int(w)]))
                    for v in picked for w in nbrs[offs[v]:offs[v + 1]] if int(w) in pos})
    eu = np.array([a for a, _ in edges], np.int64)
    ev = np.array([b for _, b in edges], np.int64)
    deg = np.bincount(np.concatenate([eu, ev]), minlength=len(picked))
    qoffs = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    synth.write_graph_file(path, dict(n=len(picked), m=len(edges), offsets=qoffs, labels=g["labels"][picked], eu=eu, ev=ev))
    return np.array(picked)


def pge_dataset(root, p):
    """<root>/gnn-pge/ as the prep step leaves it for the Test graph: partition directories and membership.txt (degree order,
    partitions alternating), as tests/golden/make_golden_pge_online.py made them for the reference."""
    deg = np.array([int(l.split()[3]) for l in open(DATA_GRAPH) if l.startswith("v")])
    n = len(deg)
    mem = np.zeros(n, np.uint32) if p == 1 else (np.arange(n) % p).astype(np.uint32)
    for i in range(p):
        os.makedirs(os.path.join(root, "gnn-pge", "partitions", f"partition-{i}"), exist_ok=True)
    synth.write_membership(os.path.join(root, "gnn-pge", "membership.txt"), np.argsort(deg, kind="stable").astype(np.uint32), mem)
    return root + "/"


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


# ---- CPU --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e", [1, 2, 4, 8])
def test_host_query_groups_equal_oracle(oracle, e):
    """main.cpp:253-329 is the data side's construction on the query graph: oracle.pge_groups restates it."""
    for name, path in QUERIES.items():
        q = binding.host_pge_query_groups(path, e)
        offs, nbrs, labels, meta = oracle.load_graph(path)
        x, _, vde = oracle.gen_vde(offs, nbrs, labels, e)
        pg, plg = oracle.pge_groups(offs, nbrs, e, x, vde)
        assert q["n_vertices"] == meta["n"] and np.array_equal(q["labels"], labels), name
        assert np.array_equal(q["degrees"], np.diff(offs)), name
        assert q["pg"].shape == (meta["n"], 4 * e)
        assert np.array_equal(q["pg"], pg) and np.array_equal(q["plg"], plg), name


def test_host_query_groups_refuse_isolated_vertex(tmp_path):
    p = tmp_path / "iso.graph"
    p.write_text("t 3 1\nv 0 0 1\nv 1 1 1\nv 2 0 0\ne 0 1\n")
    with pytest.raises(binding.GnnpeError, match=r"\[-3\].*query vertex 2 has no edge"):
        binding.host_pge_query_groups(str(p), 2)


def test_leaf_test_on_reference_data_gives_reference_answers(tmp_path):
    """The numpy leaf test over the reference's own data_vertices.bin fields (pge_test_graph_e2.npz) yields candidate sets on
    which the reference's refinement prints the reference's answer for every query."""
    if not os.path.exists(ref_online_path()):
        pytest.skip("oracle/_ref/ref_online not built")
    z = np.load(os.path.join(GOLDEN, "pge_test_graph_e2.npz"))
    n = len(z["vid"])
    for name, path in QUERIES.items():
        bm = leaf_bitmap(z["label"], z["degree"], z["pg"], z["plg"], binding.host_pge_query_groups(path, 2))
        cand = str(tmp_path / f"{name}.bin")
        write_candidates(cand, bitmap_to_sets(bm, n))
        out = subprocess.check_output([ref_online_path(), str(tmp_path) + "/", DATA_GRAPH, path, "1", "refine", cand], text=True,
                                      timeout=600)
        assert int(re.search(r"Answer Num\w*: (\d+)", out).group(1)) == GOLD["p1"][name], (name, out)


def _write_test_bin(oracle, path, e, labels=None):
    offs, nbrs, lab, _meta = oracle.load_graph(DATA_GRAPH)
    lab = lab if labels is None else labels
    x, nx, vde = oracle.gen_vde(offs, nbrs, lab, e)
    pg, plg = oracle.pge_groups(offs, nbrs, e, x, vde)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    oracle.pge_write_bin(path, e, offs, lab, x, nx, vde, pg, plg)


def test_cli_refuses_missing_or_foreign_bin_before_the_gpu(oracle, tmp_path):
    """A missing data_vertices.bin, one written at another -e and one written for another graph are refused with a message,
    before any GPU call (so the message is the same on a machine without one)."""
    root = pge_dataset(str(tmp_path), 1)
    binp = os.path.join(root, "gnn-pge", "data_vertices.bin")
    q = QUERIES["qg"]
    r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", q, "-m", "online")
    assert r.returncode != 0 and "data_vertices.bin" in r.stderr and "cannot open" in r.stderr, r.stderr
    _write_test_bin(oracle, binp, 2)
    r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", q, "-m", "online", "-e", "4")
    assert r.returncode != 0 and "another graph or another -e" in r.stderr, r.stderr
    _, _, lab, _ = oracle.load_graph(DATA_GRAPH)
    _write_test_bin(oracle, binp, 2, labels=np.roll(lab, 1))  # same size, other labels
    r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", q, "-m", "filter")
    assert r.returncode != 0 and "does not match the data graph" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(root, "gnn-pge", "candidates.bin"))


def test_cli_refuses_isolated_query_vertex(oracle, tmp_path):
    root = pge_dataset(str(tmp_path), 1)
    _write_test_bin(oracle, os.path.join(root, "gnn-pge", "data_vertices.bin"), 2)
    p = tmp_path / "iso.graph"
    p.write_text("t 3 1\nv 0 0 1\nv 1 1 1\nv 2 0 0\ne 0 1\n")
    r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", str(p), "-m", "online")
    assert r.returncode != 0 and "query vertex 2 has no edge" in r.stderr, r.stderr


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _engine(offs, nbrs, labels, e, n_labels):
    eng = binding.Engine(0)
    eng.load_csr(offs, nbrs, labels)
    eng.set_label_table(binding.host_label_table(n_labels, e))
    return eng


@pytest.mark.gpu
def test_gpu_filter_test_graph_both_group_sources(test_graph):
    z = np.load(os.path.join(GOLDEN, "pge_test_graph_e2.npz"))
    offs, nbrs, labels = test_graph["offsets"], test_graph["nbrs"], test_graph["labels"]
    deg = np.diff(offs).astype(np.uint32)
    n_labels = test_graph["meta"]["labels_count"]
    computed = _engine(offs, nbrs, labels, 2, n_labels)
    computed.vde()
    pg, plg = computed.pge_groups()
    from_file = _engine(offs, nbrs, labels, 2, n_labels)
    from_file.pge_set_groups(z["pg"], z["plg"])
    try:
        for name, path in QUERIES.items():
            q = binding.host_pge_query_groups(path, 2)
            want = leaf_bitmap(labels, deg, z["pg"], z["plg"], q)
            assert np.array_equal(leaf_bitmap(labels, deg, pg, plg, q), want), name
            for eng in (computed, from_file):
                bm, ms = eng.pge_filter_candidates(q)
                assert bm.shape == want.shape and np.array_equal(bm, want), name
                assert ms > 0
    finally:
        computed.close()
        from_file.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,m,e", [("gnm", 5003, 30011, 1), ("gnm", 5003, 30011, 2), ("gnm", 4001, 20000, 3),
                                        ("powerlaw", 20011, 150000, 4), ("powerlaw", 20011, 150000, 8),
                                        ("gnm", 97, 400, 8)])
def test_gpu_filter_random_graphs(tmp_path, kind, n, m, e):
    n_labels = 6
    g = synth.gnm_graph(n, m, n_labels=n_labels, seed=11) if kind == "gnm" else \
        synth.powerlaw_graph(n, m, max_degree=1500, n_labels=n_labels, seed=12)
    deg = np.diff(g["offsets"]).astype(np.uint32)
    if kind == "powerlaw":
        assert deg.max() > 64  # hub rows
    eng = _engine(g["offsets"], g["nbrs"], g["labels"], e, n_labels)
    try:
        eng.vde()
        pg, plg = eng.pge_groups()
        rng = np.random.default_rng(e)
        for t, k in enumerate((2, 4, 7)):
            seed_v = int(rng.choice(np.flatnonzero(deg >= 2)))
            qp = str(tmp_path / f"q{t}.graph")
            picked = cut_query(g, seed_v, k, qp)
            q = binding.host_pge_query_groups(qp, e)
            want = leaf_bitmap(g["labels"], deg, pg, plg, q)
            bm, ms = eng.pge_filter_candidates(q)
            assert np.array_equal(bm, want), (kind, n, e, t)
            sets = bitmap_to_sets(bm, n)
            # the filter is sound: the vertices the query was cut from are candidates of their query vertices
            assert all(v in set(s.tolist()) for v, s in zip(picked, sets)), (kind, e, t)
            if n % 32:
                assert not np.any(bm[:, -1] >> np.uint32(n % 32))  # no bits >= n
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("e", [2, 3])
def test_gpu_filter_bounds_are_inclusive_and_exact(e):
    """Query groups crafted from one data vertex' own bounds: equal bounds accept it, one ulp past rejects it."""
    g = synth.gnm_graph(3001, 15000, n_labels=4, seed=5)
    deg = np.diff(g["offsets"]).astype(np.uint32)
    eng = _engine(g["offsets"], g["nbrs"], g["labels"], e, 4)
    try:
        eng.vde()
        pg, plg = eng.pge_groups()
        v = int(np.flatnonzero(deg >= 3)[7])
        D = 2 * e
        base_pg = np.zeros(4 * e)
        base_pg[0::2] = pg[v, 1::2]  # lo = v's hi: pg_v[2k+1] >= pg_u[2k] holds with equality
        base_pg[1::2] = pg[v, 1::2] + 1.0
        base_plg = plg[v].copy()     # plg_v[2k+1] >= plg_u[2k] and plg_v[2k] <= plg_u[2k+1], with equality
        rows = []                    # (pg, plg, degree, v accepted?)
        rows.append((base_pg, base_plg, deg[v], True))
        rows.append((base_pg, base_plg, deg[v] + 1, False))
        for k in (0, D - 1):
            a = base_pg.copy()
            a[2 * k] = np.nextafter(a[2 * k], np.inf)
            rows.append((a, base_plg, deg[v], False))
            b = base_plg.copy()
            b[2 * k] = np.nextafter(plg[v, 2 * k + 1], np.inf)  # query lo one ulp above v's hi
            rows.append((base_pg, b, deg[v], False))
            c = base_plg.copy()
            c[2 * k + 1] = np.nextafter(plg[v, 2 * k], -np.inf)  # query hi one ulp below v's lo
            rows.append((base_pg, c, deg[v], False))
            d = base_plg.copy()
            d[2 * k], d[2 * k + 1] = plg[v, 2 * k + 1], plg[v, 2 * k]  # a point at v's hi, and a query hi at v's lo
            rows.append((base_pg, d, deg[v], plg[v, 2 * k] <= plg[v, 2 * k + 1]))
        q = dict(labels=np.full(len(rows), g["labels"][v], np.uint32), degrees=np.array([r[2] for r in rows], np.uint32),
                 pg=np.stack([r[0] for r in rows]), plg=np.stack([r[1] for r in rows]))
        bm, _ = eng.pge_filter_candidates(q)
        assert np.array_equal(bm, leaf_bitmap(g["labels"], deg, pg, plg, q))
        got = [(bm[u, v // 32] >> np.uint32(v % 32)) & 1 for u in range(len(rows))]
        assert got == [int(r[3]) for r in rows], got
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("p", [1, 2])
def test_gpu_cli_online_answers_and_filter_file(tmp_path, p):
    root = pge_dataset(str(tmp_path), p)
    r = run_cli("-f", root, "-d", DATA_GRAPH, "-m", "offline", "-p", str(p))
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(os.path.join(root, "gnn-pge", "candidates.bin"))
    for name, path in QUERIES.items():
        r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", path, "-m", "online", "-p", str(p), "--timing")
        assert r.returncode == 0, r.stderr
        assert re.fullmatch(r"Answer Num: (\d+) Query Time \(ms\): \S+\n", r.stdout), r.stdout
        assert int(re.search(r"Answer Num: (\d+)", r.stdout).group(1)) == GOLD[f"p{p}"][name], (name, r.stdout)
        t = json.loads(r.stderr.strip().splitlines()[-1])
        assert t["filter_device_ms"] > 0 and t["refine_ms"] >= 0 and t["end_to_end_s"] > 0
    cap = GOLD["capped"]
    r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", QUERIES[cap["query"]], "-m", "online", "-p", str(p), "-n", str(cap["n"]))
    assert r.returncode == 0 and int(re.search(r"Answer Num: (\d+)", r.stdout).group(1)) == cap["answer_num"], r.stdout
    z = np.load(os.path.join(GOLDEN, "pge_test_graph_e2.npz"))
    for name in ("qg", "q3"):
        r = run_cli("-f", root, "-d", DATA_GRAPH, "-q", QUERIES[name], "-m", "filter", "-p", str(p))
        assert r.returncode == 0 and r.stdout == "", (r.stdout, r.stderr)
        got = read_candidates(os.path.join(root, "gnn-pge", "candidates.bin"))
        want = bitmap_to_sets(leaf_bitmap(z["label"], z["degree"], z["pg"], z["plg"], binding.host_pge_query_groups(QUERIES[name], 2)),
                              len(z["vid"]))
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), name
    # the online mode writes nothing under partitions/ beyond what -m offline left
    for i in range(p):
        assert sorted(os.listdir(os.path.join(root, "gnn-pge", "partitions", f"partition-{i}"))) == ["index.dat"]


@pytest.mark.gpu
def test_gpu_filter_1m_vertices(tmp_path):
    g = synth.gnm_graph(1_000_000, 10_000_000)
    n = g["n"]
    deg = np.diff(g["offsets"]).astype(np.uint32)
    eng = _engine(g["offsets"], g["nbrs"], g["labels"], 2, 64)
    try:
        eng.vde()
        pg, plg = eng.pge_groups()
        qp = str(tmp_path / "q.graph")
        cut_query(g, int(np.flatnonzero(deg >= 3)[0]), 6, qp)
        q = binding.host_pge_query_groups(qp, 2)
        want = leaf_bitmap(g["labels"], deg, pg, plg, q)
        times = []
        for _ in range(3):
            bm, ms = eng.pge_filter_candidates(q)
            assert np.array_equal(bm, want)
            assert ms > 0
            times.append(ms)
        print(f"pge filter, {n} vertices / {g['m']} edges, e = 2, {len(q['labels'])} query vertices, "
              f"{int(np.unpackbits(want.view(np.uint8)).sum())} candidates: device ms {times}")
    finally:
        eng.close()
