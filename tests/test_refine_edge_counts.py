"""Per-edge match counts (include/gnnpe_online.h, ABI version 14): E_m(C)[k][j] = the matches of mode m that send query edge
k = (a_k, b_k) onto adjacency entry j = (f(a_k) -> f(b_k)) of the data CSR, on the host (gnnpe_host_refine_sets_edge_counts), on the
device (gnnpe_refine_sets_edge_counts) and through `gnnpe_main --edge-counts`.

The host form is held to yardsticks that are not the library first: np.add.at over networkx's rows, every (f(a_k), f(b_k)) turned
into its CSR index by searchsorted; the marginals, which must be rows of the per-vertex table; closed forms on H1; the guard.  The
same shapes are run again with the query's vertex ids REVERSED (u -> nq-1-u) and the sets moved with them, which puts b_k in
front of a_k in the matching order: only that tells a wrong `flip` from a right one, since a symmetric query in mode 0 has
E[k][x->y] == E[k][y->x].  The device
is then held to the host form cell for cell -- at every first-level chunk width, with the reversed files, at 1, 2, 8 and 32 query
vertices, around the guard, on the fuzz cases -- to np.add.at over the rows the device itself hands back, and to the per-vertex
kernel through the marginals.  star5 on H1 holds 4 596 520 344 maps, which no host form walks inside a test: its closed form,
E[(0,i)][x->y] = (d_x-1)(d_x-2)(d_x-3), is checked on the device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_distinct as rd
import test_refine_induced as ri
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = ((False, False), (True, False), (False, True), (True, True))  # (distinct, induced): 0, DISTINCT, INDUCED, both
REV_SHAPES = ("wedge", "triangle", "C4", "diamond")  # the reversed-id files the device runs


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _csr_keys(g):
    """x * n + y of every adjacency entry x -> y in CSR order: ascending, since the rows ascend"""
    n = len(g["labels"])
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    return src, src * n + g["nbrs"].astype(np.int64)


def _reverse_index(g):
    """rev[j] = the index of entry y -> x for j = x -> y"""
    n = len(g["labels"])
    src, keys = _csr_keys(g)
    rev = np.searchsorted(keys, g["nbrs"].astype(np.int64) * n + src)
    assert np.array_equal(keys[rev], g["nbrs"].astype(np.int64) * n + src)
    return rev


def _edges_of(name, reverse=False):
    """the sorted (a, b), a < b, of a shape, or of the shape with its vertex ids reversed"""
    nq, edges = sh.SHAPES[name]
    if reverse:
        edges = [(nq - 1 - a, nq - 1 - b) for a, b in edges]
    return sorted((min(a, b), max(a, b)) for a, b in edges)


def _table(g, rows, edges):
    """the yardstick: for every row and every query edge k = (a, b), 1 added to cell [k][index of row[a] -> row[b]]"""
    n = len(g["labels"])
    _, keys = _csr_keys(g)
    t = np.zeros((len(edges), len(keys)), np.uint64)
    rows = np.asarray(rows, np.int64)
    for k, (a, b) in enumerate(edges):
        if len(rows):
            want = rows[:, a] * n + rows[:, b]
            j = np.searchsorted(keys, want)
            assert np.array_equal(keys[j], want)
            np.add.at(t[k], j, np.uint64(1))
    return t


def _marginals(g, t, edges, nq):
    """{(u, k): the per-vertex row the edge table's row k implies for query vertex u}: sums over the entries of a data row
    for u = a_k, over the entries with nbrs[j] = y for u = b_k"""
    n = len(g["labels"])
    src, _ = _csr_keys(g)
    out = {}
    for k, (a, b) in enumerate(edges):
        for u, idx in ((a, src), (b, g["nbrs"].astype(np.int64))):
            m = np.zeros(n, np.uint64)
            np.add.at(m, idx, t[k])
            out[u, k] = m
    return out


def _reversed_file(tmp, name, variant):
    """the shape with vertex u renamed nq-1-u, labels moving with the vertices"""
    nq, edges = sh.SHAPES[name]
    labels = [0] * nq if variant == 0 else [i % 2 for i in range(nq)]
    p = str(tmp / f"rev_{name}_{variant}.graph")
    ex._write_query(p, nq, {(min(nq - 1 - a, nq - 1 - b), max(nq - 1 - a, nq - 1 - b)) for a, b in edges}, labels[::-1])
    return p


_PAIRS = {}


def _pairs(qp):
    from gnnpe_amd import binding
    if qp not in _PAIRS:
        _PAIRS[qp] = binding.host_query_symmetry(qp)[1]
    return _PAIRS[qp]


def _check_host_case(binding, g, qp, name, reverse, bm, emb, ind, where):
    """the four modes of one (graph, query file, bitmap): table == yardstick, rows sum to the host count, marginals == per-vertex
    table.  Returns whether a mode-0 or DISTINCT table has E[k][x->y] != E[k][y->x] somewhere"""
    nq = sh.SHAPES[name][0]
    edges = _edges_of(name, reverse)
    assert [tuple(e) for e in binding.host_query_edges(qp).tolist()] == edges, where
    rev = _reverse_index(g)
    skew = False
    for distinct, induced in MODES:
        rows = ind if induced else emb
        rows = rows[rs._in_sets(bm, rows)]
        if distinct:
            rows = rows[rd._ordered(rows, _pairs(qp))]
        ans, complete, t = binding.host_refine_sets_edge_counts(g, qp, bm, FULL, distinct=distinct, induced=induced)
        w = where + (distinct, induced)
        assert complete and ans == len(rows) == binding.host_refine_sets(g, qp, bm, FULL, distinct=distinct, induced=induced), w
        assert t.dtype == np.uint64 and t.shape == (len(edges), len(g["nbrs"])) and np.array_equal(t, _table(g, rows, edges)), w
        assert (t.sum(axis=1) == ans).all(), w
        v = binding.host_refine_sets_vertex_counts(g, qp, bm, FULL, distinct=distinct, induced=induced)[2]
        for (u, k), m in _marginals(g, t, edges, nq).items():
            assert np.array_equal(m, v[u]), w + (u, k)
        if not induced:
            skew |= bool((t != t[:, rev]).any())
    return skew


_H1E = {}


def _h1_tables(tmp_path_factory):
    """the host form's (answers, table) of every H1 shape on every bitmap in every mode, limit 2^64 - 1, computed once"""
    if _H1E:
        return _H1E
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    for name in sh.H1_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                ans, complete, t = binding.host_refine_sets_edge_counts(h["g"], h["q"][name], h["bm"][name][b], FULL,
                                                                        distinct=distinct, induced=induced)
                assert complete
                _H1E[name, b, distinct, induced] = (ans, t)
    return _H1E


_H1R = {}


def _h1_reversed(tmp_path_factory):
    """H1 with the reversed-id files of REV_SHAPES on two bitmaps: label/degree, and label/degree with the set of the LAST query
    vertex cut to an eighth (seed 1900 + shape), so that the matching order starts there and every other vertex, of a smaller id,
    comes later -- with one label the four shapes are their own reversals, and it is the sets that move b_k in front of a_k.
    Per (shape, bitmap): the query file, the bitmap and the host form's (answers, table) per mode"""
    if _H1R:
        return _H1R
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("h1rev")
    for k, name in enumerate(REV_SHAPES):
        qp = _reversed_file(tmp, name, 0)
        ld = ex._ld_bitmap(h["g"], qp)
        last = ld.copy()
        last[-1:] = rs._subset(ld[-1:], h["g"]["n"], 1900 + k, keep=0.125)
        sizes = [len(sh._members(row, h["g"]["n"])) for row in last]
        assert 0 < sizes[-1] < min(sizes[:-1]) and rs._start_vertex(qp, last)[0] == len(sizes) - 1, (name, sizes)
        for b, bm in (("ld", ld), ("last", last)):
            tabs = {}
            for distinct, induced in MODES:
                ans, complete, t = binding.host_refine_sets_edge_counts(h["g"], qp, bm, FULL, distinct=distinct, induced=induced)
                assert complete
                tabs[distinct, induced] = (ans, t)
            _H1R[name, b] = dict(qp=qp, bm=bm, tabs=tabs)
    return _H1R


@pytest.fixture()
def ecount_lines(monkeypatch, capfd):
    """as sh.sets_lines, for the `[refine_ecount]` lines: the first line of a call has `edges`, the second `finds`"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [{k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])}
                for ln in err.splitlines() if ln.startswith("[refine_ecount] ")]
    return take


# ---- CPU: the host form against yardsticks that are not the library ----------------------------------------------------------

def test_host_table_against_networkx(tmp_path_factory):
    """1. the 15 small graphs, the eight shapes of ri.IND_SHAPES, both label variants, the three bitmaps, the four modes: the host
    table is np.add.at over networkx's rows (inside the sets, induced for INDUCED, filtered by the ordering pairs for DISTINCT) with
    every (f(a_k), f(b_k)) turned into its CSR index by searchsorted; every row sums to the host count of the mode; the two
    marginals of every row are rows a_k and b_k of host_refine_sets_vertex_counts; host_query_edges is the sorted edge list"""
    from gnnpe_amd import binding
    cases = ri._ind_cases(tmp_path_factory)
    assert len(cases) == 15 * len(ri.IND_SHAPES) * 2
    for c in cases:
        for b in sh.BITMAPS:
            _check_host_case(binding, c["g"], c["qp"], c["name"], False, c[b], c["emb"], c["ind"], (c["gi"], c["name"], c["variant"], b))


def test_host_table_with_reversed_vertex_ids(tmp_path_factory):
    """2. the same cases with the query's vertex ids reversed (a new file): the maps are the same maps with their columns
    reversed, the sets move with the vertices, and the table is the yardstick's for that file.  At least a quarter of the (case,
    bitmap) pairs have, in mode 0 or DISTINCT, some k and some entry with E[k][x->y] != E[k][y->x]: a table that ignored the
    direction would not pass"""
    from gnnpe_amd import binding
    cases = ri._ind_cases(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("reversed")
    skew = total = 0
    for c in cases:
        qp = _reversed_file(tmp, c["name"], c["variant"])
        emb, ind = c["emb"][:, ::-1], c["ind"][:, ::-1]
        for b in sh.BITMAPS:
            bm = np.ascontiguousarray(c[b][::-1])
            if b == "ld":
                assert np.array_equal(bm, ex._ld_bitmap(c["g"], qp))
            total += 1
            skew += _check_host_case(binding, c["g"], qp, c["name"], True, bm, emb, ind, ("rev", c["gi"], c["name"], c["variant"], b))
    assert total == len(cases) * 3 and skew * 4 >= total, (skew, total)


def test_host_table_closed_forms_on_h1(tmp_path_factory):
    """3. H1, one label, label/degree bitmap, mode 0.  Edge: E[0] is all ones.  Wedge 0 - 1 - 2: E[0][x->y] = deg(y) - 1 and
    E[1][x->y] = deg(x) - 1.  Triangle: every row is the common-neighbour count of the entry's ends, A @ A masked by A"""
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g = h["g"]
    src, _ = _csr_keys(g)
    dst = g["nbrs"].astype(np.int64)
    d = h["deg"].astype(np.uint64)
    ans, t = tabs["edge", "ld", False, False]
    assert ans == len(dst) and t.shape == (1, len(dst)) and (t == 1).all()
    ans, t = tabs["wedge", "ld", False, False]
    assert np.array_equal(t[0], d[dst] - 1) and np.array_equal(t[1], d[src] - 1) and ans == int((d * (d - 1)).sum())
    A = sh._adjacency(g)
    common = np.asarray((A @ A).multiply(A).tocsr()[src, dst]).ravel().astype(np.uint64)
    ans, t = tabs["triangle", "ld", False, False]
    assert ans == 28446 == common.sum() and all(np.array_equal(t[k], common) for k in range(3))
    ans, t = tabs["vertex", "ld", False, False]
    assert ans == g["n"] and t.shape == (0, len(dst))


def test_host_guard(tmp_path_factory, tmp_path):
    """4. limit is a guard: limit == |M| and |M| - 1 give complete == 0 and answers == limit, |M| + 1 the exact table and complete
    == 1, limit 0 complete == 0, an empty C(u) zeros and complete == 1; a single-vertex query has nqe == 0; unknown mode bits and a
    disconnected query are refused; host_query_edges with too little room returns an error and still says how many"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    for distinct, induced in MODES:
        count, full = tabs["triangle", "ld", distinct, induced]
        assert count == 28446 // (6 if distinct else 1)
        assert binding.host_refine_sets_edge_counts(g, qp, bm, count, distinct=distinct, induced=induced)[:2] == (count, False)
        assert binding.host_refine_sets_edge_counts(g, qp, bm, count - 1, distinct=distinct, induced=induced)[:2] == (count - 1, False)
        ans, complete, t = binding.host_refine_sets_edge_counts(g, qp, bm, count + 1, distinct=distinct, induced=induced)
        assert (ans, complete) == (count, True) and np.array_equal(t, full)
        assert binding.host_refine_sets_edge_counts(g, qp, bm, 0, distinct=distinct, induced=induced)[:2] == (0, False)
        empty = bm.copy()
        empty[1] = 0
        ans, complete, t = binding.host_refine_sets_edge_counts(g, qp, empty, FULL, distinct=distinct, induced=induced)
        assert (ans, complete) == (0, True) and t.shape == (3, len(g["nbrs"])) and not t.any()
    ans, complete, t = binding.host_refine_sets_edge_counts(g, h["q"]["vertex"], h["bm"]["vertex"]["ld"])
    assert (ans, complete) == (g["n"], True) and t.shape == (0, len(g["nbrs"])) and len(binding.host_query_edges(h["q"]["vertex"])) == 0
    online, u32p, u64p = binding.load_online(), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)
    out, done, t = C.c_uint64(), C.c_int(), np.zeros((3, len(nb)), np.uint64)
    for mode in (4, 7, 1 << 31):
        assert online.gnnpe_host_refine_sets_edge_counts(g["n"], o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), lb.ctypes.data_as(u32p),
                                                         qp.encode(), bmc.ctypes.data_as(u32p), FULL, mode, C.byref(out),
                                                         C.byref(done), t.ctypes.data_as(u64p)) != 0
        assert b"unknown mode" in binding.load().gnnpe_last_error()
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    for limit in (FULL, 0):
        with pytest.raises(binding.GnnpeError, match="not connected"):
            binding.host_refine_sets_edge_counts(g, disc, sh._ones(2, g["n"]), limit)
    k, room = C.c_uint32(), np.zeros((2, 2), np.uint32)
    assert online.gnnpe_host_query_edges(qp.encode(), room.ctypes.data_as(u32p), 2, C.byref(k)) != 0 and k.value == 3


def test_host_form_has_no_size_limit(tmp_path):
    """the 33-vertex path on the 40-cycle: 80 maps, 32 query edges, every directed entry once under every query edge"""
    from gnnpe_amd import binding
    g = sh._cycle_graph(40)
    qp = sh._path_file(tmp_path, 33)
    ans, complete, t = binding.host_refine_sets_edge_counts(g, qp, sh._ones(33, 40))
    assert (ans, complete) == (80, True) and t.shape == (32, 80) and (t == 1).all()


def test_cli_refusals(tmp_path):
    """5. --edge-counts without --refine sets, with --matches and with --vertex-counts exits 1 with its message before a GPU is
    touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    out = str(tmp_path / "ec.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    for extra, msg in ((["--edge-counts", out], "--edge-counts needs --refine sets"),
                       (["--refine", "start", "--edge-counts", out], "--edge-counts needs --refine sets"),
                       (["--refine", "sets", "--edge-counts", out, "--matches", str(tmp_path / "m.txt")], "exclude each other"),
                       (["--refine", "sets", "--edge-counts", out, "--vertex-counts", str(tmp_path / "v.txt")], "exclude each other")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout and not os.path.exists(out), extra


# ---- GPU: the device against the host form, cell for cell ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(7))
def test_gpu_every_first_level_shift(tmp_path_factory, monkeypatch, shift):
    """6. H1 with the first-level chunk forced to 1 << shift entries: the eight shapes on the three bitmaps in the four modes, the
    device table is the host form's.  H1 has rows longer than 64 (ient comes from a later chunk), several items per start candidate
    at a small shift, hubs (the search runs in the shorter row and the reverse entry is needed), and K4, K5 and the diamond have
    back edges at the leaf.  Triangle and K4 on the label/degree bitmap: the device table is also np.add.at over the rows
    Engine.refine_sets returns, which does not go through the host form.  The marginals of the device table are the table of
    Engine.refine_sets_vertex_counts, an independent kernel"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g = h["g"]
    assert (h["deg"] > 64).sum() >= 10
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in sh.H1_SHAPES:
            edges = _edges_of(name)
            for b in sh.BITMAPS:
                for distinct, induced in MODES:
                    want, table = tabs[name, b, distinct, induced]
                    got, complete, t, ms = eng.refine_sets_edge_counts(h["q"][name], h["bm"][name][b], distinct=distinct, induced=induced)
                    where = (shift, name, b, distinct, induced)
                    assert (got, complete) == (want, True) and ms > 0, where + (got, want)
                    assert t.dtype == np.uint64 and t.shape == table.shape and np.array_equal(t, table), where + (int((t != table).sum()),)
                    if b == "thin" and edges:
                        v = eng.refine_sets_vertex_counts(h["q"][name], h["bm"][name][b], distinct=distinct, induced=induced)[2]
                        for (u, k), m in _marginals(g, t, edges, sh.SHAPES[name][0]).items():
                            assert np.array_equal(m, v[u]), where + (u, k)
        for name, count in (("triangle", 28446), ("K4", 109224)):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=count)
            assert got == count == len(rows)
            t = eng.refine_sets_edge_counts(qp, bm)[2]
            assert np.array_equal(t, _table(g, rows, _edges_of(name))), (shift, name)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_reversed_id_queries(tmp_path_factory, monkeypatch, ecount_lines):
    """7. the reversed-id files of wedge, triangle, C4 and diamond on H1 in the four modes at shifts 0 and 6, on the label/degree
    bitmap and on the one that starts the matching order at the last query vertex (_h1_reversed): device == host form.  The debug
    lines say what the plans held: over the run flipped plan edges and flipped back edges occur, and the pivot edge of the last
    position occurs both flipped and not"""
    from gnnpe_amd import binding
    h, revs = sh._h1(tmp_path_factory), _h1_reversed(tmp_path_factory)
    said = []
    for shift in (0, 6):
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
        eng = ex._engine(binding, h["g"], h["sn"], 2)
        try:
            ecount_lines()
            for (name, b), r in revs.items():
                for distinct, induced in MODES:
                    want, table = r["tabs"][distinct, induced]
                    got, complete, t, _ = eng.refine_sets_edge_counts(r["qp"], r["bm"], distinct=distinct, induced=induced)
                    assert (got, complete) == (want, True) and np.array_equal(t, table), (shift, name, b, distinct, induced)
            lines = ecount_lines()
            assert all(ln["shift"] == shift and ln["forced"] == 1 for ln in lines if "edges" in ln)
            said += lines
        finally:
            eng.close()
    plans = [ln for ln in said if "edges" in ln]
    assert len(plans) == 2 * len(revs) * len(MODES) and len(said) == 2 * len(plans)
    assert any(ln["flips"] > 0 for ln in plans) and any(ln["backflips"] > 0 for ln in plans)
    assert {ln["lastflip"] for ln in plans} == {0, 1}
    finds = [ln for ln in said if "finds" in ln]
    assert any(ln["finds"] > 0 for ln in finds)
    assert all(ln["complete"] == 1 and (ln["finds"] == 0 or ln["leaf_adds"] >= ln["finds"]) for ln in finds)


def _planted_k10():
    """gnm_graph(400, 600, one label) with a K10 planted on the vertices 0, 40, .., 360"""
    from gnnpe_amd import synth
    base = synth.gnm_graph(400, 600, n_labels=1, seed=11)
    src, _ = _csr_keys(base)
    dst = base["nbrs"].astype(np.int64)
    clique = np.arange(10, dtype=np.int64) * 40
    a, b = np.meshgrid(clique, clique)
    keys = np.unique(np.concatenate([src * 400 + dst, (a * 400 + b)[a != b]]))
    offs = np.searchsorted(keys // 400, np.arange(401)).astype(np.uint32)
    return dict(n=400, offsets=offs, nbrs=(keys % 400).astype(np.uint32), labels=np.zeros(400, np.uint32))


@pytest.mark.gpu
def test_gpu_query_sizes_and_refusals(tmp_path_factory, tmp_path):
    """8. nq == 1 (no edge: an empty table, a null device pointer, the usual answer); nq == 2 (the only level is the leaf and the
    entries come from the first-level items) against the closed form; the 32-vertex path (31 edges, k up to 30) on the 32- and the
    33-cycle in the four modes; K8 in DISTINCT mode on a K10 planted in a sparse graph (28 edges, seven back edges at the last
    position, 45 matches) against the host form.  The refusals are gnnpe_refine_sets_mode's: 33 query vertices, the multigraph
    state, unknown mode bits, a context without a gnnpe_load_csr graph"""
    from gnnpe_amd import binding, synth
    h = sh._h1(tmp_path_factory)
    g, d = h["g"], h["deg"].astype(np.uint64)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            got, complete, t, _ = eng.refine_sets_edge_counts(h["q"]["vertex"], h["bm"]["vertex"][b])
            assert (got, complete) == (len(sh._members(h["bm"]["vertex"][b][0], g["n"])), True) and t.shape == (0, len(g["nbrs"])), b
            got, complete, view, _ = eng.refine_sets_edge_counts(h["q"]["vertex"], h["bm"]["vertex"][b], device=True)
            assert view.__cuda_array_interface__["data"][0] == 0 and view.shape == (0, len(g["nbrs"]))
        for b in ("ld", "ones"):
            got, complete, t, _ = eng.refine_sets_edge_counts(h["q"]["edge"], h["bm"]["edge"][b])
            assert (got, complete) == (int(d.sum()), True) and t.shape == (1, len(g["nbrs"])) and (t == 1).all(), b
            got, complete, t, _ = eng.refine_sets_edge_counts(h["q"]["edge"], h["bm"]["edge"][b], distinct=True)
            src, _ = _csr_keys(g)
            assert (got, complete) == (int(d.sum()) // 2, True) and np.array_equal(t[0], (src < g["nbrs"]).astype(np.uint64)), b
        p33 = sh._path_file(tmp_path, 33)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets_edge_counts(p33, sh._ones(33, g["n"]))
        out, done, ms, ptr = C.c_uint64(), C.c_int(), C.c_double(), C.c_void_p()
        bmc = np.ascontiguousarray(h["bm"]["edge"]["ld"], np.uint32)
        for mode in (4, 1 << 31):
            assert binding.load_online().gnnpe_refine_sets_edge_counts(eng.ctx, h["q"]["edge"].encode(),
                                                                       bmc.ctypes.data_as(C.POINTER(C.c_uint32)), FULL, mode,
                                                                       C.byref(out), C.byref(done), None, C.byref(ptr), C.byref(ms)) != 0
            assert b"unknown mode" in binding.load().gnnpe_last_error()
        assert eng.refine_sets_edge_counts(h["q"]["edge"], h["bm"]["edge"]["ld"])[0] == int(d.sum())  # the context still answers
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.refine_sets_edge_counts(h["q"]["edge"], h["bm"]["edge"]["ld"])
    finally:
        eng.close()
    bare = binding.Engine(0)
    try:
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            bare.refine_sets_edge_counts(h["q"]["edge"], h["bm"]["edge"]["ld"])
    finally:
        bare.close()
    p32 = sh._path_file(tmp_path, 32)
    for n, plain, ind in ((32, 64, 0), (33, 66, 66)):
        cyc = sh._cycle_graph(n)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            for bm in (ex._ld_bitmap(cyc, p32), sh._ones(32, n)):
                for distinct, induced in MODES:
                    want = binding.host_refine_sets_edge_counts(cyc, p32, bm, FULL, distinct=distinct, induced=induced)
                    assert want[0] == (ind if induced else plain) // (2 if distinct else 1) and want[1] and want[2].shape == (31, 2 * n)
                    got, complete, t, _ = eng.refine_sets_edge_counts(p32, bm, distinct=distinct, induced=induced)
                    assert (got, complete) == want[:2] and np.array_equal(t, want[2]), (n, induced, distinct)
        finally:
            eng.close()
    k10 = _planted_k10()
    k8 = str(tmp_path / "K8.graph")
    ex._write_query(k8, 8, {(a, b) for a in range(8) for b in range(a + 1, 8)}, [0] * 8)
    bm = ex._ld_bitmap(k10, k8)
    want = binding.host_refine_sets_edge_counts(k10, k8, bm, FULL, distinct=True)
    assert want[:2] == (45, True) and want[2].shape[0] == 28 and (want[2].sum(axis=1) == 45).all()
    eng = ex._engine(binding, k10, synth.degree_order(k10["offsets"]), 2)
    try:
        got, complete, t, _ = eng.refine_sets_edge_counts(k8, bm, distinct=True)
        assert (got, complete) == (45, True) and np.array_equal(t, want[2])
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_star5_closed_form(tmp_path_factory):
    """9. star5 with centre 0 on H1, label/degree bitmap, mode 0: 4 596 520 344 maps; E[(0, i)][x->y] = (d_x-1)(d_x-2)(d_x-3)
    for every leaf i, where d_x >= 4 and 0 elsewhere.  The largest cell is 154 * 153 * 152 < 2^32"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, d = h["g"], h["deg"].astype(np.int64)
    qp = sh._shape_file(h["tmp"], "star5")
    src, _ = _csr_keys(g)
    cell = ((d - 1) * (d - 2) * (d - 3) * (d >= 4))[src].astype(np.uint64)
    assert cell.sum() == 4596520344 and cell.max() < 1 << 32
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        got, complete, t, ms = eng.refine_sets_edge_counts(qp, ex._ld_bitmap(g, qp))
        print(f"star5 on H1: {got} maps, {ms:.3f} ms")
        assert (got, complete) == (int(cell.sum()), True) and t.shape == (4, len(src))
        assert all(np.array_equal(t[k], cell) for k in range(4))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_device_table(tmp_path_factory):
    """10. device=True: the view, read back with Engine.edge_counts_to_host, is the host-returned table; it survives a following
    refine_sets_vertex_counts and refine_sets call (the buffer is the call's own); the next edge-count call replaces it -- the
    old view is refused as stale, the new one is right and, for a smaller table, in the same buffer --; empty sets give zeros;
    after another load_csr every view is refused"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g = h["g"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        got, complete, view5, ms = eng.refine_sets_edge_counts(h["q"]["K5"], h["bm"]["K5"]["ones"], device=True)
        want5 = tabs["K5", "ones", False, False]
        ptr5 = view5.__cuda_array_interface__["data"][0]
        assert ptr5 and view5.shape == want5[1].shape and view5.__cuda_array_interface__["typestr"] == "<i8"
        assert (got, complete) == (want5[0], True) and np.array_equal(eng.edge_counts_to_host(view5), want5[1]) and want5[1].any()
        eng.refine_sets_vertex_counts(h["q"]["K4"], h["bm"]["K4"]["ld"], device=True)
        eng.refine_sets(h["q"]["K4"], h["bm"]["K4"]["ld"], limit=FULL, matches_cap=1000)
        assert np.array_equal(eng.edge_counts_to_host(view5), want5[1])
        for name, b, distinct, induced in (("wedge", "thin", False, True), ("edge", "ld", True, False)):
            got, complete, view, _ = eng.refine_sets_edge_counts(h["q"][name], h["bm"][name][b], distinct=distinct, induced=induced,
                                                                 device=True)
            assert view.__cuda_array_interface__["data"][0] == ptr5, "the grow-only buffer was allocated again for a smaller table"
            assert (got, complete) == (tabs[name, b, distinct, induced][0], True)
            assert np.array_equal(eng.edge_counts_to_host(view), tabs[name, b, distinct, induced][1])
            with pytest.raises(binding.GnnpeError, match="stale"):
                eng.edge_counts_to_host(view5)
        empty = h["bm"]["triangle"]["ld"].copy()
        empty[2] = 0
        got, complete, view, _ = eng.refine_sets_edge_counts(h["q"]["triangle"], empty, device=True)
        assert (got, complete) == (0, True) and view.shape == (3, len(g["nbrs"])) and not eng.edge_counts_to_host(view).any()
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.edge_counts_to_host(view)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_guard(tmp_path_factory):
    """11. K4 on H1 (109 224 maps, far past the 1 024-find flush) and its distinct form (4 551): limit |M| - 1 and |M| give
    complete == 0 and answers == limit, |M| + 1 gives complete == 1 and the exact table, limit 0 complete == 0, limits around the
    flush threshold are reached; twice on one context"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    qp, bm = h["q"]["K4"], h["bm"]["K4"]["ld"]
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for distinct in (False, True):
            count, table = tabs["K4", "ld", distinct, False]
            assert count == 109224 // (24 if distinct else 1) > 1025
            for _ in range(2):
                for limit in (1, 1023, 1024, 1025, count - 1, count):
                    got, complete, _, _ = eng.refine_sets_edge_counts(qp, bm, limit=limit, distinct=distinct)
                    assert (got, complete) == (limit, False), (distinct, limit, got, complete)
                got, complete, t, _ = eng.refine_sets_edge_counts(qp, bm, limit=count + 1, distinct=distinct)
                assert (got, complete) == (count, True) and np.array_equal(t, table), distinct
                assert eng.refine_sets_edge_counts(qp, bm, limit=0, distinct=distinct)[:2] == (0, False)
    finally:
        eng.close()


# The 24 seeds of sh.FUZZ_SEEDS and one more.  A restatement of build_match_order over the 24 finds flipped pivot edges in 12 of
# them and a flipped back edge in none: a back edge is flipped only where a later-placed vertex has a smaller id than an earlier
# neighbour that is not its first-placed one.  Of the seeds 24 .. 119 six have one, and seed 107 alone has matches too (a
# 4-vertex query on a 601-vertex power-law graph, all-ones bitmap, shift 4, order 0 1 3 2, 1 527 maps): it is added so that the
# assertion over the set has something to find.
FUZZ_SEEDS = list(sh.FUZZ_SEEDS) + [107]
_FUZZ_BACKFLIPS = {}


def _fuzz_run(seed, tmp_path_factory, monkeypatch, ecount_lines):
    """one fuzz case in the four modes: device == host form; remembers the most flipped back edges a plan of it had"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    if c["shift"] is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
    else:
        monkeypatch.delenv("GNNPE_TESTING", raising=False)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        ecount_lines()
        for distinct, induced in MODES:
            want = binding.host_refine_sets_edge_counts(g, c["qp"], c["bm"], FULL, distinct=distinct, induced=induced)
            assert want[1] and (distinct or induced or want[0] == c["count"])
            got, complete, t, _ = eng.refine_sets_edge_counts(c["qp"], c["bm"], distinct=distinct, induced=induced)
            assert (got, complete) == want[:2] and np.array_equal(t, want[2]), (seed, c["which"], c["shift"], distinct, induced)
        lines = ecount_lines()
        finds = max([ln["finds"] for ln in lines if "finds" in ln], default=0)
        _FUZZ_BACKFLIPS[seed] = (max([ln["backflips"] for ln in lines if "edges" in ln], default=0), finds)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, monkeypatch, ecount_lines, seed):
    """12. the 24 fuzz cases of test_refine_sets_shapes and seed 107 (random graph, connected query of 1-6 vertices, one of four kinds of
    bitmap, a random first-level shift) in the four modes: the device table is the host form's"""
    _fuzz_run(seed, tmp_path_factory, monkeypatch, ecount_lines)


@pytest.mark.gpu
def test_gpu_fuzz_cases_flip_a_back_edge(tmp_path_factory, monkeypatch, ecount_lines):
    """12a. over the fuzz cases some plan has a flipped back edge and finds matches through it (a case the parametrised test
    has not run yet is run here)"""
    assert set(sh.FUZZ_SEEDS) <= set(FUZZ_SEEDS)
    for seed in FUZZ_SEEDS:
        if seed not in _FUZZ_BACKFLIPS:
            _fuzz_run(seed, tmp_path_factory, monkeypatch, ecount_lines)
    assert any(back > 0 and finds > 0 for back, finds in _FUZZ_BACKFLIPS.values()), _FUZZ_BACKFLIPS


@pytest.mark.gpu
@pytest.mark.parametrize("q", rs.QUERIES)
def test_gpu_cli_edge_counts(tmp_path, test_graph, q):
    """13. gnnpe_main -m online --exact --refine sets --edge-counts on the golden test graph, q0 .. q4: the first line is
    `# a_0-b_0 ...`, then one line `x y c_0 .. c_{nqe-1}` per directed entry with a non-zero cell, ascending by (x, y); every
    column sums to the golden exact answer and the cells are the binding's table (the exact filter's sets are complete, so it is
    the label/degree bitmap's table).  q2 also with --distinct and --induced, and with -n at the answer: the guard is reached, the
    exit status is non-zero, the message names -n and no file is written"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    exact = json.load(open(os.path.join(ONLINE, "exact_answers.json")))[q]["exact"]
    qp = os.path.join(ONLINE, f"{q}.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    _, keys = _csr_keys(test_graph)
    edges = binding.host_query_edges(qp)
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets"]
    for k, (distinct, induced) in enumerate(MODES if q == "q2" else MODES[:1]):
        want, complete, table = binding.host_refine_sets_edge_counts(test_graph, qp, ld, FULL, distinct=distinct, induced=induced)
        assert complete and (distinct or induced or want == exact)
        out = str(tmp_path / f"ec{k}.txt")
        cmd = base + ["--edge-counts", out] + (["--distinct"] if distinct else []) + (["--induced"] if induced else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        assert ans == want, (distinct, induced, ans, want)
        head = open(out).readline().split()
        assert head[0] == "#" and [tuple(map(int, e.split("-"))) for e in head[1:]] == [tuple(e) for e in edges.tolist()]
        lines = np.loadtxt(out, dtype=np.uint64, ndmin=2) if want else np.zeros((0, len(edges) + 2), np.uint64)
        assert lines.shape[1] == len(edges) + 2
        code = lines[:, 0].astype(np.int64) * n + lines[:, 1].astype(np.int64)
        assert (np.diff(code) > 0).all() and (lines[:, 2:].sum(axis=0) == ans).all() and (lines[:, 2:] != 0).any(axis=1).all()
        j = np.searchsorted(keys, code)
        assert np.array_equal(keys[j], code)
        got = np.zeros_like(table)
        got[:, j] = lines[:, 2:].T
        assert np.array_equal(got, table), (distinct, induced)
    if q == "q2":
        out = str(tmp_path / "guard.txt")
        r = subprocess.run(base + ["--edge-counts", out, "-n", str(exact)], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "-n" in r.stderr and not os.path.exists(out), (r.returncode, r.stderr)
        r = subprocess.run(base + ["--edge-counts", out, "-n", str(exact + 1)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"Answer Number: {exact} " in r.stdout and os.path.exists(out), r.stderr
