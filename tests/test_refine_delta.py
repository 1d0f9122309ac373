"""The matches through a given set of data edges, each once (include/gnnpe_online.h, ABI version 15): Delta_m(C, F, limit) = the
maps of mode m that put at least one query edge on an edge of F, on the host (gnnpe_host_refine_sets_delta), on the device
(gnnpe_refine_sets_delta) and through `gnnpe_main --delta-edges`.

The host form walks all of M and drops the finds that miss F.  It is held to yardsticks that are not the library: networkx's rows
filtered in numpy by "touches F", the insertion identity |M(G + F)| - |M(G)| = Delta(G + F, F), the per-edge tables for a single
edge.  The device form starts at the edges of F instead, once per query edge, and charges every match to its lowest-numbered
query edge in F; it is held to the host form, to the rows gnnpe_refine_sets_mode lists (filtered in numpy), to F = E(G), where
Delta = |M| and any match charged twice shows, and to the insertion identity between two loaded graphs.  The yardstick is never the
new kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_distinct as rd
import test_refine_edge_counts as re_
import test_refine_induced as ri
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = ((False, False), (True, False), (False, True), (True, True))  # (distinct, induced): 0, DISTINCT, INDUCED, both
H1_DELTA_SHAPES = ("edge", "wedge", "triangle", "diamond", "K4")
ROWS_MAX = 500_000  # the device's full listing is compared row for row where it is at most this long


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _und_edges(g):
    """the undirected edges (x, y), x < y, ascending: an (m, 2) int64 array"""
    src, _ = re_._csr_keys(g)
    e = np.stack([src, g["nbrs"].astype(np.int64)], axis=1)
    return e[e[:, 0] < e[:, 1]]


def _codes(edges, n):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return np.unique(e.min(axis=1) * n + e.max(axis=1))


def _touches(rows, qedges, edges, n):
    """mask of the rows that put at least one of the query edges on an edge of F"""
    rows = np.asarray(rows, np.int64)
    hit = np.zeros(len(rows), bool)
    f = _codes(edges, n)
    for a, b in qedges:
        hit |= np.isin(np.minimum(rows[:, a], rows[:, b]) * n + np.maximum(rows[:, a], rows[:, b]), f)
    return hit


def _qedges(qp):
    return rd._query_edges(qp)[1]


def _entry(g, x, y):
    """the offset of y in x's row"""
    o = g["offsets"].astype(np.int64)
    j = int(np.searchsorted(g["nbrs"][o[x]:o[x + 1]], y))
    assert g["nbrs"][o[x] + j] == y
    return j


def _without(g, edges):
    """g minus the undirected edges, on the same vertices"""
    from gnnpe_amd import synth
    n = len(g["labels"])
    e = _und_edges(g)
    keep = e[~np.isin(e[:, 0] * n + e[:, 1], _codes(edges, n))]
    offs, nbrs = synth._csr_from_edges(n, keep[:, 0], keep[:, 1])
    return dict(n=n, offsets=offs, nbrs=nbrs, labels=g["labels"])


def _label_bitmap(g, qp):
    """labels only: it is the same for a graph and the graph minus some edges (a degree bitmap would differ)"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qp)
    n = len(g["labels"])
    return np.stack([sh._row_of(np.nonzero(g["labels"] == q["labels"][u])[0], n) for u in range(q["n"])])


def _four_sets(g, seed):
    """the four forms of F on a small graph: one random edge, five random edges, two edges that share a vertex, all edges"""
    e = _und_edges(g)
    rng = np.random.default_rng(seed)
    deg = np.diff(g["offsets"].astype(np.int64))
    v = int(rng.choice(np.nonzero(deg >= 2)[0]))
    o = int(g["offsets"][v])
    share = np.array([[v, g["nbrs"][o]], [g["nbrs"][o + 1], v]], np.int64)  # (either orientation)
    return dict(one=e[rng.choice(len(e), 1)], five=e[rng.choice(len(e), min(5, len(e)), replace=False)], share=share, all=e)


_H1F = {}


def _h1_delta(tmp_path_factory):
    """H1 with the F of the device tests, each part asserted to exist: an edge between two rows longer than 64 whose entry sits at
    row offset >= 64 in one direction (the chunk base in mid row, the ordered trim of a hub pivot at depth 2); the first and the
    last entry of one row; two edges that share a vertex; the three edges of a triangle; an edge with an endpoint of degree 1; 50
    random edges (seed 1500).  57 different edges.  With it the host form's Delta of H1_DELTA_SHAPES on the three bitmaps in the
    four modes, computed once"""
    if _H1F:
        return _H1F
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, deg = h["g"], h["deg"]
    e = _und_edges(g)
    hubs = e[(deg[e[:, 0]] > 64) & (deg[e[:, 1]] > 64)]
    hub = next(((x, y) for x, y in hubs.tolist() if max(_entry(g, x, y), _entry(g, y, x)) >= 64), None)
    assert hub is not None, "no edge between two hubs past the first chunk of a row"
    v = int(np.nonzero(deg > 64)[0][0])
    o = g["offsets"].astype(np.int64)
    ends = [(v, int(g["nbrs"][o[v]])), (int(g["nbrs"][o[v + 1] - 1]), v)]
    w = int(np.nonzero((deg >= 2) & (deg <= 64))[0][0])
    share = [(w, int(g["nbrs"][o[w]])), (w, int(g["nbrs"][o[w] + 1]))]
    tri = next(((x, y, int(z)) for x, y in e.tolist()
                for z in np.intersect1d(g["nbrs"][o[x]:o[x + 1]], g["nbrs"][o[y]:o[y + 1]])[:1]), None)
    assert tri is not None
    leaf = int(np.nonzero(deg == 1)[0][0])
    pend = (leaf, int(g["nbrs"][o[leaf]]))
    rnd = e[np.random.default_rng(1500).choice(len(e), 50, replace=False)]
    F = np.array([hub] + ends + share + [(tri[0], tri[1]), (tri[2], tri[0]), (tri[1], tri[2])] + [pend] + rnd.tolist(), np.int64)
    assert len(_codes(F, g["n"])) == 57
    want = {}
    for name in H1_DELTA_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                want[name, b, distinct, induced] = binding.host_refine_sets_delta(g, h["q"][name], h["bm"][name][b], F, FULL,
                                                                                  distinct=distinct, induced=induced)
    _H1F.update(F=F, want=want, all=e)
    return _H1F


def _raw_device(binding, eng, qp, bm, edges, limit=FULL, mode=0):
    """gnnpe_refine_sets_delta through ctypes: (return code, *answers); *answers is set to a canary first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    e = np.ascontiguousarray(np.asarray(edges, np.int64).reshape(-1, 2), np.uint32)
    out, ms = C.c_uint64(12345), C.c_double()
    rc = binding.load_online().gnnpe_refine_sets_delta(eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), e.ctypes.data_as(u32p), len(e),
                                                       limit, mode, C.byref(out), None, 0, C.byref(ms))
    return rc, out.value


# ---- CPU: the host form against yardsticks that are not the library ----------------------------------------------------------

def test_host_form_against_networkx(tmp_path_factory):
    """1. the 15 small graphs, the eight shapes of ri.IND_SHAPES, both label variants, the label/degree and the thinned bitmap, the
    four modes, the four forms of F (one edge, five, two that share a vertex, all): the host form is the number of networkx's rows
    (inside the sets, induced for INDUCED, filtered by the ordering pairs for DISTINCT) with some (row[a_k], row[b_k]) in F.  Over
    the run at least a fifth of the (case, bitmap, mode, F) have a match through F and a tenth have one that avoids it"""
    from gnnpe_amd import binding
    cases = ri._ind_cases(tmp_path_factory)
    assert len(cases) == 15 * len(ri.IND_SHAPES) * 2
    some = part = total = 0
    for c in cases:
        g, n = c["g"], c["g"]["n"]
        qe = _qedges(c["qp"])
        sets = _four_sets(g, 2100 + c["gi"])
        for b in ("ld", "thin"):
            for distinct, induced in MODES:
                rows = c["ind"] if induced else c["emb"]
                rows = rows[rs._in_sets(c[b], rows)]
                if distinct:
                    rows = rows[rd._ordered(rows, re_._pairs(c["qp"]))]
                for form, F in sets.items():
                    want = int(_touches(rows, qe, F, n).sum())
                    got = binding.host_refine_sets_delta(g, c["qp"], c[b], F, FULL, distinct=distinct, induced=induced)
                    assert got == want, (c["gi"], c["name"], c["variant"], b, distinct, induced, form, got, want)
                    total += 1
                    some += want > 0
                    part += 0 < want < len(rows)
    assert some * 5 >= total and part * 10 >= total, (some, part, total)


def test_all_edges_is_the_plain_count(tmp_path_factory):
    """2. F = E(G): every match of a query with an edge touches F, so Delta is host_refine_sets' count -- H1, the eight shapes, the
    three bitmaps, the four modes; `vertex` has no edge and gives 0"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    e = _und_edges(g)
    for name in sh.H1_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                got = binding.host_refine_sets_delta(g, h["q"][name], h["bm"][name][b], e, FULL, distinct=distinct, induced=induced)
                want = binding.host_refine_sets(g, h["q"][name], h["bm"][name][b], FULL, distinct=distinct, induced=induced)
                assert got == (0 if name == "vertex" else want), (name, b, distinct, induced)
                assert name == "vertex" or distinct or induced or want == h["want"][name, b]


def test_host_insertion_identity(tmp_path_factory):
    """3. modes 0 and DISTINCT: G' a graph, F a random tenth of its edges (at least one), G = G' minus F on the same vertices, a
    labels-only bitmap: |M(G')| - |M(G)| == Delta(G', F).  The 15 small graphs with the eight shapes and both label variants, and
    H1 with its eight shapes (where F has 569 edges)"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    runs = [(c["g"], c["qp"], 2300 + c["gi"]) for c in ri._ind_cases(tmp_path_factory)]
    runs += [(h["g"], h["q"][name], 2400) for name in sh.H1_SHAPES]
    grew = 0
    for g1, qp, seed in runs:
        e = _und_edges(g1)
        F = e[np.random.default_rng(seed).choice(len(e), max(1, len(e) // 10), replace=False)]
        g0 = _without(g1, F)
        assert len(g0["nbrs"]) == len(g1["nbrs"]) - 2 * len(F)
        bm = _label_bitmap(g1, qp)
        for distinct in (False, True):
            new = binding.host_refine_sets(g1, qp, bm, FULL, distinct=distinct)
            old = binding.host_refine_sets(g0, qp, bm, FULL, distinct=distinct)
            assert new - old == binding.host_refine_sets_delta(g1, qp, bm, F, FULL, distinct=distinct), (qp, distinct, new, old)
            grew += new > old
    assert grew * 2 >= len(runs)


def test_single_edge_is_the_sum_of_its_edge_count_cells(tmp_path_factory):
    """4. F = {{x, y}}: Delta = the sum over k of E[k][x->y] + E[k][y->x] of host_refine_sets_edge_counts (a simple graph carries
    at most one query edge of a match on one data edge), in the four modes: H1, the shapes of H1_DELTA_SHAPES, the label/degree and
    the thinned bitmap, twelve edges of the device tests' F"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    g = h["g"]
    o = g["offsets"].astype(np.int64)
    tabs = re_._h1_tables(tmp_path_factory)
    for name in H1_DELTA_SHAPES:
        for b in ("ld", "thin"):
            for distinct, induced in MODES:
                t = tabs[name, b, distinct, induced][1]
                for x, y in f["F"][:12].tolist():
                    want = int(t[:, o[x] + _entry(g, x, y)].sum() + t[:, o[y] + _entry(g, y, x)].sum())
                    got = binding.host_refine_sets_delta(g, h["q"][name], h["bm"][name][b], [(x, y)], FULL, distinct=distinct,
                                                         induced=induced)
                    assert got == want, (name, b, distinct, induced, x, y)


def test_repeats_and_orientations_mean_the_set(tmp_path_factory):
    """5. F with every pair twice, once reversed, in a shuffled order: the answer of the set; and limit cuts it"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    F = f["F"]
    noisy = np.concatenate([F, F[:, ::-1], F[::3]])
    noisy = noisy[np.random.default_rng(5).permutation(len(noisy))]
    for name in ("wedge", "K4"):
        for distinct, induced in MODES:
            want = f["want"][name, "ld", distinct, induced]
            assert want > 0
            assert binding.host_refine_sets_delta(h["g"], h["q"][name], h["bm"][name]["ld"], noisy, FULL, distinct=distinct,
                                                  induced=induced) == want
            for limit in (0, 1, want - 1, want, want + 1):
                assert binding.host_refine_sets_delta(h["g"], h["q"][name], h["bm"][name]["ld"], F, limit, distinct=distinct,
                                                      induced=induced) == min(want, limit)
    assert binding.host_refine_sets_delta(h["g"], h["q"]["K4"], h["bm"]["K4"]["ld"], np.zeros((0, 2), np.uint32)) == 0


def test_host_refusals(tmp_path_factory, tmp_path):
    """6. a non-edge pair, x == y, an id >= n, unknown mode bits and a disconnected query return GNNPE_ERR_ARG with *answers = 0"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    iso = np.nonzero(h["deg"] == 0)[0]
    good = f["F"][:3].tolist()
    for bad, msg in (((int(iso[0]), int(iso[1])), "not an edge"), ((7, 7), "loop"), ((3, g["n"]), "does not have"),
                     ((g["n"] + 5, 2), "does not have")):
        with pytest.raises(binding.GnnpeError, match=msg):
            binding.host_refine_sets_delta(g, qp, bm, good + [bad])
    online, u32p = binding.load_online(), C.POINTER(C.c_uint32)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)

    def raw(qpath, edges, mode):
        e = np.ascontiguousarray(np.asarray(edges, np.int64).reshape(-1, 2), np.uint32)
        out = C.c_uint64(12345)
        rc = online.gnnpe_host_refine_sets_delta(g["n"], o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), lb.ctypes.data_as(u32p),
                                                 qpath.encode(), bmc.ctypes.data_as(u32p), e.ctypes.data_as(u32p), len(e), FULL, mode,
                                                 C.byref(out))
        return rc, out.value
    assert raw(qp, good, 0) == (0, binding.host_refine_sets_delta(g, qp, bm, good))
    for mode in (4, 7, 1 << 31):
        assert raw(qp, good, mode) == (-1, 0) and b"unknown mode" in binding.load().gnnpe_last_error()
    assert raw(qp, good + [(int(iso[0]), int(iso[1]))], 0) == (-1, 0)
    assert raw(qp, good + [(5, 5)], 1) == (-1, 0)
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    for limit in (FULL, 0):
        with pytest.raises(binding.GnnpeError, match="not connected"):
            binding.host_refine_sets_delta(g, disc, sh._ones(2, g["n"]), good, limit)


def test_cli_refusals(tmp_path):
    """--delta-edges without --refine sets, with --all-matches and with a count table exits 1 with its message before a GPU is
    touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    ef = str(tmp_path / "edges.txt")
    open(ef, "w").write("0 1\n")
    m = str(tmp_path / "m.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    for extra, msg in ((["--delta-edges", ef], "--delta-edges needs --refine sets"),
                       (["--refine", "sets", "--delta-edges", ef, "--matches", m, "--all-matches"], "--delta-edges excludes"),
                       (["--refine", "sets", "--delta-edges", ef, "--edge-counts", m], "--delta-edges excludes"),
                       (["--refine", "sets", "--delta-edges", ef, "--vertex-counts", m], "--delta-edges excludes")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout and not os.path.exists(m), extra


# ---- GPU: the device against the host form and against the plain call's rows -----------------------------------------------

def _device_equals_host(binding, eng, g, qp, bm, F, distinct, induced, want, where, rows_too=True):
    """Delta and, with room for all of them, the rows: pairwise different valid maps that touch F; where the full listing is short
    enough, exactly the plain call's rows that touch F"""
    got, rows, ms = eng.refine_sets_delta(qp, bm, F, matches_cap=want + 3, distinct=distinct, induced=induced)
    assert got == want == len(rows), where + (got, want, len(rows))
    if not rows_too or want == 0:
        return
    qe = _qedges(qp)
    n = len(g["labels"])
    assert _touches(rows, qe, F, n).all(), where
    count = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
    if count <= ROWS_MAX:
        full = eng.refine_sets(qp, bm, limit=FULL, matches_cap=count, distinct=distinct, induced=induced)[2]
        assert len(full) == count
        keep = full[_touches(full, qe, F, n)].astype(np.int64)
        mine = rows.astype(np.int64)
        assert np.array_equal(mine[np.lexsort(mine.T[::-1])], keep[np.lexsort(keep.T[::-1])]), where
    else:
        ri._assert_rows(g, qp, bm, rows, induced, re_._pairs(qp) if distinct else None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", H1_DELTA_SHAPES)
def test_gpu_h1_equals_the_host_form(tmp_path_factory, name):
    """a. H1 with the F of _h1_delta (a hub-to-hub entry past the first chunk, the ends of a row, a shared vertex, a triangle, a
    pendant edge, 50 random edges), the three bitmaps, the four modes: Delta is the host form's, and with matches_cap >= Delta the
    sorted rows are the sorted rows of refine_sets' full listing that touch F (filtered in numpy).  Host form, label/degree bitmap,
    mode 0: edge 114, wedge 8 086, triangle 738, diamond 14 408, K4 5 400"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    assert f["want"][name, "ld", False, False] == {"edge": 114, "wedge": 8086, "triangle": 738, "diamond": 14408, "K4": 5400}[name]
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                _device_equals_host(binding, eng, h["g"], h["q"][name], h["bm"][name][b], f["F"], distinct, induced,
                                    f["want"][name, b, distinct, induced], (name, b, distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_small_graphs_equal_the_host_form(tmp_path_factory, gi):
    """a'. the 15 small graphs with the eight shapes of ri.IND_SHAPES (C4, C5 and star5 among them), both label variants, the
    label/degree and the thinned bitmap, the four modes, F = five random edges and F = two edges that share a vertex: device ==
    host form, rows as in (a)"""
    from gnnpe_amd import binding, synth
    cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi]
    g = cases[0]["g"]
    sets = _four_sets(g, 2100 + gi)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            for b in ("ld", "thin"):
                for distinct, induced in MODES:
                    for form in ("five", "share"):
                        want = binding.host_refine_sets_delta(g, c["qp"], c[b], sets[form], FULL, distinct=distinct, induced=induced)
                        _device_equals_host(binding, eng, g, c["qp"], c[b], sets[form], distinct, induced, want,
                                            (gi, c["name"], c["variant"], b, distinct, induced, form))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_all_edges_is_the_plain_call(tmp_path_factory):
    """b. the charging rule.  F = E(G): Delta is refine_sets' count and the rows are its rows -- every match once, although it is
    met in the launch of each of its query edges (without the rule the count is up to nqe times too large).  H1 with triangle
    (28 446) and K4 (109 224) in the four modes, and two of the small graphs with their eight shapes"""
    from gnnpe_amd import binding, synth
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    runs = [(h["g"], h["sn"], [(h["q"][name], h["bm"][name][b]) for name in ("triangle", "K4") for b in ("ld", "thin")], f["all"])]
    for gi in (0, 7):
        cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi]
        g = cases[0]["g"]
        runs.append((g, synth.degree_order(g["offsets"]), [(c["qp"], c["ld"]) for c in cases], _und_edges(g)))
    for g, sn, queries, E in runs:
        eng = ex._engine(binding, g, sn, 2)
        try:
            for qp, bm in queries:
                for distinct, induced in MODES:
                    count = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                    assert count == binding.host_refine_sets(g, qp, bm, FULL, distinct=distinct, induced=induced)
                    got, rows, _ = eng.refine_sets_delta(qp, bm, E, matches_cap=count + 1, distinct=distinct, induced=induced)
                    assert got == count == len(rows), (qp, distinct, induced, got, count)
                    full = eng.refine_sets(qp, bm, limit=FULL, matches_cap=max(count, 1), distinct=distinct, induced=induced)[2]
                    assert sh._row_set(rows) == sh._row_set(full) and len(sh._row_set(rows)) == count
        finally:
            eng.close()
    assert h["want"]["triangle", "ld"] == 28446 and h["want"]["K4", "ld"] == 109224


@pytest.mark.gpu
def test_gpu_insertion_identity(tmp_path_factory):
    """c. modes 0 and DISTINCT, counts only: H1 and H1 with 20 of its edges taken out (seed 2500; five of them between rows longer
    than 64), a labels-only bitmap, wedge, triangle, C4 and diamond: refine_sets(G') - refine_sets(G) == refine_sets_delta(G', F).
    The context is reloaded between the two graphs"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g1, deg = h["g"], h["deg"]
    e = _und_edges(g1)
    hubs = e[(deg[e[:, 0]] > 64) & (deg[e[:, 1]] > 64)]
    assert len(hubs) >= 5
    rng = np.random.default_rng(2500)
    F = np.concatenate([hubs[rng.choice(len(hubs), 5, replace=False)], e[rng.choice(len(e), 15, replace=False)]])
    assert len(_codes(F, g1["n"])) == 20
    g0 = _without(g1, F)
    names = ("wedge", "triangle", "C4", "diamond")
    bms = {name: _label_bitmap(g1, h["q"][name]) for name in names}
    eng = ex._engine(binding, g1, h["sn"], 2)
    try:
        new = {(name, d): eng.refine_sets(h["q"][name], bms[name], limit=FULL, distinct=d)[0] for name in names for d in (False, True)}
        delta = {(name, d): eng.refine_sets_delta(h["q"][name], bms[name], F, distinct=d)[0] for name in names for d in (False, True)}
        eng.load_csr(g0["offsets"], g0["nbrs"], g0["labels"])
        for key, want in new.items():
            old = eng.refine_sets(h["q"][key[0]], bms[key[0]], limit=FULL, distinct=key[1])[0]
            assert want - old == delta[key] > 0, key + (want, old, delta[key])
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_limit_and_cap(tmp_path_factory):
    """d. K4 and the wedge on H1 with the F of _h1_delta, the four modes.  Limits 1, Delta - 1, Delta, Delta + 1: *answers ==
    min(Delta, limit), and the rows are pairwise different valid maps of the mode inside the sets that touch F.  matches_cap 0, 1
    and Delta - 1 with the limit open: Delta, and exactly min(Delta, cap) rows.  K4 in mode 0 has Delta = 5 400, far past the
    1 024-find flush; twice on one context"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    g, F = h["g"], f["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for _ in range(2):
            for name in ("K4", "wedge"):
                qp, bm = h["q"][name], h["bm"][name]["ld"]
                qe = _qedges(qp)
                for distinct, induced in MODES:
                    delta = f["want"][name, "ld", distinct, induced]
                    assert delta > 2
                    pairs = re_._pairs(qp) if distinct else None
                    for limit in (1, delta - 1, delta, delta + 1):
                        got, rows, _ = eng.refine_sets_delta(qp, bm, F, limit=limit, matches_cap=delta + 1, distinct=distinct,
                                                             induced=induced)
                        assert got == min(delta, limit) == len(rows), (name, distinct, induced, limit, got, len(rows))
                        ri._assert_rows(g, qp, bm, rows, induced, pairs)
                        assert _touches(rows, qe, F, g["n"]).all()
                    for cap in (0, 1, delta - 1):
                        got, rows, _ = eng.refine_sets_delta(qp, bm, F, matches_cap=cap, distinct=distinct, induced=induced)
                        assert got == delta and len(rows) == cap, (name, distinct, induced, cap, got, len(rows))
                        ri._assert_rows(g, qp, bm, rows, induced, pairs)
                        assert _touches(rows, qe, F, g["n"]).all()
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_query_sizes(tmp_path_factory, tmp_path):
    """e. nq == 1: 0 whatever F is (nothing is launched: device ms stays 0).  nq == 2: depth 1 is the leaf; mode 0 gives 2 |F| and
    DISTINCT |F| on one label.  nq == 8: the 8-vertex path on the 33-cycle in the four modes, and K8 on a K10 planted in a sparse
    graph, DISTINCT (45 matches; 44 through 12 of the clique's edges, host form).  nq == 32: the 32-vertex path on the 32- and
    the 33-cycle in the four modes with F = three edges, then all edges -- position 31 carries bit 30 of older, gt and non, and
    with the all-ones bitmap, where the order starts elsewhere, bit 31 of non.  The reversed-id files of test_refine_edge_counts on
    H1, which renumber the query edges"""
    from gnnpe_amd import binding, synth
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    g, F = h["g"], f["F"]
    nF = len(_codes(F, g["n"]))
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            got, rows, ms = eng.refine_sets_delta(h["q"]["vertex"], h["bm"]["vertex"][b], F, matches_cap=4)
            assert (got, len(rows), ms) == (0, 0, 0.0)
            got, rows, ms = eng.refine_sets_delta(h["q"]["edge"], h["bm"]["edge"][b], np.zeros((0, 2), np.int64), matches_cap=4)
            assert (got, len(rows), ms) == (0, 0, 0.0)
        for b in ("ld", "ones"):
            assert eng.refine_sets_delta(h["q"]["edge"], h["bm"]["edge"][b], F)[0] == 2 * nF
            got, rows, _ = eng.refine_sets_delta(h["q"]["edge"], h["bm"]["edge"][b], F, matches_cap=nF, distinct=True)
            assert got == nF == len(rows) and np.array_equal(np.unique(rows[:, 0].astype(np.int64) * g["n"] + rows[:, 1]), _codes(F, g["n"]))
        for (name, b), r in re_._h1_reversed(tmp_path_factory).items():
            for distinct, induced in MODES:
                want = binding.host_refine_sets_delta(g, r["qp"], r["bm"], F, FULL, distinct=distinct, induced=induced)
                _device_equals_host(binding, eng, g, r["qp"], r["bm"], F, distinct, induced, want, ("rev", name, b, distinct, induced))
    finally:
        eng.close()
    p8, p32 = sh._path_file(tmp_path, 8), sh._path_file(tmp_path, 32)
    for n, qp in ((33, p8), (32, p32), (33, p32)):
        cyc = sh._cycle_graph(n)
        E = _und_edges(cyc)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            nq = binding.host_load_graph(qp)["n"]
            for bm in (ex._ld_bitmap(cyc, qp), sh._ones(nq, n)):
                for distinct, induced in MODES:
                    for Fc in (E[[0, 1, n // 2]], E):
                        want = binding.host_refine_sets_delta(cyc, qp, bm, Fc, FULL, distinct=distinct, induced=induced)
                        if len(Fc) == len(E):
                            assert want == binding.host_refine_sets(cyc, qp, bm, FULL, distinct=distinct, induced=induced)
                        _device_equals_host(binding, eng, cyc, qp, bm, Fc, distinct, induced, want, (n, nq, distinct, induced))
        finally:
            eng.close()
    k10 = re_._planted_k10()
    k8 = str(tmp_path / "K8.graph")
    ex._write_query(k8, 8, {(a, b) for a in range(8) for b in range(a + 1, 8)}, [0] * 8)
    bm = ex._ld_bitmap(k10, k8)
    clique = [(40 * a, 40 * b) for a in range(10) for b in range(a + 1, 10)][:12]
    want = binding.host_refine_sets_delta(k10, k8, bm, clique, FULL, distinct=True)
    assert want == 44 and binding.host_refine_sets(k10, k8, bm, FULL, distinct=True) == 45
    eng = ex._engine(binding, k10, synth.degree_order(k10["offsets"]), 2)
    try:
        _device_equals_host(binding, eng, k10, k8, bm, clique, True, False, want, ("K8",))
        assert eng.refine_sets_delta(k8, bm, _und_edges(k10), distinct=True)[0] == 45
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, seed):
    """f. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of bitmap)
    in the four modes, F a random subset of the edges whose size is drawn from {1, 2, |E| / 4, |E|}: device == host form, rows as
    in (a)"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    E = _und_edges(g)
    rng = np.random.default_rng(2600 + seed)
    size = (1, 2, max(1, len(E) // 4), len(E))[int(rng.integers(0, 4))]
    F = E[rng.choice(len(E), min(size, len(E)), replace=False)]
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for distinct, induced in MODES:
            want = binding.host_refine_sets_delta(g, c["qp"], c["bm"], F, FULL, distinct=distinct, induced=induced)
            _device_equals_host(binding, eng, g, c["qp"], c["bm"], F, distinct, induced, want, (seed, c["which"], len(F), distinct, induced),
                                rows_too=want <= ROWS_MAX)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory, tmp_path):
    """g. a non-edge pair among valid ones returns GNNPE_ERR_ARG with *answers == 0 -- found on the device, in the call's one wait
    -- and the NEXT valid call on the same context returns the right Delta; x == y, an id >= n, unknown mode bits; 33 query
    vertices; the multigraph state; a context whose rows did not come through gnnpe_load_csr"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_delta(tmp_path_factory)
    g, F = h["g"], f["F"]
    qp, bm = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    want = f["want"]["triangle", "ld", False, False]
    iso = np.nonzero(h["deg"] == 0)[0]
    o = g["offsets"].astype(np.int64)
    x = int(np.argmax(h["deg"]))  # a non-edge between two vertices that have rows: the longest row and a vertex it does not hold
    far = (x, next(int(y) for y in np.nonzero(h["deg"] > 0)[0] if y != x and y not in g["nbrs"][o[x]:o[x + 1]]))
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        assert _raw_device(binding, eng, qp, bm, F) == (0, want)
        for bad in ((int(iso[0]), int(iso[1])), far, (far[1], far[0])):
            for mode in (0, 1, 2, 3):
                assert _raw_device(binding, eng, qp, bm, F.tolist() + [bad], mode=mode) == (-1, 0), (bad, mode)
                assert b"not an edge" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, qp, bm, F) == (0, want)
            with pytest.raises(binding.GnnpeError, match="not an edge"):
                eng.refine_sets_delta(qp, bm, [bad] + F.tolist(), matches_cap=10)
            assert eng.refine_sets_delta(qp, bm, F, matches_cap=3)[0] == want
        for bad, msg in (((7, 7), b"loop"), ((3, g["n"]), b"does not have"), ((g["n"] + 5, 2), b"does not have")):
            assert _raw_device(binding, eng, qp, bm, F.tolist() + [bad]) == (-1, 0) and msg in binding.load().gnnpe_last_error()
        for mode in (4, 1 << 31):
            assert _raw_device(binding, eng, qp, bm, F, mode=mode) == (-1, 0) and b"unknown mode" in binding.load().gnnpe_last_error()
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets_delta(sh._path_file(tmp_path, 33), sh._ones(33, g["n"]), F)
        assert _raw_device(binding, eng, qp, bm, F) == (0, want)  # the context still answers
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.refine_sets_delta(qp, bm, F)
    finally:
        eng.close()
    bare = binding.Engine(0)
    try:
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            bare.refine_sets_delta(qp, bm, F)
    finally:
        bare.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q,counts", [("q1", (46, 23, 26, 13)), ("q2", (34, 34, 33, 33))])
def test_gpu_cli_delta_edges(tmp_path, test_graph, q, counts):
    """h. gnnpe_main -m online --exact --refine sets --delta-edges on the golden test graph, q1 and q2: the answer line carries the
    host form's Delta on the label/degree bitmap (the exact filter's sets are complete) in the four modes, for F = 20 random edges
    and six of the adjacency entries that carry a match (taken from host_refine_sets_edge_counts; seed 2700), written in both
    orientations and with a repeat; with --matches the file holds Delta pairwise different rows that touch F.  Host form: q1 46,
    23, 26, 13 of 266, 133, 204, 102 matches; q2 34, 34, 33, 33 of 52, 52, 51, 51.  A file with a loop is refused"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    E = _und_edges(test_graph)
    rng = np.random.default_rng(2700)
    src, _ = re_._csr_keys(test_graph)
    used = np.nonzero(binding.host_refine_sets_edge_counts(test_graph, qp, ld)[2].sum(axis=0))[0]
    used = used[rng.choice(len(used), 6, replace=False)]
    F = np.concatenate([E[rng.choice(len(E), 20, replace=False)], np.stack([src[used], test_graph["nbrs"][used].astype(np.int64)], axis=1)])
    ef = str(tmp_path / "edges.txt")
    open(ef, "w").write("".join(f"{x} {y}\n" if i % 2 else f"{y} {x}\n" for i, (x, y) in enumerate(F.tolist() + F[:1].tolist())))
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--delta-edges", ef]
    for k, (distinct, induced) in enumerate(MODES):
        want = binding.host_refine_sets_delta(test_graph, qp, ld, F, FULL, distinct=distinct, induced=induced)
        assert want == counts[k] < binding.host_refine_sets(test_graph, qp, ld, FULL, distinct=distinct, induced=induced)
        out = str(tmp_path / f"m{k}.txt")
        cmd = base + ["--matches", out] + (["--distinct"] if distinct else []) + (["--induced"] if induced else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        assert ans == want, (distinct, induced, ans, want)
        rows = np.loadtxt(out, dtype=np.int64, ndmin=2)
        assert len(rows) == want and len(np.unique(rows, axis=0)) == want and _touches(rows, _qedges(qp), F, n).all()
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("0 0\n")
    r = subprocess.run(base[:-1] + [bad], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "loop" in r.stderr and "Answer Number" not in r.stdout
