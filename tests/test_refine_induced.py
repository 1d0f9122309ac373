"""Induced matching (include/gnnpe_online.h, ABI version 12): I(C, limit) and ID(C, limit) on the host
(gnnpe_host_refine_sets_mode), on the device in one shot (gnnpe_refine_sets_mode) and page by page
(gnnpe_refine_pages_open_mode), and `gnnpe_main --induced`.

An induced match is a monomorphism that also sends every two non-adjacent query vertices to two non-adjacent data vertices.  The
yardsticks are independent of the library: networkx's `subgraph_isomorphisms_iter` (its induced notion), the monomorphism rows
with the rows dropped that have a data edge between the images of a query non-edge (_induced_mask), and the closed form of the
induced wedge, sum d(d-1) - sum(A^2 o A).  The host form is pinned to those first (tests 1-5); the device is then held to the host
form, and its rows to _induced_mask and, on the small graphs, to networkx's row set."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_distinct as rd
import test_refine_pages as rp
import test_refine_sets as rs
import test_refine_sets_shapes as sh

sets_lines = sh.sets_lines  # the fixture that collects the `[refine_sets]` lines

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE

IND_SHAPES = ("wedge", "C4", "diamond", "C5", "star5", "triangle", "K4", "edge")
NONEDGE_SHAPES = ("wedge", "C4", "diamond", "C5", "star5")  # the shapes with a non-adjacent pair
NON_EDGES = {"wedge": 1, "C4": 2, "diamond": 1, "C5": 5, "star5": 6, "vertex": 0, "edge": 0, "triangle": 0, "K4": 0, "K5": 0}
# limits on H1: C5 has more than 10^7 monomorphisms and star5 more than 10^7 induced matches, and the host form walks every one it
# counts.  Under 10^6 C5 still has its whole I on the thinned bitmap (564 708) and its whole ID on all three (238 078 on the
# label/degree bitmap); its other counts and all of star5's meet the limit, where the rows still tell right from wrong
H1_IND_LIMIT = {"wedge": 10 ** 7, "C4": 10 ** 7, "diamond": 10 ** 7, "C5": 10 ** 6, "star5": 10 ** 6}
MODES = ((False, False), (False, True), (True, True))  # (distinct, induced): mode 0, INDUCED, INDUCED | DISTINCT


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _non_edges(qp):
    """the pairs a < b of query vertices that are not adjacent"""
    q, edges = rd._query_edges(qp)
    have = set(edges)
    return [(a, b) for a in range(q["n"]) for b in range(a + 1, q["n"]) if (a, b) not in have]


def _induced_mask(g, qp, rows):
    """mask of the rows with no data edge between the images of two non-adjacent query vertices"""
    rows = np.asarray(rows, np.int64)
    ok = np.ones(len(rows), bool)
    if len(rows) == 0:
        return ok
    n = len(g["labels"])
    deg = np.diff(g["offsets"].astype(np.int64))
    keys = np.repeat(np.arange(n, dtype=np.int64), deg) * n + g["nbrs"].astype(np.int64)  # ascending: rows sorted by id
    for a, b in _non_edges(qp):
        k = rows[:, a] * n + rows[:, b]
        pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        ok &= keys[pos] != k
    return ok


def _nx_induced(g, qpath):
    """every induced match of the query in the data graph (networkx's subgraph isomorphisms) as a row: column u = image of u"""
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
    for m in iso.GraphMatcher(D, Q, node_match=lambda a, b: a["l"] == b["l"]).subgraph_isomorphisms_iter():
        inv = {u: v for v, u in m.items()}
        rows.append([inv[u] for u in range(q["n"])])
    return np.array(rows, np.int64).reshape(len(rows), q["n"])


_IND = {}


def _ind_cases(tmp_path_factory):
    """the 15 small graphs of sh._nx_cases with the eight shapes of IND_SHAPES, every query label 0 and labels alternating 0, 1 by
    vertex id: networkx's monomorphisms (`emb`), networkx's induced matches (`ind`) and the three bitmaps.  The cases sh._nx_cases
    already holds are taken from it; the wedge is added here by the same recipe (sh._nx_case)"""
    if "cases" in _IND:
        return _IND["cases"]
    base = sh._nx_cases(tmp_path_factory)
    by = {(c["gi"], c["name"], c["variant"]): c for c in base}
    graphs = {c["gi"]: c["g"] for c in base}
    assert len(graphs) == 15
    tmp = tmp_path_factory.mktemp("induced")
    out = []
    for gi in sorted(graphs):
        for name in IND_SHAPES:
            for v in (0, 1):
                c = dict(by.get((gi, name, v)) or sh._nx_case(tmp, gi, graphs[gi], name, v))
                c["ind"] = _nx_induced(c["g"], c["qp"])
                out.append(c)
    _IND["cases"] = out
    return out


_H1I = {}


def _h1_induced(tmp_path_factory):
    """sh._h1 with the five shapes that have a non-edge: query files, the three bitmaps (thinning seed 1700 + shape), |Aut|, the pairs
    and the host form's R, I and ID on each bitmap under H1_IND_LIMIT (computed once)"""
    if _H1I:
        return _H1I
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    tmp = tmp_path_factory.mktemp("h1i")
    q, bms, want, aut, pairs = {}, {}, {}, {}, {}
    for k, name in enumerate(NONEDGE_SHAPES):
        q[name] = sh._shape_file(tmp, name)
        ld = ex._ld_bitmap(g, q[name])
        bms[name] = dict(ld=ld, thin=rs._subset(ld, g["n"], 1700 + k), ones=sh._ones(sh.SHAPES[name][0], g["n"]))
        aut[name], pairs[name] = binding.host_query_symmetry(q[name])
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                want[name, b, distinct, induced] = binding.host_refine_sets(g, q[name], bms[name][b], H1_IND_LIMIT[name],
                                                                            distinct=distinct, induced=induced)
    _H1I.update(h=h, g=g, q=q, bm=bms, want=want, aut=aut, pairs=pairs)
    return _H1I


def _assert_rows(g, qp, bm, rows, induced, pairs=None):
    """valid, pairwise different embeddings inside the sets; induced: no data edge under a query non-edge; pairs: ordered"""
    rs._assert_rows_are_embeddings(g, qp, bm, rows)
    if induced:
        assert _induced_mask(g, qp, rows).all(), "a row maps a query non-edge onto a data edge"
    if pairs is not None:
        assert rd._ordered(rows, pairs).all()


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_host_form_against_networkx(tmp_path_factory):
    """1. the 15 small graphs, eight shapes, both label variants, on the label/degree, thinned and all-ones bitmaps: the host form's I
    is the number of networkx's subgraph isomorphisms inside the sets, and the number of monomorphism rows inside the sets with no
    data edge under a query non-edge (the two row sets are equal).  Of the 150 cases whose shape has a non-edge at least a quarter
    have 0 < I < R on the label/degree bitmap; triangle, K4 and edge give I == R"""
    from gnnpe_amd import binding
    cases = _ind_cases(tmp_path_factory)
    telling, with_nonedge = 0, 0
    for c in cases:
        g, qp = c["g"], c["qp"]
        tag = (c["gi"], c["name"], c["variant"])
        assert len(_non_edges(qp)) == NON_EDGES[c["name"]]
        for b in sh.BITMAPS:
            inside = c["emb"][rs._in_sets(c[b], c["emb"])]
            kept = inside[_induced_mask(g, qp, inside)]
            nxin = c["ind"][rs._in_sets(c[b], c["ind"])]
            assert sh._row_set(kept) == sh._row_set(nxin) and len(kept) == len(nxin), (tag, b)
            i = binding.host_refine_sets(g, qp, c[b], FULL, induced=True)
            assert i == len(nxin), (tag, b, i, len(nxin))
            r = binding.host_refine_sets(g, qp, c[b], FULL)
            assert r == len(inside)
            if c["name"] not in NONEDGE_SHAPES:
                assert i == r, (tag, b)
            elif b == "ld":
                with_nonedge += 1
                telling += 0 < i < r
    assert with_nonedge == 150 and telling * 4 >= with_nonedge, (telling, with_nonedge)


def test_closed_forms_on_h1(tmp_path_factory):
    """2. H1 (one label): the induced wedges are sum d(d-1) - sum(A^2 o A) -- every wedge whose ends are adjacent closes a triangle,
    and a triangle holds six such wedges, as many as it has embeddings -- on the label/degree and the all-ones bitmap, and on the
    subgraph induced by one common subset S cut into every set (seed 77).  vertex, edge, triangle, K4, K5: I == R on every bitmap"""
    from gnnpe_amd import binding
    hi = _h1_induced(tmp_path_factory)
    h, g = hi["h"], hi["g"]
    closed = h["closed"]
    want = closed["wedge"] - closed["triangle"]
    assert 0 < want < closed["wedge"]
    for b in ("ld", "ones"):
        assert hi["want"]["wedge", b, False, True] == want
        assert hi["want"]["wedge", b, True, True] * 2 == want
    sub, s = sh._common_subset(hi["bm"]["wedge"]["ld"], g["n"], 77)
    inside = sh._closed_forms(g, s)
    assert 0 < inside["wedge"] - inside["triangle"] < want
    assert binding.host_refine_sets(g, hi["q"]["wedge"], sub, FULL, induced=True) == inside["wedge"] - inside["triangle"]
    for name in ("vertex", "edge", "triangle", "K4", "K5"):
        for b in sh.BITMAPS:
            assert binding.host_refine_sets(g, h["q"][name], h["bm"][name][b], sh.H1_LIMIT, induced=True) == h["want"][name, b] > 0


def test_extremes(tmp_path):
    """3. the 32-vertex path on the 32-cycle with one label: R = 64 and I = 0 -- the two ends land on adjacent vertices, the non-edge
    of the last position with the first (bit 0 of non[31]); on the 33-cycle I = R = 66.  Limit 0 gives 0, a limit below the count
    the limit.  An unknown mode bit is refused by the host function"""
    import ctypes as C
    from gnnpe_amd import binding
    qp = sh._path_file(tmp_path, 32)
    for n, r, i in ((32, 64, 0), (33, 66, 66)):
        g = sh._cycle_graph(n)
        for bm in (ex._ld_bitmap(g, qp), sh._ones(32, n)):
            assert binding.host_refine_sets(g, qp, bm, FULL) == r
            assert binding.host_refine_sets(g, qp, bm, FULL, induced=True) == i
            assert binding.host_refine_sets(g, qp, bm, FULL, induced=True, distinct=True) * 2 == i
            assert binding.host_refine_sets(g, qp, bm, 0, induced=True) == 0
            assert binding.host_refine_sets(g, qp, bm, 10, induced=True) == min(10, i)
            assert binding.host_refine_sets(g, qp, bm, i + 1, induced=True) == i
    g = sh._cycle_graph(33)
    o, nb, lb, bm = (np.ascontiguousarray(x, np.uint32) for x in (g["offsets"], g["nbrs"], g["labels"], sh._ones(32, 33)))
    u32p = C.POINTER(C.c_uint32)
    out = C.c_uint64(7)
    args = [33] + [x.ctypes.data_as(u32p) for x in (o, nb, lb)] + [qp.encode(), bm.ctypes.data_as(u32p), FULL]
    online = binding.load_online()
    assert online.gnnpe_host_refine_sets_mode(*args, 4, C.byref(out)) != 0
    assert b"unknown mode" in binding.load().gnnpe_last_error()
    for mode, want in ((0, 66), (binding.MATCH_DISTINCT, 33), (binding.MATCH_INDUCED, 66), (3, 33)):
        assert online.gnnpe_host_refine_sets_mode(*args, mode, C.byref(out)) == 0 and out.value == want, mode


def test_distinct_and_induced(tmp_path_factory):
    """4. the cases of test 1.  Closed bitmaps (label/degree, all ones): ID |Aut| == I, ID is the number of keys of networkx's induced
    matches inside the sets, and the induced matches that satisfy the pairs are one per key.  Thinned bitmap: ID is the number of
    networkx's induced matches inside the sets that satisfy the pairs"""
    from gnnpe_amd import binding
    some = 0
    for c in _ind_cases(tmp_path_factory):
        g, qp = c["g"], c["qp"]
        aut, pairs = binding.host_query_symmetry(qp)
        _, edges = rd._query_edges(qp)
        for b in sh.BITMAPS:
            inside = c["ind"][rs._in_sets(c[b], c["ind"])]
            rows = inside[rd._ordered(inside, pairs)]
            idd = binding.host_refine_sets(g, qp, c[b], FULL, distinct=True, induced=True)
            assert idd == len(rows), (c["gi"], c["name"], c["variant"], b, idd, len(rows))
            if b != "thin":
                keys = rd._keys(inside, edges, g["n"])
                assert rd._keys(rows, edges, g["n"]) == keys and len(rows) == len(keys)
                assert idd * aut == binding.host_refine_sets(g, qp, c[b], FULL, induced=True) == len(inside)
                some += idd > 0 and aut >= 2 and c["name"] in NONEDGE_SHAPES
    assert some >= 40, some


_FUZZ = {}


def _fuzz_case(seed, tmp_path_factory):
    """sh._fuzz_case(seed) -- random graph, random connected query of 1-6 vertices, one of four kinds of bitmap, a forced shift or
    none -- with the host form's I and ID and a limit out of (1, I // 2, I, 2^40)"""
    if seed in _FUZZ:
        return _FUZZ[seed]
    from gnnpe_amd import binding
    c = dict(sh._fuzz_case(seed, tmp_path_factory))
    rng = np.random.default_rng(9000 + seed)
    c["i"] = binding.host_refine_sets(c["g"], c["qp"], c["bm"], FULL, induced=True)
    c["id"] = binding.host_refine_sets(c["g"], c["qp"], c["bm"], FULL, induced=True, distinct=True)
    c["pairs"] = binding.host_query_symmetry(c["qp"])[1]
    c["ilimit"] = (1, c["i"] // 2, c["i"], 1 << 40)[int(rng.integers(0, 4))]
    _FUZZ[seed] = c
    return c


def test_fuzz_cases_are_telling(tmp_path_factory):
    """5. the 24 fuzz cases of test_refine_sets_shapes before any device sees them: at least 6 with 0 < I < R, I <= R and ID <= I
    throughout, and I == R where the query has no non-edge"""
    cases = [_fuzz_case(s, tmp_path_factory) for s in sh.FUZZ_SEEDS]
    assert sum(0 < c["i"] < c["count"] for c in cases) >= 6, [(c["i"], c["count"]) for c in cases]
    for c in cases:
        assert c["id"] <= c["i"] <= c["count"]
        if not _non_edges(c["qp"]):
            assert c["i"] == c["count"]


def test_cli_refuses_induced_without_refine_sets(tmp_path):
    """12a. --induced without --refine sets exits 1 with its message before the graph is read or a GPU is touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    for extra in (["--induced"], ["--refine", "start", "--induced"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--induced needs --refine sets" in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_shapes_on_small_graphs(tmp_path_factory, gi):
    """6a. the shapes with both label variants on one of the 15 small graphs, label/degree and thinned bitmap: the induced rows are
    networkx's induced matches inside the sets; induced and distinct: those of them that satisfy the pairs"""
    from gnnpe_amd import binding, synth
    cases = [c for c in _ind_cases(tmp_path_factory) if c["gi"] == gi]
    assert len(cases) == 2 * len(IND_SHAPES)
    g = cases[0]["g"]
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            pairs = binding.host_query_symmetry(c["qp"])[1]
            for b in ("ld", "thin"):
                inside = c["ind"][rs._in_sets(c[b], c["ind"])]
                got, _, rows = eng.refine_sets(c["qp"], c[b], limit=FULL, matches_cap=len(inside) + 5, induced=True)
                assert got == len(inside) == len(rows), (gi, c["name"], c["variant"], b, got, len(inside))
                assert sh._row_set(rows) == sh._row_set(inside)
                want = inside[rd._ordered(inside, pairs)]
                got, _, rows = eng.refine_sets(c["qp"], c[b], limit=FULL, matches_cap=len(inside) + 5, induced=True, distinct=True)
                assert got == len(want) == len(rows) and sh._row_set(rows) == sh._row_set(want), (gi, c["name"], c["variant"], b)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(7))
def test_gpu_every_first_level_shift_on_h1(tmp_path_factory, monkeypatch, sets_lines, shift):
    """6. H1 with the first-level chunk forced to 1 << shift entries: wedge, C4, diamond, C5 and star5 in mode 0, INDUCED and
    INDUCED | DISTINCT on the three bitmaps count what the host form counts; the rows (at most 65 536) are valid, different,
    induced and ordered as the mode asks; the line of an induced call ends in `nonedges=K`, the line of a plain call does not name
    it.  All 384 976 induced wedges on the label/degree bitmap: among the images of the two ends are pairs whose first has the
    shorter row and pairs whose second has, each with a row longer than 64 on the long side -- the non-edge search took both
    directions of its shorter-row choice"""
    from gnnpe_amd import binding
    hi = _h1_induced(tmp_path_factory)
    h, g = hi["h"], hi["g"]
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        sets_lines()
        for name in NONEDGE_SHAPES:
            qp, limit = hi["q"][name], H1_IND_LIMIT[name]
            for b in sh.BITMAPS:
                bm = hi["bm"][name][b]
                for distinct, induced in MODES:
                    want = hi["want"][name, b, distinct, induced]
                    got, _, rows = eng.refine_sets(qp, bm, limit=limit, matches_cap=sh.H1_CAP, distinct=distinct, induced=induced)
                    print(f"shift {shift} {name} {b} distinct={distinct} induced={induced}: device {got}, host {want}")
                    assert got == want, (shift, name, b, distinct, induced, got, want)
                    assert len(rows) == min(want, sh.H1_CAP)
                    _assert_rows(g, qp, bm, rows, induced, hi["pairs"][name] if distinct else None)
                    (ln,) = sets_lines()
                    assert ln["shift"] == shift and ln["forced"] == 1, ln
                    if induced:
                        assert ln["nonedges"] == NON_EDGES[name] and ("pairs" in ln) == distinct, ln
                    else:
                        assert "nonedges" not in ln and "pairs" not in ln, ln
        qp, bm, want = hi["q"]["wedge"], hi["bm"]["wedge"]["ld"], hi["want"]["wedge", "ld", False, True]
        got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=want, induced=True)
        assert got == want == len(rows)
        _assert_rows(g, qp, bm, rows, True)
        ((a, b),) = _non_edges(qp)
        da, db = h["deg"][rows[:, a].astype(np.int64)], h["deg"][rows[:, b].astype(np.int64)]
        assert ((da < db) & (db > 64)).any() and ((db < da) & (da > 64)).any() and min(da.min(), db.min()) == 1
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cycles_of_32_and_33(tmp_path):
    """7. the 32-vertex one-label path on the 32-cycle: R = 64 and I = 0, one-shot and paged; on the 33-cycle I = R = 66, ID = 33,
    and the rows are networkx's induced matches"""
    from gnnpe_amd import binding, synth
    qp = sh._path_file(tmp_path, 32)
    for n, r, i in ((32, 64, 0), (33, 66, 66)):
        g = sh._cycle_graph(n)
        ind = _nx_induced(g, qp)
        assert len(ind) == i
        eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
        try:
            for bm in (ex._ld_bitmap(g, qp), sh._ones(32, n)):
                assert eng.refine_sets(qp, bm, limit=FULL)[0] == r
                got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=100, induced=True)
                assert got == i == len(rows) and sh._row_set(rows) == sh._row_set(ind)
                got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=100, induced=True, distinct=True)
                assert got * 2 == i and len(rows) == got
                _assert_rows(g, qp, bm, rows, True, binding.host_query_symmetry(qp)[1])
                with eng.open_match_cursor(qp, bm, 7, induced=True) as cur:
                    paged, _, _ = rp._drain(cur, 7)
                assert sh._row_set(paged) == sh._row_set(ind) and len(paged) == i
        finally:
            eng.close()


@pytest.mark.gpu
def test_gpu_queries_without_a_non_edge(tmp_path_factory, sets_lines):
    """8. the single vertex, the edge and K4 on H1: the induced call returns R (2 000, the adjacency entries, 109 224), induced and
    distinct returns D, the rows are valid, and the line says nonedges=0"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        sets_lines()
        for name in ("vertex", "edge", "K4"):
            qp, bm, r = h["q"][name], h["bm"][name]["ld"], h["want"][name, "ld"]
            got, _, rows = eng.refine_sets(qp, bm, limit=sh.H1_LIMIT, matches_cap=sh.H1_CAP, induced=True)
            assert got == r and len(rows) == min(r, sh.H1_CAP), (name, got, r)
            rs._assert_rows_are_embeddings(g, qp, bm, rows)
            (ln,) = sets_lines()
            assert ln["nonedges"] == 0 and "pairs" not in ln, ln
            d = eng.refine_sets(qp, bm, limit=sh.H1_LIMIT, distinct=True)[0]
            assert eng.refine_sets(qp, bm, limit=sh.H1_LIMIT, distinct=True, induced=True)[0] == d
            said = sets_lines()
            assert "nonedges" not in said[0] and said[1]["nonedges"] == 0 and said[1]["pairs"] == said[0]["pairs"], said
            with eng.open_match_cursor(qp, bm, 50000, induced=True) as cur:
                paged, _, _ = rp._drain(cur, 50000)
            assert len(paged) == r
        assert h["want"]["vertex", "ld"] == 2000 and h["want"]["K4", "ld"] == 109224
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 6])
def test_gpu_paged(tmp_path_factory, monkeypatch, shift):
    """9. the induced cursor on H1, C4 and wedge on a bitmap thinned to a quarter per query vertex (some thousand induced matches):
    pages of 1, 63, 64 and 65 rows hold the one-shot induced row set, every row once, every page before the last full, and after
    the first page some wave is suspended.  Limits around a page of 64 rows.  An induced and a plain cursor interleaved on one
    context deliver their own sets"""
    from gnnpe_amd import binding
    hi = _h1_induced(tmp_path_factory)
    h, g = hi["h"], hi["g"]
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for k, name in enumerate(("C4", "wedge")):
            qp = hi["q"][name]
            bm = rs._subset(hi["bm"][name]["ld"], g["n"], 1800 + k, keep=0.25)
            want = binding.host_refine_sets(g, qp, bm, FULL, induced=True)
            assert 300 < want < 20000 and want < binding.host_refine_sets(g, qp, bm, FULL), (name, want)
            got, _, once = eng.refine_sets(qp, bm, limit=FULL, matches_cap=want + 5, induced=True)
            assert got == want == len(once)
            _assert_rows(g, qp, bm, once, True)
            for page_rows in (1, 63, 64, 65):
                with eng.open_match_cursor(qp, bm, page_rows, induced=True) as cur:
                    rows, n_pages, first = rp._drain(cur, page_rows)
                assert len(rows) == want and sh._row_set(rows) == sh._row_set(once), (shift, name, page_rows)
                assert -(-want // page_rows) <= n_pages <= -(-want // page_rows) + 1
                assert first["suspended_waves"] >= 1 and first["pages"] == 1 and first["rows"] == page_rows, first
            for limit in (63, 64, 65, 128, 129):
                with eng.open_match_cursor(qp, bm, 64, limit=limit, induced=True) as cur:
                    rows, _, _ = rp._drain(cur, 64)
                assert len(rows) == min(limit, want), (name, limit, len(rows))
                _assert_rows(g, qp, bm, rows, True)
                with eng.open_match_cursor(qp, bm, 64, limit=limit, induced=True, distinct=True) as cur:
                    rows, _, _ = rp._drain(cur, 64)
                assert len(rows) == min(limit, binding.host_refine_sets(g, qp, bm, FULL, induced=True, distinct=True))
                _assert_rows(g, qp, bm, rows, True, hi["pairs"][name])
        # one induced and one plain cursor, page about
        qp, bm = hi["q"]["C4"], hi["bm"]["C4"]["thin"]
        cur = {False: eng.open_match_cursor(qp, bm, 30000), True: eng.open_match_cursor(qp, bm, 7000, induced=True)}
        got, done = {False: [], True: []}, {False: False, True: False}
        while not all(done.values()):
            for k in (False, True):
                if not done[k]:
                    rows, done[k] = cur[k].next()
                    got[k].append(rows)
        for k in (False, True):
            cur[k].close()
        plain, ind = np.concatenate(got[False]), np.concatenate(got[True])
        assert len(plain) == hi["want"]["C4", "thin", False, False] and len(ind) == hi["want"]["C4", "thin", False, True]
        _assert_rows(g, qp, bm, plain, False)
        _assert_rows(g, qp, bm, ind, True)
        assert sh._row_set(ind) == sh._row_set(plain[_induced_mask(g, qp, plain)])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, monkeypatch, seed):
    """10. the 24 fuzz cases: the induced call equals the host form's I under the limit and without, induced and distinct its ID; the
    rows are valid, different and induced; the pages of the induced cursor hold I rows, the one-shot row set where that was kept
    whole (counts up to 200 000; above, pages of 2^20 rows are checked as rows)"""
    from gnnpe_amd import binding, synth
    c = _fuzz_case(seed, tmp_path_factory)
    g, qp, bm = c["g"], c["qp"], c["bm"]
    if c["shift"] is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        want = min(c["ilimit"], c["i"])
        assert binding.host_refine_sets(g, qp, bm, c["ilimit"], induced=True) == want
        for _ in range(2):
            got, _, rows = eng.refine_sets(qp, bm, limit=c["ilimit"], matches_cap=min(want, 1 << 16) + 3, induced=True)
            assert got == want and len(rows) == min(want, (1 << 16) + 3), (seed, c["which"], c["shift"], got, want)
            _assert_rows(g, qp, bm, rows, True)
        assert eng.refine_sets(qp, bm, limit=FULL, induced=True)[0] == c["i"], seed
        cap = min(c["id"], 1 << 16) + 3
        got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=cap, induced=True, distinct=True)
        assert got == c["id"] and len(rows) == min(c["id"], cap), (seed, got, c["id"])
        _assert_rows(g, qp, bm, rows, True, c["pairs"])
        small = c["i"] <= 200_000
        page_rows = 257 if small else 1 << 20
        with eng.open_match_cursor(qp, bm, page_rows, induced=True) as cur:
            paged, _, _ = rp._drain(cur, page_rows)
        assert len(paged) == c["i"], (seed, len(paged), c["i"])
        _assert_rows(g, qp, bm, paged, True)
        if small:
            once = eng.refine_sets(qp, bm, limit=FULL, matches_cap=c["i"] + 3, induced=True)[2]
            assert sh._row_set(paged) == sh._row_set(once), seed
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory, tmp_path):
    """11. an unknown mode bit (one-shot and open), a 33-vertex query, page_rows == 0 and a multigraph context are refused with their
    messages, and the context goes on answering"""
    import ctypes as C
    from gnnpe_amd import binding
    hi = _h1_induced(tmp_path_factory)
    h, g = hi["h"], hi["g"]
    qp, bm = hi["q"]["C4"], np.ascontiguousarray(hi["bm"]["C4"]["ld"], np.uint32)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        online, u32p = binding.load_online(), C.POINTER(C.c_uint32)
        out, ms, cur = C.c_uint64(), C.c_double(), C.c_void_p()
        for mode in (4, 7, 1 << 31):
            assert online.gnnpe_refine_sets_mode(eng.ctx, qp.encode(), bm.ctypes.data_as(u32p), FULL, mode, C.byref(out), None, 0,
                                                 C.byref(ms)) == online.gnnpe_refine_pages_open_mode(
                eng.ctx, qp.encode(), bm.ctypes.data_as(u32p), FULL, 10, mode, C.byref(cur)) != 0
            assert b"unknown mode" in binding.load().gnnpe_last_error() and not cur.value
        with pytest.raises(binding.GnnpeError, match="page_rows must be at least 1"):
            eng.open_match_cursor(qp, bm, 0, induced=True)
        p33 = sh._path_file(tmp_path, 33)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets(p33, sh._ones(33, g["n"]), induced=True)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.open_match_cursor(p33, sh._ones(33, g["n"]), 10, induced=True, distinct=True)
        assert not eng._cursors
        assert eng.refine_sets(qp, bm, limit=FULL, induced=True)[0] == hi["want"]["C4", "ld", False, True]
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.refine_sets(qp, bm, induced=True)
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.open_match_cursor(qp, bm, 7, induced=True)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cli_induced(tmp_path, test_graph):
    """12. gnnpe_main -m online --exact --refine sets --induced on the golden test graph, q1 and q2 (266 and 52 exact answers), with and
    without --distinct, with --matches and with --matches --all-matches: the answer is the host form's I (ID) on the label/degree
    bitmap, the file holds one valid induced row per answer, and the --timing line says "induced": true"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    assert rec["q1"]["exact"] == 266 and rec["q2"]["exact"] == 52
    for name in ("q1", "q2"):
        qp = os.path.join(ONLINE, f"{name}.graph")
        ld = ex._ld_bitmap(test_graph, qp)
        pairs = binding.host_query_symmetry(qp)[1]
        for distinct in (False, True):
            want = binding.host_refine_sets(test_graph, qp, ld, FULL, distinct=distinct, induced=True)
            assert want <= rec[name]["exact"]
            for k, extra in enumerate(([], ["--matches"], ["--matches", "--all-matches", "--match-page", "7"])):
                mf = str(tmp_path / f"{name}_{int(distinct)}_{k}.txt")
                cmd = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--induced",
                       "--timing"] + (["--distinct"] if distinct else [])
                for a in extra:
                    cmd += [a, mf] if a == "--matches" else [a]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                assert r.returncode == 0, r.stderr
                ans = next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: "))
                assert int(ans.split()[2]) == want, (name, distinct, extra, ans, want)
                line = json.loads(next(ln for ln in r.stderr.splitlines() if ln.startswith("{")))
                assert line["induced"] is True and line["refine"] == "sets"
                if extra:
                    rows = np.loadtxt(mf, dtype=np.int64, ndmin=2) if want else np.zeros((0, 1), np.int64)
                    assert len(rows) == want
                    if want:
                        _assert_rows(test_graph, qp, ld, rows, True, pairs if distinct else None)
