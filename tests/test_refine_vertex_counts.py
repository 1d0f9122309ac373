"""Per-vertex match counts (include/gnnpe_online.h, ABI version 13): V_m(C)[u][v] = the matches of mode m that send query vertex
u to data vertex v, on the host (gnnpe_host_refine_sets_vertex_counts), on the device (gnnpe_refine_sets_vertex_counts) and through
`gnnpe_main --vertex-counts`.

The host form is held to yardsticks independent of the library first: np.add.at over networkx's rows (monomorphisms, induced
matches, either filtered by the ordering pairs), the closed forms of edge, triangle and wedge on H1, the orbit identity between
the distinct and the plain tables, and the guard semantics of `limit`.  The device is then held to the host form by exact uint64
equality -- at every first-level chunk width, at 1, 2 and 32 query vertices, around the guard, on the fuzz cases -- and, for the
triangle and K4, to np.add.at over the rows the device itself hands back, which does not go through the host form.  star5 on H1
holds 4 596 520 344 maps, which no host form walks inside a test; its centre column, d(d-1)(d-2)(d-3), is checked on the device.

No test reaches a cell above 2^32: that would take more than 4 x 10^9 finds below one image.  Every add is a single 64-bit atomic
(or a 64-bit increment on the host), so there is no carry code to test and no slow case is kept for it."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_distinct as rd
import test_refine_induced as ri
import test_refine_sets as rs
import test_refine_sets_shapes as sh

sets_lines = sh.sets_lines  # (the fixture; the new call owes no `[refine_sets]` line and none is asked of it)

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = ((False, False), (True, False), (False, True), (True, True))  # (distinct, induced): 0, DISTINCT, INDUCED, both


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _table(rows, nq, n):
    """the yardstick: 1 added to cell [u][row[u]] for every row and every query vertex u"""
    t = np.zeros((nq, n), np.uint64)
    rows = np.asarray(rows, np.int64).reshape(-1, nq)
    for u in range(nq):
        np.add.at(t[u], rows[:, u], np.uint64(1))
    return t


_PAIRS = {}


def _pairs(qp):
    from gnnpe_amd import binding
    if qp not in _PAIRS:
        _PAIRS[qp] = binding.host_query_symmetry(qp)[1]
    return _PAIRS[qp]


def _orbits(qp):
    """(|Aut(Q)|, the orbits of the query vertices under the full automorphism group), by networkx"""
    auts = rd._nx_automorphisms(qp)
    nq = len(auts[0])
    return len(auts), sorted({tuple(sorted({a[u] for a in auts})) for u in range(nq)})


_H1T = {}


def _h1_tables(tmp_path_factory):
    """the host form's (answers, table) of every H1 shape on every bitmap in every mode, limit 2^64 - 1, computed once"""
    if _H1T:
        return _H1T
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    for name in sh.H1_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                ans, complete, t = binding.host_refine_sets_vertex_counts(h["g"], h["q"][name], h["bm"][name][b], FULL,
                                                                          distinct=distinct, induced=induced)
                assert complete
                _H1T[name, b, distinct, induced] = (ans, t)
    return _H1T


# ---- CPU: the host form against yardsticks independent of the library --------------------------------------------------------

def test_host_table_against_networkx(tmp_path_factory):
    """1. the 15 small graphs, the eight shapes, both label variants, the three bitmaps, the four modes: the host table is
    np.add.at over networkx's rows inside the sets (monomorphisms for mode 0, induced matches for INDUCED, either filtered by the
    ordering pairs for the DISTINCT modes), and every row of it sums to the host count of the same mode.  At least a quarter of
    the (case, bitmap) pairs have a mode-0 table with two different non-zero values, so a table of ones and zeros would not do"""
    from gnnpe_amd import binding
    cases = ri._ind_cases(tmp_path_factory)
    assert len(cases) == 15 * len(ri.IND_SHAPES) * 2
    varied = total = 0
    for c in cases:
        g, qp = c["g"], c["qp"]
        nq, n = sh.SHAPES[c["name"]][0], g["n"]
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                rows = c["ind"] if induced else c["emb"]
                rows = rows[rs._in_sets(c[b], rows)]
                if distinct:
                    rows = rows[rd._ordered(rows, _pairs(qp))]
                ans, complete, t = binding.host_refine_sets_vertex_counts(g, qp, c[b], FULL, distinct=distinct, induced=induced)
                where = (c["gi"], c["name"], c["variant"], b, distinct, induced)
                assert complete and ans == len(rows), where
                assert t.shape == (nq, n) and t.dtype == np.uint64 and np.array_equal(t, _table(rows, nq, n)), where
                assert (t.sum(axis=1) == ans).all(), where
                assert ans == binding.host_refine_sets(g, qp, c[b], FULL, distinct=distinct, induced=induced), where
                if not distinct and not induced:
                    total += 1
                    varied += len(np.unique(t[t > 0])) >= 2
    assert total == len(cases) * 3 and varied * 4 >= total, (varied, total)


def test_host_table_closed_forms_on_h1(tmp_path_factory):
    """2. H1, one label, label/degree and all-ones bitmaps, mode 0.  Edge: both columns are deg.  Triangle: every column is the row
    sums of A^2 o A.  Wedge (0 - 1 - 2): the centre's column is d(d-1), an end's column the sum over the neighbours w of d(w) - 1.
    (star5's centre column, d(d-1)(d-2)(d-3), has 4.6 x 10^9 maps behind it: test_gpu_star5_centre_column checks it on the device)"""
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    A = sh._adjacency(h["g"])
    d = h["deg"].astype(np.uint64)
    tri = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel().astype(np.uint64)
    ends = np.asarray(A @ (h["deg"] - 1)).ravel().astype(np.uint64)
    assert tri.sum() == 28446 and (d > 64).any()
    for b in ("ld", "ones"):
        ans, t = tabs["edge", b, False, False]
        assert ans == d.sum() and np.array_equal(t[0], d) and np.array_equal(t[1], d), b
        ans, t = tabs["triangle", b, False, False]
        assert ans == tri.sum() and all(np.array_equal(t[u], tri) for u in range(3)), b
        ans, t = tabs["wedge", b, False, False]
        assert np.array_equal(t[1], d * (d - 1)) and np.array_equal(t[0], ends) and np.array_equal(t[2], ends), b
        assert ans == int((d * (d - 1)).sum())
        ans, t = tabs["vertex", b, False, False]
        assert ans == h["g"]["n"] and (t == 1).all(), b


def test_orbit_identity(tmp_path_factory):
    """3. the small graphs on the label/degree bitmap (closed under Aut(Q)), plain and induced, the orbits of the full
    automorphism group by networkx: for every orbit O, u0 in O and v, sum over u in O of V_D[u][v] * |Aut| == V_R[u0][v] * |O| --
    both sides are |Aut| times the occurrences in which v plays a role of O (the header's reading of the two tables)"""
    from gnnpe_amd import binding
    telling = 0
    for c in ri._ind_cases(tmp_path_factory):
        n_aut, orbits = _orbits(c["qp"])
        assert n_aut == binding.host_query_symmetry(c["qp"])[0]
        for induced in (False, True):
            _, _, vr = binding.host_refine_sets_vertex_counts(c["g"], c["qp"], c["ld"], FULL, induced=induced)
            _, _, vd = binding.host_refine_sets_vertex_counts(c["g"], c["qp"], c["ld"], FULL, distinct=True, induced=induced)
            for orbit in orbits:
                lhs = vd[list(orbit)].sum(axis=0) * np.uint64(n_aut)
                for u0 in orbit:
                    assert np.array_equal(lhs, vr[u0] * np.uint64(len(orbit))), (c["gi"], c["name"], c["variant"], induced, orbit)
            telling += n_aut > 1 and vr.any() and not np.array_equal(vr, vd)
    assert telling * 4 >= 2 * 240, telling  # a quarter of the (case, plain / induced) pairs: symmetric, with matches, D != R


def test_host_guard(tmp_path_factory, tmp_path):
    """4. limit is a guard: limit == |M| gives complete == 0 and answers == limit, |M| + 1 the exact table and complete == 1, limit
    0 complete == 0, an empty C(u) zeros and complete == 1; unknown mode bits and a disconnected query are refused"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    for distinct, induced in MODES:
        count, full = tabs["triangle", "ld", distinct, induced]
        assert count == 28446 // (6 if distinct else 1)
        assert binding.host_refine_sets_vertex_counts(g, qp, bm, count, distinct=distinct, induced=induced)[:2] == (count, False)
        assert binding.host_refine_sets_vertex_counts(g, qp, bm, count - 1, distinct=distinct, induced=induced)[:2] == (count - 1, False)
        ans, complete, t = binding.host_refine_sets_vertex_counts(g, qp, bm, count + 1, distinct=distinct, induced=induced)
        assert (ans, complete) == (count, True) and np.array_equal(t, full)
        assert binding.host_refine_sets_vertex_counts(g, qp, bm, 0, distinct=distinct, induced=induced)[:2] == (0, False)
        empty = bm.copy()
        empty[1] = 0
        ans, complete, t = binding.host_refine_sets_vertex_counts(g, qp, empty, FULL, distinct=distinct, induced=induced)
        assert (ans, complete) == (0, True) and t.shape == (3, g["n"]) and not t.any()
    online, u32p, u64p = binding.load_online(), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)
    out, done, t = C.c_uint64(), C.c_int(), np.zeros((3, g["n"]), np.uint64)
    for mode in (4, 7, 1 << 31):
        assert online.gnnpe_host_refine_sets_vertex_counts(g["n"], o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), lb.ctypes.data_as(u32p),
                                                           qp.encode(), bmc.ctypes.data_as(u32p), FULL, mode, C.byref(out),
                                                           C.byref(done), t.ctypes.data_as(u64p)) != 0
        assert b"unknown mode" in binding.load().gnnpe_last_error()
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    for limit in (FULL, 0):
        with pytest.raises(binding.GnnpeError, match="not connected"):
            binding.host_refine_sets_vertex_counts(g, disc, sh._ones(2, g["n"]), limit)


def test_host_form_has_no_size_limit(tmp_path):
    """the 33-vertex path on the 40-cycle: 80 maps, every vertex 2 times at every position"""
    from gnnpe_amd import binding
    g = sh._cycle_graph(40)
    qp = sh._path_file(tmp_path, 33)
    ans, complete, t = binding.host_refine_sets_vertex_counts(g, qp, sh._ones(33, 40))
    assert (ans, complete) == (80, True) and t.shape == (33, 40) and (t == 2).all()


def test_cli_refusals(tmp_path):
    """10a. --vertex-counts without --refine sets, and together with --matches, exits 1 with its message before a GPU is touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    out = str(tmp_path / "vc.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    for extra, msg in ((["--vertex-counts", out], "--vertex-counts needs --refine sets"),
                       (["--refine", "start", "--vertex-counts", out], "--vertex-counts needs --refine sets"),
                       (["--refine", "sets", "--vertex-counts", out, "--matches", str(tmp_path / "m.txt")], "exclude each other")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout and not os.path.exists(out), extra


# ---- GPU: the device against the host form ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(7))
def test_gpu_every_first_level_shift(tmp_path_factory, monkeypatch, shift):
    """5. H1 with the first-level chunk forced to 1 << shift entries: the eight shapes on the three bitmaps in the four modes, the
    device table is the host form's, cell for cell.  H1 has rows longer than 64 (tallies survive chunk changes), hubs and at a
    small shift several items per start candidate (cell [qv[0]][v0] is added to by several waves), isolated vertices and
    n % 32 == 16.  Triangle and K4 on the label/degree bitmap (28 446 and 109 224 maps): the device table is also np.add.at over
    the rows Engine.refine_sets returns with room for all of them, which does not go through the host form"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g = h["g"]
    assert g["n"] % 32 == 16 and (h["deg"] > 64).sum() >= 10 and (h["deg"] == 0).sum() >= 10
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in sh.H1_SHAPES:
            for b in sh.BITMAPS:
                for distinct, induced in MODES:
                    want, table = tabs[name, b, distinct, induced]
                    got, complete, t, ms = eng.refine_sets_vertex_counts(h["q"][name], h["bm"][name][b], distinct=distinct, induced=induced)
                    where = (shift, name, b, distinct, induced)
                    assert (got, complete) == (want, True) and ms > 0, where + (got, want)
                    assert t.dtype == np.uint64 and np.array_equal(t, table), where + (int((t != table).sum()),)
        for name, count in (("triangle", 28446), ("K4", 109224)):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=count)
            assert got == count == len(rows)
            t = eng.refine_sets_vertex_counts(qp, bm)[2]
            assert np.array_equal(t, _table(rows, sh.SHAPES[name][0], g["n"])), (shift, name)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_star5_centre_column(tmp_path_factory):
    """2 (device). star5 on H1, label/degree bitmap, mode 0: 4 596 520 344 maps; the centre's column is d(d-1)(d-2)(d-3), and
    every leaf's column sums to the same total.  The largest cell is 155 * 154 * 153 * 152 < 2^32"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, d = h["g"], h["deg"].astype(np.uint64)
    qp = sh._shape_file(h["tmp"], "star5")
    centre = d * (d - 1) * (d - 2) * (d - 3) * (d >= 4)
    assert centre.sum() == 4596520344 and centre.max() < 1 << 32
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        got, complete, t, ms = eng.refine_sets_vertex_counts(qp, ex._ld_bitmap(g, qp))
        print(f"star5 on H1: {got} maps, {ms:.3f} ms")
        assert (got, complete) == (int(centre.sum()), True)
        assert np.array_equal(t[0], centre) and (t.sum(axis=1) == centre.sum()).all()
        A = sh._adjacency(g)
        leaf = np.asarray(A @ ((h["deg"] - 1) * (h["deg"] - 2) * (h["deg"] - 3) * (h["deg"] >= 4))).ravel().astype(np.uint64)
        assert all(np.array_equal(t[u], leaf) for u in range(1, 5))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_query_sizes_and_refusals(tmp_path_factory, tmp_path):
    """6. nq == 1 (the leaf add alone) and nq == 2 (the leaf feeds tally[0]) on H1 against the closed forms; the 32-vertex path on
    the 32-cycle (64 maps, none induced: the ends' images are adjacent) and on the 33-cycle (66 and 66), plain and induced, against
    the host form; 33 vertices and a context in multigraph state are refused and the context goes on answering"""
    from gnnpe_amd import binding, synth
    h = sh._h1(tmp_path_factory)
    g, d = h["g"], h["deg"].astype(np.uint64)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            got, complete, t, _ = eng.refine_sets_vertex_counts(h["q"]["vertex"], h["bm"]["vertex"][b])
            ids = sh._members(h["bm"]["vertex"][b][0], g["n"])
            assert (got, complete) == (len(ids), True) and t.shape == (1, g["n"]) and t.sum() == len(ids) and (t[0, ids] == 1).all(), b
        for b in ("ld", "ones"):
            got, complete, t, _ = eng.refine_sets_vertex_counts(h["q"]["edge"], h["bm"]["edge"][b])
            assert (got, complete) == (int(d.sum()), True) and np.array_equal(t[0], d) and np.array_equal(t[1], d), b
        p33 = sh._path_file(tmp_path, 33)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets_vertex_counts(p33, sh._ones(33, g["n"]))
        assert eng.refine_sets_vertex_counts(h["q"]["edge"], h["bm"]["edge"]["ld"])[0] == int(d.sum())
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.refine_sets_vertex_counts(h["q"]["edge"], h["bm"]["edge"]["ld"])
    finally:
        eng.close()
    p32 = sh._path_file(tmp_path, 32)
    for n, plain, ind in ((32, 64, 0), (33, 66, 66)):
        cyc = sh._cycle_graph(n)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            for bm in (ex._ld_bitmap(cyc, p32), sh._ones(32, n)):
                for induced, count in ((False, plain), (True, ind)):
                    for distinct in (False, True):
                        want = binding.host_refine_sets_vertex_counts(cyc, p32, bm, FULL, distinct=distinct, induced=induced)
                        assert want[0] == count // (2 if distinct else 1) and want[1]
                        got, complete, t, _ = eng.refine_sets_vertex_counts(p32, bm, distinct=distinct, induced=induced)
                        assert (got, complete) == want[:2] and np.array_equal(t, want[2]), (n, induced, distinct)
        finally:
            eng.close()


@pytest.mark.gpu
def test_gpu_device_table(tmp_path_factory):
    """7. device=True: the view's memory, copied back with Engine.copy_to_host, is the host-returned table; a second call with a
    smaller query reuses the buffer and returns a correct table -- no stale cell of the first shows -- and so does a call whose
    sets are empty (zeros, complete)"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    g, n = h["g"], h["g"]["n"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        def back(view):
            nq = view.shape[0]
            ptr = view.__cuda_array_interface__["data"][0]
            assert ptr and view.shape == (nq, n) and view.__cuda_array_interface__["typestr"] == "<i8"
            return ptr, eng.copy_to_host(ptr, nq * n * 8).view(np.uint64).reshape(nq, n)

        got, complete, view, ms = eng.refine_sets_vertex_counts(h["q"]["K5"], h["bm"]["K5"]["ones"], device=True)
        ptr5, t5 = back(view)
        assert (got, complete) == (tabs["K5", "ones", False, False][0], True) and np.array_equal(t5, tabs["K5", "ones", False, False][1])
        assert np.array_equal(t5, eng.refine_sets_vertex_counts(h["q"]["K5"], h["bm"]["K5"]["ones"])[2]) and t5.any()
        for name, b, distinct, induced in (("wedge", "thin", False, True), ("edge", "ld", True, False), ("vertex", "thin", False, False)):
            got, complete, view, _ = eng.refine_sets_vertex_counts(h["q"][name], h["bm"][name][b], distinct=distinct, induced=induced,
                                                                   device=True)
            ptr, t = back(view)
            assert ptr == ptr5, "the grow-only buffer was allocated again for a smaller table"
            assert (got, complete) == (tabs[name, b, distinct, induced][0], True) and np.array_equal(t, tabs[name, b, distinct, induced][1])
        empty = h["bm"]["triangle"]["ld"].copy()
        empty[2] = 0
        got, complete, view, _ = eng.refine_sets_vertex_counts(h["q"]["triangle"], empty, device=True)
        assert (got, complete) == (0, True) and not back(view)[1].any()
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_guard(tmp_path_factory):
    """8. K4 on H1 (109 224 maps, far past the 1 024-find flush) and its distinct form (4 551): limit |M| - 1 and |M| give
    complete == 0 and answers == limit, |M| + 1 gives complete == 1 and the exact table, limit 0 complete == 0; twice on one context"""
    from gnnpe_amd import binding
    h, tabs = sh._h1(tmp_path_factory), _h1_tables(tmp_path_factory)
    qp, bm = h["q"]["K4"], h["bm"]["K4"]["ld"]
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for distinct in (False, True):
            count, table = tabs["K4", "ld", distinct, False]
            assert count == 109224 // (24 if distinct else 1) > 1024
            for _ in range(2):
                for limit in (count - 1, count):
                    got, complete, _, _ = eng.refine_sets_vertex_counts(qp, bm, limit=limit, distinct=distinct)
                    assert (got, complete) == (limit, False), (distinct, limit, got, complete)
                got, complete, t, _ = eng.refine_sets_vertex_counts(qp, bm, limit=count + 1, distinct=distinct)
                assert (got, complete) == (count, True) and np.array_equal(t, table), distinct
                assert eng.refine_sets_vertex_counts(qp, bm, limit=0, distinct=distinct)[:2] == (0, False)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, monkeypatch, seed):
    """9. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of bitmap,
    a random first-level shift) in the four modes: the device table is the host form's"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    if c["shift"] is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for distinct, induced in MODES:
            want = binding.host_refine_sets_vertex_counts(g, c["qp"], c["bm"], FULL, distinct=distinct, induced=induced)
            assert want[1] and (distinct or induced or want[0] == c["count"])
            got, complete, t, _ = eng.refine_sets_vertex_counts(c["qp"], c["bm"], distinct=distinct, induced=induced)
            assert (got, complete) == want[:2] and np.array_equal(t, want[2]), (seed, c["which"], c["shift"], distinct, induced)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cli_vertex_counts(tmp_path, test_graph):
    """10. gnnpe_main -m online --exact --refine sets --vertex-counts on the golden test graph, q2 (52 exact answers): one line
    `v c_0 .. c_{nq-1}` per data vertex with a non-zero cell, ascending; every column sums to the printed answer and the cells are
    the binding's table (the exact filter's sets are complete, so it is the label/degree bitmap's table); also with --distinct and
    --induced.  With -n 52 the guard is reached: exit status non-zero, a message that names -n, no file"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    assert json.load(open(os.path.join(ONLINE, "exact_answers.json")))["q2"]["exact"] == 52
    qp = os.path.join(ONLINE, "q2.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets"]
    for k, (distinct, induced) in enumerate(MODES):
        want, complete, table = binding.host_refine_sets_vertex_counts(test_graph, qp, ld, FULL, distinct=distinct, induced=induced)
        assert complete and (distinct or induced or want == 52)
        out = str(tmp_path / f"vc{k}.txt")
        cmd = base + ["--vertex-counts", out] + (["--distinct"] if distinct else []) + (["--induced"] if induced else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        assert ans == want, (distinct, induced, ans, want)
        lines = np.loadtxt(out, dtype=np.uint64, ndmin=2) if want else np.zeros((0, table.shape[0] + 1), np.uint64)
        assert lines.shape[1] == table.shape[0] + 1 and (np.diff(lines[:, 0].astype(np.int64)) > 0).all()
        assert (lines[:, 1:].sum(axis=0) == ans).all() and (lines[:, 1:] != 0).any(axis=1).all()
        got = np.zeros((table.shape[0], n), np.uint64)
        got[:, lines[:, 0].astype(np.int64)] = lines[:, 1:].T
        assert np.array_equal(got, table), (distinct, induced)
    out = str(tmp_path / "guard.txt")
    r = subprocess.run(base + ["--vertex-counts", out, "-n", "52"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "-n" in r.stderr and not os.path.exists(out), (r.returncode, r.stderr)
    r = subprocess.run(base + ["--vertex-counts", out, "-n", "53"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Answer Number: 52 " in r.stdout and os.path.exists(out), r.stderr
    r = subprocess.run(base + ["--vertex-counts", out, "--matches", str(tmp_path / "m.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "exclude each other" in r.stderr
