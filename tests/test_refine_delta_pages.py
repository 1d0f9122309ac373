"""Paged cursors over the delta matches (include/gnnpe_online.h, "paged cursors over the delta matches";
csrc/gnnpe_refine_delta_pages.hip): gnnpe_refine_pages_open_delta, _open_delta_nonedges and _open_delta_vertices hand out the match
cursor of ABI 10 over Dset_m(C, F), Nset_m(C, F) and Sset_m(C, S).  Every page except the last is exactly full, and across the pages
-- which run through the launches of several anchors -- every map of the set comes out exactly once, up to the limit, whatever the
page size.

The yardstick is never the new kernels: the counts are the host forms' (gnnpe_host_refine_sets_delta, _delta_nonedges,
_delta_vertices) or closed forms, the rows are checked as the one-shot tests check them (valid maps of the mode inside the sets,
pairwise different, every row touching F or S) and against the listing of the one-shot device call where that is at most ROWS_MAX
rows, or against rows enumerated in the test."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_delta as dl
import test_refine_delta_nonedges as dn
import test_refine_delta_vertices as dv
import test_refine_distinct as rd
import test_refine_edge_counts as re_
import test_refine_induced as ri
import test_refine_pages as rp
import test_refine_pages_suspend as sp
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = dl.MODES  # (distinct, induced)
ROWS_MAX = dl.ROWS_MAX
FUZZ_PAGE_ROWS = rp.FUZZ_PAGE_ROWS
FUZZ_MAX_DELTA = 2_000_000
FUZZ_MAX_PAGES = 2_000  # a fuzz run draws its page size among those of FUZZ_PAGE_ROWS that need no more pages than this (or takes the largest)
SUFFIX = {"edges": "", "nonedges": "_nonedges", "vertices": "_vertices"}


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _drain(cur, page_rows):
    """every page of an open cursor: (all rows, number of next() calls up to `done`, info after the first page).  Checks on every
    run: every page before the last holds exactly page_rows rows; after `done` nothing is suspended, no item is left, the row count
    is the sum of the pages; a further next() gives 0 rows, `done`, and launches nothing (the page count stands)"""
    pages, first = [], None
    while True:
        rows, done = cur.next()
        if first is None:
            first = cur.info()
        assert rows.dtype == np.uint32 and rows.ndim == 2
        pages.append(rows)
        if done:
            break
        assert len(rows) == page_rows, (len(pages), len(rows), page_rows)
        assert len(pages) < 10 ** 6
    assert len(pages[-1]) <= page_rows
    end = cur.info()
    assert end["suspended_waves"] == 0 and end["items_left"] == 0, end
    assert end["rows"] == sum(len(p) for p in pages)
    again, done = cur.next()
    assert done and len(again) == 0 and cur.info()["pages"] == end["pages"]
    return np.concatenate(pages), len(pages), first


def _pages(eng, qp, bm, page_rows, kind, anchor, distinct=False, induced=False, limit=FULL):
    with eng.open_delta_cursor(qp, bm, page_rows, **{kind: anchor}, distinct=distinct, induced=induced, limit=limit) as cur:
        return _drain(cur, page_rows)


def _oneshot(eng, qp, bm, kind, anchor, distinct, induced, cap):
    """(answers, rows) of the one-shot device call of the anchor"""
    if kind == "edges":
        got, rows, _ = eng.refine_sets_delta(qp, bm, anchor, matches_cap=cap, distinct=distinct, induced=induced)
    elif kind == "nonedges":
        got, rows, _ = eng.refine_sets_delta_nonedges(qp, bm, anchor, matches_cap=cap, distinct=distinct)
    else:
        got, rows, _ = eng.refine_sets_delta_vertices(qp, bm, anchor, matches_cap=cap, distinct=distinct, induced=induced)
    return got, rows


def _host(binding, g, qp, bm, kind, anchor, distinct, induced):
    if kind == "edges":
        return binding.host_refine_sets_delta(g, qp, bm, anchor, FULL, distinct=distinct, induced=induced)
    if kind == "nonedges":
        return binding.host_refine_sets_delta_nonedges(g, qp, bm, anchor, FULL, distinct=distinct)
    return binding.host_refine_sets_delta_vertices(g, qp, bm, anchor, FULL, distinct=distinct, induced=induced)


def _assert_delta_rows(g, qp, bm, rows, kind, anchor, distinct, induced):
    """the row checks of the one-shot tests: valid maps of the mode inside the sets, pairwise different, every row touching F or S"""
    if len(rows) == 0:
        return
    induced = induced or kind == "nonedges"
    ri._assert_rows(g, qp, bm, rows, induced, re_._pairs(qp) if distinct else None)
    n = len(g["labels"])
    if kind == "edges":
        assert dl._touches(rows, dl._qedges(qp), anchor, n).all()
    elif kind == "nonedges":
        assert dn._hits(rows, ri._non_edges(qp), anchor, n).all()
    else:
        assert dv._hits(rows, anchor).all()


def _same_rows(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return a.shape == b.shape and (len(a) == 0 or np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]))


def _graph(n, edges):
    from gnnpe_amd import synth
    e = np.asarray(sorted(edges), np.int64).reshape(-1, 2)
    offs, nbrs = synth._csr_from_edges(n, e[:, 0], e[:, 1])
    return dict(n=n, offsets=offs, nbrs=nbrs, labels=np.zeros(n, np.uint32))


def _engine(g):
    from gnnpe_amd import binding, synth
    return ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)


def _brute(g, qp, distinct, induced):
    """every map of the query into a SMALL one-label graph in a mode, by trying every injective tuple: nothing of the library but
    the query's edge list and its symmetry pairs"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qp)
    nq, n = q["n"], g["n"]
    adj = dn._adjacent(g)
    qe = set(map(tuple, np.asarray(dl._qedges(qp)).tolist()))
    qe |= {(b, a) for a, b in qe}
    out = []
    for t in itertools.permutations(range(n), nq):
        ok = True
        for a in range(nq):
            for b in range(a + 1, nq):
                if (a, b) in qe:
                    ok = ok and adj[t[a], t[b]]
                elif induced:
                    ok = ok and not adj[t[a], t[b]]
        if ok:
            out.append(t)
    rows = np.asarray(out, np.uint32).reshape(-1, nq)
    return rows[rd._ordered(rows, re_._pairs(qp))] if distinct and len(rows) else rows


C_BOOK = 5


def _book():
    """the edge {0, 1} and C_BOOK common neighbours"""
    c = C_BOOK
    return _graph(2 + c, [(0, 1)] + [(0, i) for i in range(2, 2 + c)] + [(1, i) for i in range(2, 2 + c)])


def _k2c():
    """K_{2,c}: the centres 0 and 1 (not adjacent), C_BOOK leaves"""
    c = C_BOOK
    return _graph(2 + c, [(0, i) for i in range(2, 2 + c)] + [(1, i) for i in range(2, 2 + c)])


def _fuzz_anchors(c, seed):
    """the seeded F (one edge, five edges, all edges) and S of a fuzz case, and its seeded mode"""
    g = c["g"]
    E = dl._und_edges(g)
    rng = np.random.default_rng(8000 + seed)
    forms = []
    if len(E):
        forms += [("edges", "one", E[rng.choice(len(E), 1)]), ("edges", "five", E[rng.choice(len(E), min(5, len(E)), replace=False)]),
                  ("edges", "all", E)]
    S = np.sort(rng.choice(g["n"], max(1, g["n"] // 10), replace=False)).astype(np.int64)
    forms.append(("vertices", "S", S))
    distinct, induced = MODES[int(rng.integers(0, 4))]
    return forms, distinct, induced


_FUZZ_HOST = {}


def _fuzz_host(seed, tmp_path_factory):
    """per form of a fuzz case the host form's delta, computed once"""
    if seed not in _FUZZ_HOST:
        from gnnpe_amd import binding
        c = sh._fuzz_case(seed, tmp_path_factory)
        forms, distinct, induced = _fuzz_anchors(c, seed)
        _FUZZ_HOST[seed] = [(kind, name, anchor, _host(binding, c["g"], c["qp"], c["bm"], kind, anchor, distinct, induced))
                            for kind, name, anchor in forms], distinct, induced
    return _FUZZ_HOST[seed]


def _fuzz_fits(seed, tmp_path_factory):
    return all(want <= FUZZ_MAX_DELTA for _, _, _, want in _fuzz_host(seed, tmp_path_factory)[0])


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_cli_refuses_delta_pages_where_it_does_not_apply(tmp_path):
    """each refusal exits 1 with its message before the graph is read or a GPU is touched; the refusals that were there stay"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    mf, ef, tf = str(tmp_path / "m.txt"), str(tmp_path / "e.txt"), str(tmp_path / "t.txt")
    open(ef, "w").write("0 1\n")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact", "--refine", "sets"]
    for extra, msg in ((["--matches", mf, "--delta-pages", "50"], "--delta-pages needs --delta-edges FILE or --delta-nonedges FILE or --delta-vertices FILE"),
                       (["--delta-edges", ef, "--delta-pages", "50"], "--delta-pages needs --matches FILE"),
                       (["--delta-edges", ef, "--matches", mf, "--delta-pages", "0"], "--delta-pages must be an integer of at least 1"),
                       (["--delta-edges", ef, "--matches", mf, "--delta-pages", "x"], "--delta-pages must be an integer of at least 1"),
                       (["--delta-edges", ef, "--delta-vertex-counts", tf, "--delta-pages", "5"],
                        "--delta-pages needs --matches FILE"),
                       (["--delta-edges", ef, "--matches", mf, "--delta-edge-counts", tf, "--delta-pages", "5"],
                        "--delta-pages excludes --delta-vertex-counts and --delta-edge-counts"),
                       (["--delta-edges", ef, "--matches", mf, "--all-matches", "--delta-pages", "5"], "--delta-edges excludes --all-matches"),
                       (["--delta-edges", ef, "--matches", mf, "--delta-pages", "5", "--match-page", "5"], "--match-page needs --all-matches")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra
    assert not os.path.exists(mf) and not os.path.exists(tf)
    pge = os.path.join(os.path.dirname(CLI), "gnnpge_main")
    r = subprocess.run([pge] + base[1:] + ["--delta-edges", ef, "--matches", mf, "--delta-pages", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--delta-pages is an option of gnnpe_main" in r.stderr, r.stderr


def test_binding_wants_exactly_one_anchor():
    """Engine.open_delta_cursor and Engine.delta_pages refuse no anchor and two anchors before anything is called"""
    from gnnpe_amd import binding
    eng = binding.Engine.__new__(binding.Engine)  # no context: the refusal comes first
    bm = np.zeros((2, 1), np.uint32)
    for kw in ({}, dict(edges=[(0, 1)], vertices=[0]), dict(edges=[(0, 1)], nonedges=[(0, 2)]), dict(nonedges=[(0, 2)], vertices=[1]),
               dict(edges=[(0, 1)], nonedges=[(0, 2)], vertices=[1])):
        with pytest.raises(binding.GnnpeError, match="exactly one of edges, nonedges and vertices"):
            binding.Engine.open_delta_cursor(eng, "q.graph", bm, 10, **kw)
        with pytest.raises(binding.GnnpeError, match="exactly one of edges, nonedges and vertices"):
            next(binding.Engine.delta_pages(eng, "q.graph", bm, 10, **kw))
    for name in ("gnnpe_refine_pages_open_delta", "gnnpe_refine_pages_open_delta_nonedges", "gnnpe_refine_pages_open_delta_vertices"):
        assert name in binding.ONLINE_SIGNATURES


def test_fuzz_cases_fit_the_delta_pages_test(tmp_path_factory):
    """the 24 fuzz cases before any device sees them: for at least 20 every form (F = one edge, five edges, all edges; S) has a host
    form delta of at most 2 000 000, so the device test below runs on at least 20"""
    fits = [_fuzz_fits(s, tmp_path_factory) for s in sh.FUZZ_SEEDS]
    assert sum(fits) >= 20, fits


# ---- GPU ------------------------------------------------------------------------------------------------------------------

BOOK_PAGES = (1, 4, 7, 10, 11, 64)


@pytest.mark.gpu
def test_gpu_book_pages_cross_the_launches(tmp_path):
    """1. the deterministic suspend.  The book (edge {0, 1}, c = 5 common neighbours) with the triangle and F = {{0, 1}}: 6c maps in
    modes 0 and INDUCED, c in the distinct ones, a third of them per launch; S = {0} is the same set.  K_{2,c} with the induced wedge
    and F = the non-edge of the centres: 2c (c distinct) in one launch; with the induced C4 4c(c - 1) (c(c - 1)/2 distinct) in two
    launches.  Pages of 1, 4, 7, 10, 11 and 64 rows: the rows are the enumerated set exactly, every page before the last is full
    although it straddles two launches, and at 1 row a wave is suspended after the first page (its chunk held more than one
    survivor)"""
    c = C_BOOK
    book, k2c = _book(), _k2c()
    tri, wedge, c4 = sh._shape_file(tmp_path, "triangle"), sh._shape_file(tmp_path, "wedge"), sh._shape_file(tmp_path, "C4")
    closed = {("tri", False): 6 * c, ("tri", True): c, ("wedge", False): 2 * c, ("wedge", True): c,
              ("c4", False): 4 * c * (c - 1), ("c4", True): c * (c - 1) // 2}
    runs = [(book, tri, "edges", np.array([[0, 1]]), "tri", MODES), (book, tri, "vertices", np.array([0]), "tri", MODES),
            (k2c, wedge, "nonedges", np.array([[1, 0]]), "wedge", MODES[2:]), (k2c, c4, "nonedges", np.array([[0, 1]]), "c4", MODES[2:])]
    for g, qp, kind, anchor, key, modes in runs:
        nq = {"tri": 3, "wedge": 3, "c4": 4}[key]
        bm = sh._ones(nq, g["n"])
        eng = _engine(g)
        try:
            for distinct, induced in modes:
                ref = _brute(g, qp, distinct, induced or kind == "nonedges")
                if kind == "edges":
                    ref = ref[dl._touches(ref, dl._qedges(qp), anchor, g["n"])]
                elif kind == "vertices":
                    ref = ref[dv._hits(ref, anchor)]
                else:
                    ref = ref[dn._hits(ref, ri._non_edges(qp), anchor, g["n"])]
                assert len(ref) == closed[key, distinct], (key, kind, distinct, induced, len(ref))
                for page_rows in BOOK_PAGES:
                    rows, n_pages, first = _pages(eng, qp, bm, page_rows, kind, anchor, distinct, induced)
                    where = (key, kind, distinct, induced, page_rows)
                    assert _same_rows(rows, ref), where
                    assert -(-len(ref) // page_rows) <= n_pages <= -(-len(ref) // page_rows) + 1, where + (n_pages,)
                    if page_rows == 1:
                        assert first["suspended_waves"] >= 1 and first["rows"] == 1 and first["pages"] == 1, where + (first,)
        finally:
            eng.close()


H1_PAGES = (63, 64, 65, 1000)


def _h1_runs(eng, g, qp, bm, kind, anchor, distinct, induced, want, where, pages):
    got, listing = _oneshot(eng, qp, bm, kind, anchor, distinct, induced, min(want, ROWS_MAX) + 1)
    assert got == want, where + (got, want)
    for page_rows in pages + (want + 1,):
        rows, n_pages, _ = _pages(eng, qp, bm, page_rows, kind, anchor, distinct, induced)
        assert len(rows) == want, where + (page_rows, len(rows), want)
        if want <= ROWS_MAX:
            assert _same_rows(rows, listing), where + (page_rows,)
        else:
            _assert_delta_rows(g, qp, bm, rows, kind, anchor, distinct, induced)
        if page_rows == want + 1:
            assert n_pages == 1
    _assert_delta_rows(g, qp, bm, listing[:20000], kind, anchor, distinct, induced)  # (the listing itself, by the row checks)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dl.H1_DELTA_SHAPES)
def test_gpu_h1_edges(tmp_path_factory, name):
    """2a. H1 with the F of test_refine_delta._h1_delta, the three bitmaps, the four modes, pages of 63, 64, 65, 1 000 and Delta + 1
    rows (and of 1 row on the edge query): the host form's Delta, and the sorted rows of the one-shot call"""
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    eng = _engine(h["g"])
    try:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                pages = H1_PAGES + ((1,) if name == "edge" and b == "ld" else ())
                _h1_runs(eng, h["g"], h["q"][name], h["bm"][name][b], "edges", f["F"], distinct, induced, f["want"][name, b, distinct, induced],
                         (name, b, distinct, induced), pages)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", dn.H1_SHAPES)
def test_gpu_h1_nonedges(tmp_path_factory, name):
    """2b. H1 with the F of test_refine_delta_nonedges._h1_nonedges, the three bitmaps, the two induced modes, the same pages"""
    h, f = sh._h1(tmp_path_factory), dn._h1_nonedges(tmp_path_factory)
    eng = _engine(h["g"])
    try:
        for b in sh.BITMAPS:
            for distinct in (False, True):
                _h1_runs(eng, h["g"], h["q"][name], h["bm"][name][b], "nonedges", f["F"], distinct, True, f["want"][name, b, distinct],
                         (name, b, distinct), H1_PAGES)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [None, 0, 6])
def test_gpu_h1_vertices(tmp_path_factory, monkeypatch, shift):
    """2c. H1 with the S of test_refine_delta_vertices._h1_vertices (a hub of several first-level chunks among it), the shapes of the
    edge test and the single vertex, the three bitmaps, the four modes, the same pages; with the first-level chunk width of the
    heuristic and forced to 1 and to 64 entries"""
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    if shift is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = _engine(h["g"])
    try:
        for name in ("vertex",) + dl.H1_DELTA_SHAPES:
            for b in sh.BITMAPS:
                for distinct, induced in MODES if shift is None else MODES[::3]:
                    pages = H1_PAGES + ((1,) if name == "vertex" else ())
                    _h1_runs(eng, h["g"], h["q"][name], h["bm"][name][b], "vertices", f["S"], distinct, induced,
                             f["want"][name, b, distinct, induced], (name, b, distinct, induced, shift), pages)
    finally:
        eng.close()


_FUZZ_RAN = []


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_pages_equal_the_one_shot_call(tmp_path_factory, monkeypatch, seed):
    """3. the fuzz cases of test_refine_sets_shapes whose deltas are at most 2 000 000 (at least 20 of the 24: asserted with the last
    seed, and on the CPU), in a seeded mode, with F = one edge, five edges, all edges and a seeded S of a tenth of the vertices; the
    page size is drawn from 1, 3, 64, 257, 5 000 among those that need at most 2 000 pages.  The count is the host form's, the rows
    are the one-shot call's as sets (up to ROWS_MAX rows; the row checks beyond)"""
    c = sh._fuzz_case(seed, tmp_path_factory)
    fits = _fuzz_fits(seed, tmp_path_factory)
    if fits:
        forms, distinct, induced = _fuzz_host(seed, tmp_path_factory)
        g = c["g"]
        if c["shift"] is not None:
            monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
        eng = _engine(g)
        rng = np.random.default_rng(8100 + seed)
        try:
            for kind, name, anchor, want in forms:
                ok = [p for p in FUZZ_PAGE_ROWS if want <= p * FUZZ_MAX_PAGES] or [FUZZ_PAGE_ROWS[-1]]
                page_rows = int(rng.choice(ok))
                rows, n_pages, _ = _pages(eng, c["qp"], c["bm"], page_rows, kind, anchor, distinct, induced)
                print(f"seed {seed} {name} mode {distinct, induced}: {want} rows, pages of {page_rows}: {n_pages}")
                assert len(rows) == want, (seed, name, len(rows), want)
                if want <= ROWS_MAX:
                    got, listing = _oneshot(eng, c["qp"], c["bm"], kind, anchor, distinct, induced, want + 1)
                    assert got == want and _same_rows(rows, listing), (seed, name)
                else:
                    _assert_delta_rows(g, c["qp"], c["bm"], rows, kind, anchor, distinct, induced)
        finally:
            eng.close()
        _FUZZ_RAN.append(seed)
    if seed == sh.FUZZ_SEEDS[-1] and len(set(_FUZZ_RAN) | {seed}) > 1:  # (the whole parametrised test ran, not one seed of it)
        assert len(_FUZZ_RAN) >= 20, _FUZZ_RAN
    if not fits:
        pytest.skip("a delta of more than 2 000 000 rows")


@pytest.mark.gpu
def test_gpu_extremes(tmp_path_factory, tmp_path):
    """4. F = E(G) and S = V on H1's triangle: the union of the pages is the plain cursor's row set, |M| rows (the charging rule
    across launches).  A single-vertex query through the vertices form at pages of 1, 64 and 100 (and Delta = 0 through the edge
    form: done before the first page).  A two-vertex query through the edge form: the leaf is the item's own chunk.  The 32-vertex
    path on the 33-cycle through each form with a page of 3 rows: 31 launches of the edge form, 465 of the non-edge form, 32 of the
    vertices form"""
    from gnnpe_amd import binding
    h, f, fv = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    g = h["g"]
    eng = _engine(g)
    try:
        qp, bm, count = h["q"]["triangle"], h["bm"]["triangle"]["ld"], h["want"]["triangle", "ld"]
        with eng.open_match_cursor(qp, bm, 5000) as cur:
            plain, _, _ = rp._drain(cur, 5000)
        assert len(plain) == count == 28446
        for kind, anchor in (("edges", f["all"]), ("vertices", np.arange(g["n"]))):
            for page_rows in (1000, 4097):
                rows, _, _ = _pages(eng, qp, bm, page_rows, kind, anchor)
                assert _same_rows(rows, plain), (kind, page_rows)
        qv, bv = h["q"]["vertex"], h["bm"]["vertex"]["ld"]
        for S in (fv["S"], np.arange(g["n"])):
            want = binding.host_refine_sets_delta_vertices(g, qv, bv, S, FULL)
            assert want > 0
            for page_rows in (1, 64, 100):
                rows, n_pages, _ = _pages(eng, qv, bv, page_rows, "vertices", S)
                assert len(rows) == want and len(np.unique(rows)) == want and np.isin(rows[:, 0], S).all(), (len(S), page_rows)
                rs._assert_rows_are_embeddings(g, qv, bv, rows)
        with eng.open_delta_cursor(qv, bv, 10, edges=f["F"]) as cur:  # nothing to launch
            rows, done = cur.next()
            assert done and rows.shape == (0, 1) and cur.info()["pages"] == 0
        qe, be = h["q"]["edge"], h["bm"]["edge"]["ld"]
        for distinct in (False, True):
            want = f["want"]["edge", "ld", distinct, False]
            for page_rows in (1, 5, 64):
                rows, _, _ = _pages(eng, qe, be, page_rows, "edges", f["F"], distinct)
                assert len(rows) == want
                _assert_delta_rows(g, qe, be, rows, "edges", f["F"], distinct, False)
    finally:
        eng.close()
    cyc = sh._cycle_graph(33)
    p32 = sh._path_file(tmp_path, 32)
    E = dl._und_edges(cyc)
    non = dn._all_non_edges(cyc)
    bm = sh._ones(32, 33)
    eng = _engine(cyc)
    try:
        for kind, anchor, modes in (("edges", E[[0, 1, 16]], MODES), ("vertices", np.array([0, 7, 32]), MODES),
                                    ("nonedges", non[[0, 100, 300]], MODES[2:])):
            for distinct, induced in modes:
                want = _host(binding, cyc, p32, bm, kind, anchor, distinct, induced)
                assert want > 0
                rows, n_pages, _ = _pages(eng, p32, bm, 3, kind, anchor, distinct, induced)
                assert len(rows) == want, (kind, distinct, induced, len(rows), want)
                _assert_delta_rows(cyc, p32, bm, rows, kind, anchor, distinct, induced)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["a", "b", "c"])
def test_gpu_poll_suspends_under_an_anchored_order(tmp_path_factory, monkeypatch, family):
    """5. the combs and the hub wedge of test_refine_pages_suspend (subtrees of thousands of matchless steps: waves suspend by the
    poll, between matches) with F = E(G) and S = V, at the page sizes that file uses: the rows are its reference set.  No step counts
    are asserted: the anchored orders are not the plain cursor's"""
    c = {"a": sp._comb_leaf, "b": sp._comb_inner, "c": sp._hub_wedge}[family](tmp_path_factory)
    eng = sp._open_engine(c, monkeypatch, 6)
    E, V = dl._und_edges(c["g"]), np.arange(c["g"]["n"])
    try:
        for mode in (list(sp.MODES) if family == "c" else ["R"]):
            want = sp._reference(c, mode)
            for kind, anchor in (("edges", E), ("vertices", V)):
                for page_rows in (1, 5, 64, c["M"][mode] + 1):
                    rows, n_pages, first = _pages(eng, c["qp"], c["bm"], page_rows, kind, anchor, **sp.MODES[mode])
                    assert len(rows) == len(want) and sh._row_set(rows) == sh._row_set(want), (family, mode, kind, page_rows)
                    print(f"{family} {mode} {kind} pages of {page_rows}: {n_pages}, after the first {first}")
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_limits(tmp_path):
    """6. the book's 30 triangle maps, 10 per launch, pages of 4 rows: limit 3 (below one page), 15 (in the middle of the second
    launch), 20 (exactly at a launch boundary, and a multiple of the page), 30 and 31.  min(30, limit) valid rows, `done` with the page
    that meets the limit (no launch more), then 0 suspended waves and 0 items left (_drain).  The same through S = {0}"""
    book = _book()
    tri = sh._shape_file(tmp_path, "triangle")
    bm = sh._ones(3, book["n"])
    ref = _brute(book, tri, False, False)
    assert len(ref) == 30
    eng = _engine(book)
    try:
        for kind, anchor in (("edges", np.array([[0, 1]])), ("vertices", np.array([0]))):
            for limit in (0, 3, 15, 20, 30, 31, FULL):
                with eng.open_delta_cursor(tri, bm, 4, **{kind: anchor}, limit=limit) as cur:
                    rows, n_pages, _ = _drain(cur, 4)
                    want = min(30, limit)
                    assert len(rows) == want and sh._row_set(rows) <= sh._row_set(ref) and len(sh._row_set(rows)) == want, (kind, limit)
                    launches = cur.info()["pages"]
                    if limit <= 30:  # the page that meets the limit says `done` itself
                        assert launches == -(-want // 4) and n_pages == max(launches, 1), (kind, limit, launches, n_pages)
                    else:
                        assert launches in (8, 9), (kind, limit, launches)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cursors_are_independent(tmp_path_factory):
    """7. an edge cursor, a vertices cursor and a plain cursor on one context with their pages interleaved, and between two pages a
    one-shot refine_sets_delta and a refine_sets_delta_vertex_counts with another F: each cursor delivers its own set"""
    from gnnpe_amd import binding
    h, f, fv = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    g = h["g"]
    qd, bd = h["q"]["diamond"], h["bm"]["diamond"]["ld"]
    qt, bt = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    other = f["all"][::7]
    eng = _engine(g)
    try:
        want_other = binding.host_refine_sets_delta(g, qt, bt, other, FULL)
        vc_want = binding.host_refine_sets_delta_vertex_counts(g, qt, bt, other, FULL)
        ref_e = _oneshot(eng, qd, bd, "edges", f["F"], False, False, 10 ** 6)[1]
        ref_v = _oneshot(eng, qt, bt, "vertices", fv["S"], False, False, 10 ** 6)[1]
        assert len(ref_e) == f["want"]["diamond", "ld", False, False] and len(ref_v) == fv["want"]["triangle", "ld", False, False]
        page = {"e": 700, "v": 300, "p": 3000}
        cur = {"e": eng.open_delta_cursor(qd, bd, page["e"], edges=f["F"]), "v": eng.open_delta_cursor(qt, bt, page["v"], vertices=fv["S"]),
               "p": eng.open_match_cursor(qt, bt, page["p"])}
        got, done = {k: [] for k in cur}, {k: False for k in cur}
        step = 0
        while not all(done.values()):
            for k in cur:
                if not done[k]:
                    rows, done[k] = cur[k].next()
                    assert done[k] or len(rows) == page[k]
                    got[k].append(rows)
            if step < 4:
                assert eng.refine_sets_delta(qt, bt, other, matches_cap=50)[0] == want_other
                ans, complete, table = eng.refine_sets_delta_vertex_counts(qt, bt, other)[:3]
                assert ans == want_other and complete and np.array_equal(np.asarray(table), np.asarray(vc_want[2]))
            step += 1
        assert step >= 4
        assert _same_rows(np.concatenate(got["e"]), ref_e) and _same_rows(np.concatenate(got["v"]), ref_v)
        rp._assert_the_right_set(g, qt, bt, np.concatenate(got["p"]), h["want"]["triangle", "ld"])
        for k in cur:
            cur[k].close()
        pages = list(eng.delta_pages(qd, bd, 5000, edges=f["F"]))
        assert [len(p) for p in pages[:-1]] == [5000] * (len(pages) - 1) and not eng._cursors
        assert _same_rows(np.concatenate(pages), ref_e)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_a_graph_change_invalidates_the_cursor(tmp_path_factory):
    """8. after apply_edges, and after set_vertex_labels: next() on an open delta cursor raises and launches nothing (the page count
    stands), close works, and a cursor opened afterwards delivers the delta of the new graph.  The insertion identity on a 20-edge
    batch (the batch of test_refine_delta.test_gpu_insertion_identity): |M(G')| = |M(G)| + |rows| against the host form"""
    from gnnpe_amd import binding
    h, fv = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    g1, deg = h["g"], h["deg"]
    e = dl._und_edges(g1)
    hubs = e[(deg[e[:, 0]] > 64) & (deg[e[:, 1]] > 64)]
    rng = np.random.default_rng(2500)
    F = np.concatenate([hubs[rng.choice(len(hubs), 5, replace=False)], e[rng.choice(len(e), 15, replace=False)]])
    assert len(dl._codes(F, g1["n"])) == 20
    g0 = dl._without(g1, F)
    eng = _engine(g0)
    try:
        for name in ("triangle", "diamond"):
            qp = h["q"][name]
            bm = dl._label_bitmap(g1, qp)
            eng.load_csr(g0["offsets"], g0["nbrs"], g0["labels"])
            old_F = dl._und_edges(g0)[::50]
            cur = eng.open_delta_cursor(qp, bm, 10, edges=old_F)
            rows, done = cur.next()
            assert len(rows) == 10 and not done
            eng.apply_edges(insert=F)
            with pytest.raises(binding.GnnpeError, match="after the cursor was opened"):
                cur.next()
            assert cur.info()["pages"] == 1
            cur.close()
            rows, _, _ = _pages(eng, qp, bm, 777, "edges", F)
            new, old = binding.host_refine_sets(g1, qp, bm, FULL), binding.host_refine_sets(g0, qp, bm, FULL)
            assert new == old + len(rows) and len(rows) == binding.host_refine_sets_delta(g1, qp, bm, F, FULL) > 0, (name, new, old, len(rows))
            _assert_delta_rows(g1, qp, bm, rows, "edges", F, False, False)
        # a relabel: H1 (all labels 0) with label 1 on S; the matches of the all-0 triangle through T = the first 40 vertices
        eng.load_csr(g1["offsets"], g1["nbrs"], g1["labels"])
        qp, bm = h["q"]["triangle"], sh._ones(3, g1["n"])
        S, T = fv["S"], np.arange(40)
        cur = eng.open_delta_cursor(qp, bm, 10, vertices=T)
        rows, done = cur.next()
        assert len(rows) == 10 and not done
        eng.set_vertex_labels(S, np.ones(len(S), np.uint32))
        with pytest.raises(binding.GnnpeError, match="after the cursor was opened"):
            cur.next()
        assert cur.info()["pages"] == 1
        cur.close()
        labels = g1["labels"].copy()
        labels[S] = 1
        g2 = dict(n=g1["n"], offsets=g1["offsets"], nbrs=g1["nbrs"], labels=labels)
        want = binding.host_refine_sets_delta_vertices(g2, qp, bm, T, FULL)
        assert 0 < want < binding.host_refine_sets_delta_vertices(g1, qp, bm, T, FULL)
        rows, _, _ = _pages(eng, qp, bm, 100, "vertices", T)
        assert len(rows) == want
        _assert_delta_rows(g2, qp, bm, rows, "vertices", T, False, False)
    finally:
        eng.close()


def _raw_open(binding, eng, kind, qp, bm, ids, limit=FULL, page_rows=10, mode=0):
    """gnnpe_refine_pages_open_delta* through ctypes: (return code, *cursor, message); *cursor is set to a canary first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    a = np.ascontiguousarray(np.asarray(ids, np.int64).reshape((-1,) if kind == "vertices" else (-1, 2)), np.uint32)
    h = C.c_void_p(0xdead0)
    rc = getattr(binding.load_online(), "gnnpe_refine_pages_open_delta" + SUFFIX[kind])(
        eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), a.ctypes.data_as(u32p), len(a), limit, page_rows, mode, C.byref(h))
    msg = binding.load().gnnpe_last_error().decode() if rc else ""
    if rc == 0:
        binding.load_online().gnnpe_refine_pages_close(h)
    return rc, h.value, msg


def _tail(msg):
    """an error message without the name of the function that raised it"""
    return msg.split(": ", 1)[1]


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory):
    """9. a pair that is not an edge (edge form), a pair that is an edge (non-edge form), an id >= n, a loop, page_rows 0, a mode
    without INDUCED for the non-edge form, unknown mode bits: GNNPE_ERR_ARG, *cursor NULL, the message of the one-shot call of the
    same anchor (after the function's name), and the context answers the next one-shot call correctly"""
    from gnnpe_amd import binding
    h, f, fn, fv = (sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory), dn._h1_nonedges(tmp_path_factory),
                    dv._h1_vertices(tmp_path_factory))
    g = h["g"]
    n = g["n"]
    qt, bt = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    qc, bc = h["q"]["C4"], h["bm"]["C4"]["ld"]
    edge = tuple(f["all"][100].tolist())
    non_edge = tuple(fn["F"][0].tolist())
    eng = _engine(g)
    online, lib = binding.load_online(), binding.load()

    def one_shot_message(kind, q, b, ids, mode):
        rc, _ = {"edges": dl._raw_device, "nonedges": dn._raw_device, "vertices": dv._raw_device}[kind](binding, eng, q, b, ids, mode=mode)
        assert rc == -1
        return _tail(lib.gnnpe_last_error().decode())

    try:
        cases = [("edges", qt, bt, f["F"].tolist() + [non_edge], 0, 10, "not an edge"),
                 ("edges", qt, bt, f["F"].tolist() + [non_edge[::-1]], 3, 10, "not an edge"),
                 ("nonedges", qc, bc, fn["F"].tolist() + [edge], 2, 10, "is an edge"),
                 ("nonedges", qc, bc, [edge[::-1]] + fn["F"].tolist(), 3, 10, "is an edge"),
                 ("edges", qt, bt, f["F"].tolist() + [(3, n)], 0, 10, "does not have"),
                 ("nonedges", qc, bc, fn["F"].tolist() + [(n + 5, 2)], 2, 10, "does not have"),
                 ("vertices", qt, bt, fv["S"].tolist() + [n], 0, 10, "does not have"),
                 ("edges", qt, bt, f["F"].tolist() + [(7, 7)], 0, 10, "loop"),
                 ("nonedges", qc, bc, fn["F"].tolist() + [(7, 7)], 2, 10, "loop"),
                 ("nonedges", qc, bc, fn["F"], 0, 10, "GNNPE_MATCH_INDUCED"),
                 ("nonedges", qc, bc, fn["F"], 1, 10, "GNNPE_MATCH_INDUCED"),
                 ("edges", qt, bt, f["F"], 4, 10, "unknown mode"),
                 ("nonedges", qc, bc, fn["F"], 6, 10, "unknown mode"),
                 ("vertices", qt, bt, fv["S"], 1 << 31, 10, "unknown mode")]
        for kind, q, b, ids, mode, page_rows, text in cases:
            rc, cursor, msg = _raw_open(binding, eng, kind, q, b, ids, page_rows=page_rows, mode=mode)
            assert rc == -1 and cursor is None and text in msg, (kind, mode, text, rc, cursor, msg)
            assert _tail(msg) == one_shot_message(kind, q, b, ids, mode), (kind, mode, msg)
        for kind, q, b, ids, mode in (("edges", qt, bt, f["F"], 0), ("nonedges", qc, bc, fn["F"], 2), ("vertices", qt, bt, fv["S"], 0)):
            rc, cursor, msg = _raw_open(binding, eng, kind, q, b, ids, page_rows=0, mode=mode)
            assert rc == -1 and cursor is None and "page_rows must be at least 1" in msg, (kind, rc, cursor, msg)
            with pytest.raises(binding.GnnpeError, match="page_rows must be at least 1"):
                eng.open_delta_cursor(q, b, 0, **{kind: ids})
        assert not eng._cursors
        # the context stays usable: the one-shot calls and a cursor answer
        assert dl._raw_device(binding, eng, qt, bt, f["F"]) == (0, f["want"]["triangle", "ld", False, False])
        assert dn._raw_device(binding, eng, qc, bc, fn["F"]) == (0, fn["want"]["C4", "ld", False])
        assert dv._raw_device(binding, eng, qt, bt, fv["S"]) == (0, fv["want"]["triangle", "ld", False, False])
        rows, _, _ = _pages(eng, qt, bt, 100, "edges", f["F"])
        assert len(rows) == f["want"]["triangle", "ld", False, False]
        # nothing to launch: the pairs are not looked up, open succeeds, the cursor is done before its first page
        for kind, q, b, ids, kw in (("edges", qt, bt, [non_edge], dict(limit=0)), ("edges", qt, bt, np.zeros((0, 2), np.int64), {}),
                                    ("vertices", qt, bt, np.zeros(0, np.int64), {}), ("nonedges", qt, bt, [edge], {}),
                                    ("edges", h["q"]["vertex"], h["bm"]["vertex"]["ld"], [non_edge], {})):
            with eng.open_delta_cursor(q, b, 5, **{kind: ids}, **kw) as cur:
                rows, done = cur.next()
                info = cur.info()
                assert done and len(rows) == 0 and info["pages"] == 0 and info["suspended_waves"] == 0 and info["items_left"] == 0, (kind, info)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_device_pages(tmp_path_factory):
    """10. the device page, read through torch.as_tensor, equals the host copy of the same page: every page of one cursor is taken
    both ways (next() copies it to the host, device_ptr names the page it came from).  Then device=True, where no host buffer is
    passed: the pages' union is the same set, also through the generator"""
    import torch
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["diamond"], h["bm"]["diamond"]["ld"]
    want = f["want"]["diamond", "ld", False, False]
    eng = _engine(g)
    try:
        both = []
        with eng.open_delta_cursor(qp, bm, 4096, edges=f["F"]) as cur:
            done = False
            while not done:
                rows, done = cur.next()
                ptr = C.c_void_p()
                eng._ck(cur.lib.gnnpe_refine_pages_device_ptr(cur.h, C.byref(ptr), None))
                if len(rows):
                    view = binding._DevArray(int(ptr.value), rows.shape, "<i4", owner=cur)
                    t = torch.as_tensor(view, device="cuda:0")
                    assert t.is_cuda and t.dtype == torch.int32 and t.data_ptr() == ptr.value
                    assert np.array_equal(t.cpu().numpy().astype(np.uint32), rows), len(both)
                    del t
                both.append(rows)
        host_rows = np.concatenate(both)
        assert len(host_rows) == want
        _assert_delta_rows(g, qp, bm, host_rows, "edges", f["F"], False, False)
        pages = []
        with eng.open_delta_cursor(qp, bm, 4096, edges=f["F"], device=True) as cur:
            done = False
            while not done:
                view, done = cur.next()
                assert done or view.shape == (4096, 4)
                if view.shape[0]:
                    t = torch.as_tensor(view, device="cuda:0")
                    assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == view.shape
                    assert t.data_ptr() == view.__cuda_array_interface__["data"][0]
                    pages.append(t.cpu().numpy().astype(np.uint32))  # (copied off the page before the next next())
                    del t
        assert _same_rows(np.concatenate(pages), host_rows)
        pages = [torch.as_tensor(p, device="cuda:0").cpu().numpy() for p in eng.delta_pages(qp, bm, 10000, edges=f["F"], device=True)]
        assert _same_rows(np.concatenate(pages).astype(np.uint32), host_rows)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edges", "vertices", "nonedges"])
@pytest.mark.parametrize("q", ["q1", "q2"])
def test_gpu_cli_delta_pages(tmp_path, test_graph, q, kind):
    """11. gnnpe_main --delta-pages 50 on the golden Test graph with q1 and q2: with --delta-edges, --delta-vertices and
    --delta-nonedges --induced the file holds as many pairwise different valid rows that touch F or S as the one-shot path's
    `Answer Number` at an unbounded limit, and the answer line is the one-shot path's (the edge form with --distinct as well)"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    rng = np.random.default_rng(8700)
    E, non = dl._und_edges(test_graph), dn._all_non_edges(test_graph)
    src, _ = re_._csr_keys(test_graph)
    used_e = np.nonzero(binding.host_refine_sets_edge_counts(test_graph, qp, ld)[2].sum(axis=0))[0]
    used_e = used_e[rng.choice(len(used_e), 6, replace=False)]
    F = np.concatenate([E[rng.choice(len(E), 20, replace=False)], np.stack([src[used_e], test_graph["nbrs"][used_e].astype(np.int64)], axis=1)])
    used_v = np.nonzero(binding.host_refine_sets_vertex_counts(test_graph, qp, ld)[2].sum(axis=0))[0]
    S = np.unique(np.concatenate([rng.choice(n, 12, replace=False), used_v[rng.choice(len(used_v), 3, replace=False)]]))
    V = binding.host_refine_sets_vertex_counts(test_graph, qp, ld, induced=True)[2]
    a = dn._adjacent(test_graph)
    qnon = ri._non_edges(qp)
    live = [(int(x), int(y)) for u, w in qnon[:1] for x in np.nonzero(V[u])[0][:6] for y in np.nonzero(V[w])[0][:6] if x != y and not a[x, y]]
    N = np.concatenate([np.array(live, np.int64).reshape(-1, 2), non[rng.choice(len(non), 40, replace=False)]])
    files = {}
    for name, arr in (("edges", F), ("nonedges", N)):
        files[name] = str(tmp_path / f"{name}.txt")
        open(files[name], "w").write("".join(f"{x} {y}\n" for x, y in arr.tolist()))
    files["vertices"] = str(tmp_path / "vertices.txt")
    open(files["vertices"], "w").write("".join(f"{v}\n" for v in S.tolist()))
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets"]
    answer = lambda out: int(next(ln for ln in out.splitlines() if ln.startswith("Answer Number: ")).split()[2])
    for anchor, flags in {"edges": ((F, []), (F, ["--distinct"])), "vertices": ((S, []),), "nonedges": ((N, ["--induced"]),)}[kind]:
        distinct, induced = "--distinct" in flags, "--induced" in flags
        cmd = base + [f"--delta-{kind}", files[kind]] + flags
        one = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert one.returncode == 0, one.stderr
        want = answer(one.stdout)
        assert want == _host(binding, test_graph, qp, ld, kind, anchor, distinct, induced)
        out = str(tmp_path / f"{kind}{len(flags)}{distinct}.txt")
        r = subprocess.run(cmd + ["--matches", out, "--delta-pages", "50"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert answer(r.stdout) == want, (kind, flags)
        rows = np.loadtxt(out, dtype=np.int64, ndmin=2) if want else np.zeros((0, 1), np.int64)
        assert len(rows) == want and len(np.unique(rows, axis=0)) == want, (kind, flags, len(rows), want)
        if want:
            _assert_delta_rows(test_graph, qp, ld, rows, kind, anchor, distinct, induced)
        print(f"{q} {kind} {flags}: {want} rows")
