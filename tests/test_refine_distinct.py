"""Every matching subgraph once (include/gnnpe_online.h, ABI version 11): gnnpe_host_query_symmetry, D(C, limit) on the host
(gnnpe_host_refine_sets_distinct), on the device in one shot (gnnpe_refine_sets_distinct) and page by page
(gnnpe_refine_pages_open_distinct), and `gnnpe_main --distinct`.

The yardstick is independent of the library.  For a row f, key(f) is the set of data edges {f(a), f(b)} the query edges land on
(for a single-vertex query the vertex itself).
  * closed bitmaps (label/degree, all ones): the keys of the returned rows are the keys of networkx's embeddings inside the sets,
    and there are as many rows as keys;
  * any bitmap (thinned, random bits): the rows are networkx's rows inside the sets that satisfy the ordering pairs.
The pairs themselves are pinned first (tests 1 and 2): the table of the shapes, networkx's automorphism count, and "of the maps
f o alpha exactly one satisfies every pair" for random injective f."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_pages as rp
import test_refine_sets as rs
import test_refine_sets_shapes as sh

sets_lines = sh.sets_lines  # the fixture that collects the `[refine_sets]` lines

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE

# |Aut| with every label 0 and with labels alternating 0, 1 by vertex id; the pairs of the smaller shapes
AUT = {"vertex": (1, 1), "edge": (2, 1), "wedge": (2, 2), "triangle": (6, 2), "C4": (8, 4), "diamond": (4, 1), "C5": (10, 2),
       "star5": (24, 4), "K4": (24, 4), "K5": (120, 12)}
PAIRS = {("vertex", 0): [], ("vertex", 1): [], ("edge", 0): [(0, 1)], ("edge", 1): [], ("wedge", 0): [(0, 2)], ("wedge", 1): [(0, 2)],
         ("triangle", 0): [(0, 1), (0, 2), (1, 2)], ("triangle", 1): [(0, 2)], ("C4", 0): [(0, 1), (0, 2), (0, 3), (1, 3)],
         ("C4", 1): [(0, 2), (1, 3)], ("diamond", 0): [(0, 3), (1, 2)], ("diamond", 1): [],
         ("C5", 0): [(0, 1), (0, 2), (0, 3), (0, 4), (1, 4)], ("C5", 1): [(0, 4)]}
NX_YARDSTICK_MAX = 50_000  # fuzz: networkx enumerates (some 20 us a row) where the plain count is at most this
FUZZ_MAX_COUNT = 2_000_000


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _labels(name, variant):
    n = sh.SHAPES[name][0]
    return None if variant == 0 else [i % 2 for i in range(n)]


def _query_edges(qp):
    from gnnpe_amd import binding
    q = binding.host_load_graph(qp)
    offs = q["offsets"].astype(np.int64)
    return q, [(a, int(b)) for a in range(q["n"]) for b in q["nbrs"][offs[a]:offs[a + 1]] if a < int(b)]


def _keys(rows, edges, n):
    """set of key(row): the sorted codes min * n + max of the data edges a row's query edges land on"""
    rows = np.asarray(rows, np.int64)
    if len(rows) == 0:
        return set()
    if not edges:
        return set(map(tuple, rows.tolist()))
    a, b = rows[:, [e[0] for e in edges]], rows[:, [e[1] for e in edges]]
    return set(map(tuple, np.sort(np.minimum(a, b) * n + np.maximum(a, b), axis=1).tolist()))


def _ordered(rows, pairs):
    """mask of the rows with row[a] < row[b] for every pair"""
    rows = np.asarray(rows, np.int64)
    ok = np.ones(len(rows), bool)
    for a, b in np.asarray(pairs, np.int64).reshape(-1, 2):
        ok &= rows[:, a] < rows[:, b]
    return ok


def _nx_automorphisms(qp):
    """networkx's label-preserving isomorphisms of the query onto itself, as lists alpha[u]"""
    import networkx as nx
    from networkx.algorithms import isomorphism as iso
    q, edges = _query_edges(qp)
    Q = nx.Graph()
    for u in range(q["n"]):
        Q.add_node(u, l=int(q["labels"][u]))
    Q.add_edges_from(edges)
    return [[m[u] for u in range(q["n"])]
            for m in iso.GraphMatcher(Q, Q, node_match=lambda a, b: a["l"] == b["l"]).isomorphisms_iter()]


def _petersen_file(tmp):
    import networkx as nx
    p = str(tmp / "petersen.graph")
    ex._write_query(p, 10, {tuple(sorted(e)) for e in nx.petersen_graph().edges()}, [0] * 10)
    return p


def _symmetry_cases(tmp):
    """(name, variant, query file) of every shape with both label variants, and Petersen"""
    out = [(name, v, sh._shape_file(tmp, name, _labels(name, v))) for name in sh.SHAPES for v in (0, 1)]
    return out + [("petersen", 0, _petersen_file(tmp))]


def _assert_yardstick(g, qp, bm, rows, emb, closed):
    """rows (the library's) against emb (networkx's embeddings in the whole graph)"""
    from gnnpe_amd import binding
    q, edges = _query_edges(qp)
    n = len(g["labels"])
    inside = emb[rs._in_sets(bm, emb)]
    rs._assert_rows_are_embeddings(g, qp, bm, rows)
    if closed:
        want = _keys(inside, edges, n)
        assert _keys(rows, edges, n) == want and len(rows) == len(want), (len(rows), len(want))
    else:
        pairs = binding.host_query_symmetry(qp)[1]
        assert sh._row_set(rows) == sh._row_set(inside[_ordered(inside, pairs)])


def _k4_keys(g):
    """the keys of the K4 embeddings of a one-label graph, from networkx's cliques: all pairs of every 4-clique"""
    import networkx as nx
    n = len(g["labels"])
    offs = g["offsets"].astype(np.int64)
    G = nx.Graph()
    G.add_edges_from((v, int(w)) for v in range(n) for w in g["nbrs"][offs[v]:offs[v + 1]] if v < int(w))
    out = set()
    for c in nx.enumerate_all_cliques(G):
        if len(c) > 4:
            break
        if len(c) == 4:
            c = sorted(c)
            out.add(tuple(sorted(c[i] * n + c[j] for i in range(4) for j in range(i + 1, 4))))
    return out


_H1D = {}


def _h1_distinct(tmp_path_factory):
    """sh._h1 with, per shape, |Aut|, the pairs and the host form's D on the three bitmaps (computed once)"""
    if _H1D:
        return _H1D
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    aut, pairs, d = {}, {}, {}
    for name in sh.H1_SHAPES:
        aut[name], pairs[name] = binding.host_query_symmetry(h["q"][name])
        for b in sh.BITMAPS:
            d[name, b] = binding.host_refine_sets(h["g"], h["q"][name], h["bm"][name][b], FULL, distinct=True)
    _H1D.update(h=h, aut=aut, pairs=pairs, d=d)
    return _H1D


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_symmetry_table(tmp_path):
    """1. |Aut| and the pairs of the ten shapes with one label and with alternating labels, and of Petersen (120, 13 pairs); |Aut|
    is networkx's count; an asymmetric 7-vertex tree has (1, []); K32 saturates at 2^64 - 1 with 496 pairs; too small a
    pairs_cap is refused with the needed number"""
    from gnnpe_amd import binding
    for name, v, qp in _symmetry_cases(tmp_path):
        aut, pairs = binding.host_query_symmetry(qp)
        assert pairs.dtype == np.uint32 and pairs.shape == (len(pairs), 2)
        assert aut == len(_nx_automorphisms(qp)), (name, v)
        if name == "petersen":
            assert aut == 120 and len(pairs) == 13
            continue
        assert aut == AUT[name][v], (name, v, aut)
        if (name, v) in PAIRS:
            assert list(map(tuple, pairs.tolist())) == PAIRS[name, v], (name, v, pairs)
        assert (pairs[:, 0] < pairs[:, 1]).all() and len(pairs) <= sh.SHAPES[name][0] * (sh.SHAPES[name][0] - 1) // 2
        # the orbit sizes multiply to |Aut|
        assert aut == int(np.prod([1 + int((pairs[:, 0] == u).sum()) for u in range(sh.SHAPES[name][0])]))
    tree = str(tmp_path / "tree7.graph")
    ex._write_query(tree, 7, {(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (2, 6)}, [0] * 7)
    aut, pairs = binding.host_query_symmetry(tree)
    assert aut == 1 == len(_nx_automorphisms(tree)) and len(pairs) == 0
    k32 = str(tmp_path / "k32.graph")
    ex._write_query(k32, 32, {(a, b) for a in range(32) for b in range(a + 1, 32)}, [0] * 32)
    aut, pairs = binding.host_query_symmetry(k32)
    assert aut == FULL and len(pairs) == 496
    assert sh._row_set(pairs) == {(a, b) for a in range(32) for b in range(a + 1, 32)}
    star = str(tmp_path / "star32.graph")
    ex._write_query(star, 32, {(0, b) for b in range(1, 32)}, [0] * 32)
    assert binding.host_query_symmetry(star)[0] == FULL  # 31! > 2^64
    tri = sh._shape_file(tmp_path, "triangle")
    with pytest.raises(binding.GnnpeError, match="3 pairs"):
        binding.host_query_symmetry(tri, pairs_cap=2)
    assert len(binding.host_query_symmetry(tri, pairs_cap=3)[1]) == 3


def test_exactly_one_representative(tmp_path):
    """2. every shape, both label variants, and Petersen: for 200 random injective maps f into range(100) exactly one alpha among
    networkx's automorphisms makes f o alpha satisfy every pair"""
    from gnnpe_amd import binding
    rng = np.random.default_rng(31)
    for name, v, qp in _symmetry_cases(tmp_path):
        _, pairs = binding.host_query_symmetry(qp)
        alphas = np.array(_nx_automorphisms(qp), np.int64)
        nq = alphas.shape[1]
        for _ in range(200):
            f = rng.choice(100, nq, replace=False)
            assert int(_ordered(f[alphas], pairs).sum()) == 1, (name, v, f)


def test_host_form_against_networkx(tmp_path_factory):
    """3. the (graph, shape, labels) cases of test_refine_sets_shapes with networkx's embeddings.  Label/degree and all-ones
    bitmaps: D is the number of keys, the embeddings inside the sets that satisfy the pairs are one per key, and D |Aut| is the
    host form's plain count.  Thinned bitmap: D is the number of embeddings inside the sets that satisfy the pairs.  At least half
    of the cases with embeddings have |Aut| >= 2 and at least four have |Aut| = 1."""
    from gnnpe_amd import binding
    sym, asym = 0, 0
    cases = sh._nx_cases(tmp_path_factory)
    for c in cases:
        g, qp, emb = c["g"], c["qp"], c["emb"]
        aut, pairs = binding.host_query_symmetry(qp)
        assert aut == AUT[c["name"]][c["variant"]]
        _, edges = _query_edges(qp)
        for b in ("ld", "ones", "thin"):
            inside = emb[rs._in_sets(c[b], emb)]
            rows = inside[_ordered(inside, pairs)]
            d = binding.host_refine_sets(g, qp, c[b], FULL, distinct=True)
            assert d == len(rows), (c["gi"], c["name"], c["variant"], b, d, len(rows))
            if b != "thin":
                keys = _keys(inside, edges, g["n"])
                assert _keys(rows, edges, g["n"]) == keys and len(rows) == len(keys), (c["gi"], c["name"], c["variant"], b)
                assert d * aut == binding.host_refine_sets(g, qp, c[b], FULL) == len(inside)
        if len(emb):
            sym += aut >= 2
            asym += aut == 1
    with_emb = sum(len(c["emb"]) > 0 for c in cases)
    assert sym * 2 >= with_emb and asym >= 4, (sym, asym, with_emb)


def test_h1_counts(tmp_path_factory):
    """4. H1, every shape: D(label/degree) |Aut| is the plain count (K4: 109 224 / 24 = 4 551), the all-ones bitmap gives the same
    D, the thinned one a smaller positive one"""
    hd = _h1_distinct(tmp_path_factory)
    want = hd["h"]["want"]
    for name in sh.H1_SHAPES:
        assert hd["aut"][name] == AUT[name][0]
        assert hd["d"][name, "ld"] * hd["aut"][name] == want[name, "ld"], name
        assert hd["d"][name, "ones"] == hd["d"][name, "ld"], name
        assert 0 < hd["d"][name, "thin"] < hd["d"][name, "ld"], name
    assert want["K4", "ld"] == 109224 and hd["d"]["K4", "ld"] == 4551


def test_limits_and_size(tmp_path_factory, tmp_path):
    """5. limit 0 gives 0, limit 2^64 - 1 the whole D, a limit below D itself; a 33-vertex path with palindromic labels (0, 1, 0,
    ..., 0) on the 40-cycle with alternating labels is counted by the host form: 20 starts, two directions, |Aut| = 2"""
    from gnnpe_amd import binding
    hd = _h1_distinct(tmp_path_factory)
    h = hd["h"]
    for name in ("triangle", "K4"):
        bm, d = h["bm"][name]["ld"], hd["d"][name, "ld"]
        assert binding.host_refine_sets(h["g"], h["q"][name], bm, 0, distinct=True) == 0
        assert binding.host_refine_sets(h["g"], h["q"][name], bm, FULL, distinct=True) == d
        assert binding.host_refine_sets(h["g"], h["q"][name], bm, d - 1, distinct=True) == d - 1
        assert binding.host_refine_sets(h["g"], h["q"][name], bm, d + 1, distinct=True) == d
    g = sh._cycle_graph(40, 2)
    qp = str(tmp_path / "path33.graph")
    ex._write_query(qp, 33, {(i, i + 1) for i in range(32)}, [i % 2 for i in range(33)])
    aut, pairs = binding.host_query_symmetry(qp)
    assert aut == 2 and pairs.tolist() == [[0, 32]]
    assert binding.host_refine_sets(g, qp, sh._ones(33, 40), FULL) == 40
    assert binding.host_refine_sets(g, qp, sh._ones(33, 40), FULL, distinct=True) == 20
    assert binding.host_refine_sets(g, qp, ex._ld_bitmap(g, qp), FULL, distinct=True) == 20


def test_cli_refuses_distinct_without_refine_sets(tmp_path):
    """6. --distinct without --refine sets exits 1 with its message before the graph is read or a GPU is touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    for extra in (["--distinct"], ["--refine", "start", "--distinct"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--distinct needs --refine sets" in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout and "Automorphisms" not in r.stdout, extra


# ---- fuzz cases (host side here, device side below) -------------------------------------------------------------------------

FUZZ_SEEDS = list(range(24))
_FUZZ = {}


def _fuzz_case(seed, tmp_path_factory):
    """the graph of sh._fuzz_case(seed) (sparse G(n,m), power-law with rows of 70-110 entries, dense little graph; 1-3 labels); a
    shape of sh.SHAPES (at most four vertices on the power-law graphs, as there), its labels all equal to one data label or
    alternating between the two smallest data labels by vertex id; one of the four kinds of bitmap; the host form's R and D; a
    limit out of (1, D // 2, D, 2^40); a forced shift 0..6 or none"""
    if seed in _FUZZ:
        return _FUZZ[seed]
    from gnnpe_amd import binding
    rng = np.random.default_rng(7000 + seed)
    g = sh._fuzz_case(seed, tmp_path_factory)["g"]
    n = g["n"]
    names = [k for k in sh.SHAPES if sh.SHAPES[k][0] <= (4 if seed % 4 in (1, 3) else 5)]
    name = names[int(rng.integers(0, len(names)))]
    nq = sh.SHAPES[name][0]
    present = np.unique(g["labels"])
    variant = int(rng.integers(0, 2))
    if variant == 0:
        labels = [int(rng.choice(present))] * nq
    else:
        labels = [int(present[i % 2 % len(present)]) for i in range(nq)]
    qp = str(tmp_path_factory.mktemp("dfuzz") / f"d{seed}.graph")
    ex._write_query(qp, nq, set(sh.SHAPES[name][1]), labels)
    ld = ex._ld_bitmap(g, qp)
    which = ("ld", "thin", "ones", "random")[int(rng.integers(0, 4))]
    bm = {"ld": lambda: ld, "thin": lambda: rs._subset(ld, n, 7100 + seed), "ones": lambda: sh._ones(nq, n),
          "random": lambda: rng.integers(0, 1 << 32, ld.shape, dtype=np.uint64).astype(np.uint32)}[which]()
    aut, pairs = binding.host_query_symmetry(qp)
    r = binding.host_refine_sets(g, qp, bm, FULL)
    d = binding.host_refine_sets(g, qp, bm, FULL, distinct=True)
    limit = (1, d // 2, d, 1 << 40)[int(rng.integers(0, 4))]
    shift = int(rng.integers(0, 8))
    c = dict(g=g, qp=qp, name=name, nq=nq, bm=bm, which=which, closed=which in ("ld", "ones"), aut=aut, pairs=pairs, r=r, d=d,
             limit=limit, shift=None if shift == 7 else shift)
    _FUZZ[seed] = c
    return c


def test_fuzz_cases_are_telling(tmp_path_factory):
    """7. the 24 fuzz cases before any device sees them: at least 12 with D > 0, at least 12 with |Aut| >= 2, every kind of bitmap
    drawn, every plain count at most 2 000 000; on the closed bitmaps D |Aut| = R, and at least four closed cases with
    embeddings are small enough for the networkx yardstick of the device test"""
    cases = [_fuzz_case(s, tmp_path_factory) for s in FUZZ_SEEDS]
    assert sum(c["d"] > 0 for c in cases) >= 12
    assert sum(c["aut"] >= 2 for c in cases) >= 12
    assert {c["which"] for c in cases} == {"ld", "thin", "ones", "random"}
    assert all(c["r"] <= FUZZ_MAX_COUNT for c in cases), [c["r"] for c in cases]
    for c in cases:
        assert c["d"] <= c["r"]
        if c["closed"]:
            assert c["d"] * c["aut"] == c["r"], (c["name"], c["which"])
    assert sum(c["closed"] and 0 < c["r"] <= NX_YARDSTICK_MAX for c in cases) >= 4


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_small_cut_queries(tmp_path_factory):
    """1a. the 12 G(60, m) cases of test_refine_sets (cut queries of 3-6 vertices, 3 labels): one-shot distinct with room for every
    row, label/degree bitmap (closed) and its thinned copy"""
    from gnnpe_amd import binding
    for t, c in enumerate(rs._small_cases(tmp_path_factory)):
        eng = ex._engine(binding, c["g"], c["sn"], 2)
        try:
            for b, closed in (("bm", True), ("sub", False)):
                want = binding.host_refine_sets(c["g"], c["qp"], c[b], FULL, distinct=True)
                got, _, rows = eng.refine_sets(c["qp"], c[b], limit=FULL, matches_cap=len(c["emb"]) + 5, distinct=True)
                assert got == want == len(rows), (t, b, got, want)
                _assert_yardstick(c["g"], c["qp"], c[b], rows, c["emb"], closed)
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_shapes_on_small_graphs(tmp_path_factory, gi):
    """1b. the eight shapes with both label variants on one of the 15 small graphs of test_refine_sets_shapes: one-shot distinct
    with room for every row, label/degree bitmap (closed) and thinned bitmap, against networkx"""
    from gnnpe_amd import binding, synth
    cases = [c for c in sh._nx_cases(tmp_path_factory) if c["gi"] == gi]
    assert len(cases) == 2 * len(sh.NX_SHAPES)
    g = cases[0]["g"]
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            for b in ("ld", "thin"):
                got, _, rows = eng.refine_sets(c["qp"], c[b], limit=FULL, matches_cap=len(c["emb"]) + 5, distinct=True)
                assert got == len(rows), (gi, c["name"], c["variant"], b)
                _assert_yardstick(g, c["qp"], c[b], rows, c["emb"], b == "ld")
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(7))
def test_gpu_every_first_level_shift_on_h1(tmp_path_factory, monkeypatch, sets_lines, shift):
    """2. H1 with the first-level chunk forced to 1 << shift entries: the eight shapes on the label/degree and the thinned bitmap
    count what the host form counts, the rows (at most 65 536) are valid, different and ordered, and the `[refine_sets]` line
    says `pairs=K`.  K4 on the label/degree bitmap: the 4 551 rows are one per 4-clique of networkx."""
    from gnnpe_amd import binding
    hd = _h1_distinct(tmp_path_factory)
    h = hd["h"]
    g = h["g"]
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        sets_lines()
        for name in sh.H1_SHAPES:
            for b in ("ld", "thin"):
                bm, want = h["bm"][name][b], hd["d"][name, b]
                got, _, rows = eng.refine_sets(h["q"][name], bm, limit=sh.H1_LIMIT, matches_cap=sh.H1_CAP, distinct=True)
                assert got == want, (shift, name, b, got, want)
                assert len(rows) == min(want, sh.H1_CAP)
                rs._assert_rows_are_embeddings(g, h["q"][name], bm, rows)
                assert _ordered(rows, hd["pairs"][name]).all(), (shift, name, b)
                (ln,) = sets_lines()
                assert ln["shift"] == shift and ln["forced"] == 1 and ln["pairs"] == len(hd["pairs"][name]), ln
        _, edges = _query_edges(h["q"]["K4"])
        got, _, rows = eng.refine_sets(h["q"]["K4"], h["bm"]["K4"]["ld"], limit=FULL, matches_cap=5000, distinct=True)
        assert got == 4551 == len(rows)
        assert _keys(rows, edges, g["n"]) == _k4_keys(g)
        # the plain entry point on the same context says nothing of pairs and counts embeddings
        sets_lines()
        assert eng.refine_sets(h["q"]["K4"], h["bm"]["K4"]["ld"], limit=FULL)[0] == 109224
        (ln,) = sets_lines()
        assert "pairs" not in ln
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 6])
def test_gpu_paged(tmp_path_factory, monkeypatch, shift):
    """3. the distinct cursor on H1: the thinned triangle in pages of 1, 63, 64 and 65 rows, K4 on the label/degree bitmap in pages
    of 100 and 4 096.  The pages hold the one-shot distinct row set, every page before the last is full, and after the first page
    of at most 100 rows some wave is suspended.  A plain and a distinct cursor interleaved on one context deliver their own sets."""
    from gnnpe_amd import binding
    hd = _h1_distinct(tmp_path_factory)
    h = hd["h"]
    g = h["g"]
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name, b, sizes in (("triangle", "thin", (1, 63, 64, 65)), ("K4", "ld", (100, 4096))):
            qp, bm, want = h["q"][name], h["bm"][name][b], hd["d"][name, b]
            got, _, once = eng.refine_sets(qp, bm, limit=FULL, matches_cap=want + 5, distinct=True)
            assert got == want == len(once)
            for page_rows in sizes:
                with eng.open_match_cursor(qp, bm, page_rows, distinct=True) as cur:
                    rows, n_pages, first = rp._drain(cur, page_rows)
                assert len(rows) == want and sh._row_set(rows) == sh._row_set(once), (shift, name, page_rows)
                assert -(-want // page_rows) <= n_pages <= -(-want // page_rows) + 1
                if page_rows <= 100:
                    assert first["suspended_waves"] >= 1 and first["pages"] == 1 and first["rows"] == page_rows, first
        # one plain and one distinct cursor, page about
        qp, bm = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
        cur = {False: eng.open_match_cursor(qp, bm, 3000), True: eng.open_match_cursor(qp, bm, 700, distinct=True)}
        got, done = {False: [], True: []}, {False: False, True: False}
        while not all(done.values()):
            for k in (False, True):
                if not done[k]:
                    rows, done[k] = cur[k].next()
                    got[k].append(rows)
        for k in (False, True):
            cur[k].close()
        plain, dist = np.concatenate(got[False]), np.concatenate(got[True])
        rp._assert_the_right_set(g, qp, bm, plain, h["want"]["triangle", "ld"])
        rp._assert_the_right_set(g, qp, bm, dist, hd["d"]["triangle", "ld"])
        _, edges = _query_edges(qp)
        assert _keys(dist, edges, g["n"]) == _keys(plain, edges, g["n"]) and len(dist) * 6 == len(plain)
        assert _ordered(dist, hd["pairs"]["triangle"]).all()
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_limit(tmp_path_factory):
    """4. K4 on H1's label/degree bitmap with limits D - 1, D, D + 1 and 1: the answer is min(limit, D), twice; the rows are
    valid, as many as the answer, and pairwise different in key"""
    from gnnpe_amd import binding
    hd = _h1_distinct(tmp_path_factory)
    h = hd["h"]
    g, qp, bm, d = h["g"], h["q"]["K4"], h["bm"]["K4"]["ld"], hd["d"]["K4", "ld"]
    _, edges = _query_edges(qp)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for limit in (d - 1, d, d + 1, 1):
            for _ in range(2):
                got, _, rows = eng.refine_sets(qp, bm, limit=limit, matches_cap=d + 5, distinct=True)
                assert got == min(limit, d) == len(rows), (limit, got, len(rows))
                rs._assert_rows_are_embeddings(g, qp, bm, rows)
                assert len(_keys(rows, edges, g["n"])) == len(rows) and _ordered(rows, hd["pairs"]["K4"]).all()
            assert eng.refine_sets(qp, bm, limit=limit, distinct=True)[0] == min(limit, d)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_sizes_1_2_and_32(tmp_path_factory, tmp_path):
    """5. a single-vertex query: D = R = 2 000 on H1; the one-label edge: D = entries / 2, every edge once with the smaller end
    first; the 32-vertex one-label path on the 40-cycle: R = 80, D = 40, one row per key; 33 vertices are refused"""
    from gnnpe_amd import binding, synth
    hd = _h1_distinct(tmp_path_factory)
    h = hd["h"]
    g = h["g"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        got, _, rows = eng.refine_sets(h["q"]["vertex"], h["bm"]["vertex"]["ld"], matches_cap=2100, distinct=True)
        assert got == 2000 == eng.refine_sets(h["q"]["vertex"], h["bm"]["vertex"]["ld"])[0]
        assert np.array_equal(np.sort(rows[:, 0]), np.arange(2000))
        entries = len(g["nbrs"])
        got, _, rows = eng.refine_sets(h["q"]["edge"], h["bm"]["edge"]["ld"], matches_cap=entries, distinct=True)
        assert got * 2 == entries and len(rows) == got and (rows[:, 0] < rows[:, 1]).all()
        rs._assert_rows_are_embeddings(g, h["q"]["edge"], h["bm"]["edge"]["ld"], rows)
    finally:
        eng.close()
    g = sh._cycle_graph(40)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        qp = sh._path_file(tmp_path, 32)
        emb = rs._nx_embeddings(g, qp)
        assert len(emb) == 80
        for bm in (ex._ld_bitmap(g, qp), sh._ones(32, 40)):
            assert eng.refine_sets(qp, bm, limit=FULL)[0] == 80
            got, _, rows = eng.refine_sets(qp, bm, limit=FULL, matches_cap=100, distinct=True)
            assert got == 40 == len(rows)
            _assert_yardstick(g, qp, bm, rows, emb, True)
            with eng.open_match_cursor(qp, bm, 7, distinct=True) as cur:
                paged, _, _ = rp._drain(cur, 7)
            assert sh._row_set(paged) == sh._row_set(rows)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets(sh._path_file(tmp_path, 33), sh._ones(33, 40), distinct=True)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.open_match_cursor(sh._path_file(tmp_path, 33), sh._ones(33, 40), 10, distinct=True)
        assert eng.refine_sets(qp, sh._ones(32, 40), distinct=True)[0] == 40  # the context still answers
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_a_query_without_symmetry(tmp_path_factory, tmp_path, sets_lines):
    """6. the diamond with labels 0, 1, 0, 1 (|Aut| = 1) on H1 with labels alternating by vertex id: distinct equals plain in count
    and row set, one-shot and paged, and the line says pairs=0"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = dict(h["g"], labels=(np.arange(h["g"]["n"]) % 2).astype(np.uint32))
    qp = sh._shape_file(tmp_path, "diamond", [0, 1, 0, 1])
    assert binding.host_query_symmetry(qp)[0] == 1
    bm = ex._ld_bitmap(g, qp)
    want = binding.host_refine_sets(g, qp, bm, FULL)
    assert 0 < want < 60000 and binding.host_refine_sets(g, qp, bm, FULL, distinct=True) == want
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        sets_lines()
        a, _, plain = eng.refine_sets(qp, bm, limit=FULL, matches_cap=want + 5)
        b, _, dist = eng.refine_sets(qp, bm, limit=FULL, matches_cap=want + 5, distinct=True)
        said = sets_lines()
        assert a == b == want and sh._row_set(plain) == sh._row_set(dist) and len(dist) == want
        assert "pairs" not in said[0] and said[1]["pairs"] == 0
        with eng.open_match_cursor(qp, bm, 1000, distinct=True) as cur:
            paged, _, _ = rp._drain(cur, 1000)
        assert sh._row_set(paged) == sh._row_set(plain) and len(paged) == want
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, monkeypatch, seed):
    """7. the 24 fuzz cases: device == host form's D under the limit and without, the rows are valid, ordered and different in
    key; on a closed bitmap whose plain count is at most 50 000 the rows are one per key of networkx's embeddings"""
    from gnnpe_amd import binding, synth
    c = _fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    if c["shift"] is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
    _, edges = _query_edges(c["qp"])
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        want = min(c["limit"], c["d"])
        assert binding.host_refine_sets(g, c["qp"], c["bm"], c["limit"], distinct=True) == want
        for _ in range(2):
            got, _, rows = eng.refine_sets(c["qp"], c["bm"], limit=c["limit"], matches_cap=want + 3, distinct=True)
            assert got == want == len(rows), (seed, c["name"], c["which"], c["shift"], got, want)
            rs._assert_rows_are_embeddings(g, c["qp"], c["bm"], rows)
            assert _ordered(rows, c["pairs"]).all() and len(_keys(rows, edges, g["n"])) == len(rows)
        got, _, rows = eng.refine_sets(c["qp"], c["bm"], limit=FULL, matches_cap=c["d"] + 3, distinct=True)
        assert got == c["d"] == len(rows), seed
        if c["closed"]:
            assert len(_keys(rows, edges, g["n"])) == len(rows) and got * c["aut"] == eng.refine_sets(c["qp"], c["bm"], limit=FULL)[0]
            if 0 < c["r"] <= NX_YARDSTICK_MAX:
                _assert_yardstick(g, c["qp"], c["bm"], rows, rs._nx_embeddings(g, c["qp"]), True)
        with eng.open_match_cursor(c["qp"], c["bm"], 257, distinct=True) as cur:
            paged, _, _ = rp._drain(cur, 257)
        assert sh._row_set(paged) == sh._row_set(rows), seed
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cli_distinct(tmp_path, test_graph):
    """8. gnnpe_main -m online --exact --refine sets --distinct --matches F --all-matches on the golden test graph: for q0-q4 the
    answer line times the `Automorphisms:` line is the golden exact count, and the file holds one valid ordered row per answer"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    rec = json.load(open(os.path.join(ONLINE, "exact_answers.json")))
    for name in rs.QUERIES:
        qp = os.path.join(ONLINE, f"{name}.graph")
        mf = str(tmp_path / f"{name}.txt")
        r = subprocess.run([CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--distinct",
                            "--matches", mf, "--all-matches"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        at = next(i for i, ln in enumerate(out) if ln.startswith("Answer Number: "))
        d = int(out[at].split()[2])
        assert out[at + 1].startswith("Automorphisms: ")
        aut = int(out[at + 1].split()[1])
        assert aut == binding.host_query_symmetry(qp)[0]
        assert d * aut == rec[name]["exact"], (name, d, aut)
        rows = np.loadtxt(mf, dtype=np.int64, ndmin=2) if d else np.zeros((0, 1), np.int64)
        assert len(rows) == d
        if d:
            _, edges = _query_edges(qp)
            rs._assert_rows_are_embeddings(test_graph, qp, ex._ld_bitmap(test_graph, qp), rows)
            assert len(_keys(rows, edges, len(test_graph["labels"]))) == d
