"""Set-restricted refinement (include/gnnpe_online.h, R(C, limit)) where tests/test_refine_sets.py does not reach: every
first-level chunk width (GNNPE_TESTING=sets_first_shift=K, and the heuristic's own shift 6 on a graph with hub rows), queries of
1, 2 and 32 vertices and the refusal at 33, cyclic and symmetric queries whose vertices share one label (only the injectivity test
and the back-edge test tell right from wrong), bitmaps that are not label/degree sets (all ones with the padding bits, random
bits), isolated start candidates, and limits around the 1024-find flush.

Yardsticks: numpy / scipy closed forms (vertex, edge, wedge, triangle), networkx's monomorphisms, and the host form
gnnpe_host_refine_sets, which tests 1-3 pin to the other two first."""
import sys

import numpy as np
import pytest

import test_online_exact as ex
import test_refine_sets as rs

FULL = (1 << 64) - 1
H1_LIMIT = 10 ** 7
H1_CAP = 1 << 16

# name -> (vertices, edges); "star5" is the star on five vertices (a centre and four leaves)
SHAPES = {
    "vertex": (1, ()),
    "edge": (2, ((0, 1),)),
    "wedge": (3, ((0, 1), (1, 2))),
    "triangle": (3, ((0, 1), (0, 2), (1, 2))),
    "C4": (4, ((0, 1), (1, 2), (2, 3), (0, 3))),
    "diamond": (4, ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3))),
    "K4": (4, tuple((a, b) for a in range(4) for b in range(a + 1, 4))),
    "K5": (5, tuple((a, b) for a in range(5) for b in range(a + 1, 5))),
    "C5": (5, ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4))),
    "star5": (5, ((0, 1), (0, 2), (0, 3), (0, 4))),
}
H1_SHAPES = ("vertex", "edge", "wedge", "triangle", "C4", "diamond", "K4", "K5")
CLOSED = ("vertex", "edge", "wedge", "triangle")
NX_SHAPES = ("triangle", "C4", "C5", "diamond", "K4", "star5", "edge", "vertex")
BITMAPS = ("ld", "thin", "ones")


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _shape_file(tmp, name, labels=None):
    n, edges = SHAPES[name]
    p = str(tmp / f"{name}_{'x' if labels is None else ''.join(map(str, labels))}.graph")
    ex._write_query(p, n, set(edges), [0] * n if labels is None else labels)
    return p


def _path_file(tmp, k, label=0):
    p = str(tmp / f"path{k}.graph")
    ex._write_query(p, k, {(i, i + 1) for i in range(k - 1)}, [label] * k)
    return p


def _ones(nq, n):
    """every bit set, the padding bits of the last word included"""
    return np.full((nq, (n + 31) // 32), 0xFFFFFFFF, np.uint32)


def _row_of(ids, n):
    row = np.zeros((n + 31) // 32, np.uint32)
    ids = np.asarray(ids, np.int64)
    np.bitwise_or.at(row, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return row


def _members(row, n):
    ids = np.arange(n)
    return ids[((row[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1) != 0]


def _common_subset(bm, n, seed, keep=rs.KEEP):
    """every C(u) cut with ONE seeded random subset S of the vertices (each kept with probability `keep`): (bitmap, mask of S)"""
    s = np.random.default_rng(seed).random(n) < keep
    return bm & _row_of(np.nonzero(s)[0], n)[None, :], s


def _cycle_graph(n, n_labels=1):
    from gnnpe_amd import synth
    a = np.arange(n, dtype=np.int64)
    offs, nbrs = synth._csr_from_edges(n, a, (a + 1) % n)
    return dict(n=n, offsets=offs, nbrs=nbrs, labels=(a % n_labels).astype(np.uint32))


def _adjacency(g, mask=None):
    import scipy.sparse as sp
    n = len(g["labels"])
    offs = g["offsets"].astype(np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs))
    dst = g["nbrs"].astype(np.int64)
    if mask is not None:
        keep = mask[src] & mask[dst]
        src, dst = src[keep], dst[keep]
    return sp.csr_matrix((np.ones(len(src), np.int64), (src, dst)), shape=(n, n))


def _closed_forms(g, mask=None):
    """embeddings of the four smallest shapes in a one-label graph, on the subgraph induced by `mask` (all vertices if None):
    vertices; adjacency entries; sum d(d-1) over the induced degrees; sum of (A^2 o A)"""
    A = _adjacency(g, mask)
    d = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    n_vertices = len(d) if mask is None else int(mask.sum())
    return {"vertex": n_vertices, "edge": int(A.nnz), "wedge": int((d * (d - 1)).sum()), "triangle": int((A @ A).multiply(A).sum())}


def _hom_count(g, qpath, bm):
    """the count with the injectivity test removed: label, degree, set and edge preserving maps, two query vertices may share
    an image (never two adjacent ones: the data graphs have no loops)"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qpath)
    n = len(g["labels"])
    offs, qoffs = g["offsets"].astype(np.int64), q["offsets"].astype(np.int64)
    deg, qd = np.diff(offs), np.diff(qoffs)
    rows = [set(int(x) for x in g["nbrs"][offs[v]:offs[v + 1]]) for v in range(n)]
    qn = [[int(x) for x in q["nbrs"][qoffs[u]:qoffs[u + 1]]] for u in range(q["n"])]
    fit = [[v for v in _members(bm[u], n) if g["labels"][v] == q["labels"][u] and deg[v] >= qd[u]] for u in range(q["n"])]
    img = [0] * q["n"]

    def rec(u):
        if u == q["n"]:
            return 1
        total = 0
        for v in fit[u]:
            if all(img[w] in rows[v] for w in qn[u] if w < u):
                img[u] = int(v)
                total += rec(u + 1)
        return total
    return rec(0)


def _row_set(rows):
    return set(map(tuple, np.asarray(rows).tolist()))


_H1 = {}


def _h1(tmp_path_factory):
    """H1 = powerlaw_graph(2000, 6000, exponent=2.1, max_degree=150, n_labels=4, seed=5) with every label 0: 11 386 adjacency
    entries, 23 rows longer than 64 (the longest 155), 210 isolated vertices, 16 padding bits in the last bitmap word.  With it
    the eight query files, per shape the three bitmaps -- label/degree, a 3/4 thinning drawn for every query vertex on its own
    (seed 700 + shape), all ones -- and the host form's count on each (limit 10^7), computed once for the module."""
    if _H1:
        return _H1
    from gnnpe_amd import binding, synth
    g0 = synth.powerlaw_graph(2000, 6000, exponent=2.1, max_degree=150, n_labels=4, seed=5)
    g = dict(n=g0["n"], offsets=g0["offsets"], nbrs=g0["nbrs"], labels=np.zeros(g0["n"], np.uint32))
    deg = np.diff(g["offsets"].astype(np.int64))
    assert g["n"] == 2000 and g["n"] % 32 == 16 and (deg > 64).sum() >= 10 and (deg == 0).sum() >= 10
    tmp = tmp_path_factory.mktemp("h1")
    q, bms, want = {}, {}, {}
    for k, name in enumerate(H1_SHAPES):
        q[name] = _shape_file(tmp, name)
        ld = ex._ld_bitmap(g, q[name])
        bms[name] = dict(ld=ld, thin=rs._subset(ld, g["n"], 700 + k), ones=_ones(SHAPES[name][0], g["n"]))
        for b in BITMAPS:
            want[name, b] = binding.host_refine_sets(g, q[name], bms[name][b], H1_LIMIT)
            assert want[name, b] < H1_LIMIT
    _H1.update(g=g, deg=deg, sn=synth.degree_order(g["offsets"]), q=q, bm=bms, want=want, closed=_closed_forms(g), tmp=tmp)
    return _H1


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_host_form_equals_the_closed_forms_on_h1(tmp_path_factory):
    """1. vertex, edge, wedge, triangle on H1 (one label).  Label/degree bitmap and all-ones bitmap (padding bits set): n, the
    adjacency entries, sum d(d-1), sum (A^2 o A).  Thinned bitmap: ONE random subset S of the vertices (kept with probability
    3/4, seed 77) cut into every query vertex's label/degree set; the yardstick is the same four formulas on the subgraph
    induced by S -- |S|, entries with both ends in S, sum over S of dS(dS-1) with dS the number of neighbours in S, (A_S^2 o A_S)
    -- which is the count under the full graph's degrees too: an image with the neighbours an embedding needs inside S has at
    least the query vertex's degree.  The other four shapes' counts agree between the label/degree and the all-ones bitmap."""
    from gnnpe_amd import binding
    h = _h1(tmp_path_factory)
    g = h["g"]
    assert h["closed"]["vertex"] == g["n"] and h["closed"]["edge"] == len(g["nbrs"])
    for name in CLOSED:
        assert h["want"][name, "ld"] == h["want"][name, "ones"] == h["closed"][name] > 0, name
        sub, s = _common_subset(h["bm"][name]["ld"], g["n"], 77)
        inside = _closed_forms(g, s)[name]
        assert 0 < inside < h["closed"][name]
        assert binding.host_refine_sets(g, h["q"][name], sub, H1_LIMIT) == inside, name
    for name in H1_SHAPES:
        assert h["want"][name, "ones"] == h["want"][name, "ld"] > h["want"][name, "thin"] > 0, name


_NX = {}


def _dense_graphs():
    from gnnpe_amd import synth
    return [synth.gnm_graph(n, n * (n - 1) // 3, n_labels=2, seed=n) for n in (12, 16, 20)]


def _nx_case(tmp, gi, g, name, variant):
    """one shape on one graph: query labels all 0 (variant 0) or alternating 0, 1 by vertex id (variant 1), networkx's
    embeddings, and the three bitmaps (thinning seed 800 + graph)"""
    qp = _shape_file(tmp, name, None if variant == 0 else [i % 2 for i in range(SHAPES[name][0])])
    ld = ex._ld_bitmap(g, qp)
    return dict(gi=gi, g=g, name=name, variant=variant, qp=qp, emb=rs._nx_embeddings(g, qp), ld=ld,
                thin=rs._subset(ld, g["n"], 800 + gi), ones=_ones(SHAPES[name][0], g["n"]))


def _nx_cases(tmp_path_factory):
    """(graph, shape, labels) cases of test 2 with networkx's embeddings: gnm_graph(n, n(n-1)//3, 2 labels, seed n) for n in
    12, 16, 20 and the 12 G(60, 90..160) graphs of test_refine_sets._small_cases; the eight shapes with every query label 0 and
    with labels alternating 0, 1 by vertex id"""
    if "cases" in _NX:
        return _NX["cases"]
    graphs = _dense_graphs() + [c["g"] for c in rs._small_cases(tmp_path_factory)]
    tmp = tmp_path_factory.mktemp("shapes")
    _NX["cases"] = [_nx_case(tmp, gi, g, name, v) for gi, g in enumerate(graphs) for name in NX_SHAPES for v in (0, 1)]
    return _NX["cases"]


def test_host_form_equals_networkx_on_cyclic_and_symmetric_queries(tmp_path_factory):
    """2. host form == networkx's monomorphisms inside the sets, on the label/degree, thinned and all-ones bitmaps; at least
    half of the (graph, shape) pairs have embeddings, and at least a third of the counts are below the count of the maps that
    need not be injective, so a search without the injectivity test would be caught"""
    from gnnpe_amd import binding
    cases = _nx_cases(tmp_path_factory)
    nonzero, below = set(), 0
    for c in cases:
        for b in BITMAPS:
            want = int(rs._in_sets(c[b], c["emb"]).sum())
            assert binding.host_refine_sets(c["g"], c["qp"], c[b]) == want, (c["gi"], c["name"], c["variant"], b)
        assert int(rs._in_sets(c["ones"], c["emb"]).sum()) == len(c["emb"])
        if len(c["emb"]):
            nonzero.add((c["gi"], c["name"]))
        below += len(c["emb"]) < _hom_count(c["g"], c["qp"], c["ld"])
    pairs = len({(c["gi"], c["name"]) for c in cases})
    assert pairs == 15 * len(NX_SHAPES) and len(nonzero) * 2 >= pairs, (len(nonzero), pairs)
    assert below * 3 >= len(cases), (below, len(cases))


def test_host_form_extremes(tmp_path):
    """3. paths of 32, 33 and 2 vertices on a 40-cycle with one label: 80 each (40 starts, two directions; the host form has no
    32-vertex limit); limit 0 gives 0 and limit 2^64 - 1 the count"""
    from gnnpe_amd import binding
    g = _cycle_graph(40)
    for k in (32, 33, 2):
        qp = _path_file(tmp_path, k)
        assert binding.host_refine_sets(g, qp, ex._ld_bitmap(g, qp)) == 80, k
        assert binding.host_refine_sets(g, qp, _ones(k, 40), FULL) == 80, k
        assert binding.host_refine_sets(g, qp, _ones(k, 40), 0) == 0, k
        assert binding.host_refine_sets(g, qp, _ones(k, 40), 79) == 79, k


# ---- fuzz cases (host side here, device side below) -------------------------------------------------------------------------

FUZZ_SEEDS = list(range(24))
_FUZZ = {}


def _fuzz_case(seed, tmp_path_factory):
    """graph, connected query of 1-6 vertices (random spanning tree + random extra edges, labels drawn from the data labels),
    bitmap, host count, limit, matches_cap and forced shift (None: the heuristic) of one seed"""
    if seed in _FUZZ:
        return _FUZZ[seed]
    from gnnpe_amd import binding, synth
    rng = np.random.default_rng(4000 + seed)
    kind = (0, 1, 2, 1)[seed % 4]  # sparse G(n,m), power-law, dense little graph, power-law
    n_labels = int(rng.integers(1, 4))
    if kind == 0:
        n = int(rng.integers(40, 400))
        g = synth.gnm_graph(n, int(rng.integers(n // 2, 3 * n)), n_labels=n_labels, seed=seed)
    elif kind == 1:
        n = int(rng.integers(400, 900))
        g = synth.powerlaw_graph(n, int(rng.integers(4 * n, 6 * n)), exponent=2.0, max_degree=int(rng.integers(70, 111)),
                                 n_labels=n_labels, seed=seed)
    else:
        n = int(rng.integers(5, 17))
        g = synth.gnm_graph(n, n * (n - 1) // 3, n_labels=n_labels, seed=seed)
    n = g["n"]
    nq = int(rng.integers(1, 7))
    if kind == 1:
        nq = min(nq, 4)  # (a 5-star on a row of 110 entries alone is 10^10 embeddings)
    edges = {(int(rng.integers(0, i)), i) for i in range(1, nq)}
    for _ in range(int(rng.integers(0, nq + 1)) if nq > 2 else 0):
        a, b = sorted(int(x) for x in rng.choice(nq, 2, replace=False))
        edges.add((a, b))
    qp = str(tmp_path_factory.mktemp("fuzz") / f"f{seed}.graph")
    ex._write_query(qp, nq, edges, rng.choice(g["labels"], nq))
    ld = ex._ld_bitmap(g, qp)
    which = ("ld", "thin", "ones", "random")[int(rng.integers(0, 4))]
    bm = {"ld": lambda: ld, "thin": lambda: rs._subset(ld, n, 4100 + seed), "ones": lambda: _ones(nq, n),
          "random": lambda: rng.integers(0, 1 << 32, ld.shape, dtype=np.uint64).astype(np.uint32)}[which]()
    count = binding.host_refine_sets(g, qp, bm, FULL)
    limit = (1, count // 2, count, 1 << 40)[int(rng.integers(0, 4))]
    cap = int(rng.integers(0, min(count, 1 << 16) + 6)) if rng.random() < 0.75 else 0
    shift = int(rng.integers(0, 8))
    deg = np.diff(g["offsets"].astype(np.int64))
    start, _ = rs._start_vertex(qp, bm)
    c = dict(g=g, qp=qp, nq=nq, bm=bm, which=which, count=count, limit=limit, cap=cap, shift=None if shift == 7 else shift,
             cyclic=len(edges) >= nq > 0, hub_start=bool((deg[_members(bm[start], n)] > 64).any()))
    _FUZZ[seed] = c
    return c


def test_fuzz_cases_are_telling(tmp_path_factory):
    """the 24 fuzz cases before any device sees them: at least 12 with embeddings, 8 with a cyclic query, 6 with a vertex of
    degree > 64 among the start candidates, every forced shift and the heuristic drawn, every kind of bitmap drawn"""
    cases = [_fuzz_case(s, tmp_path_factory) for s in FUZZ_SEEDS]
    assert sum(c["count"] > 0 for c in cases) >= 12
    assert sum(c["cyclic"] for c in cases) >= 8
    assert sum(c["hub_start"] for c in cases) >= 6
    assert {c["shift"] for c in cases} >= {0, 6, None} and {c["which"] for c in cases} == {"ld", "thin", "ones", "random"}
    assert {2, 3, 4, 5} <= {c["nq"] for c in cases}


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def sets_lines(monkeypatch, capfd):
    """contexts created while this fixture is active print one `[refine_sets]` line per call (GNNPE_DEBUG=1 is read when a
    context is created); the returned callable gives the lines since it was last called as dicts of integers"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [{k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])}
                for ln in err.splitlines() if ln.startswith("[refine_sets] ")]
    return take


def _py_first_level_shift(n_cand, entries, n, cus, hubs):
    """sets_first_level_shift of csrc/gnnpe_refine_sets.hip: 64-entry chunks unless the graph has hub rows and n_cand x mean
    degree gives fewer than eight items per resident wave (4 blocks of 4 waves per CU)"""
    if hubs == 0 or entries + n >= 1 << 32:
        return 6
    est = n_cand * max(1, entries // max(n, 1))
    target = 8 * max(cus, 1) * 4 * 4
    shift = 6
    while shift > 0 and (est >> shift) < target:
        shift -= 1
    return shift


_ROWS_AT_0 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(7))
def test_gpu_every_first_level_shift(tmp_path_factory, monkeypatch, sets_lines, shift):
    """4. H1 with the first-level chunk forced to 1 << shift entries: the eight shapes on the three bitmaps count what the host
    form (and the closed form) counts, return min(count, 65 536) valid different rows, and say `shift=K forced=1`.  Triangle
    and K4 on the label/degree bitmap, asked for all their rows (28 446 and 109 224; the cap is the count), give the row set
    of shift 0.  Every start set of a query with an edge holds a row longer than 64, the all-ones ones an isolated vertex."""
    from gnnpe_amd import binding
    h = _h1(tmp_path_factory)
    g, deg = h["g"], h["deg"]
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        sets_lines()
        for name in H1_SHAPES:
            for b in BITMAPS:
                bm, want = h["bm"][name][b], h["want"][name, b]
                if b != "thin" and name in CLOSED:
                    assert want == h["closed"][name]
                start = _members(bm[rs._start_vertex(h["q"][name], bm)[0]], g["n"])
                if name != "vertex":
                    assert (deg[start] > 64).any(), (name, b)
                if b == "ones":
                    assert (deg[start] == 0).any() and (deg[start] > 64).any(), name
                got, _, rows = eng.refine_sets(h["q"][name], bm, limit=H1_LIMIT, matches_cap=H1_CAP)
                assert got == want, (shift, name, b, got, want)
                assert len(rows) == min(want, H1_CAP), (shift, name, b)
                rs._assert_rows_are_embeddings(g, h["q"][name], bm, rows)
        said = sets_lines()
        assert len(said) == len(H1_SHAPES) * len(BITMAPS)
        assert all(ln["shift"] == shift and ln["forced"] == 1 and ln["hubs"] >= 10 for ln in said), said
        for name in ("triangle", "K4"):
            want = h["want"][name, "ld"]
            got, _, rows = eng.refine_sets(h["q"][name], h["bm"][name]["ld"], limit=H1_LIMIT, matches_cap=want)
            assert got == want == len(rows), (shift, name)
            rs._assert_rows_are_embeddings(g, h["q"][name], h["bm"][name]["ld"], rows)
            if name not in _ROWS_AT_0:
                if shift:
                    monkeypatch.setenv("GNNPE_TESTING", "sets_first_shift=0")
                    eng0 = ex._engine(binding, g, h["sn"], 2)
                    rows0 = eng0.refine_sets(h["q"][name], h["bm"][name]["ld"], limit=H1_LIMIT, matches_cap=want)[2]
                    eng0.close()
                    assert sets_lines()[-1]["shift"] == 0
                else:
                    rows0 = rows
                assert len(rows0) == want
                _ROWS_AT_0[name] = _row_set(rows0)
            assert _row_set(rows) == _ROWS_AT_0[name], (shift, name)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_heuristic_shift_6_with_hub_rows(tmp_path, sets_lines):
    """5. nothing forced: powerlaw_graph(300000, 1500000, exponent=2.1, max_degree=600, n_labels=1, seed=7) -- 3 000 000
    adjacency entries, 5 854 rows longer than 64, the longest 908 -- where start candidates x mean degree passes 2^21 and the
    heuristic keeps 64-entry chunks, so a start candidate has up to 15 items.  Edge and wedge, limit 2^62: the adjacency
    entries and sum d(d-1).  The shift the library reports is the Python restatement's on the line's own cands, hubs and cus."""
    from gnnpe_amd import binding, synth
    g = synth.powerlaw_graph(300000, 1500000, exponent=2.1, max_degree=600, n_labels=1, seed=7)
    n, entries = g["n"], len(g["nbrs"])
    deg = np.diff(g["offsets"].astype(np.int64))
    assert (deg > 64).sum() >= 100 and int((deg >= 1).sum()) * (entries // n) >= 1 << 21
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    sets_lines()
    # (shape, count, least degree of a start candidate: the wedge starts at its centre, the smaller set)
    for name, want, start_deg in (("edge", entries, 1), ("wedge", int((deg * (deg - 1)).sum()), 2)):
        qp = _shape_file(tmp_path, name)
        bm = ex._ld_bitmap(g, qp)
        got, ms = eng.refine_sets(qp, bm, limit=1 << 62)
        print(f"{name} on 300 000 vertices: {got} embeddings, {ms:.3f} ms")
        (ln,) = sets_lines()
        assert ln["forced"] == 0 and ln["hubs"] == int((deg > 64).sum()) and ln["cands"] == int((deg >= start_deg).sum())
        assert ln["shift"] == _py_first_level_shift(ln["cands"], entries, n, ln["cus"], ln["hubs"]), ln
        if name == "edge" and ln["cus"] <= 256:
            assert ln["shift"] == 6
        assert got == want, (name, got, want)
    eng.close()


@pytest.mark.gpu
def test_gpu_single_vertex_queries(tmp_path_factory):
    """6a. nq == 1 with 1, 63, 64, 65 and all 2 000 start candidates on H1, and 4 097 of the 4 200 vertices of
    gnm_graph(4200, 8000, one label) (H1 is too small for that one): the count, the matches are exactly the candidates, and
    with limit 10 and room for 100 rows: 10, and 10 different candidates"""
    from gnnpe_amd import binding, synth
    h = _h1(tmp_path_factory)
    big = synth.gnm_graph(4200, 8000, n_labels=1, seed=5)
    qp = h["q"]["vertex"]
    for g, sizes in ((h["g"], (1, 63, 64, 65, 2000)), (big, (4097,))):
        eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
        for k in sizes:
            ids = np.sort(np.random.default_rng(k).permutation(g["n"])[:k])
            bm = _row_of(ids, g["n"])[None, :]
            for _ in range(2):
                got, _, rows = eng.refine_sets(qp, bm, matches_cap=k + 3)
                assert got == k and np.array_equal(np.sort(rows[:, 0]), ids), k
            assert eng.refine_sets(qp, bm)[0] == k
            got, _, rows = eng.refine_sets(qp, bm, limit=10, matches_cap=100)
            assert got == min(k, 10) == len(rows) == len(np.unique(rows[:, 0])) and np.isin(rows[:, 0], ids).all(), k
        # a candidate of another label is not an embedding, whatever the bitmap says
        other = str(h["tmp"] / "vertex_label1.graph")
        ex._write_query(other, 1, set(), [1])
        assert eng.refine_sets(other, _ones(1, g["n"]))[0] == 0
        eng.close()


@pytest.mark.gpu
def test_gpu_two_and_thirtytwo_vertex_queries(tmp_path):
    """6b. nq == 2 (the first level is the leaf level) on the three dense two-label graphs of test 2, both label variants, with matches ==
    networkx's rows; the 32-vertex path on the 40-cycle: 80 and networkx's 80 rows; 33 vertices and a disconnected pair are
    refused"""
    from gnnpe_amd import binding, synth
    for c in (_nx_case(tmp_path, gi, g, "edge", v) for gi, g in enumerate(_dense_graphs()) for v in (0, 1)):
        eng = ex._engine(binding, c["g"], synth.degree_order(c["g"]["offsets"]), 2)
        for b in BITMAPS:
            emb = c["emb"][rs._in_sets(c[b], c["emb"])]
            got, _, rows = eng.refine_sets(c["qp"], c[b], matches_cap=len(emb) + 5)
            assert got == len(emb) == len(rows) and _row_set(rows) == _row_set(emb), (c["gi"], c["variant"], b)
        eng.close()
    g = _cycle_graph(40)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    qp = _path_file(tmp_path, 32)
    emb = rs._nx_embeddings(g, qp)
    assert len(emb) == 80
    for bm in (ex._ld_bitmap(g, qp), _ones(32, 40)):
        got, _, rows = eng.refine_sets(qp, bm, matches_cap=100)
        assert got == 80 == len(rows) and _row_set(rows) == _row_set(emb)
        rs._assert_rows_are_embeddings(g, qp, bm, rows)
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == 80 and eng.refine_sets(qp, bm, limit=79)[0] == 79
    with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
        eng.refine_sets(_path_file(tmp_path, 33), _ones(33, 40))
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    with pytest.raises(binding.GnnpeError, match="not connected"):
        eng.refine_sets(disc, _ones(2, 40))
    assert eng.refine_sets(qp, _ones(32, 40))[0] == 80  # the context still answers
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [None, 6])
def test_gpu_limits_around_the_flush_threshold(tmp_path_factory, monkeypatch, sets_lines, forced):
    """7. K4 on H1 (109 224 embeddings, every resident wave at work), the heuristic's shift and shift 6: every limit gives
    min(limit, count), twice on one context; limits up to 1025 with room for 4096 rows give exactly `limit` valid different
    rows"""
    from gnnpe_amd import binding
    h = _h1(tmp_path_factory)
    g, qp, bm, count = h["g"], h["q"]["K4"], h["bm"]["K4"]["ld"], h["want"]["K4", "ld"]
    assert count > 100000
    if forced is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={forced}")
    eng = ex._engine(binding, g, h["sn"], 2)
    sets_lines()
    for limit in (1, 63, 64, 65, 1023, 1024, 1025, count - 1, count, count + 1, FULL):
        for _ in range(2):
            assert eng.refine_sets(qp, bm, limit=limit)[0] == min(limit, count), (forced, limit)
        if limit <= 1025:
            got, _, rows = eng.refine_sets(qp, bm, limit=limit, matches_cap=4096)
            assert got == limit == len(rows), (forced, limit, got, len(rows))
            rs._assert_rows_are_embeddings(g, qp, bm, rows)
    said = sets_lines()
    assert said and all(ln["forced"] == (forced is not None) and (forced is None or ln["shift"] == forced) for ln in said)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, monkeypatch, seed):
    """8. a random graph (sparse G(n,m), power-law with rows of 70-110 entries, dense little graph; 1-3 labels), a random
    connected query of 1-6 vertices, one of four kinds of bitmap (label/degree, thinned, all ones, random bits), a random
    limit, matches_cap and first-level shift: device == host form, the rows are embeddings inside the bitmap"""
    from gnnpe_amd import binding, synth
    c = _fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    if c["shift"] is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    want = min(c["limit"], c["count"])
    assert binding.host_refine_sets(g, c["qp"], c["bm"], c["limit"]) == want
    for _ in range(2):
        if c["cap"]:
            got, _, rows = eng.refine_sets(c["qp"], c["bm"], limit=c["limit"], matches_cap=c["cap"])
            assert len(rows) == min(want, c["cap"]), (seed, len(rows))
            rs._assert_rows_are_embeddings(g, c["qp"], c["bm"], rows)
        else:
            got = eng.refine_sets(c["qp"], c["bm"], limit=c["limit"])[0]
        assert got == want, (seed, c["which"], c["shift"], got, want)
    assert eng.refine_sets(c["qp"], c["bm"], limit=FULL)[0] == c["count"], seed
    eng.close()
