"""The induced matches that put a non-adjacent query pair on one of a given set of data vertex pairs, each once
(include/gnnpe_online.h, ABI version 18): N_m(C, F, limit) for the two INDUCED modes, F a set of NON-edges of the graph -- the induced
matches an insertion of F destroys, and the ones a deletion of F has created -- on the host (gnnpe_host_refine_sets_delta_nonedges),
on the device (gnnpe_refine_sets_delta_nonedges) and through `gnnpe_main --delta-nonedges`.

The host form walks all of M and drops the finds that miss F.  It is held to yardsticks that are not the library: networkx's induced
rows filtered in numpy, and the insertion and deletion identities with gnnpe_host_refine_sets_mode and gnnpe_host_refine_sets_delta
supplying the other terms.  The device form starts at the pairs of F instead, once per non-adjacent query pair, and charges every
match to its lowest-numbered non-adjacent pair in F; it is held to the host form, to the rows gnnpe_refine_sets_mode lists (filtered
in numpy), to F = all non-edges, where N = |M| and a match charged twice shows, and to the identities between the graph before and
after gnnpe_csr_apply_edges.  The yardstick is never the new kernel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_delta as rdl
import test_refine_distinct as rd
import test_refine_edge_counts as re_
import test_refine_induced as ri
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
H1_SHAPES = ("wedge", "C4", "diamond")
ROWS_MAX = 500_000  # the device's full listing is compared row for row where it is at most this long


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _adjacent(g):
    n = len(g["labels"])
    a = np.zeros((n, n), bool)
    src, _ = re_._csr_keys(g)
    a[src, g["nbrs"].astype(np.int64)] = True
    return a


def _all_non_edges(g):
    """every pair x < y that is not an edge, ascending: an (m, 2) int64 array"""
    a = _adjacent(g)
    x, y = np.nonzero(np.triu(~a, 1))
    return np.stack([x, y], axis=1).astype(np.int64)


def _hits(rows, qnon, F, n):
    """mask of the rows that put at least one of the non-adjacent query pairs on a pair of F"""
    return rdl._touches(rows, qnon, F, n)


def _nx_rows(c, b, distinct):
    """networkx's induced rows of a small case inside the sets of bitmap b, ordered for DISTINCT"""
    rows = c["ind"][rs._in_sets(c[b], c["ind"])]
    return rows[rd._ordered(rows, re_._pairs(c["qp"]))] if distinct else rows


def _small_sets(g, seed):
    """three of the four forms of F on a small graph: five random non-edges, two non-edges with a common vertex, all non-edges"""
    non = _all_non_edges(g)
    rng = np.random.default_rng(seed)
    v = next(int(v) for v in rng.permutation(len(g["labels"])) if ((non == v).any(axis=1)).sum() >= 2)
    two = non[(non == v).any(axis=1)][:2]
    share = np.array([two[0], two[1][::-1]], np.int64)  # (either orientation)
    assert len(non) >= 5
    return dict(five=non[rng.choice(len(non), 5, replace=False)], share=share, all=non)


def _hit_set(rows, qnon):
    """the form `hit`: the image of the first non-adjacent query pair of the first row, where there is a row and a pair"""
    if len(rows) == 0 or not qnon:
        return None
    return np.array([[rows[0][qnon[0][0]], rows[0][qnon[0][1]]]], np.int64)


_H1N = {}


def _h1_nonedges(tmp_path_factory):
    """H1 with the F of the device tests, each part asserted to exist: a non-adjacent pair between two rows longer than 64 (a depth-2
    pivot row of several chunks, the ordered trim), a pair with an endpoint of degree 1, a pair with an isolated vertex, two pairs
    that share a vertex, the two ends of a wedge (a hit is certain), a pair with vertex n - 1 (the padding bits of the last bitmap
    word), 50 random non-edges (seed 3100).  With it the host form's N of H1_SHAPES on the three bitmaps in the two induced modes,
    computed once"""
    if _H1N:
        return _H1N
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, deg, n = h["g"], h["deg"], h["g"]["n"]
    a = _adjacent(g)
    o = g["offsets"].astype(np.int64)
    hubs = np.nonzero(deg > 64)[0]
    hub = next(((int(x), int(y)) for x in hubs for y in hubs if x < y and not a[x, y]), None)
    assert hub is not None, "no non-adjacent pair of rows longer than 64"
    leaf = int(np.nonzero(deg == 1)[0][0])
    pend = (leaf, next(int(y) for y in np.nonzero(deg > 1)[0] if not a[leaf, y]))
    iso = (int(np.nonzero(deg == 0)[0][0]), int(hubs[0]))
    w = int(np.nonzero((deg >= 2) & (deg <= 64))[0][0])
    far = [int(y) for y in np.nonzero(deg > 0)[0] if y != w and not a[w, y]][:2]
    share = [(w, far[0]), (far[1], w)]
    mid = next(int(y) for y in np.nonzero(deg >= 2)[0] if not a[g["nbrs"][o[y]], g["nbrs"][o[y] + 1]])
    ends = (int(g["nbrs"][o[mid]]), int(g["nbrs"][o[mid] + 1]))
    last = (next(int(y) for y in np.nonzero(deg > 1)[0] if not a[n - 1, y] and y != n - 1), n - 1)
    non = _all_non_edges(g)
    rnd = non[np.random.default_rng(3100).choice(len(non), 50, replace=False)]
    F = np.array([hub, pend, iso] + share + [ends, last] + rnd.tolist(), np.int64)
    assert not a[F[:, 0], F[:, 1]].any() and len(rdl._codes(F, n)) >= 55
    want = {}
    for name in H1_SHAPES:
        for b in sh.BITMAPS:
            for distinct in (False, True):
                want[name, b, distinct] = binding.host_refine_sets_delta_nonedges(g, h["q"][name], h["bm"][name][b], F, FULL,
                                                                                  distinct=distinct)
    _H1N.update(F=F, want=want, adjacent=a, non=non, hub=hub)
    return _H1N


def _raw_host(binding, g, qp, bm, pairs, mode, limit=FULL, null=None):
    """gnnpe_host_refine_sets_delta_nonedges through ctypes: (return code, *answers); *answers is set to a canary first"""
    u32p = C.POINTER(C.c_uint32)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)
    e = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.uint32)
    out = C.c_uint64(12345)
    args = dict(offsets=o.ctypes.data_as(u32p), nbrs=nb.ctypes.data_as(u32p), labels=lb.ctypes.data_as(u32p), query=qp.encode(),
                bitmap=bmc.ctypes.data_as(u32p), pairs=e.ctypes.data_as(u32p), answers=C.byref(out))
    if null:
        args[null] = None
    rc = binding.load_online().gnnpe_host_refine_sets_delta_nonedges(g["n"], args["offsets"], args["nbrs"], args["labels"], args["query"],
                                                                     args["bitmap"], args["pairs"], len(e), limit, mode, args["answers"])
    return rc, out.value


def _raw_device(binding, eng, qp, bm, pairs, limit=FULL, mode=2):
    """gnnpe_refine_sets_delta_nonedges through ctypes: (return code, *answers); *answers is set to a canary first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    e = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.uint32)
    out, ms = C.c_uint64(12345), C.c_double()
    rc = binding.load_online().gnnpe_refine_sets_delta_nonedges(eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), e.ctypes.data_as(u32p),
                                                                len(e), limit, mode, C.byref(out), None, 0, C.byref(ms))
    return rc, out.value


# ---- CPU: the host form against yardsticks that are not the library ----------------------------------------------------------

def test_host_form_against_networkx(tmp_path_factory):
    """1. the 15 small graphs, the eight shapes of ri.IND_SHAPES, both label variants, the label/degree and the thinned bitmap, modes
    INDUCED and INDUCED | DISTINCT, four forms of F: the host form is the number of networkx's induced rows (inside the sets,
    filtered by the ordering pairs for DISTINCT) with some non-adjacent (row[a], row[b]) in F.  `hit` is the image of the first
    non-adjacent pair of the first such row, so N >= 1 exactly where there is a match; `all` is every non-edge of the graph, where N
    is the induced count; a shape without a non-adjacent pair gives 0"""
    from gnnpe_amd import binding
    cases = ri._ind_cases(tmp_path_factory)
    assert len(cases) == 15 * len(ri.IND_SHAPES) * 2
    some = part = total = 0
    for c in cases:
        g, n = c["g"], c["g"]["n"]
        qnon = ri._non_edges(c["qp"])
        assert len(qnon) == ri.NON_EDGES[c["name"]]
        sets = _small_sets(g, 3000 + c["gi"])
        for b in ("ld", "thin"):
            for distinct in (False, True):
                rows = _nx_rows(c, b, distinct)
                assert len(rows) == binding.host_refine_sets(g, c["qp"], c[b], FULL, distinct=distinct, induced=True)
                forms = dict(sets)
                hit = _hit_set(rows, qnon)
                if hit is not None:
                    forms["hit"] = hit
                for form, F in forms.items():
                    want = int(_hits(rows, qnon, F, n).sum())
                    got = binding.host_refine_sets_delta_nonedges(g, c["qp"], c[b], F, FULL, distinct=distinct)
                    where = (c["gi"], c["name"], c["variant"], b, distinct, form, got, want)
                    assert got == want, where
                    assert form != "hit" or got >= 1, where
                    assert form != "all" or got == (len(rows) if qnon else 0), where
                    assert qnon or got == 0, where
                    total += 1
                    some += want > 0
                    part += 0 < want < len(rows)
    assert some * 5 >= total and part * 20 >= total, (some, part, total)


def _identity_runs(tmp_path_factory):
    """(graph, query file, seed) of the identity tests: the small cases of the shapes with a non-adjacent pair, and H1 with the wedge
    and the diamond"""
    h = sh._h1(tmp_path_factory)
    runs = [(c["g"], c["qp"], 3200 + c["gi"]) for c in ri._ind_cases(tmp_path_factory) if c["name"] in ri.NONEDGE_SHAPES]
    return runs + [(h["g"], h["q"][name], 3300) for name in ("wedge", "diamond")]


def test_host_insertion_and_deletion_identities(tmp_path_factory):
    """2. both induced modes, labels-only bitmaps.  G' = G + F, F a random quarter of G''s edges: |M(G')| = |M(G)| - N(G, F) +
    Delta(G', F) -- which read from G' to G is the deletion identity |M(G)| = |M(G')| - Delta(G', F) + N(G, F) -- with
    gnnpe_host_refine_sets_mode and gnnpe_host_refine_sets_delta supplying the other terms.  N is positive in at least 40 of the 304
    (run, mode): the sparse two-label graphs lose few matches to an insertion"""
    from gnnpe_amd import binding
    runs = _identity_runs(tmp_path_factory)
    lost = 0
    for g1, qp, seed in runs:
        e = rdl._und_edges(g1)
        F = e[np.random.default_rng(seed).choice(len(e), max(1, len(e) // 4), replace=False)]
        g0 = rdl._without(g1, F)
        bm = rdl._label_bitmap(g1, qp)
        for distinct in (False, True):
            new = binding.host_refine_sets(g1, qp, bm, FULL, distinct=distinct, induced=True)
            old = binding.host_refine_sets(g0, qp, bm, FULL, distinct=distinct, induced=True)
            gone = binding.host_refine_sets_delta_nonedges(g0, qp, bm, F, FULL, distinct=distinct)
            came = binding.host_refine_sets_delta(g1, qp, bm, F, FULL, distinct=distinct, induced=True)
            assert new == old - gone + came, (qp, distinct, new, old, gone, came)
            lost += gone > 0
    assert lost >= 40, lost


def test_host_mixed_batch_in_two_steps(tmp_path_factory):
    """2'. a mixed batch by the recipe of the header: delete D (Delta before, N after), then insert I (N before, Delta after), against
    the count on the graph gnnpe_host_csr_apply_edges builds in one go.  D a random tenth of the edges, I as many random non-edges"""
    from gnnpe_amd import binding
    for g0, qp, seed in _identity_runs(tmp_path_factory)[::3]:
        rng = np.random.default_rng(seed + 50)
        e, non = rdl._und_edges(g0), _all_non_edges(g0)
        D = e[rng.choice(len(e), max(1, len(e) // 10), replace=False)]
        I = non[rng.choice(len(non), len(D), replace=False)]
        g1 = binding.host_apply_edges(g0, delete=D)
        g2 = binding.host_apply_edges(g1, insert=I)
        both = binding.host_apply_edges(g0, insert=I, delete=D)
        assert np.array_equal(both["nbrs"], g2["nbrs"])
        bm = rdl._label_bitmap(g0, qp)
        for distinct in (False, True):
            kw = dict(distinct=distinct)
            count = binding.host_refine_sets(g0, qp, bm, FULL, induced=True, **kw)
            count += binding.host_refine_sets_delta_nonedges(g1, qp, bm, D, FULL, **kw) - binding.host_refine_sets_delta(
                g0, qp, bm, D, FULL, induced=True, **kw)
            count += binding.host_refine_sets_delta(g2, qp, bm, I, FULL, induced=True, **kw) - binding.host_refine_sets_delta_nonedges(
                g1, qp, bm, I, FULL, **kw)
            assert count == binding.host_refine_sets(both, qp, bm, FULL, induced=True, **kw), (qp, distinct)


def test_host_query_nonedges(tmp_path):
    """3. gnnpe_host_query_nonedges: the pairs a < b that are not adjacent, ascending, NON_EDGES[shape] of them; a cap below the number
    returns GNNPE_ERR_ARG with *n_pairs set; the 32-vertex path has 465"""
    from gnnpe_amd import binding
    online, u32p = binding.load_online(), C.POINTER(C.c_uint32)
    for name in sh.SHAPES:
        qp = sh._shape_file(tmp_path, name)
        got = [tuple(p) for p in binding.host_query_nonedges(qp).tolist()]
        assert got == ri._non_edges(qp) == sorted(got) and len(got) == ri.NON_EDGES[name], name
        k = C.c_uint32(77)
        buf = np.full((len(got) + 1, 2), 9, np.uint32)
        if got:
            assert online.gnnpe_host_query_nonedges(qp.encode(), buf.ctypes.data_as(u32p), len(got) - 1, C.byref(k)) == -1
            assert k.value == len(got) and b"room for" in binding.load().gnnpe_last_error()
            assert online.gnnpe_host_query_nonedges(qp.encode(), None, 0, C.byref(k)) == -1 and k.value == len(got)
        assert online.gnnpe_host_query_nonedges(qp.encode(), buf.ctypes.data_as(u32p), len(got), C.byref(k)) == 0
        assert k.value == len(got) and (buf[len(got):] == 9).all()
    assert len(binding.host_query_nonedges(sh._path_file(tmp_path, 32))) == 465
    assert online.gnnpe_host_query_nonedges(None, None, 0, C.byref(C.c_uint32())) == -1


def test_repeats_and_orientations_mean_the_set(tmp_path_factory):
    """4. F with every pair twice, once reversed, in a shuffled order: the answer of the set; the limit cuts it; no F gives 0"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory)
    F = f["F"]
    noisy = np.concatenate([F, F[:, ::-1], F[::3]])
    noisy = noisy[np.random.default_rng(6).permutation(len(noisy))]
    for name in ("wedge", "diamond"):
        qp, bm = h["q"][name], h["bm"][name]["ld"]
        for distinct in (False, True):
            want = f["want"][name, "ld", distinct]
            assert want > 1
            assert binding.host_refine_sets_delta_nonedges(h["g"], qp, bm, noisy, FULL, distinct=distinct) == want
            for limit in (0, 1, want - 1, want, want + 1):
                assert binding.host_refine_sets_delta_nonedges(h["g"], qp, bm, F, limit, distinct=distinct) == min(want, limit)
        assert binding.host_refine_sets_delta_nonedges(h["g"], qp, bm, np.zeros((0, 2), np.uint32)) == 0


def test_host_refusals(tmp_path_factory, tmp_path):
    """5. a loop, an id >= n, a pair that is an edge, a mode without INDUCED, unknown mode bits, a disconnected query and null
    arguments return GNNPE_ERR_ARG with *answers = 0"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["wedge"], h["bm"]["wedge"]["ld"]
    good = f["F"][:4].tolist()
    edge = rdl._und_edges(g)[5].tolist()
    for bad, msg in ((edge, "is an edge"), (edge[::-1], "is an edge"), ((7, 7), "loop"), ((3, g["n"]), "does not have"),
                     ((g["n"] + 5, 2), "does not have")):
        with pytest.raises(binding.GnnpeError, match=msg):
            binding.host_refine_sets_delta_nonedges(g, qp, bm, good + [bad])
        assert _raw_host(binding, g, qp, bm, good + [bad], 2) == (-1, 0)
    assert _raw_host(binding, g, qp, bm, good, 2) == (0, binding.host_refine_sets_delta_nonedges(g, qp, bm, good))
    assert _raw_host(binding, g, qp, bm, good, 3) == (0, binding.host_refine_sets_delta_nonedges(g, qp, bm, good, distinct=True))
    for mode in (0, 1):
        assert _raw_host(binding, g, qp, bm, good, mode) == (-1, 0) and b"GNNPE_MATCH_INDUCED" in binding.load().gnnpe_last_error()
    for mode in (4, 6, 7, 1 << 31):
        assert _raw_host(binding, g, qp, bm, good, mode) == (-1, 0) and b"unknown mode" in binding.load().gnnpe_last_error()
    disc = str(tmp_path / "three.graph")
    ex._write_query(disc, 3, {(0, 1)}, [0, 0, 0])
    for limit in (FULL, 0):
        assert _raw_host(binding, g, disc, sh._ones(3, g["n"]), good, 2, limit) == (-1, 0)
        assert b"not connected" in binding.load().gnnpe_last_error()
    for null in ("offsets", "nbrs", "labels", "query", "bitmap", "pairs"):
        assert _raw_host(binding, g, qp, bm, good, 2, null=null)[0] == -1 and b"null argument" in binding.load().gnnpe_last_error()
    assert binding.load_online().gnnpe_host_refine_sets_delta_nonedges(g["n"], None, None, None, qp.encode(), None, None, 0, FULL, 2,
                                                                       None) == -1


def test_cli_refusals(tmp_path):
    """6. --delta-nonedges without --refine sets, without --induced, with --delta-edges, with --all-matches and with a count table
    exits 1 with its message before a GPU is touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    pf = str(tmp_path / "pairs.txt")
    open(pf, "w").write("0 1\n")
    m = str(tmp_path / "m.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    sets = ["--refine", "sets", "--induced", "--delta-nonedges", pf]
    for extra, msg in ((["--delta-nonedges", pf], "--delta-nonedges needs --refine sets"),
                       (["--refine", "sets", "--delta-nonedges", pf], "--delta-nonedges needs --induced"),
                       (sets + ["--delta-edges", pf], "--delta-nonedges and --delta-edges exclude each other"),
                       (sets + ["--matches", m, "--all-matches"], "--delta-nonedges excludes"),
                       (sets + ["--edge-counts", m], "--delta-nonedges excludes"),
                       (sets + ["--vertex-counts", m], "--delta-nonedges excludes"),
                       (["--delta-nonedges"], "--delta-nonedges needs a value")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout and not os.path.exists(m), extra


# ---- GPU: the device against the host form and against the plain call's rows -----------------------------------------------

def _device_equals_host(binding, eng, g, qp, bm, F, distinct, want, where, rows_too=True):
    """N and, with room for all of them, the rows: pairwise different valid induced maps on F; where the full listing is short
    enough, exactly the plain call's rows on F"""
    got, rows, ms = eng.refine_sets_delta_nonedges(qp, bm, F, matches_cap=want + 3, distinct=distinct)
    assert got == want == len(rows), where + (got, want, len(rows))
    if not rows_too or want == 0:
        return
    qnon = ri._non_edges(qp)
    n = len(g["labels"])
    assert _hits(rows, qnon, F, n).all(), where
    count = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=True)[0]
    if count <= ROWS_MAX:
        full = eng.refine_sets(qp, bm, limit=FULL, matches_cap=count, distinct=distinct, induced=True)[2]
        assert len(full) == count
        keep = full[_hits(full, qnon, F, n)].astype(np.int64)
        mine = rows.astype(np.int64)
        assert np.array_equal(mine[np.lexsort(mine.T[::-1])], keep[np.lexsort(keep.T[::-1])]), where
    else:
        ri._assert_rows(g, qp, bm, rows, True, re_._pairs(qp) if distinct else None)
        assert len(sh._row_set(rows)) == len(rows), where


@pytest.mark.gpu
@pytest.mark.parametrize("name", H1_SHAPES)
def test_gpu_h1_equals_the_host_form(tmp_path_factory, name):
    """7. H1 with the F of _h1_nonedges (a pair of hubs, a pendant and an isolated endpoint, a shared vertex, the ends of a wedge,
    vertex n - 1, 50 random non-edges), the three bitmaps, both induced modes: N is the host form's, and with matches_cap >= N the
    sorted rows are the sorted rows of refine_sets' full induced listing that hit F (filtered in numpy)"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory)
    assert f["want"][name, "ld", False] > 0
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            for distinct in (False, True):
                _device_equals_host(binding, eng, h["g"], h["q"][name], h["bm"][name][b], f["F"], distinct, f["want"][name, b, distinct],
                                    (name, b, distinct))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_small_graphs_equal_the_host_form(tmp_path_factory, gi):
    """8. the 15 small graphs with the eight shapes of ri.IND_SHAPES, both label variants, the label/degree and the thinned bitmap,
    both induced modes, the four forms of F: device == host form, rows as in 7"""
    from gnnpe_amd import binding, synth
    cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi]
    g = cases[0]["g"]
    sets = _small_sets(g, 3000 + gi)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            qnon = ri._non_edges(c["qp"])
            for b in ("ld", "thin"):
                for distinct in (False, True):
                    forms = dict(sets)
                    hit = _hit_set(_nx_rows(c, b, distinct), qnon)
                    if hit is not None:
                        forms["hit"] = hit
                    for form, F in forms.items():
                        want = binding.host_refine_sets_delta_nonedges(g, c["qp"], c[b], F, FULL, distinct=distinct)
                        _device_equals_host(binding, eng, g, c["qp"], c[b], F, distinct, want,
                                            (gi, c["name"], c["variant"], b, distinct, form))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_all_non_edges_is_the_induced_call(tmp_path_factory):
    """9. the charging rule.  F = every non-edge of the graph: N is refine_sets' induced count and the rows are its rows -- every match
    once, although it is met in the launch of each of its non-adjacent pairs (C5 five times, star5 six times without the rule).
    Three of the small graphs with the five shapes that have a non-adjacent pair, both label variants, both modes"""
    from gnnpe_amd import binding, synth
    for gi in (0, 2, 7):
        cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi and c["name"] in ri.NONEDGE_SHAPES]
        g = cases[0]["g"]
        non = _all_non_edges(g)
        eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
        try:
            for c in cases:
                for distinct in (False, True):
                    count = eng.refine_sets(c["qp"], c["ld"], limit=FULL, distinct=distinct, induced=True)[0]
                    assert count == len(_nx_rows(c, "ld", distinct))
                    got, rows, _ = eng.refine_sets_delta_nonedges(c["qp"], c["ld"], non, matches_cap=count + 1, distinct=distinct)
                    assert got == count == len(rows), (gi, c["name"], c["variant"], distinct, got, count)
                    full = eng.refine_sets(c["qp"], c["ld"], limit=FULL, matches_cap=max(count, 1), distinct=distinct, induced=True)[2]
                    assert sh._row_set(rows) == sh._row_set(full[:count]) and len(sh._row_set(rows)) == count
        finally:
            eng.close()


@pytest.mark.gpu
def test_gpu_identities_through_apply_edges(tmp_path_factory):
    """10. H1 with a labels-only bitmap, wedge, C4 and diamond, both induced modes, counts only.  Insertion of I (five pairs of hubs
    and 15 random non-edges, seed 3400): count(G), N(G, I), apply_edges(insert=I), Delta(G', I), count(G') -- count(G') = count(G) - N
    + Delta.  Deletion of D (20 random edges of G'): the mirror with Delta before and N after.  A mixed batch in the two steps of the
    header against the count on a freshly loaded graph that gnnpe_host_csr_apply_edges built in one go"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory)
    g, deg, a = h["g"], h["deg"], f["adjacent"]
    rng = np.random.default_rng(3400)
    hubs = np.nonzero(deg > 64)[0]
    hub_pairs = np.array([(x, y) for x in hubs for y in hubs if x < y and not a[x, y]], np.int64)
    assert len(hub_pairs) >= 5
    I = np.concatenate([hub_pairs[rng.choice(len(hub_pairs), 5, replace=False)], f["non"][rng.choice(len(f["non"]), 15, replace=False)]])
    assert len(rdl._codes(I, g["n"])) == 20
    g1 = binding.host_apply_edges(g, insert=I)
    e1 = rdl._und_edges(g1)
    D = e1[rng.choice(len(e1), 20, replace=False)]
    e0 = rdl._und_edges(g)
    D2 = e0[rng.choice(len(e0), 20, replace=False)]
    I2 = f["non"][rng.choice(len(f["non"]), 20, replace=False)]
    mixed = binding.host_apply_edges(g, insert=I2, delete=D2)
    eng = ex._engine(binding, g, h["sn"], 2)
    moved = 0
    try:
        for name in H1_SHAPES:
            qp = h["q"][name]
            bm = rdl._label_bitmap(g, qp)
            for distinct in (False, True):
                kw = dict(distinct=distinct)
                count = lambda: eng.refine_sets(qp, bm, limit=FULL, induced=True, **kw)[0]
                through = lambda F: eng.refine_sets_delta(qp, bm, F, induced=True, **kw)[0]
                non = lambda F: eng.refine_sets_delta_nonedges(qp, bm, F, **kw)[0]
                eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
                c0, gone = count(), non(I)
                eng.apply_edges(insert=I)
                came, c1 = through(I), count()
                assert c1 == c0 - gone + came and gone > 0 and came > 0, (name, distinct, c0, gone, came, c1)
                gone = through(D)
                eng.apply_edges(delete=D)
                came, c2 = non(D), count()
                assert c2 == c1 - gone + came and gone > 0, (name, distinct, c1, gone, came, c2)
                moved += came > 0
                # the mixed batch, in two steps, from G
                eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
                run = c0 - through(D2)
                eng.apply_edges(delete=D2)
                run += non(D2) - non(I2)
                eng.apply_edges(insert=I2)
                run += through(I2)
                assert run == count(), (name, distinct, "mixed")
                eng.load_csr(mixed["offsets"], mixed["nbrs"], mixed["labels"])
                assert run == count(), (name, distinct, "mixed, fresh")
        assert moved >= 3
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_limit_and_cap(tmp_path_factory):
    """11. C4 and the wedge on H1 with the F of _h1_nonedges, both modes.  Limits 1, N - 1, N, N + 1: *answers == min(N, limit), and
    the rows are pairwise different valid induced maps inside the sets that hit F.  matches_cap 0, 1 and N - 1 with the limit open:
    N, and exactly min(N, cap) rows.  star5 with 2 000 random non-edges and limit 10^5, which the host form reaches: the device
    returns the limit and 10^5 different valid rows.  Limit 0 launches nothing (device ms stays 0)"""
    from gnnpe_amd import binding
    h, f, hi = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory), ri._h1_induced(tmp_path_factory)
    g, F = h["g"], f["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("C4", "wedge"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            qnon = ri._non_edges(qp)
            for distinct in (False, True):
                N = f["want"][name, "ld", distinct]
                assert N > 2
                pairs = re_._pairs(qp) if distinct else None
                for limit in (1, N - 1, N, N + 1):
                    got, rows, _ = eng.refine_sets_delta_nonedges(qp, bm, F, limit=limit, matches_cap=N + 1, distinct=distinct)
                    assert got == min(N, limit) == len(rows) == len(sh._row_set(rows)), (name, distinct, limit, got, len(rows))
                    ri._assert_rows(g, qp, bm, rows, True, pairs)
                    assert _hits(rows, qnon, F, g["n"]).all()
                for cap in (0, 1, N - 1):
                    got, rows, _ = eng.refine_sets_delta_nonedges(qp, bm, F, matches_cap=cap, distinct=distinct)
                    assert got == N and len(rows) == cap, (name, distinct, cap, got, len(rows))
                    ri._assert_rows(g, qp, bm, rows, True, pairs)
                    assert _hits(rows, qnon, F, g["n"]).all()
                got, rows, ms = eng.refine_sets_delta_nonedges(qp, bm, F, limit=0, matches_cap=4, distinct=distinct)
                assert (got, len(rows), ms) == (0, 0, 0.0)
        qp, bm = hi["q"]["star5"], hi["bm"]["star5"]["ld"]
        many = f["non"][np.random.default_rng(3500).choice(len(f["non"]), 2000, replace=False)]
        limit = 10 ** 5
        assert binding.host_refine_sets_delta_nonedges(g, qp, bm, many, limit) == limit
        got, rows, _ = eng.refine_sets_delta_nonedges(qp, bm, many, limit=limit, matches_cap=limit)
        assert got == limit == len(rows) == len(sh._row_set(rows))
        ri._assert_rows(g, qp, bm, rows, True)
        assert _hits(rows, ri._non_edges(qp), many, g["n"]).all()
    finally:
        eng.close()


@pytest.fixture()
def nonedge_lines(monkeypatch, capfd):
    """contexts created while this fixture is active print one `[refine_delta_nonedges]` line per call that launches (GNNPE_DEBUG=1 is
    read when a context is created); the returned callable gives the lines since it was last called as dicts of integers"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [{k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])}
                for ln in err.splitlines() if ln.startswith("[refine_delta_nonedges] ")]
    return take


@pytest.mark.gpu
def test_gpu_query_sizes_and_orders(tmp_path_factory, tmp_path, nonedge_lines):
    """12. nq == 3: the walk begins at the leaf (the wedge on the 33-cycle; its only non-adjacent pair is the anchor, so the line says
    nonedges=0).  nq == 8: the 8-vertex path on the 33-cycle, 21 launches.  nq == 32: the 32-vertex path on the 32- and the 33-cycle,
    465 launches; position 31 carries bit 30 of older, gt and non.  F = three non-edges, then all non-edges (N = the induced count).
    The reversed-id files of test_refine_edge_counts on H1, which renumber the non-adjacent pairs.  The path 0-3-2-1 with the pair
    (0, 1), launch 0: position 2 is vertex 2, whose pivot is position 1 (the line says pivot2=1).  A query without a non-adjacent
    pair (vertex, edge, triangle, K4) gives 0 and launches nothing"""
    from gnnpe_amd import binding, synth
    h, f = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory)
    g, F = h["g"], f["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        nonedge_lines()
        for name in ("vertex", "edge", "triangle", "K4"):
            got, rows, ms = eng.refine_sets_delta_nonedges(h["q"][name], h["bm"][name]["ld"], F, matches_cap=4)
            assert (got, len(rows), ms) == (0, 0, 0.0), name
        got, rows, ms = eng.refine_sets_delta_nonedges(h["q"]["C4"], h["bm"]["C4"]["ld"], np.zeros((0, 2), np.int64), matches_cap=4)
        assert (got, len(rows), ms) == (0, 0, 0.0) and nonedge_lines() == []
        for name in H1_SHAPES:
            qp = re_._reversed_file(tmp_path, name, 0)
            bm = ex._ld_bitmap(g, qp)
            for distinct in (False, True):
                want = binding.host_refine_sets_delta_nonedges(g, qp, bm, F, FULL, distinct=distinct)
                assert want == f["want"][name, "ld", distinct] or distinct  # (one label: the shape is its own reversal)
                _device_equals_host(binding, eng, g, qp, bm, F, distinct, want, ("rev", name, distinct))
        p4 = str(tmp_path / "p0321.graph")
        ex._write_query(p4, 4, {(0, 3), (2, 3), (1, 2)}, [0] * 4)
        assert [tuple(p) for p in binding.host_query_nonedges(p4).tolist()] == [(0, 1), (0, 2), (1, 3)]
        bm = ex._ld_bitmap(g, p4)
        nonedge_lines()
        for distinct in (False, True):
            want = binding.host_refine_sets_delta_nonedges(g, p4, bm, F, FULL, distinct=distinct)
            assert want > 0
            _device_equals_host(binding, eng, g, p4, bm, F, distinct, want, ("p0321", distinct), rows_too=False)
        lines = nonedge_lines()
        assert len(lines) == 2 and all(ln["pivot2"] == 1 and ln["launches"] == 3 for ln in lines), lines
    finally:
        eng.close()
    p3, p8, p32 = sh._path_file(tmp_path, 3), sh._path_file(tmp_path, 8), sh._path_file(tmp_path, 32)
    for n, qp, launches in ((33, p3, 1), (33, p8, 21), (32, p32, 465), (33, p32, 465)):
        cyc = sh._cycle_graph(n)
        non = _all_non_edges(cyc)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            nq = binding.host_load_graph(qp)["n"]
            for bm in (ex._ld_bitmap(cyc, qp), sh._ones(nq, n)):
                for distinct in (False, True):
                    for Fc in (non[[0, 7, len(non) // 2]], non):
                        want = binding.host_refine_sets_delta_nonedges(cyc, qp, bm, Fc, FULL, distinct=distinct)
                        if len(Fc) == len(non):
                            assert want == binding.host_refine_sets(cyc, qp, bm, FULL, distinct=distinct, induced=True)
                            assert want == {(33, 3): 66, (33, 8): 66, (32, 32): 0, (33, 32): 66}[n, nq] // (2 if distinct else 1)
                        nonedge_lines()
                        _device_equals_host(binding, eng, cyc, qp, bm, Fc, distinct, want, (n, nq, distinct, len(Fc)))
                        ln = nonedge_lines()[0]
                        assert ln["launches"] == launches and ln["items"] == 2 * len(Fc), ln
                        assert nq > 3 or ln["nonedges"] == 0, ln
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, seed):
    """13. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of bitmap) in
    both induced modes, F a random subset of the non-edges whose size is drawn from {1, 2, 50, a quarter}: device == host form,
    rows as in 7"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    non = _all_non_edges(g)
    rng = np.random.default_rng(3600 + seed)
    size = (1, 2, 50, max(1, len(non) // 4))[int(rng.integers(0, 4))]
    F = non[rng.choice(len(non), min(size, len(non)), replace=False)]
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for distinct in (False, True):
            want = binding.host_refine_sets_delta_nonedges(g, c["qp"], c["bm"], F, FULL, distinct=distinct)
            _device_equals_host(binding, eng, g, c["qp"], c["bm"], F, distinct, want, (seed, c["which"], len(F), distinct),
                                rows_too=want <= ROWS_MAX)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory, tmp_path):
    """14. a pair that is an edge among valid ones returns GNNPE_ERR_ARG with *answers == 0 -- found on the device, in the call's one
    wait -- and the NEXT valid call on the same context returns the right N; x == y, an id >= n; a mode without INDUCED, unknown mode
    bits; 33 query vertices; the multigraph state; a context whose rows did not come through gnnpe_load_csr.  All of them are
    decided on the host or by the flag of the lookup kernel"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_nonedges(tmp_path_factory)
    g, F = h["g"], f["F"]
    qp, bm = h["q"]["C4"], h["bm"]["C4"]["ld"]
    want = f["want"]["C4", "ld", False]
    x = int(np.argmax(h["deg"]))
    o = g["offsets"].astype(np.int64)
    edges = [(x, int(g["nbrs"][o[x]])), (int(g["nbrs"][o[x + 1] - 1]), x), tuple(rdl._und_edges(g)[100].tolist())]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        assert _raw_device(binding, eng, qp, bm, F) == (0, want)
        for bad in edges:
            for mode in (2, 3):
                assert _raw_device(binding, eng, qp, bm, F.tolist() + [bad], mode=mode) == (-1, 0), (bad, mode)
                assert b"is an edge" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, qp, bm, F) == (0, want)
            with pytest.raises(binding.GnnpeError, match="is an edge"):
                eng.refine_sets_delta_nonedges(qp, bm, [bad] + F.tolist(), matches_cap=10)
            assert eng.refine_sets_delta_nonedges(qp, bm, F, matches_cap=3)[0] == want
        for bad, msg in (((7, 7), b"loop"), ((3, g["n"]), b"does not have"), ((g["n"] + 5, 2), b"does not have")):
            assert _raw_device(binding, eng, qp, bm, F.tolist() + [bad]) == (-1, 0) and msg in binding.load().gnnpe_last_error()
        for mode in (0, 1):
            assert _raw_device(binding, eng, qp, bm, F, mode=mode) == (-1, 0)
            assert b"GNNPE_MATCH_INDUCED" in binding.load().gnnpe_last_error()
        for mode in (4, 6, 1 << 31):
            assert _raw_device(binding, eng, qp, bm, F, mode=mode) == (-1, 0) and b"unknown mode" in binding.load().gnnpe_last_error()
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets_delta_nonedges(sh._path_file(tmp_path, 33), sh._ones(33, g["n"]), F)
        assert _raw_device(binding, eng, qp, bm, F) == (0, want)  # the context still answers
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.refine_sets_delta_nonedges(qp, bm, F)
    finally:
        eng.close()
    bare = binding.Engine(0)
    try:
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            bare.refine_sets_delta_nonedges(qp, bm, F)
    finally:
        bare.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", ["q1", "q2"])
def test_gpu_cli_delta_nonedges(tmp_path, test_graph, q):
    """15. gnnpe_main -m online --exact --refine sets --induced --delta-nonedges on the golden test graph, q1 and q2: the answer line
    carries the host form's N on the label/degree bitmap (the exact filter's sets are complete), with and without --distinct, for F =
    eight non-edges that each carry a match (found with the host form on single pairs) and 40 random non-edges (seed 3700), written
    in both orientations and with a repeat; with --matches the file holds N pairwise different rows that hit F.  A file with an edge
    of the graph is refused"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    non = _all_non_edges(test_graph)
    rng = np.random.default_rng(3700)
    qnon = ri._non_edges(qp)
    assert qnon
    # non-edges that carry a match: both ends in the support of the induced vertex table, and the host form of the single pair
    a = _adjacent(test_graph)
    V = binding.host_refine_sets_vertex_counts(test_graph, qp, ld, induced=True)[2]
    cand = [(int(x), int(y)) for u, w in qnon for x in np.nonzero(V[u])[0] for y in np.nonzero(V[w])[0] if x != y and not a[x, y]]
    live = []
    for p in cand:
        if len(live) < 8 and p not in live and binding.host_refine_sets_delta_nonedges(test_graph, qp, ld, [p], 1) == 1:
            live.append(p)
    assert len(live) == 8, "fewer than eight non-edges under a non-adjacent query pair of a match"
    F = np.concatenate([np.array(live, np.int64), non[rng.choice(len(non), 40, replace=False)]])
    pf = str(tmp_path / "pairs.txt")
    open(pf, "w").write("".join(f"{x} {y}\n" if i % 2 else f"{y} {x}\n" for i, (x, y) in enumerate(F.tolist() + F[:1].tolist())))
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--induced",
            "--delta-nonedges", pf]
    for distinct in (False, True):
        want = binding.host_refine_sets_delta_nonedges(test_graph, qp, ld, F, FULL, distinct=distinct)
        count = binding.host_refine_sets(test_graph, qp, ld, FULL, distinct=distinct, induced=True)
        assert 0 < want <= count and (q != "q1" or distinct or want < count), (want, count)
        out = str(tmp_path / f"m{int(distinct)}.txt")
        r = subprocess.run(base + ["--matches", out] + (["--distinct"] if distinct else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        assert ans == want, (distinct, ans, want)
        rows = np.loadtxt(out, dtype=np.int64, ndmin=2) if want else np.zeros((0, 1), np.int64)
        assert len(rows) == want and len(np.unique(rows, axis=0)) == want and (want == 0 or _hits(rows, qnon, F, n).all())
    bad = str(tmp_path / "bad.txt")
    x, y = rdl._und_edges(test_graph)[0].tolist()
    open(bad, "w").write(f"{x} {y}\n")
    r = subprocess.run(base[:-1] + [bad], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "is an edge" in r.stderr and "Answer Number" not in r.stdout
