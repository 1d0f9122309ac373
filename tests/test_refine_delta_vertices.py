"""The matches through a set of data vertices, each once (include/gnnpe_online.h): DeltaV_m(C, S, limit) = the maps of mode m with
at least one image in S, on the host (gnnpe_host_refine_sets_delta_vertices), on the device (gnnpe_refine_sets_delta_vertices) and
through `gnnpe_main --delta-vertices`.

The host form walks all of M and drops the finds that avoid S.  It is held to yardsticks that are not the library's new code:
networkx's rows filtered in numpy by "an image in S", the edge-anchored host form over E(S), the plain count for S = V, the column
sums of the vertex table for S = {s}, and the vertex-removal and relabel identities between two graphs.  The device form starts at
S n C(u) instead, once per query vertex, and charges every match to its lowest-numbered query vertex with an image in S; it is
held to the host form, to the existing device call over E(S), to the rows gnnpe_refine_sets_mode lists (filtered in numpy) and to
S = V, where DeltaV = |M| and any match charged twice or dropped shows.  The yardstick is never the new kernel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_delta as dl
import test_refine_distinct as rd
import test_refine_edge_counts as re_
import test_refine_induced as ri
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = dl.MODES
H1_V_SHAPES = ("vertex", "edge", "wedge", "triangle", "diamond", "K4")
ROWS_MAX = 500_000  # DeltaV up to which the rows are compared with the filtered listing of refine_sets
LIST_MAX = 2_000_000  # ... where that listing is at most this long (on H1 every one is: the longest has 413 422 rows)


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _hits(rows, S):
    """mask of the rows with at least one image in S"""
    rows = np.asarray(rows, np.int64)
    return np.isin(rows, np.asarray(S, np.int64)).any(axis=1) if len(rows) else np.zeros(0, bool)


def _edges_at(g, S):
    """E(S): the undirected edges with an endpoint in S"""
    e = dl._und_edges(g)
    return e[np.isin(e[:, 0], S) | np.isin(e[:, 1], S)]


def _mode_rows(c, b, distinct, induced):
    """the rows of a case of sh._nx_case in a mode, inside bitmap b: networkx's monomorphisms, cut in numpy"""
    rows = c["emb"][rs._in_sets(c[b], c["emb"])]
    if induced:
        rows = rows[ri._induced_mask(c["g"], c["qp"], rows)]
    if distinct:
        rows = rows[rd._ordered(rows, re_._pairs(c["qp"]))]
    return rows


def _dense_cases(tmp_path_factory):
    """the cases of sh._nx_cases on the three dense graphs of sh._dense_graphs (the first three graphs there)"""
    return [c for c in sh._nx_cases(tmp_path_factory) if c["gi"] < 3]


def _relabelled(g, S, seed, n_labels):
    """g with new labels on the vertices of S, each different from the old one where there are two labels or more"""
    rng = np.random.default_rng(seed)
    labels = g["labels"].copy()
    new = rng.integers(0, n_labels, len(S)).astype(np.uint32)
    if n_labels > 1:
        same = new == labels[S]
        new[same] = (new[same] + 1) % n_labels
    labels[S] = new
    return dict(n=g["n"], offsets=g["offsets"], nbrs=g["nbrs"], labels=labels), new


_H1S = {}


def _h1_vertices(tmp_path_factory):
    """H1 with the S of the device tests, each part asserted to exist: the vertex with the longest row (155 entries: its first level is
    several chunks), a vertex of degree 1, an isolated vertex, two adjacent vertices, the three vertices of a triangle, vertex
    n - 1, and 50 random vertices (seed 3100).  With it the host form's DeltaV of H1_V_SHAPES on the three bitmaps in the four
    modes, computed once"""
    if _H1S:
        return _H1S
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, deg = h["g"], h["deg"]
    o = g["offsets"].astype(np.int64)
    hub = int(np.argmax(deg))
    assert deg[hub] > 64
    leaf, iso = int(np.nonzero(deg == 1)[0][0]), int(np.nonzero(deg == 0)[0][0])
    w = int(np.nonzero((deg >= 2) & (deg <= 64))[0][0])
    pair = [w, int(g["nbrs"][o[w]])]
    e = dl._und_edges(g)
    tri = next(((x, y, int(z)) for x, y in e[::37].tolist()
                for z in np.intersect1d(g["nbrs"][o[x]:o[x + 1]], g["nbrs"][o[y]:o[y + 1]])[:1]), None)
    assert tri is not None
    rnd = np.random.default_rng(3100).choice(g["n"], 50, replace=False)
    S = np.unique(np.array([hub, leaf, iso] + pair + list(tri) + [g["n"] - 1] + rnd.tolist(), np.int64))
    want = {}
    for name in H1_V_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                want[name, b, distinct, induced] = binding.host_refine_sets_delta_vertices(g, h["q"][name], h["bm"][name][b], S, FULL,
                                                                                           distinct=distinct, induced=induced)
    _H1S.update(S=S, want=want, hub=hub, E=_edges_at(g, S), listing={})
    return _H1S


def _raw_device(binding, eng, qp, bm, vertices, limit=FULL, mode=0):
    """gnnpe_refine_sets_delta_vertices through ctypes: (return code, *answers); *answers is set to a canary first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    s = np.ascontiguousarray(np.asarray(vertices, np.int64).reshape(-1), np.uint32)
    out, ms = C.c_uint64(12345), C.c_double()
    rc = binding.load_online().gnnpe_refine_sets_delta_vertices(eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), s.ctypes.data_as(u32p),
                                                                len(s), limit, mode, C.byref(out), None, 0, C.byref(ms))
    return rc, out.value


# ---- CPU: the host form against yardsticks that are not the new code -------------------------------------------------------------

def test_host_form_against_networkx_and_the_edge_anchored_form(tmp_path_factory):
    """1. the three dense graphs, the eight shapes of sh.NX_SHAPES, both label variants, the label/degree and the thinned bitmap, the
    four modes, S = one vertex, three vertices, a third of the vertices, all of them: the host form is the number of networkx's rows
    of the mode with an image in S; for nq >= 2 it is host_refine_sets_delta over E(S); S = V is the plain count; S = {s} is the
    column sum of the vertex table.  At least a fifth of the cases have a match through S and a tenth one that avoids it"""
    from gnnpe_amd import binding
    cases = _dense_cases(tmp_path_factory)
    assert len(cases) == 3 * len(sh.NX_SHAPES) * 2
    some = part = total = 0
    for c in cases:
        g, n, qp = c["g"], c["g"]["n"], c["qp"]
        nq = sh.SHAPES[c["name"]][0]
        rng = np.random.default_rng(3200 + c["gi"])
        sets = dict(one=rng.choice(n, 1), three=rng.choice(n, 3, replace=False), third=rng.choice(n, n // 3, replace=False), all=np.arange(n))
        for b in ("ld", "thin"):
            for distinct, induced in MODES:
                rows = _mode_rows(c, b, distinct, induced)
                where = (c["gi"], c["name"], c["variant"], b, distinct, induced)
                for form, S in sets.items():
                    want = int(_hits(rows, S).sum())
                    got = binding.host_refine_sets_delta_vertices(g, qp, c[b], S, FULL, distinct=distinct, induced=induced)
                    assert got == want, where + (form, got, want)
                    if nq >= 2:
                        assert got == binding.host_refine_sets_delta(g, qp, c[b], _edges_at(g, S), FULL, distinct=distinct, induced=induced), where
                    total += 1
                    some += want > 0
                    part += 0 < want < len(rows)
                assert binding.host_refine_sets_delta_vertices(g, qp, c[b], sets["all"], FULL, distinct=distinct, induced=induced) == \
                    binding.host_refine_sets(g, qp, c[b], FULL, distinct=distinct, induced=induced) == len(rows), where
                s = int(sets["one"][0])
                table = binding.host_refine_sets_vertex_counts(g, qp, c[b], FULL, distinct=distinct, induced=induced)[2]
                assert binding.host_refine_sets_delta_vertices(g, qp, c[b], [s], FULL, distinct=distinct, induced=induced) == int(table[:, s].sum()), where
    assert some * 5 >= total and part * 10 >= total, (some, part, total)


def test_host_vertex_removal_and_relabel_identities(tmp_path_factory):
    """2. between two host graphs, the four modes.  REMOVAL: G' = G minus E(S), nq >= 2, a labels-only bitmap:
    |M(G')| == |M(G)| - DeltaV(G, S).  RELABEL: G' = G with new labels on S, the labels-only bitmap of each graph:
    |M(G', C')| == |M(G, C)| - DeltaV(G, C, S) + DeltaV(G', C', S).  The dense graphs with both label variants of every shape, S a
    sixth of the vertices; over the run the relabel loses matches and gains matches in at least ten cases each"""
    from gnnpe_amd import binding
    lost_n = gained_n = 0
    for c in _dense_cases(tmp_path_factory):
        g, n, qp = c["g"], c["g"]["n"], c["qp"]
        S = np.sort(np.random.default_rng(3300 + c["gi"]).choice(n, max(2, n // 6), replace=False))
        g_cut = dl._without(g, _edges_at(g, S))
        g_new, _ = _relabelled(g, S, 3400 + c["gi"], 2)
        bm, bm_new = dl._label_bitmap(g, qp), dl._label_bitmap(g_new, qp)
        for distinct, induced in MODES:
            kw = dict(distinct=distinct, induced=induced)
            where = (c["gi"], c["name"], c["variant"], distinct, induced)
            m = binding.host_refine_sets(g, qp, bm, FULL, **kw)
            lost = binding.host_refine_sets_delta_vertices(g, qp, bm, S, FULL, **kw)
            if sh.SHAPES[c["name"]][0] >= 2:
                assert binding.host_refine_sets(g_cut, qp, bm, FULL, **kw) == m - lost, where
            gained = binding.host_refine_sets_delta_vertices(g_new, qp, bm_new, S, FULL, **kw)
            assert binding.host_refine_sets(g_new, qp, bm_new, FULL, **kw) == m - lost + gained, where + (m, lost, gained)
            lost_n += lost > 0
            gained_n += gained > 0
    assert lost_n >= 10 and gained_n >= 10, (lost_n, gained_n)


def test_host_repeats_limits_and_refusals(tmp_path_factory, tmp_path):
    """3. repeats mean the set; no vertices, limit 0: 0; a limit below DeltaV cuts; an id >= n, unknown mode bits, a disconnected
    query and a null list with a count are refused with *answers == 0"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    S = np.random.default_rng(3500).choice(g["n"], 40, replace=False)
    want = binding.host_refine_sets_delta_vertices(g, qp, bm, S)
    assert 2 < want < h["want"]["triangle", "ld"]
    assert binding.host_refine_sets_delta_vertices(g, qp, bm, np.concatenate([S, S[::-1], S[:7]])) == want
    assert binding.host_refine_sets_delta_vertices(g, qp, bm, []) == 0
    assert binding.host_refine_sets_delta_vertices(g, qp, bm, S, limit=0) == 0
    assert binding.host_refine_sets_delta_vertices(g, qp, bm, S, limit=want - 1) == want - 1
    assert binding.host_refine_sets_delta_vertices(g, qp, bm, S, limit=want + 1) == want
    # nq == 1: the members of S n C(0) that pass the label and degree test; the edge-anchored form gives 0
    one = h["bm"]["vertex"]["thin"]
    inside = np.intersect1d(S, sh._members(one[0], g["n"]))
    assert 0 < len(inside) < len(S)
    assert binding.host_refine_sets_delta_vertices(g, h["q"]["vertex"], one, S) == len(inside)
    assert binding.host_refine_sets_delta(g, h["q"]["vertex"], one, _edges_at(g, S)) == 0
    for bad in (g["n"], g["n"] + 7, 0xFFFFFFFF):
        with pytest.raises(binding.GnnpeError, match="does not have"):
            binding.host_refine_sets_delta_vertices(g, qp, bm, S.tolist() + [bad])
        with pytest.raises(binding.GnnpeError, match="does not have"):
            binding.host_refine_sets_delta_vertices(g, qp, bm, [bad], limit=0)
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    with pytest.raises(binding.GnnpeError, match="not connected"):
        binding.host_refine_sets_delta_vertices(g, disc, sh._ones(2, g["n"]), S)
    u32p = C.POINTER(C.c_uint32)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    s32, bmc = np.ascontiguousarray(S, np.uint32), np.ascontiguousarray(bm, np.uint32)
    fn = binding.load_online().gnnpe_host_refine_sets_delta_vertices
    for mode, ids, cnt, msg in ((4, s32.ctypes.data_as(u32p), len(s32), b"unknown mode"), (1 << 31, s32.ctypes.data_as(u32p), len(s32), b"unknown mode"),
                                (0, None, 3, b"null argument")):
        out = C.c_uint64(12345)
        rc = fn(g["n"], o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), lb.ctypes.data_as(u32p), qp.encode(), bmc.ctypes.data_as(u32p), ids,
                cnt, FULL, mode, C.byref(out))
        assert rc == -1 and msg in binding.load().gnnpe_last_error(), (mode, cnt)
        assert out.value == (12345 if ids is None else 0)


def test_cli_refusals(tmp_path):
    """4. --delta-vertices without --refine sets, with --delta-edges, --delta-nonedges, --all-matches and the count tables, a
    malformed vertex file, --set-labels outside exact mode and a malformed label file: exit 1 with the message before a GPU is
    touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    vf, ef, bad, lf, badl = (str(tmp_path / f) for f in ("v.txt", "e.txt", "bad.txt", "l.txt", "badl.txt"))
    open(vf, "w").write("0\n5\n")
    open(ef, "w").write("0 1\n")
    open(bad, "w").write("0\nx\n")
    open(lf, "w").write("0 1\n")
    open(badl, "w").write("0 1\n3\n")
    m = str(tmp_path / "m.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online"]
    sets = ["--exact", "--refine", "sets", "--delta-vertices", vf]
    for extra, msg in ((["--exact", "--delta-vertices", vf], "--delta-vertices needs --refine sets"),
                       (sets + ["--delta-edges", ef], "--delta-vertices excludes --delta-edges"),
                       (sets + ["--induced", "--delta-nonedges", ef], "--delta-vertices excludes --delta-edges and --delta-nonedges"),
                       (sets + ["--matches", m, "--all-matches"], "--delta-vertices excludes --all-matches"),
                       (sets + ["--vertex-counts", m], "--delta-vertices excludes"),
                       (sets + ["--edge-counts", m], "--delta-vertices excludes"),
                       (sets[:-1] + [bad], "one vertex id per line expected"),
                       (["--set-labels", lf], "--set-labels applies to exact"),
                       (["--exact", "--set-labels", badl], "one `v label` per line expected")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout and not os.path.exists(m), extra


# ---- GPU: the device against the host form, the edge-anchored device call and the plain call's rows ---------------------------

def _device_equals_host(binding, eng, g, qp, bm, S, distinct, induced, want, where, listing=None, key=None):
    """DeltaV and, with room for all of them, the rows: for nq >= 2 the count of the existing device call over E(S); where DeltaV
    is at most ROWS_MAX (and the plain listing at most LIST_MAX rows), exactly the plain call's rows with an image in S (filtered in
    numpy; `listing` keeps them by `key` across the runs of one module); otherwise valid, pairwise different rows of the mode with
    an image in S.  Returns whether the rows were compared with the listing."""
    got, rows, ms = eng.refine_sets_delta_vertices(qp, bm, S, matches_cap=want + 3, distinct=distinct, induced=induced)
    assert got == want == len(rows), where + (got, want, len(rows))
    nq = np.asarray(bm).shape[0]
    if nq >= 2:
        assert eng.refine_sets_delta(qp, bm, _edges_at(g, S), distinct=distinct, induced=induced)[0] == want, where
    keep = None if listing is None else listing.get(key)
    count = 0 if keep is not None or want > ROWS_MAX else eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
    if want > ROWS_MAX or count > LIST_MAX:
        ri._assert_rows(g, qp, bm, rows, induced, re_._pairs(qp) if distinct else None)
        assert _hits(rows, S).all(), where
        return False
    if keep is None:
        full = eng.refine_sets(qp, bm, limit=FULL, matches_cap=max(count, 1), distinct=distinct, induced=induced)[2]
        assert len(full) == count
        keep = full[_hits(full, S)].astype(np.int64)
        keep = keep[np.lexsort(keep.T[::-1])]
        if listing is not None:
            listing[key] = keep
    mine = rows.astype(np.int64)
    assert np.array_equal(mine[np.lexsort(mine.T[::-1])], keep), where
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [None, 0, 3, 6])
def test_gpu_h1_equals_the_host_form(tmp_path_factory, monkeypatch, capfd, shift):
    """a. H1 with the S of _h1_vertices (the longest row, a vertex of degree 1, an isolated one, two adjacent ones, a triangle,
    vertex n - 1, 50 random ones), vertex, edge, wedge, triangle, diamond and K4 on the three bitmaps in the four modes, with the
    heuristic's first-level shift and with GNNPE_TESTING=sets_first_shift= 0, 3 and 6 (the chunk base falls mid-row, the hub of S
    gives many items): DeltaV is the host form's and, for nq >= 2, the existing device call's over E(S); the sorted rows are the
    sorted rows of refine_sets' full listing with an image in S.  At least three quarters of the cases are compared row for row"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_vertices(tmp_path_factory)
    g, deg, S = h["g"], h["deg"], f["S"]
    o = g["offsets"].astype(np.int64)
    assert (deg[S] > 64).any() and (deg[S] == 1).any() and (deg[S] == 0).any() and g["n"] - 1 in S and len(S) >= 50
    assert len(f["E"]) and np.isin(f["E"], S).all(axis=1).any()  # two adjacent vertices
    assert any(np.isin(np.intersect1d(g["nbrs"][o[x]:o[x + 1]], g["nbrs"][o[y]:o[y + 1]]), S).any()
               for x, y in f["E"][np.isin(f["E"], S).all(axis=1)].tolist())  # the three vertices of a triangle
    if shift is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    monkeypatch.setenv("GNNPE_DEBUG", "1")  # (read when the context is created: one `[refine_delta_vertices]` line per call)
    eng = ex._engine(binding, g, h["sn"], 2)
    capfd.readouterr()
    compared = total = 0
    try:
        for name in H1_V_SHAPES:
            for b in sh.BITMAPS:
                for distinct, induced in MODES:
                    key = (name, b, distinct, induced)
                    compared += _device_equals_host(binding, eng, g, h["q"][name], h["bm"][name][b], S, distinct, induced, f["want"][key],
                                                    (shift,) + key, f["listing"], key)
                    total += 1
    finally:
        eng.close()
    assert total == len(H1_V_SHAPES) * 12 and compared * 4 >= total * 3, (compared, total)
    sys.stderr.flush()
    said = [{k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])}
            for ln in capfd.readouterr().err.splitlines() if ln.startswith("[refine_delta_vertices] ")]
    # (a call that launches nothing prints nothing)
    assert total * 3 <= len(said) * 4 <= total * 4 and all(ln["vertices"] == len(S) and ln["hubs"] >= 10 and 1 <= ln["launches"] <= 4 for ln in said), said[:3]
    if shift is not None:  # the forced first-level chunk width is honoured; nothing forced, H1's few start candidates take single entries
        assert all(ln["shift"] == shift for ln in said), said[:3]
    else:
        assert all(ln["shift"] == 0 for ln in said), said[:3]
    assert f["want"]["K4", "ld", False, False] > 1024  # past the flush of a wave's finds


@pytest.mark.gpu
def test_gpu_all_vertices_is_the_plain_call(tmp_path_factory):
    """b. the charging rule.  S = V: DeltaV is refine_sets' count -- every match once, although it is met in the launch of each of
    its query vertices (without the rule the count is nq times too large) -- for every shape of H1_V_SHAPES on the three bitmaps
    in the four modes; for the triangle the rows are the plain call's rows"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    V = np.arange(g["n"])
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in H1_V_SHAPES:
            for b in sh.BITMAPS:
                for distinct, induced in MODES:
                    qp, bm = h["q"][name], h["bm"][name][b]
                    count = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                    assert distinct or induced or count == h["want"][name, b]
                    cap = count + 1 if name == "triangle" else 0
                    got, rows, _ = eng.refine_sets_delta_vertices(qp, bm, V, matches_cap=cap, distinct=distinct, induced=induced)
                    assert got == count, (name, b, distinct, induced, got, count)
                    if cap:
                        full = eng.refine_sets(qp, bm, limit=FULL, matches_cap=max(count, 1), distinct=distinct, induced=induced)[2]
                        assert len(rows) == count == len(sh._row_set(rows)) and sh._row_set(rows) == sh._row_set(full)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_form(tmp_path_factory, seed):
    """c. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of bitmap)
    in the four modes, S a seeded tenth of the vertices (at least one): device == host form, rows as in (a)"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    S = np.random.default_rng(3600 + seed).choice(g["n"], max(1, g["n"] // 10), replace=False)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for distinct, induced in MODES:
            want = binding.host_refine_sets_delta_vertices(g, c["qp"], c["bm"], S, FULL, distinct=distinct, induced=induced)
            _device_equals_host(binding, eng, g, c["qp"], c["bm"], S, distinct, induced, want, (seed, c["which"], len(S), distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_limit_and_cap(tmp_path_factory):
    """d. K4 and the wedge on H1 with the S of _h1_vertices, the four modes.  Limits 1, 1023, 1024, 1025, DeltaV - 1, DeltaV,
    DeltaV + 1: *answers == min(DeltaV, limit), and the rows are pairwise different valid maps of the mode inside the sets with an
    image in S.  matches_cap 0, 1 and DeltaV - 1 with the limit open: DeltaV, and exactly min(DeltaV, cap) rows"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_vertices(tmp_path_factory)
    g, S = h["g"], f["S"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("K4", "wedge"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            for distinct, induced in MODES:
                delta = f["want"][name, "ld", distinct, induced]
                assert delta > 2
                pairs = re_._pairs(qp) if distinct else None
                for limit in sorted({1, 1023, 1024, 1025, delta - 1, delta, delta + 1}):
                    got, rows, _ = eng.refine_sets_delta_vertices(qp, bm, S, limit=limit, matches_cap=delta + 1, distinct=distinct,
                                                                  induced=induced)
                    assert got == min(delta, limit) == len(rows), (name, distinct, induced, limit, got, len(rows))
                    ri._assert_rows(g, qp, bm, rows, induced, pairs)
                    assert _hits(rows, S).all()
                for cap in (0, 1, delta - 1):
                    got, rows, _ = eng.refine_sets_delta_vertices(qp, bm, S, matches_cap=cap, distinct=distinct, induced=induced)
                    assert got == delta and len(rows) == cap, (name, distinct, induced, cap, got, len(rows))
                    ri._assert_rows(g, qp, bm, rows, induced, pairs)
                    assert _hits(rows, S).all()
        assert f["want"]["K4", "ld", False, False] > 1025
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_query_sizes(tmp_path_factory, tmp_path):
    """e. nq == 1: DeltaV = |S n C(0)| and the rows are those vertices (the edge-anchored call gives 0); no vertices: 0 and nothing
    launched (device ms stays 0).  nq == 2: depth 1 is the leaf.  nq == 32: the 32-vertex path on the 32- and the 33-cycle in the
    four modes with S = three vertices and S = V -- position 31 carries bit 31 of the charge mask"""
    from gnnpe_amd import binding, synth
    h, f = sh._h1(tmp_path_factory), _h1_vertices(tmp_path_factory)
    g, S = h["g"], f["S"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            bm = h["bm"]["vertex"][b]
            inside = np.intersect1d(S, sh._members(bm[0], g["n"]))
            got, rows, _ = eng.refine_sets_delta_vertices(h["q"]["vertex"], bm, S, matches_cap=len(S) + 1)
            assert got == len(inside) == len(rows) and np.array_equal(np.sort(rows[:, 0]), inside), b
            assert eng.refine_sets_delta(h["q"]["vertex"], bm, f["E"])[0] == 0
            got, rows, ms = eng.refine_sets_delta_vertices(h["q"]["edge"], h["bm"]["edge"][b], [], matches_cap=4)
            assert (got, len(rows), ms) == (0, 0, 0.0)
            got, rows, ms = eng.refine_sets_delta_vertices(h["q"]["edge"], h["bm"]["edge"][b], S, limit=0, matches_cap=4)
            assert (got, len(rows), ms) == (0, 0, 0.0)
            for distinct, induced in MODES:
                want = binding.host_refine_sets_delta_vertices(g, h["q"]["edge"], h["bm"]["edge"][b], S, FULL, distinct=distinct, induced=induced)
                _device_equals_host(binding, eng, g, h["q"]["edge"], h["bm"]["edge"][b], S, distinct, induced, want, ("edge", b, distinct, induced))
        # repeats mean the set
        rep = np.concatenate([S, S[::-1]])
        assert eng.refine_sets_delta_vertices(h["q"]["triangle"], h["bm"]["triangle"]["ld"], rep)[0] == f["want"]["triangle", "ld", False, False]
    finally:
        eng.close()
    p32 = sh._path_file(tmp_path, 32)
    for n in (32, 33):
        cyc = sh._cycle_graph(n)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            for bm in (ex._ld_bitmap(cyc, p32), sh._ones(32, n)):
                for distinct, induced in MODES:
                    for Sc in (np.array([0, 1, n // 2]), np.arange(n)):
                        want = binding.host_refine_sets_delta_vertices(cyc, p32, bm, Sc, FULL, distinct=distinct, induced=induced)
                        if len(Sc) == n:
                            assert want == binding.host_refine_sets(cyc, p32, bm, FULL, distinct=distinct, induced=induced)
                        _device_equals_host(binding, eng, cyc, p32, bm, Sc, distinct, induced, want, (n, distinct, induced, len(Sc)))
        finally:
            eng.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory, tmp_path):
    """f. an id >= n among valid ones returns GNNPE_ERR_ARG with *answers == 0, and so do unknown mode bits; 33 query vertices; the
    multigraph state; a slab context (rows that did not come through gnnpe_load_csr); a context without a graph.  After each
    refusal the context answers a plain call correctly"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), _h1_vertices(tmp_path_factory)
    g, S = h["g"], f["S"]
    qp, bm = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    want, plain = f["want"]["triangle", "ld", False, False], h["want"]["triangle", "ld"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        assert _raw_device(binding, eng, qp, bm, S) == (0, want)
        for bad in (g["n"], g["n"] + 5, 0xFFFFFFFF):
            for mode in (0, 1, 2, 3):
                assert _raw_device(binding, eng, qp, bm, S.tolist() + [bad], mode=mode) == (-1, 0), (bad, mode)
                assert b"does not have" in binding.load().gnnpe_last_error()
            assert eng.refine_sets(qp, bm, limit=FULL)[0] == plain
            with pytest.raises(binding.GnnpeError, match="does not have"):
                eng.refine_sets_delta_vertices(qp, bm, [bad] + S.tolist(), matches_cap=10)
            assert _raw_device(binding, eng, qp, bm, S) == (0, want)
        for mode in (4, 1 << 31):
            assert _raw_device(binding, eng, qp, bm, S, mode=mode) == (-1, 0) and b"unknown mode" in binding.load().gnnpe_last_error()
            assert eng.refine_sets(qp, bm, limit=FULL)[0] == plain
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.refine_sets_delta_vertices(sh._path_file(tmp_path, 33), sh._ones(33, g["n"]), S)
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == plain
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.refine_sets_delta_vertices(qp, bm, S)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == plain and _raw_device(binding, eng, qp, bm, S) == (0, want)
        # a slab context: the rows of the first half of the vertices only
        half = g["n"] // 2
        o = g["offsets"].astype(np.uint64)
        eng.load_rows(g["n"], g["labels"], np.arange(half, dtype=np.uint32), o[:half + 1], g["nbrs"][:int(o[half])])
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            eng.refine_sets_delta_vertices(qp, bm, S)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == plain
    finally:
        eng.close()
    bare = binding.Engine(0)
    try:
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            bare.refine_sets_delta_vertices(qp, bm, S)
    finally:
        bare.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", ["q1", "q2"])
def test_gpu_cli_delta_vertices(tmp_path, test_graph, q):
    """g. gnnpe_main -m online --exact --refine sets --delta-vertices on the golden test graph, q1 and q2: the answer line carries the
    host form's DeltaV on the label/degree bitmap (the exact filter's sets are complete) in the four modes, for S = 12 random
    vertices and three vertices that take part in a match (from host_refine_sets_vertex_counts; seed 3700), written with a repeat;
    with --matches the file holds DeltaV pairwise different rows with an image in S"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    rng = np.random.default_rng(3700)
    used = np.nonzero(binding.host_refine_sets_vertex_counts(test_graph, qp, ld)[2].sum(axis=0))[0]
    S = np.unique(np.concatenate([rng.choice(n, 12, replace=False), used[rng.choice(len(used), 3, replace=False)]]))
    vf = str(tmp_path / "vertices.txt")
    open(vf, "w").write("".join(f"{v}\n" for v in S.tolist() + S[:1].tolist()))
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--delta-vertices", vf]
    for k, (distinct, induced) in enumerate(MODES):
        want = binding.host_refine_sets_delta_vertices(test_graph, qp, ld, S, FULL, distinct=distinct, induced=induced)
        assert 0 < want < binding.host_refine_sets(test_graph, qp, ld, FULL, distinct=distinct, induced=induced)
        out = str(tmp_path / f"m{k}.txt")
        cmd = base + ["--matches", out] + (["--distinct"] if distinct else []) + (["--induced"] if induced else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        assert ans == want, (distinct, induced, ans, want)
        rows = np.loadtxt(out, dtype=np.int64, ndmin=2)
        assert len(rows) == want and len(np.unique(rows, axis=0)) == want and _hits(rows, S).all()
