"""Count tables of the matches through a set of data vertices (include/gnnpe_online.h): VV_m(C, S) and EV_m(C, S), the tables of
ABI 13 / 14 over the maps with at least one image in S, on the host (gnnpe_host_refine_sets_delta_vertices_vertex_counts /
_edge_counts), on the device (gnnpe_refine_sets_delta_vertices_vertex_counts / _edge_counts) and through `gnnpe_main
--delta-vertices F --delta-vertex-counts / --delta-edge-counts`.

The host forms are the unchanged backtracking with the S test and the cell increments at every find.  They are held to yardsticks
that are not new code: networkx's rows with an image in S tallied in numpy, the ABI 17 host tables over E(S), the ABI 13 / 14 host
tables for S = V, the count of gnnpe_host_refine_sets_delta_vertices, and the relabel and removal identities between two graphs.
The device forms start at S n C(u), once per query vertex, and charge every match to its lowest-numbered query vertex with an image
in S; they are held to the host forms, to the existing device tables over E(S), to the existing device tables for S = V, and to a
fresh engine after relabel batches and a removal.  The yardstick is never the new kernel; all comparisons are exact integers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_delta as dl
import test_refine_delta_counts as dc
import test_refine_delta_vertices as dv
import test_refine_edge_counts as re_
import test_refine_sets as rs
import test_refine_sets_shapes as sh
import test_refine_vertex_counts as rv
import test_set_vertex_labels as sv

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = dl.MODES
H1_V_SHAPES = dv.H1_V_SHAPES
HOST_FNS = ("host_refine_sets_delta_vertices_vertex_counts", "host_refine_sets_delta_vertices_edge_counts")
DEV_FNS = ("refine_sets_delta_vertices_vertex_counts", "refine_sets_delta_vertices_edge_counts")


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _host_tables(g, qp, bm, S, distinct=False, induced=False, limit=FULL):
    """(DeltaV, VV, EV) of the two host forms, both complete and agreeing on DeltaV"""
    from gnnpe_amd import binding
    a, done_v, v = binding.host_refine_sets_delta_vertices_vertex_counts(g, qp, bm, S, limit, distinct=distinct, induced=induced)
    b, done_e, e = binding.host_refine_sets_delta_vertices_edge_counts(g, qp, bm, S, limit, distinct=distinct, induced=induced)
    assert done_v and done_e and a == b
    assert v.dtype == e.dtype == np.uint64 and e.shape == (len(dc._qe(qp)), len(g["nbrs"])) and v.shape[1] == len(g["labels"])
    return a, v, e


def _device_tables(eng, qp, bm, S, distinct=False, induced=False):
    a, done_v, v, _ = eng.refine_sets_delta_vertices_vertex_counts(qp, bm, S, distinct=distinct, induced=induced)
    b, done_e, e, _ = eng.refine_sets_delta_vertices_edge_counts(qp, bm, S, distinct=distinct, induced=induced)
    assert done_v and done_e and a == b
    return a, v, e


_same = dc._same
_H1VT = {}


def _h1_vertex_tables(tmp_path_factory):
    """the host forms' (DeltaV, VV, EV) of H1_V_SHAPES on the three bitmaps in the four modes with the S of dv._h1_vertices, computed
    once; DeltaV is the one gnnpe_host_refine_sets_delta_vertices gave"""
    if _H1VT:
        return _H1VT
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    for name in H1_V_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                t = _host_tables(h["g"], h["q"][name], h["bm"][name][b], f["S"], distinct, induced)
                assert t[0] == f["want"][name, b, distinct, induced]
                _H1VT[name, b, distinct, induced] = t
    return _H1VT


def _fuzz_set(seed, n):
    """S of fuzz case `seed`: 1 + seed mod 40 vertices (all of them where the graph has fewer), drawn with the seed"""
    return np.sort(np.random.default_rng(3800 + seed).choice(n, min(n, 1 + seed % 40), replace=False))


@pytest.fixture()
def vertices_count_lines(monkeypatch, capfd):
    """as dc.delta_count_lines, for the `[refine_delta_vertices_vcount]` and `[refine_delta_vertices_ecount]` lines"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [(ln.split()[0], {k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])})
                for ln in err.splitlines() if ln.startswith(("[refine_delta_vertices_vcount] ", "[refine_delta_vertices_ecount] "))]
    return take


# ---- CPU: the host forms against what is not new code --------------------------------------------------------------------------

def test_binding_declares_the_four_calls():
    """the four entries are declared in the binding, exported by libgnnpe_online.so and wrapped"""
    from gnnpe_amd import binding
    online = binding.load_online()
    for name in ("gnnpe_host_refine_sets_delta_vertices_vertex_counts", "gnnpe_host_refine_sets_delta_vertices_edge_counts",
                 "gnnpe_refine_sets_delta_vertices_vertex_counts", "gnnpe_refine_sets_delta_vertices_edge_counts"):
        assert name in binding.ONLINE_SIGNATURES and hasattr(online, name), name
    assert all(hasattr(binding, f) for f in HOST_FNS) and all(hasattr(binding.Engine, f) for f in DEV_FNS)


def test_host_forms_against_networkx(tmp_path_factory):
    """1. the dense cases of test_refine_delta_vertices (three G(n, m) graphs of 12, 16 and 20 vertices, the eight shapes of
    sh.NX_SHAPES, both label variants), the label/degree and the thinned bitmap, the four modes, S = one vertex, three vertices, a
    third of the vertices, all of them (seeds 3200 + gi): both tables are networkx's rows of the mode with an image in S tallied in
    numpy; for nq >= 2 they are the ABI 17 host tables over E(S); S = V gives the ABI 13 / 14 host tables; every row sums to
    host_refine_sets_delta_vertices; EV row k summed over data row x is VV[a_k][x].  At least a fifth of the cases have a match
    through S and a tenth one that avoids it"""
    from gnnpe_amd import binding
    cases = dv._dense_cases(tmp_path_factory)
    assert len(cases) == 3 * len(sh.NX_SHAPES) * 2
    some = part = total = 0
    for c in cases:
        g, n, qp = c["g"], c["g"]["n"], c["qp"]
        nq = sh.SHAPES[c["name"]][0]
        qe = re_._edges_of(c["name"])  # (the shape's own list, not the library's)
        src = re_._csr_keys(g)[0]
        rng = np.random.default_rng(3200 + c["gi"])
        sets = dict(one=rng.choice(n, 1), three=rng.choice(n, 3, replace=False), third=rng.choice(n, n // 3, replace=False), all=np.arange(n))
        for b in ("ld", "thin"):
            for distinct, induced in MODES:
                kw = dict(distinct=distinct, induced=induced)
                rows = dv._mode_rows(c, b, distinct, induced)
                where = (c["gi"], c["name"], c["variant"], b, distinct, induced)
                for form, S in sets.items():
                    keep = rows[dv._hits(rows, S)]
                    got = _host_tables(g, qp, c[b], S, distinct, induced)
                    _same(got, (len(keep), rv._table(keep, nq, n), re_._table(g, keep, qe)), where + (form,))
                    assert got[0] == binding.host_refine_sets_delta_vertices(g, qp, c[b], S, FULL, **kw), where
                    assert (got[1].sum(axis=1) == got[0]).all() and (got[2].sum(axis=1) == got[0]).all(), where
                    for k, (a, _) in enumerate(qe):
                        assert np.array_equal(np.bincount(src, got[2][k].astype(np.int64), n).astype(np.uint64), got[1][a]), where + (k,)
                    if nq >= 2:
                        _same(got, dc._host_tables(g, qp, c[b], dv._edges_at(g, S), distinct, induced), where + (form, "E(S)"))
                    total += 1
                    some += len(keep) > 0
                    part += 0 < len(keep) < len(rows)
                full = _host_tables(g, qp, c[b], sets["all"], distinct, induced)
                assert np.array_equal(full[1], binding.host_refine_sets_vertex_counts(g, qp, c[b], FULL, **kw)[2]), where
                assert np.array_equal(full[2], binding.host_refine_sets_edge_counts(g, qp, c[b], FULL, **kw)[2]), where
    assert some * 5 >= total and part * 10 >= total, (some, part, total)


def test_host_relabel_and_removal_identities(tmp_path_factory):
    """2. between two host graphs, the four modes, both tables, the inputs of dv.test_host_vertex_removal_and_relabel_identities
    (seeds 3300 + gi and 3400 + gi, labels-only bitmaps).  RELABEL: V(G', C') == V(G, C) - VV(G, C, S) + VV(G', C', S) and the same
    for E with the same entry indices.  REMOVAL, nq >= 2: V(G - E(S)) == V(G) - VV(G, S), and E by the key (x, y) of an entry.  Over
    the run the relabel loses matches and gains matches in at least ten cases each"""
    from gnnpe_amd import binding
    lost_n = gained_n = 0
    for c in dv._dense_cases(tmp_path_factory):
        g, n, qp = c["g"], c["g"]["n"], c["qp"]
        S = np.sort(np.random.default_rng(3300 + c["gi"]).choice(n, max(2, n // 6), replace=False))
        g_cut = dl._without(g, dv._edges_at(g, S))
        g_new, _ = dv._relabelled(g, S, 3400 + c["gi"], 2)
        bm, bm_new = dl._label_bitmap(g, qp), dl._label_bitmap(g_new, qp)
        for distinct, induced in MODES:
            kw = dict(distinct=distinct, induced=induced)
            where = (c["gi"], c["name"], c["variant"], distinct, induced)
            v = binding.host_refine_sets_vertex_counts(g, qp, bm, FULL, **kw)[2]
            e = binding.host_refine_sets_edge_counts(g, qp, bm, FULL, **kw)[2]
            lost, lv, le = _host_tables(g, qp, bm, S, distinct, induced)
            if sh.SHAPES[c["name"]][0] >= 2:
                assert np.array_equal(binding.host_refine_sets_vertex_counts(g_cut, qp, bm, FULL, **kw)[2], v - lv), where
                assert np.array_equal(binding.host_refine_sets_edge_counts(g_cut, qp, bm, FULL, **kw)[2], dc._carry(g, g_cut, e - le)), where
            gained, gv, ge = _host_tables(g_new, qp, bm_new, S, distinct, induced)
            assert np.array_equal(binding.host_refine_sets_vertex_counts(g_new, qp, bm_new, FULL, **kw)[2], v - lv + gv), where
            assert np.array_equal(binding.host_refine_sets_edge_counts(g_new, qp, bm_new, FULL, **kw)[2], e - le + ge), where
            lost_n += lost > 0
            gained_n += gained > 0
    assert lost_n >= 10 and gained_n >= 10, (lost_n, gained_n)


def test_host_guard_and_refusals(tmp_path_factory, tmp_path):
    """3. guard: limit = DeltaV gives complete 0; DeltaV + 1 complete 1 and the exact table; limit 1; limit 0: (0, 0); an empty S:
    zeros and complete 1 -- wedge and K4 on H1 in the four modes, both tables.  Refusals: an id >= n, unknown mode bits, a
    disconnected query, a null list with a count and a null `complete` return GNNPE_ERR_ARG with *answers == 0; the caller's counts
    are untouched but by the disconnected query, whose refusal comes from the walk after the zeroing, as in ABI 17"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    g, S = h["g"], f["S"]
    for name in ("wedge", "K4"):
        qp, bm = h["q"][name], h["bm"][name]["ld"]
        for distinct, induced in MODES:
            kw = dict(distinct=distinct, induced=induced)
            d, v, e = _host_tables(g, qp, bm, S, distinct, induced)
            assert d == f["want"][name, "ld", distinct, induced] > 2
            for k, fn in enumerate(getattr(binding, x) for x in HOST_FNS):
                want = (v, e)[k]
                for limit in (1, d - 1, d):
                    assert fn(g, qp, bm, S, limit, **kw)[:2] == (limit, False), (name, limit)
                got = fn(g, qp, bm, S, d + 1, **kw)
                assert got[:2] == (d, True) and np.array_equal(got[2], want)
                assert fn(g, qp, bm, S, 0, **kw)[:2] == (0, False)
                got = fn(g, qp, bm, [], FULL, **kw)
                assert got[:2] == (0, True) and got[2].shape == want.shape and not got[2].any()
    qp, bm = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    online, u32p, u64p = binding.load_online(), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    rng = np.random.default_rng(3900)
    for fn, cells in ((online.gnnpe_host_refine_sets_delta_vertices_vertex_counts, 3 * g["n"]),
                      (online.gnnpe_host_refine_sets_delta_vertices_edge_counts, 3 * len(nb))):
        old = rng.integers(1, 1 << 64, cells, dtype=np.uint64)

        def raw(ids, cnt, mode=0, query=qp, bitmap=bmc, complete=True, limit=FULL):
            s = None if ids is None else np.ascontiguousarray(ids, np.uint32)
            out, done, table = C.c_uint64(12345), C.c_int(7), old.copy()
            rc = fn(g["n"], o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), lb.ctypes.data_as(u32p), query.encode(),
                    bitmap.ctypes.data_as(u32p), None if s is None else s.ctypes.data_as(u32p), cnt, limit, mode, C.byref(out),
                    C.byref(done) if complete else None, table.ctypes.data_as(u64p))
            return rc, out.value, done.value if complete else None, np.array_equal(table, old)
        ok = raw(S, len(S))
        assert ok[:3] == (0, f["want"]["triangle", "ld", False, False], 1) and not ok[3]
        for bad in (g["n"], g["n"] + 7, 0xFFFFFFFF):
            for limit in (FULL, 0):
                assert raw(S.tolist() + [bad], len(S) + 1, limit=limit) == (-1, 0, 0, True), bad
                assert b"does not have" in binding.load().gnnpe_last_error()
        for mode in (4, 7, 1 << 31):
            assert raw(S, len(S), mode=mode) == (-1, 0, 0, True) and b"unknown mode" in binding.load().gnnpe_last_error()
        assert raw(None, 3) == (-1, 0, 0, True) and b"null argument" in binding.load().gnnpe_last_error()
        assert raw(S, len(S), complete=False) == (-1, 0, None, True) and b"null argument" in binding.load().gnnpe_last_error()
        ones2 = np.ascontiguousarray(sh._ones(2, g["n"]), np.uint32)
        for limit in (FULL, 0):
            assert raw(S, len(S), query=disc, bitmap=ones2, limit=limit)[:3] == (-1, 0, 0)
            assert b"not connected" in binding.load().gnnpe_last_error()
    for name in HOST_FNS:
        with pytest.raises(binding.GnnpeError, match="does not have"):
            getattr(binding, name)(g, qp, bm, [3, g["n"]])


def test_cli_refusals(tmp_path):
    """4. the two table flags with --delta-vertices: without --refine sets, together, with --matches, with --vertex-counts /
    --edge-counts / --all-matches / --delta-edges / --delta-nonedges, and a table flag without an anchor exit 1 with their message
    before a GPU is touched and leave no output file; gnnpge_main keeps refusing --delta-vertices"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    vf, ef = str(tmp_path / "v.txt"), str(tmp_path / "e.txt")
    open(vf, "w").write("0\n5\n")
    open(ef, "w").write("0 1\n")
    m, m2 = str(tmp_path / "m.txt"), str(tmp_path / "m2.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    sets = ["--refine", "sets", "--delta-vertices", vf]
    for flag in ("--delta-vertex-counts", "--delta-edge-counts"):
        for extra, msg in ((["--delta-vertices", vf, flag, m], "--delta-vertices needs --refine sets"),
                           (["--refine", "sets", flag, m], flag + " needs --delta-edges FILE or --delta-nonedges FILE"),
                           (["--refine", "sets", flag, m], "--delta-vertices FILE"),
                           (sets + [flag, m, "--matches", m2], flag + " and --matches exclude each other"),
                           (sets + ["--delta-vertex-counts", m, "--delta-edge-counts", m2],
                            "--delta-vertex-counts and --delta-edge-counts exclude each other"),
                           (sets + [flag, m, "--vertex-counts", m2], "--delta-vertices excludes"),
                           (sets + [flag, m, "--edge-counts", m2], "--delta-vertices excludes"),
                           (sets + [flag, m, "--matches", m2, "--all-matches"], "--delta-vertices excludes"),
                           (sets + [flag, m, "--delta-edges", ef], "--delta-vertices excludes"),
                           (sets + [flag, m, "--induced", "--delta-nonedges", ef], "--delta-vertices excludes")):
            r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
            assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra
            assert not os.path.exists(m) and not os.path.exists(m2), extra
    r = subprocess.run([os.path.join(os.path.dirname(CLI), "gnnpge_main"), "-f", root, "-d", graph, "-q", q, "-m", "online", "--delta-vertices", vf,
                        "--delta-vertex-counts", m], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--delta-vertices is an option of gnnpe_main" in r.stderr and not os.path.exists(m)


def test_fuzz_sets_are_telling(tmp_path_factory):
    """9 (CPU half). of the 24 fuzz cases with S = _fuzz_set at least 8 have a match through S"""
    from gnnpe_amd import binding
    hit = 0
    for seed in sh.FUZZ_SEEDS:
        c = sh._fuzz_case(seed, tmp_path_factory)
        hit += binding.host_refine_sets_delta_vertices(c["g"], c["qp"], c["bm"], _fuzz_set(seed, c["g"]["n"]), FULL) > 0
    assert hit >= 8, hit


# ---- GPU: the device forms against the host forms and the existing device calls ----------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", H1_V_SHAPES)
def test_gpu_h1_equals_the_host_forms(tmp_path_factory, name):
    """5. H1 (2000 vertices, 11 386 entries, the longest row 155) with the S of dv._h1_vertices (the hub, a leaf, an isolated vertex,
    an adjacent pair, a triangle, vertex n - 1, 50 random vertices), the three bitmaps, the four modes: both device tables equal the
    host forms'; for nq >= 2 they also equal the existing device tables over E(S)"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    tabs = _h1_vertex_tables(tmp_path_factory)
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                qp, bm = h["q"][name], h["bm"][name][b]
                got = _device_tables(eng, qp, bm, f["S"], distinct, induced)
                _same(got, tabs[name, b, distinct, induced], (name, b, distinct, induced))
                if sh.SHAPES[name][0] >= 2:
                    _same(got, dc._device_tables(eng, qp, bm, f["E"], distinct, induced), (name, b, distinct, induced, "E(S)"))
    finally:
        eng.close()
    assert tabs["K4", "ld", False, False][0] > 1024  # past the flush of a wave's finds


_HUB = {}


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [None, 0, 1, 2, 3, 4, 5, 6])
def test_gpu_items_that_share_a_start_candidate(tmp_path_factory, monkeypatch, vertices_count_lines, shift):
    """6. the hub alone and the hub with its neighbours as S, under triangle, diamond and K4 in the four modes, with
    GNNPE_TESTING=sets_first_shift=K for K = 0 .. 6 and with the heuristic: the hub's row of 155 entries is cut into 155 .. 3
    first-level items that all add to the cell of the hub.  The tables are the host forms', hence identical across K (they are also
    compared with the first K that ran)"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, deg = h["g"], h["deg"]
    hub = int(np.argmax(deg))
    o = g["offsets"].astype(np.int64)
    assert deg[hub] == 155
    sets = dict(hub=np.array([hub]), star=np.concatenate([[hub], g["nbrs"][o[hub]:o[hub + 1]]]).astype(np.int64))
    if shift is not None:
        monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    vertices_count_lines()
    try:
        for name in ("triangle", "diamond", "K4"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            for form, S in sets.items():
                for distinct, induced in MODES:
                    key = (name, form, distinct, induced)
                    if key not in _HUB:
                        _HUB[key] = _host_tables(g, qp, bm, S, distinct, induced)
                        assert _HUB[key][0] > 0
                    _same(_device_tables(eng, qp, bm, S, distinct, induced), _HUB[key], (shift,) + key)
    finally:
        eng.close()
    staged = [ln for _, ln in vertices_count_lines() if "shift" in ln]
    assert len(staged) == 3 * 2 * 4 * 2 and all(ln["accum"] == 0 and ln["sign"] == 1 and ln["launches"] >= 1 for ln in staged)
    if shift is not None:
        assert all(ln["shift"] == shift for ln in staged), staged[:2]


@pytest.mark.gpu
def test_gpu_all_vertices_gives_the_existing_device_tables(tmp_path_factory):
    """7. S = V on H1: both tables are Engine.refine_sets_vertex_counts' / _edge_counts' in the four modes, for every shape of
    H1_V_SHAPES on the label/degree and the thinned bitmap.  A match charged twice or dropped shows here"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    V = np.arange(g["n"])
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in H1_V_SHAPES:
            for b in ("ld", "thin"):
                for distinct, induced in MODES:
                    qp, bm = h["q"][name], h["bm"][name][b]
                    kw = dict(distinct=distinct, induced=induced)
                    a, done_v, v, _ = eng.refine_sets_vertex_counts(qp, bm, **kw)
                    a2, done_e, e, _ = eng.refine_sets_edge_counts(qp, bm, **kw)
                    assert done_v and done_e and a == a2
                    _same(_device_tables(eng, qp, bm, V, distinct, induced), (a, v, e), (name, b, distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_small_graphs_equal_the_host_forms(tmp_path_factory, gi):
    """8. the 15 small graphs of sh._nx_cases with the eight shapes of sh.NX_SHAPES (C5 and star5 among them: orders anchored at
    every vertex of a cycle and at the leaves of a star), both label variants, the label/degree and the thinned bitmap, the four
    modes, S a third of the vertices (seed 3700 + gi): both device tables equal the host forms'"""
    from gnnpe_amd import binding, synth
    cases = [c for c in sh._nx_cases(tmp_path_factory) if c["gi"] == gi]
    assert len(cases) == len(sh.NX_SHAPES) * 2
    g = cases[0]["g"]
    S = np.sort(np.random.default_rng(3700 + gi).choice(g["n"], g["n"] // 3, replace=False))
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            for b in ("ld", "thin"):
                for distinct, induced in MODES:
                    _same(_device_tables(eng, c["qp"], c[b], S, distinct, induced), _host_tables(g, c["qp"], c[b], S, distinct, induced),
                          (gi, c["name"], c["variant"], b, distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_forms(tmp_path_factory, seed):
    """9. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of bitmap) in
    the four modes, S = _fuzz_set: both device tables equal the host forms' (test_fuzz_sets_are_telling: at least 8 have a match)"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    S = _fuzz_set(seed, g["n"])
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for distinct, induced in MODES:
            _same(_device_tables(eng, c["qp"], c["bm"], S, distinct, induced), _host_tables(g, c["qp"], c["bm"], S, distinct, induced),
                  (seed, c["which"], len(S), distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_single_vertex_query(tmp_path_factory):
    """10. nq == 1 on H1, the three bitmaps: VV is the indicator of S n C(0); the edge call returns DeltaV, no table and
    *dev_counts == NULL; with dev_accum and sign -1 the cells of S n C(0) go to old - 1 mod 2^64 and no other cell moves"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    g, S, qp = h["g"], f["S"], h["q"]["vertex"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            bm = h["bm"]["vertex"][b]
            inside = np.intersect1d(S, sh._members(bm[0], g["n"]))
            want = np.zeros((1, g["n"]), np.uint64)
            want[0, inside] = 1
            assert 0 < len(inside) and (b != "thin" or len(inside) < len(S))
            for distinct, induced in MODES:
                kw = dict(distinct=distinct, induced=induced)
                d, hv, he = _host_tables(g, qp, bm, S, distinct, induced)
                assert d == len(inside) and np.array_equal(hv, want) and he.shape == (0, len(g["nbrs"]))
                got, done, v, _ = eng.refine_sets_delta_vertices_vertex_counts(qp, bm, S, **kw)
                assert (got, done) == (d, True) and np.array_equal(v, want), (b, distinct, induced)
                got, done, e, _ = eng.refine_sets_delta_vertices_edge_counts(qp, bm, S, **kw)
                assert (got, done) == (d, True) and e.shape == (0, len(g["nbrs"]))
                got, done, view, _ = eng.refine_sets_delta_vertices_edge_counts(qp, bm, S, device=True, **kw)
                assert (got, done) == (d, True) and view.__cuda_array_interface__["data"][0] == 0
            old = np.random.default_rng(3950).integers(0, 1 << 64, (1, g["n"]), dtype=np.uint64)
            old[0, inside[0]] = 0  # (this cell wraps to 2^64 - 1)
            t = dc._to_device(old)
            got, done, _, _ = eng.refine_sets_delta_vertices_vertex_counts(qp, bm, S, accum=t.data_ptr(), sign=-1)
            assert (got, done) == (len(inside), True) and np.array_equal(dc._to_host(t), old - want)
            assert dc._to_host(t)[0, inside[0]] == FULL
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_tables_maintained_across_relabels_and_a_removal(tmp_path):
    """11. H1 with the four labels its generator draws; triangle and diamond with mixed and with single query labels; the four modes.
    A vertex table and an edge table per (query, mode) live in caller memory.  Four batches, each relabelling 30 random vertices
    (seeds 4000 + batch): -tables of Sset(G, C, S), set_vertex_labels, +tables of Sset(G', C', S), C and C' the label bitmaps of
    the two graphs; after each batch every table equals that of a fresh context loaded with the new labels.  Then one removal:
    -tables of Sset(G, C, S) for 30 more vertices, apply_edges_map(delete=E(S)), carry_entries; the tables equal the fresh context's
    on G - E(S).  Over the run the batches lose and gain matches"""
    from gnnpe_amd import binding, synth
    import torch
    g, _ = sv._h1_four_labels()
    n, sn = g["n"], synth.degree_order(g["offsets"])
    queries = sv._mixed_queries(tmp_path)
    keys = [(qp, distinct, induced) for qp in queries for distinct, induced in MODES]
    eng, fresh = ex._engine(binding, g, sn, 2), ex._engine(binding, g, sn, 2)
    try:
        tv, te = {}, {}
        for qp, distinct, induced in keys:
            bm = dl._label_bitmap(g, qp)
            tv[qp, distinct, induced] = dc._to_device(eng.refine_sets_vertex_counts(qp, bm, distinct=distinct, induced=induced)[2])
            te[qp, distinct, induced] = dc._to_device(eng.refine_sets_edge_counts(qp, bm, distinct=distinct, induced=induced)[2])

        def add(gr, S, sign):
            moved = 0
            for qp, distinct, induced in keys:
                bm = dl._label_bitmap(gr, qp)
                kw = dict(distinct=distinct, induced=induced, sign=sign)
                a, done, view, _ = eng.refine_sets_delta_vertices_vertex_counts(qp, bm, S, accum=tv[qp, distinct, induced].data_ptr(), **kw)
                assert done and view.__cuda_array_interface__["data"][0] == tv[qp, distinct, induced].data_ptr()
                b, done, _, _ = eng.refine_sets_delta_vertices_edge_counts(qp, bm, S, accum=te[qp, distinct, induced].data_ptr(), **kw)
                assert done and a == b
                moved += a > 0
            return moved

        def check(gr, what):
            for qp, distinct, induced in keys:
                bm = dl._label_bitmap(gr, qp)
                kw = dict(distinct=distinct, induced=induced)
                assert np.array_equal(dc._to_host(tv[qp, distinct, induced]), fresh.refine_sets_vertex_counts(qp, bm, **kw)[2]), (what, qp, kw, "vertex table")
                assert np.array_equal(dc._to_host(te[qp, distinct, induced]), fresh.refine_sets_edge_counts(qp, bm, **kw)[2]), (what, qp, kw, "edge table")

        lost = gained = 0
        for batch in range(4):
            S = np.sort(np.random.default_rng(4000 + batch).choice(n, 30, replace=False))
            g_new, new = dv._relabelled(g, S, 4100 + batch, 4)
            lost += add(g, S, -1)
            eng.set_vertex_labels(S, new)
            gained += add(g_new, S, 1)
            fresh.load_csr(g_new["offsets"], g_new["nbrs"], g_new["labels"])
            check(g_new, batch)
            g = g_new
        assert lost >= 8 and gained >= 8, (lost, gained)
        # the removal of E(S): the vertices of S end isolated
        S = np.sort(np.random.default_rng(4200).choice(np.nonzero(np.diff(g["offsets"].astype(np.int64)) >= 2)[0], 30, replace=False))
        ES = dv._edges_at(g, S)
        g_cut = dl._without(g, ES)
        assert add(g, S, -1) >= 4
        before, after, _ = eng.apply_edges_map(delete=ES)
        assert (before, after) == (len(g["nbrs"]), len(g_cut["nbrs"]))
        for key in keys:
            dst = torch.zeros((te[key].shape[0], after), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()  # torch fills on its own stream, the context carries on its own
            eng.carry_entries(te[key], dst, te[key].shape[0])
            te[key] = dst
        fresh.load_csr(g_cut["offsets"], g_cut["nbrs"], g_cut["labels"])
        check(g_cut, "removal")
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_gpu_plus_then_minus_restores_the_bytes(tmp_path_factory):
    """12. the four modes, diamond and triangle on H1 with the S of dv._h1_vertices: a caller's table of random 64-bit words, +1 then
    -1 with the same S, is byte for byte what it was; after the +1 it is old + table mod 2^64"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    tabs = _h1_vertex_tables(tmp_path_factory)
    rng = np.random.default_rng(4300)
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for name in ("diamond", "triangle"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            for distinct, induced in MODES:
                d, v, e = tabs[name, "ld", distinct, induced]
                for fn, table in zip((getattr(eng, x) for x in DEV_FNS), (v, e)):
                    old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
                    t = dc._to_device(old)
                    assert fn(qp, bm, f["S"], distinct=distinct, induced=induced, accum=t.data_ptr(), sign=1)[:2] == (d, True)
                    assert np.array_equal(dc._to_host(t), old + table), (name, distinct, induced)
                    assert fn(qp, bm, f["S"], distinct=distinct, induced=induced, accum=t.data_ptr(), sign=-1)[:2] == (d, True)
                    assert dc._to_host(t).tobytes() == old.tobytes(), (name, distinct, induced)
    finally:
        eng.close()


def _raw_device(binding, eng, kind, qp, bm, vertices, host_counts=None, accum=None, sign=1, limit=FULL, mode=0):
    """a device form through ctypes: (return code, *answers, *complete); both are set to canaries first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    s = np.ascontiguousarray(np.asarray(vertices, np.int64).reshape(-1), np.uint32)
    out, done, ms, ptr = C.c_uint64(12345), C.c_int(7), C.c_double(), C.c_void_p()
    fn = getattr(binding.load_online(), f"gnnpe_refine_sets_delta_vertices_{kind}_counts")
    rc = fn(eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), s.ctypes.data_as(u32p), len(s), limit, mode, C.byref(out), C.byref(done),
            None if host_counts is None else host_counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ptr),
            None if accum is None else C.c_void_p(accum), sign, C.byref(ms))
    return rc, out.value, done.value


@pytest.mark.gpu
def test_gpu_guard_and_refusals(tmp_path_factory, vertices_count_lines):
    """13. K4 and the wedge on H1 with the S of dv._h1_vertices, the four modes, both tables; K4 in mode 0 is far past the 1 024-find
    flush.  limit = 1, DeltaV - 1 and DeltaV: complete 0, answers == limit and nothing copied (the host table keeps its zeros);
    DeltaV + 1: complete 1 and the exact table; limit 0: (0, 0); a limit of 1 with K4 gives answers 1; an empty S and a set outside
    every C(u): zeros, complete 1, a caller's table untouched.  Under GNNPE_DEBUG=1 the line after the wait carries finds and
    flush_adds.  A refused call in accumulate mode -- an id == n, a bad sign, host_counts with dev_accum, unknown mode bits -- leaves
    a caller's random words untouched and the context usable"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    tabs = _h1_vertex_tables(tmp_path_factory)
    g, S = h["g"], f["S"]
    rng = np.random.default_rng(4400)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("K4", "wedge"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            for distinct, induced in MODES:
                kw = dict(distinct=distinct, induced=induced)
                d, v, e = tabs[name, "ld", distinct, induced]
                assert d > 2
                for k, fn in enumerate(getattr(eng, x) for x in DEV_FNS):
                    for limit in (1, d - 1, d):
                        got = fn(qp, bm, S, limit=limit, **kw)
                        assert got[:2] == (limit, False) and not got[2].any(), (name, distinct, induced, k, limit, got[:2])
                    got = fn(qp, bm, S, limit=d + 1, **kw)
                    assert got[:2] == (d, True) and np.array_equal(got[2], (v, e)[k]), (name, distinct, induced, k)
                    assert fn(qp, bm, S, limit=0, **kw)[:2] == (0, False)
                    got = fn(qp, bm, [], **kw)
                    assert got[:2] == (0, True) and got[2].shape == (v, e)[k].shape and not got[2].any() and got[3] == 0.0
        vertices_count_lines()
        qp, bm = h["q"]["K4"], h["bm"]["K4"]["ld"]
        d, v, e = tabs["K4", "ld", False, False]
        assert d > 1024
        for x in DEV_FNS:
            getattr(eng, x)(qp, bm, S)
        done = [(tag, ln) for tag, ln in vertices_count_lines() if "finds" in ln]
        assert [tag for tag, _ in done] == ["[refine_delta_vertices_vcount]", "[refine_delta_vertices_ecount]"]
        for _, ln in done:
            assert ln["finds"] == d and ln["complete"] == 1 and 0 < ln["flush_adds"], ln
        assert done[0][1]["flush_adds"] <= 3 * d  # at most one flush add per visited image above the leaf of a 4-vertex query
        # no vertex of S in any set: the thinned sets without S
        none = h["bm"]["K4"]["thin"].copy()
        for u in range(len(none)):
            np.bitwise_and.at(none[u], S >> 5, ~(np.uint32(1) << (S & 31).astype(np.uint32)))
        for kind, table in (("vertex", v), ("edge", e)):
            old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
            t = dc._to_device(old)
            for ids, bitmap in (([], bm), (S, none)):
                assert _raw_device(binding, eng, kind, qp, bitmap, ids, accum=t.data_ptr(), sign=-1) == (0, 0, 1)
                host = np.ones(table.shape, np.uint64)
                assert _raw_device(binding, eng, kind, qp, bitmap, ids, host_counts=host) == (0, 0, 1) and not host.any()
            for bad in (g["n"], g["n"] + 5, 0xFFFFFFFF):
                for sign in (1, -1):
                    for mode in (0, 1, 2, 3):
                        got = _raw_device(binding, eng, kind, qp, bm, S.tolist() + [bad], accum=t.data_ptr(), sign=sign, mode=mode)
                        assert got == (-1, 0, 0) and b"does not have" in binding.load().gnnpe_last_error(), (kind, bad, got)
            host = np.zeros(table.shape, np.uint64)
            for sign in (0, 2, -2, 3):
                assert _raw_device(binding, eng, kind, qp, bm, S, accum=t.data_ptr(), sign=sign) == (-1, 0, 0)
                assert b"sign" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, kind, qp, bm, S, sign=-1) == (-1, 0, 0) and b"sign" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, kind, qp, bm, S, host_counts=host, accum=t.data_ptr()) == (-1, 0, 0)
            assert b"host_counts" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, kind, qp, bm, S, accum=t.data_ptr(), mode=4) == (-1, 0, 0)
            assert dc._to_host(t).tobytes() == old.tobytes() and not host.any(), kind
            with pytest.raises(binding.GnnpeError, match="sign"):
                getattr(eng, f"refine_sets_delta_vertices_{kind}_counts")(qp, bm, S, sign=-1)
            # the context is usable: the next call is right, accumulating and into the host table
            assert _raw_device(binding, eng, kind, qp, bm, S, accum=t.data_ptr(), sign=1) == (0, d, 1)
            assert np.array_equal(dc._to_host(t), old + table), kind
            assert _raw_device(binding, eng, kind, qp, bm, S, host_counts=host) == (0, d, 1) and np.array_equal(host, table)
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == h["want"]["K4", "ld"]
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_views(tmp_path_factory):
    """14. the device=True views of refine_sets_vertex_counts (ABI 13), refine_sets_edge_counts (ABI 14), the tables over a set of
    edges (ABI 17) and over a set of non-edges (ABI 19) survive calls of the two new functions, with a context-owned table and
    accumulating, and the new views survive calls of those: the eight tables live in eight buffers.  A later call of the same new
    function replaces its view (the old one is refused as stale); after set_vertex_labels every view is refused"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dv._h1_vertices(tmp_path_factory)
    tabs = _h1_vertex_tables(tmp_path_factory)
    vt, et = rv._h1_tables(tmp_path_factory), re_._h1_tables(tmp_path_factory)
    g, S, E = h["g"], f["S"], f["E"]
    iso = np.nonzero(h["deg"] == 0)[0]
    non = np.array([[iso[0], iso[1]], [iso[2], iso[3]]], np.int64)  # two pairs that are no edges
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        qp, bm = h["q"]["diamond"], h["bm"]["diamond"]["ld"]
        _, _, view_v, _ = eng.refine_sets_vertex_counts(qp, bm, device=True)
        _, _, view_e, _ = eng.refine_sets_edge_counts(qp, bm, device=True)
        d17, _, view_dv, _ = eng.refine_sets_delta_vertex_counts(qp, bm, E, device=True)
        _, _, view_de, _ = eng.refine_sets_delta_edge_counts(qp, bm, E, device=True)
        _, _, view_nv, _ = eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, non, device=True)
        _, _, view_ne, _ = eng.refine_sets_delta_nonedges_edge_counts(qp, bm, non, device=True)
        d, v, e = tabs["diamond", "ld", False, False]
        assert d17 == d
        nv, ne = eng.delta_counts_to_host(view_nv), eng.delta_counts_to_host(view_ne)

        def old_views():
            got = eng.copy_to_host(view_v.__cuda_array_interface__["data"][0], 4 * g["n"] * 8).view(np.uint64).reshape(4, g["n"])
            assert np.array_equal(got, vt["diamond", "ld", False, False][1])
            assert np.array_equal(eng.edge_counts_to_host(view_e), et["diamond", "ld", False, False][1])
            # (for a connected query of two or more vertices the tables over E(S) are the tables through S)
            assert np.array_equal(eng.delta_counts_to_host(view_dv), v) and np.array_equal(eng.delta_counts_to_host(view_de), e)
            assert np.array_equal(eng.delta_counts_to_host(view_nv), nv) and np.array_equal(eng.delta_counts_to_host(view_ne), ne)
        old_views()
        got, done, vv, _ = eng.refine_sets_delta_vertices_vertex_counts(qp, bm, S, device=True)
        assert (got, done) == (d, True) and vv.shape == v.shape and vv.__cuda_array_interface__["typestr"] == "<i8"
        got, done, ev, _ = eng.refine_sets_delta_vertices_edge_counts(qp, bm, S, device=True)
        assert (got, done) == (d, True) and ev.shape == e.shape
        ptrs = {x.__cuda_array_interface__["data"][0] for x in (view_v, view_e, view_dv, view_de, view_nv, view_ne, vv, ev)}
        assert len(ptrs) == 8 and 0 not in ptrs
        old_views()
        assert np.array_equal(eng.delta_counts_to_host(vv), v) and np.array_equal(eng.delta_counts_to_host(ev), e)
        t = dc._to_device(np.zeros(v.shape, np.uint64))
        eng.refine_sets_delta_vertices_vertex_counts(qp, bm, S, accum=t.data_ptr(), sign=1)
        old_views()
        assert np.array_equal(eng.delta_counts_to_host(vv), v) and np.array_equal(dc._to_host(t), v)  # accumulating leaves the context's own
        # the new views survive calls of the existing functions
        eng.refine_sets_vertex_counts(h["q"]["triangle"], h["bm"]["triangle"]["ld"], device=True)
        eng.refine_sets_delta_vertex_counts(h["q"]["triangle"], h["bm"]["triangle"]["ld"], E, device=True)
        eng.refine_sets_delta_edge_counts(h["q"]["triangle"], h["bm"]["triangle"]["ld"], E, device=True)
        eng.refine_sets_delta_nonedges_vertex_counts(h["q"]["wedge"], h["bm"]["wedge"]["ld"], non, device=True)
        eng.refine_sets_delta_nonedges_edge_counts(h["q"]["wedge"], h["bm"]["wedge"]["ld"], non, device=True)
        assert np.array_equal(eng.delta_counts_to_host(vv), v) and np.array_equal(eng.delta_counts_to_host(ev), e)
        d3, v3, _ = tabs["triangle", "thin", True, False]
        got, done, vv3, _ = eng.refine_sets_delta_vertices_vertex_counts(h["q"]["triangle"], h["bm"]["triangle"]["thin"], S, distinct=True, device=True)
        assert (got, done) == (d3, True) and np.array_equal(eng.delta_counts_to_host(vv3), v3)
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.delta_counts_to_host(vv)
        assert np.array_equal(eng.delta_counts_to_host(ev), e)
        eng.set_vertex_labels([5], [0])
        for view in (vv3, ev):
            with pytest.raises(binding.GnnpeError, match="stale"):
                eng.delta_counts_to_host(view)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", ["q1", "q2"])
def test_gpu_cli_delta_vertices_count_tables(tmp_path, test_graph, q):
    """15. gnnpe_main -m online --exact --refine sets --delta-vertices S --delta-vertex-counts / --delta-edge-counts on the golden test
    graph, q1 and q2, modes 0 and DISTINCT + INDUCED: the files, in the formats of --vertex-counts and --edge-counts, hold the host
    forms' tables on the label/degree bitmap (the exact filter's sets are complete) and the answer line their DeltaV; with -n at
    DeltaV the guard is reached: non-zero exit, the message names -n, no file"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    n = len(test_graph["labels"])
    ld = ex._ld_bitmap(test_graph, qp)
    rng = np.random.default_rng(3700)
    used = np.nonzero(binding.host_refine_sets_vertex_counts(test_graph, qp, ld)[2].sum(axis=0))[0]
    S = np.unique(np.concatenate([rng.choice(n, 12, replace=False), used[rng.choice(len(used), 3, replace=False)]]))
    vf = str(tmp_path / "vertices.txt")
    open(vf, "w").write("".join(f"{v}\n" for v in S.tolist() + S[:1].tolist()))
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--delta-vertices", vf]
    qe = dc._qe(qp)
    keys = re_._csr_keys(test_graph)[1]

    def run(extra, out):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        rows = [[int(x) for x in ln.split()] for ln in open(out) if not ln.startswith("#")]
        return ans, np.array(rows, np.uint64).reshape(len(rows), -1)

    total = 0
    for k, (distinct, induced) in enumerate(((False, False), (True, True))):
        d, v, e = _host_tables(test_graph, qp, ld, S, distinct, induced)
        mode = (["--distinct"] if distinct else []) + (["--induced"] if induced else [])
        out = str(tmp_path / f"v{k}.txt")
        ans, lines = run(mode + ["--delta-vertex-counts", out], out)
        got = np.zeros_like(v)
        if len(lines):
            assert lines.shape[1] == v.shape[0] + 1 and (np.diff(lines[:, 0].astype(np.int64)) > 0).all() and (lines[:, 1:] != 0).any(axis=1).all()
            got[:, lines[:, 0].astype(np.int64)] = lines[:, 1:].T
        assert ans == d and np.array_equal(got, v), (k, "vertex table")
        out = str(tmp_path / f"e{k}.txt")
        ans, lines = run(mode + ["--delta-edge-counts", out], out)
        head = open(out).readline().split()
        assert head[0] == "#" and [tuple(map(int, x.split("-"))) for x in head[1:]] == qe
        got = np.zeros_like(e)
        if len(lines):
            code = lines[:, 0].astype(np.int64) * n + lines[:, 1].astype(np.int64)
            j = np.searchsorted(keys, code)
            assert lines.shape[1] == len(qe) + 2 and (np.diff(code) > 0).all() and np.array_equal(keys[j], code)
            got[:, j] = lines[:, 2:].T
        assert ans == d and np.array_equal(got, e), (k, "edge table")
        total += d
    assert total > 0
    d = _host_tables(test_graph, qp, ld, S)[0]
    for flag in ("--delta-vertex-counts", "--delta-edge-counts"):
        out = str(tmp_path / "guard.txt")
        r = subprocess.run(base + [flag, out, "-n", str(d)], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "-n" in r.stderr and flag in r.stderr and not os.path.exists(out), (r.returncode, r.stderr)
