"""Count tables of the matches through a set of data edges (include/gnnpe_online.h, ABI version 17): VDelta_m(C, F)[u][v] and
EDelta_m(C, F)[k][j], the tables of ABI 13 and 14 over the maps Delta_m(C, F) counts only -- on the host
(gnnpe_host_refine_sets_delta_vertex_counts / _edge_counts), on the device (gnnpe_refine_sets_delta_vertex_counts / _edge_counts,
with a context-owned table or accumulating with a sign into the caller's) and through `gnnpe_main --delta-vertex-counts /
--delta-edge-counts`.

The host forms are held to networkx's rows tallied in numpy, to the full tables for F = E(G), to the insertion and deletion
identities between two graphs and to their own sums.  The device forms are held to the host forms, to the existing device tables
for F = E(G) (a match charged twice shows there), and to a table maintained across Engine.apply_edges against a fresh engine on
the new graph.  The yardstick is never the new kernel."""
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
import test_refine_vertex_counts as rv

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = dl.MODES


# ---- helpers --------------------------------------------------------------------------------------------------------------

_QE = {}


def _qe(qp):
    """the query edges as the tables number them: a list of (a, b)"""
    from gnnpe_amd import binding
    if qp not in _QE:
        _QE[qp] = [tuple(e) for e in binding.host_query_edges(qp).tolist()]
    return _QE[qp]


def _host_tables(g, qp, bm, F, distinct=False, induced=False, limit=FULL):
    """(Delta, VDelta, EDelta) of the two host forms, both complete and agreeing on Delta"""
    from gnnpe_amd import binding
    a, done_v, v = binding.host_refine_sets_delta_vertex_counts(g, qp, bm, F, limit, distinct=distinct, induced=induced)
    b, done_e, e = binding.host_refine_sets_delta_edge_counts(g, qp, bm, F, limit, distinct=distinct, induced=induced)
    assert done_v and done_e and a == b
    assert v.dtype == e.dtype == np.uint64 and e.shape == (len(_qe(qp)), len(g["nbrs"])) and v.shape[1] == len(g["labels"])
    return a, v, e


def _device_tables(eng, qp, bm, F, distinct=False, induced=False):
    a, done_v, v, _ = eng.refine_sets_delta_vertex_counts(qp, bm, F, distinct=distinct, induced=induced)
    b, done_e, e, _ = eng.refine_sets_delta_edge_counts(qp, bm, F, distinct=distinct, induced=induced)
    assert done_v and done_e and a == b
    return a, v, e


def _same(got, want, where):
    assert got[0] == want[0], where + (got[0], want[0])
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), where + ("vertex table",)
    assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2]), where + ("edge table",)


def _carry(g_from, g_to, table):
    """an edge table moved from the entries of one graph to those of another on the same vertices by the key (x, y) of an entry;
    entries the target does not have must be zero, entries the source does not have become zero"""
    k_from, k_to = re_._csr_keys(g_from)[1], re_._csr_keys(g_to)[1]
    out = np.zeros((table.shape[0], len(k_to)), np.uint64)
    there = np.isin(k_from, k_to)
    assert not table[:, ~there].any()
    out[:, np.searchsorted(k_to, k_from[there])] = table[:, there]
    return out


_H1DT = {}


def _h1_delta_tables(tmp_path_factory):
    """the host forms' (Delta, VDelta, EDelta) of dl.H1_DELTA_SHAPES on the three bitmaps in the four modes with the 57-edge F of
    dl._h1_delta, computed once"""
    if _H1DT:
        return _H1DT
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    for name in dl.H1_DELTA_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                t = _host_tables(h["g"], h["q"][name], h["bm"][name][b], f["F"], distinct, induced)
                assert t[0] == f["want"][name, b, distinct, induced]
                _H1DT[name, b, distinct, induced] = t
    return _H1DT


def _to_device(arr):
    """a uint64 array as an int64 torch tensor on device 0, uploaded and finished"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _to_host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture()
def delta_count_lines(monkeypatch, capfd):
    """as sh.sets_lines, for the `[refine_delta_vcount]` and `[refine_delta_ecount]` lines: (tag, fields) per line"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [(ln.split()[0], {k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])})
                for ln in err.splitlines() if ln.startswith(("[refine_delta_vcount] ", "[refine_delta_ecount] "))]
    return take


# ---- CPU: the host forms against yardsticks that are not the library ---------------------------------------------------------

def test_host_forms_against_networkx(tmp_path_factory):
    """1. the inputs of test 1 of test_refine_delta.py -- the 15 small graphs, the eight shapes of ri.IND_SHAPES, both label variants,
    the label/degree and the thinned bitmap, the four modes, the four forms of F --: both tables are np.add.at over networkx's rows
    (inside the sets, induced for INDUCED, filtered by the ordering pairs for DISTINCT, then by "touches F"), cell for cell.  Over
    the run at least a fifth of the cases have a match through F and a tenth have one that avoids it"""
    cases = ri._ind_cases(tmp_path_factory)
    assert len(cases) == 15 * len(ri.IND_SHAPES) * 2
    some = part = total = 0
    for c in cases:
        g, n = c["g"], c["g"]["n"]
        qe = re_._edges_of(c["name"])  # (the shape's own list, not the library's)
        nq = sh.SHAPES[c["name"]][0]
        sets = dl._four_sets(g, 2100 + c["gi"])
        for b in ("ld", "thin"):
            for distinct, induced in MODES:
                rows = c["ind"] if induced else c["emb"]
                rows = rows[rs._in_sets(c[b], rows)]
                if distinct:
                    rows = rows[rd._ordered(rows, re_._pairs(c["qp"]))]
                for form, F in sets.items():
                    keep = rows[dl._touches(rows, qe, F, n)]
                    got = _host_tables(g, c["qp"], c[b], F, distinct, induced)
                    _same(got, (len(keep), rv._table(keep, nq, n), re_._table(g, keep, qe)),
                          (c["gi"], c["name"], c["variant"], b, distinct, induced, form))
                    total += 1
                    some += len(keep) > 0
                    part += 0 < len(keep) < len(rows)
    assert some * 5 >= total and part * 10 >= total, (some, part, total)


def test_all_edges_gives_the_full_tables(tmp_path_factory):
    """2. F = E(G) on H1, the eight shapes, the three bitmaps, the four modes: the tables are host_refine_sets_vertex_counts' and
    host_refine_sets_edge_counts'; `vertex` has no edge: zeros and an empty edge table"""
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    E = dl._und_edges(g)
    vt, et = rv._h1_tables(tmp_path_factory), re_._h1_tables(tmp_path_factory)
    for name in sh.H1_SHAPES:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                got = _host_tables(g, h["q"][name], h["bm"][name][b], E, distinct, induced)
                key = (name, b, distinct, induced)
                if name == "vertex":
                    assert got[0] == 0 and not got[1].any() and got[1].shape == (1, g["n"]) and got[2].shape == (0, len(g["nbrs"]))
                else:
                    assert vt[key][0] == et[key][0]
                    _same(got, (vt[key][0], vt[key][1], et[key][1]), key)


def _identity_runs(tmp_path_factory):
    h = sh._h1(tmp_path_factory)
    runs = [(c["g"], c["qp"], 2300 + c["gi"]) for c in ri._ind_cases(tmp_path_factory)]
    return runs + [(h["g"], h["q"][name], 2400) for name in dl.H1_DELTA_SHAPES]


def test_host_insertion_and_deletion_identities(tmp_path_factory):
    """3. modes 0 and DISTINCT, G' a graph, F a random tenth of its edges (at least one), G = G' minus F on the same vertices, a
    labels-only bitmap.  Insertion: V(G') == V(G) + VDelta(G', F), and E(G') == E(G) carried to the entries of G' by (x, y) +
    EDelta(G', F).  Deletion, the same equation read from G': V(G' - F) == V(G') - VDelta(G', F), and an entry of F holds in
    EDelta(G', F) all of E(G').  The 15 small graphs with the eight shapes and both label variants, and H1 with five shapes"""
    from gnnpe_amd import binding
    grew = 0
    runs = _identity_runs(tmp_path_factory)
    for g1, qp, seed in runs:
        e = dl._und_edges(g1)
        F = e[np.random.default_rng(seed).choice(len(e), max(1, len(e) // 10), replace=False)]
        g0 = dl._without(g1, F)
        bm = dl._label_bitmap(g1, qp)
        in_f = np.isin(re_._csr_keys(g1)[1], np.concatenate([F[:, 0] * g1["n"] + F[:, 1], F[:, 1] * g1["n"] + F[:, 0]]))
        assert in_f.sum() == 2 * len(F)
        for distinct in (False, True):
            d, vd, ed = _host_tables(g1, qp, bm, F, distinct)
            new_v = binding.host_refine_sets_vertex_counts(g1, qp, bm, FULL, distinct=distinct)
            old_v = binding.host_refine_sets_vertex_counts(g0, qp, bm, FULL, distinct=distinct)
            new_e = binding.host_refine_sets_edge_counts(g1, qp, bm, FULL, distinct=distinct)
            old_e = binding.host_refine_sets_edge_counts(g0, qp, bm, FULL, distinct=distinct)
            where = (qp, distinct)
            assert new_v[0] - old_v[0] == d, where
            assert np.array_equal(new_v[2], old_v[2] + vd) and np.array_equal(new_v[2] - vd, old_v[2]), where
            carried = _carry(g0, g1, old_e[2])
            assert np.array_equal(new_e[2], carried + ed) and np.array_equal(new_e[2] - ed, carried), where
            assert not carried[:, in_f].any() and np.array_equal(ed[:, in_f], new_e[2][:, in_f]), where
            grew += d > 0
    assert grew * 2 >= len(runs)  # (the condition of test 3 of test_refine_delta.py, on its runs)


def test_sums_and_the_set_of_f(tmp_path_factory):
    """4. H1 with the 57-edge F, five shapes, the three bitmaps, the four modes: every row of either table sums to
    host_refine_sets_delta; EDelta row k summed over data row x is VDelta[a_k][x], and over the entries with nbrs[j] = y it is
    VDelta[b_k][y]; F with every pair twice, once reversed, shuffled, gives the same tables"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    g, F = h["g"], f["F"]
    tabs = _h1_delta_tables(tmp_path_factory)
    noisy = np.concatenate([F, F[:, ::-1], F[::3]])
    noisy = noisy[np.random.default_rng(5).permutation(len(noisy))]
    for (name, b, distinct, induced), (d, v, e) in tabs.items():
        where = (name, b, distinct, induced)
        assert d == binding.host_refine_sets_delta(g, h["q"][name], h["bm"][name][b], F, FULL, distinct=distinct, induced=induced)
        assert (v.sum(axis=1) == d).all() and (e.sum(axis=1) == d).all(), where
        qe = _qe(h["q"][name])
        for (u, k), m in re_._marginals(g, e, qe, v.shape[0]).items():
            assert np.array_equal(m, v[u]), where + (u, k)
        if b == "ld":
            _same(_host_tables(g, h["q"][name], h["bm"][name][b], noisy, distinct, induced), (d, v, e), where + ("noisy",))
    assert tabs["K4", "ld", False, False][0] == 5400 and tabs["wedge", "ld", False, False][0] == 8086


def test_host_guard(tmp_path_factory):
    """5. limit = Delta: complete 0 and answers == Delta; limit = Delta + 1: complete 1 and the exact table; limit 1; limit 0:
    answers 0, complete 0; no F: zeros, complete 1 -- wedge and K4 on H1 in the four modes, both tables"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    g, F = h["g"], f["F"]
    tabs = _h1_delta_tables(tmp_path_factory)
    for name in ("wedge", "K4"):
        qp, bm = h["q"][name], h["bm"][name]["ld"]
        for distinct, induced in MODES:
            d, v, e = tabs[name, "ld", distinct, induced]
            assert d > 2
            for k, fn in enumerate((binding.host_refine_sets_delta_vertex_counts, binding.host_refine_sets_delta_edge_counts)):
                want = (v, e)[k]
                for limit in (1, d - 1, d):
                    assert fn(g, qp, bm, F, limit, distinct=distinct, induced=induced)[:2] == (limit, False), (name, limit)
                got = fn(g, qp, bm, F, d + 1, distinct=distinct, induced=induced)
                assert got[:2] == (d, True) and np.array_equal(got[2], want)
                assert fn(g, qp, bm, F, 0, distinct=distinct, induced=induced)[:2] == (0, False)
                got = fn(g, qp, bm, np.zeros((0, 2), np.int64), FULL, distinct=distinct, induced=induced)
                assert got[:2] == (0, True) and got[2].shape == want.shape and not got[2].any()


def test_host_refusals(tmp_path_factory, tmp_path):
    """6a. both host forms: a non-edge pair, x == y, an id >= n, unknown mode bits and a disconnected query return GNNPE_ERR_ARG
    with *answers = 0 and *complete = 0, each with its message"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    iso = np.nonzero(h["deg"] == 0)[0]
    good = f["F"][:3].tolist()
    online, u32p, u64p = binding.load_online(), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)
    disc = str(tmp_path / "pair.graph")
    ex._write_query(disc, 2, set(), [0, 0])
    for fn, raw_fn, cells in ((binding.host_refine_sets_delta_vertex_counts, online.gnnpe_host_refine_sets_delta_vertex_counts, 3 * g["n"]),
                              (binding.host_refine_sets_delta_edge_counts, online.gnnpe_host_refine_sets_delta_edge_counts, 3 * len(nb))):
        for bad, msg in (((int(iso[0]), int(iso[1])), "not an edge"), ((7, 7), "loop"), ((3, g["n"]), "does not have"),
                         ((g["n"] + 5, 2), "does not have")):
            with pytest.raises(binding.GnnpeError, match=msg):
                fn(g, qp, bm, good + [bad])

        def raw(edges, mode):
            e = np.ascontiguousarray(np.asarray(edges, np.int64).reshape(-1, 2), np.uint32)
            out, done, table = C.c_uint64(12345), C.c_int(7), np.zeros(cells, np.uint64)
            rc = raw_fn(g["n"], o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), lb.ctypes.data_as(u32p), qp.encode(),
                        bmc.ctypes.data_as(u32p), e.ctypes.data_as(u32p), len(e), FULL, mode, C.byref(out), C.byref(done),
                        table.ctypes.data_as(u64p))
            return rc, out.value, done.value
        assert raw(good, 0) == (0, binding.host_refine_sets_delta(g, qp, bm, good), 1)
        for mode in (4, 7, 1 << 31):
            assert raw(good, mode) == (-1, 0, 0) and b"unknown mode" in binding.load().gnnpe_last_error()
        assert raw(good + [(int(iso[0]), int(iso[1]))], 0) == (-1, 0, 0)
        assert raw(good + [(5, 5)], 1) == (-1, 0, 0)
        for limit in (FULL, 0):
            with pytest.raises(binding.GnnpeError, match="not connected"):
                fn(g, disc, sh._ones(2, g["n"]), good, limit)


def test_cli_refusals(tmp_path):
    """6b. the two flags without --refine sets, without --delta-edges, together, with --matches and with a full count table exit 1
    with their message before a GPU is touched, and leave no output file"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    ef = str(tmp_path / "edges.txt")
    open(ef, "w").write("0 1\n")
    m, m2 = str(tmp_path / "m.txt"), str(tmp_path / "m2.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact"]
    sets = ["--refine", "sets"]
    for flag in ("--delta-vertex-counts", "--delta-edge-counts"):
        for extra, msg in (([flag, m], flag + " needs --refine sets"),
                           ([flag, m, "--delta-edges", ef], "--delta-edges needs --refine sets"),
                           (sets + [flag, m], flag + " needs --delta-edges"),
                           (sets + ["--delta-edges", ef, flag, m, "--matches", m2], flag + " and --matches exclude each other"),
                           (sets + ["--delta-edges", ef, flag, m, "--vertex-counts", m2], "--delta-edges excludes"),
                           (sets + ["--delta-edges", ef, flag, m, "--edge-counts", m2], "--delta-edges excludes"),
                           (sets + ["--delta-edges", ef, "--delta-vertex-counts", m, "--delta-edge-counts", m2],
                            "--delta-vertex-counts and --delta-edge-counts exclude each other")):
            r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
            assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra
            assert not os.path.exists(m) and not os.path.exists(m2), extra
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert "--delta-vertex-counts FILE" in r.stdout and "--delta-edge-counts FILE" in r.stdout


# ---- GPU: the device forms against the host forms and the existing device calls ----------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", dl.H1_DELTA_SHAPES)
def test_gpu_h1_equals_the_host_forms(tmp_path_factory, name):
    """7. H1 with the 57-edge F of dl._h1_delta (a hub-to-hub entry past the first chunk, the ends of a row, a shared vertex, a
    triangle, a pendant edge, 50 random edges), the three bitmaps, the four modes: both tables equal the host forms' exactly.
    GNNPE_TESTING=sets_first_shift is taken as it comes: the items of these calls are the entries of F"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    tabs = _h1_delta_tables(tmp_path_factory)
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            for distinct, induced in MODES:
                _same(_device_tables(eng, h["q"][name], h["bm"][name][b], f["F"], distinct, induced), tabs[name, b, distinct, induced],
                      (name, b, distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_small_graphs_equal_the_host_forms(tmp_path_factory, gi):
    """8. the 15 small graphs with the eight shapes of ri.IND_SHAPES, both label variants, the label/degree and the thinned
    bitmap, the four modes, F = five random edges and F = two edges that share a vertex: device == host forms"""
    from gnnpe_amd import binding, synth
    cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi]
    g = cases[0]["g"]
    sets = dl._four_sets(g, 2100 + gi)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            for b in ("ld", "thin"):
                for distinct, induced in MODES:
                    for form in ("five", "share"):
                        _same(_device_tables(eng, c["qp"], c[b], sets[form], distinct, induced),
                              _host_tables(g, c["qp"], c[b], sets[form], distinct, induced),
                              (gi, c["name"], c["variant"], b, distinct, induced, form))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_all_edges_gives_the_existing_device_tables(tmp_path_factory):
    """9. the charging rule.  F = E(G): the tables are those of Engine.refine_sets_vertex_counts and refine_sets_edge_counts on
    the same engine -- every match once, although it is met in the launch of each of its query edges.  H1 with wedge, triangle,
    C4, diamond and K4 on two bitmaps in the four modes, and two of the small graphs with their eight shapes"""
    from gnnpe_amd import binding, synth
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    runs = [(h["g"], h["sn"], [(h["q"][name], h["bm"][name][b]) for name in ("wedge", "triangle", "C4", "diamond", "K4")
                               for b in ("ld", "thin")], f["all"])]
    for gi in (0, 7):
        cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi]
        g = cases[0]["g"]
        runs.append((g, synth.degree_order(g["offsets"]), [(c["qp"], c["ld"]) for c in cases], dl._und_edges(g)))
    some = 0
    for g, sn, queries, E in runs:
        eng = ex._engine(binding, g, sn, 2)
        try:
            for qp, bm in queries:
                for distinct, induced in MODES:
                    cv, done_v, v, _ = eng.refine_sets_vertex_counts(qp, bm, distinct=distinct, induced=induced)
                    ce, done_e, e, _ = eng.refine_sets_edge_counts(qp, bm, distinct=distinct, induced=induced)
                    assert done_v and done_e and cv == ce
                    _same(_device_tables(eng, qp, bm, E, distinct, induced), (cv, v, e), (qp, distinct, induced))
                    some += cv > 0
        finally:
            eng.close()
    assert some >= 40


@pytest.mark.gpu
def test_gpu_query_sizes_and_reversed_ids(tmp_path_factory, tmp_path):
    """10a. the graphs of dl.test_gpu_query_sizes.  nq == 1: zeros and an empty edge table, nothing launched (device ms 0).  nq == 2:
    the leaf runs at depth 1 on the item's single-entry chunk.  nq == 8: the 8-vertex path on the 33-cycle in the four modes, K8 on
    the planted K10, DISTINCT.  nq == 32: the 32-vertex path on the 32- and the 33-cycle, F = three edges and all edges.  The
    reversed-id files of test_refine_edge_counts on H1, where b_k is placed before a_k: the flip paths of the edge table"""
    from gnnpe_amd import binding, synth
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    g, F = h["g"], f["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for b in sh.BITMAPS:
            got, done, v, ms = eng.refine_sets_delta_vertex_counts(h["q"]["vertex"], h["bm"]["vertex"][b], F)
            assert (got, done, ms) == (0, True, 0.0) and v.shape == (1, g["n"]) and not v.any()
            got, done, e, ms = eng.refine_sets_delta_edge_counts(h["q"]["vertex"], h["bm"]["vertex"][b], F)
            assert (got, done, ms) == (0, True, 0.0) and e.shape == (0, len(g["nbrs"]))
            got, done, v, ms = eng.refine_sets_delta_vertex_counts(h["q"]["edge"], h["bm"]["edge"][b], np.zeros((0, 2), np.int64))
            assert (got, done, ms) == (0, True, 0.0) and not v.any()
            for distinct, induced in MODES:
                _same(_device_tables(eng, h["q"]["edge"], h["bm"]["edge"][b], F, distinct, induced),
                      _host_tables(g, h["q"]["edge"], h["bm"]["edge"][b], F, distinct, induced), ("edge", b, distinct, induced))
        flipped = 0
        for (name, b), r in re_._h1_reversed(tmp_path_factory).items():
            for distinct, induced in MODES:
                want = _host_tables(g, r["qp"], r["bm"], F, distinct, induced)
                _same(_device_tables(eng, r["qp"], r["bm"], F, distinct, induced), want, ("rev", name, b, distinct, induced))
                flipped += want[0] > 0
        assert flipped >= 16
    finally:
        eng.close()
    p8, p32 = sh._path_file(tmp_path, 8), sh._path_file(tmp_path, 32)
    for n, qp in ((33, p8), (32, p32), (33, p32)):
        cyc = sh._cycle_graph(n)
        E = dl._und_edges(cyc)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            nq = binding.host_load_graph(qp)["n"]
            for bm in (ex._ld_bitmap(cyc, qp), sh._ones(nq, n)):
                for distinct, induced in MODES:
                    for Fc in (E[[0, 1, n // 2]], E):
                        _same(_device_tables(eng, qp, bm, Fc, distinct, induced), _host_tables(cyc, qp, bm, Fc, distinct, induced),
                              (n, nq, distinct, induced, len(Fc)))
        finally:
            eng.close()
    k10 = re_._planted_k10()
    k8 = str(tmp_path / "K8.graph")
    ex._write_query(k8, 8, {(a, b) for a in range(8) for b in range(a + 1, 8)}, [0] * 8)
    bm = ex._ld_bitmap(k10, k8)
    clique = [(40 * a, 40 * b) for a in range(10) for b in range(a + 1, 10)][:12]
    want = _host_tables(k10, k8, bm, clique, True)
    assert want[0] == 44
    eng = ex._engine(binding, k10, synth.degree_order(k10["offsets"]), 2)
    try:
        _same(_device_tables(eng, k8, bm, clique, True), want, ("K8",))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_forms(tmp_path_factory, seed):
    """10b. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of
    bitmap) in the four modes, F a random subset of the edges whose size is drawn from {1, 2, |E| / 4, |E|} as in
    test_refine_delta.py: device == host forms"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    g = c["g"]
    E = dl._und_edges(g)
    rng = np.random.default_rng(2600 + seed)
    size = (1, 2, max(1, len(E) // 4), len(E))[int(rng.integers(0, 4))]
    F = E[rng.choice(len(E), min(size, len(E)), replace=False)]
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for distinct, induced in MODES:
            _same(_device_tables(eng, c["qp"], c["bm"], F, distinct, induced), _host_tables(g, c["qp"], c["bm"], F, distinct, induced),
                  (seed, c["which"], len(F), distinct, induced))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_guard(tmp_path_factory, delta_count_lines):
    """11. K4 and the wedge on H1 with the 57-edge F, the four modes, both tables; K4 in mode 0 has Delta = 5 400, far past the
    1 024-find flush.  limit = 1, Delta - 1 and Delta: complete 0 and answers == limit; Delta + 1: complete 1 and the exact
    table; limit 0: (0, 0).  Twice on one context.  Under GNNPE_DEBUG=1 the line after the wait carries finds and flush_adds"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    tabs = _h1_delta_tables(tmp_path_factory)
    F = f["F"]
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for _ in range(2):
            for name in ("K4", "wedge"):
                qp, bm = h["q"][name], h["bm"][name]["ld"]
                for distinct, induced in MODES:
                    d, v, e = tabs[name, "ld", distinct, induced]
                    for k, fn in enumerate((eng.refine_sets_delta_vertex_counts, eng.refine_sets_delta_edge_counts)):
                        for limit in (1, d - 1, d):
                            got = fn(qp, bm, F, limit=limit, distinct=distinct, induced=induced)
                            assert got[:2] == (limit, False), (name, distinct, induced, k, limit, got[:2])
                        got = fn(qp, bm, F, limit=d + 1, distinct=distinct, induced=induced)
                        assert got[:2] == (d, True) and np.array_equal(got[2], (v, e)[k]), (name, distinct, induced, k)
                        assert fn(qp, bm, F, limit=0, distinct=distinct, induced=induced)[:2] == (0, False)
        delta_count_lines()
        d, v, e = tabs["K4", "ld", False, False]
        eng.refine_sets_delta_vertex_counts(h["q"]["K4"], h["bm"]["K4"]["ld"], F)
        eng.refine_sets_delta_edge_counts(h["q"]["K4"], h["bm"]["K4"]["ld"], F)
        done = [(tag, ln) for tag, ln in delta_count_lines() if "finds" in ln]
        assert [tag for tag, _ in done] == ["[refine_delta_vcount]", "[refine_delta_ecount]"]
        for _, ln in done:
            assert ln["finds"] == d and ln["complete"] == 1 and 0 < ln["flush_adds"], ln
        # the vertex table: one flush add per visited image with a find below it, at most 3 per find of a 4-vertex query
        assert done[0][1]["flush_adds"] <= 3 * d
    finally:
        eng.close()


def _batch(g, seed, k=30):
    """k edges of g to delete and k pairs that are no edges of g to insert, as (k, 2) int64 arrays"""
    n = g["n"]
    e = dl._und_edges(g)
    rng = np.random.default_rng(seed)
    D = e[rng.choice(len(e), k, replace=False)]
    have = set((e[:, 0] * n + e[:, 1]).tolist())
    ins = set()
    busy = np.nonzero(np.diff(g["offsets"].astype(np.int64)) >= 3)[0]  # between vertices that have rows: the new edges close matches
    while len(ins) < k:
        x, y = sorted(int(v) for v in rng.choice(busy, 2, replace=False))
        if x * n + y not in have:
            ins.add((x, y))
    return D, np.array(sorted(ins), np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [False, True])
def test_gpu_tables_maintained_across_apply_edges(tmp_path_factory, distinct):
    """12a. modes 0 and DISTINCT, a labels-only bitmap, H1, a batch of 30 deletions and 30 insertions (seed 2800); wedge, triangle,
    diamond and K4.  Vertex table: a caller-owned device table holds V(G); sign -1 with D on G; Engine.apply_edges; sign +1 with I
    on G'; copied back it equals refine_sets_vertex_counts of a FRESH engine on G'.  Edge table: the same, with the table carried
    from G's entries to G''s in numpy by (x, y) between the two steps (the entries of D hold zero by then)"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    D, I = _batch(g, 2800)
    g2 = binding.host_apply_edges(g, insert=I, delete=D)
    assert len(g2["nbrs"]) == len(g["nbrs"])
    names = ("wedge", "triangle", "diamond", "K4")
    bms = {name: dl._label_bitmap(g, h["q"][name]) for name in names}
    fresh = ex._engine(binding, g2, h["sn"], 2)
    try:
        want_v = {name: fresh.refine_sets_vertex_counts(h["q"][name], bms[name], distinct=distinct) for name in names}
        want_e = {name: fresh.refine_sets_edge_counts(h["q"][name], bms[name], distinct=distinct) for name in names}
    finally:
        fresh.close()
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        tv, te = {}, {}
        moved = 0
        for name in names:
            qp, bm = h["q"][name], bms[name]
            v0 = eng.refine_sets_vertex_counts(qp, bm, distinct=distinct)
            e0 = eng.refine_sets_edge_counts(qp, bm, distinct=distinct)
            assert v0[1] and e0[1]
            tv[name], te[name] = _to_device(v0[2]), _to_device(e0[2])
            gone, done, view, _ = eng.refine_sets_delta_vertex_counts(qp, bm, D, distinct=distinct, accum=tv[name].data_ptr(), sign=-1)
            assert done and view.__cuda_array_interface__["data"][0] == tv[name].data_ptr()
            gone_e, done, _, _ = eng.refine_sets_delta_edge_counts(qp, bm, D, distinct=distinct, accum=te[name].data_ptr(), sign=-1)
            assert done and gone_e == gone
            te[name] = _to_device(_carry(g, g2, _to_host(te[name])))
            moved += gone > 0
        assert eng.apply_edges(insert=I, delete=D) == len(g2["nbrs"])
        for name in names:
            qp, bm = h["q"][name], bms[name]
            came, done, _, _ = eng.refine_sets_delta_vertex_counts(qp, bm, I, distinct=distinct, accum=tv[name].data_ptr(), sign=1)
            assert done
            came_e, done, _, _ = eng.refine_sets_delta_edge_counts(qp, bm, I, distinct=distinct, accum=te[name].data_ptr(), sign=1)
            assert done and came_e == came
            assert np.array_equal(_to_host(tv[name]), want_v[name][2]), (name, "vertex table")
            assert np.array_equal(_to_host(te[name]), want_e[name][2]), (name, "edge table")
            moved += came > 0
        assert moved >= 4, moved
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_plus_then_minus_restores_the_bytes(tmp_path_factory):
    """12b. the four modes, diamond and triangle on H1 with the 57-edge F: a caller's table of random 64-bit words, +1 then -1 with
    the same F, is byte for byte what it was; after the +1 it is old + table mod 2^64"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    tabs = _h1_delta_tables(tmp_path_factory)
    g, F = h["g"], f["F"]
    rng = np.random.default_rng(2900)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("diamond", "triangle"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            for distinct, induced in MODES:
                d, v, e = tabs[name, "ld", distinct, induced]
                for fn, table in ((eng.refine_sets_delta_vertex_counts, v), (eng.refine_sets_delta_edge_counts, e)):
                    old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
                    t = _to_device(old)
                    assert fn(qp, bm, F, distinct=distinct, induced=induced, accum=t.data_ptr(), sign=1)[:2] == (d, True)
                    assert np.array_equal(_to_host(t), old + table), (name, distinct, induced)
                    assert fn(qp, bm, F, distinct=distinct, induced=induced, accum=t.data_ptr(), sign=-1)[:2] == (d, True)
                    assert _to_host(t).tobytes() == old.tobytes(), (name, distinct, induced)
    finally:
        eng.close()


def _raw_device(binding, eng, kind, qp, bm, edges, host_counts=None, accum=None, sign=1, limit=FULL, mode=0):
    """the device form through ctypes: (return code, *answers, *complete); both are set to canaries first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    e = np.ascontiguousarray(np.asarray(edges, np.int64).reshape(-1, 2), np.uint32)
    out, done, ms, ptr = C.c_uint64(12345), C.c_int(7), C.c_double(), C.c_void_p()
    fn = getattr(binding.load_online(), f"gnnpe_refine_sets_delta_{kind}_counts")
    rc = fn(eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), e.ctypes.data_as(u32p), len(e), limit, mode, C.byref(out), C.byref(done),
            None if host_counts is None else host_counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ptr),
            None if accum is None else C.c_void_p(accum), sign, C.byref(ms))
    return rc, out.value, done.value


@pytest.mark.gpu
def test_gpu_refusals_in_accumulate_mode(tmp_path_factory):
    """13. F = the 57 valid edges plus one pair that is no edge, accumulating into a caller's table of random words: GNNPE_ERR_ARG
    with *answers == 0, found on the device; the table is byte for byte what it was (a wave that finds the error flag set leaves
    before its first item); the next call on the context is right.  sign outside +-1, host_counts together with dev_accum, and
    sign -1 without dev_accum are refused before anything is launched; a loop and an id >= n too"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    tabs = _h1_delta_tables(tmp_path_factory)
    g, F = h["g"], f["F"]
    o = g["offsets"].astype(np.int64)
    x = int(np.argmax(h["deg"]))  # a non-edge between two vertices that have rows
    far = (x, next(int(y) for y in np.nonzero(h["deg"] > 0)[0] if y != x and y not in g["nbrs"][o[x]:o[x + 1]]))
    rng = np.random.default_rng(3000)
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("triangle", "K4"):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            for distinct, induced in MODES:
                mode = binding.match_mode(distinct, induced)
                d, v, e = tabs[name, "ld", distinct, induced]
                for kind, table in (("vertex", v), ("edge", e)):
                    old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
                    t = _to_device(old)
                    for bad in (far, (far[1], far[0])):
                        for sign in (1, -1):
                            got = _raw_device(binding, eng, kind, qp, bm, F.tolist() + [bad], accum=t.data_ptr(), sign=sign, mode=mode)
                            assert got == (-1, 0, 0) and b"not an edge" in binding.load().gnnpe_last_error(), (name, mode, kind, got)
                            assert _to_host(t).tobytes() == old.tobytes(), (name, mode, kind, "the refused call wrote to the caller's table")
                    assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), sign=1, mode=mode) == (0, d, 1)
                    assert np.array_equal(_to_host(t), old + table), (name, mode, kind)
        qp, bm = h["q"]["triangle"], h["bm"]["triangle"]["ld"]
        d, v, e = tabs["triangle", "ld", False, False]
        for kind, table in (("vertex", v), ("edge", e)):
            old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
            t = _to_device(old)
            host = np.zeros(table.shape, np.uint64)
            for sign in (0, 2, -2, 3):
                assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), sign=sign) == (-1, 0, 0)
                assert b"sign" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, kind, qp, bm, F, sign=-1) == (-1, 0, 0) and b"sign" in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, kind, qp, bm, F, host_counts=host, sign=-1) == (-1, 0, 0)
            assert _raw_device(binding, eng, kind, qp, bm, F, host_counts=host, accum=t.data_ptr()) == (-1, 0, 0)
            assert b"host_counts" in binding.load().gnnpe_last_error()
            for bad, msg in (((7, 7), b"loop"), ((3, g["n"]), b"does not have")):
                assert _raw_device(binding, eng, kind, qp, bm, F.tolist() + [bad], accum=t.data_ptr()) == (-1, 0, 0)
                assert msg in binding.load().gnnpe_last_error()
            assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), mode=4) == (-1, 0, 0)
            assert _to_host(t).tobytes() == old.tobytes() and not host.any()
            with pytest.raises(binding.GnnpeError, match="sign"):
                getattr(eng, f"refine_sets_delta_{kind}_counts")(qp, bm, F, sign=-1)
            assert _raw_device(binding, eng, kind, qp, bm, F, host_counts=host) == (0, d, 1) and np.array_equal(host, table)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_views(tmp_path_factory):
    """14. the device=True views of refine_sets_vertex_counts (ABI 13) and refine_sets_edge_counts (ABI 14) survive calls of the
    new functions, with a context-owned table and accumulating: the new tables live in buffers of their own.  The new device=True
    views are the host-returned tables; a later call of the same function replaces its view (the old one is refused as stale, the
    other function's stays); after Engine.apply_edges every view is refused, the way edge_counts_to_host refuses"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), dl._h1_delta(tmp_path_factory)
    tabs = _h1_delta_tables(tmp_path_factory)
    vt, et = rv._h1_tables(tmp_path_factory), re_._h1_tables(tmp_path_factory)
    g, F = h["g"], f["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        qp, bm = h["q"]["K4"], h["bm"]["K4"]["ld"]
        _, _, view_v, _ = eng.refine_sets_vertex_counts(qp, bm, device=True)
        _, _, view_e, _ = eng.refine_sets_edge_counts(qp, bm, device=True)

        def old_views():
            v = eng.copy_to_host(view_v.__cuda_array_interface__["data"][0], 4 * g["n"] * 8).view(np.uint64).reshape(4, g["n"])
            assert np.array_equal(v, vt["K4", "ld", False, False][1]) and np.array_equal(eng.edge_counts_to_host(view_e), et["K4", "ld", False, False][1])
        old_views()
        d, v, e = tabs["K4", "ld", False, False]
        got, done, dv, _ = eng.refine_sets_delta_vertex_counts(qp, bm, F, device=True)
        assert (got, done) == (d, True) and dv.shape == v.shape and dv.__cuda_array_interface__["typestr"] == "<i8"
        got, done, de, _ = eng.refine_sets_delta_edge_counts(qp, bm, F, device=True)
        assert (got, done) == (d, True) and de.shape == e.shape
        ptrs = {x.__cuda_array_interface__["data"][0] for x in (view_v, view_e, dv, de)}
        assert len(ptrs) == 4 and 0 not in ptrs
        assert np.array_equal(eng.delta_counts_to_host(dv), v) and np.array_equal(eng.delta_counts_to_host(de), e)
        t = _to_device(np.zeros(v.shape, np.uint64))
        eng.refine_sets_delta_vertex_counts(qp, bm, F, accum=t.data_ptr(), sign=1)
        old_views()
        assert np.array_equal(eng.delta_counts_to_host(dv), v) and np.array_equal(_to_host(t), v)  # accumulating leaves the context's own
        d3, v3, _ = tabs["triangle", "thin", True, False]
        got, done, dv3, _ = eng.refine_sets_delta_vertex_counts(h["q"]["triangle"], h["bm"]["triangle"]["thin"], F, distinct=True, device=True)
        assert (got, done) == (d3, True) and np.array_equal(eng.delta_counts_to_host(dv3), v3)
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.delta_counts_to_host(dv)
        assert np.array_equal(eng.delta_counts_to_host(de), e)
        old_views()
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.delta_counts_to_host(view_e)
        eng.apply_edges(delete=F[:1])
        for view in (dv3, de):
            with pytest.raises(binding.GnnpeError, match="stale"):
                eng.delta_counts_to_host(view)
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.edge_counts_to_host(view_e)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", ["q1", "q2"])
def test_gpu_cli_delta_count_tables(tmp_path, test_graph, q):
    """15. gnnpe_main -m online --exact --refine sets --delta-edges F --delta-vertex-counts / --delta-edge-counts on the golden test
    graph, q1 and q2, modes 0 and DISTINCT + INDUCED: the files, in the formats of --vertex-counts and --edge-counts, hold the host
    forms' tables on the label/degree bitmap (computed here, not pinned) and the answer line their Delta; with -n at Delta the guard
    is reached: non-zero exit, the message names -n, no file.  With --apply-edges the tables are the updated graph's"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    n = len(test_graph["labels"])
    E = dl._und_edges(test_graph)
    rng = np.random.default_rng(2700)
    src, _ = re_._csr_keys(test_graph)
    ld = ex._ld_bitmap(test_graph, qp)
    used = np.nonzero(binding.host_refine_sets_edge_counts(test_graph, qp, ld)[2].sum(axis=0))[0]
    used = used[rng.choice(len(used), 6, replace=False)]
    F = np.concatenate([E[rng.choice(len(E), 20, replace=False)], np.stack([src[used], test_graph["nbrs"][used].astype(np.int64)], axis=1)])
    ef = str(tmp_path / "edges.txt")
    open(ef, "w").write("".join(f"{x} {y}\n" if i % 2 else f"{y} {x}\n" for i, (x, y) in enumerate(F.tolist() + F[:1].tolist())))
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--delta-edges", ef]
    qe = _qe(qp)

    def run(extra, out):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        rows = [[int(x) for x in ln.split()] for ln in open(out) if not ln.startswith("#")]
        return ans, np.array(rows, np.uint64).reshape(len(rows), -1)

    def check(gr, bm, extra, distinct, induced, tag):
        d, v, e = _host_tables(gr, qp, bm, F, distinct, induced)
        keys = re_._csr_keys(gr)[1]
        mode = (["--distinct"] if distinct else []) + (["--induced"] if induced else [])
        out = str(tmp_path / f"v_{tag}.txt")
        ans, lines = run(extra + mode + ["--delta-vertex-counts", out], out)
        got = np.zeros_like(v)
        if len(lines):
            assert lines.shape[1] == v.shape[0] + 1 and (np.diff(lines[:, 0].astype(np.int64)) > 0).all() and (lines[:, 1:] != 0).any(axis=1).all()
            got[:, lines[:, 0].astype(np.int64)] = lines[:, 1:].T
        assert ans == d and np.array_equal(got, v), (tag, "vertex table")
        out = str(tmp_path / f"e_{tag}.txt")
        ans, lines = run(extra + mode + ["--delta-edge-counts", out], out)
        head = open(out).readline().split()
        assert head[0] == "#" and [tuple(map(int, x.split("-"))) for x in head[1:]] == qe
        got = np.zeros_like(e)
        if len(lines):
            code = lines[:, 0].astype(np.int64) * n + lines[:, 1].astype(np.int64)
            j = np.searchsorted(keys, code)
            assert lines.shape[1] == len(qe) + 2 and (np.diff(code) > 0).all() and np.array_equal(keys[j], code)
            got[:, j] = lines[:, 2:].T
        assert ans == d and np.array_equal(got, e), (tag, "edge table")
        return d

    total = 0
    for k, (distinct, induced) in enumerate(((False, False), (True, True))):
        total += check(test_graph, ld, [], distinct, induced, f"m{k}")
    assert total > 0
    d = _host_tables(test_graph, qp, ld, F)[0]
    for flag in ("--delta-vertex-counts", "--delta-edge-counts"):
        out = str(tmp_path / "guard.txt")
        r = subprocess.run(base + [flag, out, "-n", str(d)], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "-n" in r.stderr and flag in r.stderr and not os.path.exists(out), (r.returncode, r.stderr)
    if q == "q2":
        # the batch deletes three edges outside F and inserts one pair that is no edge: F stays a set of edges of the new graph
        rest = E[~np.isin(E[:, 0] * n + E[:, 1], dl._codes(F, n))]
        D = rest[rng.choice(len(rest), 3, replace=False)]
        have = set((E[:, 0] * n + E[:, 1]).tolist())
        x, y = next((int(a), int(b)) for a, b in rng.integers(0, n, (1000, 2)) if a < b and int(a) * n + int(b) not in have)
        af = str(tmp_path / "batch.txt")
        open(af, "w").write("".join(f"- {a} {b}\n" for a, b in D.tolist()) + f"+ {x} {y}\n")
        g2 = binding.host_apply_edges(test_graph, insert=[(x, y)], delete=D)
        check(g2, ex._ld_bitmap(g2, qp), ["--apply-edges", af], False, False, "applied")
