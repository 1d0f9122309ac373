"""Count tables of the induced matches on a set of non-edges (include/gnnpe_online.h, ABI version 19): VN_m(C, F)[u][v] and
EN_m(C, F)[k][j], the tables of ABI 13 and 14 over the maps N_m(C, F) of ABI 18 counts only -- on the host
(gnnpe_host_refine_sets_delta_nonedges_vertex_counts / _edge_counts), on the device (gnnpe_refine_sets_delta_nonedges_vertex_counts /
_edge_counts, with a context-owned table or accumulating with a sign into the caller's) and through `gnnpe_main --delta-nonedges F
--delta-vertex-counts / --delta-edge-counts`.

The host forms are held to networkx's induced rows tallied in numpy, to the full induced tables for F = all non-edges, to the
insertion, deletion and two-step identities with the existing host calls supplying the other terms, and to their own sums.  The
device forms are held to the host forms, to the existing device tables for F = all non-edges (a match charged twice, or a cell of
position 1 missed, shows there), and to an induced table maintained across Engine.apply_edges against a fresh engine on the new
graph.  The yardstick is never the new kernel."""
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
import test_refine_delta_nonedges as rn
import test_refine_edge_counts as re_
import test_refine_induced as ri
import test_refine_sets as rs
import test_refine_sets_shapes as sh
import test_refine_vertex_counts as rv

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
H1_SHAPES = ("wedge", "C4", "diamond", "C5", "path4")  # wedge and diamond: the anchor is the only non-adjacent pair, no SetsNon


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _host_tables(g, qp, bm, F, distinct=False, limit=FULL):
    """(N, VN, EN) of the two host forms, both complete and agreeing on N"""
    from gnnpe_amd import binding
    a, done_v, v = binding.host_refine_sets_delta_nonedges_vertex_counts(g, qp, bm, F, limit, distinct=distinct)
    b, done_e, e = binding.host_refine_sets_delta_nonedges_edge_counts(g, qp, bm, F, limit, distinct=distinct)
    assert done_v and done_e and a == b
    assert v.dtype == e.dtype == np.uint64 and e.shape == (len(dc._qe(qp)), len(g["nbrs"])) and v.shape[1] == len(g["labels"])
    return a, v, e


def _device_tables(eng, qp, bm, F, distinct=False):
    a, done_v, v, _ = eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, F, distinct=distinct)
    b, done_e, e, _ = eng.refine_sets_delta_nonedges_edge_counts(qp, bm, F, distinct=distinct)
    assert done_v and done_e and a == b
    return a, v, e


def _delta_host(g, qp, bm, F, distinct):
    """(Delta, VD, ED) of the ABI 17 host forms in the induced mode of `distinct`"""
    return dc._host_tables(g, qp, bm, F, distinct, True)


def _full_host(g, qp, bm, distinct):
    """(|M|, V, E) of the ABI 13 / 14 host forms in the induced mode of `distinct`"""
    from gnnpe_amd import binding
    a, done_v, v = binding.host_refine_sets_vertex_counts(g, qp, bm, FULL, distinct=distinct, induced=True)
    b, done_e, e = binding.host_refine_sets_edge_counts(g, qp, bm, FULL, distinct=distinct, induced=True)
    assert done_v and done_e and a == b
    return a, v, e


_H1Q = {}


def _h1_queries(tmp_path_factory):
    """H1 with the five query files of H1_SHAPES and their label/degree bitmaps: wedge, C4 and diamond are sh._h1's, C5 and the
    4-vertex path are written here"""
    if _H1Q:
        return _H1Q
    h = sh._h1(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("h1n")
    q = {name: h["q"][name] for name in ("wedge", "C4", "diamond")}
    q["C5"] = sh._shape_file(tmp, "C5")
    q["path4"] = sh._path_file(tmp, 4)
    _H1Q.update(q=q, ld={name: ex._ld_bitmap(h["g"], qp) for name, qp in q.items()})
    return _H1Q


_H1T = {}


class _H1Tables:
    """the host forms' (N, VN, EN) of H1_SHAPES on the label/degree bitmap in both induced modes with the F of rn._h1_nonedges (a pair
    of hubs, a pendant and an isolated endpoint, a shared vertex, the ends of a wedge, vertex n - 1, 50 random non-edges): [name,
    distinct], each computed once, when it is first asked for (C5 walks 10^7 monomorphisms on the host)"""

    def __init__(self, tmp_path_factory):
        self.tf = tmp_path_factory

    def __getitem__(self, key):
        if key not in _H1T:
            h, f, hq = sh._h1(self.tf), rn._h1_nonedges(self.tf), _h1_queries(self.tf)
            _H1T[key] = _host_tables(h["g"], hq["q"][key[0]], hq["ld"][key[0]], f["F"], key[1])
        return _H1T[key]

    def items(self):
        return [((name, distinct), self[name, distinct]) for name in H1_SHAPES for distinct in (False, True)]


def _h1_tables(tmp_path_factory):
    return _H1Tables(tmp_path_factory)


def _wedge_ends(g, qp, bm):
    """the non-adjacent data pairs x < y with a common neighbour z such that (x, z, y) have the labels of some wedge a - m - b of the
    query with a and b not adjacent and lie in C(a), C(m), C(b), ascending: an (m, 2) int64 array.  (A connected query with a
    non-adjacent pair has such a wedge; whether a pair carries a whole match is not asked here.)"""
    from gnnpe_amd import binding
    q = binding.host_load_graph(qp)
    n = len(g["labels"])
    qa = rn._adjacent(q)
    a = rn._adjacent(g)
    ai = a.astype(np.int64)
    lab, ql = np.asarray(g["labels"]), np.asarray(q["labels"])
    ids = np.arange(n)
    bits = np.asarray(bm, np.uint32).reshape(q["n"], -1)
    fits = [(lab == ql[u]) & (((bits[u][ids >> 5] >> (ids & 31).astype(np.uint32)) & 1) != 0) for u in range(q["n"])]
    ok = np.zeros_like(a)
    for u, w in ri._non_edges(qp):
        for m in np.nonzero(qa[u] & qa[w])[0]:
            ok |= ((ai[:, fits[m]] @ ai[fits[m], :]) > 0) & fits[u][:, None] & fits[w][None, :]
    ok = (ok | ok.T) & ~a
    x, y = np.nonzero(np.triu(ok, 1))
    return np.stack([x, y], axis=1).astype(np.int64)


_FUZZ = {}


def _fuzz_cases(tmp_path_factory):
    """the 24 fuzz cases of test_refine_sets_shapes, each with an F whose size is drawn from {2, 8, 50, a quarter of the non-edges}:
    half of it from the non-adjacent pairs with a common neighbour that fit a wedge of the query (_wedge_ends), where a match with a
    non-adjacent pair is likely (a single pair is the `hit` form of the small graphs), the rest from all non-edges; and the host forms' tables in both induced modes, computed once"""
    if _FUZZ:
        return _FUZZ
    for seed in sh.FUZZ_SEEDS:
        c = sh._fuzz_case(seed, tmp_path_factory)
        g = c["g"]
        non, near = rn._all_non_edges(g), _wedge_ends(g, c["qp"], c["bm"])
        rng = np.random.default_rng(3900 + seed)
        size = min((2, 8, 50, max(2, len(non) // 4))[int(rng.integers(0, 4))], len(non))
        k = min((size + 1) // 2, len(near))
        first = near[rng.choice(len(near), k, replace=False)]
        rest = non[~np.isin(non[:, 0] * g["n"] + non[:, 1], dl._codes(first, g["n"]))]
        F = np.concatenate([first, rest[rng.choice(len(rest), size - k, replace=False)]])
        _FUZZ[seed] = dict(c=c, F=F, want={d: _host_tables(g, c["qp"], c["bm"], F, d) for d in (False, True)})
    return _FUZZ


def _raw_host(binding, kind, g, qp, bm, pairs, mode, limit=FULL, null=None):
    """a host form through ctypes: (return code, *answers, *complete); both are set to canaries first"""
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    o, nb, lb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    bmc = np.ascontiguousarray(bm, np.uint32)
    e = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.uint32)
    nq = bmc.shape[0]
    table = np.zeros(max(nq * g["n"], nq * nq * len(nb)), np.uint64)
    out, done = C.c_uint64(12345), C.c_int(7)
    args = dict(offsets=o.ctypes.data_as(u32p), nbrs=nb.ctypes.data_as(u32p), labels=lb.ctypes.data_as(u32p), query=qp.encode(),
                bitmap=bmc.ctypes.data_as(u32p), pairs=e.ctypes.data_as(u32p), answers=C.byref(out), complete=C.byref(done),
                counts=table.ctypes.data_as(u64p))
    if null:
        args[null] = None
    fn = getattr(binding.load_online(), f"gnnpe_host_refine_sets_delta_nonedges_{kind}_counts")
    rc = fn(g["n"], args["offsets"], args["nbrs"], args["labels"], args["query"], args["bitmap"], args["pairs"], len(e), limit, mode,
            args["answers"], args["complete"], args["counts"])
    return rc, out.value, done.value


def _raw_device(binding, eng, kind, qp, bm, pairs, host_counts=None, accum=None, sign=1, limit=FULL, mode=2):
    """a device form through ctypes: (return code, *answers, *complete); both are set to canaries first"""
    u32p = C.POINTER(C.c_uint32)
    bmc = np.ascontiguousarray(bm, np.uint32)
    e = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), np.uint32)
    out, done, ms, ptr = C.c_uint64(12345), C.c_int(7), C.c_double(), C.c_void_p()
    fn = getattr(binding.load_online(), f"gnnpe_refine_sets_delta_nonedges_{kind}_counts")
    rc = fn(eng.ctx, qp.encode(), bmc.ctypes.data_as(u32p), e.ctypes.data_as(u32p), len(e), limit, mode, C.byref(out), C.byref(done),
            None if host_counts is None else host_counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ptr),
            None if accum is None else C.c_void_p(accum), sign, C.byref(ms))
    return rc, out.value, done.value


@pytest.fixture()
def nonedge_count_lines(monkeypatch, capfd):
    """as dc.delta_count_lines, for the `[refine_delta_nonedges_vcount]` and `[refine_delta_nonedges_ecount]` lines: (tag, fields)
    per line"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [(ln.split()[0], {k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])})
                for ln in err.splitlines() if ln.startswith(("[refine_delta_nonedges_vcount] ", "[refine_delta_nonedges_ecount] "))]
    return take


# ---- CPU: the host forms against yardsticks that are not the library ---------------------------------------------------------

def test_host_forms_against_networkx(tmp_path_factory):
    """1. the inputs of test 1 of test_refine_delta_nonedges.py -- the 15 small graphs, the eight shapes of ri.IND_SHAPES, both label
    variants, the label/degree and the thinned bitmap, both induced modes, the four forms of F (`hit` is certain to hit, `all` is
    every non-edge) --: both tables are np.add.at over networkx's induced rows (inside the sets, filtered by the ordering pairs for
    DISTINCT, then by "a non-adjacent query pair lies in F"), cell for cell.  For `all` they are host_refine_sets_vertex_counts' and
    host_refine_sets_edge_counts' of the same mode where the query has a non-adjacent pair, and zero where it has none"""
    cases = ri._ind_cases(tmp_path_factory)
    assert len(cases) == 15 * len(ri.IND_SHAPES) * 2
    some = part = total = 0
    for c in cases:
        g, n = c["g"], c["g"]["n"]
        qe = re_._edges_of(c["name"])  # (the shape's own list, not the library's)
        qnon = ri._non_edges(c["qp"])
        nq = sh.SHAPES[c["name"]][0]
        sets = rn._small_sets(g, 3000 + c["gi"])
        for b in ("ld", "thin"):
            for distinct in (False, True):
                rows = rn._nx_rows(c, b, distinct)
                forms = dict(sets)
                hit = rn._hit_set(rows, qnon)
                if hit is not None:
                    forms["hit"] = hit
                for form, F in forms.items():
                    keep = rows[rn._hits(rows, qnon, F, n)]
                    got = _host_tables(g, c["qp"], c[b], F, distinct)
                    where = (c["gi"], c["name"], c["variant"], b, distinct, form)
                    dc._same(got, (len(keep), rv._table(keep, nq, n), re_._table(g, keep, qe)), where)
                    assert form != "hit" or got[0] >= 1, where
                    if form == "all" and qnon:
                        dc._same(got, _full_host(g, c["qp"], c[b], distinct), where + ("the full tables",))
                    assert qnon or (got[0] == 0 and not got[1].any() and not got[2].any()), where
                    total += 1
                    some += len(keep) > 0
                    part += 0 < len(keep) < len(rows)
    assert some * 5 >= total and part * 20 >= total, (some, part, total)


def test_sums_and_marginals(tmp_path_factory):
    """2. H1 with the F of rn._h1_nonedges, the five shapes of H1_SHAPES, both induced modes: every row of either table sums to
    host_refine_sets_delta_nonedges; EN row k summed over the entries of data row x is VN[a_k][x], and over the entries with nbrs[j]
    = y it is VN[b_k][y]; F with every pair twice, once reversed, shuffled, gives the same tables"""
    from gnnpe_amd import binding
    h, f, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), _h1_queries(tmp_path_factory)
    g, F = h["g"], f["F"]
    noisy = np.concatenate([F, F[:, ::-1], F[::3]])
    noisy = noisy[np.random.default_rng(7).permutation(len(noisy))]
    for (name, distinct), (N, v, e) in _h1_tables(tmp_path_factory).items():
        where = (name, distinct)
        qp, bm = hq["q"][name], hq["ld"][name]
        assert N == binding.host_refine_sets_delta_nonedges(g, qp, bm, F, FULL, distinct=distinct) and N > 0, where
        assert name not in rn.H1_SHAPES or N == f["want"][name, "ld", distinct], where
        assert (v.sum(axis=1) == N).all() and (e.sum(axis=1) == N).all(), where
        for (u, k), m in re_._marginals(g, e, dc._qe(qp), v.shape[0]).items():
            assert np.array_equal(m, v[u]), where + (u, k)
        if name in ("wedge", "C4"):
            dc._same(_host_tables(g, qp, bm, noisy, distinct), (N, v, e), where + ("noisy",))


def _identity_check(binding, g0, g1, qp, bm, F, distinct, where):
    """G1 = G0 + F.  Insertion: T(G1) = T(G0) - TN(G0, F) + TD(G1, F); deletion, from G1 to G0: T(G0) = T(G1) - TD(G1, F) + TN(G0, F);
    for V cell by cell, for E by the key (x, y) of an entry.  Returns (N, Delta)"""
    n_, vn, en = _host_tables(g0, qp, bm, F, distinct)
    d_, vd, ed = _delta_host(g1, qp, bm, F, distinct)
    c0, v0, e0 = _full_host(g0, qp, bm, distinct)
    c1, v1, e1 = _full_host(g1, qp, bm, distinct)
    assert c1 == c0 - n_ + d_, where
    assert np.array_equal(v1, v0 - vn + vd) and np.array_equal(v0, v1 - vd + vn), where + ("vertex table",)
    assert np.array_equal(e1, dc._carry(g0, g1, e0 - en) + ed), where + ("edge table, insertion")
    assert np.array_equal(e0, dc._carry(g1, g0, e1 - ed) + en), where + ("edge table, deletion")  # (_carry: the entries of F hold 0 by then)
    return n_, d_


def test_host_insertion_and_deletion_identities(tmp_path_factory):
    """3a. both induced modes, labels-only bitmaps, the runs of test_refine_delta_nonedges.py (the small cases of the shapes with a
    non-adjacent pair, and H1 with the wedge and the diamond): G' = G + F, F a random quarter of G''s edges.  V(G') = V(G) - VN(G, F)
    + VD(G', F), and the same for E compared by the key (x, y) of an entry -- an entry of F has E(G) = 0 and EN(G, F) = 0, which
    dc._carry asserts -- with the existing host calls supplying V, E, VD and ED; read from G' to G it is the deletion identity.  N
    is positive in at least 40 of the 304 (run, mode), Delta in at least 40"""
    from gnnpe_amd import binding
    lost = came = 0
    for g1, qp, seed in rn._identity_runs(tmp_path_factory):
        e = dl._und_edges(g1)
        F = e[np.random.default_rng(seed).choice(len(e), max(1, len(e) // 4), replace=False)]
        g0 = dl._without(g1, F)
        bm = dl._label_bitmap(g1, qp)
        for distinct in (False, True):
            n_, d_ = _identity_check(binding, g0, g1, qp, bm, F, distinct, (qp, distinct))
            lost += n_ > 0
            came += d_ > 0
    assert lost >= 40 and came >= 40, (lost, came)


def test_host_mixed_batch_in_two_steps(tmp_path_factory):
    """3b. a mixed batch by the recipe of the header, delete then insert, every third run of 3a: D a random tenth of the edges, I as
    many random non-edges; G1 = G0 - D, G2 = G1 + I by gnnpe_host_csr_apply_edges.  T(G2) = T(G0) - TD(G0, D) + TN(G1, D) - TN(G1, I) +
    TD(G2, I) against the tables on the graph built in one go, V cell by cell and E by keys"""
    from gnnpe_amd import binding
    for g0, qp, seed in rn._identity_runs(tmp_path_factory)[::3]:
        rng = np.random.default_rng(seed + 50)
        e, non = dl._und_edges(g0), rn._all_non_edges(g0)
        D = e[rng.choice(len(e), max(1, len(e) // 10), replace=False)]
        I = non[rng.choice(len(non), len(D), replace=False)]
        g1 = binding.host_apply_edges(g0, delete=D)
        g2 = binding.host_apply_edges(g1, insert=I)
        both = binding.host_apply_edges(g0, insert=I, delete=D)
        assert np.array_equal(both["nbrs"], g2["nbrs"])
        bm = dl._label_bitmap(g0, qp)
        for distinct in (False, True):
            _, v, e_ = _full_host(g0, qp, bm, distinct)
            _, vd, ed = _delta_host(g0, qp, bm, D, distinct)
            _, vn, en = _host_tables(g1, qp, bm, D, distinct)
            v, e_ = v - vd + vn, dc._carry(g0, g1, e_ - ed) + en
            _, vn, en = _host_tables(g1, qp, bm, I, distinct)
            _, vd, ed = _delta_host(g2, qp, bm, I, distinct)
            v, e_ = v - vn + vd, dc._carry(g1, g2, e_ - en) + ed
            want = _full_host(both, qp, bm, distinct)
            assert np.array_equal(v, want[1]) and np.array_equal(e_, want[2]), (qp, distinct)


def test_host_nothing_to_find_and_the_guard(tmp_path_factory):
    """4. queries without a non-adjacent pair (edge, triangle, K4), the single vertex, and n_pairs == 0 under C4: the V table is all
    zeros, the E table all zeros (empty for the vertex), answers 0 and complete 1; limit == 0 gives complete 0.  The guard on C4 and
    the wedge: limit = N gives complete 0 and answers N, limit = N + 1 complete 1 and the exact table"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory)
    g, F = h["g"], f["F"]
    fns = (binding.host_refine_sets_delta_nonedges_vertex_counts, binding.host_refine_sets_delta_nonedges_edge_counts)
    none = np.zeros((0, 2), np.int64)
    for name, Fq in (("vertex", F), ("edge", F), ("triangle", F), ("K4", F), ("C4", none)):
        qp, bm = h["q"][name], h["bm"][name]["ld"]
        nq, nqe = sh.SHAPES[name][0], len(sh.SHAPES[name][1])
        for distinct in (False, True):
            for fn, shape in zip(fns, ((nq, g["n"]), (nqe, len(g["nbrs"])))):
                got = fn(g, qp, bm, Fq, FULL, distinct=distinct)
                assert got[:2] == (0, True) and got[2].shape == shape and not got[2].any(), (name, distinct)
                assert fn(g, qp, bm, Fq, 0, distinct=distinct)[:2] == (0, False), (name, distinct)
    tabs = _h1_tables(tmp_path_factory)
    hq = _h1_queries(tmp_path_factory)
    for name in ("C4", "wedge"):
        qp, bm = hq["q"][name], hq["ld"][name]
        for distinct in (False, True):
            N, v, e = tabs[name, distinct]
            assert N > 2
            for fn, want in zip(fns, (v, e)):
                for limit in (1, N - 1, N):
                    assert fn(g, qp, bm, F, limit, distinct=distinct)[:2] == (limit, False), (name, limit)
                got = fn(g, qp, bm, F, N + 1, distinct=distinct)
                assert got[:2] == (N, True) and np.array_equal(got[2], want)
                assert fn(g, qp, bm, F, 0, distinct=distinct)[:2] == (0, False)


def test_host_refusals(tmp_path_factory, tmp_path):
    """5. both host forms through the raw C entries: a pair that is an edge in either orientation, a loop, an id >= n, mode 0 and
    mode 1, unknown mode bits, a disconnected query and null arguments return -1 with *answers = 0 and *complete = 0, each with its
    message"""
    from gnnpe_amd import binding
    h, f = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["wedge"], h["bm"]["wedge"]["ld"]
    good = f["F"][:4].tolist()
    edge = dl._und_edges(g)[5].tolist()
    err = lambda: binding.load().gnnpe_last_error()
    disc = str(tmp_path / "three.graph")
    ex._write_query(disc, 3, {(0, 1)}, [0, 0, 0])
    for kind, fn in (("vertex", binding.host_refine_sets_delta_nonedges_vertex_counts),
                     ("edge", binding.host_refine_sets_delta_nonedges_edge_counts)):
        for bad, msg in ((edge, "is an edge"), (edge[::-1], "is an edge"), ((7, 7), "loop"), ((3, g["n"]), "does not have"),
                         ((g["n"] + 5, 2), "does not have")):
            with pytest.raises(binding.GnnpeError, match=msg):
                fn(g, qp, bm, good + [bad])
            assert _raw_host(binding, kind, g, qp, bm, good + [bad], 2) == (-1, 0, 0) and msg.encode() in err()
        want = binding.host_refine_sets_delta_nonedges(g, qp, bm, good)
        assert _raw_host(binding, kind, g, qp, bm, good, 2) == (0, want, 1)
        assert _raw_host(binding, kind, g, qp, bm, good, 3) == (0, binding.host_refine_sets_delta_nonedges(g, qp, bm, good, distinct=True), 1)
        for mode in (0, 1):
            assert _raw_host(binding, kind, g, qp, bm, good, mode) == (-1, 0, 0) and b"GNNPE_MATCH_INDUCED" in err()
        for mode in (4, 6, 7, 1 << 31):
            assert _raw_host(binding, kind, g, qp, bm, good, mode) == (-1, 0, 0) and b"unknown mode" in err()
        for limit in (FULL, 0):
            assert _raw_host(binding, kind, g, disc, sh._ones(3, g["n"]), good, 2, limit) == (-1, 0, 0) and b"not connected" in err()
        for null in ("offsets", "nbrs", "labels", "query", "bitmap", "pairs", "answers", "complete") + (("counts",) if kind == "vertex" else ()):
            assert _raw_host(binding, kind, g, qp, bm, good, 2, null=null)[0] == -1 and b"null argument" in err(), (kind, null)


def test_cli_refusals(tmp_path):
    """6. the table flags with --delta-nonedges but without --induced, together with --matches, both at once, with a full count
    table, and without any F exit 1 with their message before a GPU is touched, and leave no output file"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q2.graph")
    pf = str(tmp_path / "pairs.txt")
    open(pf, "w").write("0 1\n")
    m, m2 = str(tmp_path / "m.txt"), str(tmp_path / "m2.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact", "--refine", "sets"]
    non = ["--induced", "--delta-nonedges", pf]
    for flag in ("--delta-vertex-counts", "--delta-edge-counts"):
        for extra, msg in ((["--delta-nonedges", pf, flag, m], "--delta-nonedges needs --induced"),
                           (non + [flag, m, "--matches", m2], flag + " and --matches exclude each other"),
                           (non + ["--delta-vertex-counts", m, "--delta-edge-counts", m2],
                            "--delta-vertex-counts and --delta-edge-counts exclude each other"),
                           (non + [flag, m, "--vertex-counts", m2], "--delta-nonedges excludes"),
                           (non + [flag, m, "--edge-counts", m2], "--delta-nonedges excludes"),
                           (non + [flag, m, "--delta-edges", pf], "--delta-nonedges and --delta-edges exclude each other"),
                           (["--induced", flag, m], flag + " needs --delta-edges FILE or --delta-nonedges FILE")):
            r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
            assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra
            assert not os.path.exists(m) and not os.path.exists(m2), extra
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert "--delta-edges or --delta-nonedges" in r.stdout


def test_fuzz_draw_hits(tmp_path_factory):
    """8'. the draw of the fuzz test, confirmed with the host form before it goes to a GPU: N > 0 in at least 12 of the 24 seeds, and
    every F holds non-edges only"""
    cases = _fuzz_cases(tmp_path_factory)
    assert len(cases) == 24
    for k in cases.values():
        a = rn._adjacent(k["c"]["g"])
        assert len(k["F"]) and not a[k["F"][:, 0], k["F"][:, 1]].any() and len(dl._codes(k["F"], k["c"]["g"]["n"])) == len(k["F"])
    assert sum(k["want"][False][0] > 0 for k in cases.values()) >= 12, [k["want"][False][0] for k in cases.values()]


# ---- GPU: the device forms against the host forms and the existing device calls ----------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", H1_SHAPES)
def test_gpu_h1_equals_the_host_forms(tmp_path_factory, name):
    """7. H1 with the F of rn._h1_nonedges under wedge, C4, diamond, C5 and the 4-vertex path on the label/degree bitmap, both
    induced modes, both tables, context-owned: the device tables are the host forms', cell for cell.  Wedge and diamond run the
    instantiations without SetsNon; the wedge's walk begins at the leaf, which tallies into position 1"""
    from gnnpe_amd import binding
    h, f, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), _h1_queries(tmp_path_factory)
    tabs = _h1_tables(tmp_path_factory)
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for distinct in (False, True):
            assert tabs[name, distinct][0] > 0
            dc._same(_device_tables(eng, hq["q"][name], hq["ld"][name], f["F"], distinct), tabs[name, distinct], (name, distinct))
        if name in ("wedge", "C4", "diamond"):
            for b in ("thin", "ones"):
                bm = h["bm"][name][b]
                dc._same(_device_tables(eng, h["q"][name], bm, f["F"]), _host_tables(h["g"], h["q"][name], bm, f["F"]), (name, b))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(15))
def test_gpu_small_graphs_equal_the_host_forms(tmp_path_factory, gi):
    """8a. the 15 small graphs with the eight shapes of ri.IND_SHAPES, both label variants, the label/degree and the thinned bitmap,
    both induced modes, F = five random non-edges, two non-edges that share a vertex and, where there is a match, the pair under
    its first non-adjacent query pair: device == host forms"""
    from gnnpe_amd import binding, synth
    cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi]
    g = cases[0]["g"]
    sets = rn._small_sets(g, 3000 + gi)
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        for c in cases:
            qnon = ri._non_edges(c["qp"])
            for b in ("ld", "thin"):
                for distinct in (False, True):
                    forms = dict(five=sets["five"], share=sets["share"])
                    hit = rn._hit_set(rn._nx_rows(c, b, distinct), qnon)
                    if hit is not None:
                        forms["hit"] = hit
                    for form, F in forms.items():
                        dc._same(_device_tables(eng, c["qp"], c[b], F, distinct), _host_tables(g, c["qp"], c[b], F, distinct),
                                 (gi, c["name"], c["variant"], b, distinct, form))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_equals_the_host_forms(tmp_path_factory, seed):
    """8b. the 24 fuzz cases of test_refine_sets_shapes (random graph, connected query of 1-6 vertices, one of four kinds of bitmap)
    in both induced modes, F as _fuzz_cases draws it -- half of it from the non-adjacent pairs with a common neighbour --: device ==
    host forms, and N > 0 in at least 12 of the 24 seeds"""
    from gnnpe_amd import binding, synth
    cases = _fuzz_cases(tmp_path_factory)
    assert sum(k["want"][False][0] > 0 for k in cases.values()) >= 12
    k = cases[seed]
    c, F = k["c"], k["F"]
    eng = ex._engine(binding, c["g"], synth.degree_order(c["g"]["offsets"]), 2)
    try:
        for distinct in (False, True):
            dc._same(_device_tables(eng, c["qp"], c["bm"], F, distinct), k["want"][distinct], (seed, c["which"], len(F), distinct))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_all_non_edges_gives_the_existing_device_tables(tmp_path_factory):
    """9. the charging rule and the cells of position 1.  F = every non-edge of the graph: the tables are those of
    Engine.refine_sets_vertex_counts and refine_sets_edge_counts in the induced mode on the same engine -- every match once,
    although it is met in the launch of each of its non-adjacent pairs, and every cell of the anchor's two positions filled.  Three
    of the small graphs with the five shapes that have a non-adjacent pair, both label variants, both modes"""
    from gnnpe_amd import binding, synth
    some = 0
    for gi in (0, 2, 7):
        cases = [c for c in ri._ind_cases(tmp_path_factory) if c["gi"] == gi and c["name"] in ri.NONEDGE_SHAPES]
        g = cases[0]["g"]
        non = rn._all_non_edges(g)
        eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
        try:
            for c in cases:
                for distinct in (False, True):
                    cv, done_v, v, _ = eng.refine_sets_vertex_counts(c["qp"], c["ld"], distinct=distinct, induced=True)
                    ce, done_e, e, _ = eng.refine_sets_edge_counts(c["qp"], c["ld"], distinct=distinct, induced=True)
                    assert done_v and done_e and cv == ce == len(rn._nx_rows(c, "ld", distinct))
                    dc._same(_device_tables(eng, c["qp"], c["ld"], non, distinct), (cv, v, e), (gi, c["name"], c["variant"], distinct))
                    some += cv > 0
        finally:
            eng.close()
    assert some >= 20, some


@pytest.mark.gpu
def test_gpu_query_sizes_and_orders(tmp_path_factory, tmp_path, nonedge_count_lines):
    """10. nq == 3: the wedge on the 33-cycle (the walk begins at the leaf; nonedges=0 in the line).  nq == 8: the 8-vertex path on
    the 33-cycle, 21 launches.  nq == 32: the 32-vertex path on the 32- and the 33-cycle, 465 launches.  F = three non-edges, then
    all non-edges (the tables of the induced call).  The reversed-id files of test_refine_edge_counts on H1: flipped plan edges.
    The path 0-3-2-1 with the pair (0, 1), launch 0: position 2 is vertex 2, whose pivot is position 1 (the lines say pivot2=1) --
    its entries are taken from the row of the item's second vertex.  In C4, the wedge and that path the anchor (a, b) sorts below a
    query edge, so counting position 1's pseudo-pivot as an edge would shift that edge's number (and trip the nqe check).  Queries
    without a non-adjacent pair and n_pairs == 0 launch nothing: zero tables, complete, device ms 0"""
    from gnnpe_amd import binding, synth
    h, f, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), _h1_queries(tmp_path_factory)
    g, F = h["g"], f["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        nonedge_count_lines()
        for name, Fq in (("vertex", F), ("edge", F), ("triangle", F), ("K4", F), ("C4", np.zeros((0, 2), np.int64))):
            qp, bm = h["q"][name], h["bm"][name]["ld"]
            got, done, v, ms = eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, Fq)
            assert (got, done, ms) == (0, True, 0.0) and v.shape == (sh.SHAPES[name][0], g["n"]) and not v.any(), name
            got, done, e, ms = eng.refine_sets_delta_nonedges_edge_counts(qp, bm, Fq)
            assert (got, done, ms) == (0, True, 0.0) and e.shape == (len(sh.SHAPES[name][1]), len(g["nbrs"])) and not e.any(), name
            assert eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, Fq, limit=0)[:2] == (0, False)
        assert nonedge_count_lines() == []
        for name in ("wedge", "C4", "diamond"):
            qp = re_._reversed_file(tmp_path, name, 0)
            bm = ex._ld_bitmap(g, qp)
            for distinct in (False, True):
                dc._same(_device_tables(eng, qp, bm, F, distinct), _host_tables(g, qp, bm, F, distinct), ("rev", name, distinct))
        p4 = str(tmp_path / "p0321.graph")
        ex._write_query(p4, 4, {(0, 3), (2, 3), (1, 2)}, [0] * 4)
        for qp in (p4, hq["q"]["C4"], hq["q"]["wedge"]):
            anchors, edges = [tuple(p) for p in binding.host_query_nonedges(qp).tolist()], dc._qe(qp)
            assert any(a < e for a in anchors for e in edges)
        bm = ex._ld_bitmap(g, p4)
        nonedge_count_lines()
        for distinct in (False, True):
            want = _host_tables(g, p4, bm, F, distinct)
            assert want[0] > 0
            dc._same(_device_tables(eng, p4, bm, F, distinct), want, ("p0321", distinct))
        lines = [ln for _, ln in nonedge_count_lines() if "launches" in ln]
        assert len(lines) == 4 and all(ln["pivot2"] == 1 and ln["launches"] == 3 for ln in lines), lines
    finally:
        eng.close()
    p3, p8, p32 = sh._path_file(tmp_path, 3), sh._path_file(tmp_path, 8), sh._path_file(tmp_path, 32)
    for n, qp, launches in ((33, p3, 1), (33, p8, 21), (32, p32, 465), (33, p32, 465)):
        cyc = sh._cycle_graph(n)
        non = rn._all_non_edges(cyc)
        eng = ex._engine(binding, cyc, synth.degree_order(cyc["offsets"]), 2)
        try:
            nq = binding.host_load_graph(qp)["n"]
            for bm in (ex._ld_bitmap(cyc, qp), sh._ones(nq, n)):
                for distinct in (False, True):
                    for Fc in (non[[0, 7, len(non) // 2]], non):
                        want = _host_tables(cyc, qp, bm, Fc, distinct)
                        if len(Fc) == len(non):
                            dc._same(want, _full_host(cyc, qp, bm, distinct), (n, nq, distinct, "the full tables"))
                            assert want[0] == {(33, 3): 66, (33, 8): 66, (32, 32): 0, (33, 32): 66}[n, nq] // (2 if distinct else 1)
                        nonedge_count_lines()
                        dc._same(_device_tables(eng, qp, bm, Fc, distinct), want, (n, nq, distinct, len(Fc)))
                        lines = [ln for _, ln in nonedge_count_lines() if "launches" in ln]
                        assert len(lines) == 2 and all(ln["launches"] == launches and ln["items"] == 2 * len(Fc) for ln in lines), lines
                        assert nq > 3 or all(ln["nonedges"] == 0 for ln in lines), lines
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [False, True])
def test_gpu_induced_tables_maintained_across_apply_edges(tmp_path_factory, distinct):
    """11. INDUCED and INDUCED | DISTINCT, a labels-only bitmap, H1, 30 deletions D and 30 insertions I (dc._batch, seed 4000) in two
    steps; wedge, C4 and diamond.  Vertex table: a caller-owned device table holds V(G); -VD(G, D); apply_edges(delete=D); +VN(G1, D);
    -VN(G1, I); apply_edges(insert=I); +VD(G2, I); copied back it equals refine_sets_vertex_counts of a FRESH engine on G2.  Edge
    table: the same, carried from the entries of one graph to the next in numpy by (x, y) between the steps.  At least one N term
    and one Delta term are nonzero"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    D, I = dc._batch(g, 4000)
    g1 = binding.host_apply_edges(g, delete=D)
    g2 = binding.host_apply_edges(g1, insert=I)
    names = ("wedge", "C4", "diamond")
    bms = {name: dl._label_bitmap(g, h["q"][name]) for name in names}
    kw = dict(distinct=distinct, induced=True)
    fresh = ex._engine(binding, g2, h["sn"], 2)
    try:
        want_v = {name: fresh.refine_sets_vertex_counts(h["q"][name], bms[name], **kw) for name in names}
        want_e = {name: fresh.refine_sets_edge_counts(h["q"][name], bms[name], **kw) for name in names}
    finally:
        fresh.close()
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        tv, te = {}, {}
        n_terms = d_terms = 0
        for name in names:
            qp, bm = h["q"][name], bms[name]
            v0, e0 = eng.refine_sets_vertex_counts(qp, bm, **kw), eng.refine_sets_edge_counts(qp, bm, **kw)
            assert v0[1] and e0[1]
            tv[name], te[name] = dc._to_device(v0[2]), dc._to_device(e0[2])
            gone, done, view, _ = eng.refine_sets_delta_vertex_counts(qp, bm, D, accum=tv[name].data_ptr(), sign=-1, **kw)
            assert done and view.__cuda_array_interface__["data"][0] == tv[name].data_ptr()
            gone_e, done, _, _ = eng.refine_sets_delta_edge_counts(qp, bm, D, accum=te[name].data_ptr(), sign=-1, **kw)
            assert done and gone_e == gone
            te[name] = dc._to_device(dc._carry(g, g1, dc._to_host(te[name])))
            d_terms += gone > 0
        assert eng.apply_edges(delete=D) == len(g1["nbrs"])
        for name in names:
            qp, bm = h["q"][name], bms[name]
            for F, sign in ((D, 1), (I, -1)):
                moved, done, view, _ = eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, F, distinct=distinct, accum=tv[name].data_ptr(),
                                                                                    sign=sign)
                assert done and view.__cuda_array_interface__["data"][0] == tv[name].data_ptr()
                moved_e, done, _, _ = eng.refine_sets_delta_nonedges_edge_counts(qp, bm, F, distinct=distinct, accum=te[name].data_ptr(),
                                                                                 sign=sign)
                assert done and moved_e == moved
                n_terms += moved > 0
            te[name] = dc._to_device(dc._carry(g1, g2, dc._to_host(te[name])))
        assert eng.apply_edges(insert=I) == len(g2["nbrs"])
        for name in names:
            qp, bm = h["q"][name], bms[name]
            came, done, _, _ = eng.refine_sets_delta_vertex_counts(qp, bm, I, accum=tv[name].data_ptr(), sign=1, **kw)
            assert done
            came_e, done, _, _ = eng.refine_sets_delta_edge_counts(qp, bm, I, accum=te[name].data_ptr(), sign=1, **kw)
            assert done and came_e == came
            d_terms += came > 0
            assert np.array_equal(dc._to_host(tv[name]), want_v[name][2]), (name, "vertex table")
            assert np.array_equal(dc._to_host(te[name]), want_e[name][2]), (name, "edge table")
        assert n_terms >= 1 and d_terms >= 1, (n_terms, d_terms)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_plus_then_minus_restores_the_bytes(tmp_path_factory):
    """12. both induced modes, C4 and the wedge on H1 with the F of rn._h1_nonedges: a caller's table of random 64-bit words, +1 then
    -1 with the same F, is byte for byte what it was; after the +1 it is old + table mod 2^64"""
    from gnnpe_amd import binding
    h, f, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), _h1_queries(tmp_path_factory)
    tabs = _h1_tables(tmp_path_factory)
    rng = np.random.default_rng(4100)
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for name in ("C4", "wedge"):
            qp, bm = hq["q"][name], hq["ld"][name]
            for distinct in (False, True):
                N, v, e = tabs[name, distinct]
                for fn, table in ((eng.refine_sets_delta_nonedges_vertex_counts, v), (eng.refine_sets_delta_nonedges_edge_counts, e)):
                    old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
                    t = dc._to_device(old)
                    assert fn(qp, bm, f["F"], distinct=distinct, accum=t.data_ptr(), sign=1)[:2] == (N, True)
                    assert np.array_equal(dc._to_host(t), old + table), (name, distinct)
                    assert fn(qp, bm, f["F"], distinct=distinct, accum=t.data_ptr(), sign=-1)[:2] == (N, True)
                    assert dc._to_host(t).tobytes() == old.tobytes(), (name, distinct)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_refusals_in_accumulate_mode(tmp_path_factory, nonedge_count_lines):
    """13. F plus one pair that is an edge (either orientation, both signs), accumulating into a caller's table of random words:
    GNNPE_ERR_ARG with *answers == 0, found on the device; the table is byte for byte what it was; the next call on the context is
    right.  sign outside +-1, host_counts together with dev_accum, sign -1 without dev_accum, a loop, an id >= n, a mode without
    INDUCED and unknown mode bits are refused before anything is launched (no line under GNNPE_DEBUG=1)"""
    from gnnpe_amd import binding
    h, f, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), _h1_queries(tmp_path_factory)
    tabs = _h1_tables(tmp_path_factory)
    g, F = h["g"], f["F"]
    o = g["offsets"].astype(np.int64)
    x = int(np.argmax(h["deg"]))
    edge = (x, int(g["nbrs"][o[x]]))
    rng = np.random.default_rng(4200)
    err = lambda: binding.load().gnnpe_last_error()
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("C4", "wedge"):
            qp, bm = hq["q"][name], hq["ld"][name]
            for distinct in (False, True):
                mode = binding.match_mode(distinct, True)
                N, v, e = tabs[name, distinct]
                for kind, table in (("vertex", v), ("edge", e)):
                    old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
                    t = dc._to_device(old)
                    for bad in (edge, edge[::-1]):
                        for sign in (1, -1):
                            got = _raw_device(binding, eng, kind, qp, bm, F.tolist() + [bad], accum=t.data_ptr(), sign=sign, mode=mode)
                            assert got == (-1, 0, 0) and b"is an edge" in err(), (name, mode, kind, got)
                            assert dc._to_host(t).tobytes() == old.tobytes(), (name, mode, kind, "the refused call wrote to the caller's table")
                    assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), sign=1, mode=mode) == (0, N, 1)
                    assert np.array_equal(dc._to_host(t), old + table), (name, mode, kind)
        qp, bm = hq["q"]["C4"], hq["ld"]["C4"]
        N, v, e = tabs["C4", False]
        for kind, table in (("vertex", v), ("edge", e)):
            old = rng.integers(0, 1 << 64, table.shape, dtype=np.uint64)
            t = dc._to_device(old)
            host = np.zeros(table.shape, np.uint64)
            nonedge_count_lines()
            for sign in (0, 2, -2, 3):
                assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), sign=sign) == (-1, 0, 0) and b"sign" in err()
            assert _raw_device(binding, eng, kind, qp, bm, F, sign=-1) == (-1, 0, 0) and b"sign" in err()
            assert _raw_device(binding, eng, kind, qp, bm, F, host_counts=host, sign=-1) == (-1, 0, 0)
            assert _raw_device(binding, eng, kind, qp, bm, F, host_counts=host, accum=t.data_ptr()) == (-1, 0, 0) and b"host_counts" in err()
            for bad, msg in (((7, 7), b"loop"), ((3, g["n"]), b"does not have")):
                assert _raw_device(binding, eng, kind, qp, bm, F.tolist() + [bad], accum=t.data_ptr()) == (-1, 0, 0) and msg in err()
            for mode in (0, 1):
                assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), mode=mode) == (-1, 0, 0)
                assert b"GNNPE_MATCH_INDUCED" in err()
            for mode in (4, 6, 1 << 31):
                assert _raw_device(binding, eng, kind, qp, bm, F, accum=t.data_ptr(), mode=mode) == (-1, 0, 0) and b"unknown mode" in err()
            assert nonedge_count_lines() == []  # nothing was launched
            assert dc._to_host(t).tobytes() == old.tobytes() and not host.any()
            with pytest.raises(binding.GnnpeError, match="sign"):
                getattr(eng, f"refine_sets_delta_nonedges_{kind}_counts")(qp, bm, F, sign=-1)
            assert _raw_device(binding, eng, kind, qp, bm, F, host_counts=host) == (0, N, 1) and np.array_equal(host, table)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_views(tmp_path_factory):
    """14. the device=True views of refine_sets_vertex_counts (ABI 13), refine_sets_edge_counts (ABI 14) and
    refine_sets_delta_vertex_counts / _edge_counts (ABI 17) survive calls of the new functions, context-owned and accumulating, and
    the new views survive calls of those: six buffers.  A later call of the same new function replaces its view (the old one is
    refused as stale, the others stay); after Engine.apply_edges every view is refused"""
    from gnnpe_amd import binding
    h, f, fd, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), dl._h1_delta(tmp_path_factory), _h1_queries(tmp_path_factory)
    tabs = _h1_tables(tmp_path_factory)
    g, F, FD = h["g"], f["F"], fd["F"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        qp, bm = hq["q"]["C4"], hq["ld"]["C4"]
        full = _full_host(g, qp, bm, False)
        delta = _delta_host(g, qp, bm, FD, False)
        N, v, e = tabs["C4", False]
        _, _, view_v, _ = eng.refine_sets_vertex_counts(qp, bm, induced=True, device=True)
        _, _, view_e, _ = eng.refine_sets_edge_counts(qp, bm, induced=True, device=True)
        _, _, view_dv, _ = eng.refine_sets_delta_vertex_counts(qp, bm, FD, induced=True, device=True)
        _, _, view_de, _ = eng.refine_sets_delta_edge_counts(qp, bm, FD, induced=True, device=True)

        def old_views():
            got = eng.copy_to_host(view_v.__cuda_array_interface__["data"][0], 4 * g["n"] * 8).view(np.uint64).reshape(4, g["n"])
            assert np.array_equal(got, full[1]) and np.array_equal(eng.edge_counts_to_host(view_e), full[2])
            assert np.array_equal(eng.delta_counts_to_host(view_dv), delta[1]) and np.array_equal(eng.delta_counts_to_host(view_de), delta[2])
        old_views()
        got, done, nv, _ = eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, F, device=True)
        assert (got, done) == (N, True) and nv.shape == v.shape and nv.__cuda_array_interface__["typestr"] == "<i8"
        got, done, ne, _ = eng.refine_sets_delta_nonedges_edge_counts(qp, bm, F, device=True)
        assert (got, done) == (N, True) and ne.shape == e.shape
        ptrs = {x.__cuda_array_interface__["data"][0] for x in (view_v, view_e, view_dv, view_de, nv, ne)}
        assert len(ptrs) == 6 and 0 not in ptrs
        assert np.array_equal(eng.delta_counts_to_host(nv), v) and np.array_equal(eng.delta_counts_to_host(ne), e)
        old_views()
        t = dc._to_device(np.zeros(v.shape, np.uint64))
        eng.refine_sets_delta_nonedges_vertex_counts(qp, bm, F, accum=t.data_ptr(), sign=1)
        assert np.array_equal(eng.delta_counts_to_host(nv), v) and np.array_equal(dc._to_host(t), v)  # accumulating leaves the context's own
        # the other way round: the calls of ABI 13, 14 and 17 leave the new views
        eng.refine_sets_vertex_counts(qp, bm, induced=True)
        eng.refine_sets_edge_counts(qp, bm, induced=True)
        eng.refine_sets_delta_vertex_counts(qp, bm, FD, induced=True)
        eng.refine_sets_delta_edge_counts(qp, bm, FD, induced=True)
        assert np.array_equal(eng.delta_counts_to_host(nv), v) and np.array_equal(eng.delta_counts_to_host(ne), e)
        Nw, vw, _ = tabs["wedge", True]
        got, done, nv2, _ = eng.refine_sets_delta_nonedges_vertex_counts(hq["q"]["wedge"], hq["ld"]["wedge"], F, distinct=True, device=True)
        assert (got, done) == (Nw, True) and np.array_equal(eng.delta_counts_to_host(nv2), vw)
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.delta_counts_to_host(nv)
        assert np.array_equal(eng.delta_counts_to_host(ne), e)
        eng.apply_edges(insert=F[:1])
        for view in (nv2, ne, view_dv, view_de):
            with pytest.raises(binding.GnnpeError, match="stale"):
                eng.delta_counts_to_host(view)
        with pytest.raises(binding.GnnpeError, match="stale"):
            eng.edge_counts_to_host(view_e)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_guard(tmp_path_factory, nonedge_count_lines):
    """15. C4, the wedge and C5 on H1 with the F of rn._h1_nonedges, both induced modes, both tables.  limit = 1, N - 1 and N: complete
    0, answers == limit and nothing is copied (the host table stays zero); N + 1: complete 1 and the exact table; limit 0: (0, 0).
    Under GNNPE_DEBUG=1 the line after the wait carries finds and flush_adds: in the vertex kernel at most one flush add per position
    below the leaf and find, in the edge kernel none at all for a 3-vertex query (position 1 has no entry)"""
    from gnnpe_amd import binding
    h, f, hq = sh._h1(tmp_path_factory), rn._h1_nonedges(tmp_path_factory), _h1_queries(tmp_path_factory)
    tabs = _h1_tables(tmp_path_factory)
    F = f["F"]
    eng = ex._engine(binding, h["g"], h["sn"], 2)
    try:
        for name in ("C4", "wedge", "C5"):
            qp, bm = hq["q"][name], hq["ld"][name]
            for distinct in (False, True):
                N, v, e = tabs[name, distinct]
                assert N > 2
                for k, fn in enumerate((eng.refine_sets_delta_nonedges_vertex_counts, eng.refine_sets_delta_nonedges_edge_counts)):
                    for limit in (1, N - 1, N):
                        got = fn(qp, bm, F, limit=limit, distinct=distinct)
                        assert got[:2] == (limit, False) and not got[2].any(), (name, distinct, k, limit, got[:2])
                    got = fn(qp, bm, F, limit=N + 1, distinct=distinct)
                    assert got[:2] == (N, True) and np.array_equal(got[2], (v, e)[k]), (name, distinct, k)
                    assert fn(qp, bm, F, limit=0, distinct=distinct)[:2] == (0, False)
        for name in ("C4", "wedge"):
            N = tabs[name, False][0]
            nonedge_count_lines()
            eng.refine_sets_delta_nonedges_vertex_counts(hq["q"][name], hq["ld"][name], F)
            eng.refine_sets_delta_nonedges_edge_counts(hq["q"][name], hq["ld"][name], F)
            done = [(tag, ln) for tag, ln in nonedge_count_lines() if "finds" in ln]
            assert [tag for tag, _ in done] == ["[refine_delta_nonedges_vcount]", "[refine_delta_nonedges_ecount]"]
            assert all(ln["finds"] == N and ln["complete"] == 1 for _, ln in done), done
            last = sh.SHAPES[name][0] - 1
            assert 0 < done[0][1]["flush_adds"] <= last * N
            assert (done[1][1]["flush_adds"] == 0) if name == "wedge" else (0 < done[1][1]["flush_adds"]), done
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", ["q1", "q2"])
def test_gpu_cli_nonedge_count_tables(tmp_path, test_graph, q):
    """16. gnnpe_main -m online --exact --refine sets --induced --delta-nonedges F --delta-vertex-counts / --delta-edge-counts on the
    golden test graph, q1 and q2, with and without --distinct: the files, in the formats of --vertex-counts and --edge-counts, hold
    the host forms' tables on the label/degree bitmap (computed here, not pinned) and the answer line their N.  F = non-edges that
    each carry a match (found with the host form) and 40 random ones, in both orientations and with a repeat.  With -n at N the
    guard is reached: non-zero exit, the message names -n, no file"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, f"{q}.graph")
    ld = ex._ld_bitmap(test_graph, qp)
    n = len(test_graph["labels"])
    non = rn._all_non_edges(test_graph)
    rng = np.random.default_rng(4300)
    qnon = ri._non_edges(qp)
    a = rn._adjacent(test_graph)
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
    qe = dc._qe(qp)
    keys = re_._csr_keys(test_graph)[1]

    def run(extra, out):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ans = int(next(ln for ln in r.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
        rows = [[int(x) for x in ln.split()] for ln in open(out) if not ln.startswith("#")]
        return ans, np.array(rows, np.uint64).reshape(len(rows), -1)

    for distinct in (False, True):
        N, v, e = _host_tables(test_graph, qp, ld, F, distinct)
        assert N > 0
        mode = ["--distinct"] if distinct else []
        out = str(tmp_path / f"v{int(distinct)}.txt")
        ans, lines = run(mode + ["--delta-vertex-counts", out], out)
        got = np.zeros_like(v)
        assert lines.shape[1] == v.shape[0] + 1 and (np.diff(lines[:, 0].astype(np.int64)) > 0).all() and (lines[:, 1:] != 0).any(axis=1).all()
        got[:, lines[:, 0].astype(np.int64)] = lines[:, 1:].T
        assert ans == N and np.array_equal(got, v), (distinct, "vertex table")
        out = str(tmp_path / f"e{int(distinct)}.txt")
        ans, lines = run(mode + ["--delta-edge-counts", out], out)
        head = open(out).readline().split()
        assert head[0] == "#" and [tuple(map(int, x.split("-"))) for x in head[1:]] == qe
        got = np.zeros_like(e)
        code = lines[:, 0].astype(np.int64) * n + lines[:, 1].astype(np.int64)
        j = np.searchsorted(keys, code)
        assert lines.shape[1] == len(qe) + 2 and (np.diff(code) > 0).all() and np.array_equal(keys[j], code)
        got[:, j] = lines[:, 2:].T
        assert ans == N and np.array_equal(got, e), (distinct, "edge table")
    N = _host_tables(test_graph, qp, ld, F)[0]
    for flag in ("--delta-vertex-counts", "--delta-edge-counts"):
        out = str(tmp_path / "guard.txt")
        r = subprocess.run(base + [flag, out, "-n", str(N)], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "-n" in r.stderr and flag in r.stderr and not os.path.exists(out), (r.returncode, r.stderr)
