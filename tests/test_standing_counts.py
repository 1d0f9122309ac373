"""The count tables a standing exact query keeps (gnnpe_standing_keep_counts / _counts / _count_changes of include/gnnpe_online.h) and
gnnpe_table_fold of include/gnnpe_hip.h: the fold against numpy, and the loop of gnnpe_standing_apply_edges against brute force.

Yardsticks, none of which shares code with the library:
  * numpy for the fold: T0 + D0 on uint64 (which wraps), np.flatnonzero(D0);
  * `embeddings` of tests/test_standing_query.py, every map of a query into the numpy graph, and np.add.at: V[u][f(u)] += 1, and
    E[k][j] += 1 with j found BY KEY x * n + y in a numpy CSR of the current graph (the CSRs are sorted by (x, y)).
    The modes that are not distinct are compared cell by cell.  In the DISTINCT modes a single row of a symmetric query splits by
    the library's ordering pairs (the header says so), and what does not depend on the representative is compared: with the
    automorphisms found here by trying every permutation, the sum of the rows of a vertex orbit -- for E the rows of an edge orbit,
    both directions -- times |Aut(Q)| equals the same sum of the full brute-force table, and count * |Aut(Q)| the number of maps.
    Cell by cell the distinct tables are compared with the one-shot calls on a FRESH engine holding the new graph, with a label
    bitmap: the representative of an occurrence is fixed by the ordering pairs alone, so every sound set gives the same table.
  * the change list: the nonzero cells of new - old of the tables just checked, old moved to the new entries by key for E.

Shapes.  The fold: cells at the wave edges (1, 63 .. 65) and around the 2048-cell tile of k_fold_count / k_fold_apply (2047, 2048,
2049, and 6161 = three tiles and 17 cells: more than one block).  The loop: make_graph(hub_deg=64) of the support tests (n = 301, a
hub row that goes from 64 to 65 entries and back, so that a first-level row is cut into chunks), e = 2, and for the five-vertex
query G(60, 240) as in the standing tests."""
import numpy as np
import pytest

import test_filter_support as fs
import test_standing_query as sqt
from test_standing_query import E, MODES, QUERIES, HUB, ISOLATED, write_query, pack

pytestmark = pytest.mark.gpu

FULL = np.uint64((1 << 64) - 1)
TILE = 2048  # cells per tile of k_fold_count / k_fold_apply (kFoldTile)
CANARY = -0x0123456789ABCDEF
BIG = 1 << 18  # a changes_cap no batch of these tests reaches


# ---- 1. the fold against numpy ------------------------------------------------------------------------------------------------------

FOLD_CELLS = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
FOLD_PATTERNS = ("zero", "all", "first", "last", "every 64th", "1 %", "50 %")


def fold_case(cells, pattern, rng):
    """(T0, D0): the nonzero deltas where the pattern says, the last of them 2^64 - 1 (read as -1), and a table cell that wraps"""
    where = {"zero": np.zeros(cells, bool), "all": np.ones(cells, bool), "first": np.arange(cells) == 0, "last": np.arange(cells) == cells - 1,
             "every 64th": np.arange(cells) % 64 == 0, "1 %": rng.random(cells) < 0.01, "50 %": rng.random(cells) < 0.5}[pattern]
    D0 = np.where(where, rng.integers(1, 1 << 64, cells, dtype=np.uint64), np.uint64(0))
    T0 = rng.integers(0, 1 << 64, cells, dtype=np.uint64)
    nz = np.flatnonzero(D0)
    if len(nz):
        D0[nz[-1]] = FULL
        T0[nz[0]] = FULL  # + a nonzero delta: past 2^64
    return T0, D0


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


@pytest.mark.parametrize("cells", FOLD_CELLS)
def test_gpu_fold_against_numpy(cells):
    import torch
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    rng = np.random.default_rng(1000 + cells)
    for pattern in FOLD_PATTERNS:
        T0, D0 = fold_case(cells, pattern, rng)
        nz = np.flatnonzero(D0)
        n = len(nz)
        want = T0 + D0  # uint64: mod 2^64
        assert n == 0 or want[nz[0]] == D0[nz[0]] - np.uint64(1), "the case has a cell that wraps"
        for cap in sorted({0, max(n - 1, 0), n, n + 5}):
            what = (cells, pattern, cap)
            t, d = dev(T0), dev(D0)
            cc = torch.full((cap + 16,), CANARY, dtype=torch.int64, device="cuda:0") if cap else None
            cd = torch.full((cap + 16,), CANARY, dtype=torch.int64, device="cuda:0") if cap else None
            torch.cuda.synchronize()  # torch fills on its own stream, the context works on its own
            assert eng.table_fold(t, d, cells, cc, cd, cap) == n, what
            assert np.array_equal(fs.to_np(t), want), what
            assert not fs.to_np(d).any(), what
            if cap:
                take = min(cap, n)
                got_c, got_d = cc.cpu().numpy(), cd.cpu().numpy()
                assert np.array_equal(got_c[:take], nz[:take]), what  # ascending, and exactly the nonzero cells
                assert np.array_equal(got_d[:take], D0[nz[:take]].view(np.int64)), what
                assert (got_c[take:] == CANARY).all() and (got_d[take:] == CANARY).all(), (what, "written behind min(cap, n)")
    eng.close()


def test_gpu_fold_refusals():
    import torch
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    T0, D0 = np.arange(100, dtype=np.uint64), np.zeros(100, np.uint64)
    D0[7] = 3
    t, d = dev(T0), dev(D0)
    cc, cd = dev(np.zeros(8, np.uint64)), dev(np.zeros(8, np.uint64))
    torch.cuda.synchronize()
    p = lambda x, off=0: x.data_ptr() + off
    refused = {
        "a null table": (0, p(d), 100, p(cc), p(cd), 8, "null"),
        "a null delta": (p(t), 0, 100, p(cc), p(cd), 8, "null"),
        "a misaligned table": (p(t, 4), p(d), 50, p(cc), p(cd), 8, "aligned"),
        "a misaligned delta": (p(t), p(d, 4), 50, p(cc), p(cd), 8, "aligned"),
        "a misaligned change array": (p(t), p(d), 100, p(cc, 4), p(cd), 4, "aligned"),
        "table and delta overlap": (p(t), p(t, 8 * 50), 100, p(cc), p(cd), 8, "overlap"),
        "a change array inside the table": (p(t), p(d), 100, p(t, 8 * 96), p(cd), 8, "overlap"),
        "the two change arrays overlap": (p(t), p(d), 100, p(cc), p(cc, 8 * 4), 8, "overlap"),
        "cap without the cells": (p(t), p(d), 100, 0, p(cd), 8, "change arrays"),
        "cap without the deltas": (p(t), p(d), 100, p(cc), 0, 8, "change arrays"),
    }
    for what, (a, b, cells, c1, c2, cap, msg) in refused.items():
        with pytest.raises(binding.GnnpeError, match=msg) as err:
            eng.table_fold(a, b, cells, c1 or None, c2 or None, cap)
        assert "[-1]" in str(err.value), (what, str(err.value))
        assert np.array_equal(fs.to_np(t), T0) and np.array_equal(fs.to_np(d), D0), (what, "a refused fold wrote")
    assert eng.table_fold(t, d, 0) == 0 and eng.table_fold(None, None, 0, cc, cd, 8) == 0
    assert np.array_equal(fs.to_np(t), T0) and np.array_equal(fs.to_np(d), D0)
    assert eng.table_fold(t, d, 100, cc, cd, 8) == 1 and fs.to_np(t)[7] == 10 and cc.cpu().numpy()[0] == 7 and cd.cpu().numpy()[0] == 3
    eng.close()


# ---- the brute-force tables -----------------------------------------------------------------------------------------------------------

def csr_keys(g):
    """x * n + y of every adjacency entry, in entry order: ascending, since the rows are sorted"""
    n = g["n"]
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(g["offsets"].astype(np.int64))) * n + g["nbrs"].astype(np.int64)
    assert (np.diff(keys) > 0).all()
    return keys


def query_edges(query):
    return sorted((min(a, b), max(a, b)) for a, b in query[1])


def np_tables(g, query, rows):
    """(V, E) of the maps `rows` (int64 [K, nq]) by np.add.at, the entry of E found by key"""
    nq, n, keys, qe = query[0], g["n"], csr_keys(g), query_edges(query)
    V, Et = np.zeros((nq, n), np.uint64), np.zeros((len(qe), len(keys)), np.uint64)
    for u in range(nq):
        np.add.at(V[u], rows[:, u], 1)
    for k, (a, b) in enumerate(qe):
        want = rows[:, a] * n + rows[:, b]
        j = np.searchsorted(keys, want)
        assert np.array_equal(keys[j], want), "a match runs over a pair that is no entry"
        np.add.at(Et[k], j, 1)
    return V, Et


def yardstick(g, query):
    """per `induced`: (V, E, number of maps) of the brute force, every map counted (the modes that are not distinct)"""
    out = {}
    for induced in (False, True):
        rows = sqt.embeddings(g, query, induced)
        out[induced] = np_tables(g, query, rows) + (len(rows),)
    return out


def orbits(query):
    nq, qe, auts = query[0], query_edges(query), sqt.automorphisms(query)
    vo = {frozenset(p[u] for p in auts) for u in range(nq)}
    eo = {frozenset(qe.index((min(p[a], p[b]), max(p[a], p[b]))) for p in auts) for a, b in qe}
    return len(auts), [sorted(o) for o in vo], [sorted(o) for o in eo]


def check_tables(sq, g, query, mode, Y, fresh, what):
    """the two kept tables of a handle on the graph g; returns them"""
    distinct, induced = mode
    V, Et = sq.counts("vertex"), sq.counts("edge")
    BV, BE, K = Y[induced]
    count = sq.result()[0]
    assert V.shape == BV.shape and Et.shape == BE.shape, (what, mode, V.shape, Et.shape)
    assert sq.counts_ptr("vertex")[1:] == BV.shape and sq.counts_ptr("edge")[1:] == BE.shape
    if not distinct:
        assert count == K, (what, mode, count, K)
        assert np.array_equal(V, BV), (what, mode, "V")
        assert np.array_equal(Et, BE), (what, mode, "E")
    else:
        n_aut, vo, eo = orbits(query)
        n, keys = g["n"], csr_keys(g)
        rev = np.searchsorted(keys, (keys % n) * n + keys // n)  # the entry y -> x of the entry x -> y
        assert count * n_aut == K, (what, mode, count, n_aut, K)
        for o in vo:
            assert np.array_equal(V[o].sum(axis=0) * np.uint64(n_aut), BV[o].sum(axis=0)), (what, mode, "V over the orbit", o)
        for o in eo:
            both = lambda T: T[o].sum(axis=0) + T[o].sum(axis=0)[rev]
            assert np.array_equal(both(Et) * np.uint64(n_aut), both(BE)), (what, mode, "E over the orbit", o)
    if fresh is not None:  # cell by cell against the one-shot calls on a fresh engine
        assert np.array_equal(V, fresh[mode][0]) and np.array_equal(Et, fresh[mode][1]), (what, mode, "the one-shot tables")
    assert (V.sum(axis=1) == count).all() and (Et.sum(axis=1) == count).all(), (what, mode, "a row does not sum to the count")
    return V, Et


def fresh_tables(g, qp, query):
    """the one-shot tables of every mode on a fresh engine with g, the sets being the label bitmap"""
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    bm = pack(np.array([g["labels"] == lb for lb in query[2]]))
    out = {}
    for d, i in MODES:
        v = eng.refine_sets_vertex_counts(qp, bm, distinct=d, induced=i)
        e = eng.refine_sets_edge_counts(qp, bm, distinct=d, induced=i)
        assert v[1] and e[1]
        out[d, i] = (v[2], e[2])
    eng.close()
    return out


def match_edges(g, query):
    """the data edges (not at the hub) that carry the first query edge of an induced match: deleting one destroys matches in every mode"""
    u0, u1 = query_edges(query)[0]
    rows = sqt.embeddings(g, query, True)
    return sorted({(int(min(r[u0], r[u1])), int(max(r[u0], r[u1]))) for r in rows} - {e for e in g["edges"] if HUB in e})


def moved_by_key(old, g_old, g_new):
    """the entry table `old` of g_old in the entries of g_new: the same (x, y), 0 for an entry g_old has not"""
    ko, kn = csr_keys(g_old), csr_keys(g_new)
    out = np.zeros((old.shape[0], len(kn)), np.uint64)
    if len(ko):
        pos = np.minimum(np.searchsorted(ko, kn), len(ko) - 1)
        hit = ko[pos] == kn
        out[:, hit] = old[:, pos[hit]]
    return out


def check_changes(sq, which, old, new, what, short=None):
    """the change list of the last batch == the nonzero cells of new - old (old in the cells of new); short: a handle of the same
    mode with a changes_cap of 3, whose number is the true one and whose pairs are the first three"""
    diff = new.ravel() - old.ravel()  # uint64: mod 2^64, read as int64 below
    cells = np.flatnonzero(diff)
    c, d = sq.count_changes(which)
    assert sq.n_changes(which) == len(cells), (what, which, sq.n_changes(which), len(cells))
    assert np.array_equal(c, cells) and c.dtype == np.uint64, (what, which, "cells")
    assert np.array_equal(d, diff[cells].view(np.int64)) and d.dtype == np.int64, (what, which, "deltas")
    assert len(sq.count_changes(which, cap=1)[0]) == min(1, len(cells))
    if short is not None:
        c3, d3 = short.count_changes(which)
        assert short.n_changes(which) == len(cells), (what, which, "the number under a small cap")
        assert np.array_equal(c3, c[:3]) and np.array_equal(d3, d[:3]), (what, which, "the prefix under a small cap")
        assert len(short.count_changes(which, cap=100)[0]) == min(3, len(cells))
    return len(cells)


# ---- 2. the loop against brute force ------------------------------------------------------------------------------------------------

def run_counts_loop(tmp_path, g0, name, l, batches):
    """on one context: a filter handle per mode that keeps V and E (rows_cap 0: the table searches alone), one more of mode 0 with a
    changes_cap of 3, and an open_sets handle with the label bitmap that keeps rows as well; every batch, every table"""
    query = QUERIES[name]
    qp = write_query(tmp_path, name)
    eng = fs.open_engine(g0, E)
    handles = [eng.standing_open(qp, l=l, distinct=d, induced=i) for d, i in MODES]
    for sq in handles:
        sq.keep_counts(vertex=True, edge=True, changes_cap=BIG)
    short = eng.standing_open(qp, l=l)
    short.keep_counts(vertex=True, edge=True, changes_cap=3)
    sets = eng.standing_open(qp, bitmap=pack(np.array([g0["labels"] == lb for lb in query[2]])), rows_cap=100000)
    sets.keep_counts(vertex=True, edge=True, changes_cap=BIG)
    cases = list(zip(handles, MODES)) + [(short, MODES[0]), (sets, MODES[0])]
    cur = g0
    Y = yardstick(cur, query)
    tables = [check_tables(sq, cur, query, m, Y, fresh_tables(cur, qp, query), (name, l, "open")) for sq, m in cases]
    assert all(sq.n_changes(w) == 0 for sq, _ in cases for w in ("vertex", "edge"))
    changed = 0
    for what, ins, dele in batches:
        nxt = fs.apply_edges_np(fs.apply_edges_np(cur, [], dele), ins, [])
        eng.standing_apply_edges(insert=ins, delete=dele)
        off, nb = eng.download_csr()
        assert np.array_equal(off, nxt["offsets"]) and np.array_equal(nb, nxt["nbrs"]), (what, "the graph")
        Y, fresh = yardstick(nxt, query), fresh_tables(nxt, qp, query)
        for i, (sq, m) in enumerate(cases):
            V, Et = check_tables(sq, nxt, query, m, Y, fresh, (name, l, what))
            if sq is not short:
                changed += check_changes(sq, "vertex", tables[i][0], V, (name, l, what, m), short if i == 0 else None)
                changed += check_changes(sq, "edge", moved_by_key(tables[i][1], cur, nxt), Et, (name, l, what, m), short if i == 0 else None)
            tables[i] = (V, Et)
        # the handle that keeps rows runs the row searches beside the table searches: the same created and destroyed
        assert sets.result()[1:3] == handles[0].result()[1:3] and sets.result()[3:5] == sets.result()[1:3], (name, l, what)
        cur = nxt
    eng.close()
    return changed


@pytest.mark.parametrize("l", [2, 3])
@pytest.mark.parametrize("name", ["wedge", "triangle", "path3", "c4", "diamond"])
def test_gpu_counts_loop_against_brute_force(tmp_path, name, l):
    g0 = fs.make_graph(hub_deg=64)
    assert run_counts_loop(tmp_path, g0, name, l, sqt.loop_batches(g0, 71, name)) > 0, "no batch changed a cell: the test shows nothing"


def test_gpu_counts_loop_five_vertex_query(tmp_path):
    """the house on G(60, 240), two labels, as the standing tests take it: brute force stays within seconds"""
    from gnnpe_amd import synth
    g0 = synth.gnm_graph(60, 240, n_labels=2, seed=5)
    g = fs.graph_of(60, {(int(a), int(b)) for a, b in zip(g0["eu"], g0["ev"])}, g0["labels"])
    rng = np.random.default_rng(9)
    batches, cur = [], g
    for k in (1, 8):
        have = sorted(cur["edges"])
        dele = {have[int(i)] for i in rng.choice(len(have), k, replace=False)}
        ins = set()
        while len(ins) < k:
            a, b = sorted(int(x) for x in rng.choice(60, 2, replace=False))
            if (a, b) not in cur["edges"]:
                ins.add((a, b))
        batches.append((f"{k} + {k}", sqt.norm_pairs(ins), sqt.norm_pairs(dele)))
        cur = fs.apply_edges_np(cur, ins, dele)
    assert run_counts_loop(tmp_path, g, "house", 2, batches) > 0


# ---- 3. an induced handle and a mixed batch: two applies, one change list -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["path3", "diamond"])
def test_gpu_induced_mixed_batch_one_change_list(tmp_path, name):
    """D and I at once on a context with an induced handle: the graph goes through G - D, D is carried through both entry maps, and
    the one change list is in the cells of the final graph.  The second batch deletes and inserts at one vertex."""
    query = QUERIES[name]
    qp = write_query(tmp_path, name)
    g0 = fs.make_graph(hub_deg=64)
    eng = fs.open_engine(g0, E)
    modes = [(False, True), (True, True), (False, False)]
    handles = [eng.standing_open(qp, l=2, distinct=d, induced=i, rows_cap=r) for (d, i), r in zip(modes, (0, 1000, 0))]
    for sq in handles:
        sq.keep_counts(vertex=True, edge=True, changes_cap=BIG)
    # the deleted edges carry the first query edge of an induced match, so that every batch destroys matches
    have = match_edges(g0, query)
    assert len(have) >= 2, "the graph has no induced match of the query: the test shows nothing"
    a, b = have[-1]
    c = next(v for v in range(300) if v not in (a, b, ISOLATED) and (min(a, v), max(a, v)) not in g0["edges"]
             and g0["labels"][v] == g0["labels"][b])
    shared = ([(min(a, c), max(a, c))], [(a, b)])  # the deleted and the inserted edge meet in a
    rng = np.random.default_rng(5)
    ins = set()
    while len(ins) < 15:
        x, y = sorted(int(v) for v in rng.choice(300, 2, replace=False))
        if (x, y) not in g0["edges"] and ISOLATED not in (x, y):
            ins.add((x, y))
    cur = g0
    tables = [check_tables(sq, cur, query, m, yardstick(cur, query), None, (name, "open")) for sq, m in zip(handles, modes)]
    changed = 0
    for what, (i_, d_) in (("15 + 15", (sorted(ins), have[:-1][:15])), ("a shared vertex", shared)):
        nxt = fs.apply_edges_np(fs.apply_edges_np(cur, [], d_), i_, [])
        gen = handles[0].result()[5]
        eng.standing_apply_edges(insert=i_, delete=d_)
        assert handles[0].result()[5] == gen + 2, (what, "two applies")
        Y, fresh = yardstick(nxt, query), fresh_tables(nxt, qp, query)
        for k, (sq, m) in enumerate(zip(handles, modes)):
            V, Et = check_tables(sq, nxt, query, m, Y, fresh, (name, what))
            changed += check_changes(sq, "vertex", tables[k][0], V, (name, what, m))
            changed += check_changes(sq, "edge", moved_by_key(tables[k][1], cur, nxt), Et, (name, what, m))
            tables[k] = (V, Et)
        cur = nxt
    assert changed > 0
    eng.close()


# ---- 4. a handle with tables and one without on one context -----------------------------------------------------------------------------

def test_gpu_handle_without_tables_beside_one_with(tmp_path):
    """the handle without tables is opened FIRST and the second one keeps E alone: the entry map must be asked for all the same.
    What the handle without tables reports is what it reports on a context of its own."""
    g0 = fs.make_graph(hub_deg=64)
    tri, c4 = write_query(tmp_path, "triangle"), write_query(tmp_path, "c4")
    eng, alone = fs.open_engine(g0, E), fs.open_engine(g0, E)
    plain = eng.standing_open(c4, l=3, distinct=True, induced=True, rows_cap=100000)
    kept = eng.standing_open(tri, l=2)
    kept.keep_counts(vertex=False, edge=True, changes_cap=BIG)
    twin = alone.standing_open(c4, l=3, distinct=True, induced=True, rows_cap=100000)
    query = QUERIES["triangle"]
    cur, old = g0, kept.counts("edge")
    rng = np.random.default_rng(3)
    for k, k_del in ((3, 3), (25, 25), (250, 0)):  # the last one outgrows the room the tables were given: T moves to a larger buffer
        have = sorted(cur["edges"])
        dele = [have[int(i)] for i in rng.choice(len(have), k_del, replace=False)]
        ins = set()
        while len(ins) < k:
            x, y = sorted(int(v) for v in rng.choice(301, 2, replace=False))
            if (x, y) not in cur["edges"]:
                ins.add((x, y))
        nxt = fs.apply_edges_np(fs.apply_edges_np(cur, [], dele), ins, [])
        eng.standing_apply_edges(insert=sorted(ins), delete=dele)
        alone.standing_apply_edges(insert=sorted(ins), delete=dele)
        assert plain.result() == twin.result(), k
        rows_of = lambda h, w: np.array(sorted(map(tuple, h.rows(w).tolist())), np.uint32)  # (the waves write their rows in no fixed order)
        for f in (lambda h: rows_of(h, 0), lambda h: rows_of(h, 1), lambda h: h.bitmap(), lambda h: h.table()):
            assert f(plain).tobytes() == f(twin).tobytes(), k
        BV, BE, K = yardstick(nxt, query)[False]
        Et = kept.counts("edge")
        assert kept.count == K and np.array_equal(Et, BE), k
        check_changes(kept, "edge", moved_by_key(old, cur, nxt), Et, ("E alone", k))
        cur, old = nxt, Et
    from gnnpe_amd import binding
    for call in (lambda: plain.counts("vertex"), lambda: plain.count_changes("edge"), lambda: kept.counts("vertex"), lambda: kept.n_changes("vertex"),
                 lambda: kept.counts(3), lambda: kept.counts(0)):
        with pytest.raises(binding.GnnpeError, match=r"\[-1\]"):
            call()
    eng.close()
    alone.close()


# ---- 5. refused batches ------------------------------------------------------------------------------------------------------------------

def counts_snapshot(eng, handles):
    off, nb = eng.download_csr()
    out = [off.tobytes(), nb.tobytes()]
    for sq in handles:
        out += [sq.table().tobytes(), sq.bitmap().tobytes(), sq.result()]
        for w in ("vertex", "edge"):
            c, d = sq.count_changes(w)
            out += [sq.counts(w).tobytes(), sq.n_changes(w), c.tobytes(), d.tobytes()]
    return out


def test_gpu_refused_batches_leave_tables_and_change_lists(tmp_path):
    from gnnpe_amd import binding
    g0 = fs.make_graph(hub_deg=64)
    query = QUERIES["c4"]
    qp = write_query(tmp_path, "c4")
    eng = fs.open_engine(g0, E)
    modes = [(False, False), (False, True)]
    handles = [eng.standing_open(qp, l=2, distinct=d, induced=i) for d, i in modes]
    for sq in handles:
        sq.keep_counts(vertex=True, edge=True, changes_cap=BIG)
    first = match_edges(g0, query)[:3]  # deleting them destroys matches: the change lists of the good batch are not empty
    assert len(first) == 3
    have = first + sorted(g0["edges"] - set(first))
    non = next((a, b) for a in range(300) for b in range(a + 1, 300) if (a, b) not in g0["edges"])
    good_ins = [(a, b) for a in range(40, 60) for b in range(60, 62) if (a, b) not in g0["edges"]][:6]
    eng.standing_apply_edges(insert=good_ins[:3], delete=have[:3])  # a good batch first
    cur = fs.apply_edges_np(g0, good_ins[:3], have[:3])
    assert all(sq.n_changes(w) > 0 for sq in handles for w in ("vertex", "edge"))
    before = counts_snapshot(eng, handles)
    refused = {
        "a non-edge in D": (good_ins[3:4], [have[10], non], "not an edge"),
        "an existing edge in I": ([good_ins[3], have[11]], have[12:13], "already an edge"),
        "an edge in both lists": ([have[20]], [have[20]], "both lists"),
    }
    for what, (ins, dele, msg) in refused.items():
        with pytest.raises(binding.GnnpeError, match=msg):
            eng.standing_apply_edges(insert=ins, delete=dele)
        assert counts_snapshot(eng, handles) == before, what
    # the next good batch is exact: the scratch tables were all zeros
    ins, dele = good_ins[3:], have[30:34]
    nxt = fs.apply_edges_np(fs.apply_edges_np(cur, [], dele), ins, [])
    old = [(sq.counts("vertex"), sq.counts("edge")) for sq in handles]
    eng.standing_apply_edges(insert=ins, delete=dele)
    Y = yardstick(nxt, query)
    for sq, m, (oV, oE) in zip(handles, modes, old):
        V, Et = check_tables(sq, nxt, query, m, Y, None, "after the refusals")
        check_changes(sq, "vertex", oV, V, "after the refusals")
        check_changes(sq, "edge", moved_by_key(oE, cur, nxt), Et, "after the refusals")
    eng.close()


# ---- 6. lifecycle -------------------------------------------------------------------------------------------------------------------------

def test_gpu_keep_counts_lifecycle(tmp_path):
    from gnnpe_amd import binding
    g0 = fs.make_graph(hub_deg=64)
    query = QUERIES["wedge"]
    qp = write_query(tmp_path, "wedge")
    eng = fs.open_engine(g0, E)
    sq = eng.standing_open(qp, l=2, induced=True)
    rows = eng.standing_open(qp, l=2, induced=True, rows_cap=100000)
    for bad in (0, 4, 7):
        with pytest.raises(binding.GnnpeError, match=r"\[-1\]"):
            eng._ck(binding.load_online().gnnpe_standing_keep_counts(sq.handle, bad, 0, None))
    with pytest.raises(binding.GnnpeError, match="keep_counts"):
        sq.counts("vertex")
    # V, then E added; the tables of the handle with rows are the same
    sq.keep_counts(vertex=True, edge=False, changes_cap=BIG)
    with pytest.raises(binding.GnnpeError, match="keep_counts"):
        sq.counts("edge")
    have = sorted(e for e in g0["edges"] if HUB not in e)
    eng.standing_apply_edges(delete=have[:4])
    cur = fs.apply_edges_np(g0, [], have[:4])
    sq.keep_counts(vertex=False, edge=True, changes_cap=BIG)  # E is built on the graph as it is now; V stays
    rows.keep_counts(vertex=True, edge=True, changes_cap=BIG)
    Y = yardstick(cur, query)
    mode = (False, True)
    check_tables(sq, cur, query, mode, Y, None, "E added")
    ins = [(a, b) for a in range(10, 14) for b in range(200, 203) if (a, b) not in cur["edges"]][:5]
    nxt = fs.apply_edges_np(fs.apply_edges_np(cur, [], have[10:14]), ins, [])
    old = (sq.counts("vertex"), sq.counts("edge"))
    eng.standing_apply_edges(insert=ins, delete=have[10:14])
    Y = yardstick(nxt, query)
    V, Et = check_tables(sq, nxt, query, mode, Y, None, "a batch after E was added")
    check_tables(rows, nxt, query, mode, Y, None, "the handle with rows")
    check_changes(sq, "vertex", old[0], V, "lifecycle")
    check_changes(sq, "edge", moved_by_key(old[1], cur, nxt), Et, "lifecycle")
    # rows_cap == 0 and rows_cap > 0: the same created and destroyed, the second with every row held
    assert sq.result()[:3] == rows.result()[:3] and rows.result()[3:5] == rows.result()[1:3] and sq.result()[3:5] == (0, 0)
    assert rows.result()[1] + rows.result()[2] > 0
    # a new changes_cap: the tables stay, the lists are emptied
    sq.keep_counts(vertex=True, edge=True, changes_cap=2)
    assert np.array_equal(sq.counts("vertex"), V) and sq.n_changes("vertex") == 0 and len(sq.count_changes("edge")[0]) == 0
    # a change behind the handle's back: stale until refresh, which rebuilds the tables
    eng.apply_edges(delete=have[20:25])
    cur = fs.apply_edges_np(nxt, [], have[20:25])
    for call in (lambda: sq.counts("vertex"), lambda: sq.counts_ptr("edge"), lambda: sq.n_changes("vertex"),
                 lambda: sq.keep_counts(vertex=True, edge=True)):
        with pytest.raises(binding.GnnpeError, match="gnnpe_standing_refresh"):
            call()
    eng.vde(want=False)
    sq.refresh()
    rows.refresh()
    Y = yardstick(cur, query)
    check_tables(sq, cur, query, mode, Y, None, "refresh")
    assert sq.n_changes("vertex") == 0 and sq.n_changes("edge") == 0
    eng.standing_apply_edges(insert=have[20:22])
    cur = fs.apply_edges_np(cur, have[20:22], [])
    check_tables(sq, cur, query, mode, yardstick(cur, query), None, "a batch after the refresh")
    assert len(sq.count_changes("vertex")[0]) == min(2, sq.n_changes("vertex")) and len(sq.count_changes("edge")[0]) == min(2, sq.n_changes("edge"))
    sq.close()
    eng.close()  # gnnpe_destroy closes the handle with tables that is still open


def test_gpu_single_vertex_and_single_edge_queries(tmp_path):
    g0 = fs.make_graph(hub_deg=64)
    one, edge = str(tmp_path / "one.graph"), str(tmp_path / "edge.graph")
    sqt._write_query(one, 1, set(), [1])
    sqt._write_query(edge, 2, {(0, 1)}, [1, 0])
    q1, q2 = (1, set(), [1]), (2, {(0, 1)}, [1, 0])
    eng = fs.open_engine(g0, E)
    a = eng.standing_open(one, l=2)
    b = eng.standing_open(edge, l=2, distinct=True, induced=True)
    for sq in (a, b):
        sq.keep_counts(vertex=True, edge=True, changes_cap=BIG)
    V1 = a.counts("vertex")
    assert a.counts("edge").shape == (0, len(g0["nbrs"])) and a.counts_ptr("edge")[0] == 0
    assert np.array_equal(V1[0], (g0["labels"] == 1).astype(np.uint64)) and a.count == int((g0["labels"] == 1).sum())
    cur = g0
    have = sorted(e for e in g0["edges"] if HUB not in e and {int(g0["labels"][e[0]]), int(g0["labels"][e[1]])} == {0, 1})
    non = [(x, y) for x in range(20, 40) for y in range(100, 110) if (x, y) not in g0["edges"]
           and {int(g0["labels"][x]), int(g0["labels"][y])} == {0, 1}][:4]
    for ins, dele in ((non, have[:3]), ([], have[5:9])):
        nxt = fs.apply_edges_np(fs.apply_edges_np(cur, [], dele), ins, [])
        old = (b.counts("vertex"), b.counts("edge"))
        eng.standing_apply_edges(insert=ins, delete=dele)
        assert np.array_equal(a.counts("vertex"), V1) and a.n_changes("vertex") == 0 and a.n_changes("edge") == 0
        assert a.counts("edge").shape == (0, len(nxt["nbrs"]))
        V, Et = check_tables(b, nxt, q2, (False, True), yardstick(nxt, q2), None, "a single edge")  # (no symmetry: distinct changes nothing)
        assert check_changes(b, "vertex", old[0], V, "a single edge") > 0
        # (the entry of a match that stays keeps its 1 and a deleted one is gone: the list holds the inserted entries that run from
        # the label of query vertex 0 to that of query vertex 1, one of the two directions of every inserted edge)
        assert check_changes(b, "edge", moved_by_key(old[1], cur, nxt), Et, "a single edge") == len(ins)
        cur = nxt
    eng.close()


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [[], ["-l", "3", "--refine", "sets", "--induced", "--distinct"]])
def test_gpu_cli_standing_counts(tmp_path, test_graph, flags):
    """gnnpe_main -m online --exact --standing with two batch files and both tables on the Test graph: the files written after the
    last batch are, byte for byte, those of --vertex-counts / --edge-counts of a fresh run that applies the net batch in one go"""
    import os
    import subprocess
    from conftest import GOLDEN
    base = sqt.base
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    qp = os.path.join(base.ONLINE, "q1.graph")
    n = len(test_graph["labels"])
    und = {(v, int(w)) for v in range(n) for w in test_graph["nbrs"][test_graph["offsets"][v]:test_graph["offsets"][v + 1]] if v < w}
    rng = np.random.default_rng(23)
    lines = [ln.split() for ln in open(qp)]
    qlab = [int(ln[2]) for ln in lines if ln[0] == "v"]
    el = {(qlab[int(ln[1])], qlab[int(ln[2])]) for ln in lines if ln[0] == "e"}
    lab = test_graph["labels"]
    fits = lambda e: (int(lab[e[0]]), int(lab[e[1]])) in el or (int(lab[e[1]]), int(lab[e[0]])) in el  # the labels of a query edge
    cur, files = set(und), []
    for i, (k_ins, k_del) in enumerate(((12, 12), (6, 20))):
        have = [e for e in sorted(cur) if fits(e)]
        dele = [have[int(j)] for j in rng.choice(len(have), k_del, replace=False)]
        ins = set()
        while len(ins) < k_ins:
            a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False))
            if (a, b) not in cur and fits((a, b)):
                ins.add((a, b))
        files.append(str(tmp_path / f"batch{i}.txt"))
        open(files[-1], "w").write("".join(f"+ {a} {b}\n" for a, b in sorted(ins)) + "".join(f"- {a} {b}\n" for a, b in dele))
        cur = (cur - set(dele)) | ins
    net = str(tmp_path / "net.txt")
    open(net, "w").write("".join(f"+ {a} {b}\n" for a, b in sorted(cur - und)) + "".join(f"- {a} {b}\n" for a, b in sorted(und - cur)))
    root = base._dataset(tmp_path, graph)
    head = [base.CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact"] + flags
    out_v, out_e = str(tmp_path / "standing_v.txt"), str(tmp_path / "standing_e.txt")
    cmd = head + ["--standing", "--standing-vertex-counts", out_v, "--standing-edge-counts", out_e]
    for f in files:
        cmd += ["--apply-edges", f]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    changes = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("changes: ")]
    assert len(changes) == 2 and len([ln for ln in r.stdout.splitlines() if ln.startswith("standing: ")]) == 3, r.stdout
    for flag, got in (("--vertex-counts", out_v), ("--edge-counts", out_e)):
        want = str(tmp_path / ("fresh" + flag))
        r = subprocess.run(head + ([] if flags else ["--refine", "sets"]) + ["--apply-edges", net, flag, want], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert open(got).read() == open(want).read() and len(open(want).read().splitlines()) > 1, flag
    assert sum(changes) > 0
    r = subprocess.run(head + ["--apply-edges", files[0], "--standing-vertex-counts", out_v], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--standing" in r.stderr + r.stdout
