"""Label and vertex batches through the standing exact query (gnnpe_standing_set_labels, gnnpe_standing_apply_vertices of
include/gnnpe_online.h) against brute force.

Yardsticks, none of which shares code with the library: match_set of tests/test_standing_query.py for the count, created,
destroyed and both row lists; np_support / fresh_bits of tests/test_filter_support.py for S and C; yardstick / fresh_tables /
check_changes of tests/test_standing_counts.py for the kept tables V and E and their change lists.  Across a vertex batch the
yardstick moves through fs.apply_vertices_np's new ids: the destroyed rows are matches of G in the ids of G (exactly those through
a removed vertex), the created rows matches of G' in the ids of G' (exactly those through an added vertex), and the change lists
are the difference to the old tables carried to the new ids by key.

One context per (query, l) runs all batches in a row, so that every kind follows another: eight relabel batches, then an edge at
the hub, six vertex batches, the empty one, and an edge batch naming the new ids.  Open on it: the four modes with rows (mode 0
keeping V and E, DISTINCT | INDUCED keeping V) and a mode-0 handle with rows_cap == 0 that keeps V and E, whose created and
destroyed come from the count kernels alone.  The graph is make_graph(hub_deg=64) of the support tests (n = 301, a hub row of 64
entries, vertex 17 isolated), e = 2."""
import numpy as np
import pytest

import dynamic_session as ds
import test_dynamic_sessions as tds
import test_filter_support as fs
import test_standing_counts as sc
from test_standing_query import QUERIES as SQ_QUERIES, MODES, match_set, as_mode, check_batch, write_query, pack

pytestmark = pytest.mark.gpu

E, NL, BIG = 2, fs.NL, 1 << 18
HUB, ISOLATED = fs.HUB, fs.ISOLATED
QUERIES = {k: SQ_QUERIES[k] for k in ("wedge", "triangle", "path3", "c4")}
QUERIES["single"] = (1, set(), [1])
CASES = [(name, 2) for name in QUERIES] + [("triangle", 3), ("c4", 3)]


def query_file(tmp_path, name):
    if name != "single":
        return write_query(tmp_path, name)
    from test_online_exact import _write_query
    qp = str(tmp_path / "single.graph")
    _write_query(qp, *QUERIES[name])
    return qp


def relabelled(g, R, labels):
    new = g["labels"].copy()
    new[np.asarray(R, np.int64)] = labels
    return fs.graph_of(g["n"], g["edges"], new)


def through(rows, new_id):
    """match tuples of G in the ids of G' (monotone on the survivors: an orbit's smallest image stays the smallest); the second
    value: the tuples with a removed vertex"""
    kept, gone = set(), set()
    for r in rows:
        m = tuple(int(new_id[v]) for v in r)
        (gone.add(r) if min(m) < 0 else kept.add(m))
    return kept, gone


class Run:
    """the handles of one context and the model graph they must be exact for"""

    def __init__(self, oracle, tmp_path, name, l, g):
        from gnnpe_amd import binding
        self.oracle, self.name, self.l, self.query, self.g = oracle, name, l, QUERIES[name], g
        self.qp = query_file(tmp_path, name)
        self.plan = binding.host_query_plan_exact(self.qp, E, l)
        self.eng = fs.open_engine(g, E)
        self.handles = []
        for mode in MODES:
            sq = self.eng.standing_open(self.qp, l=l, distinct=mode[0], induced=mode[1], rows_cap=BIG)
            keeps = ["vertex", "edge"] if mode == (False, False) else ["vertex"] if mode == (True, True) else []
            if keeps:
                sq.keep_counts(vertex=True, edge="edge" in keeps, changes_cap=BIG)
            self.handles.append(tds.Handle(sq, mode, l, keeps))
        sq = self.eng.standing_open(self.qp, l=l)  # rows_cap == 0 with kept tables: the count kernels' answers serve
        sq.keep_counts(vertex=True, edge=True, changes_cap=BIG)
        self.norows = tds.Handle(sq, (False, False), l, ["vertex", "edge"])
        self.sets = {m: match_set(g, self.query, *m) for m in MODES}
        self.moved = np.zeros(2, np.int64)
        self.changed = 0
        self.check_state("open", None)

    def all(self):
        return self.handles + [self.norows]

    def check_state(self, what, old):
        """S, C, the sizes, the kept tables of every handle on self.g; old: {handle: tables in the cells of self.g} for the change
        lists of the batch that led here (None: no batch)"""
        g, query = self.g, self.query
        vde = fs.vde_of(self.oracle, g, E)
        want_s, bits = fs.np_support(g, vde, self.plan), fs.fresh_bits(g, E, self.plan)
        Y = sc.yardstick(g, query)
        ft = sc.fresh_tables(g, self.qp, query) if query[0] > 1 else None
        for h in self.all():
            assert h.sq.count == len(self.sets[h.mode]), (what, h.mode, "count")
            assert np.array_equal(h.sq.table(), want_s), (what, h.mode, "S")
            bm = h.sq.bitmap()
            assert bm.shape[1] == (g["n"] + 31) // 32 and (g["n"] % 32 == 0 or not np.any(bm[:, -1] >> np.uint32(g["n"] % 32))), (what, "bits past n")
            assert np.array_equal(fs.bits_of(bm, g["n"]), bits), (what, h.mode, "C against the fresh filter")
            assert list(h.sq.set_sizes()) == list(bits.sum(axis=1)), (what, h.mode, "sizes")
            if h.keeps == {"vertex", "edge"}:
                V, Et = sc.check_tables(h.sq, g, query, h.mode, Y, ft, what)
                new = dict(vertex=V, edge=Et)
            elif h.keeps and ft is not None:
                new = tds.check_kept(h, g, query, Y, ft, what)
            elif h.keeps:
                new = dict(vertex=h.sq.counts("vertex"))
                assert np.array_equal(new["vertex"], Y[h.mode[1]][0]), (what, h.mode, "V")
            else:
                new = {}
            if old is not None:
                for w in sorted(h.keeps):
                    self.changed += sc.check_changes(h.sq, w, old[id(h)][w], new[w], (what, h.mode, w))
            h.tables = new
        a, b = self.handles[0].sq.result(), self.norows.sq.result()
        assert a[:3] == b[:3] and b[3:5] == (0, 0), (what, "rows_cap == 0 against the handle with rows", a, b)

    def check_rows(self, what, created, destroyed):
        """created / destroyed: {mode: set of tuples}, in the ids the call reports them in"""
        for h in self.handles:
            c, d = sorted(created[h.mode]), sorted(destroyed[h.mode])
            count, n_c, n_d, rows_c, rows_d, _ = h.sq.result()
            assert (n_c, n_d) == (len(c), len(d)), (what, h.mode, "created, destroyed", n_c, n_d, len(c), len(d))
            assert (rows_c, rows_d) == (len(c), len(d)), (what, h.mode, "rows held")
            assert as_mode(h.sq.rows(0), self.query, h.mode[0]) == c, (what, h.mode, "created rows")
            assert as_mode(h.sq.rows(1), self.query, h.mode[0]) == d, (what, h.mode, "destroyed rows")
        self.moved += (len(created[False, False]), len(destroyed[False, False]))

    def old_tables(self, move_v=None, move_e=None):
        out = {}
        for h in self.all():
            t = dict(h.tables)
            if "vertex" in t and move_v:
                t["vertex"] = move_v(t["vertex"])
            if "edge" in t and move_e:
                t["edge"] = move_e(t["edge"])
            out[id(h)] = t
        return out

    def generation(self):
        return self.handles[0].sq.result()[5]

    def relabel(self, what, R, labels):
        g, query = self.g, self.query
        nxt = relabelled(g, R, labels)
        real = bool((nxt["labels"] != g["labels"]).any())
        gen = self.generation()
        old = self.old_tables()
        ms = self.eng.standing_set_labels(R, labels, timing=True)
        assert ms >= 0.0 and self.generation() == gen + (1 if real else 0), (what, "generation")
        assert np.array_equal(self.eng.download_labels(), nxt["labels"]), (what, "the labels")
        after = {m: match_set(nxt, query, *m) for m in MODES}
        self.check_rows(what, {m: after[m] - self.sets[m] for m in MODES}, {m: self.sets[m] - after[m] for m in MODES})
        self.sets, self.g = after, nxt
        self.check_state(what, old)
        if not real:
            for h in self.all():
                assert h.sq.result()[1:5] == (0, 0, 0, 0) and all(h.sq.n_changes(w) == 0 for w in h.keeps), (what, "a no-op batch")

    def vertices(self, what, rem, add):
        g, query = self.g, self.query
        nxt, new_id = fs.apply_vertices_np(g, rem, add)
        gen = self.generation()
        keep = np.flatnonzero(new_id >= 0)

        def move_v(V):
            out = np.zeros((V.shape[0], nxt["n"]), np.uint64)
            out[:, new_id[keep]] = V[:, keep]
            return out

        def move_e(Et):
            rows = [ds.carry_tags(g, Et[k], nxt, new_id) for k in range(Et.shape[0])]
            return np.array(rows, np.uint64).reshape(Et.shape[0], len(nxt["nbrs"]))

        old = self.old_tables(move_v, move_e)
        got = self.eng.standing_apply_vertices(rem, add, timing=True)
        assert got[0] == nxt["n"] == self.eng.n and got[1] >= 0.0, (what, got)
        assert self.generation() == gen + (1 if len(rem) or len(add) else 0), (what, "generation")
        off, nb = self.eng.download_csr()
        assert np.array_equal(off, nxt["offsets"]) and np.array_equal(nb, nxt["nbrs"]), (what, "the graph")
        assert np.array_equal(self.eng.download_labels(), nxt["labels"]), (what, "the labels")
        after = {m: match_set(nxt, query, *m) for m in MODES}
        created, destroyed = {}, {}
        for m in MODES:
            kept, gone = through(self.sets[m], new_id)
            assert kept <= after[m], (what, m, "the yardstick: a surviving match is a match of G'")
            created[m], destroyed[m] = after[m] - kept, gone
            added = set(range(nxt["n"] - len(add), nxt["n"]))
            assert all(added & set(r) for r in created[m]), (what, m, "the yardstick: a new match uses an added vertex")
        self.check_rows(what, created, destroyed)
        self.sets, self.g = after, nxt
        self.check_state(what, old)
        return new_id

    def edges(self, what, ins, dele):
        g, query = self.g, self.query
        mid = fs.apply_edges_np(g, [], dele)
        nxt = fs.apply_edges_np(mid, ins, [])
        old = self.old_tables(None, lambda Et: sc.moved_by_key(Et, g, nxt))
        self.eng.standing_apply_edges(insert=ins, delete=dele)
        for h in self.handles:
            sets3 = (self.sets[h.mode], match_set(mid, query, *h.mode), match_set(nxt, query, *h.mode))
            check_batch(h.sq, query, h.mode, sets3, what)
            self.sets[h.mode] = sets3[2]
        self.g = nxt
        self.check_state(what, old)


def telling(g, query, candidates, change):
    """of the candidate batches the one that moves most matches (by the yardstick alone)"""
    M = match_set(g, query, False, False)
    return max(candidates, key=lambda c: len(match_set(change(g, c), query, False, False) ^ M))


@pytest.mark.parametrize("name,l", CASES)
def test_gpu_label_and_vertex_batches_against_brute_force(oracle, tmp_path, name, l):
    g0 = fs.make_graph(hub_deg=64)
    query = QUERIES[name]
    qlabels = sorted(set(query[2]))
    run = Run(oracle, tmp_path, name, l, g0)
    rng = np.random.default_rng(500 + len(name) + l)
    hub = HUB

    def other(v, k=1):
        return (int(run.g["labels"][v]) + k) % NL

    # ---- relabel batches ----
    cands = [int(v) for v in rng.choice(300, 30, replace=False) if v != ISOLATED]
    v = telling(run.g, query, cands, lambda g, v: relabelled(g, [v], [qlabels[0] if g["labels"][v] != qlabels[0] else (qlabels[-1] + 1) % NL]))
    run.relabel("one vertex", [v], [qlabels[0] if run.g["labels"][v] != qlabels[0] else (qlabels[-1] + 1) % NL])
    run.relabel("the hub", [hub], [0])
    w = int(fs.nbrs_of(run.g, hub)[3])
    run.relabel("a hub neighbour", [w], [other(w)])
    run.relabel("the hub back, listed twice", [hub, hub], [1, 1])
    run.relabel("the isolated vertex", [ISOLATED], [1 if run.g["labels"][ISOLATED] != 1 else 0])
    R = sorted(rng.choice(301, 65, replace=False).tolist())
    run.relabel("65 vertices", R, [other(x, 1 + i % 3) for i, x in enumerate(R)])
    R = sorted(rng.choice(301, 40, replace=False).tolist())
    run.relabel("only no-ops", R, run.g["labels"][R])
    run.relabel("count == 0", [], [])
    labels = [other(x) if i % 3 == 0 else int(run.g["labels"][x]) for i, x in enumerate(R)]
    run.relabel("no-ops among real changes", R, labels)
    lab = qlabels[0]
    R = np.flatnonzero(run.g["labels"] == lab).tolist()
    run.relabel("a label leaves the graph: C(u) is empty", R, [(qlabels[-1] + 1) % NL] * len(R))
    assert run.handles[0].sq.count == 0 and 0 in list(run.handles[0].sq.set_sizes())
    run.relabel("and comes back", R, [lab] * len(R))
    assert run.handles[0].sq.count > 0

    # ---- vertex batches ----
    free = next(v for v in range(300) if (v, hub) not in run.g["edges"] and v != ISOLATED and run.g["labels"][v] == 0)
    run.edges("hub 64 -> 65", [(free, hub)], [])
    assert ds.deg_of(run.g)[hub] == 65
    new_id = run.vertices("a hub neighbour leaves: 65 -> 64", [int(fs.nbrs_of(run.g, hub)[10])], [])
    hub = int(new_id[hub])
    assert ds.deg_of(run.g)[hub] == 64 and run.g["n"] == 300
    new_id = run.vertices("add only: n over 320", [], [i % NL for i in range(25)])
    hub = int(new_id[hub])
    assert run.g["n"] == 325
    n = run.g["n"]
    new_id = run.vertices("vertices 0 and n - 1 leave", [0, n - 1], [])
    hub = int(new_id[hub])
    rem = [int(x) for x in rng.choice(run.g["n"], 3, replace=False) if x != hub]
    new_id = run.vertices("remove and add in one batch", rem + rem[:1], [1, 0])
    hub = int(new_id[hub])
    run.vertices("the hub leaves", [hub], [])
    rem = sorted(rng.choice(run.g["n"], 40, replace=False).tolist())
    run.vertices("n under 320 and under 288", rem, [])
    assert run.g["n"] < 288
    run.vertices("the empty batch", [], [])
    # edges naming vertices of the new numbering, the last ones among them
    n = run.g["n"]
    el = {(query[2][a], query[2][b]) for a, b in query[1]} | {(query[2][b], query[2][a]) for a, b in query[1]}
    lab = run.g["labels"]
    ins = [(a, b) for a in range(n - 12, n) for b in range(0, n - 12, 7)
           if (a, b) not in run.g["edges"] and (b, a) not in run.g["edges"] and ((int(lab[a]), int(lab[b])) in el or not el)][:12]
    ins = sorted((min(a, b), max(a, b)) for a, b in ins)
    dele = sorted(run.g["edges"])[5:9]
    run.edges("edges at the new ids", ins, dele)
    run.eng.close()
    if query[0] > 1:
        assert run.moved[0] > 0 and run.moved[1] > 0 and run.changed > 0, (name, l, "nothing created or destroyed: the test shows nothing", run.moved)
    else:
        assert run.moved.sum() > 0 and run.changed > 0, (name, l, run.moved)


def test_gpu_two_handles_one_keeping_e(oracle, tmp_path):
    """two queries on one context, one of the handles keeping E, through a relabel and a vertex batch"""
    g = fs.make_graph(hub_deg=64)
    eng = fs.open_engine(g, E)
    tri, c4 = write_query(tmp_path, "triangle"), write_query(tmp_path, "c4")
    a = eng.standing_open(tri, l=2, rows_cap=BIG)
    b = eng.standing_open(c4, l=3, distinct=True, induced=True, rows_cap=BIG)
    b.keep_counts(vertex=False, edge=True, changes_cap=BIG)
    cases = ((a, "triangle", (False, False)), (b, "c4", (True, True)))
    R = [int(x) for x in fs.nbrs_of(g, HUB)[:20]]
    labels = [(int(g["labels"][x]) + 1) % NL for x in R]
    g1 = relabelled(g, R, labels)
    eng.standing_set_labels(R, labels)
    for sq, name, m in cases:
        M0, M1 = (match_set(x, QUERIES[name], *m) for x in (g, g1))
        check_batch(sq, QUERIES[name], m, (M0, M1, M1), (name, "relabel"))
    rem = [HUB, 3, 4]
    g2, new_id = fs.apply_vertices_np(g1, rem, [1, 0, 1])
    old = ds.carry_tags(g1, b.counts("edge")[0], g2, new_id)
    assert eng.standing_apply_vertices(rem, [1, 0, 1]) == g2["n"]
    moved = 0
    for sq, name, m in cases:
        kept, gone = through(match_set(g1, QUERIES[name], *m), new_id)
        M2 = match_set(g2, QUERIES[name], *m)
        count, created, destroyed = sq.result()[:3]
        assert (count, created, destroyed) == (len(M2), len(M2 - kept), len(gone)), (name, "vertices")
        assert as_mode(sq.rows(1), QUERIES[name], m[0]) == sorted(gone) and as_mode(sq.rows(0), QUERIES[name], m[0]) == sorted(M2 - kept)
        moved += destroyed
    assert moved > 0
    Et = b.counts("edge")
    assert Et.shape == (4, len(g2["nbrs"])) and (Et.sum(axis=1) == b.count).all()
    assert np.array_equal(Et, sc.fresh_tables(g2, c4, QUERIES["c4"])[True, True][1]), "E against the one-shot table"
    diff = Et[0] - old
    cells, deltas = b.count_changes("edge")
    first = cells < len(g2["nbrs"])  # the cells of query edge 0
    assert np.array_equal(cells[first], np.flatnonzero(diff)) and np.array_equal(deltas[first], diff[np.flatnonzero(diff)].view(np.int64))
    with pytest.raises(Exception, match="keep_counts"):
        a.counts("vertex")
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def refusal_setup(tmp_path):
    g = fs.make_graph(hub_deg=64)
    qp = write_query(tmp_path, "c4")
    eng = fs.open_engine(g, E)
    handles = []
    for mode, l, keeps in (((False, False), 2, ["vertex", "edge"]), ((True, True), 3, ["vertex"])):
        sq = eng.standing_open(qp, l=l, distinct=mode[0], induced=mode[1], rows_cap=BIG)
        sq.keep_counts(vertex=True, edge="edge" in keeps, changes_cap=BIG)
        handles.append(tds.Handle(sq, mode, l, keeps))
    # a good batch first, so that rows are kept and the change lists are not empty
    R = [int(x) for x in fs.nbrs_of(g, HUB)[:12]]
    labels = [(int(g["labels"][x]) + 1) % NL for x in R]
    eng.standing_set_labels(R, labels)
    assert all(h.sq.result()[2] > 0 and h.sq.n_changes("vertex") > 0 for h in handles), "the good batch destroyed nothing: the snapshots show little"
    return eng, handles, relabelled(g, R, labels), qp


def test_gpu_refused_relabels_change_nothing(oracle, tmp_path):
    from gnnpe_amd import binding
    eng, handles, g, qp = refusal_setup(tmp_path)
    n = g["n"]
    before = tds.snapshot_a(eng, handles)
    refused = {
        "an id >= n": ([3, n], [1, 1], str(n), "-1"),
        "one vertex with two labels": ([3, 9, 3], [1, 1, 2], "labels 1 and 2", "-1"),
        "a label outside the label table": ([3, 9], [1, NL], "label table", "-1"),
    }
    for what, (R, labels, msg, code) in refused.items():
        with pytest.raises(binding.GnnpeError, match=msg) as err:
            eng.standing_set_labels(R, labels)
        assert f"[{code}]" in str(err.value), (what, str(err.value))
        assert tds.snapshot_a(eng, handles) == before, (what, "a refused relabel changed something")
    rc = binding.load_online().gnnpe_standing_set_labels(eng.ctx, None, None, 2, None)
    assert rc == -1 and tds.snapshot_a(eng, handles) == before
    # a stale handle: refused before the labels are touched
    eng.apply_edges(delete=sorted(g["edges"])[:1])
    labels = eng.download_labels().tobytes()
    with pytest.raises(binding.GnnpeError, match=tds.STALE):
        eng.standing_set_labels([3], [(int(g["labels"][3]) + 1) % NL])
    assert eng.download_labels().tobytes() == labels
    # the handles go on exactly after a refresh
    g = fs.apply_edges_np(g, [], sorted(g["edges"])[:1])
    eng.vde(want=False)
    for h in handles:
        h.sq.refresh()
    R, new = [3, 9, HUB], [(int(g["labels"][x]) + 2) % NL for x in (3, 9, HUB)]
    eng.standing_set_labels(R, new)
    g2 = relabelled(g, R, new)
    plan = {l: binding.host_query_plan_exact(qp, E, l) for l in (2, 3)}
    vde = fs.vde_of(oracle, g2, E)
    for h in handles:
        M0, M1 = (match_set(x, QUERIES["c4"], *h.mode) for x in (g, g2))
        check_batch(h.sq, QUERIES["c4"], h.mode, (M0, M1, M1), "after the refusals")
        assert np.array_equal(h.sq.table(), fs.np_support(g2, vde, plan[h.l]))
    eng.close()


def test_gpu_refused_vertex_batches_change_nothing(oracle, tmp_path):
    from gnnpe_amd import binding
    eng, handles, g, qp = refusal_setup(tmp_path)
    n = g["n"]
    before = tds.snapshot_a(eng, handles)
    refused = {
        "an id >= n": ([3, n], [1], str(n), "-1"),
        "every vertex": (list(range(n)), [], "leaves no vertex", "-1"),
        "an added label outside the label table": ([3], [0, NL], "label table", "-1"),
    }
    for what, (rem, add, msg, code) in refused.items():
        with pytest.raises(binding.GnnpeError, match=msg) as err:
            eng.standing_apply_vertices(rem, add)
        assert f"[{code}]" in str(err.value), (what, str(err.value))
        assert eng.n == n and tds.snapshot_a(eng, handles) == before, (what, "a refused vertex batch changed something")
    rc = binding.load_online().gnnpe_standing_apply_vertices(eng.ctx, None, 2, None, 0, None, None)
    assert rc == -1 and tds.snapshot_a(eng, handles) == before
    # an open_sets handle on the context: its bitmap was made for the old n
    third = eng.standing_open(qp, bitmap=pack(np.array([g["labels"] == lb for lb in QUERIES["c4"][2]])), rows_cap=10)
    with pytest.raises(binding.GnnpeError, match="gnnpe_standing_open_sets") as err:
        eng.standing_apply_vertices([3], [1])
    assert "[-3]" in str(err.value) and tds.snapshot_a(eng, handles) == before
    # ... which a relabel takes along, under the caller's promise (a bitmap of all ones keeps it)
    third.close()
    ones = np.full((4, (n + 31) // 32), 0xFFFFFFFF, np.uint32)
    third = eng.standing_open(qp, bitmap=ones, rows_cap=BIG)
    R, new = [3, 9, HUB], [(int(g["labels"][x]) + 2) % NL for x in (3, 9, HUB)]
    eng.standing_set_labels(R, new)
    g1 = relabelled(g, R, new)
    M0, M1 = (match_set(x, QUERIES["c4"], False, False) for x in (g, g1))
    check_batch(third, QUERIES["c4"], (False, False), (M0, M1, M1), "the open_sets handle through a relabel")
    third.close()
    # a stale handle: refused before the graph is touched
    eng.set_vertex_labels([5], [(int(g1["labels"][5]) + 1) % NL])
    off = eng.download_csr()[0].tobytes()
    with pytest.raises(binding.GnnpeError, match=tds.STALE):
        eng.standing_apply_vertices([3], [1])
    assert eng.download_csr()[0].tobytes() == off and eng.n == n
    g1 = relabelled(g1, [5], [(int(g1["labels"][5]) + 1) % NL])
    eng.vde(want=False)
    for h in handles:
        h.sq.refresh()
    # the handles go on exactly
    g2, new_id = fs.apply_vertices_np(g1, [3, HUB], [1, 1])
    assert eng.standing_apply_vertices([3, HUB], [1, 1]) == g2["n"]
    plan = {l: binding.host_query_plan_exact(qp, E, l) for l in (2, 3)}
    vde = fs.vde_of(oracle, g2, E)
    for h in handles:
        kept, gone = through(match_set(g1, QUERIES["c4"], *h.mode), new_id)
        M2 = match_set(g2, QUERIES["c4"], *h.mode)
        assert h.sq.result()[:3] == (len(M2), len(M2 - kept), len(gone)), h.mode
        assert np.array_equal(h.sq.table(), fs.np_support(g2, vde, plan[h.l]))
    eng.close()


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,mode", [([], (False, False)), (["-l", "3", "--refine", "sets", "--induced", "--distinct"], (True, True))])
def test_gpu_cli_standing_all_three_kinds(tmp_path, test_graph, flags, mode):
    """gnnpe_main -m online --exact --standing with an edge batch, a relabel, a vertex batch and an edge batch naming the new ids in
    one command line, applied in that order: the `standing:` lines against the library's answers for the same batches and against
    brute force"""
    import os
    import subprocess
    import test_online_exact as base
    from conftest import GOLDEN
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    qp = os.path.join(base.ONLINE, "q1.graph")
    lines = [ln.split() for ln in open(qp)]
    query = (int(lines[0][1]), {(int(ln[1]), int(ln[2])) for ln in lines if ln[0] == "e"}, [int(ln[2]) for ln in lines if ln[0] == "v"])
    n = len(test_graph["labels"])
    und = {(v, int(w)) for v in range(n) for w in test_graph["nbrs"][test_graph["offsets"][v]:test_graph["offsets"][v + 1]] if v < w}
    g0 = fs.graph_of(n, und, test_graph["labels"])
    n_labels = int(g0["labels"].max()) + 1
    rng = np.random.default_rng(23)
    rows = embeddings_of(g0, query)
    used = np.unique(rows) if len(rows) else np.arange(n)
    # the batches: delete edges of matches, relabel vertices of matches (with a no-op among them), remove two of them and add three
    el = {(query[2][x], query[2][y]) for x, y in query[1]} | {(query[2][y], query[2][x]) for x, y in query[1]}
    have = [e for e in sorted(g0["edges"]) if (int(g0["labels"][e[0]]), int(g0["labels"][e[1]])) in el]
    dele = [have[int(j)] for j in rng.choice(len(have), 8, replace=False)]
    ins = []
    while len(ins) < 8:
        a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False))
        if (a, b) not in g0["edges"] and (a, b) not in ins and (int(g0["labels"][a]), int(g0["labels"][b])) in el:
            ins.append((a, b))
    g1 = fs.apply_edges_np(fs.apply_edges_np(g0, [], dele), ins, [])
    R = [int(v) for v in rng.choice(used, 6, replace=False)]
    new = [(int(g1["labels"][v]) + 1) % n_labels for v in R[:5]] + [int(g1["labels"][R[5]])]
    g2 = relabelled(g1, R, new)
    rem = [int(v) for v in rng.choice(used, 2, replace=False)]
    add = [query[2][0], query[2][1], query[2][0]]
    g3, new_id = fs.apply_vertices_np(g2, rem, add)
    n3 = g3["n"]
    ins3 = [(a, n3 - 1 - k) for k in range(3) for a in rng.choice(n3 - 3, 4, replace=False).tolist()]
    ins3 = sorted({(int(min(a, b)), int(max(a, b))) for a, b in ins3} - g3["edges"])
    g4 = fs.apply_edges_np(g3, ins3, [])
    files = [str(tmp_path / f"batch{i}.txt") for i in range(4)]
    open(files[0], "w").write("".join(f"+ {a} {b}\n" for a, b in ins) + "".join(f"- {a} {b}\n" for a, b in dele))
    open(files[1], "w").write("".join(f"{v} {lab}\n" for v, lab in zip(R, new)))
    open(files[2], "w").write("".join(f"- {v}\n" for v in rem) + "".join(f"+ {lab}\n" for lab in add))
    open(files[3], "w").write("".join(f"+ {a} {b}\n" for a, b in ins3))
    # the library's answers
    eng = binding.Engine(0)
    eng.load_csr(g0["offsets"], g0["nbrs"], g0["labels"])
    eng.set_label_table(binding.host_label_table(n_labels, E))
    eng.vde(want=False)
    sq = eng.standing_open(qp, l=3 if flags else 2, distinct=mode[0], induced=mode[1])
    want = [sq.result()[:3]]
    eng.standing_apply_edges(insert=ins, delete=dele)
    want.append(sq.result()[:3])
    eng.standing_set_labels(R, new)
    want.append(sq.result()[:3])
    eng.standing_apply_vertices(rem, add)
    want.append(sq.result()[:3])
    eng.standing_apply_edges(insert=ins3)
    want.append(sq.result()[:3])
    eng.close()
    # ... which are the brute force's counts
    assert [w[0] for w in want] == [len(match_set(x, query, *mode)) for x in (g0, g1, g2, g3, g4)], want
    assert sum(w[1] for w in want) > 0 and sum(w[2] for w in want) > 0, want
    root = base._dataset(tmp_path, graph)
    cmd = [base.CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--exact", "--standing"] + flags
    cmd += ["--apply-edges", files[0], "--set-labels", files[1], "--apply-vertices", files[2], "--apply-edges", files[3]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("standing: ")]
    assert [tuple(int(x) for x in ln[1:4]) for ln in out] == want, (out, want)
    assert all(float(ln[4]) >= 0 for ln in out)
    # --incremental still does not go with --standing
    r = subprocess.run(cmd + ["--incremental"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--standing" in r.stderr + r.stdout


def embeddings_of(g, query):
    from test_standing_query import embeddings
    return embeddings(g, query, False)


def test_gpu_no_handle_plain_calls_and_noop_views(tmp_path):
    """a context without a handle gets the plain relabel / vertex batch and gnnpe_vde (a handle opened afterwards needs nothing more);
    with a handle, a batch of nothing but no-ops leaves the binding's device views valid, a real one ends them"""
    g = fs.make_graph(hub_deg=64)
    query = QUERIES["wedge"]
    qp = write_query(tmp_path, "wedge")
    eng = fs.open_engine(g, E)
    R, new = [3, HUB], [(int(g["labels"][3]) + 1) % NL, 0]
    eng.standing_set_labels(R, new)
    g1 = relabelled(g, R, new)
    assert np.array_equal(eng.download_labels(), g1["labels"])
    g2, _ = fs.apply_vertices_np(g1, [5, 9], [1, 0, 1])
    assert eng.standing_apply_vertices([5, 9], [1, 0, 1]) == g2["n"] == eng.n
    off, nb = eng.download_csr()
    assert np.array_equal(off, g2["offsets"]) and np.array_equal(nb, g2["nbrs"]) and np.array_equal(eng.download_labels(), g2["labels"])
    sq = eng.standing_open(qp, l=2)  # needs a current gnnpe_vde: the two calls left one
    assert sq.count == len(match_set(g2, query, False, False))
    gen, views = sq.result()[5], eng._rows_gen
    same = [7, 8, 11]
    eng.standing_set_labels(same, g2["labels"][same])
    assert sq.result()[5] == gen and eng._rows_gen == views, "a batch of no-ops ended the device views"
    eng.standing_set_labels(same, (g2["labels"][same] + 1) % NL)
    assert sq.result()[5] == gen + 1 and eng._rows_gen == views + 1
    assert sq.count == len(match_set(relabelled(g2, same, (g2["labels"][same] + 1) % NL), query, False, False))
    eng.close()
