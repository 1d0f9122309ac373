"""Random update sessions with the standing handles carried through EVERY kind of update: the kind-"A" sessions of
tests/dynamic_session.py replayed with relabel steps through gnnpe_standing_set_labels and vertex steps through
gnnpe_standing_apply_vertices, where tests/test_dynamic_sessions.py lets them happen behind the handles' backs and refreshes.

After every step the engine and the two handles (mode 0 at l = 2 keeping V and E, DISTINCT | INDUCED at l = 3 keeping V) are held
to the model, to the brute force and to a fresh engine as run_a of that file holds them: count, created, destroyed and both row
lists, S, C, the set sizes, the kept tables, their change lists, the graph.  Only an offline pass (which sets an order and a label
table) still leaves the handles stale; the next step refreshes them.  The open / close steps of the generator (its open_sets
handle) are passed over: a vertex batch refuses such a handle, which tests/test_standing_updates.py checks.

The CPU test asserts on the model alone that the seeds reach a relabel next to a row of more than 64 entries, a removal of the
hub, n across a multiple of 32 in both directions, and a vertex step directly followed by an edge step and by a relabel."""
import numpy as np
import pytest

import dynamic_session as ds
import test_dynamic_sessions as tds
import test_filter_support as fs
import test_standing_counts as sc
from test_standing_query import QUERIES, match_set, as_mode, check_batch, write_query
from test_standing_updates import through, relabelled

E, BIG = ds.E, tds.BIG
SEEDS = [285, 292, 309, 323, 335, 338, 339, 351]
MOVES = ("edges", "edges_hub", "empty", "vertices", "relabel")


def test_update_sessions_cover_what_they_are_for():
    sessions = [ds.session("A", s) for s in SEEDS]
    c = ds.coverage(sessions)
    assert c["relabel_at_long_row"] > 0, "no relabel at a row of more than 64 entries"
    assert c["n32_up"] > 0 and c["n32_down"] > 0, ("n across a multiple of 32", c["n32_up"], c["n32_down"])
    assert ("vertices", "edges") in c["pairs"] and ("vertices", "relabel") in c["pairs"], sorted(c["pairs"])
    hub_removed = 0
    for s in sessions:
        hub = s["hub"]
        for st in s["steps"]:
            hub_removed += st["kind"] == "vertices" and hub >= 0 and st["hub"] < 0
            hub = st["hub"]
    assert hub_removed > 0, "the hub is never removed"
    assert {s["qname"] for s in sessions} == set(ds.QNAMES)
    kinds = [st["kind"] for s in sessions for st in s["steps"]]
    assert kinds.count("relabel") >= 8 and kinds.count("vertices") >= 8 and kinds.count("refused") >= 2, kinds


def run_session(oracle, tmp_path, seed):
    from gnnpe_amd import binding
    s = ds.session("A", seed)
    name, query = s["qname"], QUERIES[s["qname"]]
    qp = write_query(tmp_path, name)
    plans = {l: binding.host_query_plan_exact(qp, E, l) for l in (2, 3)}
    g = s["g0"]
    eng, fresh = fs.open_engine(g, E), tds.Fresh()
    handles = []
    for mode, l, keep_e in tds.HANDLES:
        sq = eng.standing_open(qp, l=l, distinct=mode[0], induced=mode[1], rows_cap=BIG)
        sq.keep_counts(vertex=True, edge=keep_e, changes_cap=BIG)
        handles.append(tds.Handle(sq, mode, l, ["vertex", "edge"] if keep_e else ["vertex"]))
    sets = {h.mode: match_set(g, query, *h.mode) for h in handles}
    stale = False
    moved = np.zeros(2, np.int64)

    def check_exact(graph, what, old):
        """every handle against the brute force on `graph`; old: {handle: the tables of before in the cells of `graph`}; None
        after an open or a refresh, whose rows and change lists must be empty; "kept": after keep_counts, which leaves the rows"""
        vde = fs.vde_of(oracle, graph, E)
        Y, ft = sc.yardstick(graph, query), sc.fresh_tables(graph, qp, query)
        for h in handles:
            assert h.sq.count == len(sets[h.mode]), (what, h.mode, "count")
            assert np.array_equal(h.sq.table(), fs.np_support(graph, vde, plans[h.l])), (what, h.mode, "S")
            bits = fs.fresh_bits(graph, E, plans[h.l])
            bm = h.sq.bitmap()
            assert np.array_equal(fs.bits_of(bm, graph["n"]), bits), (what, h.mode, "C against the fresh filter")
            assert bm.shape[1] == (graph["n"] + 31) // 32 and (graph["n"] % 32 == 0 or not np.any(bm[:, -1] >> np.uint32(graph["n"] % 32)))
            assert list(h.sq.set_sizes()) == list(bits.sum(axis=1)), (what, h.mode, "sizes")
            new = tds.check_kept(h, graph, query, Y, ft, what)
            if old is None:
                assert h.sq.result()[1:5] == (0, 0, 0, 0), (what, h.mode, "rows after a refresh")
                assert all(h.sq.n_changes(w) == 0 for w in h.keeps), (what, "change lists after a refresh")
            elif old != "kept":
                for w in sorted(h.keeps):
                    sc.check_changes(h.sq, w, old[id(h)][w], new[w], (what, h.mode, w))
            h.tables = new

    def refresh(graph, what):
        nonlocal stale, sets
        eng.vde(want=False)
        sets = {h.mode: match_set(graph, query, *h.mode) for h in handles}
        for h in handles:
            assert h.sq.refresh() == len(sets[h.mode]), (what, h.mode, "refresh")
        stale = False
        check_exact(graph, (what, "refresh"), None)

    def check_rows(what, created, destroyed):
        for h in handles:
            c, d = sorted(created[h.mode]), sorted(destroyed[h.mode])
            assert h.sq.result()[1:5] == (len(c), len(d), len(c), len(d)), (what, h.mode, h.sq.result(), len(c), len(d))
            assert as_mode(h.sq.rows(0), query, h.mode[0]) == c and as_mode(h.sq.rows(1), query, h.mode[0]) == d, (what, h.mode, "rows")
        moved[:] += (len(created[False, False]), len(destroyed[False, False]))

    check_exact(g, "open", None)
    for i, st in enumerate(s["steps"]):
        kind, nxt = st["kind"], st["g"]
        what = ("A", seed, i, kind)
        if kind in MOVES + ("keep_counts",) and stale:
            refresh(g, what)
        gen = None if stale else handles[0].sq.result()[5]
        if kind in ("edges", "edges_hub", "empty"):
            ins, dele = st.get("ins", []), st.get("dele", [])
            mid = fs.apply_edges_np(g, [], dele)
            old = {id(h): {w: (sc.moved_by_key(t, g, nxt) if w == "edge" else t) for w, t in h.tables.items()} for h in handles}
            eng.standing_apply_edges(insert=ins, delete=dele)
            assert handles[0].sq.result()[5] == gen + (2 if ins and dele else 1 if ins or dele else 0), (what, "generation")
            for h in handles:
                sets3 = (sets[h.mode], match_set(mid, query, *h.mode), match_set(nxt, query, *h.mode))
                got = check_batch(h.sq, query, h.mode, sets3, what)
                if h.mode == (False, False):
                    moved[:] += got
                sets[h.mode] = sets3[2]
            check_exact(nxt, what, old)
        elif kind == "relabel":
            old = {id(h): dict(h.tables) for h in handles}
            eng.standing_set_labels(st["R"], st["labels"])
            assert handles[0].sq.result()[5] == gen + 1, (what, "generation")
            after = {m: match_set(nxt, query, *m) for m in sets}
            check_rows(what, {m: after[m] - sets[m] for m in sets}, {m: sets[m] - after[m] for m in sets})
            sets = after
            check_exact(nxt, what, old)
        elif kind == "vertices":
            new_id = st["new_id"]
            keep = np.flatnonzero(new_id >= 0)
            old = {}
            for h in handles:
                V = np.zeros((h.tables["vertex"].shape[0], nxt["n"]), np.uint64)
                V[:, new_id[keep]] = h.tables["vertex"][:, keep]
                old[id(h)] = dict(vertex=V)
                if "edge" in h.tables:
                    Et = h.tables["edge"]
                    old[id(h)]["edge"] = np.array([ds.carry_tags(g, Et[k], nxt, new_id) for k in range(len(Et))], np.uint64).reshape(len(Et), -1)
            assert eng.standing_apply_vertices(st["rem"], st["add"]) == nxt["n"], what
            assert handles[0].sq.result()[5] == gen + 1, (what, "generation")
            after = {m: match_set(nxt, query, *m) for m in sets}
            created, destroyed = {}, {}
            for m in sets:
                kept, destroyed[m] = through(sets[m], new_id)
                assert kept <= after[m], (what, m, "the yardstick")
                created[m] = after[m] - kept
            check_rows(what, created, destroyed)
            sets = after
            check_exact(nxt, what, old)
        elif kind == "offline":
            tds.offline_pass(eng, g, oracle, what)
            stale = True
            with pytest.raises(binding.GnnpeError, match=tds.STALE):
                eng.standing_set_labels([0], [int(g["labels"][0]) ^ 1])
            with pytest.raises(binding.GnnpeError, match=tds.STALE):
                eng.standing_apply_vertices([0], [])
            assert np.array_equal(eng.download_labels(), g["labels"]) and eng.n == g["n"], (what, "a refused call touched the graph")
        elif kind == "refused":
            if stale:
                tds.refused_call(eng, st, False)
            else:
                before = tds.snapshot_a(eng, handles)
                with pytest.raises(binding.GnnpeError, match=st["msg"]) as err:
                    if st["why"] == "all":
                        eng.standing_apply_vertices(st["rem"], st["add"])
                    else:
                        eng.standing_apply_edges(insert=st["ins"], delete=st["dele"])
                assert "[-1]" in str(err.value), str(err.value)
                assert tds.snapshot_a(eng, handles) == before, (what, st["why"], "a refused batch changed something")
        elif kind == "refresh":
            refresh(g, what)
        elif kind == "keep_counts":
            h = handles[1]
            if "edge" not in h.keeps:
                h.sq.keep_counts(vertex=False, edge=True, changes_cap=BIG)
                h.keeps.add("edge")  # E is built on the graph as it is now; V stays
            else:
                handles[0].sq.keep_counts(vertex=True, edge=True, changes_cap=BIG + i)  # a new cap: the tables stay, the lists are emptied
                assert all(handles[0].sq.n_changes(w) == 0 for w in ("vertex", "edge")), what
            check_exact(g, what, "kept")
        tds.check_graph(eng, fresh, nxt, what)
        g = nxt
    if stale:
        refresh(g, ("A", seed, "end"))
    eng.close()
    fresh.close()
    return moved


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_update_session(oracle, tmp_path, seed):
    run_session(oracle, tmp_path, seed)
