"""Random update sessions on the resident graph against numpy and fresh engines: every kind of update after every other.

The files of the update calls script one kind of update each; what they share -- the generations, the validity flags, the derived
rows, grow-only buffers with the tile counts of the previous graph, bitmap widths of ceil(n / 32) words -- goes wrong only when
one kind follows another.  tests/dynamic_session.py draws sessions of ten steps (edge batches, one edge at the hub, vertex batches,
relabels, empty and refused batches, an offline pass) against a numpy model; here each session is replayed on one engine and after
EVERY step the engine is held to the model, to the brute force of tests/test_standing_query.py and tests/test_standing_counts.py,
to np_support / fresh_bits of tests/test_filter_support.py and to a fresh engine that loaded the model graph.

Kind A: standing handles stay open (mode 0 at l = 2 keeping V and E; DISTINCT | INDUCED at l = 3 keeping V; sometimes an open_sets
handle with the label bitmap); edge batches go through standing_apply_edges, everything else happens behind the handles' backs.
Kind B: no handles; the caller keeps a support table by the three recipes of include/gnnpe_hip.h, a tag per vertex and a tag per
entry through the carries, and a MatchCursor.

The CPU tests assert, from the generator and the model alone, that the chosen seeds reach what the sessions are for (every ordered
pair of update kinds, the hub row across 64 / 65, n across a word edge, the entries across 2048 and under 1024, matches gained and
lost, candidate sets moved).

Wall time on one MI355X (pytest --durations, the call phase), run beside tests/test_standing_counts.py::
test_gpu_counts_loop_against_brute_force, which is unchanged: its slowest case (path3-2) took 0.22 - 0.34 s over five runs; the kind-A sessions
0.07 - 0.22 s (slowest: seed 0), the kind-B sessions 0.06 - 0.10 s (slowest: seed 0).  No session may take more than twice the
slowest case of that test."""
import ctypes as C

import numpy as np
import pytest

import dynamic_session as ds
import test_csr_apply_vertices as av
import test_filter_support as fs
import test_standing_counts as sc
import test_standing_query as sqt
from test_standing_query import QUERIES, match_set, two_step, check_batch, write_query, pack

E, NL, BIG = ds.E, ds.NL, 1 << 18
SEEDS = {"A": [0, 131, 338, 477, 480, 664, 672, 686], "B": [0, 6, 41, 150, 299, 409, 416, 428]}
STANDING = ("edges", "edges_hub", "empty")
STALE = "gnnpe_standing_refresh"


def label_bits(g, query):
    return np.array([g["labels"] == lb for lb in query[2]])


HANDLES = [((False, False), 2, True), ((True, True), 3, False)]  # (mode, l, keeps E) of the two handles every kind-A session opens


def plan_b(g0, seed, tmp_path):
    """the plan whose support table a kind-B session keeps: the cut query at l = 2, the star at l = 3 on alternate seeds"""
    l, which = ((2, 0), (3, 1))[seed % 2]
    return fs.make_plans(g0, E, l, tmp_path, 31)[which]


def branch_counters():
    return dict(third_batches=0, third_refresh_ok=0, third_refresh_after_relabel=0, third_refresh_refused=0, new_cap=0, refused_current=set(),
                refused_stale=0)


def replay_a(s):
    """what run_a does with the steps of a kind-A session, from the model alone: how often its rarer branches run.  This follows
    run_a's control flow by hand; run_a counts the same branches as it takes them (`taken`) and ends by comparing the two."""
    c = branch_counters()
    st8 = dict(stale=False, third=None, relabelled=False, keeps_e=False)
    n = s["g0"]["n"]

    def refresh():
        if st8["third"] is not None:
            if st8["third"] != n:
                c["third_refresh_refused"] += 1
                st8["third"] = None
            else:
                c["third_refresh_ok"] += 1
                c["third_refresh_after_relabel"] += st8["relabelled"]
                st8["relabelled"] = False
        st8["stale"] = False

    for st in s["steps"]:
        kind = st["kind"]
        if kind in STANDING + ("open", "keep_counts") and st8["stale"]:
            refresh()
        if kind in STANDING:
            c["third_batches"] += st8["third"] is not None
        elif kind in ("vertices", "relabel", "offline"):
            st8["stale"] = True
            st8["relabelled"] = st8["relabelled"] or (kind == "relabel" and st8["third"] is not None)
        elif kind == "refused":
            if st8["stale"] or st["why"] == "all":
                c["refused_stale"] += st8["stale"]
            if not st8["stale"]:
                c["refused_current"].add(st["why"])
        elif kind == "refresh":
            refresh()
        elif kind == "open":
            st8["third"], st8["relabelled"] = n, False
        elif kind == "close":
            st8["third"] = None
        elif kind == "keep_counts":
            c["new_cap"] += st8["keeps_e"]
            st8["keeps_e"] = True
        n = st["g"]["n"]
    if st8["stale"]:
        refresh()
    return c


# ---- CPU: the generator and what its sessions cover ---------------------------------------------------------------------------------

def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items() if k != "edges"}
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


@pytest.mark.parametrize("kind", ["A", "B"])
def test_generator_is_deterministic(kind):
    for seed in SEEDS[kind]:
        first = _plain(ds.session(kind, seed))
        ds._SESSIONS.pop((kind, seed))
        assert _plain(ds.session(kind, seed)) == first, (kind, seed)
        assert len(ds.session(kind, seed)["steps"]) == ds.STEPS


def test_session_seeds_differ():
    kinds = {k: [tuple(st["kind"] for st in ds.session(k, s)["steps"]) for s in SEEDS[k]] for k in "AB"}
    assert all(len(set(v)) == len(v) >= 8 for v in kinds.values()), kinds


@pytest.mark.parametrize("kind", ["A", "B"])
def test_sessions_cover_what_they_are_for(kind):
    """the graph-shaped conditions, over the seeds of each kind, with the measured value in the message"""
    sessions = [ds.session(kind, s) for s in SEEDS[kind]]
    c = ds.coverage(sessions)
    want = {(a, b) for a in ds.STRUCT for b in ds.STRUCT}
    assert c["pairs"] >= want, ("ordered pairs of update kinds never seen", sorted(want - c["pairs"]))
    want = {(a, b) for a in ds.STRUCT for b in ("refused", "empty")}
    assert c["then"] >= want, ("never followed by", sorted(want - c["then"]))
    for key in ("hub_up", "hub_down", "hub_down_by_removal", "relabel_at_long_row", "n32_up", "n32_down", "n_320_or_288", "e2048_up",
                "e2048_down", "e1024_down"):
        assert c[key] > 0, (kind, key, c[key], {k: v for k, v in c.items() if isinstance(v, int)})
    if kind == "A":  # the branches of run_a that few sessions reach
        r = [replay_a(s) for s in sessions]
        total = {k: sum(x[k] for x in r) for k in r[0] if k != "refused_current"}
        whys = set().union(*(x["refused_current"] for x in r))
        assert total["third_batches"] >= 3, ("standing batches with the open_sets handle open", total)
        assert total["third_refresh_after_relabel"] >= 1 and total["third_refresh_refused"] >= 1, ("refreshes of the open_sets handle", total)
        assert total["new_cap"] >= 1, ("keep_counts with a new changes_cap", total)
        assert len(whys - {"all"}) >= 2 and total["refused_stale"] >= 1, ("refused through the standing call", sorted(whys), total)
    kinds = {st["kind"] for s in sessions for st in s["steps"]}
    want = set(ds.WEIGHTS_A if kind == "A" else ds.WEIGHTS)
    assert kinds == want, ("step kinds never drawn", sorted(want - kinds))
    assert {s["qname"] for s in sessions} == set(ds.QNAMES), sorted(s["qname"] for s in sessions)
    for s in sessions:
        assert s["hub"] == fs.HUB and ds.deg_of(s["g0"])[fs.HUB] == 64 and 1960 <= len(s["g0"]["nbrs"]) <= 2040
        for st in s["steps"]:
            if st["kind"] in ("edges", "edges_hub"):
                assert 1 <= len(st["ins"]) + len(st["dele"]) <= 40
            if st["kind"] == "vertices":
                assert len(st["rem"]) <= 20 and len(st["add"]) <= 20 and len(st["rem"]) + len(st["add"]) > 0
            if st["kind"] == "relabel":
                assert 1 <= len(st["R"]) <= 15


@pytest.mark.parametrize("kind", ["A", "B"])
def test_vertex_steps_two_yardsticks_agree(kind):
    """fs.apply_vertices_np (the model's) and _apply_np of tests/test_csr_apply_vertices.py, which share no code, on every vertex step"""
    seen = 0
    for seed in SEEDS[kind]:
        s = ds.session(kind, seed)
        g = s["g0"]
        for st in s["steps"]:
            if st["kind"] == "vertices":
                g2, vmap, emap = av._apply_np(g, st["rem"], st["add"])
                assert av._same_graph(st["g"], g2) and g2["n"] == st["g"]["n"], (kind, seed)
                old = vmap != av.NO
                assert np.array_equal(st["new_id"][vmap[old].astype(np.int64)], np.flatnonzero(old)), (kind, seed, "vertex map")
                assert (st["new_id"] >= 0).sum() == old.sum()
                assert np.array_equal(ds.keys_of(g)[emap.astype(np.int64)] // g["n"], vmap[ds.keys_of(g2) // g2["n"]]), (kind, seed, "entry map")
                seen += 1
            g = st["g"]
    assert seen >= 8, seen


def test_sessions_are_telling(oracle, tmp_path):
    """on the brute force alone: in kind A every handle's query gains and loses matches over the standing batches of its session;
    over each kind's seeds a relabel and a vertex batch change a candidate set of the exact filter"""
    from gnnpe_amd import binding
    for kind in "AB":
        moves = {"relabel": fs.Moves(), "vertices": fs.Moves()}
        for seed in SEEDS[kind]:
            s = ds.session(kind, seed)
            query = QUERIES[s["qname"]]
            g = s["g0"]
            plan = binding.host_query_plan_exact(write_query(tmp_path, s["qname"]), E, 2) if kind == "A" else plan_b(g, seed, tmp_path)
            moved = {m: np.zeros(2, np.int64) for m, _, _ in HANDLES}
            for st in s["steps"]:
                if kind == "A" and st["kind"] in ("edges", "edges_hub"):
                    mid = fs.apply_edges_np(g, [], st["dele"])
                    for m in moved:
                        created, destroyed = two_step(*(match_set(x, query, *m) for x in (g, mid, st["g"])))
                        moved[m] += (len(created), len(destroyed))
                if st["kind"] in moves:
                    before, after = (fs.np_support(x, fs.vde_of(oracle, x, E), plan) for x in (g, st["g"]))
                    col_map = None
                    if st["kind"] == "vertices":
                        col_map = np.full(st["g"]["n"], -1, np.int64)
                        col_map[st["new_id"][st["new_id"] >= 0]] = np.flatnonzero(st["new_id"] >= 0)
                    moves[st["kind"]].step(before, after, col_map)
                g = st["g"]
            if kind == "A":
                for m, v in moved.items():
                    assert v[0] > 0 and v[1] > 0, (seed, s["qname"], m, "created, destroyed over the session", v.tolist())
        for what, mv in moves.items():
            assert mv.cleared + mv.set > 0, (kind, what, "no candidate set changed", mv.cleared, mv.set, mv.moved)


# ---- GPU: what both kinds check ---------------------------------------------------------------------------------------------------------

class Fresh:
    """one spare engine that loads the model graph after every step: what the engine under test must be"""

    def __init__(self):
        from gnnpe_amd import binding
        self.eng = binding.Engine(0)

    def load(self, g):
        self.eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        return self.eng

    def close(self):
        self.eng.close()


def check_graph(eng, fresh, g, what):
    off, nb = eng.download_csr()
    assert np.array_equal(off, g["offsets"]) and np.array_equal(nb, g["nbrs"]), (what, "the rows")
    assert np.array_equal(eng.download_labels(), g["labels"]), (what, "the labels")
    assert eng.n == g["n"] and eng.rows_held() == fresh.load(g).rows_held(), (what, "rows_held", eng.rows_held())
    assert eng.rows_held()[:2] == (g["n"], len(g["nbrs"])), (what, "rows_held")


def offline_pass(eng, g, oracle, what):
    """set_order(degree_order), the label table, vde, count_paths(2), fill_paths: x, nx, vde, the ids and pde against the oracle"""
    from gnnpe_amd import binding, synth
    sn = synth.degree_order(g["offsets"])
    eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
    eng.set_label_table(binding.host_label_table(NL, E))
    x, nx, vde = eng.vde()
    ox, onx, ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], E)
    assert np.array_equal(x, ox) and np.array_equal(nx, onx) and np.array_equal(vde, ovde), (what, "vde")
    want = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    assert eng.count_paths(2) == len(want) > 0, (what, "count_paths")
    ids, pde = eng.fill_paths()[:2]
    assert np.array_equal(ids, want), (what, "fill_paths ids")
    assert np.array_equal(pde, ovde[want].reshape(len(want), 3 * E)), (what, "fill_paths pde")
    return sn, (x, nx, vde)


def refused_call(eng, st, standing):
    """the refused batch of a step: raises with the text the step names, through the standing call where the handles are current"""
    from gnnpe_amd import binding
    with pytest.raises(binding.GnnpeError, match=st["msg"]) as err:
        if st["why"] == "all":
            eng.apply_vertices(st["rem"], st["add"])
        elif standing:
            eng.standing_apply_edges(insert=st["ins"], delete=st["dele"])
        else:
            eng.apply_edges_map(insert=st["ins"], delete=st["dele"])
    assert "[-1]" in str(err.value), str(err.value)


# ---- GPU, kind A: standing handles ----------------------------------------------------------------------------------------------------

class Handle:
    def __init__(self, sq, mode, l, keeps):
        self.sq, self.mode, self.l, self.keeps = sq, mode, l, set(keeps)
        self.tables = {}


def snapshot_a(eng, handles):
    out = [x.tobytes() for x in eng.download_csr()] + [eng.download_labels().tobytes()]
    for h in handles:
        sq = h.sq
        out += [sq.bitmap().tobytes(), sq.result(), sq.rows(0).tobytes(), sq.rows(1).tobytes(), sq.set_sizes().tobytes()]
        if h.l:
            out.append(sq.table().tobytes())
        for w in sorted(h.keeps):
            c, d = sq.count_changes(w)
            out += [sq.counts(w).tobytes(), sq.n_changes(w), c.tobytes(), d.tobytes()]
    return out


def check_kept(h, g, query, Y, fresh, what):
    """the kept tables of a handle against the brute force (sc.check_tables where both are kept, its V half otherwise)"""
    if h.keeps == {"vertex", "edge"}:
        V, Et = sc.check_tables(h.sq, g, query, h.mode, Y, fresh, what)
        return dict(vertex=V, edge=Et)
    assert h.keeps == {"vertex"}
    distinct, induced = h.mode
    V = h.sq.counts("vertex")
    BV, _, K = Y[induced]
    count = h.sq.result()[0]
    assert V.shape == BV.shape, (what, V.shape)
    if not distinct:
        assert count == K and np.array_equal(V, BV), (what, h.mode, "V")
    else:
        n_aut, vo, _ = sc.orbits(query)
        assert count * n_aut == K, (what, h.mode, count, n_aut, K)
        for o in vo:
            assert np.array_equal(V[o].sum(axis=0) * np.uint64(n_aut), BV[o].sum(axis=0)), (what, h.mode, "V over the orbit", o)
    assert np.array_equal(V, fresh[h.mode][0]), (what, h.mode, "the one-shot table")
    assert (V.sum(axis=1) == count).all(), (what, h.mode, "a row does not sum to the count")
    with pytest.raises(Exception, match="keep_counts"):
        h.sq.counts("edge")
    return dict(vertex=V)


def run_a(oracle, tmp_path, seed):
    from gnnpe_amd import binding
    s = ds.session("A", seed)
    name, query = s["qname"], QUERIES[s["qname"]]
    qp = write_query(tmp_path, name)
    plans = {l: binding.host_query_plan_exact(qp, E, l) for l in (2, 3)}
    g = s["g0"]
    eng, fresh = fs.open_engine(g, E), Fresh()
    handles = []
    for mode, l, keep_e in HANDLES:
        sq = eng.standing_open(qp, l=l, distinct=mode[0], induced=mode[1], rows_cap=BIG)
        sq.keep_counts(vertex=True, edge=keep_e, changes_cap=BIG)
        handles.append(Handle(sq, mode, l, ["vertex", "edge"] if keep_e else ["vertex"]))
    third = None  # the open_sets handle, and the n its bitmap was made for
    state = dict(stale=False, need_vde=False, relabelled=False, sets={})
    taken = branch_counters()  # the branches replay_a counts from the model, as they are taken here

    def live():
        return handles + ([third[0]] if third else [])

    def sets_of(graph):
        return {m: match_set(graph, query, *m) for m in {h.mode for h in live()}}

    def check_exact(graph, what, emptied):
        """count, S, C, V and E of every handle against the brute force on `graph`; emptied: after a refresh"""
        vde = fs.vde_of(oracle, graph, E)
        Y, ft = sc.yardstick(graph, query), sc.fresh_tables(graph, qp, query)
        for h in live():
            assert h.sq.count == len(state["sets"][h.mode]), (what, h.mode, "count")
            if h.l:
                assert np.array_equal(h.sq.table(), fs.np_support(graph, vde, plans[h.l])), (what, h.mode, "S")
                bits = fs.fresh_bits(graph, E, plans[h.l])
                assert np.array_equal(fs.bits_of(h.sq.bitmap(), graph["n"]), bits), (what, h.mode, "C against the fresh filter")
                assert list(h.sq.set_sizes()) == list(bits.sum(axis=1)), (what, h.mode, "sizes")
            bm = h.sq.bitmap()
            assert bm.shape[1] == (graph["n"] + 31) // 32 and (graph["n"] % 32 == 0 or not np.any(bm[:, -1] >> np.uint32(graph["n"] % 32)))
            if h.keeps:
                h.tables = check_kept(h, graph, query, Y, ft, what)
            if emptied:
                assert h.sq.result()[1:5] == (0, 0, 0, 0), (what, h.mode, "rows after a refresh")
                assert all(h.sq.n_changes(w) == 0 and len(h.sq.count_changes(w)[0]) == 0 for w in h.keeps), (what, "change lists")

    def check_stale(graph, what):
        for h in live():
            calls = [h.sq.result, h.sq.bitmap, h.sq.set_sizes, lambda: h.sq.set_members(0), lambda: h.sq.rows(0, cap=1), h.sq.table_ptr]
            calls += [lambda: h.sq.count, lambda: h.sq.rows(1), lambda: h.sq.keep_counts(vertex=True, edge=False)]
            calls += [h.sq.table] if h.l else [lambda: h.sq.set_bitmap(pack(label_bits(graph, query)))]
            for w in sorted(h.keeps):
                calls += [lambda w=w: h.sq.counts(w), lambda w=w: h.sq.counts_ptr(w), lambda w=w: h.sq.n_changes(w), lambda w=w: h.sq.count_changes(w)]
            for call in calls:
                with pytest.raises(binding.GnnpeError, match=STALE):
                    call()
        have = sorted(graph["edges"])
        with pytest.raises(binding.GnnpeError, match=STALE):
            eng.standing_apply_edges(delete=have[:1])
        with pytest.raises(binding.GnnpeError, match=STALE):
            eng.standing_apply_edges()
        assert np.array_equal(eng.download_csr()[1], graph["nbrs"]), (what, "a refused apply touched the graph")

    def refresh(graph, what):
        nonlocal third
        if state["stale"]:
            if state["need_vde"]:  # refresh needs what open needs
                with pytest.raises(binding.GnnpeError, match="gnnpe_vde"):
                    handles[0].sq.refresh()
            eng.vde(want=False)
            state["need_vde"] = False
        state["sets"] = sets_of(graph)
        for h in handles:
            assert h.sq.refresh() == len(state["sets"][h.mode]), (what, h.mode, "refresh")
        if third:
            if third[1] != graph["n"]:
                with pytest.raises(binding.GnnpeError, match="close the handle and open it again"):
                    third[0].sq.refresh()
                third[0].sq.close()
                third = None
                taken["third_refresh_refused"] += 1
            else:
                taken["third_refresh_ok"] += 1
                taken["third_refresh_after_relabel"] += state["relabelled"]
                state["relabelled"] = False
                third[0].sq.refresh()
                third[0].sq.set_bitmap(pack(label_bits(graph, query)))  # the labels may have moved: the bitmap is the caller's to renew
        state["stale"] = False
        check_exact(graph, (what, "refresh"), True)

    state["sets"] = sets_of(g)
    check_exact(g, "open", False)
    for i, st in enumerate(s["steps"]):
        kind, nxt = st["kind"], st["g"]
        what = ("A", seed, i, kind)
        if kind in STANDING + ("open", "keep_counts") and state["stale"]:
            refresh(g, what)
        if kind in STANDING:
            ins, dele = st.get("ins", []), st.get("dele", [])
            taken["third_batches"] += third is not None
            mid = fs.apply_edges_np(g, [], dele)
            gen = handles[0].sq.result()[5]
            induced = any(h.mode[1] for h in live())
            eng.standing_apply_edges(insert=ins, delete=dele)
            assert handles[0].sq.result()[5] == gen + (2 if ins and dele and induced else 1 if ins or dele else 0), (what, "generation")
            after = {m: (match_set(mid, query, *m), match_set(nxt, query, *m)) for m in state["sets"]}
            old = {id(h): dict(h.tables) for h in live()}
            for h in live():
                check_batch(h.sq, query, h.mode, (state["sets"][h.mode],) + after[h.mode], what)
            state["sets"] = {m: after[m][1] for m in after}
            check_exact(nxt, what, False)
            for h in live():
                before = old[id(h)]
                if "vertex" in before:
                    sc.check_changes(h.sq, "vertex", before["vertex"], h.tables["vertex"], (what, h.mode))
                if "edge" in before:
                    sc.check_changes(h.sq, "edge", sc.moved_by_key(before["edge"], g, nxt), h.tables["edge"], (what, h.mode))
        elif kind in ("vertices", "relabel", "offline"):
            if kind == "vertices":
                assert eng.apply_vertices(st["rem"], st["add"])[0] == nxt["n"]
            elif kind == "relabel":
                eng.set_vertex_labels(st["R"], st["labels"])
            else:
                offline_pass(eng, g, oracle, what)
            state["stale"], state["need_vde"] = True, kind != "offline"
            state["relabelled"] = state["relabelled"] or (kind == "relabel" and third is not None)
            check_stale(nxt, what)
        elif kind == "refused":
            if state["stale"]:
                taken["refused_stale"] += 1
                refused_call(eng, st, False)
                check_stale(g, what)
            else:
                taken["refused_current"].add(st["why"])
                before = snapshot_a(eng, live())
                refused_call(eng, st, True)
                assert snapshot_a(eng, live()) == before, (what, st["why"], "a refused batch changed something")
        elif kind == "refresh":
            refresh(g, what)
        elif kind == "open":
            if third:
                third[0].sq.close()
            sq = eng.standing_open(qp, bitmap=pack(label_bits(g, query)), rows_cap=BIG)
            third = (Handle(sq, (False, False), 0, []), g["n"])
            state["relabelled"] = False
            state["sets"] = sets_of(g)
            assert sq.table() is None and sq.count == len(state["sets"][False, False]), (what, "open_sets")
        elif kind == "close":
            if third:
                third[0].sq.close()
                third = None
        elif kind == "keep_counts":  # on a handle that has been through batches
            h = handles[1]
            if "edge" not in h.keeps:
                h.sq.keep_counts(vertex=False, edge=True, changes_cap=BIG)  # E is built on the graph as it is now; V stays
                h.keeps.add("edge")
            else:
                taken["new_cap"] += 1
                handles[0].sq.keep_counts(vertex=True, edge=True, changes_cap=BIG + i)  # a new cap: the tables stay, the lists are emptied
                assert all(handles[0].sq.n_changes(w) == 0 for w in ("vertex", "edge")), what
            check_exact(g, what, False)
        check_graph(eng, fresh, nxt, what)
        g = nxt
    if state["stale"]:
        refresh(g, ("A", seed, "end"))
    assert taken == replay_a(s), ("run_a and replay_a took different branches", taken, replay_a(s))
    eng.close()
    fresh.close()


# ---- GPU, kind B: the caller keeps the state ----------------------------------------------------------------------------------------------

def check_support(eng, g, vde, plan, table, what):
    """fs.check_tables for any n (a multiple of 32 included): the carried table == the table recomputed on the engine == numpy's;
    the bitmap == the fresh filter's, no bit past n.  Returns numpy's"""
    want = fs.np_support(g, vde, plan)
    got = fs.to_np(table)
    assert got.shape == want.shape, (what, got.shape)
    assert np.array_equal(fs.to_np(eng.filter_support_exact(plan)[0]), want), (what, "recomputed")
    assert np.array_equal(got, want), (what, "carried", int((got != want).sum()))
    bm = eng.support_bitmap(table, int(plan["n_vertices"]))[0]
    assert bm.shape == (want.shape[0], (g["n"] + 31) // 32)
    assert g["n"] % 32 == 0 or not np.any(bm[:, -1] >> np.uint32(g["n"] % 32)), (what, "bits past n")
    assert np.array_equal(fs.bits_of(bm, g["n"]), want != 0), (what, "bitmap of the table")
    assert np.array_equal(fs.bits_of(bm, g["n"]), fs.fresh_bits(g, E, plan)), (what, "fresh filter")
    return want


def dev64(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(1, -1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def fresh_state(eng, g, oracle, tmp_path, what):
    """after the same order and label table the engine is a fresh engine with the model graph: x, nx, vde bit for bit, the l = 2
    paths against the oracle, refine_sets in the four modes on triangle and wedge against the fresh engine and the brute force"""
    from gnnpe_amd import binding
    sn, mine = offline_pass(eng, g, oracle, what)
    other = sqt.base._engine(binding, g, sn, E)
    other.set_label_table(binding.host_label_table(NL, E))
    for a, b, name in zip(mine, other.vde(), ("x", "nx", "vde")):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, name)
    assert eng.count_paths(2) == other.count_paths(2)
    for name in ("triangle", "wedge"):
        query = QUERIES[name]
        qp = write_query(tmp_path, name)
        bits = label_bits(g, query)
        for d, i in sqt.MODES:
            got = eng.refine_sets(qp, pack(bits), limit=sqt.FULL, distinct=d, induced=i)[0]
            assert got == other.refine_sets(qp, pack(bits), limit=sqt.FULL, distinct=d, induced=i)[0], (what, name, d, i, "fresh engine")
            assert got == len(match_set(g, query, d, i, bits)), (what, name, d, i, "brute force")
    other.close()


def run_b(oracle, tmp_path, seed):
    import torch
    from gnnpe_amd import binding
    s = ds.session("B", seed)
    g = s["g0"]
    plan = plan_b(g, seed, tmp_path)
    nq = int(plan["n_vertices"])
    wedge = QUERIES["wedge"]
    wq = write_query(tmp_path, "wedge")
    eng, fresh = fs.open_engine(g, E), Fresh()
    table, _ = eng.filter_support_exact(plan)
    vt, et = dev64(s["vtags"]), dev64(s["etags"])
    maps = dict(v=None, e=None)  # the table a still valid map was last applied to, None without a valid map
    ordered = False  # an order is set: the next update must throw it away
    moves = fs.Moves()

    def open_cursor(graph):
        bits = label_bits(graph, wedge)
        return binding.MatchCursor(eng, wq, pack(bits), 5), match_set(graph, wedge, False, False, bits), set()

    def next_page(c, what):
        rows = set(map(tuple, np.asarray(c[0].next()[0], np.int64).tolist()))
        assert len(rows) == 5 and rows <= c[1] and not rows & c[2], (what, "a page of the cursor")
        c[2].update(rows)

    def carried(fn, src, width):
        dst = torch.zeros((1, width), dtype=torch.int64, device=src.device)
        torch.cuda.synchronize()
        fn(src, dst, 1)
        eng.sync()
        return dst

    def check_maps(st, what, changed):
        """the tag tables through whichever map is valid -- again through a map an earlier step left, which must still give what it
        gave; a carry without a valid map is refused with GNNPE_ERR_ARG"""
        nonlocal vt, et
        for key, fn in (("v", eng.carry_vertices), ("e", eng.carry_entries)):
            tab, now = (vt, st["vtags"]) if key == "v" else (et, st["etags"])
            m = maps[key]
            if m is None:
                room = torch.zeros((1, len(now) + 8), dtype=torch.int64, device=tab.device)
                torch.cuda.synchronize()
                raw = eng.lib.gnnpe_csr_carry_vertices if key == "v" else eng.lib.gnnpe_csr_carry_entries
                rc = raw(eng.ctx, 1, 8, C.c_void_p(tab.data_ptr()), C.c_void_p(room.data_ptr()), None)
                assert rc == av.ERR_ARG and b"no valid" in eng.lib.gnnpe_last_error(), (what, key, rc)  # GNNPE_ERR_ARG, nothing launched
                assert not fs.to_np(room).any(), (what, key, "a refused carry wrote")
                assert changed or np.array_equal(fs.to_np(tab).ravel(), now), (what, key, "the caller's table")
            else:
                got = carried(fn, m["src"], len(m["want"]))
                assert np.array_equal(fs.to_np(got).ravel(), m["want"]), (what, key, "carried", int((fs.to_np(got).ravel() != m["want"]).sum()))
                if m["new"]:
                    m["new"] = False
                    if key == "v":
                        vt = got
                    else:
                        et = got
        # the caller writes fresh tags where the carry left 0, and the whole table after a change that left no map
        if not np.array_equal(fs.to_np(vt).ravel(), st["vtags_new"]):
            assert changed and (maps["v"] is None or (st["vtags"] == 0).any()), (what, "vertex tags")
            vt = dev64(st["vtags_new"])
        if not np.array_equal(fs.to_np(et).ravel(), st["etags_new"]):
            assert changed and (maps["e"] is None or (st["etags"] == 0).any()), (what, "entry tags")
            et = dev64(st["etags_new"])

    def made(key, src, want):
        maps[key] = dict(src=src, want=want, new=True)

    def wants_vde(what):
        """every update call resets gnnpe_vde, which the next support call asks for (refused on the host: the table stays)"""
        with pytest.raises(binding.GnnpeError, match="gnnpe_vde"):
            eng.filter_support_delta(plan, [0], +1, table)
        eng.vde(want=False)

    cur = open_cursor(g)
    next_page(cur, "open")
    before = check_support(eng, g, fs.vde_of(oracle, g, E), plan, table, ("B", seed, "start"))
    for i, st in enumerate(s["steps"]):
        kind, nxt = st["kind"], st["g"]
        what = ("B", seed, i, kind)
        changed = kind in ("edges", "edges_hub", "vertices", "relabel")
        col_map = None
        if kind in ("edges", "edges_hub"):
            T = np.unique(np.array(st["ins"] + st["dele"], np.int64))
            eng.filter_support_delta(plan, T, -1, table)
            if kind == "edges":
                b, a, _ = eng.apply_edges_map(insert=st["ins"], delete=st["dele"])
                assert (b, a) == (len(g["nbrs"]), len(nxt["nbrs"])), what
                maps.update(v=None)
                made("e", et, st["etags"])
            else:
                assert eng.apply_edges(insert=st["ins"], delete=st["dele"]) == len(nxt["nbrs"]), what
                maps.update(v=None, e=None)
            wants_vde(what)
            eng.filter_support_delta(plan, T, +1, table)
        elif kind == "relabel":
            T = fs.with_neighbours(g, st["R"])
            eng.filter_support_delta(plan, T, -1, table)
            eng.set_vertex_labels(st["R"], st["labels"])
            maps.update(v=None, e=None)
            wants_vde(what)
            eng.filter_support_delta(plan, T, +1, table)
        elif kind == "vertices":
            new_id = st["new_id"]
            T = fs.with_neighbours(g, st["rem"]) if st["rem"] else np.zeros(0, np.int64)
            eng.filter_support_delta(plan, T, -1, table)
            assert not fs.to_np(table)[:, st["rem"]].any(), (what, "the columns of R hold zero")
            n2, b, a, vview, eview = eng.apply_vertices(st["rem"], st["add"], entry_map=True)
            assert (n2, b, a) == (nxt["n"], len(g["nbrs"]), len(nxt["nbrs"])), what
            _, vmap, emap = av._apply_np(g, st["rem"], st["add"])
            assert np.array_equal(eng.vertex_map_to_host(vview), vmap) and np.array_equal(eng.entry_map_to_host(eview), emap), (what, "maps")
            moved = torch.zeros((nq, n2), dtype=torch.int64, device=table.device)
            torch.cuda.synchronize()
            eng.carry_vertices(table, moved, nq, 8)
            table = moved
            made("v", vt, st["vtags"])
            made("e", et, st["etags"])
            wants_vde(what)
            T2 = np.concatenate([new_id[T][new_id[T] >= 0], np.arange(n2 - len(st["add"]), n2)])
            eng.filter_support_delta(plan, T2, +1, table)
            col_map = np.full(n2, -1, np.int64)
            col_map[new_id[new_id >= 0]] = np.flatnonzero(new_id >= 0)
        elif kind == "empty":
            b, a, view = eng.apply_edges_map()
            assert (b, a) == (len(g["nbrs"]), len(g["nbrs"])) and np.array_equal(eng.entry_map_to_host(view), np.arange(a)), what
            made("e", et, st["etags"])
        elif kind == "refused":
            refused_call(eng, st, False)
            maps.update(e=None)
            if st["why"] == "all":
                maps.update(v=None)
        elif kind == "offline":
            offline_pass(eng, g, oracle, what)
            ordered = True
        # the cursor opened before the step
        if changed:
            with pytest.raises(binding.GnnpeError):
                cur[0].next()
            cur[0].close()
            if ordered:
                with pytest.raises(binding.GnnpeError):
                    eng.count_paths(2)
                ordered = False
            cur = open_cursor(nxt)
        next_page(cur, what)
        check_graph(eng, fresh, nxt, what)
        after = check_support(eng, nxt, fs.vde_of(oracle, nxt, E), plan, table, what)
        moves.step(before, after, col_map)
        before = after
        check_maps(st, what, changed)
        if i % 3 == 2 or i == len(s["steps"]) - 1:
            fresh_state(eng, nxt, oracle, tmp_path, what)
            ordered = True
            next_page(cur, (what, "after the offline calls"))
        g = nxt
    assert moves.cleared + moves.set + moves.moved > 0, ("B", seed, "the support table never moved")
    cur[0].close()
    eng.close()
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS["A"])
def test_gpu_session_with_standing_handles(oracle, tmp_path, seed):
    run_a(oracle, tmp_path, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS["B"])
def test_gpu_session_with_caller_kept_state(oracle, tmp_path, seed):
    run_b(oracle, tmp_path, seed)
