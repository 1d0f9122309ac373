"""gnnpe_standing_peel and gnnpe_standing_truss_levels (include/gnnpe_online.h, "PEELING THE GRAPH BY EDGE SUPPORT") against the Python
peel of tests/peel_yardstick.py, which recounts every match of the current numpy graph each round, deletes all edges below t at once,
and finds the levels by peeling the whole graph for every t from 0 up to the largest support: no level jumping, no library code.

Graphs: make_graph(hub_deg=64) of the support tests (n = 301); G(60, 240) with two labels for the 4-cycle and the five-vertex query;
the cascade graph (a K5 with a strip of triangles hanging off it, 18 vertices), where the DISTINCT triangle at t = 2 takes 7 rounds
and stops at the K5.  The thresholds were chosen with the yardstick alone so that every case removes some but not all edges; each
test asserts that (and the cascade its rounds).  Handles are opened with open_sets on a label bitmap, which is sound under deletions;
one case is opened with the exact filter at l = 2 and at l = 3."""
import os
import subprocess

import numpy as np
import pytest

import peel_yardstick as py
import test_filter_support as fs
import test_online_exact as base
from test_standing_counts import counts_snapshot
from test_standing_query import E, QUERIES, match_set, pack, write_query

pytestmark = pytest.mark.gpu

FULL = (1 << 64) - 1
WEDGE_ONES = (3, {(0, 1), (1, 2)}, [1, 1, 1])  # the second handle on the cascade graph, whose labels are all 1

_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = {"hub": lambda: fs.make_graph(hub_deg=64), "gnm": lambda: py.gnm(60, 240, 2, 2), "cascade": py.cascade_graph}[name]()
        _GRAPHS[name]["edges"] = {(min(a, b), max(a, b)) for a, b in _GRAPHS[name]["edges"]}
    return _GRAPHS[name]


def label_bitmap(g, query):
    return pack(np.array([g["labels"] == lb for lb in query[2]]))


def open_pair(tmp_path, g, name, distinct, filter_l=0):
    """an engine with g, the handle under test (keeping V and E) and a second handle on the context: the induced wedge"""
    from gnnpe_amd import binding
    query = QUERIES[name]
    qp = write_query(tmp_path, name)
    wedge = WEDGE_ONES if (g["labels"] == 1).all() else QUERIES["wedge"]
    wp = str(tmp_path / "second.graph")
    base._write_query(wp, *wedge)
    if filter_l:
        eng = fs.open_engine(g, E)
        sq = eng.standing_open(qp, l=filter_l, distinct=distinct)
    else:
        eng = binding.Engine(0)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        sq = eng.standing_open(qp, distinct=distinct, bitmap=label_bitmap(g, query))
    sq.keep_counts(vertex=True, edge=True)
    other = eng.standing_open(wp, induced=True, bitmap=label_bitmap(g, wedge))
    return eng, sq, other, query, wedge, qp


def fresh_state(g, qp, query, distinct):
    """(count, V, E) of the one-shot calls on a fresh engine with g"""
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    bm = label_bitmap(g, query)
    v = eng.refine_sets_vertex_counts(qp, bm, distinct=distinct)
    e = eng.refine_sets_edge_counts(qp, bm, distinct=distinct)
    assert v[1] and e[1] and v[0] == e[0]
    eng.close()
    return v[0], v[2], e[2]


def check_state(eng, sq, other, g_now, qp, query, wedge, distinct, what):
    """the resident graph is g_now, and count, V and E of the handle are those of a fresh engine on it; the second handle is exact"""
    off, nb = eng.download_csr()
    assert np.array_equal(off, g_now["offsets"]) and np.array_equal(nb, g_now["nbrs"]), (what, "the graph")
    count, V, Et = fresh_state(g_now, qp, query, distinct)
    assert sq.count == count == len(match_set(g_now, query, distinct, False)), (what, sq.count, count)
    assert np.array_equal(sq.counts("vertex"), V) and np.array_equal(sq.counts("edge"), Et), (what, "the tables")
    assert other.count == len(match_set(g_now, wedge, False, True)), (what, "the second handle")


def pairs_of(a):
    return [tuple(p) for p in np.asarray(a, np.int64).reshape(-1, 2).tolist()]


CASES = [("hub", "triangle", True, 1), ("hub", "triangle", False, 6), ("gnm", "c4", True, 2), ("gnm", "c4", False, 8), ("gnm", "house", True, 2),
         ("gnm", "house", False, 4), ("cascade", "triangle", True, 2), ("cascade", "triangle", False, 12)]


@pytest.mark.parametrize("gname,name,distinct,t", CASES)
def test_gpu_peel_against_the_yardstick(tmp_path, gname, name, distinct, t):
    g = graph(gname)
    eng, sq, other, query, wedge, qp = open_pair(tmp_path, g, name, distinct)
    left, removed, rounds, out = py.peel(g, query, distinct, t)
    assert 0 < out[1] < g["m"] and out[3] == 1, ("the case is not telling", out)
    if gname == "cascade":
        assert out[0] >= 5 and left["edges"] == py.K5, out
    got_removed, got_rounds, got_out = sq.peel(t)
    assert got_out == out, (got_out, out)
    assert pairs_of(got_removed) == removed and got_rounds.tolist() == rounds
    check_state(eng, sq, other, left, qp, query, wedge, distinct, (gname, name, distinct, t))
    # a second peel at the same threshold finds nothing and changes nothing
    gen = sq.result()[5]
    again = sq.peel(t)
    assert again[2] == [0, 0, left["m"], 1] and len(again[0]) == 0 and sq.result()[5] == gen
    eng.close()


@pytest.mark.parametrize("l", [2, 3])
def test_gpu_peel_with_the_exact_filter(tmp_path, l):
    g = graph("hub")
    eng, sq, other, query, wedge, qp = open_pair(tmp_path, g, "triangle", True, filter_l=l)
    left, removed, rounds, out = py.peel(g, query, True, 1)
    assert 0 < out[1] < g["m"]
    got_removed, got_rounds, got_out = sq.peel(1)
    assert got_out == out and pairs_of(got_removed) == removed and got_rounds.tolist() == rounds
    check_state(eng, sq, other, left, qp, query, wedge, True, ("filter", l))
    eng.close()


def test_gpu_peel_max_rounds_cuts_and_a_second_call_finishes(tmp_path):
    g = graph("cascade")
    eng, sq, other, query, wedge, qp = open_pair(tmp_path, g, "triangle", True)
    left, removed, rounds, out = py.peel(g, query, True, 2)
    cut = rounds.index(3)  # the edges of rounds 1 and 2
    mid, removed2, rounds2, out2 = py.peel(g, query, True, 2, max_rounds=2)
    assert out2 == [2, cut, g["m"] - cut, 0] and removed2 == removed[:cut]
    a = sq.peel(2, max_rounds=2)
    assert a[2] == out2 and pairs_of(a[0]) == removed[:cut] and a[1].tolist() == rounds[:cut]
    check_state(eng, sq, other, mid, qp, query, wedge, True, "cut after two rounds")
    b = sq.peel(2)
    assert b[2] == [out[0] - 2, out[1] - cut, left["m"], 1]
    assert pairs_of(b[0]) == removed[cut:] and b[1].tolist() == [r - 2 for r in rounds[cut:]]
    check_state(eng, sq, other, left, qp, query, wedge, True, "the second call")
    eng.close()


def test_gpu_peel_threshold_above_every_support_and_threshold_zero(tmp_path):
    g = graph("gnm")
    eng, sq, other, query, wedge, qp = open_pair(tmp_path, g, "c4", False)
    off0, nb0 = eng.download_csr()
    before = (off0.tobytes(), nb0.tobytes(), sq.result(), sq.counts("edge").tobytes(), sq.counts("vertex").tobytes(), other.result())
    none = sq.peel(0)
    off1, nb1 = eng.download_csr()
    assert none[2] == [0, 0, g["m"], 1] and len(none[0]) == 0
    assert (off1.tobytes(), nb1.tobytes(), sq.result(), sq.counts("edge").tobytes(), sq.counts("vertex").tobytes(), other.result()) == before
    removed, rounds, out = sq.peel(FULL)
    assert out == [1, g["m"], 0, 1] and pairs_of(removed) == sorted(g["edges"]) and set(rounds.tolist()) == {1}
    off2, nb2 = eng.download_csr()
    assert len(nb2) == 0 and not off2.any() and sq.count == 0 and other.count == 0
    assert sq.counts("edge").shape == (4, 0) and not sq.counts("vertex").any()
    eng.close()


@pytest.mark.parametrize("gname,name,distinct", [("cascade", "triangle", True), ("cascade", "triangle", False), ("gnm", "c4", True),
                                                 ("gnm", "house", False)])
def test_gpu_truss_levels_with_restore(tmp_path, gname, name, distinct):
    g = graph(gname)
    eng, sq, other, query, wedge, qp = open_pair(tmp_path, g, name, distinct)
    want = py.levels(g, query, distinct)
    assert len(set(want.values())) > 1, "the case is not telling"
    off0, nb0 = eng.download_csr()
    before = (off0.tobytes(), nb0.tobytes(), sq.count, sq.bitmap().tobytes(), sq.counts("vertex").tobytes(), sq.counts("edge").tobytes(),
              other.count)
    edges, levels, out = sq.truss_levels(restore=True)
    got = dict(zip(pairs_of(edges), levels.tolist()))
    assert len(got) == len(edges) == g["m"] and got == want
    assert (np.diff(levels.astype(np.int64)) >= 0).all(), "removal order is by level"
    rounds, cur = 0, g
    for lv in sorted(set(want.values())):  # the rounds: the yardstick's peel at level + 1, from the truss of that level
        cur, _, _, o = py.peel(cur, query, distinct, lv + 1)
        rounds += o[0]
    assert out == [g["m"], len(set(want.values())), max(want.values()), rounds], out
    off1, nb1 = eng.download_csr()
    after = (off1.tobytes(), nb1.tobytes(), sq.count, sq.bitmap().tobytes(), sq.counts("vertex").tobytes(), sq.counts("edge").tobytes(),
             other.count)
    assert after == before, "restore does not give back the state of before the call"
    check_state(eng, sq, other, g, qp, query, wedge, distinct, "restored")
    eng.close()


def test_gpu_truss_levels_without_restore(tmp_path):
    g = graph("cascade")
    eng, sq, other, query, wedge, qp = open_pair(tmp_path, g, "triangle", True)
    want = py.levels(g, query, True)
    edges, levels, out = sq.truss_levels(restore=False)
    assert dict(zip(pairs_of(edges), levels.tolist())) == want and out[0] == g["m"]
    off, nb = eng.download_csr()
    assert len(nb) == 0 and not off.any() and sq.count == 0 and other.count == 0
    assert sq.counts("edge").shape == (3, 0) and not sq.counts("vertex").any()
    # the emptied graph: both calls find nothing to do
    assert sq.truss_levels(restore=True)[2] == [0, 0, 0, 0] and sq.peel(5)[2] == [0, 0, 0, 1]
    eng.close()


def test_gpu_peel_refusals_change_nothing(tmp_path):
    from gnnpe_amd import binding
    g = graph("hub")
    tri, one = write_query(tmp_path, "triangle"), str(tmp_path / "one.graph")
    base._write_query(one, 1, set(), [1])
    eng = fs.open_engine(g, E)
    kept = eng.standing_open(tri, l=2, distinct=True)
    induced = eng.standing_open(tri, l=2, induced=True)
    single = eng.standing_open(one, l=2)
    bare = eng.standing_open(tri, l=2)
    handles = [kept, induced, single]
    for sq in handles:
        sq.keep_counts(vertex=True, edge=True, changes_cap=64)
    eng.standing_apply_edges(delete=sorted(g["edges"])[:3])  # so that the handles hold the results of a batch
    before = counts_snapshot(eng, handles) + [bare.result(), bare.bitmap().tobytes()]
    refused = [(induced, r"\[-3\].*induced"), (single, r"\[-1\].*without an edge"), (bare, r"\[-1\].*gnnpe_standing_keep_counts")]
    for sq, msg in refused:
        for call in (lambda: sq.peel(1), lambda: sq.truss_levels(restore=True), lambda: sq.truss_levels(restore=False)):
            with pytest.raises(binding.GnnpeError, match=msg):
                call()
            assert counts_snapshot(eng, handles) + [bare.result(), bare.bitmap().tobytes()] == before, msg
    online = binding.load_online()
    import ctypes as C
    out = (C.c_uint64 * 4)()
    assert online.gnnpe_standing_peel(None, 1, 0, None, None, 0, out, None) == -1
    assert online.gnnpe_standing_peel(kept.handle, 1, 0, None, None, 0, None, None) == -1
    assert online.gnnpe_standing_peel(kept.handle, 1, 0, None, None, 5, out, None) == -1  # cap without host_removed
    assert online.gnnpe_standing_truss_levels(kept.handle, 1, None, None, 5, out, None) == -1
    assert counts_snapshot(eng, handles) + [bare.result(), bare.bitmap().tobytes()] == before
    # a stale handle: a plain apply behind its back.  The graph stays what that apply left; a refresh makes the peel exact again
    some = sorted(g["edges"])[10:12]
    eng.apply_edges(delete=some)
    off0, nb0 = eng.download_csr()
    for call in (lambda: kept.peel(1), lambda: kept.truss_levels()):
        with pytest.raises(binding.GnnpeError, match="gnnpe_standing_refresh"):
            call()
    off1, nb1 = eng.download_csr()
    assert off0.tobytes() == off1.tobytes() and nb0.tobytes() == nb1.tobytes()
    eng.vde(want=False)
    for sq in handles + [bare]:
        sq.refresh()
    cur = fs.apply_edges_np(g, [], sorted(g["edges"])[:3] + some)
    left, removed, rounds, out = py.peel(cur, QUERIES["triangle"], True, 1)
    got = kept.peel(1)
    assert got[2] == out and pairs_of(got[0]) == removed
    assert induced.count == len(match_set(left, QUERIES["triangle"], False, True)) and bare.count == len(match_set(left, QUERIES["triangle"], False, False))
    eng.close()


def test_gpu_cli_peel_and_truss_levels(tmp_path):
    """gnnpe_main --standing --truss-levels FILE --peel T --peel-out FILE on the cascade graph: the same files as the binding gives"""
    from gnnpe_amd import synth
    g = dict(graph("cascade"))
    und = np.array(sorted(g["edges"]), np.int64)
    g["eu"], g["ev"] = und[:, 0], und[:, 1]
    gp = str(tmp_path / "cascade.graph")
    synth.write_graph_file(gp, g)
    qp = write_query(tmp_path, "triangle")
    eng = fs.open_engine(g, E)
    sq = eng.standing_open(qp, l=2, distinct=True)
    sq.keep_counts(vertex=False, edge=True)
    edges, levels, lout = sq.truss_levels(restore=True)
    removed, rounds, pout = sq.peel(2)
    count = sq.count
    eng.close()
    root = base._dataset(tmp_path, gp)
    f_levels, f_peel = str(tmp_path / "levels.txt"), str(tmp_path / "peel.txt")
    cmd = [base.CLI, "-f", root, "-d", gp, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets", "--distinct", "--standing", "--truss-levels", f_levels,
           "--peel", "2", "--peel-out", f_peel]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(f_levels).read() == "".join(f"{a} {b} {lv}\n" for (a, b), lv in zip(pairs_of(edges), levels.tolist()))
    assert open(f_peel).read() == "".join(f"{a} {b} {rd}\n" for (a, b), rd in zip(pairs_of(removed), rounds.tolist()))
    lines = r.stdout.splitlines()
    truss = [ln.split() for ln in lines if ln.startswith("truss: ")]
    peel = [ln.split() for ln in lines if ln.startswith("peel: ")]
    assert len(truss) == 1 and [int(v) for v in truss[0][1:5]] == lout
    assert len(peel) == 1 and [int(v) for v in peel[0][1:6]] == pout + [count] and pout[2] == 10 and pout[0] >= 5
    # the flags need --standing, and an induced handle is refused by the library
    r = subprocess.run([c for c in cmd if c != "--standing"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--standing" in r.stderr + r.stdout
    r = subprocess.run(cmd + ["--induced"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "induced" in r.stderr + r.stdout
    assert os.path.getsize(f_peel) > 0
