"""The contract of the eight host entries of the set-restricted refinement (include/gnnpe_online.h: gnnpe_host_refine_sets,
_distinct, _mode, _vertex_counts, _edge_counts, _delta, _delta_vertex_counts, _delta_edge_counts), case by case: what a call
returns, what it leaves in *answers and *complete (both pre-set to a sentinel), the whole gnnpe_last_error() text of a refusal,
and whether `counts` (pre-filled with 0xAB bytes) is left untouched, zeroed or filled.

The expected values are tests/golden/host_sets_contract.json, recorded once from the library as it was before the eight entries
were folded onto one scaffold (tests/golden/make_golden.py host_sets_contract writes it): the entries differ in which pointers may
be null, in what they clear before the mode check, in whether a refusal carries the entry's name, and in whether the table is
zeroed before or after the refusals -- and none of that may move.

The data graph is H1 of tests/test_refine_sets_shapes.py; the queries are its triangle, wedge, edge and single vertex, a
disconnected pair, an edge beside a vertex and a file that does not exist.  Raw ctypes calls; no GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import test_online_exact as ex
import test_refine_sets_shapes as sh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_sets_contract.json")
FULL = (1 << 64) - 1
ANSWERS_SENTINEL = 0xDEADBEEFDEADBEEF
COMPLETE_SENTINEL = -77

# entry -> (takes a mode word, table kind, takes F)
ENTRIES = {
    "gnnpe_host_refine_sets": (False, None, False),
    "gnnpe_host_refine_sets_distinct": (False, None, False),
    "gnnpe_host_refine_sets_mode": (True, None, False),
    "gnnpe_host_refine_sets_vertex_counts": (True, "vertex", False),
    "gnnpe_host_refine_sets_edge_counts": (True, "edge", False),
    "gnnpe_host_refine_sets_delta": (True, None, True),
    "gnnpe_host_refine_sets_delta_vertex_counts": (True, "vertex", True),
    "gnnpe_host_refine_sets_delta_edge_counts": (True, "edge", True),
}
# ("edge_and_vertex": disconnected too, but with an edge, so that its edge table has cells)
QUERIES = ("triangle", "wedge", "edge", "vertex", "disconnected", "edge_and_vertex", "missing")
N_QUERY_VERTICES = dict(triangle=3, wedge=3, edge=2, vertex=1, disconnected=2, edge_and_vertex=3, missing=3)
N_QUERY_EDGES = dict(triangle=3, wedge=2, edge=1, vertex=0, disconnected=0, edge_and_vertex=1, missing=3)

_WORLD = {}


def _world(tmp_path_factory):
    """H1, the seven query files with a bitmap each, and the six forms of F"""
    if _WORLD:
        return _WORLD
    h = sh._h1(tmp_path_factory)
    g, tmp = h["g"], h["tmp"]
    n = int(g["n"])
    q = {name: h["q"][name] for name in ("triangle", "wedge", "edge", "vertex")}
    bm = {name: h["bm"][name]["ld"] for name in q}
    q["disconnected"] = str(tmp / "disconnected.graph")
    ex._write_query(q["disconnected"], 2, set(), [0, 0])
    q["edge_and_vertex"] = str(tmp / "edge_and_vertex.graph")
    ex._write_query(q["edge_and_vertex"], 3, {(0, 1)}, [0, 0, 0])
    q["missing"] = str(tmp / "no_such_query.graph")
    for name in ("disconnected", "edge_and_vertex", "missing"):
        bm[name] = sh._ones(N_QUERY_VERTICES[name], n)
    # F: three edges at the vertex of the highest degree, so that matches run through them
    offs = g["offsets"].astype(np.int64)
    hub = int(np.argmax(np.diff(offs)))
    row = [int(y) for y in g["nbrs"][offs[hub]:offs[hub + 1]]]
    three = [(hub, y) for y in row[:3]]
    stranger = next(v for v in range(n) if v != hub and v not in row)
    F = {
        "empty": [],
        "three": three,
        "repeats_flipped": three + [(y, x) for x, y in three] + three[:1],
        "non_edge": three[:1] + [(hub, stranger)],
        "loop": three[:1] + [(hub, hub)],
        "id_n": three[:1] + [(hub, n)],
    }
    _WORLD.update(g=g, n=n, entries=int(offs[n]), q=q, bm=bm, tmp=str(tmp),
                  F={k: np.ascontiguousarray(np.asarray(v, np.uint32).reshape(-1, 2)) for k, v in F.items()})
    return _WORLD


def _cases(entry):
    """[(case name, keyword arguments of _call)] of one entry, in a fixed order"""
    has_mode, table, has_f = ENTRIES[entry]
    cases = [("base", {})]
    nullable = ["offsets", "nbrs", "labels", "path", "bitmap", "answers"] + (["complete", "counts"] if table else []) + \
        (["F"] if has_f else [])
    cases += [(f"null_{arg}", {"null": arg}) for arg in nullable]  # (null_counts: a table with cells; null_F: n_delta stays 3)
    if table:
        cases.append(("null_counts_no_edge_table", dict(query="vertex", null="counts")))  # the edge tables have no cell there
    if has_mode:
        cases += [("mode_4", dict(mode=4)), ("mode_bit31", dict(mode=1 << 31)), ("mode_bit31_null_answers", dict(mode=1 << 31, null="answers"))]
        cases += [(f"mode_{m}", dict(mode=m)) for m in (1, 2, 3)]
        cases += [(f"mode_{m}_limit_1", dict(mode=m, limit=1)) for m in (1, 2, 3)]
    for query in QUERIES:
        cases += [(f"{query}_limit_{name}", dict(query=query, limit=limit)) for name, limit in (("0", 0), ("below", 2), ("full", FULL))]
    if has_f:
        for f in ("empty", "repeats_flipped", "non_edge", "loop", "id_n"):
            cases.append((f"F_{f}", dict(F=f)))
        cases += [("F_empty_limit_0", dict(F="empty", limit=0)), ("F_empty_disconnected", dict(F="empty", query="disconnected")),
                  ("F_empty_missing", dict(F="empty", query="missing")), ("F_non_edge_disconnected", dict(F="non_edge", query="disconnected")),
                  ("F_loop_mode_4", dict(F="loop", mode=4)), ("F_three_distinct_induced", dict(F="three", mode=3))]
    return cases


def _call(w, entry, query="triangle", limit=FULL, mode=0, F="three", null=None):
    """one raw call; what it left, as the fixture records it"""
    from gnnpe_amd import binding
    has_mode, table, has_f = ENTRIES[entry]
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    g = w["g"]
    arrays = dict(offsets=np.ascontiguousarray(g["offsets"], np.uint32), nbrs=np.ascontiguousarray(g["nbrs"], np.uint32),
                  labels=np.ascontiguousarray(g["labels"], np.uint32), bitmap=np.ascontiguousarray(w["bm"][query], np.uint32))
    ptr = {k: None if null == k else a.ctypes.data_as(u32p) for k, a in arrays.items()}
    path = None if null == "path" else w["q"][query].encode()
    answers, complete = C.c_uint64(ANSWERS_SENTINEL), C.c_int(COMPLETE_SENTINEL)
    cells = 0
    if table:
        cells = N_QUERY_VERTICES[query] * w["n"] if table == "vertex" else N_QUERY_EDGES[query] * w["entries"]
    counts = np.full(max(cells, 1) * 8, 0xAB, np.uint8)  # (one spare cell where the table is empty: it must stay untouched)
    args = [w["n"], ptr["offsets"], ptr["nbrs"], ptr["labels"], path, ptr["bitmap"]]
    if has_f:
        f = w["F"][F]
        args += [None if null == "F" or len(f) == 0 else f.ctypes.data_as(u32p), len(f)]
    args.append(limit)
    if has_mode:
        args.append(mode)
    args.append(None if null == "answers" else C.byref(answers))
    if table:
        args += [None if null == "complete" else C.byref(complete), None if null == "counts" else counts.ctypes.data_as(u64p)]
    rc = getattr(binding.load_online(), entry)(*args)
    err = binding.load().gnnpe_last_error().decode().replace(w["tmp"], "<tmp>") if rc else None
    left = dict(rc=rc, answers=answers.value, error=err)
    if table:
        left["complete"] = complete.value
        if (counts == 0xAB).all():
            left["counts"] = "untouched"
        elif not counts.any():
            left["counts"] = "zeroed"
        else:
            left["counts"] = "filled:" + hashlib.sha1(counts.tobytes()).hexdigest()
    return left


def observe(tmp_path_factory, entry):
    """{case name: what the call left} of one entry"""
    w = _world(tmp_path_factory)
    return {name: _call(w, entry, **kw) for name, kw in _cases(entry)}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_host_entry_leaves_what_the_recorded_library_left(tmp_path_factory, entry):
    want = json.load(open(GOLDEN))[entry]
    got = observe(tmp_path_factory, entry)
    assert list(got) == list(want), "the case list and the fixture differ: regenerate neither, find out why"
    wrong = {name: (got[name], want[name]) for name in got if got[name] != want[name]}
    assert not wrong, "\n".join(f"{entry} {name}:\n  got  {g}\n  want {w}" for name, (g, w) in wrong.items())


def test_the_cases_reach_every_kind_of_outcome():
    """the fixture itself: every entry is refused at the scaffold, at the loader and in the library, answers below and at the
    limit, and every table is seen untouched, zeroed and filled"""
    gold = json.load(open(GOLDEN))
    assert list(gold) == list(ENTRIES)
    for entry, (has_mode, table, has_f) in ENTRIES.items():
        cases = gold[entry]
        assert cases["base"]["rc"] == 0 and cases["base"]["answers"] > 2 and cases["triangle_limit_below"]["answers"] == 2, entry
        assert cases["null_answers"]["error"] == f"{entry}: null argument", entry
        assert "<tmp>" in cases["missing_limit_full"]["error"], entry
        assert cases["disconnected_limit_full"]["error"].endswith("the query graph is not connected"), entry
        if table:
            assert {c["counts"].split(":")[0] for c in cases.values()} == {"untouched", "zeroed", "filled"}, entry
            assert {c["complete"] for c in cases.values()} == {COMPLETE_SENTINEL, 0, 1}, entry
        if has_f:
            assert cases["F_empty"]["rc"] == 0 and cases["F_empty"]["answers"] == 0, entry
