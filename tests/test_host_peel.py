"""The host forms of the peel (gnnpe_host_csr_edges_below of include/gnnpe_hip.h, gnnpe_host_truss_levels of include/gnnpe_online.h)
against the Python yardstick of tests/peel_yardstick.py, on the cascade graph and on G(30, 90).  No GPU is needed."""
import os
import re

import numpy as np
import pytest

import peel_yardstick as py
from conftest import ROOT
from test_standing_query import QUERIES, write_query

FULL = (1 << 64) - 1
NEW_HIP = {"gnnpe_csr_edges_below", "gnnpe_host_csr_edges_below"}
NEW_ONLINE = {"gnnpe_standing_peel", "gnnpe_standing_truss_levels", "gnnpe_host_truss_levels"}


def label_bitmap(g, query):
    from test_standing_query import pack
    return pack(np.array([g["labels"] == lb for lb in query[2]]))


def graphs():
    g = py.gnm(30, 90, seed=5, n_labels=1)
    g["labels"][:] = 1  # the triangle's label
    return {"cascade": py.cascade_graph(), "gnm": g}


def test_the_new_names_are_declared_bound_and_exported():
    from gnnpe_amd import binding
    for header, names, sigs, lib in (("gnnpe_hip.h", NEW_HIP, binding.SIGNATURES, binding.load()),
                                     ("gnnpe_online.h", NEW_ONLINE, binding.ONLINE_SIGNATURES, binding.load_online())):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, txt), (header, name)
            assert name in sigs and hasattr(lib, name), name
    assert binding.load().gnnpe_abi_version() == 20


def test_the_cascade_is_telling():
    g, query = py.cascade_graph(), QUERIES["triangle"]
    left, removed, rounds, out = py.peel(g, query, True, 2)
    assert out[0] >= 5 and out[3] == 1 and left["edges"] == py.K5 and 0 < len(removed) < g["m"], out
    # one step per round: no round is empty and the last edges to go touch the middle of the strip
    assert sorted(set(rounds)) == list(range(1, out[0] + 1))


@pytest.mark.parametrize("name", ["cascade", "gnm"])
@pytest.mark.parametrize("distinct", [False, True])
def test_host_edges_below_against_the_yardstick(tmp_path, name, distinct):
    from gnnpe_amd import binding
    g, query = graphs()[name], QUERIES["triangle"]
    qp = write_query(tmp_path, "triangle")
    answers, complete, table = binding.host_refine_sets_edge_counts(g, qp, label_bitmap(g, query), distinct=distinct)
    assert complete
    sup = py.supports(g, query, distinct)
    top = max(sup.values())
    assert top > 0 and min(sup.values()) < top
    for t in sorted({0, 1, 2, top // 2, top, top + 1, FULL}):
        want = sorted(e for e, s in sup.items() if s < t)
        kept = [s for s in sup.values() if s >= t]
        for cap in sorted({0, max(len(want) - 1, 0), len(want), len(want) + 5}):
            pairs, n_sel, low = binding.host_edges_below(g, table, t, cap=cap)
            assert n_sel == len(want) and low == (min(kept) if kept else FULL), (name, t, cap)
            assert [tuple(p) for p in pairs.tolist()] == want[:cap], (name, t, cap)
    with pytest.raises(binding.GnnpeError, match="rows"):
        binding.host_edges_below(g, np.zeros((0, len(g["nbrs"])), np.uint64), 1)


def test_host_edges_below_wraps_as_numpy_does():
    from gnnpe_amd import binding
    g = py.graph_from(4, {(0, 1), (1, 2), (2, 3)}, np.zeros(4))
    # entries: 0->1, 1->0, 1->2, 2->1, 2->3, 3->2
    table = np.array([[FULL - 2, 5, 1, 1, 1 << 63, 0], [0, 0, 1, 0, 0, 0]], np.uint64)
    pairs, n_sel, low = binding.host_edges_below(g, table, 3)
    assert pairs.tolist() == [[0, 1]] and n_sel == 1 and low == 3  # (0, 1) wraps to 2; (1, 2) has 3; (2, 3) has 2^63
    pairs, n_sel, low = binding.host_edges_below(g, table, 4)
    assert pairs.tolist() == [[0, 1], [1, 2]] and low == 1 << 63


@pytest.mark.parametrize("name", ["cascade", "gnm"])
@pytest.mark.parametrize("distinct", [False, True])
def test_host_truss_levels_against_the_yardstick(tmp_path, name, distinct):
    from gnnpe_amd import binding
    g, query = graphs()[name], QUERIES["triangle"]
    qp = write_query(tmp_path, "triangle")
    want = py.levels(g, query, distinct)
    edges, levels, out = binding.host_truss_levels(g, qp, label_bitmap(g, query), distinct=distinct)
    got = {tuple(e): int(lv) for e, lv in zip(edges.tolist(), levels.tolist())}
    assert len(got) == len(edges) == g["m"] and got == want, name
    assert out[:3] == [g["m"], len(set(want.values())), max(want.values())] and len(set(want.values())) > 1, out
    assert (np.diff(levels.astype(np.int64)) >= 0).all(), "removal order is by level"
    # the rounds: per level the yardstick's peel at level + 1 from the truss of that level
    rounds, cur = 0, g
    for lv in sorted(set(want.values())):
        cur, _, _, o = py.peel(cur, query, distinct, lv + 1)
        rounds += o[0]
    assert out[3] == rounds and cur["m"] == 0


def test_host_truss_levels_refusals(tmp_path):
    from gnnpe_amd import binding
    g = py.cascade_graph()
    qp = write_query(tmp_path, "triangle")
    bm = label_bitmap(g, QUERIES["triangle"])
    import ctypes as C
    online = binding.load_online()
    args = lambda mode: (g["n"], binding._ptr(g["offsets"], binding._u32p), binding._ptr(g["nbrs"], binding._u32p), binding._ptr(g["labels"], binding._u32p),
                         qp.encode(), binding._ptr(bm, binding._u32p), mode, None, None, 0, (C.c_uint64 * 4)())
    assert online.gnnpe_host_truss_levels(*args(2)) == -3  # GNNPE_ERR_UNSUPPORTED: induced
    assert online.gnnpe_host_truss_levels(*args(8)) == -1
    assert online.gnnpe_host_truss_levels(*args(0)) == 0
