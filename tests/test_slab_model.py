"""The numpy model of the slab exchange (tests/slab_support.py) held to the oracle and to tests/fake_engine.py: the
GPU tests compare every C-ABI helper with this model, so the model has to be right first.  No GPU."""
import numpy as np
import pytest
import torch

import slab_support as ss
from fake_engine import FakeEngine


@pytest.fixture(scope="module")
def G():
    return ss.build_graph()


@pytest.fixture(scope="module")
def paths(oracle, G):
    return {l: oracle.enumerate_closed(G["offsets"], G["nbrs"], G["sorted_nodes"], l + 1) for l in (2, 3)}


BSETS = list(ss.bounds_sets(600))
ALL_SETS = BSETS + ["R64_small"]  # 64 ranks over the ten vertices of build_small_graph: n < n_ranks, most slabs empty


@pytest.fixture(scope="module")
def S():
    return ss.build_small_graph()


@pytest.fixture(scope="module")
def small_paths(oracle, S):
    return {l: oracle.enumerate_closed(S["offsets"], S["nbrs"], S["sorted_nodes"], l + 1) for l in (2, 3)}


def _model(G, name):
    b = ss.small_bounds(G["n"]) if name == "R64_small" else ss.bounds_sets(G["n"])[name]
    return ss.SlabModel(G["offsets"], G["nbrs"], G["sorted_nodes"], b)


def test_small_graph_spreads_over_64_ranks(S, small_paths):
    m = _model(S, "R64_small")
    lens = np.diff(m.bounds)
    assert S["n"] == 10 and m.R == 64 and (lens == 1).sum() == 10 and (lens == 0).sum() == 54
    assert lens[0] == 0 and lens[-1] == 1  # the first slab is empty, the last one is not
    assert np.array_equal(np.sort(m.owner(np.arange(10))), np.flatnonzero(lens))
    assert len(small_paths[2]) > 0 and len(small_paths[3]) > 0


def test_graph_has_the_planted_rows(G):
    deg = np.diff(G["offsets"].astype(np.int64))
    assert tuple(deg[:10]) == ss.PLANTED_DEGREES and G["n"] == 600 and G["m"] == 2400
    assert int(G["labels"].max()) == 4
    rank = np.empty(600, np.int64)
    rank[G["sorted_nodes"].astype(np.int64)] = np.arange(600)
    # ranks are mixed inside the rows: no planted row is ascending in rank
    for v in range(2, 10):
        r = rank[G["nbrs"][G["offsets"][v]:G["offsets"][v + 1]].astype(np.int64)]
        assert np.any(np.diff(r) < 0) and np.any(np.diff(r) > 0)


@pytest.mark.parametrize("name", [b for b in BSETS if b != "R1"])
def test_planted_rows_land_in_a_halo(G, name):
    """Every planted row that anybody refers to (degree >= 1) is fetched by a rank that does not own it (the seed of
    slab_support.build_graph was chosen for that: with another one the single neighbour of vertex 1 may share its slab)."""
    m = _model(G, name)
    for v in range(1, 10):
        assert m.in_some_halo(v), (name, v)
    assert not m.in_some_halo(0)  # degree 0: nobody refers to it


def test_owner_skips_empty_slabs(G):
    m = _model(G, "R5_empty_ends")
    own = m.owner(np.arange(600))
    assert set(own.tolist()) == {1, 2, 3}
    for r in range(m.R):
        assert np.array_equal(np.sort(np.flatnonzero(own == r)), np.sort(m.owned(r)))
    m = _model(G, "R3_empty_middle")
    assert set(m.owner(np.arange(600)).tolist()) == {0, 2}


@pytest.mark.parametrize("l", [2, 3])
@pytest.mark.parametrize("name", ALL_SETS)
def test_held_rows_suffice_for_the_slab_paths(G, paths, S, small_paths, name, l):
    """Hops 1..l-1 installed as dist.SlabBuild.install_halo does (last hop truncated at bounds[r]): every adjacency
    entry a path of slab r walks over is present in the rows rank r holds."""
    if name == "R64_small":
        G, paths = S, small_paths
    m = _model(G, name)
    P = paths[l]
    covered = 0
    for r in range(m.R):
        held, _ = m.hops(r, l)
        have = np.unique(held.pairs())
        p = m.slab_paths(P, r).astype(np.int64)
        covered += len(p)
        for j in range(l):
            used = (p[:, j] << 32) | p[:, j + 1]
            assert np.all(np.isin(used, have)), (name, l, r, j)
    assert covered == len(P) and covered > 0


@pytest.mark.parametrize("name", [b for b in BSETS if b != "R1"])
def test_truncation_keeps_nothing_and_everything_somewhere(G, name):
    """The edges of the truncation that the GPU tests rely on.  A first-hop row always keeps an entry (the owned vertex
    that referred to it), so a row that keeps NOTHING exists on the second hop only; rows that keep everything although
    the slab does not start at 0 exist on the first."""
    m = _model(G, name)
    none = all_ = False
    for r in range(m.R):
        if m.bounds[r] == 0:
            continue
        h2, _ = m.hops(r, 2)
        for v in h2.halo_ids():
            assert len(h2.rows[int(v)]) > 0
            all_ |= len(h2.rows[int(v)]) == m.deg[v]
        h3, lists = m.hops(r, 3)
        none |= any(len(h3.rows[int(v)]) == 0 and m.deg[v] > 0 for v in lists[1][0])
    assert none and all_, (name, none, all_)


@pytest.mark.parametrize("name", ["R2", "R3_empty_middle", "R5_empty_ends", "R64_small"])
def test_model_agrees_with_the_fake_engine(oracle, G, S, name):
    """Need lists of both hops and the truncated rows, against the stand-in engine of the gloo tests."""
    if name == "R64_small":
        G = S
    m = _model(G, name)
    n = G["n"]
    for r in range(m.R):
        rows, roff, rn = m.owned_csr(r)
        fe = FakeEngine(oracle, n, G["labels"], rows, roff, rn, G["sorted_nodes"], 2)
        held = m.start(r)
        for hop, min_rank in ((0, 0), (1, int(m.bounds[r]))):
            buf = torch.zeros(n, dtype=torch.int32)
            counts = fe.halo_need(m.bounds, buf, n)
            ids, mc = m.need(held)
            assert np.array_equal(counts.astype(np.int64), mc), (name, r, hop)
            assert np.array_equal(buf[:len(ids)].numpy().astype(np.int64), ids), (name, r, hop)
            deg, nb = m.concat_rows(ids)
            fe.rows_append(len(ids), torch.from_numpy(ids), torch.from_numpy(deg), torch.from_numpy(nb.astype(np.int32)),
                           len(nb), min_rank)
            m.install(held, ids, min_rank)
            for v in ids:
                assert np.array_equal(fe.halo[int(v)], held.rows[int(v)]), (name, r, hop, int(v))
