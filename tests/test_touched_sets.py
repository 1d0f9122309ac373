"""Touched vertex sets made and used on the device (include/gnnpe_hip.h, "touched sets on the device"): gnnpe_csr_closed_neighbourhood,
gnnpe_csr_carry_vertex_set and gnnpe_filter_support_exact_delta_device, against numpy and against the host-list support call; and
the resident form of "S n C(u)" of the vertex-anchored searches (k_vset_member_of), through the standing query's relabel call.

Yardsticks: np.unique over the CSR rows for T = R u N(R); fs.apply_vertices_np's new ids for the carried set; for the support call
the table bytes gnnpe_filter_support_exact_delta leaves for the same T; for the membership the brute-force match sets of
tests/test_standing_query.py.

Shapes: the n = 301 graph of the support tests (a hub row of 64 entries that an insert takes to 65, one isolated vertex) with one
vertex joined to all others (a row of 300), and paths of n vertices around the word edges and around the 8192-vertex tile of the
compaction."""
import os
import re

import numpy as np
import pytest

import test_filter_support as fs
from conftest import ROOT
from test_standing_query import QUERIES, match_set, as_mode, path_graph, write_query, pack

E = 2
HUB, ISOLATED = fs.HUB, fs.ISOLATED
TILE = 8192  # vertices per step of the ordered compaction
PATH_N = (1, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1)
CANARY = 0xDEADBEEF
NAMES_HIP = ("gnnpe_csr_closed_neighbourhood", "gnnpe_csr_carry_vertex_set", "gnnpe_filter_support_exact_delta_device")
NAMES_ONLINE = ("gnnpe_standing_set_labels", "gnnpe_standing_apply_vertices")


def test_symbols_are_exported_and_declared():
    from gnnpe_amd import binding
    binding.build()
    lib, online = binding.load(), binding.load_online()
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    for names, so, header, sigs in ((NAMES_HIP, lib, "gnnpe_hip.h", binding.SIGNATURES),
                                    (NAMES_ONLINE, online, "gnnpe_online.h", binding.ONLINE_SIGNATURES)):
        decl = set(re.findall(r"\b(gnnpe_[a-z0-9_]+)\s*\(", strip(header)))
        for name in names:
            assert hasattr(so, name), name
            assert name in decl and name in sigs, name
    assert lib.gnnpe_abi_version() == binding.ABI_VERSION == 20
    for method in ("closed_neighbourhood", "carry_vertex_set", "filter_support_delta_device", "standing_set_labels", "standing_apply_vertices"):
        assert callable(getattr(binding.Engine, method))


def row_graph():
    """make_graph(hub_deg=64) with one more edge at the hub (a row of 65) and 65 more vertices, 366 in all: vertex 5 joined to 300
    vertices, 303 to 63, 302 to 64, 301 to one; the isolated vertex keeps its empty row"""
    g = fs.make_graph(hub_deg=64)
    edges = set(g["edges"])
    edges.add((next(v for v in range(300) if (v, HUB) not in edges and v != ISOLATED), HUB))
    edges |= {(min(5, v), max(5, v)) for v in range(300) if v not in (5, ISOLATED)} | {(5, 301), (5, 303)}
    edges |= {(303, 304 + i) for i in range(62)}
    edges |= {(302, 304 + i) for i in range(62)} | {(1, 302), (2, 302)}
    return fs.graph_of(366, edges, np.concatenate([g["labels"], np.zeros(65, np.uint32)]))


def closed_np(g, R):
    R = np.asarray(R, np.int64)
    return np.unique(np.concatenate([R] + [fs.nbrs_of(g, int(v)) for v in R])) if len(R) else np.zeros(0, np.int64)


def dev_set(n, extra=16):
    """a bitmap full of ones and an id list full of canaries on the device"""
    import torch
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")
    ids = torch.full((n + extra,), CANARY - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return bits, ids


def host(t):
    return t.cpu().numpy().view(np.uint32)


def check_set(bits, ids, count, want, n, cap, what):
    """every word of the bitmap, the ids, and the words behind them"""
    want = np.asarray(want, np.int64)
    assert count == len(want), (what, count, len(want))
    b = host(bits)
    assert np.array_equal(fs.bits_of(b.reshape(1, -1), n)[0], np.isin(np.arange(n), want)), (what, "bitmap")
    assert n % 32 == 0 or not (b[-1] >> np.uint32(n % 32)), (what, "bits past n")
    i = host(ids)
    assert np.array_equal(i[:min(cap, len(want))], want[:cap]), (what, "ids")
    assert np.all(i[cap:] == CANARY), (what, "ids written past ids_cap")
    if cap >= len(want):
        assert np.all(i[len(want):] == CANARY), (what, "ids written past the set")


@pytest.mark.gpu
def test_gpu_closed_neighbourhood_rows():
    from gnnpe_amd import binding
    g = row_graph()
    n = g["n"]
    deg = np.diff(g["offsets"].astype(np.int64))
    assert [deg[v] for v in (ISOLATED, 301, 303, 302, HUB, 5)] == [0, 1, 63, 64, 65, 300]
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    shared = [int(x) for x in fs.nbrs_of(g, HUB)[:2]]  # two vertices of R with the hub (and vertex 5) as a common neighbour
    word = [304 + i for i in range(8)]  # their neighbours 302 and 303 and they themselves are in one bitmap word (288 .. 319)
    cases = {"row of 0": [ISOLATED], "row of 1": [301], "row of 63": [303], "row of 64": [302], "row of 65": [HUB], "row of 300": [5],
             "a shared neighbour": shared, "one word": word, "repeats": [HUB, 7, HUB, 7, 7, 301], "nothing": [],
             "all": list(range(n)), "many": list(range(0, n, 3))}
    for what, R in cases.items():
        want = closed_np(g, R)
        bits, ids = dev_set(n)
        for timing in (False, True):
            got = eng.closed_neighbourhood(R, bits, ids, ids_cap=n, timing=timing)
            count = got[0] if timing else got
            assert not timing or got[1] >= 0.0
            check_set(bits, ids, count, want, n, n, what)
        if len(want) > 1:  # ids_cap below the true number: refused, *n_ids set, the bitmap written, nothing behind the cap
            bits, ids = dev_set(n)
            cap = len(want) // 2
            with pytest.raises(binding.GnnpeError, match="ids_cap") as err:
                eng.closed_neighbourhood(R, bits, ids, ids_cap=cap)
            assert "[-1]" in str(err.value) and eng.last_set_size == len(want), what
            check_set(bits, ids, len(want), want, n, cap, (what, "cap"))
    # refusals before any launch: the buffers stay as they were
    bits, ids = dev_set(n)
    for R, msg in (([3, n], str(n)), ([n + 7], "not a vertex")):
        with pytest.raises(binding.GnnpeError, match=msg):
            eng.closed_neighbourhood(R, bits, ids)
    rc = eng.lib.gnnpe_csr_closed_neighbourhood(eng.ctx, None, 2, bits.data_ptr(), ids.data_ptr(), n, None, None)
    assert rc == -1 and b"null argument" in eng.lib.gnnpe_last_error()
    assert np.all(host(bits) == 0xFFFFFFFF) and np.all(host(ids) == CANARY)
    eng.close()
    # a multigraph context and a slab-only context
    eng = binding.Engine(0)
    eng.load_multigraph(np.array([0, 2, 4], np.uint32), np.array([1, 1, 0, 0], np.uint32), np.zeros(2, np.uint32))
    with pytest.raises(binding.GnnpeError, match=r"\[-3\]"):
        eng.closed_neighbourhood([0], bits, ids)
    eng.close()
    eng = binding.Engine(0)
    rows = np.arange(10, dtype=np.uint32)
    ro = np.concatenate([[0], np.cumsum(deg[:10])]).astype(np.uint64)
    eng.load_rows(g["n"], g["labels"], rows, ro, g["nbrs"][:int(ro[-1])])
    with pytest.raises(binding.GnnpeError, match=r"\[-3\]"):
        eng.closed_neighbourhood([0], bits, ids)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PATH_N)
def test_gpu_closed_neighbourhood_paths(n):
    from gnnpe_amd import binding
    g = path_graph(n)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    rng = np.random.default_rng(3000 + n)
    cases = [[0], [n - 1], list(range(n)), list(range(0, n, 3)), sorted(rng.choice(n, max(1, n // 50), replace=False).tolist())]
    cases += [[31, 32], [63, 64]] if n > 64 else []
    for R in cases:
        want = closed_np(g, R)
        bits, ids = dev_set(n)
        check_set(bits, ids, eng.closed_neighbourhood(R, bits, ids, ids_cap=n), want, n, n, (n, R[:4]))
    eng.close()


CARRY = {  # name: (n before, removed, added)
    "first and last": (301, [0, 300], 0),
    "up over 320": (301, [0], 25),
    "down under 288": (301, list(range(0, 28, 2)), 0),
    "added across a word": (301, [5, 6, 7], 40),  # the added ids 298..337 straddle 320
    "to a multiple of 32": (301, [], 19),
    "only added": (64, [], 3),
    "one left": (33, list(range(32)), 0),
    "over a tile": (TILE - 1, [10], 5),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CARRY))
def test_gpu_carry_vertex_set(case):
    import torch
    from gnnpe_amd import binding
    n, rem, k_add = CARRY[case]
    g = fs.make_graph(hub_deg=64) if n == 301 else path_graph(n)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    rng = np.random.default_rng(len(case))
    sets = [closed_np(g, rem), np.arange(n), np.zeros(0, np.int64), np.flatnonzero(rng.random(n) < 0.3), np.array([0, n - 1])]
    old = []
    for T in sets:  # made on the graph of before
        bits, _ = dev_set(n)
        bits.copy_(torch.from_numpy(pack(np.isin(np.arange(n), T)[None, :])[0].view(np.int32)))
        old.append(bits)
    torch.cuda.synchronize()
    # no valid map yet
    nb, ni = dev_set(n + k_add)
    with pytest.raises(binding.GnnpeError, match="no valid vertex map"):
        eng.carry_vertex_set(old[0], nb, ni)
    g2, new_id = fs.apply_vertices_np(g, rem, [0] * k_add)
    n2 = eng.apply_vertices(rem, [0] * k_add)[0]
    assert n2 == g2["n"]
    added = np.arange(n2 - k_add, n2)
    for T, bits in zip(sets, old):
        for with_added in (False, True):
            moved = new_id[np.asarray(T, np.int64)]
            want = np.unique(np.concatenate([moved[moved >= 0], added if with_added else []])).astype(np.int64)
            nb, ni = dev_set(n2)
            count = eng.carry_vertex_set(bits, nb, ni, with_added=with_added, ids_cap=n2)
            check_set(nb, ni, count, want, n2, n2, (case, len(T), with_added))
            if len(want) > 1:
                nb, ni = dev_set(n2)
                with pytest.raises(binding.GnnpeError, match="ids_cap"):
                    eng.carry_vertex_set(bits, nb, ni, with_added=with_added, ids_cap=len(want) - 1)
                assert eng.last_set_size == len(want)
                check_set(nb, ni, len(want), want, n2, len(want) - 1, (case, "cap"))
    # overlapping bitmaps, then a following edge batch ends the map
    nb, ni = dev_set(n2)
    with pytest.raises(binding.GnnpeError, match="overlap"):
        eng.carry_vertex_set(nb, nb, ni)
    if n2 >= 2:
        eng.apply_edges(insert=[next((x, y) for x in range(n2) for y in range(x + 1, n2) if (x, y) not in g2["edges"])])
        with pytest.raises(binding.GnnpeError, match="no valid vertex map"):
            eng.carry_vertex_set(old[0], nb, ni)
        assert np.all(host(nb) == 0xFFFFFFFF) and np.all(host(ni) == CANARY), "a refused carry wrote something"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("l", [2, 3])
def test_gpu_support_delta_device_equals_the_host_list(tmp_path, l):
    """for the same T the device-list call and the host-list call leave byte-equal tables: sign +1 and -1, T of one vertex, T at the
    hub of 150 entries (n_slices > 1), T = V"""
    import torch
    g = fs.make_graph()
    n = g["n"]
    eng = fs.open_engine(g, E)
    assert eng.rows_held()[2] >= 1  # a hub row: the items of a list are cut into slices
    moved = 0  # the calls that changed the table at all
    sets = {"one": [7], "hub": closed_np(g, [HUB]), "isolated": [ISOLATED], "some": closed_np(g, [3, 50, 200]), "V": np.arange(n)}
    for k, plan in enumerate(fs.make_plans(g, E, l, tmp_path, 21)):
        nq = int(plan["n_vertices"])
        for what, T in sets.items():
            bits, ids = dev_set(n)
            T = np.asarray(T, np.int64)
            bits.copy_(torch.from_numpy(pack(np.isin(np.arange(n), T)[None, :])[0].view(np.int32)))
            ids[:len(T)].copy_(torch.from_numpy(T.astype(np.uint32).view(np.int32)))
            torch.cuda.synchronize()
            for sign in (1, -1):
                a, pat = fs.pattern(nq, n)
                b, _ = fs.pattern(nq, n)
                eng.filter_support_delta(plan, T[::-1], sign, a)  # the host list in another order
                ms = eng.filter_support_delta_device(plan, bits, ids, len(T), sign, b)
                assert ms >= 0.0 and torch.equal(a, b), (l, k, what, sign)
                moved += not np.array_equal(fs.to_np(b), pat)
        # T from closed_neighbourhood itself, and the empty set
        bits, ids = dev_set(n)
        count = eng.closed_neighbourhood([HUB, 3], bits, ids)
        a, pat = fs.pattern(nq, n)
        b, _ = fs.pattern(nq, n)
        eng.filter_support_delta(plan, closed_np(g, [HUB, 3]), 1, a)
        eng.filter_support_delta_device(plan, bits, ids, count, 1, b)
        assert torch.equal(a, b), (l, k, "from closed_neighbourhood")
        eng.filter_support_delta_device(plan, bits, ids, 0, 1, b)
        assert torch.equal(a, b), (l, k, "the empty set")
    assert moved >= 12, moved
    # refusals: the table's bytes stay
    from gnnpe_amd import binding
    plan = fs.make_plans(g, E, l, tmp_path, 21)[0]
    b, pat = fs.pattern(int(plan["n_vertices"]), n)
    bits, ids = dev_set(n)
    for args, msg in (((bits, ids, 1, 2), "sign"), ((bits, ids, n + 1, 1), "ids"), ((None, ids, 1, 1), "aligned"),
                      ((bits, ids.data_ptr() + 2, 1, 1), "aligned")):
        with pytest.raises(binding.GnnpeError, match=msg):
            eng.filter_support_delta_device(plan, args[0], args[1], args[2], args[3], b)
    assert np.array_equal(fs.to_np(b), pat)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_gpu_resident_membership_through_a_relabel(tmp_path, k):
    """S n C(u) of the vertex-anchored searches from the device bitmap: relabel batches of 1, 63, 64 and 65 vertices, the last vertex
    of the graph (in the last, partial word of a row) among them, on a handle whose sets never reach the host.  What the searches
    find depends on every answer of the membership kernel: a vertex wrongly left out loses its matches, one wrongly taken in is a
    start candidate outside C(u) -- the kernels do not test the start candidate against its set again."""
    g = fs.make_graph(hub_deg=64)
    n = g["n"]
    name, query = "wedge", QUERIES["wedge"]
    qp = write_query(tmp_path, name)
    rng = np.random.default_rng(100 + k)
    R = [n - 1] + sorted(rng.choice(n - 1, k - 1, replace=False).tolist())
    labels = (g["labels"][R] + 1 + (np.arange(k) % 2)) % fs.NL
    eng = fs.open_engine(g, E)
    handles = [(eng.standing_open(qp, l=2, distinct=d, induced=i, rows_cap=1 << 18), (d, i)) for d, i in ((False, False), (True, True))]
    eng.standing_set_labels(R, labels)
    new = g["labels"].copy()
    new[R] = labels
    g2 = fs.graph_of(n, g["edges"], new)
    moved = 0
    for sq, m in handles:
        M0, M1 = match_set(g, query, *m), match_set(g2, query, *m)
        count, created, destroyed = sq.result()[:3]
        assert (count, created, destroyed) == (len(M1), len(M1 - M0), len(M0 - M1)), (k, m)
        assert as_mode(sq.rows(0), query, m[0]) == sorted(M1 - M0) and as_mode(sq.rows(1), query, m[0]) == sorted(M0 - M1), (k, m)
        moved += created + destroyed
    assert moved > 0
    eng.close()
