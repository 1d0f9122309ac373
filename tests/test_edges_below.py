"""gnnpe_csr_edges_below (include/gnnpe_hip.h, csrc/gnnpe_edges_below.hip) against numpy on uint64, and its host form on the same cases.

Yardstick: the key x * n + y of every entry, the reverse entry by np.searchsorted, the support as table.sum(axis=0) + the same at
the reverse entry (uint64 arithmetic: it wraps as the device's does), np.flatnonzero for the selection.  No code of the library.

Graphs: entry counts at the wave edges (2, 62, 64, 66) and around the 2 048-entry tile (2 046, 2 048, 2 050, 3 * 2 048 + 18).  Every
graph has isolated vertices; those of 2 046 entries and more have a row longer than 64 entries; those of more than 2 048 entries a
row that straddles a tile boundary (asserted here: the smaller ones have no room for either).
Tables: 1 and 3 rows of small random cells (1 .. 8, so that every support is at least 2), one edge whose two directions sum past
2^64, one edge with a huge cell on one direction only.
Patterns, through the threshold and the cells: none, all, only the first edge, only the last, about 1 %, about 50 %, threshold 0,
threshold 2^64 - 1.  For every pattern cap in {0, n - 1, n, n + 5}: the pairs, the canary behind min(cap, n), n_selected, min_kept,
and the table byte for byte."""
import ctypes as C

import numpy as np
import pytest

import peel_yardstick as py

pytestmark = pytest.mark.gpu

FULL = (1 << 64) - 1
TILE = 2048  # entries per tile of k_below_count / k_below_write (kBelowTile)
ENTRIES = (2, 62, 64, 66, TILE - 2, TILE, TILE + 2, 3 * TILE + 18)
CANARY = 0x5A5A5A5A
PATTERNS = ("none", "all", "first", "last", "1 %", "50 %", "threshold 0", "threshold 2^64 - 1")


def make_graph(entries):
    """a simple graph with exactly entries / 2 edges; ids 1 and n - 1 stay isolated"""
    m = entries // 2
    for seed in range(200):
        rng = np.random.default_rng(7000 + entries + seed)
        n = m + 5 if m < 100 else m // 4 + 10
        free = np.setdiff1d(np.arange(n), [1, n - 1])
        edges = set()
        if m >= 100:  # a row longer than 64 entries, in the middle of the ids
            hub = int(free[len(free) // 2])
            edges = {(min(hub, int(v)), max(hub, int(v))) for v in rng.choice(np.setdiff1d(free, [hub]), 70, replace=False)}
        while len(edges) < m:
            a, b = sorted(int(v) for v in rng.choice(free, 2, replace=False))
            edges.add((a, b))
        g = py.graph_from(n, edges, np.zeros(n))
        off = g["offsets"].astype(np.int64)
        straddles = any(((off[:-1] < b) & (off[1:] > b)).any() for b in range(TILE, entries, TILE))
        if entries <= TILE or straddles:
            break
    deg = np.diff(off)
    assert len(g["nbrs"]) == entries and deg[1] == 0 and deg[n - 1] == 0
    assert m < 100 or deg.max() > 64
    assert entries <= TILE or straddles
    return g


def entry_arrays(g):
    n = g["n"]
    x = np.repeat(np.arange(n, dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    y = g["nbrs"].astype(np.int64)
    keys = x * n + y
    rev = np.searchsorted(keys, y * n + x)
    assert np.array_equal(keys[rev], y * n + x)
    return x, y, rev


def reference(g, table, threshold):
    """(pairs int64 [k, 2], n_selected, min_kept) in numpy"""
    x, y, rev = entry_arrays(g)
    with np.errstate(over="ignore"):
        col = table.sum(axis=0, dtype=np.uint64)
        sup = col + col[rev]
    fwd = x < y
    sel = fwd & (sup < np.uint64(threshold))
    kept = sup[fwd & ~sel]
    return np.column_stack([x[sel], y[sel]]), int(sel.sum()), int(kept.min()) if len(kept) else FULL


def cases(g, n_rows, rng):
    """(pattern, table, threshold) for every pattern"""
    x, y, rev = entry_arrays(g)
    entries = len(x)
    fwd = np.flatnonzero(x < y)
    base = rng.integers(1, 9, (n_rows, entries)).astype(np.uint64)
    if len(fwd) >= 2:  # the two directions sum past 2^64: FULL - 2 + 5 wraps to 2 (+ the other rows)
        j = fwd[len(fwd) // 2]
        base[0, j], base[0, rev[j]] = FULL - 2, 5
    if len(fwd) >= 3:  # a huge cell on one direction only
        j = fwd[len(fwd) // 3]
        base[n_rows - 1, rev[j]] = (1 << 63) + 12345
    sup = reference(g, base, 0)

    def zeroed(which):
        t = base.copy()
        t[:, which] = 0
        t[:, rev[which]] = 0
        return t

    with np.errstate(over="ignore"):
        col = base.sum(axis=0, dtype=np.uint64)
        all_sup = (col + col[rev])[fwd]
    out = [("none", base, int(all_sup.min())), ("all", base, int(all_sup.max()) + 1), ("first", zeroed(fwd[:1]), 1), ("last", zeroed(fwd[-1:]), 1),
           ("1 %", zeroed(fwd[rng.random(len(fwd)) < 0.01]), 1), ("50 %", base, int(np.sort(all_sup)[len(all_sup) // 2])),
           ("threshold 0", base, 0), ("threshold 2^64 - 1", base, FULL)]
    assert int(all_sup.max()) < FULL and sup[1] == 0
    return out


@pytest.mark.parametrize("entries", ENTRIES)
def test_gpu_edges_below_against_numpy(entries):
    import torch
    from gnnpe_amd import binding
    g = make_graph(entries)
    rng = np.random.default_rng(100 + entries)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    seen = {}
    for n_rows in (1, 3):
        for pattern, table, threshold in cases(g, n_rows, rng):
            want, n, low = reference(g, table, threshold)
            seen[pattern] = n
            assert np.all(want[:, 0] < want[:, 1]) and np.all(np.diff(want[:, 0] * g["n"] + want[:, 1]) > 0)  # ascending and unique
            dev = torch.from_numpy(table.view(np.int64).copy()).cuda()
            for cap in sorted({0, max(n - 1, 0), n, n + 5}):
                pairs = torch.full((max(cap, n) + 8, 2), CANARY, dtype=torch.int32, device="cuda")
                got_n, got_low = eng.edges_below(dev, n_rows, threshold, pairs, cap)
                what = (entries, n_rows, pattern, cap)
                assert (got_n, got_low) == (n, low), (what, got_n, n, got_low, low)
                host = pairs.cpu().numpy().view(np.uint32).astype(np.int64)
                k = min(cap, n)
                assert np.array_equal(host[:k], want[:k]), (what, "pairs")
                assert (host[k:] == CANARY).all(), (what, "canary")
                assert dev.cpu().numpy().tobytes() == table.tobytes(), (what, "the table changed")
            # the host form on the same case
            hp, hn, hlow = binding.host_edges_below(g, table, threshold)
            assert (hn, hlow) == (n, low) and np.array_equal(hp.astype(np.int64), want), (entries, n_rows, pattern, "host form")
            # without a pair buffer: the counts alone
            assert eng.edges_below(dev, n_rows, threshold) == (n, low)
    m = entries // 2
    assert seen["none"] == 0 and seen["threshold 0"] == 0 and seen["all"] == m and seen["threshold 2^64 - 1"] == m
    assert seen["first"] == seen["last"] == 1 and (m < 4 or 0 < seen["50 %"] < m)
    eng.close()


def test_gpu_edges_below_without_edges():
    import torch
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    eng.load_csr(np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(5, np.uint32))
    dev = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert eng.edges_below(dev, 1, 7) == (0, FULL)
    eng.close()


def test_gpu_edges_below_refusals():
    import torch
    from gnnpe_amd import binding
    g = make_graph(66)
    entries = len(g["nbrs"])
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    table = torch.arange(1, 2 * entries + 2, dtype=torch.int64, device="cuda")
    pairs = torch.full((entries, 2), CANARY, dtype=torch.int32, device="cuda")
    before = (table.cpu().numpy().tobytes(), pairs.cpu().numpy().tobytes())
    lib, ctx = eng.lib, eng.ctx
    n, low = C.c_uint64(77), C.c_uint64(78)
    vp = lambda t, shift=0: C.c_void_p(t.data_ptr() + shift)
    refused = {
        "a null context": (None, vp(table), 2, 5, vp(pairs), 4, C.byref(n), C.byref(low)),
        "a null table": (ctx, None, 2, 5, vp(pairs), 4, C.byref(n), C.byref(low)),
        "a null n_selected": (ctx, vp(table), 2, 5, vp(pairs), 4, None, C.byref(low)),
        "a null min_kept": (ctx, vp(table), 2, 5, vp(pairs), 4, C.byref(n), None),
        "a misaligned table": (ctx, vp(table, 4), 2, 5, vp(pairs), 4, C.byref(n), C.byref(low)),
        "pairs inside the table": (ctx, vp(table), 2, 5, vp(table, 8 * entries), 4, C.byref(n), C.byref(low)),
        "cap without pairs": (ctx, vp(table), 2, 5, None, 4, C.byref(n), C.byref(low)),
        "no rows": (ctx, vp(table), 0, 5, vp(pairs), 4, C.byref(n), C.byref(low)),
    }
    for what, args in refused.items():
        assert lib.gnnpe_csr_edges_below(*args, None) == -1, what
        torch.cuda.synchronize()
        assert (table.cpu().numpy().tobytes(), pairs.cpu().numpy().tobytes()) == before, what
        assert (n.value, low.value) == (77, 78), what
    # the multigraph state and a slab context
    offs64 = g["offsets"].astype(np.uint64)
    eng.set_multigraph_rows(offs64, g["nbrs"])
    with pytest.raises(binding.GnnpeError, match="simple graphs only"):
        eng.edges_below(table, 2, 5, pairs, 4)
    rows = np.arange(0, g["n"], 2, dtype=np.uint32)
    deg = np.diff(g["offsets"].astype(np.int64))
    row_off = np.concatenate([[0], np.cumsum(deg[rows])]).astype(np.uint64)
    row_nb = np.concatenate([g["nbrs"][g["offsets"][v]:g["offsets"][v + 1]] for v in rows]).astype(np.uint32)
    eng.load_rows(g["n"], g["labels"], rows, row_off, row_nb)
    with pytest.raises(binding.GnnpeError, match="whole graph"):
        eng.edges_below(table, 2, 5, pairs, 4)
    assert (table.cpu().numpy().tobytes(), pairs.cpu().numpy().tobytes()) == before
    # and after a proper load the call works again
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    t2 = table[:2 * entries].cpu().numpy().view(np.uint64).reshape(2, entries)
    assert eng.edges_below(table, 2, 5, pairs, 4)[0] == reference(g, t2, 5)[1]
    eng.close()
