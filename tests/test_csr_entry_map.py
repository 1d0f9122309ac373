"""The entry map of an edge batch and a per-entry table carried through it (include/gnnpe_hip.h, ABI version 20):
gnnpe_host_csr_entry_map on the host, gnnpe_csr_apply_edges_map and gnnpe_csr_carry_entries on the graph a context holds.

The yardstick for a map is numpy, never the library: the keys x * n + y of a compact simple CSR ascend, so the map is the
searchsorted of the new keys among the old ones plus an equality test.  The graph after a batch is test_csr_apply_edges._apply_np's.
The maintained edge tables are held to refine_sets_edge_counts of a FRESH engine that loaded numpy's graph."""
import ctypes as C
import time

import numpy as np
import pytest

import test_csr_apply_edges as ap
import test_online_exact as ex
import test_refine_delta as dl
import test_refine_delta_counts as rdc
import test_refine_edge_counts as re_
import test_refine_sets_shapes as sh

NO = 0xFFFFFFFF  # GNNPE_NO_ENTRY
ERR_ARG = -1
MERGE_TILE = 2048  # kMergeTile of csrc/gnnpe_update.hip: entries of the old array per streaming block and step
CANARY64, CANARY32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _map_np(g_old, g_new):
    """the numpy yardstick: for every entry of g_new its index among the entries of g_old, NO where g_old does not have it"""
    k0, k1 = re_._csr_keys(g_old)[1], re_._csr_keys(g_new)[1]
    if not len(k0):
        return np.full(len(k1), NO, np.uint32)
    pos = np.searchsorted(k0, k1)
    hit = (pos < len(k0)) & (k0[np.minimum(pos, len(k0) - 1)] == k1)
    return np.where(hit, pos, NO).astype(np.uint32)


def _pairs(a):
    return np.asarray(a, np.int64).reshape(-1, 2)


def _case(name, g, ins, dele, rng):
    ins, dele = _pairs(ins), _pairs(dele)
    g2 = ap._apply_np(g, ins, dele)
    return dict(name=name, g=g, g2=g2, ins_set=ins, del_set=dele, ins=ap._noisy(ins, rng), dele=ap._noisy(dele, rng), map=_map_np(g, g2))


_BATCHES, _PLACES = [], []


def _batch_cases(tmp_path_factory):
    """the 19 small graphs and H1, each with the four batch kinds of test_host_form_against_numpy applied in a row, then delete-all
    and insert-into-empty: 120 cases, the graph of a case being the result of the one before; computed once"""
    if _BATCHES:
        return _BATCHES
    graphs = ap._small_graphs() + [sh._h1(tmp_path_factory)["g"]]
    for gi, g0 in enumerate(graphs):
        rng = np.random.default_rng(5200 + gi)
        g = g0
        for ni, nd in ((7, 5), (9, 0), (0, 6), (len(g0["nbrs"]) // 8, len(g0["nbrs"]) // 8)):
            ins, dele = ap._random_batch(g, rng, ni, nd)
            _BATCHES.append(_case((gi, ni, nd), g, ins, dele, rng))
            g = _BATCHES[-1]["g2"]
        every = dl._und_edges(g)
        _BATCHES.append(_case((gi, "delete-all"), g, [], every, rng))
        _BATCHES.append(_case((gi, "insert-into-empty"), _BATCHES[-1]["g2"], every[:, ::-1], [], rng))
    return _BATCHES


def _place_graph():
    """G(700, 3000) with one label, edited so that every place of test 3 exists: vertex 350 is a hub row of 150 entries, all of them
    in [50, 650); vertex 123 is isolated; (0, 1), (5, 6) and (698, 699) are edges; 6 000 and some entries, so the streaming part
    takes three tiles"""
    from gnnpe_amd import synth
    n = 700
    g0 = synth.gnm_graph(n, 3000, n_labels=1, seed=5300)
    g = dict(n=n, offsets=g0["offsets"], nbrs=g0["nbrs"], labels=np.zeros(n, np.uint32))
    e = dl._und_edges(g)
    have = set(map(tuple, e.tolist()))
    rng = np.random.default_rng(5301)
    dele = [p for p in e.tolist() if 123 in p]
    row = set(e[(e == 350).any(axis=1)].ravel().tolist()) - {350}
    dele += [(min(350, w), max(350, w)) for w in row if (w < 50 or w >= 650) and w != 123]
    inside = sorted(w for w in row if 50 <= w < 650 and w != 123)
    pool = [w for w in rng.permutation(np.arange(50, 650)).tolist() if w not in row and w not in (350, 123)]
    ins = [(min(350, w), max(350, w)) for w in pool[:150 - len(inside)]]
    ins += [p for p in ((0, 1), (5, 6), (698, 699)) if p not in have]
    g = ap._apply_np(g, ins, dele)
    deg = np.diff(g["offsets"].astype(np.int64))
    assert deg[350] == 150 and deg[123] == 0 and len(g["nbrs"]) > 2 * MERGE_TILE + 500
    r350 = g["nbrs"][g["offsets"][350]:g["offsets"][351]]
    assert r350[0] >= 50 and r350[-1] < 650
    return g


def _place_cases(tmp_path_factory):
    """the places where the merge can go wrong (the docstring of test_gpu_places lists them), each a batch on _place_graph, with
    delete-all and insert-into-empty behind them; computed once.  An undirected edge touches the rows of both its ends, so `only the
    first row` is an edge between vertices 0 and 1 (no stretch in front of the touched rows) and `only the last row` one between
    n - 2 and n - 1 (no stretch behind them)"""
    if _PLACES:
        return _PLACES
    g = _place_graph()
    n = g["n"]
    o = g["offsets"].astype(np.int64)
    deg = np.diff(o)
    rng = np.random.default_rng(5302)
    row = lambda v: g["nbrs"][o[v]:o[v + 1]].astype(np.int64)
    is_edge = lambda x, y: y in row(x).tolist()

    def add(name, ins, dele, base=None):
        _PLACES.append(_case(name, g if base is None else base, ins, dele, rng))
        return _PLACES[-1]

    add("first row", [], [(0, 1)])
    add("last row", [], [(n - 2, n - 1)])
    add("first row, an insert", [(0, 1)], [], base=_PLACES[0]["g2"])  # ... into the graph that lost the edge
    v = next(x for x in range(10, n) if 3 <= deg[x] <= 12 and x not in (123, 350))
    c = add("a row that becomes empty", [], [(v, w) for w in row(v).tolist()])
    assert np.diff(c["g2"]["offsets"].astype(np.int64))[v] == 0
    c = add("an empty row receives its first entries", [(123, 7), (400, 123), (123, 699)], [])
    assert np.diff(c["g2"]["offsets"].astype(np.int64))[123] == 3
    half = n // 2
    every_i = [(i, i + half) for i in range(half) if not is_edge(i, i + half)]
    every_d = [(i, i + half) for i in range(half) if is_edge(i, i + half)]
    c = add("every row touched", every_i, every_d)
    assert (np.diff(c["g2"]["offsets"].astype(np.int64)) != deg).all()
    # the rows that hold old entries 2047 | 2048 and 4095 | 4096 between their first and last entry
    r1, r2 = (int(np.searchsorted(o, t, side="right")) - 1 for t in (MERGE_TILE, 2 * MERGE_TILE))
    for r, t in ((r1, MERGE_TILE), (r2, 2 * MERGE_TILE)):
        assert o[r] < t < o[r + 1] - 1 and r not in (123, 350), (r, t, o[r], o[r + 1])
    w1 = next(int(w) for w in row(r1) if w not in (r2, 350, 123))
    apart = lambda x: x not in (r1, r2, 350, 123) and not is_edge(x, r1) and not is_edge(x, r2)
    a = next(x for x in range(20, r1) if apart(x) and deg[x] >= 2)
    b = next(x for x in range(r2 + 1, n) if apart(x) and not is_edge(a, x))
    a2 = next(int(w) for w in row(a) if w not in (r1, r2))
    # r1 is touched (it loses an entry) and r2 is not, though rows in front of it change length; then the other way round
    c = add("a touched row across the first tile boundary, an untouched one across the second", [(a, b)], [(r1, w1), (a, a2)])
    d2 = np.diff(c["g2"]["offsets"].astype(np.int64))
    assert d2[r1] == deg[r1] - 1 and d2[r2] == deg[r2] and c["g2"]["offsets"][r2] != o[r2]
    w2 = next(int(w) for w in row(r2) if w not in (r1, 350, 123) and w > r1)  # (below r1 it would cancel a's new entry)
    c = add("an untouched row across the first tile boundary, a touched one across the second", [(a, b)], [(r2, w2)])
    d2 = np.diff(c["g2"]["offsets"].astype(np.int64))
    assert d2[r1] == deg[r1] and d2[r2] == deg[r2] - 1 and c["g2"]["offsets"][r1] != o[r1]
    hub = row(350)
    mid = next(w for w in range(int(hub[70]), int(hub[-1])) if w not in hub.tolist() and w != 350)
    c = add("a row of 150 entries: inserts below, between and above, its first and last entry deleted",
            [(350, 3), (mid, 350), (350, 697)], [(350, int(hub[0])), (int(hub[-1]), 350)])
    r2_ = c["g2"]["nbrs"][c["g2"]["offsets"][350]:c["g2"]["offsets"][351]]
    assert len(r2_) == 151 and r2_[0] == 3 and r2_[-1] == 697 and mid in r2_.tolist()
    c = add("two adjacent touched rows, then a long untouched stretch", [], [(5, 6)])
    assert (np.diff(c["g2"]["offsets"].astype(np.int64)) != deg).sum() == 2
    every = dl._und_edges(g)
    c = add("delete-all", [], every)
    assert len(c["map"]) == 0
    c = add("insert-into-empty", every[:, ::-1], [], base=c["g2"])
    assert len(c["map"]) == len(g["nbrs"]) and (c["map"] == NO).all()
    return _PLACES


def _check_map_call(eng, c):
    """apply_edges_map of the case on the context (which holds c["g"]): the counts, the map and the download against numpy"""
    before, after, view = eng.apply_edges_map(c["ins"], c["dele"])
    assert (before, after) == (len(c["g"]["nbrs"]), len(c["g2"]["nbrs"])) and eng.entries == after, c["name"]
    assert view.shape == (after,)
    got = eng.entry_map_to_host(view)
    assert got.dtype == np.uint32 and np.array_equal(got, c["map"]), c["name"]
    assert ap._same(c["g2"], *eng.download_csr()), c["name"]


def _load(eng, g):
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])


def _dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    t = torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _gather_np(src, m, after):
    out = np.zeros((src.shape[0], after), src.dtype)
    there = m != NO
    out[:, there] = src[:, m[there]]
    return out


def _check_carry(eng, c, rng, combos=((1, 8), (3, 8), (1, 4), (3, 4))):
    """carry_entries through the map the context holds for case c, for every (n_rows, elem_bytes): random words in src, a canary in
    dst; the result is numpy's gather with zeros at the inserts and src keeps its bytes"""
    before, after = len(c["g"]["nbrs"]), len(c["g2"]["nbrs"])
    for n_rows, eb in combos:
        dt = np.uint64 if eb == 8 else np.uint32
        src = rng.integers(1, 1 << (8 * eb), (n_rows, before), dtype=dt)
        t_src, t_dst = _dev(src), _dev(np.full((n_rows, after), CANARY64 if eb == 8 else CANARY32, dt))
        eng.carry_entries(t_src, t_dst, n_rows, elem_bytes=eb)
        eng.sync()
        assert np.array_equal(_host(t_dst, dt), _gather_np(src, c["map"], after)), (c["name"], n_rows, eb)
        assert _host(t_src, dt).tobytes() == src.tobytes(), (c["name"], n_rows, eb)


# ---- CPU: the host form ------------------------------------------------------------------------------------------------------

def test_host_entry_map_against_numpy(tmp_path_factory):
    """1. gnnpe_host_csr_entry_map on the 19 small graphs and H1 with the four batch kinds, delete-all and insert-into-empty: the
    map is numpy's; it ascends strictly off GNNPE_NO_ENTRY; its image is the old entries minus the directed entries of D;
    GNNPE_NO_ENTRY sits exactly at the directed entries of I; new_nbrs[j'] == old_nbrs[map[j']] wherever the map is defined.  The
    identity for a graph and itself; a null argument is GNNPE_ERR_ARG"""
    from gnnpe_amd import binding
    assert binding.ABI_VERSION == 20 and binding.NO_ENTRY == NO
    for c in _batch_cases(tmp_path_factory):
        g, g2 = c["g"], c["g2"]
        n = g["n"]
        m = binding.host_entry_map(g, g2)
        assert m.dtype == np.uint32 and np.array_equal(m, c["map"]), c["name"]
        there = m != NO
        kept = m[there].astype(np.int64)
        assert (np.diff(kept) > 0).all(), c["name"]
        k_old, k_new = re_._csr_keys(g)[1], re_._csr_keys(g2)[1]
        both = lambda e: np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]])
        d_keys, i_keys = both(c["del_set"]), both(c["ins_set"])
        assert np.array_equal(kept, np.nonzero(~np.isin(k_old, d_keys))[0]), c["name"]
        assert np.array_equal(np.nonzero(~there)[0], np.nonzero(np.isin(k_new, i_keys))[0]), c["name"]
        assert (~there).sum() == 2 * len(c["ins_set"]) and np.array_equal(g2["nbrs"][there], g["nbrs"][kept]), c["name"]
    g = _BATCHES[0]["g"]
    assert np.array_equal(binding.host_entry_map(g, g), np.arange(len(g["nbrs"]), dtype=np.uint32))
    u32p = C.POINTER(C.c_uint32)
    o, nb, out = g["offsets"].astype(np.uint32), g["nbrs"].astype(np.uint32), np.zeros(len(g["nbrs"]), np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    lib = binding.load()
    assert lib.gnnpe_host_csr_entry_map(g["n"], p(o), p(nb), p(o), p(nb), p(out)) == 0
    for k in range(5):
        args = [p(o), p(nb), p(o), p(nb), p(out)]
        args[k] = None
        assert lib.gnnpe_host_csr_entry_map(g["n"], *args) == ERR_ARG, k


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_map_on_the_batches(tmp_path_factory):
    """2. apply_edges_map on the 20 graphs, the six batches of each applied in a row on one context (lists with repeats and both
    orientations): n_entries_before / _after, the downloaded CSR (numpy's G' bit for bit) and the map (numpy's)"""
    from gnnpe_amd import binding
    cases = _batch_cases(tmp_path_factory)
    eng = binding.Engine(0)
    try:
        for k, c in enumerate(cases):
            if k % 6 == 0:
                _load(eng, c["g"])
            _check_map_call(eng, c)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_places(tmp_path_factory):
    """3. the places where the merge can go wrong, on a graph of 6 000 entries built for them, each against numpy as in test 2: the
    first two rows touched and nothing else (no stretch in front), the last two (none behind), an insert into the first row; a
    touched row that becomes empty; an empty row that receives its first entries; every row touched; a touched row and an
    untouched row that straddle the 2 048-entry tile boundaries of the streaming part, both ways round; a touched row of 150 entries
    (three chunks of a row wave) with inserts below, between and above its old entries and its first and last entry deleted; two
    adjacent touched rows and a long untouched stretch; delete-all (the map has no entries); insert-into-empty (all
    GNNPE_NO_ENTRY)"""
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    try:
        for c in _place_cases(tmp_path_factory):
            _load(eng, c["g"])
            _check_map_call(eng, c)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_empty_batch_gives_the_identity(tmp_path_factory):
    """3 (last place). the empty batch: the identity map, the same entry count before and after, the graph and the generation left
    alone -- a match cursor opened before it delivers its remaining pages, all of refine_sets' rows -- and a table carried through
    it is a copy"""
    from gnnpe_amd import binding, synth
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    qp, bm = h["q"]["triangle"], dl._label_bitmap(g, h["q"]["triangle"])
    eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
    try:
        count = eng.refine_sets(qp, bm, limit=ap.FULL)[0]
        cur = eng.open_match_cursor(qp, bm, 5000)
        rows = [cur.next()[0]]
        for args in ((), ([], [])):
            before, after, view, ms = eng.apply_edges_map(*args, timing=True)
            assert before == after == len(g["nbrs"]) == eng.entries and ms >= 0
            assert np.array_equal(eng.entry_map_to_host(view), np.arange(after, dtype=np.uint32))
        ident = dict(name="empty batch", g=g, g2=g, map=np.arange(len(g["nbrs"]), dtype=np.uint32))
        _check_carry(eng, ident, np.random.default_rng(5400), combos=((3, 8), (1, 4)))
        done = False
        while not done:
            page, done = cur.next()
            rows.append(page)
        cur.close()
        assert count > 5000 and len(sh._row_set(np.concatenate(rows))) == count == sum(len(r) for r in rows)
        assert ap._same(g, *eng.download_csr())
    finally:
        eng.close()


def _big_graph(n, m, seed):
    """m random undirected edges on n vertices as a compact CSR, with its ascending keys x * n + y; numpy sorts only"""
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, n, int(m * 1.02), dtype=np.int64), rng.integers(0, n, int(m * 1.02), dtype=np.int64)
    code = np.unique(np.minimum(x, y)[x != y] * n + np.maximum(x, y)[x != y])[:m]
    lo, hi = code // n, code % n
    keys = np.sort(np.concatenate([lo * n + hi, hi * n + lo]))
    return keys, code


def _csr_of_keys(keys, n):
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(keys // n, minlength=n), out=offs[1:])
    return offs.astype(np.uint32), (keys % n).astype(np.uint32)


@pytest.mark.gpu
def test_gpu_more_entries_than_one_pass_of_the_streaming_blocks():
    """4. a graph with more entries than the streaming blocks cover in one pass of their grid-stride loop: copy_blocks is at most
    8 per CU and a block takes 2 048 entries per step, so 8 * CUs * 2 048 entries plus a twentieth (4.4 million on 256 CUs).  A
    batch of 1 edge each way, then one of 1 000 on the result: the map and the downloaded CSR equal numpy's, worked out on the
    sorted keys directly"""
    import torch
    from gnnpe_amd import binding
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    entries = int(8 * cus * MERGE_TILE * 1.05)
    n, t0 = entries // 20, time.perf_counter()
    keys, code = _big_graph(n, entries // 2, 5500)
    if time.perf_counter() - t0 > 5.0:
        pytest.skip(f"building a graph of {entries} entries in numpy took {time.perf_counter() - t0:.1f} s: over this test's budget")
    assert len(keys) > 8 * cus * MERGE_TILE
    rng = np.random.default_rng(5501)
    offs, nbrs = _csr_of_keys(keys, n)
    eng = binding.Engine(0)
    try:
        eng.load_csr(offs, nbrs, np.zeros(n, np.uint32))
        for k in (1, 1000):
            dele = code[rng.choice(len(code), k, replace=False)]
            a, b = rng.integers(0, n, 2 * k + 8, dtype=np.int64), rng.integers(0, n, 2 * k + 8, dtype=np.int64)
            ins = np.unique(np.minimum(a, b)[a != b] * n + np.maximum(a, b)[a != b])
            ins = ins[~np.isin(ins, code)][:k]
            assert len(ins) == k
            both = lambda cds: np.concatenate([cds, (cds % n) * n + cds // n])
            new_keys = np.union1d(np.setdiff1d(keys, both(dele), assume_unique=True), both(ins))
            pos = np.searchsorted(keys, new_keys)
            want = np.where(keys[np.minimum(pos, len(keys) - 1)] == new_keys, pos, NO).astype(np.uint32)
            before, after, view = eng.apply_edges_map(np.stack([ins % n, ins // n], axis=1), np.stack([dele // n, dele % n], axis=1))
            assert (before, after) == (len(keys), len(new_keys)) and (want == NO).sum() == 2 * k
            assert np.array_equal(eng.entry_map_to_host(view), want), k
            o2, nb2 = _csr_of_keys(new_keys, n)
            got_o, got_nb = eng.download_csr()
            assert np.array_equal(got_o, o2) and np.array_equal(got_nb, nb2), k
            keys, code = new_keys, np.union1d(np.setdiff1d(code, dele, assume_unique=True), ins)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["batches", "places"])
def test_gpu_carry_entries(tmp_path_factory, which):
    """5. carry_entries with n_rows 1 and 3 and elem_bytes 8 and 4 over every case of test 2 (`batches`) and of test 3 (`places`):
    random non-zero words in src, a canary in dst so that an unwritten cell shows; dst is numpy's gather through numpy's map with
    zeros at the inserts, and src keeps its bytes"""
    from gnnpe_amd import binding
    cases = _batch_cases(tmp_path_factory) if which == "batches" else _place_cases(tmp_path_factory)
    rng = np.random.default_rng(5600)
    eng = binding.Engine(0)
    try:
        for c in cases:
            _load(eng, c["g"])
            before, after, view = eng.apply_edges_map(c["ins"], c["dele"])
            assert np.array_equal(eng.entry_map_to_host(view), c["map"]), c["name"]
            _check_carry(eng, c, rng)
    finally:
        eng.close()


def _raw_carry(eng, n_rows, eb, src, dst):
    rc = eng.lib.gnnpe_csr_carry_entries(eng.ctx, n_rows, eb, C.c_void_p(src) if src else None, C.c_void_p(dst) if dst else None, None)
    return rc, eng.lib.gnnpe_last_error().decode() if rc else ""


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory):
    """6. GNNPE_ERR_ARG with dst untouched and the context usable afterwards: carry before any map, after a plain apply_edges, after
    load_csr, after a refused apply_edges_map (an insertion that is already an edge: the download is still the old CSR and both
    entry counts are the old one); elem_bytes 3; dst overlapping src; a null dst; a stale map_view handed to entry_map_to_host.
    In the end a good batch and its carry go through"""
    from gnnpe_amd import binding
    g = sh._h1(tmp_path_factory)["g"]
    entries = len(g["nbrs"])
    rng = np.random.default_rng(5700)
    ins, dele = ap._random_batch(g, rng, 12, 12)
    edge = dl._und_edges(g)[100]
    src = rng.integers(1, 1 << 64, (2, entries + 64), dtype=np.uint64)
    t_src, t_dst = _dev(src), _dev(np.full((2, entries + 64), CANARY64, np.uint64))
    eng = binding.Engine(0)

    def refused(what, n_rows=2, eb=8, s=None, d=None):
        rc, text = _raw_carry(eng, n_rows, eb, t_src.data_ptr() if s is None else s, t_dst.data_ptr() if d is None else d)
        assert rc == ERR_ARG and text, (what, rc, text)
        eng.sync()
        assert (_host(t_dst, np.uint64) == CANARY64).all() and _host(t_src, np.uint64).tobytes() == src.tobytes(), what
        return text

    try:
        _load(eng, g)
        assert "no valid entry map" in refused("before any map")
        _, _, view0 = eng.apply_edges_map(ins, dele)
        g1 = ap._apply_np(g, ins, dele)
        assert entries == len(g1["nbrs"])
        assert "elem_bytes" in refused("elem_bytes 3", eb=3)
        assert "overlap" in refused("dst inside src", d=t_src.data_ptr() + 8 * entries)
        assert "overlap" in refused("src inside dst", s=t_dst.data_ptr() + 16)
        assert "null" in refused("null dst", d=0)
        eng.apply_edges(dele, ins)  # plain, and back to g
        assert "no valid entry map" in refused("after a plain apply_edges")
        with pytest.raises(binding.GnnpeError, match="stale entry-map view"):
            eng.entry_map_to_host(view0)
        _, _, view1 = eng.apply_edges_map(ins, dele)
        _load(eng, g)
        assert "no valid entry map" in refused("after load_csr")
        with pytest.raises(binding.GnnpeError, match="stale entry-map view"):
            eng.entry_map_to_host(view1)
        _, _, view2 = eng.apply_edges_map()
        u32p = C.POINTER(C.c_uint32)
        bad = np.ascontiguousarray(np.concatenate([ins, edge[None, ::-1]]), np.uint32)
        b, a, ptr = C.c_uint64(7), C.c_uint64(7), C.c_void_p(7)
        rc = eng.lib.gnnpe_csr_apply_edges_map(eng.ctx, bad.ctypes.data_as(u32p), len(bad), None, 0, C.byref(b), C.byref(a), C.byref(ptr), None)
        assert rc == ERR_ARG and "is already an edge" in eng.lib.gnnpe_last_error().decode()
        assert b.value == a.value == entries and not ptr.value and ap._same(g, *eng.download_csr())
        assert "no valid entry map" in refused("after a refused apply_edges_map")
        with pytest.raises(binding.GnnpeError, match="is already an edge"):
            eng.apply_edges_map(bad)
        with pytest.raises(binding.GnnpeError, match="stale entry-map view"):
            eng.entry_map_to_host(view2)
        assert eng.entries == entries
        c = _case("after the refusals", g, ins, dele, rng)
        _check_map_call(eng, c)
        _check_carry(eng, c, rng, combos=((2, 8),))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_state_of_a_fresh_load(tmp_path_factory):
    """7. after apply_edges_map (H1, 40 inserts and 40 deletes) the triangle's per-edge table and the wedge's per-vertex table are
    those of a fresh engine that loaded numpy's G', and rows_held agrees"""
    from gnnpe_amd import binding, synth
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    rng = np.random.default_rng(5800)
    ins, dele = ap._random_batch(g, rng, 40, 40)
    g2 = ap._apply_np(g, ins, dele)
    eng, fresh = (ex._engine(binding, x, synth.degree_order(x["offsets"]), 2) for x in (g, g2))
    try:
        eng.count_paths(2)  # derived state of the old graph, to be reset
        eng.apply_edges_map(ap._noisy(ins, rng), ap._noisy(dele, rng))
        assert eng.rows_held() == fresh.rows_held()
        bm = dl._label_bitmap(g2, h["q"]["triangle"])
        mine, theirs = (e.refine_sets_edge_counts(h["q"]["triangle"], bm) for e in (eng, fresh))
        assert mine[0] == theirs[0] > 0 and mine[1] and mine[2].shape == (3, len(g2["nbrs"])) and np.array_equal(mine[2], theirs[2])
        bm = dl._label_bitmap(g2, h["q"]["wedge"])
        mine, theirs = (e.refine_sets_vertex_counts(h["q"]["wedge"], bm) for e in (eng, fresh))
        assert mine[0] == theirs[0] > 0 and mine[1] and np.array_equal(mine[2], theirs[2])
        with pytest.raises(binding.GnnpeError):
            eng.count_paths(2)
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("distinct,induced", dl.MODES)
def test_gpu_edge_tables_maintained_on_the_device(tmp_path_factory, distinct, induced):
    """8. edge tables kept exact with no host in the loop: H1, a labels-only bitmap, three consecutive batches of 30 deletions and
    30 insertions (seeds 5900 ..).  The table of every shape is a device tensor from refine_sets_edge_counts(device=True) to the
    end.  Modes 0 and DISTINCT (wedge, triangle, diamond, C4), one step per batch: -ED(G, D), apply_edges_map(I, D), carry_entries,
    +ED(G', I).  INDUCED and INDUCED | DISTINCT (wedge and C4: a query needs a non-adjacent pair for EN to mean anything), two
    steps per batch: -ED(G, D), apply D, carry, +EN(G', D); then -EN(G', I), apply I, carry, +ED(G'', I).  After each batch every
    table, copied back, equals refine_sets_edge_counts of a fresh engine on numpy's graph in the same mode; at least four of the
    delta calls moved something"""
    import torch
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    names = ("wedge", "C4") if induced else ("wedge", "triangle", "diamond", "C4")
    bms = {name: dl._label_bitmap(g, h["q"][name]) for name in names}
    mode = dict(distinct=distinct)
    eng = ex._engine(binding, g, h["sn"], 2)
    moved = 0

    def ed(name, edges, sign):
        got = eng.refine_sets_delta_edge_counts(h["q"][name], bms[name], edges, induced=induced, accum=tab[name].data_ptr(), sign=sign, **mode)
        assert got[1]
        return got[0] > 0

    def en(name, pairs, sign):
        got = eng.refine_sets_delta_nonedges_edge_counts(h["q"][name], bms[name], pairs, accum=tab[name].data_ptr(), sign=sign, **mode)
        assert got[1]
        return got[0] > 0

    def apply_and_carry(ins, dele):
        before, after, _ = eng.apply_edges_map(ins, dele)
        for name in names:
            assert tab[name].shape[1] == before
            dst = torch.empty((tab[name].shape[0], after), dtype=torch.int64, device="cuda:0")
            eng.carry_entries(tab[name], dst, dst.shape[0])
            eng.sync()
            tab[name] = dst

    try:
        tab = {}
        for name in names:
            got = eng.refine_sets_edge_counts(h["q"][name], bms[name], induced=induced, device=True, **mode)
            assert got[1]
            tab[name] = torch.as_tensor(got[2], device="cuda:0").clone()
            torch.cuda.synchronize()
        for step in range(3):
            D, I = rdc._batch(g, 5900 + step)
            if induced:
                moved += sum(ed(name, D, -1) for name in names)
                apply_and_carry(None, D)
                moved += sum(en(name, D, 1) for name in names)
                moved += sum(en(name, I, -1) for name in names)
                apply_and_carry(I, None)
                moved += sum(ed(name, I, 1) for name in names)
            else:
                moved += sum(ed(name, D, -1) for name in names)
                apply_and_carry(I, D)
                moved += sum(ed(name, I, 1) for name in names)
            g = ap._apply_np(g, I, D)
            assert ap._same(g, *eng.download_csr()), step
            fresh = ex._engine(binding, g, h["sn"], 2)
            try:
                for name in names:
                    want = fresh.refine_sets_edge_counts(h["q"][name], bms[name], induced=induced, **mode)
                    assert want[1] and want[2].any()
                    assert np.array_equal(_host(tab[name], np.uint64), want[2]), (step, name)
            finally:
                fresh.close()
        assert moved >= 4, moved
    finally:
        eng.close()
