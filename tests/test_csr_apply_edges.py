"""Edge insert/delete batches applied to a CSR (include/gnnpe_hip.h, ABI version 16): gnnpe_host_csr_apply_edges on the host,
gnnpe_csr_apply_edges on the graph a context holds, gnnpe_csr_download, and `gnnpe_main --apply-edges`.

The yardstick for the graph is always numpy: synth._csr_from_edges on the edited edge set, never the library.  The host form is
held to it bit for bit and tied to ABI 15 by |M(G')| = |M(G)| - Delta(G, D) + Delta(G', I).  The device form is held to numpy through
the download, and to a FRESH engine that loaded G' for everything derived from the rows (hub list, reverse positions, neighbour
labels): "the state gnnpe_load_csr leaves" is checked as behaviour."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_online_exact as ex
import test_refine_delta as dl
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
MODES = dl.MODES
ERR_ARG, ERR_UNSUPPORTED = -1, -3
IDENTITY_SHAPES = ("wedge", "triangle", "C4")
COUNT_SHAPES = ("edge", "wedge", "triangle", "diamond", "K4")


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _codes(edges, n):
    return dl._codes(edges, n) if len(edges) else np.zeros(0, np.int64)


def _apply_np(g, ins, dele):
    """the numpy yardstick: the undirected edge set of g minus `dele` plus `ins`, as a fresh CSR with g's labels"""
    from gnnpe_amd import synth
    n = len(g["labels"])
    have = _codes(dl._und_edges(g), n)
    d, i = _codes(dele, n), _codes(ins, n)
    assert np.isin(d, have).all() and not np.isin(i, have).any() and not np.isin(i, d).any()
    keep = np.union1d(np.setdiff1d(have, d), i)
    offs, nbrs = synth._csr_from_edges(n, keep // n, keep % n)
    return dict(n=n, offsets=offs, nbrs=nbrs, labels=g["labels"])


def _same(g, offsets, nbrs):
    return (offsets.dtype == np.uint32 and nbrs.dtype == np.uint32 and np.array_equal(offsets, g["offsets"]) and
            np.array_equal(nbrs, g["nbrs"]))


def _non_edges(g, k, rng, avoid=()):
    """k different non-edges (x < y) of g, none of its codes in `avoid`, no endpoint in avoid's vertex set"""
    n = len(g["labels"])
    have = set(_codes(dl._und_edges(g), n).tolist())
    out = set()
    while len(out) < k:
        x, y = (int(v) for v in rng.integers(0, n, 2))
        if x != y and min(x, y) * n + max(x, y) not in have and x not in avoid and y not in avoid:
            out.add((min(x, y), max(x, y)))
    return np.array(sorted(out), np.int64).reshape(-1, 2)


def _random_batch(g, rng, n_ins, n_del, avoid=()):
    e = dl._und_edges(g)
    if len(avoid):
        e = e[~np.isin(e[:, 0], list(avoid)) & ~np.isin(e[:, 1], list(avoid))]
    dele = e[rng.choice(len(e), min(n_del, len(e)), replace=False)] if n_del and len(e) else np.zeros((0, 2), np.int64)
    return _non_edges(g, n_ins, rng, avoid), dele


def _noisy(edges, rng):
    """the same set with repeats, both orientations, shuffled"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if not len(e):
        return e
    e = np.concatenate([e, e[::2, ::-1], e[:3]])
    return e[rng.permutation(len(e))]


def _small_graphs():
    from gnnpe_amd import synth
    out = []
    for k in range(19):
        n = 40 + (k * 37) % 261
        g = synth.gnm_graph(n, n + (k * 53) % (2 * n), n_labels=1 + k % 3, seed=3100 + k)
        out.append(dict(n=n, offsets=g["offsets"], nbrs=g["nbrs"], labels=g["labels"]))
    return out


def _raw_host(binding, g, ins, dele, cap=None, canary=0xABCD1234):
    """gnnpe_host_csr_apply_edges through ctypes: (rc, *n_entries_after, out_offsets, out_nbrs); the outputs start as canaries"""
    u32p = C.POINTER(C.c_uint32)
    o, nb = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs"))
    i, d = (np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1, 2), np.uint32) for x in (ins, dele))
    cap = len(nb) + 2 * len(i) if cap is None else cap
    oo, on, after = np.full(len(o), canary, np.uint32), np.full(max(cap, 1), canary, np.uint32), C.c_uint64(777)
    rc = binding.load().gnnpe_host_csr_apply_edges(len(o) - 1, o.ctypes.data_as(u32p), nb.ctypes.data_as(u32p), i.ctypes.data_as(u32p), len(i),
                                                   d.ctypes.data_as(u32p), len(d), oo.ctypes.data_as(u32p), on.ctypes.data_as(u32p), cap,
                                                   C.byref(after))
    return rc, after.value, oo, on


def _raw_device(eng, ins, dele):
    """gnnpe_csr_apply_edges through ctypes: (rc, message)"""
    u32p = C.POINTER(C.c_uint32)
    i, d = (np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1, 2), np.uint32) for x in (ins, dele))
    after = C.c_uint64()
    rc = eng.lib.gnnpe_csr_apply_edges(eng.ctx, i.ctypes.data_as(u32p) if len(i) else None, len(i), d.ctypes.data_as(u32p) if len(d) else None,
                                       len(d), C.byref(after), None)
    return rc, eng.lib.gnnpe_last_error().decode() if rc else ""


# ---- CPU: the host form ------------------------------------------------------------------------------------------------------

def test_host_form_against_numpy(tmp_path_factory):
    """1. 19 seeded G(n, m) of 40 to 300 vertices and H1, four batches each -- random non-edge inserts and random existing deletes
    handed over with repeats and both orientations, insert-only, delete-only, and both on one graph in a row -- then delete-all and
    insert-into-empty: offsets and neighbours equal numpy's bit for bit"""
    from gnnpe_amd import binding
    graphs = _small_graphs() + [sh._h1(tmp_path_factory)["g"]]
    assert len(graphs) == 20
    for gi, g0 in enumerate(graphs):
        rng = np.random.default_rng(3200 + gi)
        g = g0
        for ni, nd in ((7, 5), (9, 0), (0, 6), (len(g0["nbrs"]) // 8, len(g0["nbrs"]) // 8)):
            ins, dele = _random_batch(g, rng, ni, nd)
            want = _apply_np(g, ins, dele)
            got = binding.host_apply_edges(g, _noisy(ins, rng), _noisy(dele, rng))
            assert _same(want, got["offsets"], got["nbrs"]), (gi, ni, nd)
            assert np.array_equal(got["labels"], g["labels"])
            g = want  # the next batch edits the edited graph
        every = dl._und_edges(g)
        empty = binding.host_apply_edges(g, None, every)
        assert len(empty["nbrs"]) == 0 and not empty["offsets"].any() and len(empty["offsets"]) == g["n"] + 1
        back = binding.host_apply_edges(empty, every[:, ::-1], None)
        assert _same(g, back["offsets"], back["nbrs"]), gi
        same = binding.host_apply_edges(g)
        assert _same(g, same["offsets"], same["nbrs"])


def test_host_refusals(tmp_path_factory):
    """2. a self-pair, id == n, an insertion that is an edge, a deletion that is none, one edge in both lists with opposite
    orientations: GNNPE_ERR_ARG, a message that names the pair, outputs untouched.  out_cap one too small: GNNPE_ERR_ARG with
    *n_entries_after set and the outputs untouched"""
    from gnnpe_amd import binding
    g = sh._h1(tmp_path_factory)["g"]
    n = g["n"]
    rng = np.random.default_rng(3300)
    ins, dele = _random_batch(g, rng, 6, 6)
    e = dl._und_edges(g)
    other = e[~np.isin(_codes(e, n), _codes(dele, n))]
    x, y = (int(v) for v in other[0])
    a, b = (int(v) for v in _non_edges(g, 1, rng, avoid=set(ins.ravel().tolist()))[0])
    lib = binding.load()
    rc, after, oo, on = _raw_host(binding, g, ins, dele)
    assert rc == 0 and after == len(g["nbrs"]) and _same(_apply_np(g, ins, dele), oo, on[:after])
    for bad_i, bad_d, msg in (([(5, 5)], [], "(5, 5) is a loop"), ([], [(9, 9)], "(9, 9) is a loop"), ([(3, n)], [], f"(3, {n})"),
                              ([], [(n, 3)], f"({n}, 3)"), ([(y, x)], [], f"({x}, {y}) is already an edge"),
                              ([], [(b, a)], f"({a}, {b}) is not an edge"), ([(a, b)], [(b, a)], f"({a}, {b}) is in both lists"),
                              ([(y, x)], [(x, y)], f"({x}, {y}) is in both lists")):
        rc, after, oo, on = _raw_host(binding, g, ins.tolist() + bad_i, dele.tolist() + bad_d)
        assert rc == ERR_ARG and msg in lib.gnnpe_last_error().decode(), (bad_i, bad_d, lib.gnnpe_last_error())
        assert (oo == 0xABCD1234).all() and (on == 0xABCD1234).all() and after == 0
        with pytest.raises(binding.GnnpeError):
            binding.host_apply_edges(g, ins.tolist() + bad_i, dele.tolist() + bad_d)
    grow = _non_edges(g, 4, rng)
    rc, after, oo, on = _raw_host(binding, g, grow, [], cap=len(g["nbrs"]) + 7)
    assert rc == ERR_ARG and after == len(g["nbrs"]) + 8 and (oo == 0xABCD1234).all() and (on == 0xABCD1234).all()
    rc, after, oo, on = _raw_host(binding, g, grow, [], cap=len(g["nbrs"]) + 8)
    assert rc == 0 and after == len(g["nbrs"]) + 8


def test_host_round_trip(tmp_path_factory):
    """3. (I, D) and then (D, I) restores the original arrays: the 19 small graphs and H1"""
    from gnnpe_amd import binding
    for gi, g in enumerate(_small_graphs() + [sh._h1(tmp_path_factory)["g"]]):
        ins, dele = _random_batch(g, np.random.default_rng(3400 + gi), 11, 9)
        there = binding.host_apply_edges(g, ins, dele)
        assert not _same(g, there["offsets"], there["nbrs"])
        back = binding.host_apply_edges(there, dele, ins)
        assert _same(g, back["offsets"], back["nbrs"]), gi


def test_host_identity_with_the_delta_call(tmp_path_factory):
    """4. the tie to ABI 15, host forms only: wedge, triangle and C4 with the labels-only bitmap, modes 0 and DISTINCT,
    |M(G')| = |M(G)| - Delta(G, D) + Delta(G', I), on H1 (60 inserts, 60 deletes, seed 3500) and six of the small graphs"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    moved = 0
    # (the H1 query files are all label 0: the small graphs take one label too)
    small = [dict(g, labels=np.zeros(g["n"], np.uint32)) for g in _small_graphs()[:6]]
    for gi, (g, k) in enumerate([(h["g"], 60)] + [(g, 8) for g in small]):
        ins, dele = _random_batch(g, np.random.default_rng(3500 + gi), k, k)
        g2 = binding.host_apply_edges(g, ins, dele)
        for name in IDENTITY_SHAPES:
            qp = h["q"][name]
            bm = dl._label_bitmap(g, qp)
            for distinct in (False, True):
                before = binding.host_refine_sets(g, qp, bm, FULL, distinct=distinct)
                after = binding.host_refine_sets(g2, qp, bm, FULL, distinct=distinct)
                gone = binding.host_refine_sets_delta(g, qp, bm, dele, FULL, distinct=distinct)
                new = binding.host_refine_sets_delta(g2, qp, bm, ins, FULL, distinct=distinct)
                assert after == before - gone + new, (gi, name, distinct, before, gone, new, after)
                moved += gone > 0 and new > 0
    assert moved >= 6


def test_cli_apply_edges_outside_exact_mode(tmp_path):
    """11b. --apply-edges without --exact / -l 3, with -m offline and with gnnpge_main exits non-zero with its message before a
    GPU is touched"""
    from conftest import GOLDEN
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(rs.ONLINE, "q2.graph")
    ef = str(tmp_path / "batch.txt")
    open(ef, "w").write("+ 0 1\n")
    for tool, mode, msg in ((CLI, ["-m", "online"], "--apply-edges applies to exact"), (CLI, ["-m", "filter"], "--apply-edges applies to exact"),
                            (CLI, ["-m", "offline"], "--apply-edges applies to exact"),
                            (os.path.join(os.path.dirname(CLI), "gnnpge_main"), ["-m", "online"], "--apply-edges is an option of gnnpe_main")):
        r = subprocess.run([tool, "-f", root, "-d", graph, "-q", q, "-p", "2", "--apply-edges", ef] + mode, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (tool, mode, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

_BATTERY = {}


def _h1_battery(tmp_path_factory):
    """H1 with ONE batch that holds every shape of row edit, each part asserted to exist (the docstring of
    test_gpu_shape_battery_on_h1 lists them); computed once.  Target rows are reserved: no other part touches them"""
    if _BATTERY:
        return _BATTERY
    h = sh._h1(tmp_path_factory)
    g, deg, n = h["g"], h["deg"], h["g"]["n"]
    o = g["offsets"].astype(np.int64)
    rng = np.random.default_rng(3600)
    row = lambda v: g["nbrs"][o[v]:o[v + 1]].astype(np.int64)

    def pick(mask, what):
        """the first vertex of the mask that is not 0, n - 1, reserved, or adjacent to a reserved vertex"""
        for v in np.nonzero(mask)[0].tolist():
            if v in (0, n - 1) or v in reserved or any(w in reserved for w in row(v).tolist()):
                continue
            return v
        raise AssertionError("H1 has no " + what)

    reserved = set()
    parts = {}
    first = np.array([row(v)[0] if deg[v] else 0 for v in range(n)])
    last = np.array([row(v)[-1] if deg[v] else n for v in range(n)])
    for name, mask in (("cut", deg > 64), ("hub_both", deg > 64), ("grow", (deg >= 20) & (deg <= 64)), ("flood", (deg >= 1) & (deg <= 8)),
                       ("leaf", deg == 1), ("emptied", (deg >= 3) & (deg <= 12)), ("isolated", deg == 0),
                       ("ends", (deg >= 4) & (deg <= 64) & (first > 20) & (last < n - 20)), ("small_both", (deg >= 5) & (deg <= 64))):
        v = pick(mask, name)
        parts[name] = v
        reserved.add(v)
    ends = parts["ends"]
    used = set()
    ins, dele = [], []

    def add_inserts(v, k, lo=0, hi=n):
        """k partners in [lo, hi): unreserved, not 0 / n - 1, non-adjacent to v, pair unused"""
        mine = set(row(v).tolist())
        pool = [w for w in rng.permutation(np.arange(lo, hi)).tolist()
                if w != v and w not in reserved and w not in (0, n - 1) and w not in mine and (min(v, w), max(v, w)) not in used]
        assert len(pool) >= k
        for w in pool[:k]:
            used.add((min(v, w), max(v, w)))
            ins.append((v, w))

    def add_deletes(v, k):
        pool = [w for w in row(v).tolist() if w not in reserved and (min(v, w), max(v, w)) not in used]
        assert len(pool) >= k
        for w in pool[:k]:
            used.add((min(v, w), max(v, w)))
            dele.append((w, v))

    add_inserts(parts["grow"], 65 - int(deg[parts["grow"]]))  # <= 64 -> exactly 65: becomes a hub row
    add_deletes(parts["cut"], int(deg[parts["cut"]]) - 64)  # a hub row -> exactly 64: leaves the hub list
    add_inserts(parts["flood"], 70)  # more inserts than one 64-entry chunk into a short row
    add_deletes(parts["leaf"], 1)  # a leaf's only edge
    add_deletes(parts["emptied"], int(deg[parts["emptied"]]))  # a row of degree >= 3 emptied
    add_inserts(parts["isolated"], 2)  # an empty row receives two
    add_inserts(ends, 1, 1, int(row(ends)[0]))  # below the first entry
    add_inserts(ends, 1, int(row(ends)[-1]) + 1, n - 1)  # above the last
    for v in (parts["hub_both"], parts["small_both"]):  # insert and delete in one row
        add_inserts(v, 2)
        add_deletes(v, 2)
    assert (0, n - 1) not in used and n - 1 not in row(0).tolist()
    ins.append((n - 1, 0))  # vertex 0 and vertex n - 1, each other's last / first entry
    used.add((0, n - 1))
    block = reserved | {0, n - 1}
    e = dl._und_edges(g)
    e = e[~np.isin(e[:, 0], list(block)) & ~np.isin(e[:, 1], list(block))]
    e = e[np.array([tuple(p) not in used for p in e.tolist()])]
    rnd_del = e[rng.choice(len(e), 50, replace=False)]
    rnd_ins = [p for p in _non_edges(g, 80, rng, avoid=block).tolist() if tuple(p) not in used][:50]
    assert len(rnd_ins) == 50
    ins_set = np.array(ins + rnd_ins, np.int64)
    del_set = np.concatenate([np.array(dele, np.int64), rnd_del])
    g2 = _apply_np(g, ins_set, del_set)
    deg2 = np.diff(g2["offsets"].astype(np.int64))
    assert deg2[parts["grow"]] == 65 and deg2[parts["cut"]] == 64 and deg2[parts["flood"]] == deg[parts["flood"]] + 70
    assert deg2[parts["leaf"]] == 0 and deg2[parts["emptied"]] == 0 and deg2[parts["isolated"]] == 2
    assert deg2[ends] == deg[ends] + 2 and deg2[parts["hub_both"]] == deg[parts["hub_both"]] > 64
    assert g2["nbrs"][g2["offsets"][1] - 1] == n - 1 and g2["nbrs"][g2["offsets"][n - 1]] == 0
    every = dl._und_edges(g)
    stays = every[~np.isin(_codes(every, n), _codes(del_set, n))][-1:]
    _BATTERY.update(g=g, g2=g2, stays=stays, ins=_noisy(ins_set, rng), dele=_noisy(del_set, rng), ins_set=ins_set, del_set=del_set, parts=parts,
                    hubs=(int((deg > 64).sum()), int((deg2 > 64).sum())))
    return _BATTERY


def _fresh(binding, g):
    from gnnpe_amd import synth
    return ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)


@pytest.mark.gpu
def test_gpu_shape_battery_on_h1(tmp_path_factory):
    """5. H1, one batch (repeats and both orientations in both lists): a row of degree <= 64 grown to exactly 65 and a hub row cut to
    exactly 64 (both crossings of the hub threshold); a row of degree <= 8 that receives 70 insertions; a leaf's only edge deleted
    and a row of degree >= 3 emptied; an isolated vertex that receives two edges; an insert below a row's first entry and one above
    its last; an insert and a delete in one row, for a hub row and a short one; vertex 0 and vertex n - 1 joined; 50 random deletes
    and 50 random non-edge inserts.  The same batch with an edge that stays among the insertions is refused first and leaves the
    download as it was; a cursor opened before the batch goes on after the refusal and is refused after the batch.  Then the
    download is numpy's CSR bit for bit; rows_held is a fresh engine's; the counts of
    edge, wedge, triangle, diamond and K4 in the four modes on the labels-only bitmap are the fresh engine's and the host form's on
    the host-updated CSR; the triangle's per-edge table (reverse positions, entry layout) and the wedge's per-vertex table are the
    fresh engine's"""
    from gnnpe_amd import binding
    h, b = sh._h1(tmp_path_factory), _h1_battery(tmp_path_factory)
    g, g2 = b["g"], b["g2"]
    host = binding.host_apply_edges(g, b["ins"], b["dele"])
    assert _same(g2, host["offsets"], host["nbrs"])
    eng, fresh = _fresh(binding, g), _fresh(binding, g2)
    try:
        assert eng.rows_held() == (g["n"], len(g["nbrs"]), b["hubs"][0])
        cur = eng.open_match_cursor(h["q"]["triangle"], dl._label_bitmap(g, h["q"]["triangle"]), 1000)
        assert len(cur.next()[0]) == 1000
        with pytest.raises(binding.GnnpeError, match="is already an edge"):
            eng.apply_edges(np.concatenate([b["ins"], b["stays"]]), b["dele"])
        assert _same(g, *eng.download_csr()) and eng.entries == len(g["nbrs"]) and len(cur.next()[0]) == 1000
        entries, ms = eng.apply_edges(b["ins"], b["dele"], timing=True)
        assert entries == len(g2["nbrs"]) == eng.entries and ms > 0
        with pytest.raises(binding.GnnpeError, match=r"^\[-1\]"):
            cur.next()
        cur.close()
        assert _same(g2, *eng.download_csr())
        assert eng.rows_held() == fresh.rows_held() == (g["n"], len(g2["nbrs"]), b["hubs"][1])
        for name in COUNT_SHAPES:
            qp = h["q"][name]
            bm = dl._label_bitmap(g2, qp)
            for distinct, induced in MODES:
                got = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                assert got == fresh.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0], (name, distinct, induced)
                assert got == binding.host_refine_sets(host, qp, bm, FULL, distinct=distinct, induced=induced), (name, distinct, induced)
        bm = dl._label_bitmap(g2, h["q"]["triangle"])
        mine, theirs = (e.refine_sets_edge_counts(h["q"]["triangle"], bm) for e in (eng, fresh))
        assert mine[0] == theirs[0] > 0 and mine[1] and mine[2].shape == (3, len(g2["nbrs"])) and np.array_equal(mine[2], theirs[2])
        bm = dl._label_bitmap(g2, h["q"]["wedge"])
        mine, theirs = (e.refine_sets_vertex_counts(h["q"]["wedge"], bm) for e in (eng, fresh))
        assert mine[0] == theirs[0] > 0 and mine[1] and np.array_equal(mine[2], theirs[2])
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_gpu_extremes(tmp_path_factory):
    """6. every edge deleted: the edge query counts 0 and the download's offsets are all zero; all inserted back: the download is
    the original; the empty batch: nothing changes and an open cursor keeps delivering; a batch that more than doubles the entries
    (the buffers grow), and back"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    every = dl._und_edges(g)
    qp, bm = h["q"]["edge"], dl._label_bitmap(g, h["q"]["edge"])
    eng = _fresh(binding, g)
    try:
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == len(g["nbrs"])
        assert eng.apply_edges(None, every) == 0
        offs, nbrs = eng.download_csr()
        assert len(offs) == g["n"] + 1 and not offs.any() and len(nbrs) == 0
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == 0 and eng.rows_held() == (g["n"], 0, 0)
        assert eng.apply_edges(every[:, ::-1], None) == len(g["nbrs"])
        assert _same(g, *eng.download_csr())
        bm_t = dl._label_bitmap(g, h["q"]["triangle"])
        count = eng.refine_sets(h["q"]["triangle"], bm_t, limit=FULL)[0]
        cur = eng.open_match_cursor(h["q"]["triangle"], bm_t, 5000)
        rows = [cur.next()[0]]
        assert eng.apply_edges() == len(g["nbrs"]) and eng.apply_edges([], []) == len(g["nbrs"])
        done = False
        while not done:
            page, done = cur.next()
            rows.append(page)
        cur.close()
        assert count > 5000 and len(sh._row_set(np.concatenate(rows))) == count == sum(len(r) for r in rows)
        many = _non_edges(g, len(g["nbrs"]) // 2 + 500, np.random.default_rng(3700))
        g2 = _apply_np(g, many, [])
        assert len(g2["nbrs"]) > 2 * len(g["nbrs"])
        assert eng.apply_edges(many) == len(g2["nbrs"]) and _same(g2, *eng.download_csr())
        assert eng.refine_sets(qp, bm, limit=FULL)[0] == len(g2["nbrs"])
        assert eng.apply_edges(None, many) == len(g["nbrs"]) and _same(g, *eng.download_csr())
        assert eng.refine_sets(h["q"]["triangle"], bm_t, limit=FULL)[0] == count
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_six_batches_on_one_context(tmp_path_factory):
    """7. six consecutive seeded batches on one context (H1; 40 + 40, insert-only, delete-only, 300 + 10, 10 + 300, 1 + 1), so
    that each spare buffer is reused at least twice: after each the download equals numpy, and the identity of test 4 holds with
    the device forms -- refine_sets_delta over D before the apply, over I after it, refine_sets for the totals -- for wedge,
    triangle and C4 in modes 0 and DISTINCT"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    bms = {name: dl._label_bitmap(g, h["q"][name]) for name in IDENTITY_SHAPES}
    keys = [(name, d) for name in IDENTITY_SHAPES for d in (False, True)]
    rng = np.random.default_rng(3800)
    eng = _fresh(binding, g)
    try:
        total = {k: eng.refine_sets(h["q"][k[0]], bms[k[0]], limit=FULL, distinct=k[1])[0] for k in keys}
        for step, (ni, nd) in enumerate(((40, 40), (25, 0), (0, 25), (300, 10), (10, 300), (1, 1))):
            ins, dele = _random_batch(g, rng, ni, nd)
            gone = {k: eng.refine_sets_delta(h["q"][k[0]], bms[k[0]], dele, distinct=k[1])[0] for k in keys}
            g = _apply_np(g, ins, dele)
            assert eng.apply_edges(_noisy(ins, rng), _noisy(dele, rng)) == len(g["nbrs"])
            assert _same(g, *eng.download_csr()), step
            for k in keys:
                new = eng.refine_sets_delta(h["q"][k[0]], bms[k[0]], ins, distinct=k[1])[0]
                after = eng.refine_sets(h["q"][k[0]], bms[k[0]], limit=FULL, distinct=k[1])[0]
                assert after == total[k] - gone[k] + new, (step, k, total[k], gone[k], new, after)
                total[k] = after
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory):
    """8. an insertion that is an edge, a deletion that is none, one edge in both lists (found on the device), a self-pair, id == n
    (found on the host), each among valid pairs: GNNPE_ERR_ARG, the message names the pair, the download is unchanged, and a cursor
    opened before the calls delivers its remaining pages, which together are refine_sets' rows; the derived state is kept: the
    order, the label table and the embeddings set before the refusals still serve count_paths and fill_paths, with the results of
    before.  Then a valid batch succeeds, and there the derived state is reset: count_paths is refused until the order is set again.
    The multigraph state and a context filled by load_rows: GNNPE_ERR_UNSUPPORTED"""
    from gnnpe_amd import binding, synth
    h = sh._h1(tmp_path_factory)
    g, n = h["g"], h["g"]["n"]
    rng = np.random.default_rng(3900)
    ins, dele = _random_batch(g, rng, 20, 20)
    e = dl._und_edges(g)
    x, y = (int(v) for v in e[~np.isin(_codes(e, n), _codes(dele, n))][5])
    a, b = (int(v) for v in _non_edges(g, 1, rng, avoid=set(ins.ravel().tolist()))[0])
    qp = h["q"]["triangle"]
    bm = dl._label_bitmap(g, qp)
    eng = _fresh(binding, g)
    try:
        paths = eng.count_paths(2)  # (_fresh set the order and the table and computed the embeddings)
        ids0, pde0, _ = eng.fill_paths()
        assert paths == synth.expected_paths_l2(g["offsets"]) == len(ids0)
        count, _, full = eng.refine_sets(qp, bm, limit=FULL, matches_cap=1 << 16)
        assert 5000 < count == len(full)
        cur = eng.open_match_cursor(qp, bm, 3000)
        rows = [cur.next()[0]]
        for bad_i, bad_d, msg in (([(y, x)], [], f"({x}, {y}) is already an edge"), ([], [(b, a)], f"({a}, {b}) is not an edge"),
                                  ([(a, b)], [(b, a)], f"({a}, {b}) is in both lists"), ([(y, x)], [(x, y)], f"({x}, {y}) is in both lists"),
                                  ([(6, 6)], [], "(6, 6) is a loop"), ([], [(n, 2)], f"({n}, 2)")):
            rc, text = _raw_device(eng, ins.tolist() + bad_i, dele.tolist() + bad_d)
            assert rc == ERR_ARG and msg in text, (bad_i, bad_d, rc, text)
            assert _same(g, *eng.download_csr()) and eng.rows_held()[1] == len(g["nbrs"])
            page, done = cur.next()
            assert len(page) and not done
            rows.append(page)
        done = False
        while not done:
            page, done = cur.next()
            rows.append(page)
        cur.close()
        assert sh._row_set(np.concatenate(rows)) == sh._row_set(full) and sum(len(r) for r in rows) == count
        ids1, pde1, _ = eng.fill_paths()  # the count of before the refusals is still there
        assert np.array_equal(ids1, ids0) and np.array_equal(pde1, pde0)
        assert eng.count_paths(2) == paths  # ... and so are the order and the embeddings: no set_order, no vde in between
        g2 = _apply_np(g, ins, dele)
        assert eng.apply_edges(ins, dele) == len(g2["nbrs"]) and _same(g2, *eng.download_csr())
        with pytest.raises(binding.GnnpeError):
            eng.count_paths(2)
        eng.set_multigraph_rows(g2["offsets"].astype(np.uint64), g2["nbrs"])
        rc, text = _raw_device(eng, dele, [])
        assert rc == ERR_UNSUPPORTED and "simple graphs only" in text
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.download_csr()
    finally:
        eng.close()
    part = binding.Engine(0)
    try:
        rc, text = _raw_device(part, ins, dele)
        assert rc == ERR_UNSUPPORTED and "gnnpe_load_csr" in text
        rows_ = np.arange(0, n, 2, dtype=np.uint32)
        o = g["offsets"].astype(np.int64)
        lens = (o[rows_ + 1] - o[rows_])
        part.load_rows(n, g["labels"], rows_, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
                       np.concatenate([g["nbrs"][o[v]:o[v + 1]] for v in rows_.tolist()]).astype(np.uint32))
        rc, text = _raw_device(part, ins, dele)
        assert rc == ERR_UNSUPPORTED and "gnnpe_load_csr" in text
    finally:
        part.close()


@pytest.mark.gpu
def test_gpu_cursor_lifetime(tmp_path_factory):
    """9. a cursor opened before a successful apply: next() is refused with GNNPE_ERR_ARG and close() works; a cursor opened after
    the apply lists exactly the matches of the new graph"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    ins, dele = _random_batch(g, np.random.default_rng(4000), 30, 30)
    g2 = _apply_np(g, ins, dele)
    qp = h["q"]["triangle"]
    bm = dl._label_bitmap(g, qp)
    eng = _fresh(binding, g)
    try:
        cur = eng.open_match_cursor(qp, bm, 1000)
        assert len(cur.next()[0]) == 1000
        eng.apply_edges(ins, dele)
        with pytest.raises(binding.GnnpeError, match=r"^\[-1\]"):
            cur.next()
        cur.close()
        want = binding.host_refine_sets(g2, qp, bm, FULL)
        pages = list(eng.match_pages(qp, bm, 4096))
        rows = np.concatenate(pages)
        assert len(rows) == want == len(sh._row_set(rows)) and want != binding.host_refine_sets(g, qp, bm, FULL)
        o2 = g2["offsets"].astype(np.int64)
        adj = set((np.repeat(np.arange(g["n"]), np.diff(o2)) * g["n"] + g2["nbrs"]).tolist())
        r = rows.astype(np.int64)
        assert all(set((r[:, p] * g["n"] + r[:, q]).tolist()) <= adj for p, q in ((0, 1), (0, 2), (1, 2)))
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_offline_path_after_an_apply(tmp_path_factory):
    """10. set_order, set_label_table, vde and count_paths(l = 2) on the updated context: the count is
    synth.expected_paths_l2(offsets') and x / nx / vde are bitwise a fresh engine's on G' (neighbour labels, hub list).  The graph
    is H1's battery with four labels"""
    from gnnpe_amd import binding, synth
    b = _h1_battery(tmp_path_factory)
    labels = (np.arange(b["g"]["n"]) % 4).astype(np.uint32)
    g, g2 = dict(b["g"], labels=labels), dict(b["g2"], labels=labels)
    sn2 = synth.degree_order(g2["offsets"])
    eng, fresh = _fresh(binding, g), binding.Engine(0)
    try:
        eng.count_paths(2)  # derived state of the old graph, to be reset
        eng.apply_edges(b["ins"], b["dele"])
        fresh.load_csr(g2["offsets"], g2["nbrs"], g2["labels"])
        got = []
        for e in (eng, fresh):
            e.set_order(sn2, np.zeros(g["n"], np.uint32), 1)
            e.set_label_table(binding.host_label_table(4, 2))
            got.append(e.vde())
            assert e.count_paths(2) == synth.expected_paths_l2(g2["offsets"])
        for mine, theirs in zip(*got):
            assert np.array_equal(mine, theirs)
        assert not np.array_equal(got[0][2], _fresh_vde(binding, g))
    finally:
        eng.close()
        fresh.close()


def _fresh_vde(binding, g):
    eng = _fresh(binding, g)
    try:
        return eng.vde()[2]
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cli_apply_edges(tmp_path, test_graph):
    """11. gnnpe_main -m online --exact --refine sets --apply-edges F on the golden test graph prints the answer line that the same
    command without the flag prints on the graph file of G' (synth.write_graph_file), after the same metadata block and plan size
    (they describe G', not the file): q1 and q2, plain and --distinct; the batch (30 random inserts, 12 random deletes and the
    deletion of six edges that carry a match of q1, so G' has more entries than G; seed 4100) changes the answer of at least one of
    them.  With --edge-counts and with --vertex-counts the file written is byte for byte the one of the run on G''s graph file --
    the tables are indexed by the entries of the CSR the context holds after the batch -- and not the one of the run on G"""
    from conftest import GOLDEN
    from gnnpe_amd import binding, synth
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    g = dict(n=len(test_graph["labels"]), offsets=test_graph["offsets"], nbrs=test_graph["nbrs"], labels=test_graph["labels"])
    rng = np.random.default_rng(4100)
    ins, dele = _random_batch(g, rng, 30, 12)
    q1 = os.path.join(rs.ONLINE, "q1.graph")
    used = np.nonzero(binding.host_refine_sets_edge_counts(g, q1, ex._ld_bitmap(g, q1))[2].sum(axis=0))[0]
    used = used[rng.choice(len(used), 6, replace=False)]
    src = np.repeat(np.arange(g["n"], dtype=np.int64), np.diff(g["offsets"].astype(np.int64)))
    carry = np.stack([src[used], g["nbrs"][used].astype(np.int64)], axis=1)
    carry.sort(axis=1)
    dele = np.unique(np.concatenate([dele, carry]), axis=0)
    g2 = _apply_np(g, ins, dele)
    assert len(g2["nbrs"]) > len(g["nbrs"])
    e2 = dl._und_edges(g2)
    graph2 = str(tmp_path / "updated.graph")
    synth.write_graph_file(graph2, dict(g2, m=len(e2), eu=e2[:, 0], ev=e2[:, 1]))
    # (the processing order of the dataset directory is the old graph's: any order gives the same candidate sets)
    ef = str(tmp_path / "batch.txt")
    open(ef, "w").write("".join(f"+ {x} {y}\n" for x, y in ins.tolist()) + "".join(f"- {y} {x}\n" for x, y in dele.tolist()))
    changed = 0
    for q in ("q1", "q2"):
        qp = os.path.join(rs.ONLINE, f"{q}.graph")
        for extra in ([], ["--distinct"]):
            answers, heads = [], []
            for data, flag in ((graph, ["--apply-edges", ef]), (graph2, []), (graph, [])):
                r = subprocess.run([CLI, "-f", root, "-d", data, "-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets"] + flag + extra,
                                   capture_output=True, text=True, timeout=300)
                assert r.returncode == 0, r.stderr
                lines = r.stdout.splitlines()
                answers.append(int(next(ln for ln in lines if ln.startswith("Answer Number: ")).split()[2]))
                heads.append(lines[:3])  # |V|, |E|, labels; max degree, max label frequency; the plan size
            assert answers[0] == answers[1], (q, extra, answers)
            assert heads[0] == heads[1] != heads[2] and f"|E|: {len(e2)}," in heads[0][0], heads
            changed += answers[0] != answers[2]
    assert changed >= 1
    for table in ("--edge-counts", "--vertex-counts"):
        files = []
        for k, (data, flag) in enumerate(((graph, ["--apply-edges", ef]), (graph2, []), (graph, []))):
            out = str(tmp_path / f"{table[2:]}_{k}.txt")
            r = subprocess.run([CLI, "-f", root, "-d", data, "-q", q1, "-p", "2", "-m", "online", "--exact", "--refine", "sets", table, out] + flag,
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            files.append(open(out, "rb").read())
        assert files[0] == files[1] != files[2] and files[0].count(b"\n") > 10, table
