"""Vertex removals and additions on a CSR (include/gnnpe_hip.h, "vertex removals and additions on the resident graph"):
gnnpe_host_csr_apply_vertices on the host, gnnpe_csr_apply_vertices on the graph a context holds with its vertex and entry maps,
gnnpe_csr_carry_vertices, the removal and growth loops with the delta calls, and `gnnpe_main --apply-vertices`.

The yardstick for a graph after a batch is always numpy (_apply_np: a keep mask, cumsum for the new ids, the kept keys relabelled
and regrouped, the entry map by searchsorted among the old keys), never the library.  The host form is held to it bit for bit, the
device form to the host form and to numpy, and to a FRESH engine that loaded numpy's G' for everything derived from the rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_csr_apply_edges as ap
import test_csr_entry_map as em
import test_online_exact as ex
import test_refine_delta as dl
import test_refine_edge_counts as re_
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
NO = 0xFFFFFFFF  # GNNPE_NO_VERTEX
ERR_ARG, ERR_UNSUPPORTED = -1, -3
VERT_TILE = 2048  # kVertTile of csrc/gnnpe_update_vertices.hip: entries of the old array per block and step of the compaction
CANARY = 0xABCD1234
SIX_SHAPES = ("edge", "wedge", "triangle", "C4", "diamond", "K4")
LOOP_SHAPES = ("triangle", "wedge", "diamond")
_u32p = C.POINTER(C.c_uint32)


# ---- helpers --------------------------------------------------------------------------------------------------------------

def _ids(a):
    return np.asarray(a, np.int64).reshape(-1)


def _apply_np(g, rem, add):
    """the numpy yardstick: (g2, vertex_map, entry_map) of g without the vertices of `rem`, with one empty-rowed vertex per label
    of `add` appended"""
    n = len(g["labels"])
    rem, add = _ids(rem), _ids(add)
    keep = np.ones(n, bool)
    keep[rem] = False
    new_id = np.cumsum(keep) - 1
    src, k0 = re_._csr_keys(g)
    dst = g["nbrs"].astype(np.int64)
    both = keep[src] & keep[dst]
    n2 = int(keep.sum()) + len(add)
    keys = np.sort(new_id[src[both]] * n2 + new_id[dst[both]])
    offsets = np.concatenate([[0], np.cumsum(np.bincount(keys // max(n2, 1), minlength=n2))]).astype(np.uint32)
    vmap = np.concatenate([np.nonzero(keep)[0], np.full(len(add), NO, np.int64)])
    g2 = dict(n=n2, offsets=offsets, nbrs=(keys % max(n2, 1)).astype(np.uint32),
              labels=np.concatenate([g["labels"][keep], add]).astype(np.uint32))
    old_keys = vmap[keys // max(n2, 1)] * n + vmap[keys % max(n2, 1)]  # (no entry touches an added vertex)
    emap = np.searchsorted(k0, old_keys)
    assert len(keys) == 0 or (k0[emap] == old_keys).all()
    return g2, vmap.astype(np.uint32), emap.astype(np.uint32)


def _same_graph(g, got):
    return all(np.asarray(got[k]).dtype == np.uint32 and np.array_equal(got[k], g[k]) for k in ("offsets", "nbrs", "labels"))


def _chain(g0, rng):
    """the five batches of the issue, each on the result of the one before: add only, remove only, both, all but one vertex
    removed, additions into the one-vertex graph.  Yields (name, g, rem, add, g2, vmap, emap)"""
    g = g0
    for name in ("add", "remove", "both", "all but one", "into one"):
        n = g["n"]
        if name == "add":
            rem, add = [], rng.integers(0, 3, 5)
        elif name == "remove":
            rem, add = rng.choice(n, min(7, n - 1), replace=False), []
        elif name == "both":
            rem, add = rng.choice(n, min(6, n - 1), replace=False), rng.integers(0, 3, 4)
        elif name == "all but one":
            rem, add = np.delete(np.arange(n), int(rng.integers(0, n))), []
        else:
            rem, add = [], rng.integers(0, 3, 6)
        g2, vmap, emap = _apply_np(g, rem, add)
        yield name, g, _ids(rem), _ids(add), g2, vmap, emap
        g = g2


_CHAINS = []


def _chains(tmp_path_factory):
    """the 19 small graphs and H1 with the five chained batches each: 100 cases, computed once"""
    if not _CHAINS:
        graphs = ap._small_graphs() + [sh._h1(tmp_path_factory)["g"]]
        assert len(graphs) == 20
        for gi, g0 in enumerate(graphs):
            _CHAINS.append(list(_chain(g0, np.random.default_rng(7100 + gi))))
    return _CHAINS


def _noisy(rem, rng):
    """the same set with repeats, shuffled"""
    rem = _ids(rem)
    if not len(rem):
        return rem
    r = np.concatenate([rem, rem[::2], rem[:3]])
    return r[rng.permutation(len(r))]


def _raw_host(binding, g, rem, add, cap=None, null=()):
    """gnnpe_host_csr_apply_vertices through ctypes, the outputs canary-filled: (rc, n_after, entries_after, offsets, nbrs, labels,
    vmap).  null: names of the lists handed over as NULL with their count"""
    o, nb, lab = (np.ascontiguousarray(g[k], np.uint32) for k in ("offsets", "nbrs", "labels"))
    r, a = np.ascontiguousarray(_ids(rem), np.uint32), np.ascontiguousarray(_ids(add), np.uint32)
    room = len(lab) + len(a)
    cap = len(nb) if cap is None else cap
    oo, on, ol, vm = (np.full(k, CANARY, np.uint32) for k in (room + 1, max(cap, 1), room, room))
    n2, after = C.c_uint32(777), C.c_uint64(777)
    rc = binding.load().gnnpe_host_csr_apply_vertices(len(lab), o.ctypes.data_as(_u32p), nb.ctypes.data_as(_u32p), lab.ctypes.data_as(_u32p),
                                                      None if "remove" in null else r.ctypes.data_as(_u32p), len(r),
                                                      None if "add" in null else a.ctypes.data_as(_u32p), len(a), oo.ctypes.data_as(_u32p),
                                                      on.ctypes.data_as(_u32p), cap, ol.ctypes.data_as(_u32p), vm.ctypes.data_as(_u32p),
                                                      C.byref(n2), C.byref(after))
    return rc, n2.value, after.value, oo, on, ol, vm


def _raw_device(eng, rem, add, null=()):
    """gnnpe_csr_apply_vertices through ctypes: (rc, message, n_after, entries_before, entries_after, vertex map pointer)"""
    r, a = np.ascontiguousarray(_ids(rem), np.uint32), np.ascontiguousarray(_ids(add), np.uint32)
    n2, b, af, vp, ep = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7), C.c_void_p(7), C.c_void_p(7)
    rc = eng.lib.gnnpe_csr_apply_vertices(eng.ctx, None if "remove" in null or not len(r) else r.ctypes.data_as(_u32p), len(r),
                                          None if "add" in null or not len(a) else a.ctypes.data_as(_u32p), len(a), C.byref(n2), C.byref(b),
                                          C.byref(af), C.byref(vp), C.byref(ep), None)
    return rc, eng.lib.gnnpe_last_error().decode() if rc else "", n2.value, b.value, af.value, vp.value


def _load(eng, g):
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])


def _device_graph(eng):
    o, nb = eng.download_csr()
    return dict(offsets=o, nbrs=nb, labels=eng.download_labels())


def _check_apply(eng, binding, g, rem, add, want, rng=None, what=""):
    """apply_vertices(entry_map=True) of the batch on the context (which holds g): counts, both maps, download and labels against
    numpy's (g2, vmap, emap) and against the host form"""
    g2, vmap, emap = want
    n2, before, after, vview, eview = eng.apply_vertices(rem if rng is None else _noisy(rem, rng), add, entry_map=True)
    assert (n2, before, after) == (g2["n"], len(g["nbrs"]), len(g2["nbrs"])) and eng.n == n2 and eng.entries == after, what
    assert vview.shape == (n2,) and eview.shape == (after,)
    assert np.array_equal(eng.vertex_map_to_host(vview), vmap), what
    assert np.array_equal(eng.entry_map_to_host(eview), emap), what
    got = _device_graph(eng)
    assert _same_graph(g2, got), what
    h2, hmap = binding.host_apply_vertices(g, rem, add)
    assert _same_graph(h2, got) and np.array_equal(hmap, vmap), what
    if after:
        assert (np.diff(emap.astype(np.int64)) > 0).all()


# ---- CPU: the host form ------------------------------------------------------------------------------------------------------

def test_binding_declares_the_vertex_calls():
    """the three calls are declared, exported by libgnnpe_hip.so and wrapped; the ABI version stays"""
    from gnnpe_amd import binding
    lib = binding.load()
    for name in ("gnnpe_host_csr_apply_vertices", "gnnpe_csr_apply_vertices", "gnnpe_csr_carry_vertices"):
        assert name in binding.SIGNATURES and hasattr(lib, name)
    for name in ("apply_vertices", "carry_vertices", "vertex_map_to_host"):
        assert hasattr(binding.Engine, name)
    assert binding.NO_VERTEX == NO and lib.gnnpe_abi_version() == binding.ABI_VERSION == 20


def test_host_form_against_numpy(tmp_path_factory):
    """1. the 19 small graphs and H1, the five chained batches each (add only, remove only, both, all but one vertex removed,
    additions into the one-vertex graph): offsets, neighbours, labels, vertex map and both counts equal numpy's bit for bit; a
    remove list with repeats in noise order gives the same result; the empty batch gives the graph back with the identity map"""
    from gnnpe_amd import binding
    for gi, chain in enumerate(_chains(tmp_path_factory)):
        rng = np.random.default_rng(7200 + gi)
        for name, g, rem, add, g2, vmap, _ in chain:
            rc, n2, after, oo, on, ol, vm = _raw_host(binding, g, rem, add)
            assert rc == 0 and (n2, after) == (g2["n"], len(g2["nbrs"])), (gi, name)
            got = dict(offsets=oo[:n2 + 1], nbrs=on[:after], labels=ol[:n2])
            assert _same_graph(g2, got) and np.array_equal(vm[:n2], vmap), (gi, name)
            assert (oo[n2 + 1:] == CANARY).all() and (on[after:] == CANARY).all() and (vm[n2:] == CANARY).all() and (ol[n2:] == CANARY).all()
            h2, hmap = binding.host_apply_vertices(g, _noisy(rem, rng), add)
            assert _same_graph(g2, h2) and h2["n"] == g2["n"] and np.array_equal(hmap, vmap), (gi, name)
        g = chain[0][1]
        same, ident = binding.host_apply_vertices(g)
        assert _same_graph(g, same) and np.array_equal(ident, np.arange(g["n"]))
        assert chain[3][4]["n"] == 1 and len(chain[3][4]["nbrs"]) == 0 and chain[4][4]["n"] == 7


def test_host_refusals(tmp_path_factory):
    """2. each refusal of the host form returns its code with every output array untouched (canary-filled): an id >= n, n' == 0, a
    null list with a count > 0, and an out_cap one word short -- that one with *n_after and *n_entries_after set"""
    from gnnpe_amd import binding
    g = ap._small_graphs()[3]
    n = g["n"]
    untouched = lambda r: all((a == CANARY).all() for a in r[3:])
    r = _raw_host(binding, g, [3, n], [])
    assert r[0] == ERR_ARG and untouched(r) and "not a vertex" in binding.load().gnnpe_last_error().decode()
    r = _raw_host(binding, g, np.arange(n), [])
    assert r[0] == ERR_ARG and untouched(r) and "leaves no vertex" in binding.load().gnnpe_last_error().decode()
    for which, rem, add in (("remove", [1, 2], []), ("add", [], [0, 1])):
        r = _raw_host(binding, g, rem, add, null=(which,))
        assert r[0] == ERR_ARG and untouched(r) and "null" in binding.load().gnnpe_last_error().decode()
    g2, _, _ = _apply_np(g, [5], [1, 1])
    r = _raw_host(binding, g, [5], [1, 1], cap=len(g2["nbrs"]) - 1)
    assert r[0] == ERR_ARG and untouched(r) and (r[1], r[2]) == (g2["n"], len(g2["nbrs"]))
    r = _raw_host(binding, g, [5], [1, 1], cap=len(g2["nbrs"]))
    assert r[0] == 0
    with pytest.raises(binding.GnnpeError, match="not a vertex"):
        binding.host_apply_vertices(g, [n + 4])


def test_cli_apply_vertices_outside_exact_mode_and_malformed_files(tmp_path):
    """3. no GPU is touched: --apply-vertices outside exact -m online / -m filter is refused, and so is a file with a line that is
    neither `- v` nor `+ label`"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    good = str(tmp_path / "good.txt")
    open(good, "w").write("- 3\n+ 1\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--apply-vertices", good], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and "--apply-vertices applies to exact" in r.stderr + r.stdout
    for k, text in enumerate(("- 3\n* 4\n", "+ x\n", "- 3 4\n", "- 99999999999\n", "3\n")):
        bad = str(tmp_path / f"bad{k}.txt")
        open(bad, "w").write(text)
        r = subprocess.run([CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact", "--refine", "sets",
                            "--apply-vertices", bad], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode != 0 and "one `- v` or `+ label` per line expected" in r.stderr + r.stdout, (text, r.stderr)


# ---- GPU: the device form ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_device_form_on_the_chains(tmp_path_factory):
    """4. the same 100 chained cases on one context per graph, each batch applied to what the batch before left: n_after, the entry
    counts, csr_download, labels_download and both maps copied back equal numpy's and the host form's bit for bit; the remove lists
    go in with repeats and in noise order"""
    from gnnpe_amd import binding
    for gi, chain in enumerate(_chains(tmp_path_factory)):
        rng = np.random.default_rng(7300 + gi)
        eng = binding.Engine(0)
        try:
            _load(eng, chain[0][1])
            for name, g, rem, add, g2, vmap, emap in chain:
                _check_apply(eng, binding, g, rem, add, (g2, vmap, emap), rng, (gi, name))
        finally:
            eng.close()


def _place_cases():
    g = em._place_graph()
    n = g["n"]
    o = g["offsets"].astype(np.int64)
    deg = np.diff(o)
    row = lambda v: g["nbrs"][o[v]:o[v + 1]].astype(np.int64)
    assert n % 32 != 0 and len(g["nbrs"]) > 2 * VERT_TILE + 500 and deg[123] == 0 and deg[350] > 64
    r1 = int(np.searchsorted(o, VERT_TILE, side="right")) - 1
    assert o[r1] < VERT_TILE < o[r1 + 1] - 1
    in_tile = np.nonzero((o[1:] > VERT_TILE) & (o[:-1] < 2 * VERT_TILE))[0]
    w = int(np.nonzero(deg >= 2)[0][np.argmin(deg[deg >= 2])])
    cases = [("vertex 0", [0], []), ("vertex n - 1", [n - 1], []), ("31", [31], []), ("32", [32], []), ("63", [63], []), ("64", [64], []),
             ("31, 32, 63 and 64", [31, 32, 63, 64], []), ("an aligned word", np.arange(64, 96), []),
             ("an isolated vertex: nothing is dropped", [123], []), ("a row of 150 entries", [350], []),
             ("a row across the first tile boundary", [r1], []), ("every entry of the second tile dropped", in_tile, []),
             ("both ends of an edge", [0, 1], []), ("all neighbours of a vertex: its row becomes empty", row(w), []),
             ("add and remove", [0, 31, 350, n - 1], [0, 0, 0]), ("the last word and additions", np.arange(n - n % 32, n), [0] * 40)]
    assert len(row(w)) >= 2 and 1 in row(0).tolist()
    return g, cases


@pytest.mark.gpu
def test_gpu_places(tmp_path_factory):
    """5. one batch each on the place graph of test_csr_entry_map (700 vertices, n % 32 = 28, 6 000 and some entries: three tiles of
    the compaction, vertex 350 a row of 150 entries, vertex 123 isolated): vertex 0 removed; vertex n - 1; vertices 31, 32, 63 and 64
    singly and together (the bitmap's word edges); the aligned word 64 .. 95; the isolated vertex alone (nothing is dropped); the
    row of 150 entries (more than one wave step); the row that straddles the first tile boundary; every row that reaches into the
    second tile (all of the tile's entries dropped); both ends of an edge; all neighbours of one vertex (two or more removed
    vertices share a neighbour whose row becomes empty); add and remove in one batch; the vertices of the last, partial bitmap word
    with 40 additions.  Both maps, the download and the labels equal numpy's and the host form's"""
    from gnnpe_amd import binding
    g, cases = _place_cases()
    eng = binding.Engine(0)
    try:
        for name, rem, add in cases:
            _load(eng, g)
            want = _apply_np(g, rem, add)
            _check_apply(eng, binding, g, _ids(rem), _ids(add), want, None, name)
            if name.startswith("all neighbours"):
                assert (np.diff(want[0]["offsets"].astype(np.int64)) == 0).sum() > 1
            if name.startswith("an isolated"):
                assert len(want[0]["nbrs"]) == len(g["nbrs"])
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_growth_past_every_vertex_sized_buffer():
    """6. from a 50-vertex graph 5 000 vertices are added in one batch (every n-sized array of the context has to grow), then
    apply_edges inserts edges between old and new ids and among the new ones: download and labels equal numpy's, and the counts of
    the triangle equal a fresh engine's"""
    from gnnpe_amd import binding, synth
    g0 = synth.gnm_graph(50, 120, n_labels=2, seed=7400)
    g = dict(n=50, offsets=g0["offsets"], nbrs=g0["nbrs"], labels=g0["labels"].astype(np.uint32))
    rng = np.random.default_rng(7401)
    add = rng.integers(0, 2, 5000)
    want = _apply_np(g, [], add)
    g2 = want[0]
    I = np.unique(np.stack([rng.integers(0, 50, 300), rng.integers(50, 5050, 300)], axis=1), axis=0)
    I = np.concatenate([I, np.stack([np.arange(60, 160), np.arange(4000, 4100)], axis=1), [[5049, 0], [5048, 5049]]])
    I = I[np.unique(np.minimum(I[:, 0], I[:, 1]) * 6000 + np.maximum(I[:, 0], I[:, 1]), return_index=True)[1]]
    g3 = ap._apply_np(g2, I, [])
    eng, fresh = binding.Engine(0), binding.Engine(0)
    try:
        _load(eng, g)
        _check_apply(eng, binding, g, [], add, want, None, "growth")
        assert eng.apply_edges(I) == len(g3["nbrs"])
        got = _device_graph(eng)
        assert ap._same(g3, got["offsets"], got["nbrs"]) and np.array_equal(got["labels"], g2["labels"])
        _load(fresh, dict(g3, labels=g2["labels"]))
        assert eng.rows_held() == fresh.rows_held()
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_gpu_state_of_a_fresh_load(tmp_path):
    """7. H1 with its four labels: the longest row, an isolated vertex, vertex 0, vertex n - 1 and 40 random vertices removed, 10
    added.  Afterwards the context is what a fresh context that loaded numpy's G' is: rows_held; after the same order and label
    table x, nx and vde bit for bit and the l = 2 path count; refine_sets in the four modes on six query shapes (mixed and single
    query labels); the wedge's per-vertex table.  The old order is gone, as after a load"""
    import test_set_vertex_labels as tsl
    from gnnpe_amd import binding, synth
    g, _ = tsl._h1_four_labels()
    deg = np.diff(g["offsets"].astype(np.int64))
    rng = np.random.default_rng(7500)
    rem = np.unique(np.concatenate([[int(np.argmax(deg)), int(np.nonzero(deg == 0)[0][0]), 0, g["n"] - 1], rng.choice(g["n"], 40, replace=False)]))
    add = rng.integers(0, 4, 10)
    g2, _, _ = _apply_np(g, rem, add)
    sn2 = synth.degree_order(g2["offsets"])
    eng, fresh = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2), ex._engine(binding, g2, sn2, 2)
    try:
        eng.count_paths(2)  # derived state of the old graph, to be reset
        eng.apply_vertices(rem, add)
        assert eng.rows_held() == fresh.rows_held()
        with pytest.raises(binding.GnnpeError):
            eng.count_paths(2)
        eng.set_order(sn2, np.zeros(g2["n"], np.uint32), 1)
        eng.set_label_table(binding.host_label_table(4, 2))
        for a, b, what in zip(eng.vde(), fresh.vde(), ("x", "nx", "vde")):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what
        assert eng.count_paths(2) == fresh.count_paths(2) > 0
        moved = 0
        for name in SIX_SHAPES:
            k = sh.SHAPES[name][0]
            for labels in ([i % 2 for i in range(k)], [1] * k):
                qp = sh._shape_file(tmp_path, name, labels)
                bm = ex._ld_bitmap(g2, qp)
                for distinct, induced in dl.MODES:
                    a = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                    assert a == fresh.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0], (name, labels, distinct, induced)
                    moved += a > 0
        assert moved >= 16, moved  # (edge and wedge have matches in every mode and labelling)
        qp = sh._shape_file(tmp_path, "wedge", [1, 1, 1])
        bm = dl._label_bitmap(g2, qp)
        mine, theirs = (e.refine_sets_vertex_counts(qp, bm) for e in (eng, fresh))
        assert mine[0] == theirs[0] > 0 and mine[1] and mine[2].shape == (3, g2["n"]) and np.array_equal(mine[2], theirs[2])
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_gpu_transactions(tmp_path_factory):
    """8. every refusal (an id >= n, n' == 0, a null list with a count) leaves download, labels and the counts as they were and an
    open MatchCursor yields its next page; the empty batch keeps the cursor valid and yields identity maps; after a successful batch
    the same cursor refuses to go on.  carry_entries after apply_vertices(entry_map=False) and carry_vertices before any apply, after
    a refused apply and after a following load_csr return GNNPE_ERR_ARG; a stale vertex-map view is refused.  The multigraph state, a
    load_rows context and a context without a graph are GNNPE_ERR_UNSUPPORTED"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, qp = h["g"], h["q"]["triangle"]
    n, entries = g["n"], len(g["nbrs"])
    bm = h["bm"]["triangle"]["ld"]
    eng = ex._engine(binding, g, h["sn"], 2)

    room = em._dev(np.zeros(2 * (entries + 64), np.uint64))  # (a carry that is not refused would stay inside it)

    def carry(fn):
        rc = fn(eng.ctx, 1, 8, C.c_void_p(room.data_ptr()), C.c_void_p(room.data_ptr() + 8 * (entries + 64)), None)
        return rc, eng.lib.gnnpe_last_error().decode()

    try:
        rc, text = carry(eng.lib.gnnpe_csr_carry_vertices)
        assert rc == ERR_ARG and "no valid vertex map" in text
        cur = binding.MatchCursor(eng, qp, bm, 16)
        seen = len(cur.next()[0])
        for rem, add, null, msg in (([3, n], [], (), "not a vertex"), (np.arange(n), [], (), "leaves no vertex"),
                                    ([1, 2], [], ("remove",), "null argument"), ([], [1, 2], ("add",), "null argument")):
            rc, text, n2, b, a, vp = _raw_device(eng, rem, add, null)
            assert rc == ERR_ARG and msg in text and (n2, b, a) == (n, entries, entries) and not vp, (msg, rc, text)
            assert _same_graph(g, _device_graph(eng)) and eng.rows_held()[:2] == (n, entries)
            seen += len(cur.next()[0])
            rc, text = carry(eng.lib.gnnpe_csr_carry_vertices)
            assert rc == ERR_ARG and "no valid vertex map" in text
        with pytest.raises(binding.GnnpeError, match="not a vertex"):
            eng.apply_vertices([n])
        assert eng.n == n
        n2, b, a, vview, eview = eng.apply_vertices(entry_map=True)  # the empty batch
        assert (n2, b, a) == (n, entries, entries)
        assert np.array_equal(eng.vertex_map_to_host(vview), np.arange(n)) and np.array_equal(eng.entry_map_to_host(eview), np.arange(entries))
        seen += len(cur.next()[0])
        assert seen == 16 * 6  # the cursor went on after every refusal and after the empty batch
        n2, b, a, vview2, none = eng.apply_vertices()
        assert none is None and carry(eng.lib.gnnpe_csr_carry_entries)[0] == ERR_ARG
        with pytest.raises(binding.GnnpeError, match="stale vertex-map view"):
            eng.vertex_map_to_host(vview)
        seen += len(cur.next()[0])
        n2, b, a, vview3, none = eng.apply_vertices([int(np.argmax(h["deg"])), 9], [0])
        assert (n2, b) == (n - 1, entries) and a < entries and none is None
        rc, text = carry(eng.lib.gnnpe_csr_carry_entries)
        assert rc == ERR_ARG and "no valid entry map" in text
        with pytest.raises(binding.GnnpeError):
            cur.next()
        cur.close()
        with pytest.raises(binding.GnnpeError, match="stale vertex-map view"):
            eng.vertex_map_to_host(vview2)
        assert eng.vertex_map_to_host(vview3)[-1] == NO
        _load(eng, g)
        rc, text = carry(eng.lib.gnnpe_csr_carry_vertices)
        assert rc == ERR_ARG and "no valid vertex map" in text
        with pytest.raises(binding.GnnpeError, match="stale vertex-map view"):
            eng.vertex_map_to_host(vview3)
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        rc, text = _raw_device(eng, [1], [])[:2]
        assert rc == ERR_UNSUPPORTED and "simple graphs only" in text
        half = n // 2
        o = g["offsets"].astype(np.uint64)
        eng.load_rows(n, g["labels"], np.arange(half, dtype=np.uint32), o[:half + 1], g["nbrs"][:int(o[half])])
        rc, text = _raw_device(eng, [1], [])[:2]
        assert rc == ERR_UNSUPPORTED and "gnnpe_load_csr" in text
    finally:
        eng.close()
    bare = binding.Engine(0)
    try:
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            bare.apply_vertices([0])
    finally:
        bare.close()


@pytest.mark.gpu
def test_gpu_carry_vertices(tmp_path_factory):
    """9. after a batch on H1 (30 removed, 20 added) carry_vertices with 8- and 4-byte cells and 1 and 5 rows equals numpy's fancy
    indexing through the vertex map, zeros at the added vertices, src keeps its bytes and nothing is written around dst; the
    argument refusals (elem_bytes 3, overlapping ranges, a null dst, a misaligned dst) leave dst's canaries"""
    from gnnpe_amd import binding
    g = sh._h1(tmp_path_factory)["g"]
    rng = np.random.default_rng(7600)
    rem, add = rng.choice(g["n"], 30, replace=False), np.zeros(20, np.int64)
    g2, vmap, _ = _apply_np(g, rem, add)
    n, n2 = g["n"], g2["n"]
    eng = binding.Engine(0)
    try:
        _load(eng, g)
        eng.apply_vertices(rem, add)
        for n_rows, eb in ((1, 8), (5, 8), (1, 4), (5, 4)):
            dt, can = (np.uint64, em.CANARY64) if eb == 8 else (np.uint32, em.CANARY32)
            src = rng.integers(1, 1 << (8 * eb), (n_rows, n), dtype=dt)
            t_src, t_dst = em._dev(src), em._dev(np.full(n_rows * n2 + 128, can, dt))
            dst_ptr = t_dst.data_ptr() + 64 * eb
            ms = eng.carry_vertices(t_src, dst_ptr, n_rows, elem_bytes=eb, timing=True)
            eng.sync()
            got = em._host(t_dst, dt)
            assert ms > 0 and (got[:64] == can).all() and (got[64 + n_rows * n2:] == can).all(), (n_rows, eb)
            assert np.array_equal(got[64:64 + n_rows * n2].reshape(n_rows, n2), em._gather_np(src, vmap, n2)), (n_rows, eb)
            assert em._host(t_src, dt).tobytes() == src.tobytes()
        src = rng.integers(1, 1 << 64, (2, n), dtype=np.uint64)
        t_src, t_dst = em._dev(src), em._dev(np.full((2, n2 + 8), em.CANARY64, np.uint64))

        def refused(what, eb=8, s=None, d=None):
            rc = eng.lib.gnnpe_csr_carry_vertices(eng.ctx, 2, eb, C.c_void_p(t_src.data_ptr() if s is None else s),
                                                  C.c_void_p(t_dst.data_ptr() if d is None else d) if d != 0 else None, None)
            text = eng.lib.gnnpe_last_error().decode()
            eng.sync()
            assert rc == ERR_ARG and (em._host(t_dst, np.uint64) == em.CANARY64).all() and em._host(t_src, np.uint64).tobytes() == src.tobytes(), what
            return text

        assert "elem_bytes" in refused("elem_bytes 3", eb=3)
        assert "overlap" in refused("dst inside src", d=t_src.data_ptr() + 8 * n)
        assert "overlap" in refused("src inside dst", s=t_dst.data_ptr() + 16)
        assert "null" in refused("null dst", d=0)
        assert "aligned" in refused("misaligned dst", d=t_dst.data_ptr() + 4)
        eng.carry_vertices(t_src, t_dst, 2)
        eng.sync()
        assert np.array_equal(em._host(t_dst, np.uint64).ravel()[:2 * n2].reshape(2, n2), em._gather_np(src, vmap, n2))
    finally:
        eng.close()


def _loop_graph(which, tmp_path_factory):
    from gnnpe_amd import synth
    if which == "h1":
        return sh._h1(tmp_path_factory)["g"]
    g = synth.gnm_graph(200, 800, n_labels=3, seed=7700 + which)
    return dict(n=200, offsets=g["offsets"], nbrs=g["nbrs"], labels=g["labels"].astype(np.uint32))


def _carry_bitmap(bm, vmap, add_rows):
    """the caller's bitmap columns through the vertex map, in numpy: bit v' of row u = bit vmap[v'] of the old row, add_rows[u][i] for
    the i-th added vertex"""
    n2 = len(vmap)
    out = np.zeros((bm.shape[0], (n2 + 31) // 32), np.uint32)
    old = vmap != NO
    for u in range(bm.shape[0]):
        bit = np.zeros(n2, bool)
        ids = vmap[old].astype(np.int64)
        bit[old] = ((bm[u][ids >> 5] >> (ids & 31).astype(np.uint32)) & 1) != 0
        if add_rows is not None:
            bit[~old] = add_rows[u]
        out[u] = sh._row_of(np.nonzero(bit)[0], n2)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("which", ["h1"] + list(range(8)))
def test_gpu_removal_and_growth_loops(tmp_path_factory, tmp_path, which, induced):
    """10. the two loops of the header with no host copy of a table: H1 (one label) and 8 seeded G(200, 800) with 3 labels; mode 0
    and INDUCED; triangle, wedge and diamond (two query labels on the seeded graphs), labels-only candidate sets carried through
    the vertex map in numpy.  The count |M| and the tables VV (per vertex) and EV (per entry) of every shape live on the device from
    refine_sets_*_counts(device=True) to the end.
    Removal of 1, 5 and 40 random vertices, each step: lost = DeltaV(G, C, R); VV -= VV(G, C, R); EV -= EV(G, C, R);
    apply_vertices(R, entry_map=True); VV = carry_vertices(VV); EV = carry_entries(EV); |M| -= lost.
    Growth: apply_vertices(3 added vertices), both carries; then the edges I between them and old vertices: in the induced mode
    first |M| -= DeltaN(G', I) with its tables subtracted; apply_edges_map(I); EV = carry_entries(EV); |M| += Delta(G'', I) with its
    tables added.
    After every step the count, VV and EV copied back equal refine_sets / _vertex_counts / _edge_counts of a fresh context on
    numpy's graph; matches were lost and gained"""
    import torch
    from gnnpe_amd import binding, synth
    g = _loop_graph(which, tmp_path_factory)
    n_labels = int(g["labels"].max()) + 1
    qs = {name: sh._shape_file(tmp_path, name, [i % min(n_labels, 2) for i in range(sh.SHAPES[name][0])]) for name in LOOP_SHAPES}
    qlab = {name: binding.host_load_graph(qs[name])["labels"] for name in LOOP_SHAPES}
    bms = {name: dl._label_bitmap(g, qs[name]) for name in LOOP_SHAPES}
    rng = np.random.default_rng(7800 + (100 if which == "h1" else which))
    mode = dict(induced=induced)
    eng, fresh = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2), binding.Engine(0)
    M, VV, EV = {}, {}, {}
    lost_n = gained_n = 0

    def carry(tab, fn, width):
        for name in LOOP_SHAPES:
            dst = torch.empty((tab[name].shape[0], width), dtype=torch.int64, device="cuda:0")
            fn(tab[name], dst, dst.shape[0])
            eng.sync()
            tab[name] = dst

    def check(step):
        assert _same_graph(g, _device_graph(eng)), step
        _load(fresh, g)
        for name in LOOP_SHAPES:
            assert np.array_equal(bms[name], dl._label_bitmap(g, qs[name])), (step, name)
            assert M[name] == fresh.refine_sets(qs[name], bms[name], limit=FULL, **mode)[0], (step, name)
            want = fresh.refine_sets_vertex_counts(qs[name], bms[name], **mode)
            assert want[1] and np.array_equal(em._host(VV[name], np.uint64), want[2]), (step, name)
            want = fresh.refine_sets_edge_counts(qs[name], bms[name], **mode)
            assert want[1] and np.array_equal(em._host(EV[name], np.uint64), want[2]), (step, name)

    try:
        for name in LOOP_SHAPES:
            M[name] = eng.refine_sets(qs[name], bms[name], limit=FULL, **mode)[0]
            for tab, fn in ((VV, eng.refine_sets_vertex_counts), (EV, eng.refine_sets_edge_counts)):
                got = fn(qs[name], bms[name], device=True, **mode)
                assert got[1]
                tab[name] = torch.as_tensor(got[2], device="cuda:0").clone()
                torch.cuda.synchronize()
        for k in (1, 5, 40):
            R = rng.choice(g["n"], k, replace=False)
            for name in LOOP_SHAPES:
                lost = eng.refine_sets_delta_vertices(qs[name], bms[name], R, **mode)[0]
                assert eng.refine_sets_delta_vertices_vertex_counts(qs[name], bms[name], R, accum=VV[name].data_ptr(), sign=-1, **mode)[1]
                assert eng.refine_sets_delta_vertices_edge_counts(qs[name], bms[name], R, accum=EV[name].data_ptr(), sign=-1, **mode)[1]
                M[name] -= lost
                lost_n += lost > 0
            n2, before, after, vview, _ = eng.apply_vertices(R, entry_map=True)
            vmap = eng.vertex_map_to_host(vview)
            carry(VV, eng.carry_vertices, n2)
            carry(EV, eng.carry_entries, after)
            g, want_map, _ = _apply_np(g, R, [])
            assert np.array_equal(vmap, want_map)
            bms = {name: _carry_bitmap(bms[name], vmap, None) for name in LOOP_SHAPES}
            check(("removal", k))
        add = np.arange(3) % n_labels
        n2, before, after, vview, _ = eng.apply_vertices(None, add, entry_map=True)
        vmap = eng.vertex_map_to_host(vview)
        carry(VV, eng.carry_vertices, n2)
        carry(EV, eng.carry_entries, after)
        bms = {name: _carry_bitmap(bms[name], vmap, [add == qlab[name][u] for u in range(len(qlab[name]))]) for name in LOOP_SHAPES}
        g, _, _ = _apply_np(g, [], add)
        check("added")
        busy = np.nonzero(np.diff(g["offsets"].astype(np.int64)) >= 3)[0]
        I = np.array([(int(w), n2 - 3 + i) for i in range(3) for w in rng.choice(busy, 8, replace=False)] + [(n2 - 3, n2 - 2), (n2 - 2, n2 - 1)])
        for name in LOOP_SHAPES:
            if induced:
                M[name] -= eng.refine_sets_delta_nonedges(qs[name], bms[name], I)[0]
                assert eng.refine_sets_delta_nonedges_vertex_counts(qs[name], bms[name], I, accum=VV[name].data_ptr(), sign=-1)[1]
                assert eng.refine_sets_delta_nonedges_edge_counts(qs[name], bms[name], I, accum=EV[name].data_ptr(), sign=-1)[1]
        before, after, _ = eng.apply_edges_map(I)
        carry(EV, eng.carry_entries, after)
        g = ap._apply_np(g, I, [])
        for name in LOOP_SHAPES:
            gained = eng.refine_sets_delta(qs[name], bms[name], I, **mode)[0]
            assert eng.refine_sets_delta_vertex_counts(qs[name], bms[name], I, accum=VV[name].data_ptr(), sign=1, **mode)[1]
            assert eng.refine_sets_delta_edge_counts(qs[name], bms[name], I, accum=EV[name].data_ptr(), sign=1, **mode)[1]
            M[name] += gained
            gained_n += gained > 0
        check("grown")
        assert lost_n >= 3 and gained_n >= 1, (lost_n, gained_n)
    finally:
        eng.close()
        fresh.close()


def _write_graph(path, g):
    e = dl._und_edges(g)
    deg = np.diff(g["offsets"].astype(np.int64))
    with open(path, "w") as out:
        out.write(f"t {g['n']} {len(e)}\n")
        out.write("".join(f"v {v} {int(g['labels'][v])} {int(deg[v])}\n" for v in range(g["n"])))
        out.write("".join(f"e {a} {b}\n" for a, b in e.tolist()))


@pytest.mark.gpu
def test_gpu_cli_apply_vertices(tmp_path, test_graph):
    """11. gnnpe_main -m online --exact --refine sets --apply-vertices FILE on the golden test graph, alone and together with
    --apply-edges (whose file names the new ids) and --set-labels, prints what the same command prints on a graph file of numpy's
    G' (metadata block, plan size, answer): q1 in mode 0 alone, q2 in DISTINCT | INDUCED with the edges, q1 in both modes and q2 in
    mode 0 with all three; the answer is the host form's on G'"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    g = dict(n=len(test_graph["labels"]), offsets=test_graph["offsets"], nbrs=test_graph["nbrs"], labels=test_graph["labels"].astype(np.uint32))
    rng = np.random.default_rng(7900)
    deg = np.diff(g["offsets"].astype(np.int64))
    rem = np.unique(np.concatenate([[int(np.argmax(deg))], rng.choice(g["n"], 12, replace=False)]))
    n_labels = int(g["labels"].max()) + 1
    add = rng.integers(0, n_labels, 4)
    g1, _, _ = _apply_np(g, rem, add)
    vf, ef, lf = (str(tmp_path / f) for f in ("vertices.txt", "edges.txt", "labels.txt"))
    minus, plus = [f"- {v}\n" for v in rem.tolist()], [f"+ {l}\n" for l in add.tolist()]
    open(vf, "w").write("".join(minus[:3] + plus[:2] + minus[3:] + plus[2:]))
    new = np.arange(g1["n"] - 4, g1["n"])
    busy = np.nonzero(np.diff(g1["offsets"].astype(np.int64)) >= 3)[0]
    I = np.array([(int(w), int(v)) for v in new for w in rng.choice(busy, 6, replace=False)] + [(int(new[0]), int(new[1]))])
    D = dl._und_edges(g1)[rng.choice(len(dl._und_edges(g1)), 10, replace=False)]
    open(ef, "w").write("".join(f"+ {a} {b}\n" for a, b in I.tolist()) + "".join(f"- {a} {b}\n" for a, b in D.tolist()))
    g2 = ap._apply_np(g1, I, D)
    g2["labels"] = g1["labels"]
    S = np.concatenate([new[:2], rng.choice(g1["n"] - 4, 5, replace=False)])
    g3 = dict(g2, labels=g2["labels"].copy())
    g3["labels"][S] = (g3["labels"][S] + 1) % n_labels
    open(lf, "w").write("".join(f"{v} {int(g3['labels'][v])}\n" for v in S.tolist()))
    (tmp_path / "a").mkdir()
    root = ex._dataset(tmp_path / "a", graph)
    # (the vertex file has its `+` and `-` lines interleaved: the added vertices get their ids in the order of the `+` lines)
    plain, both = ([], {}), (["--distinct", "--induced"], dict(distinct=True, induced=True))
    for tag, flags, gx, runs in (("v", ["--apply-vertices", vf], g1, (("q1", plain),)),
                                 ("ve", ["--apply-vertices", vf, "--apply-edges", ef], g2, (("q2", both),)),
                                 ("vel", ["--set-labels", lf, "--apply-edges", ef, "--apply-vertices", vf], g3, (("q1", plain), ("q1", both), ("q2", plain)))):
        new_graph = str(tmp_path / f"{tag}.graph")
        _write_graph(new_graph, gx)
        (tmp_path / tag).mkdir()
        root_b = ex._dataset(tmp_path / tag, new_graph)
        for q, (mflags, kw) in runs:
            qp = os.path.join(ONLINE, f"{q}.graph")
            ld = ex._ld_bitmap(gx, qp)
            tail = ["-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets"] + mflags
            a = subprocess.run([CLI, "-f", root, "-d", graph] + tail + flags, capture_output=True, text=True, timeout=300)
            b = subprocess.run([CLI, "-f", root_b, "-d", new_graph] + tail, capture_output=True, text=True, timeout=300)
            assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
            strip = lambda s: [ln.split(" Query Time")[0] for ln in s.splitlines()]
            assert strip(a.stdout) == strip(b.stdout), (tag, a.stdout, b.stdout)
            ans = int(next(ln for ln in a.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
            assert ans == binding.host_refine_sets(gx, qp, ld, FULL, **kw), (tag, q, mflags)
