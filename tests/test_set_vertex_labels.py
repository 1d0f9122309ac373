"""Vertex relabel on the resident graph (include/gnnpe_hip.h): gnnpe_set_vertex_labels and gnnpe_labels_download, the relabel loop
with gnnpe_refine_sets_delta_vertices, and `gnnpe_main --set-labels`.

The yardstick of the state after a relabel is a fresh context loaded with the new labels (gnnpe_load_csr, existing code): the
labels, x / nx / vde bit for bit, the counts of refine_sets in the four modes.  The relabel identity |M'| = |M| - DeltaV(G, C, S) +
DeltaV(G', C', S) is held between plain counts of existing code on both sides."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_delta as dl
import test_refine_delta_vertices as dv
import test_refine_sets as rs
import test_refine_sets_shapes as sh
from pge_support import ladder_graph, ladder_vertices

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
MODES = dl.MODES


def _h1_four_labels():
    """H1 of test_refine_sets_shapes with the four labels its generator draws, and S: the longest row, a vertex of degree 1, an
    isolated vertex, two adjacent vertices, vertex n - 1, 50 random vertices (seed 4100)"""
    from gnnpe_amd import synth
    g = synth.powerlaw_graph(2000, 6000, exponent=2.1, max_degree=150, n_labels=4, seed=5)
    deg = np.diff(g["offsets"].astype(np.int64))
    o = g["offsets"].astype(np.int64)
    w = int(np.nonzero((deg >= 2) & (deg <= 64))[0][0])
    S = np.unique(np.array([int(np.argmax(deg)), int(np.nonzero(deg == 1)[0][0]), int(np.nonzero(deg == 0)[0][0]), w, int(g["nbrs"][o[w]]),
                            g["n"] - 1] + np.random.default_rng(4100).choice(g["n"], 50, replace=False).tolist(), np.int64))
    assert (deg[S] > 64).any() and (deg[S] == 0).any() and len(set(g["labels"].tolist())) == 4
    return dict(n=g["n"], offsets=g["offsets"], nbrs=g["nbrs"], labels=g["labels"].astype(np.uint32)), S


def _ladder_case():
    """the degree ladder (degrees 0 .. 257, four labels) and S: a vertex of degree 257 with 40 of its neighbours, a vertex of degree
    100 and one of degree 65 with ten neighbours each (k_vde_hubs reads their relabelled neighbour labels), vertices of degree
    0, 1 and 64, and 30 random vertices (seed 4200)"""
    g = ladder_graph(4)
    o = g["offsets"].astype(np.int64)
    parts = []
    for d, k in ((257, 40), (100, 10), (65, 10)):
        v = int(ladder_vertices(d)[0])
        parts += [v] + g["nbrs"][o[v]:o[v] + k].tolist()
    parts += [int(ladder_vertices(d)[1]) for d in (0, 1, 64)]
    S = np.unique(np.array(parts + np.random.default_rng(4200).choice(g["n"], 30, replace=False).tolist(), np.int64))
    return dict(n=g["n"], offsets=g["offsets"], nbrs=g["nbrs"], labels=g["labels"].astype(np.uint32)), S


def _mixed_queries(tmp_path):
    """triangle and diamond with mixed query labels, and with one label"""
    return [sh._shape_file(tmp_path, name, labels) for name in ("triangle", "diamond")
            for labels in ([i % 2 for i in range(sh.SHAPES[name][0])], [1] * sh.SHAPES[name][0])]


def test_binding_declares_the_relabel_calls():
    """CPU: the two calls are declared, exported by libgnnpe_hip.so and wrapped"""
    from gnnpe_amd import binding
    lib = binding.load()
    for name in ("gnnpe_set_vertex_labels", "gnnpe_labels_download"):
        assert name in binding.SIGNATURES and hasattr(lib, name)
    assert hasattr(binding.Engine, "set_vertex_labels") and hasattr(binding.Engine, "download_labels")
    assert lib.gnnpe_abi_version() == binding.ABI_VERSION == 20


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["h1", "ladder"])
def test_gpu_relabel_equals_a_fresh_load(tmp_path, which):
    """a. after set_vertex_labels the context is what a fresh context loaded with the new labels is: download_labels, x, nx and vde
    bit for bit (the ladder's rows of 65, 100 and 257 entries go through k_vde_hubs, which reads the patched neighbour labels),
    and the counts of refine_sets in the four modes for triangle and diamond with mixed and with single query labels.  The same
    pair listed twice means it once; a second relabel back to the old labels gives the old state"""
    from gnnpe_amd import binding, synth
    g, S = _h1_four_labels() if which == "h1" else _ladder_case()
    g_new, new = dv._relabelled(g, S, 4300, 4)
    assert (g_new["labels"][S] != g["labels"][S]).all() and np.array_equal(np.delete(g_new["labels"], S), np.delete(g["labels"], S))
    sn = synth.degree_order(g["offsets"])
    table = binding.host_label_table(4, 2)
    queries = _mixed_queries(tmp_path)
    eng, fresh = ex._engine(binding, g, sn, 2), ex._engine(binding, g_new, sn, 2)
    try:
        assert np.array_equal(eng.download_labels(), g["labels"])
        old = eng.vde()
        ms = eng.set_vertex_labels(np.concatenate([S, S[:5]]), np.concatenate([new, new[:5]]), timing=True)
        assert ms > 0
        assert np.array_equal(eng.download_labels(), g_new["labels"]) and np.array_equal(fresh.download_labels(), g_new["labels"])
        # order and slab are reset as a load resets them: the order is given again, as after load_csr
        with pytest.raises(binding.GnnpeError):
            eng.count_paths(2)
        eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
        eng.set_label_table(table)
        got, want = eng.vde(), fresh.vde()
        for a, b, what in zip(got, want, ("x", "nx", "vde")):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what
        assert not np.array_equal(got[1].view(np.uint64), old[1].view(np.uint64))
        assert eng.count_paths(2) == fresh.count_paths(2)
        for qp in queries:
            bm = ex._ld_bitmap(g_new, qp)
            for distinct, induced in MODES:
                a = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                assert a == fresh.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0], (qp, distinct, induced)
                assert a == binding.host_refine_sets(g_new, qp, bm, FULL, distinct=distinct, induced=induced)
        eng.set_vertex_labels(S, g["labels"][S])
        assert np.array_equal(eng.download_labels(), g["labels"])
        eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
        back = eng.vde()
        for a, b in zip(back, old):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["h1", "ladder"])
def test_gpu_relabel_identity(tmp_path, which):
    """b. the relabel loop on the device, labels-only bitmaps of each graph, the four modes, triangle and diamond with mixed and
    with single query labels: |M(G', C')| == |M(G, C)| - DeltaV(G, C, S) + DeltaV(G', C', S), each term from the device and equal
    to the host form's; the relabel loses matches and gains matches"""
    from gnnpe_amd import binding, synth
    g, S = _h1_four_labels() if which == "h1" else _ladder_case()
    g_new, new = dv._relabelled(g, S, 4400, 4)
    sn = synth.degree_order(g["offsets"])
    queries = _mixed_queries(tmp_path)
    eng = ex._engine(binding, g, sn, 2)
    try:
        before = {}
        for qp in queries:
            bm = dl._label_bitmap(g, qp)
            for distinct, induced in MODES:
                m = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                lost = eng.refine_sets_delta_vertices(qp, bm, S, distinct=distinct, induced=induced)[0]
                assert lost == binding.host_refine_sets_delta_vertices(g, qp, bm, S, FULL, distinct=distinct, induced=induced)
                before[qp, distinct, induced] = (m, lost)
        eng.set_vertex_labels(S, new)
        lost_n = gained_n = 0
        for qp in queries:
            bm = dl._label_bitmap(g_new, qp)
            for distinct, induced in MODES:
                m, lost = before[qp, distinct, induced]
                gained = eng.refine_sets_delta_vertices(qp, bm, S, distinct=distinct, induced=induced)[0]
                assert gained == binding.host_refine_sets_delta_vertices(g_new, qp, bm, S, FULL, distinct=distinct, induced=induced)
                after = eng.refine_sets(qp, bm, limit=FULL, distinct=distinct, induced=induced)[0]
                assert after == m - lost + gained, (qp, distinct, induced, after, m, lost, gained)
                lost_n += lost > 0
                gained_n += gained > 0
        assert lost_n >= 4 and gained_n >= 4, (lost_n, gained_n)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cursors_refusals_and_the_label_check(tmp_path_factory, tmp_path):
    """c. an open match cursor refuses after a successful relabel and goes on after a refused one and after count == 0; every
    refusal (an id >= n, one vertex with two labels, a null list with a count, the multigraph state, a slab context, no graph)
    leaves download_labels byte for byte as it was; a label past the label table is found by the next vde, as after a load"""
    import ctypes as C
    from gnnpe_amd import binding, synth
    g, S = _h1_four_labels()
    sn = synth.degree_order(g["offsets"])
    qp = sh._shape_file(tmp_path, "triangle", [0, 1, 0])
    bm = ex._ld_bitmap(g, qp)
    count = binding.host_refine_sets(g, qp, bm, FULL)
    assert count > 100
    eng = ex._engine(binding, g, sn, 2)
    try:
        cur = binding.MatchCursor(eng, qp, bm, 16)
        seen = len(cur.next()[0])
        for vs, ls, msg in (([3, g["n"]], [1, 1], "not a vertex"), ([g["n"] + 9], [0], "not a vertex"), ([5, 7, 5], [1, 2, 3], "labels 1 and 3")):
            with pytest.raises(binding.GnnpeError, match=msg):
                eng.set_vertex_labels(vs, ls)
            assert np.array_equal(eng.download_labels(), g["labels"])
            seen += len(cur.next()[0])
        u32p = C.POINTER(C.c_uint32)
        assert eng.lib.gnnpe_set_vertex_labels(eng.ctx, None, None, 2, None) == -1 and b"null argument" in eng.lib.gnnpe_last_error()
        assert np.array_equal(eng.download_labels(), g["labels"])
        eng.set_vertex_labels([], [])  # count == 0: nothing changes, the cursor lives
        assert np.array_equal(eng.download_labels(), g["labels"])
        seen += len(cur.next()[0])
        assert seen > 16  # the cursor went on after every refusal
        eng.set_vertex_labels([5, 7, 5], [1, 2, 1])  # the same pair twice means it once
        want = g["labels"].copy()
        want[[5, 7]] = (1, 2)
        assert np.array_equal(eng.download_labels(), want)
        with pytest.raises(binding.GnnpeError):
            cur.next()
        cur.close()
        # a label the table has no row for: the next vde checks the labels again, as after a load
        eng.set_vertex_labels([11], [4])
        eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
        with pytest.raises(binding.GnnpeError, match="no row in the 4-row label table"):
            eng.vde()
        eng.set_vertex_labels([11], [0])
        eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
        eng.vde()
        now = eng.download_labels()
        eng.set_multigraph_rows(g["offsets"].astype(np.uint64), g["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.set_vertex_labels([1], [1])
        eng.load_csr(g["offsets"], g["nbrs"], now)
        assert np.array_equal(eng.download_labels(), now)
        half = g["n"] // 2
        o = g["offsets"].astype(np.uint64)
        eng.load_rows(g["n"], now, np.arange(half, dtype=np.uint32), o[:half + 1], g["nbrs"][:int(o[half])])
        for call in (lambda: eng.set_vertex_labels([1], [1]), eng.download_labels):
            with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
                call()
    finally:
        eng.close()
    bare = binding.Engine(0)
    try:
        with pytest.raises(binding.GnnpeError, match="gnnpe_load_csr"):
            bare.set_vertex_labels([0], [0])
    finally:
        bare.close()


@pytest.mark.gpu
def test_gpu_cli_set_labels(tmp_path, test_graph):
    """d. gnnpe_main -m online --exact --refine sets --set-labels FILE on the golden test graph prints what the same command prints
    on a graph file written with the new labels (metadata block, plan size, answer), for q1 and q2 in mode 0 and DISTINCT |
    INDUCED; the answer is the host form's on the relabelled graph"""
    from gnnpe_amd import binding
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    n = len(test_graph["labels"])
    rng = np.random.default_rng(4500)
    S = np.sort(rng.choice(n, 15, replace=False))
    n_labels = int(test_graph["labels"].max()) + 1
    g_new, new = dv._relabelled(dict(n=n, offsets=test_graph["offsets"], nbrs=test_graph["nbrs"], labels=test_graph["labels"].astype(np.uint32)),
                                S, 4600, n_labels)
    lf = str(tmp_path / "labels.txt")
    open(lf, "w").write("".join(f"{v} {l}\n" for v, l in zip(S.tolist(), new.tolist())))
    new_graph = str(tmp_path / "relabelled.graph")
    with open(new_graph, "w") as out:
        for ln in open(graph):
            f = ln.split()
            if f and f[0] == "v":
                f[2] = str(int(g_new["labels"][int(f[1])]))
                ln = " ".join(f) + "\n"
            out.write(ln)
    root = ex._dataset(tmp_path, graph)
    for q in ("q1", "q2"):
        qp = os.path.join(ONLINE, f"{q}.graph")
        ld = ex._ld_bitmap(g_new, qp)
        for flags, kw in (([], {}), (["--distinct", "--induced"], dict(distinct=True, induced=True))):
            tail = ["-q", qp, "-p", "2", "-m", "online", "--exact", "--refine", "sets"] + flags
            a = subprocess.run([CLI, "-f", root, "-d", graph] + tail + ["--set-labels", lf], capture_output=True, text=True, timeout=300)
            b = subprocess.run([CLI, "-f", root, "-d", new_graph] + tail, capture_output=True, text=True, timeout=300)
            assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
            strip = lambda s: [ln.split(" Query Time")[0] for ln in s.splitlines()]
            assert strip(a.stdout) == strip(b.stdout), (a.stdout, b.stdout)
            ans = int(next(ln for ln in a.stdout.splitlines() if ln.startswith("Answer Number: ")).split()[2])
            assert ans == binding.host_refine_sets(g_new, qp, ld, FULL, **kw), (q, flags)
