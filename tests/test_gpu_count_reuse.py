"""The structure of a ranked l = 2 count (pair records, record order and id words, start records, the total, the hub rows' pairs) is
built once per graph / order / membership / slab / record layout; later counts only refresh the embeddings inside the row blocks
(k_rows_refresh).  Every case here compares with a FRESH engine given the same final inputs (and with the oracle where the other GPU
tests do), bit for bit, and reads the library's `[count] structure: built | reused` line (GNNPE_DEBUG=1, read when a context is
created) to see which path a count took."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def binding():
    from gnnpe_amd import binding as b
    b.load()
    return b


@pytest.fixture()
def debug_lines(monkeypatch, capfd):
    """Contexts created while this fixture is active print their launch decisions; the returned callable gives the `[count] structure`
    decisions since it was last called."""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [ln.split(": ")[1] for ln in err.splitlines() if ln.startswith("[count] structure")]
    return take


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_table(n_labels, e, seed):
    """Not host_label_table: values of another distribution, no row sums to one."""
    return np.random.default_rng(seed).uniform(-3.0, 7.0, (n_labels, e))


def graph(n=3000, m=20000, n_labels=11, seed=5):
    from gnnpe_amd import synth
    g = synth.gnm_graph(n, m, n_labels=n_labels, seed=seed)
    return g, synth.degree_order(g["offsets"])


def graph_with_hubs(seed=9):
    """G(2500, 15000) plus three vertices of degree 70, 150 and 300 (hub rows: degree > 64) wired to random ordinary vertices."""
    from gnnpe_amd import synth
    rng = np.random.default_rng(seed)
    g = synth.gnm_graph(2500, 15000, n_labels=11, seed=seed)
    n0 = g["n"]
    offs = g["offsets"].astype(np.int64)
    eu = np.repeat(np.arange(n0, dtype=np.int64), np.diff(offs))
    ev = g["nbrs"].astype(np.int64)
    keep = eu < ev
    eu, ev = eu[keep], ev[keep]
    hubs = []
    for k, d in enumerate((70, 150, 300)):
        to = rng.choice(n0, d, replace=False).astype(np.int64)
        hubs.append((to, np.full(d, n0 + k, np.int64)))
    eu = np.concatenate([eu] + [h[0] for h in hubs])
    ev = np.concatenate([ev] + [h[1] for h in hubs])
    n = n0 + 3
    o, nb = synth._csr_from_edges(n, eu, ev)
    labels = rng.integers(0, 11, n).astype(np.uint32)
    assert np.diff(o.astype(np.int64)).max() == 300
    g2 = dict(n=n, offsets=o, nbrs=nb, labels=labels)
    return g2, synth.degree_order(o)


def fresh(binding, g, sn, mem, p, table, slab=None, variant=4, parts=False):
    """What an engine that has seen nothing else computes: (total, ids, pde[, partitions])."""
    eng = binding.Engine(0)
    eng.set_fill_variant(variant)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, p)
    if slab is not None:
        eng.set_slab(*slab)
    eng.set_label_table(table)
    eng.vde(want=False)
    total = eng.count_paths(2)
    ids, pde, _ = eng.fill_paths()
    out = (total, ids, pde)
    if parts:
        out = out + (partitions(eng, total),)
    eng.close()
    return out


def partitions(eng, total):
    import torch
    part = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # (torch's stream is not the engine's: the clearing must have finished before the kernel is queued)
    eng.path_partitions_device(0, total, part)
    eng.sync()
    return part[:total].cpu().numpy()


def same(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(u64(got[2]), u64(want[2]))


def step(eng, table=None):
    if table is not None:
        eng.set_label_table(table)
    eng.vde(want=False)
    total = eng.count_paths(2)
    ids, pde, _ = eng.fill_paths()
    return total, ids, pde


@pytest.mark.parametrize("e", [1, 2, 3, 4, 8])
def test_reembedding_reuses_the_structure(binding, oracle, debug_lines, e):
    """Table A -> vde, count, fill; another table of the same width -> vde, count, fill: the second count refreshes, and its rows
    carry the second table's embeddings."""
    g, sn = graph()
    mem = np.zeros(g["n"], np.uint32)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)[2]
    tab_b = random_table(11, e, 100 + e)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    a = step(eng, binding.host_label_table(11, e))
    assert debug_lines() == ["built"]
    assert a[0] == len(ref) and np.array_equal(a[1], ref) and np.array_equal(u64(a[2]), u64(ovde[ref].reshape(len(ref), 3 * e)))
    b = step(eng, tab_b)
    assert debug_lines() == ["reused"]
    vde_b = eng.vde()[2]
    assert not np.array_equal(vde_b, ovde)
    assert np.array_equal(b[1], ref) and np.array_equal(u64(b[2]), u64(vde_b[ref].reshape(len(ref), 3 * e)))
    assert same(b, fresh(binding, g, sn, mem, 1, tab_b))
    debug_lines()
    # and back: a third table, a count that finds the records current (nothing to refresh), the same rows again
    c = step(eng, binding.host_label_table(11, e))
    assert eng.count_paths(2) == len(ref)
    assert debug_lines() == ["reused", "reused"]
    ids, pde, _ = eng.fill_paths()
    assert same(c, a) and np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(a[2]))
    eng.close()


def test_new_embeddings_between_count_and_fill(binding, oracle, debug_lines):
    """The vde table changes after the count (gnnpe_vde again, then a peer's slab unpacked over it) and no second count runs: the
    fill refreshes the records itself and its pde rows carry the table as it is now."""
    import torch
    g, sn = graph()
    n = g["n"]
    mem = np.zeros(n, np.uint32)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    eng.set_label_table(binding.host_label_table(11, 2))
    eng.vde(want=False)
    total = eng.count_paths(2)
    assert debug_lines() == ["built"]
    eng.vde(want=False)
    new = np.random.default_rng(3).normal(size=(n, 2))  # by position in the order, as vde_pack_slab lays a slab out
    new_dev = torch.from_numpy(new).to("cuda:0")
    torch.cuda.synchronize()  # (torch's stream is not the engine's)
    eng.vde_unpack_slab(0, n, new_dev)
    ids, pde, _ = eng.fill_paths()
    assert debug_lines() == ["reused"]
    now = np.empty((n, 2))
    now[sn] = new
    assert total == len(ref) and np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(now[ref].reshape(len(ref), 6)))
    eng.close()


def test_ids_only_count_before_any_vde(binding, oracle, debug_lines):
    g, sn = graph()
    mem = np.zeros(g["n"], np.uint32)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], 2)[2]
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    assert eng.count_paths(2) == len(ref)  # before any table: records of width 2 without embeddings
    assert eng.count_paths(2) == len(ref)  # nothing to refresh, nothing launched
    assert debug_lines() == ["built", "reused"]
    assert np.array_equal(eng.fill_paths(pde=False)[0], ref)
    eng.set_label_table(binding.host_label_table(11, 2))  # the width the records have: the structure stays
    eng.vde(want=False)
    assert eng.count_paths(2) == len(ref)
    assert debug_lines() == ["reused"]
    ids, pde, _ = eng.fill_paths()
    assert np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(ovde[ref].reshape(len(ref), 6)))
    # ... and the other way round: counted without embeddings, the vde table arrives before the fill
    eng2 = binding.Engine(0)
    eng2.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng2.set_order(sn, mem, 1)
    eng2.set_label_table(binding.host_label_table(11, 2))
    assert eng2.count_paths(2) == len(ref)
    eng2.vde(want=False)
    ids, pde, _ = eng2.fill_paths()
    assert debug_lines() == ["built", "reused"]
    assert np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(ovde[ref].reshape(len(ref), 6)))
    eng.close()
    eng2.close()


CHANGES = ["order", "membership", "slab", "graph", "width", "variant", "deep_count"]


@pytest.mark.parametrize("change", CHANGES)
def test_a_changed_input_rebuilds_the_structure(binding, debug_lines, change):
    """Between two counts one of the structure's inputs changes: the second count builds again and gives what a fresh engine gives
    for the final inputs; the count after it reuses again."""
    from gnnpe_amd import synth
    g, sn = graph()
    n = g["n"]
    mem, p = synth.block_membership(n, 3), 3
    table = binding.host_label_table(11, 2)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, p)
    first = step(eng, table)
    assert step(eng)[0] == first[0]
    assert debug_lines() == ["built", "reused"]
    slab, expect = None, ["built"]
    if change == "order":
        sn = np.random.default_rng(1).permutation(n).astype(np.uint32)
        eng.set_order(sn, mem, p)
    elif change == "membership":
        mem, p = (np.arange(n) % 5).astype(np.uint32), 5
        eng.set_order(sn, mem, p)
    elif change == "slab":
        slab = (200, 2500)
        eng.set_slab(*slab)
    elif change == "graph":
        g, sn = graph(2800, 23000, seed=6)
        mem = synth.block_membership(g["n"], 3)
        eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
        eng.set_order(sn, mem, p)
        eng.set_label_table(table)
    elif change == "width":
        table = binding.host_label_table(11, 3)
        eng.set_label_table(table)
    elif change == "variant":
        eng.set_fill_variant(1)
        assert step(eng)[0] == first[0]
        eng.set_fill_variant(4)
        expect = ["built"]  # (the pair-wave count prints nothing: it has no structure of this kind)
    elif change == "deep_count":
        assert eng.count_paths(3) > first[0]
    got = step(eng)
    assert debug_lines() == expect
    want = fresh(binding, g, sn, mem, p, table, slab=slab, parts=True)
    assert same(got, want) and np.array_equal(partitions(eng, got[0]), want[3])
    debug_lines()  # (the fresh engine's own `built`)
    # the structure of the new inputs serves the next embedding
    tab2 = random_table(11, table.shape[1], 7)
    got2 = step(eng, tab2)
    assert debug_lines() == ["reused"]
    want2 = fresh(binding, g, sn, mem, p, tab2, slab=slab, parts=True)
    assert same(got2, want2) and np.array_equal(partitions(eng, got2[0]), want2[3])
    eng.close()


def test_rows_appended_and_dropped_rebuild_the_structure(binding, oracle, debug_lines):
    """Two slab contexts on one device (load_rows + halo rows through the C-ABI helpers, as the multi-GPU path drives them): a count
    with the halo in place builds, the next embedding reuses; dropping the halo and appending it again (truncated this time) builds
    again.  The concatenated rows are the oracle's every time."""
    import torch
    from gnnpe_amd import synth
    g, sn = graph(3000, 20000, n_labels=13, seed=77)
    n = g["n"]
    mem = synth.block_membership(n, 3)
    ref_ids = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    bounds = np.array([0, 1700, n], np.uint32)
    dev = torch.device("cuda:0")
    offs = g["offsets"].astype(np.int64)
    tables = [binding.host_label_table(13, 2), random_table(13, 2, 21), random_table(13, 2, 22), random_table(13, 2, 23)]
    engs = []
    for r in range(2):
        rows = sn[bounds[r]:bounds[r + 1]]
        deg = offs[rows + 1] - offs[rows]
        roff = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
        rn = np.concatenate([g["nbrs"][offs[v]:offs[v + 1]] for v in rows])
        eng = binding.Engine(0)
        eng.load_rows(n, g["labels"], rows, roff, rn, nbr_capacity=2 * len(g["nbrs"]))
        eng.set_order(sn, mem, 3)
        eng.set_slab(int(bounds[r]), int(bounds[r + 1]))
        engs.append(eng)

    def exchange_halo(min_rank):
        for r in range(2):
            engs[r].rows_drop_halo()
        for r in range(2):
            o = 1 - r
            need = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            k = int(engs[r].halo_need(bounds, need, n)[o])
            ids = need[:k]
            degs = torch.zeros(k, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            engs[o].rows_degree(k, ids, degs)
            engs[o].sync()
            tot = int(degs.long().sum())
            nb = torch.zeros(max(tot, 1), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            engs[o].rows_pack(k, ids, nb, tot)
            engs[o].sync()
            engs[r].rows_append(k, ids, degs, nb, tot, int(bounds[r]) if min_rank else 0)

    def both_steps(table):
        """vde of the own rows, the peers' halves exchanged, count, fill; returns the concatenated rows and the full vde table"""
        for r in range(2):
            engs[r].set_label_table(table)
            engs[r].vde(want=False)
        bufs = []
        for r in range(2):
            buf = torch.zeros((int(bounds[r + 1] - bounds[r]), 2), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            engs[r].vde_pack_slab(int(bounds[r]), int(bounds[r + 1]), buf)
            engs[r].sync()
            bufs.append(buf)
        for r in range(2):
            engs[r].vde_unpack_slab(int(bounds[1 - r]), int(bounds[2 - r]), bufs[1 - r])
        out_ids, out_pde = [], []
        for r in range(2):
            total = engs[r].count_paths(2)
            i, q, _ = engs[r].fill_paths(0, total)
            out_ids.append(i)
            out_pde.append(q)
        vde = np.empty((n, 2))
        vde[sn] = np.concatenate([b.cpu().numpy() for b in bufs])
        return np.concatenate(out_ids), np.concatenate(out_pde), vde

    def check(table, expect):
        debug_lines()
        ids, pde, vde = both_steps(table)
        assert debug_lines() == expect
        assert np.array_equal(ids, ref_ids) and np.array_equal(u64(pde), u64(vde[ref_ids].reshape(len(ref_ids), 6)))

    exchange_halo(False)
    check(tables[0], ["built", "built"])
    check(tables[1], ["reused", "reused"])
    exchange_halo(True)  # dropped, appended again without the entries ranked before the slab
    check(tables[2], ["built", "built"])
    check(tables[3], ["reused", "reused"])
    for r in range(2):  # the halo dropped and nothing appended: the structure of the rows that are left is another one
        engs[r].rows_drop_halo()
        engs[r].vde(want=False)
    debug_lines()
    t0 = engs[0].count_paths(2)
    assert debug_lines() == ["built"] and 0 < t0 < len(ref_ids)
    for e in engs:
        e.close()


def test_hub_rows_are_refreshed_with_the_ordinary_rows(binding, oracle):
    g, sn = graph_with_hubs()
    mem = np.zeros(g["n"], np.uint32)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], 2)[2]
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    a = step(eng, binding.host_label_table(11, 2))
    assert a[0] == len(ref) and np.array_equal(a[1], ref) and np.array_equal(u64(a[2]), u64(ovde[ref].reshape(len(ref), 6)))
    for seed in (31, 32):
        tab = random_table(11, 2, seed)
        b = step(eng, tab)
        assert same(b, fresh(binding, g, sn, mem, 1, tab)) and np.array_equal(b[1], ref)
    total, per_start = eng.count_paths(2, per_start=True)  # (the per-pair offsets are built on demand, also over a reused structure)
    assert total == len(ref) and int(per_start.sum()) == total
    eng.close()


def test_hub_rows_decisions(binding, debug_lines):
    """The sequence of decisions on a graph with hub rows (fresh engines in between print their own `built`)."""
    g, sn = graph_with_hubs()
    mem = np.zeros(g["n"], np.uint32)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    first = step(eng, binding.host_label_table(11, 2))
    again = step(eng, random_table(11, 2, 1))
    back = step(eng, binding.host_label_table(11, 2))
    assert debug_lines() == ["built", "reused", "reused"]
    assert same(back, first) and again[0] == first[0] and not np.array_equal(again[2], first[2])
    eng.close()


def test_wide_records_are_refreshed(binding, oracle, debug_lines):
    """Beyond 2^26 vertices the records are {id, id-position, vde}: the wide instantiation of the refresh kernel (the construction of
    tests/test_gpu_parity.py's wide-record test)."""
    from gnnpe_amd import synth
    avail = [int(ln.split()[1]) >> 20 for ln in open("/proc/meminfo") if ln.startswith("MemAvailable:")][0]
    if avail < 32:
        pytest.skip(f"{avail} GiB of host memory available, 32 needed")
    n = (1 << 26) + 4099
    rng = np.random.default_rng(26)
    verts = np.unique(np.concatenate([rng.integers(0, n, 1500), np.arange(n - 60, n), np.arange(0, 60)])).astype(np.int64)
    a, b = verts[rng.integers(0, len(verts), 9000)], verts[rng.integers(0, len(verts), 9000)]
    keep = a != b
    eu, ev = np.minimum(a[keep], b[keep]), np.maximum(a[keep], b[keep])
    uniq = np.unique(eu * n + ev)
    eu, ev = uniq // n, uniq % n
    offs, nbrs = synth._csr_from_edges(n, eu, ev)
    labels = rng.integers(0, 5, n).astype(np.uint32)
    assert int(nbrs.max()) > (1 << 26) and np.diff(offs.astype(np.int64)).max() <= 64
    sn = np.arange(n, dtype=np.uint32)[::-1].copy()
    mem = np.zeros(n, np.uint32)
    g = dict(n=n, offsets=offs, nbrs=nbrs, labels=labels)
    want = oracle.enumerate_closed(offs, nbrs, sn, 3)
    eng = binding.Engine(0)
    eng.load_csr(offs, nbrs, labels)
    eng.set_order(sn, mem, 1)
    first = step(eng, binding.host_label_table(5, 2))
    tab = random_table(5, 2, 26)
    got = step(eng, tab)
    assert debug_lines() == ["built", "reused"]
    vde = eng.vde()[2]
    eng.close()
    assert first[0] == len(want) and np.array_equal(first[1], want) and np.array_equal(got[1], want)
    assert np.array_equal(u64(got[2]), u64(vde[want].reshape(len(want), 6))) and not np.array_equal(got[2], first[2])
    assert same(got, fresh(binding, g, sn, mem, 1, tab))


@pytest.mark.parametrize("shape", [1, 4, 2])
def test_enqueued_steps_and_the_resident_emit_shape(binding, oracle, debug_lines, shape):
    """The benchmark's call sequence -- vde, enqueue-only count, capped fill, the total read at the end -- over several steps with
    another table each; shape 4 (the resident grid) takes its start vertices from ticket heads that the refresh kernel has to leave
    zero, as k_start_scan does in a full count."""
    import torch
    g, sn = graph(20000, 160000, seed=12)
    mem = np.zeros(g["n"], np.uint32)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    P = len(ref)
    dev = torch.device("cuda:0")
    ref_t = torch.from_numpy(ref.view(np.int32)).to(dev)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    eng.set_emit_shape(shape)
    cap = P + 9
    ids = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
    pde = torch.zeros((cap, 6), dtype=torch.float64, device=dev)
    for k in range(4):
        eng.set_label_table(random_table(11, 2, 40 + k))
        ids.zero_()
        pde.fill_(-1.0)
        torch.cuda.synchronize()
        eng.vde(want=False)
        eng.count_paths_enqueue(2)
        eng.fill_paths_capped_device(cap, ids, pde)
        eng.sync()
        assert eng.emit_kernel_name() == eng.EMIT_SHAPE_KERNELS[shape]
        assert eng.count_total() == P
        vde = torch.from_numpy(eng.vde()[2]).to(dev)
        # (that vde call made the records stale again: the next step refreshes whatever the table)
        assert torch.equal(ids[:P], ref_t) and bool((ids[P:] == 0).all()) and bool((pde[P:] == -1.0).all())
        assert torch.equal(pde[:P].view(torch.int64), vde[ref_t.long().reshape(-1)].reshape(P, 6).view(torch.int64))
    assert debug_lines() == ["built", "reused", "reused", "reused"]
    # two fills of one refresh step into the resident shape: the second finds the heads used and clears them itself
    eng.vde(want=False)
    eng.count_paths_enqueue(2)
    for _ in range(2):
        ids.zero_()
        torch.cuda.synchronize()
        eng.fill_paths_capped_device(cap, ids, pde)
        eng.sync()
        assert torch.equal(ids[:P], ref_t)
    eng.close()


def test_index_after_a_refresh_is_the_fresh_engines(binding, debug_lines):
    """The partition index carries the embeddings (leaf points, sort keys): built after a refresh step it must be the image a fresh
    engine builds for the second table, not one served from the pair order of the first."""
    from gnnpe_amd import synth
    g, sn = graph(4000, 30000, seed=14)
    mem, p = synth.block_membership(g["n"], 2), 2
    tab_a, tab_b = binding.host_label_table(11, 2), random_table(11, 2, 50)

    def images(eng):
        out = []
        for pid in range(p):
            img, nbytes, hdr = eng.build_index_partition_device(pid)
            out.append(eng.copy_to_host(img, nbytes).tobytes())
        return out

    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, p)
    step(eng, tab_a)
    img_a = images(eng)
    step(eng, tab_b)
    assert debug_lines() == ["built", "reused"]
    img_b = images(eng)
    eng.close()
    new = binding.Engine(0)
    new.load_csr(g["offsets"], g["nbrs"], g["labels"])
    new.set_order(sn, mem, p)
    step(new, tab_b)
    want_b = images(new)
    new.close()
    assert img_b == want_b and img_a != img_b


def test_decisions_of_a_step_loop_in_a_child_process():
    """The same through a process of its own, the way the launches of a step are pinned elsewhere: the first count builds, every later
    one on the same graph / order / slab reuses, a new slab builds once."""
    from conftest import ROOT
    code = (
        "import numpy as np, torch, gnnpe_amd\n"
        "from gnnpe_amd import binding, synth\n"
        "g = synth.gnm_graph(5000, 40000, n_labels=8, seed=4)\n"
        "eng = binding.Engine(0)\n"
        "eng.load_csr(g['offsets'], g['nbrs'], g['labels']); eng.set_order(synth.degree_order(g['offsets']), np.zeros(5000, np.uint32), 1)\n"
        "eng.set_label_table(binding.host_label_table(8, 2))\n"
        "tot = []\n"
        "for step in range(3):\n"
        "    eng.vde(want=False); tot.append(eng.count_paths(2)); ids, pde, _ = eng.fill_paths()\n"
        "x, nx, vde = eng.vde()\n"
        "assert len(set(tot)) == 1 and np.array_equal(pde, vde[ids].reshape(len(ids), 6))\n"
        "eng.set_slab(100, 4000); eng.vde(want=False); eng.count_paths(2)\n"
        "eng.vde(want=False); eng.count_paths(2)\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, GNNPE_DEBUG="1"), cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    how = [ln.split(": ")[1] for ln in r.stderr.splitlines() if ln.startswith("[count] structure")]
    assert how == ["built", "reused", "reused", "built", "reused"], how
