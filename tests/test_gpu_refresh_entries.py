"""The embedding refresh of a count whose structure is reused (k_rows_refresh) gathers from the compact vde table, and a refresh
no longer packs the per-vertex records {vde, rank, pair offset} that only the full count and the hub rows read.  Every case has
one form: table A -> vde, count, fill; table B -> vde, count (the refresh), fill; the rows of B compared bit for bit with a FRESH engine
that does a full count under B, and with the oracle (its enumeration, and its gen_pde over embeddings summed on the host in the
reference's operation order).  The library's `[count] structure: built | reused` and `[count] vertex records: ...` lines
(GNNPE_DEBUG=1) say which path a count took.  The shapes are the ones at which a refresh kernel can go wrong, whatever drives it:
entry counts around 64, 256 and 1024 (a wave's lanes, a workgroup's, four instructions of one), rows that start on the last lane of
such a unit, rows without entries, hub rows beside ordinary ones, every record width, rows that are not held.  (They were written
against an entry-driven refresh, one lane per adjacency entry, that was measured and not kept -- profiles/refresh_entries.txt -- and
hold for any shape of the kernel.)"""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WG_ITEMS = 1024  # four 64-lane instructions for each of a workgroup's four waves


@pytest.fixture(scope="module")
def binding():
    from gnnpe_amd import binding as b
    b.load()
    return b


@pytest.fixture()
def debug_lines(monkeypatch, capfd):
    """Contexts created while this fixture is active print their launch decisions; the returned callable gives the decisions of one
    kind (`structure`, `vertex records`) since it was last asked for that kind."""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()
    seen, cursor = [], {}

    def take(kind="structure"):
        sys.stderr.flush()
        seen.extend(capfd.readouterr().err.splitlines())
        out = [ln.split(": ")[1] for ln in seen if ln.startswith("[count] " + kind + ":")]
        first = cursor.get(kind, 0)
        cursor[kind] = len(out)
        return out[first:]
    return take


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_table(n_labels, e, seed):
    return np.random.default_rng(seed).uniform(-3.0, 7.0, (n_labels, e))


def host_vde(g, table):
    """x and vde as gen_vde computes them (custom.h:513-544): x = the label's row, vde = x + the neighbours' rows added one after the
    other in ascending-neighbour order."""
    offs, nbrs, labels = g["offsets"].astype(np.int64), g["nbrs"], g["labels"]
    x = table[labels]
    vde = np.empty_like(x)
    for v in range(len(labels)):
        acc = np.zeros(table.shape[1])
        for u in nbrs[offs[v]:offs[v + 1]]:
            acc = acc + table[labels[u]]
        vde[v] = x[v] + acc
    return x, vde


def from_edges(n, edges, n_labels=7, seed=1):
    from gnnpe_amd import synth
    e = np.array(sorted({(min(a, b), max(a, b)) for a, b in edges}), np.int64).reshape(-1, 2)
    offs, nbrs = synth._csr_from_edges(n, e[:, 0], e[:, 1])
    labels = np.random.default_rng(seed).integers(0, n_labels, n).astype(np.uint32)
    return dict(n=n, offsets=offs, nbrs=nbrs, labels=labels)


def step(eng, table=None):
    if table is not None:
        eng.set_label_table(table)
    eng.vde(want=False)
    total = eng.count_paths(2)
    ids, pde, _ = eng.fill_paths()
    return total, ids, pde


def fresh(binding, g, sn, table, slab=None, mem=None, p=1):
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, np.zeros(g["n"], np.uint32) if mem is None else mem, p)
    if slab is not None:
        eng.set_slab(*slab)
    out = step(eng, table)
    eng.close()
    return out


def same(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(u64(got[2]), u64(want[2]))


def oracle_rows(oracle, g, sn, table):
    e = table.shape[1]
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    x, vde = host_vde(g, table)
    pde = oracle.gen_pde(ref, e, g["offsets"], g["labels"], x, vde)[0] if len(ref) else np.zeros((0, 3 * e))
    return len(ref), ref, pde


def a_then_b(binding, oracle, debug_lines, g, sn, e=2, tables=None):
    """The common form, on the whole graph (load_csr).  Returns the engine after the last table's step and, per refresh step, what
    became of the per-vertex records."""
    n_labels = int(g["labels"].max()) + 1
    tables = tables or [binding.host_label_table(n_labels, e), random_table(n_labels, e, 10 + e)]
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
    vinfo = []
    for k, tab in enumerate(tables):
        for kind in ("structure", "vertex records"):
            debug_lines(kind)  # (what fresh engines printed)
        got = step(eng, tab)
        assert debug_lines() == (["reused"] if k else ["built"])
        if k:
            vinfo += debug_lines("vertex records")
        assert same(got, oracle_rows(oracle, g, sn, tab)), f"table {k}: rows differ from the oracle"
        if k:
            assert same(got, fresh(binding, g, sn, tab)), f"table {k}: rows differ from a fresh engine's"
    for kind in ("structure", "vertex records"):
        debug_lines(kind)
    return eng, vinfo


# ---- entry counts against the lane, wave and workgroup granularity ----------------------------------------------------------

ENTRY_COUNTS = [1, 63, 64, 65, 255, 256, 257, WG_ITEMS - 1, WG_ITEMS, WG_ITEMS + 1]


def stars_with_entries(total):
    """Disjoint stars of up to 40 leaves and a list of HELD rows with exactly `total` stored entries: every centre's row, then leaf rows
    one by one (one entry each).  Isolated vertices (rows without entries) come first, last and between the others."""
    edges, held, left, n = [], [], total, 0
    while left:
        d = min(40, left)
        c = n
        leaves = list(range(n + 1, n + 1 + d))
        n += d + 1
        edges += [(c, u) for u in leaves]
        held.append(c)
        left -= d
        take = min(left, d)
        held += leaves[:take]
        left -= take
    iso = list(range(n, n + len(held) // 3 + 2))
    n += len(iso)
    rows = [iso[0]]
    for k, v in enumerate(held):
        rows.append(v)
        if k % 3 == 2:
            rows.append(iso[1 + k // 3])
    rows.append(iso[-1])
    return from_edges(n, edges), np.array(rows, np.uint32)


def rows_engine(binding, g, rows, sn, slab=None):
    offs = g["offsets"].astype(np.int64)
    deg = offs[rows.astype(np.int64) + 1] - offs[rows.astype(np.int64)]
    roff = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    rn = np.concatenate([g["nbrs"][offs[v]:offs[v + 1]] for v in rows] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    eng = binding.Engine(0)
    eng.load_rows(g["n"], g["labels"], rows, roff, rn)
    eng.set_order(sn, np.zeros(g["n"], np.uint32), 1)
    if slab is not None:
        eng.set_slab(*slab)
    return eng, int(roff[-1])


def rows_step(eng, n, sn, table, vde_seed):
    """vde of the held rows, then EVERY vertex's embedding given (as a peer's slab arrives: by position in the order), count, fill.
    Returns the rows and the table as the engine now has it, by vertex."""
    import torch
    eng.set_label_table(table)
    eng.vde(want=False)
    new = np.random.default_rng(vde_seed).normal(size=(n, table.shape[1]))
    dev = torch.from_numpy(new).to("cuda:0")
    torch.cuda.synchronize()  # (torch's stream is not the engine's)
    eng.vde_unpack_slab(0, n, dev)
    total = eng.count_paths(2)
    ids, pde, _ = eng.fill_paths()
    now = np.empty_like(new)
    now[sn] = new
    return (total, ids, pde), now


@pytest.mark.parametrize("total", ENTRY_COUNTS)
def test_entry_counts_around_the_granularity(binding, debug_lines, total):
    from gnnpe_amd import synth
    g, rows = stars_with_entries(total)
    n, sn = g["n"], synth.degree_order(g["offsets"])
    tab_a, tab_b = binding.host_label_table(7, 2), random_table(7, 2, 3)
    eng, used = rows_engine(binding, g, rows, sn)
    assert used == total
    a, _ = rows_step(eng, n, sn, tab_a, 1)
    b, now = rows_step(eng, n, sn, tab_b, 2)
    assert debug_lines() == ["built", "reused"]
    eng.close()
    new, used = rows_engine(binding, g, rows, sn)
    want, _ = rows_step(new, n, sn, tab_b, 2)
    new.close()
    assert (b[0] > 0) == (total > 2)  # (a held leaf and another leaf of its centre: a path)
    assert same(b, want) and np.array_equal(a[1], b[1])
    assert np.array_equal(u64(b[2]), u64(now[b[1].astype(np.int64)].reshape(b[0], 6)))


@pytest.mark.parametrize("m", [32, 128, WG_ITEMS // 2])
def test_whole_graph_with_exactly_full_waves(binding, oracle, debug_lines, m):
    """Identity rows: a path of m edges (2m entries: 64, 256, 1024) between isolated vertices."""
    from gnnpe_amd import synth
    edges = [(3 + i, 4 + i) for i in range(m)]
    g = from_edges(m + 7, edges)
    assert len(g["nbrs"]) == 2 * m
    a_then_b(binding, oracle, debug_lines, g, synth.degree_order(g["offsets"]))[0].close()


@pytest.mark.parametrize("n", [3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_row_counts_around_the_rows_per_wave_and_workgroup(binding, oracle, debug_lines, n):
    """k_rows_refresh takes four rows per wave, sixteen per workgroup: a cycle of n vertices (every row two entries) ends a wave or a
    workgroup early, exactly, or one row into the next."""
    from gnnpe_amd import synth
    g = from_edges(n, [(i, (i + 1) % n) for i in range(n)])
    a_then_b(binding, oracle, debug_lines, g, synth.degree_order(g["offsets"]))[0].close()


# ---- rows that straddle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [63, 255, WG_ITEMS - 1, 2 * WG_ITEMS - 1])
def test_a_full_row_that_starts_on_the_last_lane(binding, oracle, debug_lines, first):
    """A row of degree 64 whose first entry is entry `first`, the last before a multiple of 64, 256 and 1024.  In front of it
    a path ((first - 1) entries) and one vertex tied to a vertex behind it; the row's 64 neighbours are tied among themselves so that
    its records are read in many pairs."""
    from gnnpe_amd import synth
    pe = (first - 1) // 2  # edges of the path in front: vertices 0 .. pe
    edges = [(i, i + 1) for i in range(pe)]
    x, h = pe + 1, pe + 2
    leaves = list(range(h + 1, h + 65))
    edges += [(x, leaves[-1])] + [(h, u) for u in leaves] + [(leaves[i], leaves[i + 1]) for i in range(0, 62, 3)]
    g = from_edges(leaves[-1] + 1, edges)
    offs = g["offsets"].astype(np.int64)
    assert offs[h] == first and offs[h + 1] - offs[h] == 64
    a_then_b(binding, oracle, debug_lines, g, synth.degree_order(g["offsets"]))[0].close()


@pytest.mark.parametrize("run", [256, WG_ITEMS])
def test_a_run_of_single_entry_rows_ends_on_a_boundary(binding, oracle, debug_lines, run):
    """Vertices 0 .. run-1 are leaves (one entry each), four to a centre; the centres' rows follow from entry `run` on."""
    from gnnpe_amd import synth
    edges = [(u, run + u // 4) for u in range(run)]
    g = from_edges(run + run // 4, edges)
    offs = g["offsets"].astype(np.int64)
    assert offs[run] == run and np.all(np.diff(offs[:run + 1]) == 1)
    a_then_b(binding, oracle, debug_lines, g, synth.degree_order(g["offsets"]))[0].close()


def test_rows_without_entries_first_last_and_between(binding, oracle, debug_lines):
    from gnnpe_amd import synth
    edges = []
    for c in range(2, 600, 6):  # vertices c .. c+3 a star round c, c+4 and c+5 isolated; 0, 1 and the last two isolated as well
        edges += [(c, c + 1), (c, c + 2), (c, c + 3), (c + 1, c + 2)]
    g = from_edges(604, edges)
    deg = np.diff(g["offsets"].astype(np.int64))
    assert deg[0] == deg[1] == deg[-1] == deg[-2] == 0 and (deg == 0).sum() > 200
    a_then_b(binding, oracle, debug_lines, g, synth.degree_order(g["offsets"]))[0].close()


# ---- the hub boundary --------------------------------------------------------------------------------------------------------

def graph_around_the_hub_degree(seed=19):
    """G(1500, 6000) plus four vertices of degree 63, 64, 65 and 168, tied to random ordinary vertices and to each other: hub rows
    (degree > 64) with ordinary neighbours, ordinary rows with hub neighbours."""
    from gnnpe_amd import synth
    rng = np.random.default_rng(seed)
    base = synth.gnm_graph(1500, 6000, n_labels=7, seed=seed)
    n0 = base["n"]
    offs = base["offsets"].astype(np.int64)
    eu = np.repeat(np.arange(n0, dtype=np.int64), np.diff(offs))
    edges = [(int(a), int(b)) for a, b in zip(eu, base["nbrs"]) if a < b]
    special = [n0, n0 + 1, n0 + 2, n0 + 3]
    edges += [(special[i], special[j]) for i in range(4) for j in range(i + 1, 4)]
    for v, d in zip(special, (63, 64, 65, 168)):
        edges += [(int(u), v) for u in rng.choice(n0, d - 3, replace=False)]
    g = from_edges(n0 + 4, edges, seed=seed)
    deg = np.diff(g["offsets"].astype(np.int64))
    assert list(deg[n0:]) == [63, 64, 65, 168] and deg[:n0].max() < 63
    return g


def test_rows_on_both_sides_of_the_hub_degree(binding, oracle, debug_lines):
    from gnnpe_amd import synth
    g = graph_around_the_hub_degree()
    sn = synth.degree_order(g["offsets"])
    tabs = [binding.host_label_table(7, 2), random_table(7, 2, 5), random_table(7, 2, 6)]
    eng, vinfo = a_then_b(binding, oracle, debug_lines, g, sn, tables=tabs)
    assert vinfo == ["k_pack_vinfo", "k_pack_vinfo"]  # (k_hub_records reads them: packed on every step)
    eng.close()


# ---- record widths, twice, stale records at the fill -------------------------------------------------------------------------

@pytest.mark.parametrize("e", [1, 2, 3, 4, 8])
def test_every_record_width_refreshed_twice(binding, oracle, debug_lines, e):
    """Records of 12, 20, 28, 36 and 68 bytes: they cross the 128-byte lines at every phase, and the doubles sit on 4-byte alignment.
    A -> B -> C: the second refresh runs over refreshed records."""
    from gnnpe_amd import synth
    g = synth.gnm_graph(700, 4100, n_labels=7, seed=40 + e)
    g = dict(n=g["n"], offsets=g["offsets"], nbrs=g["nbrs"], labels=g["labels"])
    sn = synth.degree_order(g["offsets"])
    tabs = [binding.host_label_table(7, e), random_table(7, e, 50 + e), random_table(7, e, 60 + e)]
    eng, vinfo = a_then_b(binding, oracle, debug_lines, g, sn, e=e, tables=tabs)
    assert "k_pack_vinfo" not in vinfo and len(vinfo) == 2  # (written by k_vde in passing where it can, else not needed)
    eng.close()


def test_new_embeddings_between_count_and_fill(binding, oracle, debug_lines):
    """The count refreshes under table B; then other embeddings arrive (gnnpe_vde again, a peer's slab unpacked over it) and no count
    runs: the fill finds the records stale and refreshes them itself."""
    import torch
    from gnnpe_amd import synth
    g = synth.gnm_graph(700, 4100, n_labels=7, seed=71)
    n, sn = g["n"], synth.degree_order(g["offsets"])
    tab_b = random_table(7, 2, 72)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, np.zeros(n, np.uint32), 1)
    step(eng, binding.host_label_table(7, 2))
    eng.set_label_table(tab_b)
    eng.vde(want=False)
    total = eng.count_paths(2)
    eng.vde(want=False)
    new = np.random.default_rng(73).normal(size=(n, 2))  # by position in the order, as vde_pack_slab lays a slab out
    new_dev = torch.from_numpy(new).to("cuda:0")
    torch.cuda.synchronize()  # (torch's stream is not the engine's)
    eng.vde_unpack_slab(0, n, new_dev)
    ids, pde, _ = eng.fill_paths()
    assert debug_lines() == ["built", "reused", "reused"]
    eng.close()
    now = np.empty((n, 2))
    now[sn] = new
    assert total == len(ref) and np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(now[ref].reshape(len(ref), 6)))
    assert np.array_equal(ids, fresh(binding, g, sn, tab_b)[1])


# ---- rows that are not held ---------------------------------------------------------------------------------------------------

def test_a_slab_narrower_than_the_graph(binding, debug_lines):
    from gnnpe_amd import synth
    g = synth.gnm_graph(900, 5000, n_labels=7, seed=81)
    sn = synth.degree_order(g["offsets"])
    mem = synth.block_membership(g["n"], 3)
    tab_b = random_table(7, 2, 82)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 3)
    eng.set_slab(130, 700)
    a = step(eng, binding.host_label_table(7, 2))
    b = step(eng, tab_b)
    assert debug_lines() == ["built", "reused"]
    eng.close()
    assert 0 < b[0] == a[0] and same(b, fresh(binding, g, sn, tab_b, slab=(130, 700), mem=mem, p=3))


def test_slab_rows_with_halo_rows(binding, oracle, debug_lines):
    """Two slab contexts on one device as the multi-GPU path drives them: the slab's own rows (load_rows) and the halo rows appended,
    truncated to the entries ranked from the slab on.  Rows that are not held have no block and must never be written through.
    The concatenated rows are the oracle's after every table, and a fresh pair of engines gives the same per slab."""
    import torch
    from gnnpe_amd import synth
    g = synth.gnm_graph(1200, 7000, n_labels=7, seed=91)
    n, sn = g["n"], synth.degree_order(g["offsets"])
    mem = synth.block_membership(n, 2)
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    bounds = np.array([0, 700, n], np.uint32)
    dev = torch.device("cuda:0")
    offs = g["offsets"].astype(np.int64)

    def make():
        engs = []
        for r in range(2):
            rows = sn[bounds[r]:bounds[r + 1]]
            deg = offs[rows + 1] - offs[rows]
            roff = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
            rn = np.concatenate([g["nbrs"][offs[v]:offs[v + 1]] for v in rows])
            eng = binding.Engine(0)
            eng.load_rows(n, g["labels"], rows, roff, rn, nbr_capacity=2 * len(g["nbrs"]))
            eng.set_order(sn, mem, 2)
            eng.set_slab(int(bounds[r]), int(bounds[r + 1]))
            engs.append(eng)
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
            engs[r].rows_append(k, ids, degs, nb, tot, int(bounds[r]))
        return engs

    def both_steps(engs, table):
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
        out = []
        for r in range(2):
            total = engs[r].count_paths(2)
            i, q, _ = engs[r].fill_paths(0, total)
            out.append((total, i, q))
        return out

    tabs = [binding.host_label_table(7, 2), random_table(7, 2, 92), random_table(7, 2, 93)]
    engs = make()
    for k, tab in enumerate(tabs):
        debug_lines()
        got = both_steps(engs, tab)
        assert debug_lines() == (["reused", "reused"] if k else ["built", "built"])
        ids, pde = np.concatenate([o[1] for o in got]), np.concatenate([o[2] for o in got])
        _, vde = host_vde(g, tab)
        assert np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(vde[ref].reshape(len(ref), 6)))
    for eng in engs:
        eng.close()
    new = make()
    want = both_steps(new, tabs[-1])
    for eng in new:
        eng.close()
    assert all(same(got[r], want[r]) and got[r][0] > 0 for r in range(2))


# ---- wide records --------------------------------------------------------------------------------------------------------------

def test_wide_records_refreshed_from_the_compact_table(binding, oracle, debug_lines):
    """Beyond 2^26 vertices the records are {id, id-position, vde} (the construction of tests/test_gpu_count_reuse.py's wide-record
    test): the wide instantiation of the refresh kernel, bit-equal with its gathers coming from the compact vde table."""
    from gnnpe_amd import synth
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
    g = dict(n=n, offsets=offs, nbrs=nbrs, labels=labels)
    want = oracle.enumerate_closed(offs, nbrs, sn, 3)
    eng = binding.Engine(0)
    eng.load_csr(offs, nbrs, labels)
    eng.set_order(sn, np.zeros(n, np.uint32), 1)
    first = step(eng, binding.host_label_table(5, 2))
    tab = random_table(5, 2, 26)
    got = step(eng, tab)
    assert debug_lines() == ["built", "reused"]
    vde = eng.vde()[2]
    eng.close()
    assert first[0] == len(want) and np.array_equal(first[1], want) and np.array_equal(got[1], want)
    assert np.array_equal(u64(got[2]), u64(vde[want].reshape(len(want), 6))) and not np.array_equal(got[2], first[2])
    assert same(got, fresh(binding, g, sn, tab))


# ---- per-vertex records only when somebody reads them ---------------------------------------------------------------------------

def test_a_full_count_after_a_refresh_that_packed_no_vertex_records(binding, oracle, debug_lines):
    """Embeddings that arrive after gnnpe_vde (a peer's slab unpacked) make k_vde's per-vertex records stale; the refresh does not
    need them and packs none.  Then the order changes, which invalidates the structure: the full count that follows must pack them
    for the NEW order and the embeddings as they are, not find the stale ones."""
    import torch
    from gnnpe_amd import synth
    g = synth.gnm_graph(900, 5000, n_labels=7, seed=95)
    n, sn = g["n"], synth.degree_order(g["offsets"])
    mem = np.zeros(n, np.uint32)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, 1)
    first = step(eng, binding.host_label_table(7, 2))
    ref = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    eng.vde(want=False)
    new = np.random.default_rng(96).normal(size=(n, 2))  # by position in the order, as vde_pack_slab lays a slab out
    new_dev = torch.from_numpy(new).to("cuda:0")
    torch.cuda.synchronize()  # (torch's stream is not the engine's)
    eng.vde_unpack_slab(0, n, new_dev)
    total = eng.count_paths(2)
    ids, pde, _ = eng.fill_paths()
    assert debug_lines() == ["built", "reused"] and debug_lines("vertex records")[-1] == "not needed"
    now = np.empty((n, 2))
    now[sn] = new
    assert total == first[0] == len(ref) and np.array_equal(ids, ref) and np.array_equal(u64(pde), u64(now[ref].reshape(len(ref), 6)))
    # another order, no new vde: a full count over the embeddings as they are
    sn2 = np.random.default_rng(98).permutation(n).astype(np.uint32)
    ref2 = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn2, 3)
    eng.set_order(sn2, mem, 1)
    total = eng.count_paths(2)
    ids, pde, _ = eng.fill_paths()
    assert debug_lines() == ["built"] and debug_lines("vertex records") == ["k_pack_vinfo"]
    assert total == len(ref2) and np.array_equal(ids, ref2) and np.array_equal(u64(pde), u64(now[ref2].reshape(len(ref2), 6)))
    # ... and the structure of the new order serves the next table
    tab = random_table(7, 2, 100)
    again = step(eng, tab)
    assert debug_lines() == ["reused"] and same(again, oracle_rows(oracle, g, sn2, tab)) and same(again, fresh(binding, g, sn2, tab))
    eng.close()
