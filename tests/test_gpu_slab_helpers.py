"""The C-ABI helpers of the slab halo and embedding exchange (gnnpe_halo_need, gnnpe_rows_degree / _pack / _append /
_drop_halo, gnnpe_vde_pack_slab / _unpack_slab / _unpack_all, gnnpe_count_paths_enqueue + gnnpe_count_total_device),
each held to the numpy model of tests/slab_support.py -- never to another helper.

One context at a time plays one rank; the model plays its peers.  Every device buffer is longer than the capacity the
call is told, with a sentinel tail that must stay untouched.  All comparisons are exact.  Context streams do not
block on torch's: torch.cuda.synchronize() follows every fill, eng.sync() precedes every read."""
import re

import numpy as np
import pytest
import torch

import slab_support as ss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x5A5A5A5A          # int32 sentinel of the guarded buffers (no vertex id, degree or entry of these graphs)
SENT_F = -6.02214076e23    # float64 sentinel: padding rows and guard tails
POISON_F = 2.718281828e200 # float64 poison: the rank's own block of an all-gathered table, which must not be read
ES = (1, 2, 3, 8)
CASES = ["R1", "R2", "R3_empty_middle", "R5_empty_ends", "R64", "R64_small"]


@pytest.fixture(scope="module")
def binding():
    from gnnpe_amd import binding as b
    b.load()
    return b


@pytest.fixture(scope="module")
def world(oracle):
    """Both graphs with the oracle's tables, computed once and left unchanged."""
    out = {}
    for key, G in (("big", ss.build_graph()), ("small", ss.build_small_graph())):
        G["vde"] = {e: oracle.gen_vde(G["offsets"], G["nbrs"], G["labels"], e)[2] for e in ES}
        G["paths"] = {l: oracle.enumerate_closed(G["offsets"], G["nbrs"], G["sorted_nodes"], l + 1) for l in (2, 3)}
        out[key] = G
    return out


def case(world, name):
    if name == "R64_small":
        G = world["small"]
        b = ss.small_bounds(G["n"])
    else:
        G = world["big"]
        b = ss.bounds_sets(G["n"])[name]
    return G, ss.SlabModel(G["offsets"], G["nbrs"], G["sorted_nodes"], b)


def ranks_for(m):
    """Every rank up to five; of 64 the first and the last, the first, a middle and the last that own something (all of
    them where at most a dozen do), an empty one -- the owner search has no other shapes of neighbourhood -- and one
    on which the truncation empties a row."""
    if m.R <= 5:
        return list(range(m.R))
    key = (m.n, tuple(m.bounds.tolist()))
    if key not in _RANKS:
        full = [r for r in range(m.R) if m.bounds[r + 1] > m.bounds[r]]
        empty = [r for r in range(m.R) if m.bounds[r + 1] == m.bounds[r]]
        pick = set(full) if len(full) <= 12 else {full[0], full[len(full) // 2], full[-1]}
        if len(full) > 12:  # ... and the first rank on which a second-hop row keeps none of its entries
            pick.add(next(r for r in full if m.bounds[r] > 0 and _keeps_nothing(m, r)))
        _RANKS[key] = sorted(pick | {0, m.R - 1} | set(empty[:1]))
    return _RANKS[key]


_RANKS = {}


def _keeps_nothing(m, r):
    held, lists = m.hops(r, 3)
    return any(len(held.rows[int(v)]) == 0 and m.deg[v] > 0 for v in lists[1][0])


class Guard:
    """A device buffer of `cap` elements followed by a tail the call must not touch."""

    def __init__(self, cap, dtype=torch.int32, fill=SENT, tail=48):
        self.cap, self.fill = int(cap), fill
        self.t = torch.full((self.cap + tail,), fill, dtype=dtype, device=DEV)
        torch.cuda.synchronize()

    def head(self, k):
        return self.t[:int(k)].cpu().numpy()

    def untouched(self, used=None):
        """Everything from `used` (default: the capacity) on still holds the sentinel."""
        assert bool((self.t[self.cap if used is None else int(used):] == self.fill).all())


def up(a, np_dtype=np.int32):
    """Host array -> device tensor, complete before a context stream reads it (at least one element: never a null pointer)."""
    a = np.ascontiguousarray(np.asarray(a).astype(np_dtype))
    if a.size == 0:
        a = np.zeros(1, np_dtype)
    t = torch.from_numpy(a).to(DEV)
    torch.cuda.synchronize()
    return t


@pytest.fixture
def mk(binding):
    """Factory of contexts that play one rank: load_rows of the slab's rows, set_order, set_slab, set_label_table."""
    made = []

    def make(G, m, r, e=2, cap=None, variant=None, order=True):
        rows, roff, rn = m.owned_csr(r)
        eng = binding.Engine(0)
        made.append(eng)
        if variant is not None:
            eng.set_fill_variant(variant)
        eng.load_rows(G["n"], G["labels"], rows, roff, rn, nbr_capacity=2 * len(G["nbrs"]) if cap is None else cap)
        if order:
            eng.set_order(G["sorted_nodes"], G["membership"], 1)
            eng.set_slab(int(m.bounds[r]), int(m.bounds[r + 1]))
        eng.set_label_table(binding.host_label_table(G["n_labels"], e))
        return eng

    def whole(G, e=2, variant=None):
        eng = binding.Engine(0)
        made.append(eng)
        if variant is not None:
            eng.set_fill_variant(variant)
        eng.load_csr(G["offsets"], G["nbrs"], G["labels"])
        eng.set_order(G["sorted_nodes"], G["membership"], 1)
        eng.set_label_table(binding.host_label_table(G["n_labels"], e))
        return eng

    make.whole = whole
    yield make
    for eng in made:
        eng.close()


def gpu_need(eng, bounds, cap):
    buf = Guard(cap)
    counts = eng.halo_need(bounds, buf.t, cap).astype(np.int64)
    eng.sync()
    used = int(counts.sum())
    assert used <= cap
    buf.untouched(used)
    return buf.head(used).astype(np.int64), counts


def append(eng, m, ids, min_rank=0):
    """The rows of `ids` as their owners hold them (the model plays the owners), installed on `eng`."""
    deg, nb = m.concat_rows(ids)
    eng.rows_append(len(ids), up(ids), up(deg), up(nb), len(nb), min_rank)


def read_rows(eng, ids):
    """(degrees, rows back to back) of `ids` as the context holds them: rows_degree + rows_pack with exact capacities."""
    k = len(ids)
    d_ids = up(ids)
    deg = Guard(k)
    eng.rows_degree(k, d_ids, deg.t)
    eng.sync()
    deg.untouched()
    d = deg.head(k).astype(np.int64)
    tot = int(d.sum())
    out = Guard(tot)
    eng.rows_pack(k, d_ids, out.t, tot)
    eng.sync()
    out.untouched()
    return d, out.head(tot).view(np.uint32)


def check_held(eng, held):
    """rows_held() and every held row, read back, equal the model's state."""
    assert eng.rows_held() == held.stats()
    ids = held.ids()
    d, rows = read_rows(eng, ids)
    assert np.array_equal(d, [len(held.rows[int(v)]) for v in ids])
    want = [held.rows[int(v)] for v in ids if len(held.rows[int(v)])]
    assert np.array_equal(rows, np.concatenate(want) if want else np.zeros(0, np.uint32))


def gathered(G, m, e, stride, own=None, own_fill=POISON_F):
    """The all-gathered table [R][stride][e] of the oracle's vde rows: padding rows hold SENT_F, the block of rank `own` own_fill."""
    buf = np.full((m.R, stride, e), SENT_F)
    for o in range(m.R):
        rows = m.owned(o)
        buf[o, :len(rows)] = own_fill if o == own else G["vde"][e][rows]
    return buf


def table(eng, n, e):
    """The context's vde table, read through vde_device_ptr + copy_to_host."""
    eng.sync()
    ptr, _ = eng.vde_device_ptr()
    return eng.copy_to_host(ptr, n * e * 8).view(np.float64).reshape(n, e)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def install_hops(eng, m, r, l, truncate=True):
    """The halo of dist.SlabBuild.install_halo, fed from the model; returns the model's held state."""
    held = m.start(r)
    for hop in range(l - 1):
        ids, _ = m.need(held)
        mr = int(m.bounds[r]) if (truncate and hop == l - 2) else 0
        append(eng, m, ids, mr)
        m.install(held, ids, mr)
    return held


def exchange_vde(eng, G, m, r, e, stride_pad=3):
    """vde of the rank's own rows + the peers' slabs from the model; nothing is counted."""
    lens = np.diff(m.bounds)
    stride = int(lens.max()) + stride_pad
    eng.vde(want=False)
    buf = up(gathered(G, m, e, stride, own=r), np.float64)
    eng.vde_unpack_all(m.bounds, stride, r, buf)
    eng.sync()  # (before `buf` goes back to torch's allocator)


def emit(eng, G, m, r, l, e):
    """vde + the peers' slabs from the model + count + fill of rank r: (ids, pde)."""
    exchange_vde(eng, G, m, r, e)
    total = eng.count_paths(l)
    ids, pde, _ = eng.fill_paths(0, total)
    return ids, pde


def want_emit(G, m, r, l, e):
    p = m.slab_paths(G["paths"][l], r)
    return p, G["vde"][e][p.astype(np.int64)].reshape(len(p), (l + 1) * e)


# ---- gnnpe_halo_need ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_halo_need_first_hop(binding, world, mk, name):
    G, m = case(world, name)
    n = G["n"]
    for r in ranks_for(m):
        eng = mk(G, m, r)
        ids, counts = m.need(m.start(r))
        got, gc = gpu_need(eng, m.bounds, n)
        assert np.array_equal(gc, counts) and np.array_equal(got, ids), (name, r)
        assert gc[r] == 0
        used = len(ids)
        got, gc = gpu_need(eng, m.bounds, used)  # cap == used
        assert np.array_equal(gc, counts) and np.array_equal(got, ids), (name, r)
        if used:
            buf = Guard(used - 1)
            with pytest.raises(binding.GnnpeError, match=rf"id buffer too small \({used} needed\)"):
                eng.halo_need(m.bounds, buf.t, used - 1)
            eng.sync()
            buf.untouched(0)
            got, gc = gpu_need(eng, m.bounds, used)  # the call after the refusal
            assert np.array_equal(gc, counts) and np.array_equal(got, ids), (name, r)


def test_halo_need_refusals(binding, world, mk):
    G, m = case(world, "R2")
    n = G["n"]
    eng = mk(G, m, 1)
    buf = Guard(n)
    b65 = ((np.arange(66, dtype=np.int64) * n) // 65).astype(np.uint32)
    with pytest.raises(binding.GnnpeError, match="more than 64 ranks"):
        eng.halo_need(b65, buf.t, n)
    for bad in ([0, 300, 200, n], [1, 257, n], [0, 257, n - 1], [0, 257, n + 1], [0, n + 7, n]):
        with pytest.raises(binding.GnnpeError, match="slab bounds must run from 0 to n"):
            eng.halo_need(np.array(bad, np.uint32), buf.t, n)
    eng.sync()
    buf.untouched(0)
    ids, counts = m.need(m.start(1))
    got, gc = gpu_need(eng, m.bounds, n)
    assert np.array_equal(gc, counts) and np.array_equal(got, ids)
    no_order = mk(G, m, 1, order=False)
    with pytest.raises(binding.GnnpeError, match="no processing order"):
        no_order.halo_need(m.bounds, buf.t, n)


@pytest.mark.parametrize("name", CASES)
def test_halo_need_second_hop(world, mk, name):
    """Hop 1 installed whole: the second call lists the rows two hops out and nothing that is already there."""
    G, m = case(world, name)
    for r in ranks_for(m):
        eng = mk(G, m, r)
        held = install_hops(eng, m, r, 2, truncate=False)
        ids, counts = m.need(held)
        got, gc = gpu_need(eng, m.bounds, G["n"])
        assert np.array_equal(gc, counts) and np.array_equal(got, ids), (name, r)
        assert gc[r] == 0 and not np.isin(got, held.ids()).any()


# ---- gnnpe_rows_degree / gnnpe_rows_pack at the owner -----------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_rows_degree_and_pack_at_the_owner(binding, world, mk, name):
    G, m = case(world, name)
    rng = np.random.default_rng(7)
    for o in ranks_for(m):
        eng = mk(G, m, o)
        eng.rows_degree(0, None, None)  # n_req == 0 with null pointers: nothing to do
        eng.rows_pack(0, None, None, 0)
        own = m.owned(o)
        other = np.setdiff1d(np.arange(G["n"]), own)
        # every owned row in a random order, the first-hop requests of the other picked ranks (repeats of the former),
        # and two vertices this context does not hold
        req = [rng.permutation(own)]
        for r in ranks_for(m):
            ids, counts = m.need(m.start(r))
            lo = int(counts[:o].sum())
            req.append(ids[lo:lo + int(counts[o])])
        req.append(other[:2])
        req = np.concatenate(req).astype(np.int64)
        mine = np.isin(req, own)
        d, rows = read_rows(eng, req)
        assert np.array_equal(d, np.where(mine, m.deg[req], 0)), (name, o)
        assert np.array_equal(rows, m.concat_rows(req[mine])[1]), (name, o)
        tot = int(d.sum())
        if tot:
            out = Guard(tot - 1)
            with pytest.raises(binding.GnnpeError, match=rf"output holds {tot - 1} entries, need {tot}"):
                eng.rows_pack(len(req), up(req), out.t, tot - 1)
            eng.sync()
            out.untouched(0)


# ---- gnnpe_rows_append ----------------------------------------------------------------------------------------------
def _chunks(ids, chunked):
    if not chunked:
        return [ids]
    cuts = [c for c in (1, 3, 6, 10) if c < len(ids)]  # calls of 1, 2, 3, 4 rows and the rest: every residue mod 4
    return [c for c in np.split(ids, cuts) if len(c)]


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("mode", ["whole", "truncated", "two_hops"])
@pytest.mark.parametrize("name", CASES)
def test_rows_append_from_the_model(world, mk, name, mode, chunked):
    """min_rank = 0, min_rank = bounds[r], and the two hops of l = 3 (whole, then truncated: only there does a row keep
    nothing).  rows_held() after every call and every row read back equal the model."""
    G, m = case(world, name)
    for r in ranks_for(m):
        eng = mk(G, m, r)
        held = m.start(r)
        b = int(m.bounds[r])
        for min_rank in {"whole": [0], "truncated": [b], "two_hops": [0, b]}[mode]:
            ids, _ = m.need(held)
            for part in _chunks(ids, chunked):
                append(eng, m, part, min_rank)
                m.install(held, part, min_rank)
                assert eng.rows_held() == held.stats(), (name, r, mode)
        check_held(eng, held)


def test_rows_append_refusals(binding, world, mk):
    G, m = case(world, "R2")
    n, r = G["n"], 1
    b = int(m.bounds[r])
    owned = m.start(r)
    ids, _ = m.need(owned)
    deg, nb = m.concat_rows(ids)
    keep = sum(len(m.truncate(m.row(v), b)) for v in ids)
    d_ids, d_deg, d_nb = up(ids), up(deg), up(np.concatenate([nb, nb[:1]]))

    eng = mk(G, m, r)
    with pytest.raises(binding.GnnpeError, match=rf"degrees sum to {len(nb)} but {len(nb) + 1} entries given"):
        eng.rows_append(len(ids), d_ids, d_deg, d_nb, len(nb) + 1, b)
    assert eng.rows_held() == owned.stats()
    k = n - len(owned.rows) + 1
    with pytest.raises(binding.GnnpeError, match="more rows than vertices"):
        eng.rows_append(k, up(np.arange(k)), up(np.zeros(k)), up([0]), 0, 0)
    assert eng.rows_held() == owned.stats()

    # the neighbour buffer holds AT LEAST nbr_capacity entries; the refusal says how many it does hold
    own_e = owned.stats()[1]
    tight = mk(G, m, r, cap=0)
    with pytest.raises(binding.GnnpeError, match=rf"neighbour buffer full \({own_e} \+ {keep} > (\d+)\)") as err:
        tight.rows_append(len(ids), d_ids, d_deg, d_nb, len(nb), b)
    room = int(re.search(r"> (\d+)\)", str(err.value)).group(1)) - own_e
    assert 0 <= room < keep
    check_held(tight, owned)
    # rows of exactly room + 1 entries (the last one cut short: still a valid row) are one too many, room entries fit
    cs = np.cumsum(deg)
    j = int(np.searchsorted(cs, room + 1))  # rows 0..j hold at least room + 1 entries
    for total in (room + 1, room):
        cut = deg[:j + 1].copy()
        cut[j] -= int(cs[j]) - total
        rows = np.concatenate([m.row(v)[:int(c)] for v, c in zip(ids[:j + 1], cut)])
        args = (j + 1, d_ids, up(cut), up(rows), total, 0)
        if total > room:
            with pytest.raises(binding.GnnpeError, match=rf"neighbour buffer full \({own_e} \+ {total} > {own_e + room}\)"):
                tight.rows_append(*args)
            check_held(tight, owned)
        else:
            tight.rows_append(*args)
            assert tight.rows_held()[:2] == (len(owned.rows) + j + 1, own_e + room)
            d, got = read_rows(tight, ids[:j + 1])
            assert np.array_equal(d, cut) and np.array_equal(got, rows)

    no_order = mk(G, m, r, order=False)
    with pytest.raises(binding.GnnpeError, match="min_rank needs gnnpe_set_order"):
        no_order.rows_append(len(ids), d_ids, d_deg, d_nb, len(nb), b)
    assert no_order.rows_held() == owned.stats()

    csr = mk.whole(G)
    before = csr.rows_held()
    assert before[:2] == (n, len(G["nbrs"]))
    with pytest.raises(binding.GnnpeError, match="more rows than vertices"):
        csr.rows_append(1, d_ids, d_deg, d_nb, int(deg[0]), 0)
    assert csr.rows_held() == before

    # the refused context takes the same rows afterwards
    eng.rows_append(len(ids), d_ids, d_deg, d_nb, len(nb), b)
    check_held(eng, m.install(m.start(r), ids, b))


def test_rows_append_refuses_ids_that_are_no_new_rows(binding, world, mk):
    """An id >= n, an owned vertex and a vertex already in the halo are refused before anything is installed (with
    min_rank > 0 a second copy of an owned row would be truncated); the context goes on as if nothing had been sent."""
    G, m = case(world, "R2")
    n, r, l, e = G["n"], 1, 2, 2
    b = int(m.bounds[r])
    eng = mk(G, m, r)
    held = m.start(r)
    ids, _ = m.need(held)
    first, rest = ids[:len(ids) // 2], ids[len(ids) // 2:]
    append(eng, m, first, b)
    m.install(held, first, b)
    own = m.owned(r)

    def refused(bad_ids, pos, pattern):
        deg, nb = m.concat_rows([v if v < n else 0 for v in bad_ids])
        with pytest.raises(binding.GnnpeError, match=rf"row {pos} is vertex {bad_ids[pos] & 0xFFFFFFFF}, {pattern}"):
            eng.rows_append(len(bad_ids), up(np.array(bad_ids, np.int64).astype(np.uint32).view(np.int32)), up(deg), up(nb),
                            len(nb), b)
        assert eng.rows_held() == held.stats()

    refused([int(rest[0]), int(own[3])], 1, "whose row this context already holds")
    refused([int(own[0])], 0, "whose row this context already holds")
    refused([int(rest[0]), int(rest[1]), int(first[2])], 2, "whose row this context already holds")
    refused([int(rest[0]), n], 1, f"but the graph has {n} vertices")
    refused([0xFFFFFFFF], 0, f"but the graph has {n} vertices")
    refused([int(rest[0]), n + 5, int(own[1]), n], 1, f"but the graph has {n} vertices")  # the smallest position is named
    check_held(eng, held)  # owned rows whole, the first half of the halo as installed
    append(eng, m, rest, b)
    m.install(held, rest, b)
    check_held(eng, held)
    got_ids, got_pde = emit(eng, G, m, r, l, e)
    want_ids, want_pde = want_emit(G, m, r, l, e)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(bits(got_pde), bits(want_pde))


@pytest.mark.parametrize("fault", ["unsorted", "repeated", "self_loop", "id_out_of_range"])
def test_a_refused_peer_row_leaves_the_context_as_it_was(binding, world, mk, fault):
    """A peer sends a row that is no strictly ascending list of ids < n: the append names the vertex and installs none
    of its rows; halo_need still lists them; rows_drop_halo and a correct exchange give the exact enumeration."""
    G, m = case(world, "R2")
    n, r, l, e = G["n"], 1, 2, 2
    b = int(m.bounds[r])
    eng = mk(G, m, r)
    held = m.start(r)
    ids, _ = m.need(held)
    first, rest = ids[-7:], ids[:-7]  # (the planted rows have the smallest ids: they come with the refused call)
    append(eng, m, first, b)
    m.install(held, first, b)
    deg, nb = m.concat_rows(rest)
    # The refused call asks for a HIGHER truncation rank than the one in force (b), so that a refusal which kept it would
    # show; the faulty entries are chosen among those that survive it.  (A self-loop of a vertex of slab 0 never
    # survives a truncation: that row comes with min_rank = 0.)
    mr = 0 if fault == "self_loop" else b + 5
    offs = np.concatenate([[0], np.cumsum(deg)])
    kept = [np.flatnonzero(m.rank[nb[offs[i]:offs[i + 1]].astype(np.int64)] >= mr) for i in range(len(rest))]
    k = next(i for i in range(len(rest)) if deg[i] >= 17 and len(kept[i]) >= 3)  # longer than the 16 lanes that check it
    v, lo = int(rest[k]), int(offs[k])
    p, q = lo + int(kept[k][1]), lo + int(kept[k][2])  # two entries that end up side by side
    nb = nb.copy()
    if fault == "unsorted":
        nb[p], nb[q] = nb[q], nb[p]
    elif fault == "repeated":
        nb[q] = nb[p]
    elif fault == "self_loop":
        nb[lo + min(int(np.searchsorted(nb[lo:lo + int(deg[k])], v)), int(deg[k]) - 1)] = v  # (still ascending)
    else:
        nb[q] = n + 3
    with pytest.raises(binding.GnnpeError, match=rf"adjacency row of vertex {v} is not a strictly ascending list"):
        eng.rows_append(len(rest), up(rest), up(deg), up(nb.view(np.int32)), len(nb), mr)
    check_held(eng, held)  # nothing of the refused call stays
    got, gc = gpu_need(eng, m.bounds, n)
    want, wc = m.need(held)
    assert np.array_equal(got, want) and np.array_equal(gc, wc) and np.array_equal(want, rest)
    eng.set_slab(b, n)  # the refused call has not raised the rank the halo is truncated at ...
    with pytest.raises(binding.GnnpeError, match=rf"starts before rank {b}, below"):
        eng.set_slab(b - 1, n)  # ... nor lowered it
    eng.rows_drop_halo()
    assert eng.rows_held() == m.start(r).stats()
    held = install_hops(eng, m, r, l)
    check_held(eng, held)
    got_ids, got_pde = emit(eng, G, m, r, l, e)
    want_ids, want_pde = want_emit(G, m, r, l, e)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(bits(got_pde), bits(want_pde))


def test_set_slab_after_a_truncated_append(binding, world, mk):
    G, m = case(world, "R2")
    n, r = G["n"], 1
    b = int(m.bounds[r])
    eng = mk(G, m, r)
    install_hops(eng, m, r, 2)
    for begin in (0, b - 1):
        with pytest.raises(binding.GnnpeError, match=rf"starts before rank {b}, below which the halo rows on this device "
                                                     "were truncated"):
            eng.set_slab(begin, n)
    eng.set_slab(5, 5)  # an empty slab counts nothing
    eng.set_slab(b, n)
    eng.set_slab(b + 1, n - 1)
    eng.rows_drop_halo()
    eng.set_slab(0, n)
    eng.set_slab(b, n)


# ---- gnnpe_rows_drop_halo --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_rows_drop_halo(world, mk, name):
    G, m = case(world, name)
    n = G["n"]
    for r in ranks_for(m):
        eng = mk(G, m, r)
        owned = m.start(r)
        ids, counts = m.need(owned)
        held = install_hops(eng, m, r, 3)
        halo = held.halo_ids()
        eng.rows_drop_halo()
        check_held(eng, owned)
        d, rows = read_rows(eng, halo)  # no halo row is left behind
        assert not d.any() and len(rows) == 0
        got, gc = gpu_need(eng, m.bounds, n)
        assert np.array_equal(gc, counts) and np.array_equal(got, ids), (name, r)
        eng.rows_drop_halo()  # nothing to drop
        check_held(eng, owned)
        check_held(eng, install_hops(eng, m, r, 2))  # and the exchange can be repeated
    csr = mk.whole(G)
    before = csr.rows_held()
    assert before == (n, len(G["nbrs"]), int((m.deg > ss.HUB_DEGREE).sum()))
    csr.rows_drop_halo()
    assert csr.rows_held() == before


# ---- gnnpe_vde_pack_slab / _unpack_slab / _unpack_all ---------------------------------------------------------------
@pytest.mark.parametrize("e", ES)
def test_vde_pack_slab(world, mk, e):
    G = world["big"]
    n = G["n"]
    eng = mk.whole(G, e)
    eng.vde(want=False)
    slabs = set()
    for name in ("R2", "R5_empty_ends", "R64"):
        b = ss.bounds_sets(n)[name]
        slabs |= {(int(b[r]), int(b[r + 1])) for r in range(len(b) - 1)}
    slabs |= {(0, n), (n, n), (n - 1, n)}
    for lo, hi in sorted(slabs):
        buf = Guard((hi - lo) * e, torch.float64, SENT_F)
        eng.vde_pack_slab(lo, hi, buf.t)
        eng.sync()
        buf.untouched()  # (an empty slab: the whole buffer)
        want = G["vde"][e][G["sorted_nodes"][lo:hi].astype(np.int64)]
        assert np.array_equal(bits(buf.head((hi - lo) * e)), bits(want).reshape(-1)), (e, lo, hi)


@pytest.mark.parametrize("e", ES)
@pytest.mark.parametrize("name", ["R2", "R3_empty_middle", "R5_empty_ends", "R64", "R64_small"])
def test_vde_unpack_all(world, mk, name, e):
    """All-gather buffer [R][stride][e] with stride = longest slab + 3, sentinel padding and a poisoned own block."""
    G, m = case(world, name)
    n = G["n"]
    stride = int(np.diff(m.bounds).max()) + 3
    want = G["vde"][e]
    for r in [x for x in ranks_for(m) if m.bounds[x + 1] > m.bounds[x]][:4]:
        eng = mk(G, m, r, e)
        eng.vde(want=False)
        buf = up(gathered(G, m, e, stride, own=r), np.float64)
        eng.vde_unpack_all(m.bounds, stride, r, buf)
        got = table(eng, n, e)
        assert np.array_equal(bits(got), bits(want)), (name, r, e)
        assert not np.isin(got, (SENT_F, POISON_F)).any()
        # no rank skipped: the own block is written too
        eng.vde_unpack_all(m.bounds, stride, 0xFFFFFFFF, buf)
        got = table(eng, n, e)
        mine = np.zeros(n, bool)
        mine[m.owned(r)] = True
        assert np.all(got[mine] == POISON_F) and np.array_equal(bits(got[~mine]), bits(want[~mine])), (name, r, e)
        # slab by slab
        eng.vde(want=False)
        sent = []  # (alive until the context has read them)
        for o in range(m.R):
            if o != r and m.bounds[o + 1] > m.bounds[o]:
                sent.append(up(want[m.owned(o)], np.float64))
                eng.vde_unpack_slab(int(m.bounds[o]), int(m.bounds[o + 1]), sent[-1])
        assert np.array_equal(bits(table(eng, n, e)), bits(want)), (name, r, e)


def test_vde_unpack_all_refusals(binding, world, mk):
    G, m = case(world, "R3_empty_middle")
    n, e, r = G["n"], 2, 2
    lens = np.diff(m.bounds)
    stride = int(lens.max())
    buf = up(gathered(G, m, e, stride + 3, own=r), np.float64)
    eng = mk(G, m, r, e)
    with pytest.raises(binding.GnnpeError, match="bad state"):
        eng.vde_unpack_all(m.bounds, stride + 3, r, buf)  # before gnnpe_vde
    eng.vde(want=False)
    with pytest.raises(binding.GnnpeError, match=rf"slab 2: \[211, {n}\) does not fit rows of stride {stride - 1}"):
        eng.vde_unpack_all(m.bounds, stride - 1, r, buf)
    for bad in ([1, 211, 211, n], [0, 211, 211, n - 1]):
        with pytest.raises(binding.GnnpeError, match="slab bounds must run from 0 to n"):
            eng.vde_unpack_all(np.array(bad, np.uint32), stride + 3, r, buf)
    with pytest.raises(binding.GnnpeError, match="does not fit rows of stride"):
        eng.vde_unpack_all(np.array([0, 300, 200, n], np.uint32), stride + 3, r, buf)  # a step down
    eng.vde_unpack_all(m.bounds, stride + 3, r, buf)
    assert np.array_equal(bits(table(eng, n, e)), bits(G["vde"][e]))


# ---- gnnpe_count_paths_enqueue + gnnpe_count_total_device ------------------------------------------------------------
@pytest.mark.parametrize("name", ["R1", "R2", "R5_empty_ends"])
def test_count_total_device(binding, world, mk, name):
    """The device word a collective sends, read BEFORE any host fetch of the total, on a context that has never counted
    and again after the rows changed (both are fresh counts: no structure of an earlier count to reuse), equals the
    oracle.  The enqueue-only count is l = 2 only (it says so); for l = 3 the word follows gnnpe_count_paths."""
    G, m = case(world, name)
    want = {l: [len(m.slab_paths(G["paths"][l], r)) for r in range(m.R)] for l in (2, 3)}
    assert sum(want[2]) == len(G["paths"][2]) > 0
    for r in [x for x in range(m.R) if m.bounds[x + 1] > m.bounds[x]]:
        eng = mk(G, m, r)
        for hops in (2, 3):  # the halo of l = 2, then (dropped and fetched again) the two hops of l = 3
            eng.rows_drop_halo()
            install_hops(eng, m, r, hops)
            exchange_vde(eng, G, m, r, 2)
            word = Guard(1, torch.int64, -7)
            eng.count_paths_enqueue(2)
            eng.count_total_device(word.t)
            eng.sync()
            word.untouched()
            assert int(word.head(1)[0]) == want[2][r], (name, r, hops)
            assert eng.count_total() == want[2][r] == eng.count_paths(2)
        with pytest.raises(binding.GnnpeError, match="l=2 with a specialised embedding width only"):
            eng.count_paths_enqueue(3)
        word = Guard(1, torch.int64, -7)
        assert eng.count_paths(3) == want[3][r]
        eng.count_total_device(word.t)
        eng.sync()
        word.untouched()
        assert int(word.head(1)[0]) == want[3][r] == eng.count_total(), (name, r)


# ---- the helpers chained --------------------------------------------------------------------------------------------
def _assert_enumeration(G, m, l, e, parts):
    ids = np.concatenate([p[0] for p in parts])
    pde = np.concatenate([p[1] for p in parts])
    want = G["paths"][l]
    assert np.array_equal(ids, want)
    assert np.array_equal(bits(pde), bits(G["vde"][e][want.astype(np.int64)].reshape(len(want), (l + 1) * e)))


@pytest.mark.parametrize("l,variant", [(2, 1), (2, 4), (3, 4)])
def test_three_ranks_engine_to_engine(world, mk, l, variant):
    """Real peers, one of them with an empty slab: need -> degree and pack at the owner -> append, per hop (the last one
    truncated); pack_slab -> the all-gathered table -> unpack_all; the ranks' rows in order are the whole enumeration."""
    G, m = case(world, "R3_empty_middle")
    n, e, R = G["n"], 2, m.R
    engs = [mk(G, m, r, e, variant=variant) for r in range(R)]
    for hop in range(l - 1):
        for r in range(R):
            ids, counts = gpu_need(engs[r], m.bounds, n)
            assert counts[r] == 0 and counts[1] == 0  # nobody asks itself, nobody asks the empty slab
            deg = Guard(len(ids))
            pos = 0
            for o in range(R):
                k = int(counts[o])
                if k:
                    engs[o].rows_degree(k, up(ids[pos:pos + k]), deg.t[pos:pos + k])
                    engs[o].sync()
                pos += k
            deg.untouched()
            d = deg.head(len(ids)).astype(np.int64)
            assert np.array_equal(d, m.deg[ids])
            tot = int(d.sum())
            nb = Guard(tot)
            pos = at = 0
            for o in range(R):
                k = int(counts[o])
                if k:
                    part = int(d[pos:pos + k].sum())
                    engs[o].rows_pack(k, up(ids[pos:pos + k]), nb.t[at:at + part], part)
                    engs[o].sync()
                    at += part
                pos += k
            nb.untouched()
            engs[r].rows_append(len(ids), up(ids), deg.t, nb.t, tot, int(m.bounds[r]) if hop == l - 2 else 0)
    for r in range(R):
        assert engs[r].rows_held() == m.hops(r, l)[0].stats()
    lens = np.diff(m.bounds)
    stride = int(lens.max()) + 3
    allg = torch.full((R, stride, e), SENT_F, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    for r in range(R):
        if lens[r]:
            engs[r].vde(want=False)
            engs[r].vde_pack_slab(int(m.bounds[r]), int(m.bounds[r + 1]), allg[r])
            engs[r].sync()
    parts = []
    for r in range(R):
        if lens[r]:  # (a context without rows has nothing to count: its slab is empty)
            engs[r].vde_unpack_all(m.bounds, stride, r, allg)
            total = engs[r].count_paths(l)
            ids, pde, _ = engs[r].fill_paths(0, total)
            parts.append((ids, pde))
    _assert_enumeration(G, m, l, e, parts)


@pytest.mark.parametrize("l,variant", [(2, 1), (2, 4), (3, 4)])
@pytest.mark.parametrize("name", ["R5_empty_ends", "R64", "R64_small"])
def test_model_fed_ranks_enumerate_everything(world, mk, name, l, variant):
    """Every rank of the set, fed by the model alone (halo rows, the peers' vde slabs): all exchanged state is used."""
    G, m = case(world, name)
    e = 2
    parts = []
    for r in range(m.R):
        if m.bounds[r + 1] == m.bounds[r]:
            continue
        eng = mk(G, m, r, e, variant=variant)
        held = install_hops(eng, m, r, l)
        assert eng.rows_held() == held.stats()
        parts.append(emit(eng, G, m, r, l, e))
        eng.close()
    _assert_enumeration(G, m, l, e, parts)
