"""The standing exact query (gnnpe_standing_* of include/gnnpe_online.h, gnnpe_filter_support_bitmap_device of include/gnnpe_hip.h):
the two set kernels against numpy, and the loop of gnnpe_standing_apply_edges against brute force.

Yardsticks, none of which shares code with the library:
  * np.unpackbits / np.flatnonzero for k_sets_sizes and k_sets_members;
  * `embeddings`: every map of a query into the numpy graph by joining CSR rows position by position (labels, injectivity, the query
    edges on data edges, under `induced` the query non-edges on data non-edges).  The distinct modes are checked on ORBITS: the
    automorphisms of the query are found here by trying every permutation, a row is reduced to the smallest of its images under
    them, and the library's rows must hit every orbit of the yardstick exactly once;
  * np_support of tests/test_filter_support.py for S, and for bitmaps gnnpe_filter_candidates_exact on a FRESH engine (fresh_bits).

What a batch creates and destroys is compared in the two steps the header describes -- G, G1 = G - D, G' = G1 + I -- because a
context with an induced handle applies a mixed batch that way: created = (M(G1) - M(G)) + (M(G') - M(G1)) and destroyed =
(M(G) - M(G1)) + (M(G1) - M(G')) as multisets.  For a handle that is not induced, and for a batch with one list empty, these are
M(G') - M(G) and M(G) - M(G').

Shapes.  The set kernels: n at the word edges (1, 31 .. 65), 301, and around the 8192-vertex tile of k_sets_members (8191, 8192,
8193, and 24593 = three tiles and 17 vertices); the graph under them is the path 0 - 1 - ... - (n - 1), so that the count of open
depends on every start candidate k_sets_members wrote.  The loop: make_graph(hub_deg=64) of the support tests (n = 301, a hub row
that goes from 64 to 65 entries and back, an isolated vertex that gets its first edge), e = 2."""
import itertools

import numpy as np
import pytest

import test_filter_support as fs
import test_online_exact as base
from test_online_exact import _write_query

pytestmark = pytest.mark.gpu

FULL = (1 << 64) - 1
E = 2
TILE = 8192  # vertices per tile of k_sets_members (256 words)
MODES = [(False, False), (True, False), (False, True), (True, True)]  # (distinct, induced)
HUB, ISOLATED = fs.HUB, fs.ISOLATED

# name: (vertices, edges, labels).  The labels are those of the support tests' graph (4 labels, the hub has label 1).
QUERIES = {
    "wedge": (3, {(0, 1), (1, 2)}, [1, 0, 1]),
    "triangle": (3, {(0, 1), (1, 2), (0, 2)}, [1, 1, 1]),
    "path3": (4, {(0, 1), (1, 2), (2, 3)}, [1, 0, 0, 1]),
    "c4": (4, {(0, 1), (1, 2), (2, 3), (0, 3)}, [1, 0, 1, 0]),
    "diamond": (4, {(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)}, [1, 0, 1, 0]),
    "house": (5, {(0, 1), (1, 2), (2, 3), (0, 3), (0, 4), (1, 4)}, [0, 0, 1, 1, 0]),
}


def write_query(tmp_path, name):
    nq, edges, labels = QUERIES[name]
    qp = str(tmp_path / f"{name}.graph")
    _write_query(qp, nq, edges, labels)
    return qp


# ---- the brute force ------------------------------------------------------------------------------------------------------------------

def embeddings(g, query, induced, bits=None):
    """every map of the mode (not distinct): int64 [K, nq], column = query vertex.  bits: bool [nq, n], the candidate sets"""
    nq, qedges, qlabels = query
    n = g["n"]
    offs, nb, lab = g["offsets"].astype(np.int64), g["nbrs"].astype(np.int64), g["labels"].astype(np.int64)
    deg = np.diff(offs)
    keys = np.unique(np.repeat(np.arange(n), deg) * n + nb)  # the directed entries, sorted
    qadj = {(a, b) for a, b in qedges} | {(b, a) for a, b in qedges}
    order = [0]
    while len(order) < nq:
        order.append(next(u for u in range(nq) if u not in order and any((u, w) in qadj for w in order)))

    def fits(u, x):
        ok = lab[x] == qlabels[u]
        return ok & bits[u][x] if bits is not None else ok

    v0 = np.arange(n)
    rows = v0[fits(order[0], v0)][:, None]
    for i in range(1, nq):
        u = order[i]
        p = next(j for j in range(i) if (order[j], u) in qadj)
        cnt = deg[rows[:, p]]
        rep = np.repeat(np.arange(len(rows)), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        x = nb[offs[rows[rep, p]] + within]
        keep = fits(u, x) & np.all(rows[rep] != x[:, None], axis=1)
        for j in range(i):
            if j == p:
                continue
            joined = np.isin(rows[rep, j] * n + x, keys)
            if (order[j], u) in qadj:
                keep &= joined
            elif induced:
                keep &= ~joined
        rows = np.column_stack([rows[rep][keep], x[keep]])
    out = np.zeros_like(rows)
    out[:, order] = rows
    return out


def automorphisms(query):
    nq, qedges, qlabels = query
    qadj = {(a, b) for a, b in qedges} | {(b, a) for a, b in qedges}
    return [p for p in itertools.permutations(range(nq))
            if all(qlabels[p[u]] == qlabels[u] for u in range(nq)) and all((p[a], p[b]) in qadj for a, b in qedges)]


def orbit_reps(rows, auts):
    """every row reduced to the smallest of its images under the automorphisms, as a list of tuples (with repeats)"""
    return [min(tuple(int(r[a]) for a in p) for p in auts) for r in np.asarray(rows, np.int64)]


def match_set(g, query, distinct, induced, bits=None):
    """the matches of a mode as a set of tuples: embeddings, or with `distinct` their orbit representatives"""
    rows = embeddings(g, query, induced, bits)
    return set(orbit_reps(rows, automorphisms(query))) if distinct else set(map(tuple, rows.tolist()))


def as_mode(rows, query, distinct):
    """the library's rows in the form match_set uses: a sorted list, so that a repeated orbit or row shows"""
    return sorted(orbit_reps(rows, automorphisms(query)) if distinct else map(tuple, np.asarray(rows, np.int64).tolist()))


def two_step(M0, M1, M2):
    """(created, destroyed) of a batch applied as D, then I: sorted lists, a transient match of the graph in between in both"""
    return sorted(list(M1 - M0) + list(M2 - M1)), sorted(list(M0 - M1) + list(M1 - M2))


def check_batch(sq, query, mode, sets3, what):
    """count, created, destroyed and the kept rows of a handle after a batch against the three match sets of the yardstick"""
    distinct, induced = mode
    created, destroyed = two_step(*sets3)
    count, n_created, n_destroyed, rows_c, rows_d, _ = sq.result()
    assert count == len(sets3[2]), (what, mode, count, len(sets3[2]))
    assert (n_created, n_destroyed) == (len(created), len(destroyed)), (what, mode, n_created, n_destroyed, len(created), len(destroyed))
    assert (rows_c, rows_d) == (len(created), len(destroyed)), (what, mode, "rows held")
    assert as_mode(sq.rows(0), query, distinct) == created, (what, mode, "created rows")
    assert as_mode(sq.rows(1), query, distinct) == destroyed, (what, mode, "destroyed rows")
    return len(created), len(destroyed)


# ---- 1. the two set kernels ---------------------------------------------------------------------------------------------------------

SET_N = (1, 31, 32, 33, 63, 64, 65, 301, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)


def path_graph(n):
    e = {(i, i + 1) for i in range(n - 1)}
    if not e:
        return dict(n=n, offsets=np.zeros(n + 1, np.uint32), nbrs=np.zeros(0, np.uint32), labels=np.zeros(n, np.uint32), edges=set())
    return fs.graph_of(n, e, np.zeros(n, np.uint32))


def set_rows(n, rng):
    """the rows of the issue as bool [rows, n]"""
    words = (n + 31) // 32
    alt = np.repeat(np.arange(words) % 2 == 0, 32)[:n]
    rows = [np.zeros(n, bool), np.ones(n, bool), np.arange(n) == 0, np.arange(n) == n - 1, alt]
    rows += [rng.random(n) < p for p in (0.01, 0.5, 0.99)]
    return np.array(rows)


def pack(bits, garbage=False):
    """bool [rows, n] -> the uint32 bitmap; garbage: the bits at and above n of the last word set, which the kernels must not see"""
    rows, n = bits.shape
    words = (n + 31) // 32
    full = np.zeros((rows, words * 32), bool)
    full[:, :n] = bits
    if garbage:
        full[:, n:] = True
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little").view(np.uint32).reshape(rows, words))


@pytest.mark.parametrize("n", SET_N)
def test_gpu_set_kernels_against_numpy(tmp_path, n):
    from gnnpe_amd import binding
    rng = np.random.default_rng(1000 + n)
    g = path_graph(n)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    rows = set_rows(n, rng)
    _write_query(str(tmp_path / "one.graph"), 1, set(), [0])
    wedge = (3, {(0, 1), (1, 2)}, [0, 0, 0])
    _write_query(str(tmp_path / "three.graph"), *wedge)
    # the single-vertex query: every row of the issue in turn, through set_bitmap, bits past n set in the upload
    sq = eng.standing_open(str(tmp_path / "one.graph"), bitmap=pack(rows[:1], garbage=True))
    for r in range(len(rows)):
        sq.set_bitmap(pack(rows[r:r + 1], garbage=True))
        want = np.flatnonzero(rows[r])
        assert list(sq.set_sizes()) == [len(want)], (n, r)
        ids, size = sq.set_members(0)
        assert size == len(want) and np.array_equal(ids, want), (n, r, "members")
        assert np.all(np.diff(ids.astype(np.int64)) > 0), (n, r, "ascending")
        assert sq.count == len(want), (n, r, "the count of a single-vertex query is its set's size")
        for cap in sorted({0, 1, len(want) // 2, max(len(want) - 1, 0)}):  # a cap below the size: the first ids, the true size
            out = np.full(len(want) + 8, 0xDEADBEEF, np.uint32)
            ids, size = sq.set_members(0, cap=cap, out=out)
            assert size == len(want) and np.array_equal(ids, want[:cap]), (n, r, cap)
            assert np.all(out[cap:] == 0xDEADBEEF), (n, r, cap, "canary")
    sq.close()
    # the 3-vertex query: three different rows at once; the count needs every start candidate the device wrote
    for pick in ([5, 6, 7], [1, 6, 4], [7, 2, 6], [6, 0, 5]):
        bits = rows[pick]
        sq = eng.standing_open(str(tmp_path / "three.graph"), bitmap=pack(bits, garbage=True))
        assert list(sq.set_sizes()) == list(bits.sum(axis=1)), (n, pick)
        for u in range(3):
            ids, size = sq.set_members(u)
            assert size == bits[u].sum() and np.array_equal(ids, np.flatnonzero(bits[u])), (n, pick, u)
        assert sq.count == len(embeddings(g, wedge, False, bits)), (n, pick, "count")
        assert np.array_equal(fs.bits_of(sq.bitmap(), n), bits), (n, pick, "bitmap")
        sq.close()
    eng.close()


@pytest.mark.parametrize("n", SET_N)
def test_gpu_bitmap_device_equals_the_host_form(n):
    """gnnpe_filter_support_bitmap_device against gnnpe_filter_support_bitmap on patterned tables with zeros planted; a buffer full
    of ones beforehand shows that every word is written and that the bits at and above n are zero"""
    import ctypes as C
    import torch
    from gnnpe_amd import binding
    g = path_graph(n)
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    rng = np.random.default_rng(2000 + n)
    nq, words = 3, (n + 31) // 32
    _, pat = fs.pattern(nq, n)
    pat = pat.copy()
    pat[rng.random(pat.shape) < 0.4] = 0
    pat[0, :] = 0  # an empty row
    pat[1, n - 1] = 7  # the last vertex
    table = torch.from_numpy(pat.view(np.int64)).cuda()
    out = torch.full((nq, words), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for timed in (False, True):
        ms = C.c_double(-1.0)
        eng._ck(eng.lib.gnnpe_filter_support_bitmap_device(eng.ctx, nq, table.data_ptr(), out.data_ptr(), C.byref(ms) if timed else None))
        eng.sync()
        got = out.cpu().numpy().view(np.uint32)
        want, _ = eng.support_bitmap(table, nq)
        assert np.array_equal(got, want), (n, timed)
        assert np.array_equal(fs.bits_of(got, n), pat != 0), (n, timed)
        assert n % 32 == 0 or not np.any(got[:, -1] >> np.uint32(n % 32)), (n, "bits past n")
        assert not timed or ms.value >= 0.0
        out.fill_(-1)
        torch.cuda.synchronize()
    eng.close()


# ---- 2. the loop against brute force ----------------------------------------------------------------------------------------------------

def norm_pairs(pairs):
    return sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in pairs})


_BATCHES = {}


def loop_batches(g0, seed, name):
    """the batches of the issue on make_graph(hub_deg=64) for a query, each as (name, insert, delete), drawn against the graph as it
    then is.  The pairs carry the labels of a query edge, and the single insert and the single delete are the most telling of 30
    drawn -- by the yardstick alone -- so that the small batches create and destroy matches as well"""
    if (seed, name) in _BATCHES:
        return _BATCHES[seed, name]
    query = QUERIES[name]
    rng = np.random.default_rng(seed)
    out, cur = [], g0
    edge_labels = {(query[2][a], query[2][b]) for a, b in query[1]} | {(query[2][b], query[2][a]) for a, b in query[1]}

    def fits(a, b):
        return (int(cur["labels"][a]), int(cur["labels"][b])) in edge_labels

    def draw(k_ins, k_del):
        ins, dele = set(), set()
        have = [e for e in sorted(cur["edges"]) if HUB not in e and fits(*e)]
        while len(dele) < k_del:
            dele.add(have[int(rng.integers(len(have)))])
        while len(ins) < k_ins:
            a, b = sorted(int(x) for x in rng.choice(300, 2, replace=False))
            if (a, b) not in cur["edges"] and ISOLATED not in (a, b) and fits(a, b):
                ins.add((a, b))
        return sorted(ins), sorted(dele)

    def telling(k_ins, k_del):
        M = match_set(cur, query, False, False)
        return max((draw(k_ins, k_del) for _ in range(30)),
                   key=lambda b: len(match_set(fs.apply_edges_np(cur, *b), query, False, False) ^ M))

    def push(what, ins, dele):
        nonlocal cur
        out.append((what, norm_pairs(ins), norm_pairs(dele)))
        cur = fs.apply_edges_np(cur, ins, dele)

    push("one insert", *telling(1, 0))
    push("one delete", *telling(0, 1))
    push("20 + 20", *draw(20, 20))
    free = next(v for v in range(300) if (v, HUB) not in cur["edges"] and v != ISOLATED and cur["labels"][v] == 0)
    push("hub 64 -> 65", [(free, HUB)], [])
    push("hub 65 -> 64", [], [(free, HUB)])
    deg = np.diff(cur["offsets"].astype(np.int64))
    v = next(int(x) for x in np.argsort(deg, kind="stable") if deg[x] > 0 and x != HUB)
    push("a row emptied", [], [(v, int(w)) for w in fs.nbrs_of(cur, v)])
    push("the isolated vertex's first edge", [(ISOLATED, HUB)], [])
    push("the empty batch", [], [])
    _BATCHES[seed, name] = out
    return out


def run_loop(oracle, tmp_path, g0, name, l, batches, check_filter=True):
    """four handles (the four modes) of one query on one context through every batch"""
    from gnnpe_amd import binding
    query = QUERIES[name]
    qp = write_query(tmp_path, name)
    plan = binding.host_query_plan_exact(qp, E, l)
    eng = fs.open_engine(g0, E)
    handles = [eng.standing_open(qp, l=l, distinct=d, induced=i, rows_cap=200000) for d, i in MODES]
    cur = g0
    sets = {m: match_set(cur, query, *m) for m in MODES}
    for sq, m in zip(handles, MODES):
        assert sq.count == len(sets[m]), (name, l, m, "open")
    moved = np.zeros(2, np.int64)
    for what, ins, dele in batches:
        mid = fs.apply_edges_np(cur, [], dele)
        nxt = fs.apply_edges_np(mid, ins, [])
        gen = handles[0].result()[5]
        eng.standing_apply_edges(insert=ins, delete=dele)
        assert handles[0].result()[5] == gen + (2 if ins and dele else 1 if ins or dele else 0), (what, "generation")
        off, nb = eng.download_csr()
        assert np.array_equal(off, nxt["offsets"]) and np.array_equal(nb, nxt["nbrs"]), (what, "the graph")
        for sq, m in zip(handles, MODES):
            after = {k: match_set(k_g, query, *m) for k, k_g in (("mid", mid), ("nxt", nxt))}
            moved += check_batch(sq, query, m, (sets[m], after["mid"], after["nxt"]), (name, l, what))
            sets[m] = after["nxt"]
        if check_filter:
            vde = fs.vde_of(oracle, nxt, E)
            want = fs.np_support(nxt, vde, plan)
            fresh = fs.fresh_bits(nxt, E, plan)
            for sq in handles:
                assert np.array_equal(sq.table(), want), (name, l, what, "S")
                assert np.array_equal(fs.bits_of(sq.bitmap(), nxt["n"]), fresh), (name, l, what, "C against the fresh filter")
                assert list(sq.set_sizes()) == list(fresh.sum(axis=1)), (name, l, what, "sizes")
            # a fresh open on a fresh engine with G'
            eng2 = fs.open_engine(nxt, E)
            for m in MODES:
                sq2 = eng2.standing_open(qp, l=l, distinct=m[0], induced=m[1])
                assert sq2.count == len(sets[m]), (name, l, what, m, "fresh open")
            eng2.close()
        cur = nxt
    eng.close()
    return moved


@pytest.mark.parametrize("l", [2, 3])
@pytest.mark.parametrize("name", ["wedge", "triangle", "path3", "c4", "diamond"])
def test_gpu_loop_against_brute_force(oracle, tmp_path, name, l):
    g0 = fs.make_graph(hub_deg=64)
    moved = run_loop(oracle, tmp_path, g0, name, l, loop_batches(g0, 71, name))
    assert moved[0] > 0 and moved[1] > 0, (name, l, "the batches neither created nor destroyed a match: the test shows nothing", moved)


@pytest.mark.parametrize("l", [2, 3])
def test_gpu_loop_five_vertex_query(oracle, tmp_path, l):
    """the house on G(60, 240), two labels: brute force stays within seconds"""
    from gnnpe_amd import synth
    g0 = synth.gnm_graph(60, 240, n_labels=2, seed=5)
    g = fs.graph_of(60, {(int(a), int(b)) for a, b in zip(g0["eu"], g0["ev"])}, g0["labels"])
    rng = np.random.default_rng(9)
    batches, cur = [], g
    for k in (1, 6, 12):
        have = sorted(cur["edges"])
        dele = {have[int(i)] for i in rng.choice(len(have), k, replace=False)}
        ins = set()
        while len(ins) < k:
            a, b = sorted(int(x) for x in rng.choice(60, 2, replace=False))
            if (a, b) not in cur["edges"]:
                ins.add((a, b))
        batches.append((f"{k} + {k}", norm_pairs(ins), norm_pairs(dele)))
        cur = fs.apply_edges_np(cur, ins, dele)
    moved = run_loop(oracle, tmp_path, g, "house", l, batches)
    assert moved[0] > 0 and moved[1] > 0, moved


# ---- 3. two handles on one context -----------------------------------------------------------------------------------------------------

def test_gpu_two_handles_and_the_seventeenth(oracle, tmp_path):
    from gnnpe_amd import binding
    g0 = fs.make_graph(hub_deg=64)
    tri, c4 = write_query(tmp_path, "triangle"), write_query(tmp_path, "c4")
    eng = fs.open_engine(g0, E)
    a = eng.standing_open(tri, l=2, rows_cap=100000)
    b = eng.standing_open(c4, l=3, distinct=True, induced=True, rows_cap=100000)
    cases = ((a, "triangle", (False, False)), (b, "c4", (True, True)))
    sets = {name: match_set(g0, QUERIES[name], *m) for _, name, m in cases}
    cur = g0
    rng = np.random.default_rng(3)
    for k in (3, 10, 25):
        have = [e for e in sorted(cur["edges"])]
        dele = [have[int(i)] for i in rng.choice(len(have), k, replace=False)]
        ins = set()
        while len(ins) < k:
            x, y = sorted(int(v) for v in rng.choice(301, 2, replace=False))
            if (x, y) not in cur["edges"]:
                ins.add((x, y))
        mid = fs.apply_edges_np(cur, [], dele)
        nxt = fs.apply_edges_np(mid, ins, [])
        eng.standing_apply_edges(insert=sorted(ins), delete=dele)
        for sq, name, m in cases:
            after = (match_set(mid, QUERIES[name], *m), match_set(nxt, QUERIES[name], *m))
            check_batch(sq, QUERIES[name], m, (sets[name], after[0], after[1]), (name, k))
            sets[name] = after[1]
        cur = nxt
    more = [eng.standing_open(tri, l=2) for _ in range(14)]
    assert all(sq.count == a.count for sq in more)
    with pytest.raises(binding.GnnpeError, match="16 standing queries"):
        eng.standing_open(tri, l=2)
    more[0].close()
    eng.standing_open(tri, l=2).close()  # a closed handle gives its place back
    eng.close()  # closes the fifteen that are still open


# ---- 4. refusals, transactionality, staleness ---------------------------------------------------------------------------------------------

def snapshot(eng, handles):
    off, nb = eng.download_csr()
    return [off.tobytes(), nb.tobytes()] + [x for sq in handles for x in (sq.table().tobytes(), sq.bitmap().tobytes(), sq.result(),
                                                                          sq.rows(0).tobytes(), sq.rows(1).tobytes())]


def test_gpu_refused_batches_change_nothing(oracle, tmp_path):
    from gnnpe_amd import binding
    g0 = fs.make_graph(hub_deg=64)
    name, query = "c4", QUERIES["c4"]
    qp = write_query(tmp_path, name)
    eng = fs.open_engine(g0, E)
    handles = [eng.standing_open(qp, l=2, distinct=d, induced=i, rows_cap=100000) for d, i in ((False, False), (True, True))]
    modes = [(False, False), (True, True)]
    have = sorted(g0["edges"])
    non = next((a, b) for a in range(300) for b in range(a + 1, 300) if (a, b) not in g0["edges"])
    good_ins = [(a, b) for a in range(40, 60) for b in range(60, 62) if (a, b) not in g0["edges"]][:6]
    eng.standing_apply_edges(insert=good_ins[:3], delete=have[:3])  # so that rows are kept and created / destroyed are not zero
    cur = fs.apply_edges_np(g0, good_ins[:3], have[:3])
    before = snapshot(eng, handles)
    refused = {
        "a non-edge in D": (good_ins[3:4], [have[10], non], "not an edge"),
        "an existing edge in I": ([good_ins[3], have[11]], have[12:13], "already an edge"),
        "a loop": ([(5, 5)], have[12:13], "loop|5, 5"),
        "an id >= n": (good_ins[3:4], [(3, 301)], "301"),
        "an edge in both lists": ([have[20]], [have[20]], "both lists"),
    }
    for what, (ins, dele, msg) in refused.items():
        with pytest.raises(binding.GnnpeError, match=msg) as err:
            eng.standing_apply_edges(insert=ins, delete=dele)
        assert "[-1]" in str(err.value), (what, str(err.value))
        assert snapshot(eng, handles) == before, what
    # a following valid batch is exact
    ins, dele = good_ins[3:], have[30:34]
    mid = fs.apply_edges_np(cur, [], dele)
    nxt = fs.apply_edges_np(mid, ins, [])
    eng.standing_apply_edges(insert=ins, delete=dele)
    vde = fs.vde_of(oracle, nxt, E)
    plan = binding.host_query_plan_exact(qp, E, 2)
    for sq, m in zip(handles, modes):
        check_batch(sq, query, m, tuple(match_set(x, query, *m) for x in (cur, mid, nxt)), "after the refusals")
        assert np.array_equal(sq.table(), fs.np_support(nxt, vde, plan))
    eng.close()


def test_gpu_rows_cap_truncates_rows_not_counts(tmp_path):
    g0 = fs.make_graph(hub_deg=64)
    query = QUERIES["wedge"]
    qp = write_query(tmp_path, "wedge")
    eng = fs.open_engine(g0, E)
    sq = eng.standing_open(qp, l=2, rows_cap=3)
    v = next(v for v in range(300) if (v, HUB) not in g0["edges"] and v != ISOLATED and g0["labels"][v] == 0)
    nxt = fs.apply_edges_np(g0, [(v, HUB)], [])
    M0, M1 = match_set(g0, query, False, False), match_set(nxt, query, False, False)
    assert len(M1 - M0) > 3
    eng.standing_apply_edges(insert=[(v, HUB)])
    count, created, destroyed, rows_c, rows_d, _ = sq.result()
    assert (count, created, destroyed, rows_c, rows_d) == (len(M1), len(M1 - M0), 0, 3, 0)
    rows = set(map(tuple, sq.rows(0).astype(np.int64).tolist()))
    assert len(rows) == 3 and rows <= (M1 - M0)
    assert len(sq.rows(0, cap=2)) == 2 and len(sq.rows(1)) == 0
    eng.close()


def test_gpu_staleness_and_refresh(tmp_path):
    from gnnpe_amd import binding
    g0 = fs.make_graph(hub_deg=64)
    query = QUERIES["wedge"]
    qp = write_query(tmp_path, "wedge")
    lab_bits = np.array([g0["labels"] == lb for lb in query[2]])
    eng = fs.open_engine(g0, E)
    sq = eng.standing_open(qp, l=2, induced=True, rows_cap=10)
    sets = eng.standing_open(qp, bitmap=pack(lab_bits), rows_cap=10)  # a label bitmap: sound for every edge batch
    assert sets.table() is None and sets.count == len(match_set(g0, query, False, False))
    have = sorted(g0["edges"])

    def stale_everywhere():
        for h in (sq, sets):
            for call in (h.result, h.bitmap, h.set_sizes, lambda: h.set_members(0), lambda: h.rows(0, cap=1), h.table_ptr):
                with pytest.raises(binding.GnnpeError, match="gnnpe_standing_refresh"):
                    call()
        with pytest.raises(binding.GnnpeError, match="gnnpe_standing_refresh"):
            sets.set_bitmap(pack(lab_bits))
        off = eng.download_csr()[0].tobytes()
        with pytest.raises(binding.GnnpeError, match="gnnpe_standing_refresh"):
            eng.standing_apply_edges(delete=have[50:51])
        assert eng.download_csr()[0].tobytes() == off, "a refused apply touched the graph"

    # a plain apply_edges behind the handles' back
    eng.apply_edges(delete=have[:5])
    cur = fs.apply_edges_np(g0, [], have[:5])
    stale_everywhere()
    with pytest.raises(binding.GnnpeError, match="gnnpe_vde"):  # refresh needs what open needs
        sq.refresh()
    eng.vde(want=False)
    assert sq.refresh() == len(match_set(cur, query, False, True))
    assert sets.refresh() == len(match_set(cur, query, False, False))
    # a relabel: the label bitmap of the open_sets handle is the caller's to renew
    verts = np.array([have[60][0], have[61][1], HUB], np.uint32)
    labels = cur["labels"].copy()
    labels[verts] = (labels[verts] + 1) % fs.NL
    eng.set_vertex_labels(verts, labels[verts])
    cur = fs.graph_of(cur["n"], cur["edges"], labels)
    stale_everywhere()
    eng.vde(want=False)
    count = sq.refresh()
    eng2 = fs.open_engine(cur, E)
    fresh = eng2.standing_open(qp, l=2, induced=True)
    assert count == fresh.count == len(match_set(cur, query, False, True))
    assert np.array_equal(sq.table(), fresh.table()) and np.array_equal(sq.bitmap(), fresh.bitmap())
    assert sq.result()[1:5] == (0, 0, 0, 0)
    eng2.close()
    sets.refresh()
    sets.set_bitmap(pack(np.array([labels == lb for lb in query[2]])))
    assert sets.count == len(match_set(cur, query, False, False))
    # a new label table
    eng.set_label_table(binding.host_label_table(fs.NL, E))
    stale_everywhere()
    eng.vde(want=False)
    assert sq.refresh() == count and sets.refresh() == sets.count
    # both go on exactly after the refresh
    nxt = fs.apply_edges_np(cur, [], have[70:72])
    eng.standing_apply_edges(delete=have[70:72])
    assert sq.count == len(match_set(nxt, query, False, True)) and sets.count == len(match_set(nxt, query, False, False))
    eng.close()


def test_gpu_refusals_at_open(tmp_path):
    from gnnpe_amd import binding
    g = fs.make_graph(hub_deg=64)
    qp = write_query(tmp_path, "wedge")
    two = str(tmp_path / "two_parts.graph")
    _write_query(two, 4, {(0, 1), (2, 3)}, [1, 0, 1, 0])
    ones = np.full((3, (g["n"] + 31) // 32), 0xFFFFFFFF, np.uint32)
    # a missing gnnpe_vde, and a missing label table
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    with pytest.raises(binding.GnnpeError, match="label table"):
        eng.standing_open(qp, l=2)
    eng.set_label_table(binding.host_label_table(fs.NL, E))
    with pytest.raises(binding.GnnpeError, match="gnnpe_vde"):
        eng.standing_open(qp, l=2)
    eng.vde(want=False)
    for bad_l in (1, 4):
        with pytest.raises(binding.GnnpeError, match=r"\[-3\]"):
            eng.standing_open(qp, l=bad_l)
    with pytest.raises(binding.GnnpeError, match="connected"):
        eng.standing_open(two, l=2)
    with pytest.raises(binding.GnnpeError, match="connected"):
        eng.standing_open(two, bitmap=np.full((4, ones.shape[1]), 0xFFFFFFFF, np.uint32))
    with pytest.raises(binding.GnnpeError, match="mode"):
        binding.StandingQuery(eng, qp, 2, 1e-6, 4, 0, None)
    assert eng._standing == [] and eng.standing_open(qp, l=2).count > 0  # the refusals left nothing behind
    eng.close()
    # a multigraph context
    eng = binding.Engine(0)
    dup_off = np.array([0, 2, 4], np.uint32)
    eng.load_multigraph(dup_off, np.array([1, 1, 0, 0], np.uint32), np.zeros(2, np.uint32))
    for kw in (dict(l=2), dict(bitmap=np.full((3, 1), 3, np.uint32))):
        with pytest.raises(binding.GnnpeError, match=r"\[-3\]"):
            eng.standing_open(qp, **kw)
    eng.close()
    # a slab-only context
    eng = binding.Engine(0)
    rows = np.arange(10, dtype=np.uint32)
    ro = np.concatenate([[0], np.cumsum(np.diff(g["offsets"].astype(np.int64))[:10])]).astype(np.uint64)
    eng.load_rows(g["n"], g["labels"], rows, ro, g["nbrs"][:int(ro[-1])])
    for kw in (dict(l=2), dict(bitmap=ones)):
        with pytest.raises(binding.GnnpeError, match=r"\[-3\]"):
            eng.standing_open(qp, **kw)
    eng.close()


# ---- 5. the existing entries are what they were ----------------------------------------------------------------------------------------

def test_gpu_existing_entries_unchanged(tmp_path):
    g0 = fs.make_graph(hub_deg=64)
    query = QUERIES["c4"]
    qp = write_query(tmp_path, "c4")
    bm = pack(np.array([g0["labels"] == lb for lb in query[2]]))
    edges = sorted(g0["edges"])[100:140]
    eng = fs.open_engine(g0, E)

    def answers():
        d = eng.refine_sets_delta(qp, bm, edges, matches_cap=100000, distinct=True)
        m = eng.refine_sets(qp, bm, limit=FULL, matches_cap=100000, induced=True)
        with eng.open_match_cursor(qp, bm, 97) as cur:
            pages = []
            while True:
                rows, done = cur.next()[:2]
                pages.append(np.asarray(rows).copy())
                if done:
                    break
        paged = np.concatenate(pages)
        return (d[0], sorted(map(tuple, d[1].tolist()))), (m[0], sorted(map(tuple, m[2].tolist()))), sorted(map(tuple, paged.tolist()))

    before = answers()
    assert before[0][0] > 0 and before[1][0] > 0 and len(before[2]) == len(match_set(g0, query, False, False, fs.bits_of(bm, g0["n"])))
    sq = eng.standing_open(qp, l=2, distinct=True, induced=True, rows_cap=1000)
    ins = [(a, b) for a in range(10, 14) for b in range(200, 203) if (a, b) not in g0["edges"]][:5]
    eng.standing_apply_edges(insert=ins)
    eng.standing_apply_edges(delete=ins)  # the graph of before again; the handle's buffers hold a batch's rows and its own sets
    kept = (sq.result(), sq.rows(1).tobytes(), sq.bitmap().tobytes(), sq.table().tobytes())
    assert answers() == before
    assert (sq.result(), sq.rows(1).tobytes(), sq.bitmap().tobytes(), sq.table().tobytes()) == kept, "the handle's buffers are its own"
    eng.close()


# ---- 6. CLI ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,mode", [([], (False, False)), (["-l", "3", "--refine", "sets", "--induced", "--distinct"], (True, True))])
def test_gpu_cli_standing(tmp_path, test_graph, flags, mode):
    """gnnpe_main -m online --exact --standing with three batch files on the Test graph: a `standing:` line for the open and one per
    batch, count / created / destroyed against brute force"""
    import os
    import subprocess
    from conftest import GOLDEN
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    qp = os.path.join(base.ONLINE, "q1.graph")
    lines = [ln.split() for ln in open(qp)]
    query = (int(lines[0][1]), {(int(ln[1]), int(ln[2])) for ln in lines if ln[0] == "e"}, [int(ln[2]) for ln in lines if ln[0] == "v"])
    n = len(test_graph["labels"])
    und = {(v, int(w)) for v in range(n) for w in test_graph["nbrs"][test_graph["offsets"][v]:test_graph["offsets"][v + 1]] if v < w}
    cur = fs.graph_of(n, und, test_graph["labels"])
    rng = np.random.default_rng(17)
    want, files = [(len(match_set(cur, query, *mode)), 0, 0)], []
    el = {(query[2][x], query[2][y]) for x, y in query[1]} | {(query[2][y], query[2][x]) for x, y in query[1]}
    fits = lambda e: (int(cur["labels"][e[0]]), int(cur["labels"][e[1]])) in el  # the labels of a query edge
    gone = []
    for i, (k_ins, k_del) in enumerate(((10, 10), (0, 25), (25, 0))):  # the third batch puts the second one's edges back
        have = [e for e in sorted(cur["edges"]) if fits(e)]
        dele = [have[int(j)] for j in rng.choice(len(have), k_del, replace=False)]
        ins = set(gone)
        while len(ins) < k_ins:
            a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False))
            if (a, b) not in cur["edges"] and fits((a, b)):
                ins.add((a, b))
        gone = dele if i == 1 else []
        files.append(str(tmp_path / f"batch{i}.txt"))
        open(files[-1], "w").write("".join(f"+ {a} {b}\n" for a, b in sorted(ins)) + "".join(f"- {a} {b}\n" for a, b in dele))
        mid = fs.apply_edges_np(cur, [], dele)
        nxt = fs.apply_edges_np(mid, ins, [])
        sets3 = [match_set(x, query, *mode) for x in (cur, mid, nxt)]
        created, destroyed = two_step(*sets3)
        want.append((len(sets3[2]), len(created), len(destroyed)))
        cur = nxt
    assert sum(w[1] for w in want) > 0 and sum(w[2] for w in want) > 0
    root = base._dataset(tmp_path, graph)
    head = [base.CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online"]
    cmd = head + ["--exact", "--standing"] + flags
    for f in files:
        cmd += ["--apply-edges", f]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("standing: ")]
    assert [tuple(int(x) for x in ln[1:4]) for ln in out] == want, (out, want)
    assert all(float(ln[4]) >= 0 for ln in out)
    # the flag's refusals, before a GPU is touched: no batch, --incremental, neither --exact nor -l 3
    for bad in (head + ["--exact", "--standing"], cmd + ["--incremental"], head + ["--standing", "--apply-edges", files[0]]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and ("--standing" in r.stderr + r.stdout or "--exact" in r.stderr + r.stdout), bad
