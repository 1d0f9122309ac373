"""The support table of the exact filter (gnnpe_filter_support_exact, gnnpe_filter_support_exact_delta, gnnpe_filter_support_bitmap)
and the three update loops that keep it exact, against numpy.

Yardstick 1: np_support -- directed_paths / matching_paths of tests/test_online_exact_fields.py (every directed simple path, the plan
as listed, no order), summed per (plan path, position) into a uint64 table; restricted to the paths through T for S_T.  It shares no
code with the library.  Yardstick 2, for bitmaps: gnnpe_filter_candidates_exact on a FRESH engine loaded with the final graph, after
set_order and vde.  The engines under test never get an order: the support calls must not need one.

Shapes: G(300, 1500) with 4 labels plus one hub joined to 150 vertices (n = 301: a multiple of neither 32 nor 64; the hub's row is
three chunks of 64 lanes, the last one partial), one vertex isolated; e in {1, 2, 3}, l in {2, 3}.  The edge loop wants a row that goes
from 64 to 65 entries and back, so its graph has the hub joined to 64 vertices instead.  The slices of k_support_walk want more
than 2^18 items and a row of more than 128 entries: 350 000 vertices, nearly all isolated, and a hub of 300 (sparse_hub_graph)."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_online_exact as base
import test_online_exact_fields as fields
from conftest import GOLDEN, ROOT
from test_online_exact import EPS, _write_query
from test_online_exact_fields import matching_paths

NL = 4
HUB, ISOLATED = 300, 17
CLI = base.CLI
LE = [(2, 1), (3, 1), (2, 2), (3, 2), (2, 3), (3, 3)]


# ---- graphs -----------------------------------------------------------------------------------------------------------------------

def graph_of(n, edges, labels):
    from gnnpe_amd import synth
    e = np.array(sorted(edges), np.int64).reshape(-1, 2)
    offs, nbrs = synth._csr_from_edges(n, e[:, 0], e[:, 1])
    return dict(n=n, m=len(e), offsets=offs, nbrs=nbrs, labels=np.asarray(labels, np.uint32).copy(), edges=set(edges))


def make_graph(hub_deg=150):
    from gnnpe_amd import synth
    g0 = synth.gnm_graph(300, 1500, n_labels=NL, seed=11)
    edges = {(int(a), int(b)) for a, b in zip(g0["eu"], g0["ev"]) if ISOLATED not in (int(a), int(b))}
    rng = np.random.default_rng(12)
    others = np.setdiff1d(np.arange(300), [ISOLATED])
    edges |= {(int(v), HUB) for v in rng.choice(others, hub_deg, replace=False)}
    labels = np.concatenate([g0["labels"], [1]])
    g = graph_of(301, edges, labels)
    deg = np.diff(g["offsets"].astype(np.int64))
    assert deg[HUB] == hub_deg and deg[ISOLATED] == 0 and g["n"] % 32 and g["n"] % 64
    return g


def nbrs_of(g, v):
    return g["nbrs"][g["offsets"][v]:g["offsets"][v + 1]].astype(np.int64)


def with_neighbours(g, R):
    return np.unique(np.concatenate([np.asarray(R, np.int64)] + [nbrs_of(g, int(v)) for v in R]))


def apply_edges_np(g, ins, dele):
    norm = lambda pairs: {(min(int(a), int(b)), max(int(a), int(b))) for a, b in pairs}
    I, D = norm(ins), norm(dele)
    assert not (I & g["edges"]) and D <= g["edges"]
    return graph_of(g["n"], (g["edges"] - D) | I, g["labels"])


def apply_vertices_np(g, rem, add_labels):
    """the graph after the batch and the new id of every old vertex (-1 for a removed one)"""
    rem = np.unique(np.asarray(rem, np.int64))
    keep = np.setdiff1d(np.arange(g["n"]), rem)
    new_id = np.full(g["n"], -1, np.int64)
    new_id[keep] = np.arange(len(keep))
    edges = {(int(new_id[a]), int(new_id[b])) for a, b in g["edges"] if new_id[a] >= 0 and new_id[b] >= 0}
    labels = np.concatenate([g["labels"][keep], np.asarray(add_labels, np.uint32)])
    return graph_of(len(keep) + len(add_labels), edges, labels), new_id


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------

def np_support(g, vde, plan, T=None, eps=EPS):
    """S (T None) or S_T of the contract: uint64 [n_query_vertices, n]"""
    nq, n = int(plan["n_vertices"]), g["n"]
    S = np.zeros((nq, n), np.uint64)
    in_t = None if T is None else np.isin(np.arange(n), np.asarray(T, np.int64))
    for part in ("main", "tri"):
        p = plan[part]
        for k in range(len(p["vids"])):
            rows = matching_paths(g, vde, p["labels"][k], p["degrees"][k], p["pde"][k], eps)
            if in_t is not None:
                rows = rows[in_t[rows].any(axis=1)]  # the paths with a vertex of T, each once
            for j, u in enumerate(p["vids"][k]):
                np.add.at(S[int(u)], rows[:, j], np.uint64(1))
    s = plan["single"]
    labels = np.asarray(g["labels"], np.int64)
    deg = np.diff(np.asarray(g["offsets"], np.int64))
    for i in range(len(s["vids"])):
        q = np.asarray(s["pde"][i], np.float64).reshape(1, -1)
        ok = (labels == int(s["labels"][i, 0])) & (deg >= int(s["degrees"][i, 0]))
        ok &= ~np.any((q > vde) & (np.abs(q - vde) > eps), axis=1)
        if in_t is not None:
            ok &= in_t
        S[int(s["vids"][i, 0])] += ok.astype(np.uint64)
    return S


def bits_of(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), bitorder="little").reshape(bm.shape[0], -1)[:, :n].astype(bool)


def to_np(table):
    return table.cpu().numpy().view(np.uint64)


def pattern(nq, n):
    import torch
    pat = (np.arange(nq * n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    return torch.from_numpy(pat.view(np.int64).reshape(nq, n).copy()).cuda(), pat.reshape(nq, n)


def open_engine(g, e):
    """the graph, the label table and the embeddings -- and NO order"""
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_label_table(binding.host_label_table(NL, e))
    eng.vde(want=False)
    return eng


def fresh_bits(g, e, plan, seed=5):
    """yardstick 2: the exact filter on a fresh engine with an order"""
    from gnnpe_amd import binding
    sn = np.random.default_rng(seed).permutation(g["n"]).astype(np.uint32)
    eng = base._engine(binding, g, sn, e)
    bm = eng.filter_candidates_exact(plan)[0]
    eng.close()
    return bits_of(bm, g["n"])


def vde_of(oracle, g, e):
    return oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)[2]


def make_plans(g, e, l, tmp_path, seed):
    """a query cut from the data graph, a star (at l = 3: the 3-vertex part) and a single edge (its two vertices lie on no plan
    path: the single entries)"""
    from gnnpe_amd import binding
    rng = np.random.default_rng(seed)
    out = []
    qp = str(tmp_path / f"cut_{l}_{e}_{seed}.graph")
    open(qp, "w").write(base._cut_query()(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], 5, rng))
    out.append(binding.host_query_plan_exact(qp, e, l))
    qp = str(tmp_path / f"star_{l}_{e}_{seed}.graph")
    _write_query(qp, 4, {(0, 1), (0, 2), (0, 3)}, [1, 0, 2, 1])
    out.append(binding.host_query_plan_exact(qp, e, l))
    qp = str(tmp_path / f"edge_{l}_{e}_{seed}.graph")
    _write_query(qp, 2, {(0, 1)}, [1, 3])
    out.append(binding.host_query_plan_exact(qp, e, l))
    assert len(out[0]["main"]["vids"]) and len(out[2]["single"]["vids"]) == 2
    assert l == 2 or len(out[1]["tri"]["vids"])
    return out


def label_plan(g, l, e, label):
    """hand-written: one single entry that asks for the label alone (degree 0, a zero embedding) -- the only test a vertex added
    with an empty row can pass, so the only way a vertex batch SETS a bit"""
    c = fields._case(g, np.zeros((g["n"], e)), [int(np.flatnonzero(g["labels"] == label)[0])])
    c["degrees"][:] = 0
    return fields.make_plan(l, e, [], [], [c])


class Moves:
    """what the loop tests must see ON THE YARDSTICK, so that they cannot pass vacuously"""

    def __init__(self):
        self.cleared = self.set = self.moved = 0

    def step(self, before, after, col_map=None):
        """col_map: for every column of `after` its column in `before` (-1: a new vertex)"""
        if col_map is not None:
            b = np.zeros_like(after)
            b[:, col_map >= 0] = before[:, col_map[col_map >= 0]]
            gone = np.setdiff1d(np.arange(before.shape[1]), col_map[col_map >= 0])
            self.cleared += int((before[:, gone] != 0).sum())
            before = b
        self.cleared += int(((before != 0) & (after == 0)).sum())
        self.set += int(((before == 0) & (after != 0)).sum())
        self.moved += int(((before != 0) & (after != 0) & (before != after)).sum())

    def check(self):
        assert self.cleared > 0 and self.set > 0 and self.moved > 0, (self.cleared, self.set, self.moved)


def check_tables(eng, g, vde, plan, table, e, what):
    """the carried table == the table recomputed on the engine == numpy's on g; the bitmap == the fresh filter's.  Returns numpy's"""
    want = np_support(g, vde, plan)
    got = to_np(table)
    again = to_np(eng.filter_support_exact(plan)[0])
    assert np.array_equal(again, want), (what, "recomputed")
    assert np.array_equal(got, want), (what, "carried", int((got != want).sum()))
    bm = eng.support_bitmap(table, int(plan["n_vertices"]))[0]
    assert bm.shape == (want.shape[0], (g["n"] + 31) // 32)
    assert not np.any(bm[:, -1] >> np.uint32(g["n"] % 32)), "bits past n"
    assert np.array_equal(bits_of(bm, g["n"]), want != 0), (what, "bitmap of the table")
    assert np.array_equal(bits_of(bm, g["n"]), fresh_bits(g, e, plan)), (what, "fresh filter")
    return want


# ---- 8. CPU -------------------------------------------------------------------------------------------------------------------------

NAMES = ("gnnpe_filter_support_exact", "gnnpe_filter_support_exact_delta", "gnnpe_filter_support_bitmap")


def test_symbols_are_exported_and_declared():
    from gnnpe_amd import binding
    binding.build()
    lib = binding.load()
    txt = open(os.path.join(ROOT, "include", "gnnpe_hip.h")).read()
    decl = set(re.findall(r"\b(gnnpe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in decl and name in binding.SIGNATURES, name
    assert lib.gnnpe_abi_version() == binding.ABI_VERSION == 20
    for method in ("filter_support_exact", "filter_support_delta", "support_bitmap"):
        assert callable(getattr(binding.Engine, method))


def test_loop_graphs_are_telling(oracle, tmp_path):
    """the conditions of the three loops hold on the yardstick for the seeds the GPU tests use (no GPU: numpy alone)"""
    for l, e in ((2, 2), (3, 1)):
        for scenario in (edge_scenario, relabel_scenario, vertex_scenario):
            g, steps = scenario()
            moves = Moves()
            for plan in make_plans(g, e, l, tmp_path, 31) + ([label_plan(g, l, e, 3)] if scenario is vertex_scenario else []):
                gb, before = g, np_support(g, vde_of(oracle, g, e), plan)
                for step in steps:
                    after = np_support(step["g"], vde_of(oracle, step["g"], e), plan)
                    moves.step(before, after, step.get("col_map"))
                    gb, before = step["g"], after
            moves.check()


# ---- the scenarios of the loops (numpy only) --------------------------------------------------------------------------------------------

def edge_scenario():
    """batches of 1, 8 and 64 mixed insertions and deletions; the first takes the hub's row from 64 to 65 entries, the second back"""
    g = make_graph(hub_deg=64)
    rng = np.random.default_rng(41)
    steps = []
    cur = g

    def draw(k_ins, k_del, forced_ins=(), forced_del=()):
        ins, dele = set(forced_ins), set(forced_del)
        have = sorted(cur["edges"])
        while len(dele) < k_del:
            a, b = have[int(rng.integers(len(have)))]
            if HUB not in (a, b):
                dele.add((a, b))
        while len(ins) < k_ins:
            a, b = sorted(int(x) for x in rng.choice(300, 2, replace=False))
            if (a, b) not in cur["edges"] and ISOLATED not in (a, b):
                ins.add((a, b))
        return sorted(ins), sorted(dele)

    free = next(v for v in range(300) if (v, HUB) not in g["edges"] and v != ISOLATED)
    for k_ins, k_del, f_ins, f_del in ((1, 0, [(free, HUB)], []), (4, 4, [], [(free, HUB)]), (32, 32, [], [])):
        ins, dele = draw(k_ins, k_del, f_ins, f_del)
        nxt = apply_edges_np(cur, ins, dele)
        steps.append(dict(g=nxt, ins=ins, dele=dele, T=np.unique(np.array(ins + dele, np.int64))))
        cur = nxt
    deg = [np.diff(s["g"]["offsets"].astype(np.int64))[HUB] for s in steps]
    assert deg[0] == 65 and deg[1] == 64 and [len(s["ins"]) + len(s["dele"]) for s in steps] == [1, 8, 64]
    return g, steps


def relabel_scenario():
    """the hub alone, then 8 vertices, then 24: each to the next label"""
    g = make_graph()
    rng = np.random.default_rng(43)
    steps, cur = [], g
    for R in ([HUB], rng.choice(300, 8, replace=False).tolist(), rng.choice(300, 24, replace=False).tolist()):
        labels = cur["labels"].copy()
        labels[R] = (labels[R] + 1) % NL
        nxt = graph_of(cur["n"], cur["edges"], labels)
        steps.append(dict(g=nxt, R=np.asarray(R, np.int64), labels=labels[R], T=with_neighbours(cur, R)))
        cur = nxt
    return g, steps


def vertex_scenario():
    """the hub and five others leave and two vertices arrive; then three leave and one arrives"""
    g = make_graph()
    rng = np.random.default_rng(47)
    steps, cur = [], g
    for rem, add in ((np.concatenate([[HUB], rng.choice(300, 5, replace=False)]), [1, 3]), (rng.choice(250, 3, replace=False), [0])):
        nxt, new_id = apply_vertices_np(cur, rem, add)
        T = with_neighbours(cur, rem)
        T2 = np.concatenate([new_id[T][new_id[T] >= 0], np.arange(nxt["n"] - len(add), nxt["n"])])
        col_map = np.full(nxt["n"], -1, np.int64)
        col_map[new_id[new_id >= 0]] = np.flatnonzero(new_id >= 0)
        steps.append(dict(g=nxt, rem=np.asarray(rem, np.int64), add=add, T=T, T2=T2, col_map=col_map))
        cur = nxt
    return g, steps


# ---- 1. the full table ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("l,e", LE)
def test_gpu_full_table(oracle, tmp_path, l, e):
    g = make_graph()
    vde = vde_of(oracle, g, e)
    eng = open_engine(g, e)
    for k, plan in enumerate(make_plans(g, e, l, tmp_path, 21)):
        table, ms = eng.filter_support_exact(plan)
        assert tuple(table.shape) == (int(plan["n_vertices"]), g["n"]) and ms >= 0.0
        want = check_tables(eng, g, vde, plan, table, e, ("full", l, e, k))
        assert (want != 0).any()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["l2", "l3", "tri"])
def test_gpu_full_table_plan_of_256_paths_and_refusal_at_257(oracle, mode):
    """256 hand-written plan paths, copies of 256 distinct data paths (512 after the exact filter's doubling): accepted, equal to
    numpy; 257: GNNPE_ERR_UNSUPPORTED and the table's bytes stay"""
    from gnnpe_amd import binding
    e = 2
    g = make_graph()
    vde = vde_of(oracle, g, e)
    eng = open_engine(g, e)
    l, W = (2, 3) if mode == "l2" else (3, 3 if mode == "tri" else 4)
    P = fields.path_index(g, W).P
    rng = np.random.default_rng(71)
    cases = [fields._case(g, vde, P[i]) for i in rng.choice(len(P), 257, replace=False)]
    build = lambda c: fields.make_plan(l, e, [], c) if mode == "tri" else fields.make_plan(l, e, c, [])
    plan = build(cases[:256])
    table, _ = eng.filter_support_exact(plan)
    want = check_tables(eng, g, vde, plan, table, e, ("256", mode))
    assert (want != 0).sum() >= 256 * W
    table, pat = pattern(int(build(cases)["n_vertices"]), g["n"])
    with pytest.raises(binding.GnnpeError, match="limit 512"):
        eng.filter_support_exact(build(cases), table=table)
    with pytest.raises(binding.GnnpeError, match="limit 512"):
        eng.filter_support_delta(build(cases), [0], 1, table)
    assert np.array_equal(to_np(table), pat)
    eng.close()


# ---- 2. S_T on a fixed graph ------------------------------------------------------------------------------------------------------------

def vertex_sets(g):
    adj = [set(nbrs_of(g, v).tolist()) for v in range(g["n"])]
    a, b = next((a, b) for a, b in sorted(g["edges"]) if HUB not in (a, b))
    tri = next((a, b, c) for a, b in sorted(g["edges"]) for c in sorted(adj[a] & adj[b]))
    cyc = next((a, b, c, d) for a in range(g["n"]) for b in sorted(adj[a]) for d in sorted(adj[a]) if b < d
               for c in sorted((adj[b] & adj[d]) - {a}))
    return dict(empty=[], one=[5], hub=[HUB], isolated=[ISOLATED], adjacent=[a, b], triangle=list(tri), cycle4=list(cyc),
                duplicates=[a, HUB, a, b, HUB, a], everything=list(range(g["n"])))


@pytest.mark.gpu
@pytest.mark.parametrize("l,e", LE)
def test_gpu_delta_on_a_fixed_graph(oracle, tmp_path, l, e):
    """S_T against numpy for every T of vertex_sets: from a table filled with a nonzero pattern, sign = +1 adds S_T (mod 2^64) and
    sign = -1 restores the caller's bytes; T = {} leaves them alone; T = V is the full table"""
    g = make_graph()
    vde = vde_of(oracle, g, e)
    eng = open_engine(g, e)
    sets = vertex_sets(g)
    for k, plan in enumerate(make_plans(g, e, l, tmp_path, 21)):
        nq = int(plan["n_vertices"])
        full = np_support(g, vde, plan)
        table, pat = pattern(nq, g["n"])
        for name, T in sets.items():
            want = np_support(g, vde, plan, T)
            ms = eng.filter_support_delta(plan, T, +1, table)
            got = to_np(table) - pat  # wrapping
            assert np.array_equal(got, want), (name, l, e, k, int((got != want).sum()))
            if name == "empty":
                assert ms == 0.0 and not want.any()
            if name == "everything":
                assert np.array_equal(want, full)
            if name == "duplicates":
                assert np.array_equal(want, np_support(g, vde, plan, sorted(set(T))))
            eng.filter_support_delta(plan, T, -1, table)
            assert np.array_equal(to_np(table), pat), (name, "restored")
        if k == 0:  # paths hold T-vertices at every position: more than one T-vertex on a path, each path still once
            assert np_support(g, vde, plan, sets["triangle"]).sum() < sum(np_support(g, vde, plan, [v]).sum() for v in sets["triangle"])
    eng.close()


# ---- 3 - 5. the loops ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("l,e", LE)
def test_gpu_edge_loop(oracle, tmp_path, l, e):
    g, steps = edge_scenario()
    moves = Moves()
    for k, plan in enumerate(make_plans(g, e, l, tmp_path, 31)):
        eng = open_engine(g, e)
        table, _ = eng.filter_support_exact(plan)
        before = check_tables(eng, g, vde_of(oracle, g, e), plan, table, e, ("edges", k, "start"))
        for i, s in enumerate(steps):
            eng.filter_support_delta(plan, s["T"], -1, table)
            eng.apply_edges(insert=s["ins"], delete=s["dele"])
            eng.vde(want=False)
            eng.filter_support_delta(plan, s["T"], +1, table)
            after = check_tables(eng, s["g"], vde_of(oracle, s["g"], e), plan, table, e, ("edges", k, i))
            moves.step(before, after)
            before = after
        eng.close()
    moves.check()


@pytest.mark.gpu
@pytest.mark.parametrize("l,e", LE)
def test_gpu_relabel_loop(oracle, tmp_path, l, e):
    g, steps = relabel_scenario()
    moves = Moves()
    for k, plan in enumerate(make_plans(g, e, l, tmp_path, 31)):
        eng = open_engine(g, e)
        table, _ = eng.filter_support_exact(plan)
        before = np_support(g, vde_of(oracle, g, e), plan)
        for i, s in enumerate(steps):
            eng.filter_support_delta(plan, s["T"], -1, table)
            eng.set_vertex_labels(s["R"], s["labels"])
            eng.vde(want=False)
            eng.filter_support_delta(plan, s["T"], +1, table)
            after = check_tables(eng, s["g"], vde_of(oracle, s["g"], e), plan, table, e, ("relabel", k, i))
            moves.step(before, after)
            before = after
        eng.close()
    moves.check()


@pytest.mark.gpu
@pytest.mark.parametrize("l,e", LE)
def test_gpu_vertex_loop(oracle, tmp_path, l, e):
    import torch
    g, steps = vertex_scenario()
    moves = Moves()
    for k, plan in enumerate(make_plans(g, e, l, tmp_path, 31) + [label_plan(g, l, e, 3)]):
        nq = int(plan["n_vertices"])
        eng = open_engine(g, e)
        table, _ = eng.filter_support_exact(plan)
        before = np_support(g, vde_of(oracle, g, e), plan)
        for i, s in enumerate(steps):
            eng.filter_support_delta(plan, s["T"], -1, table)
            assert not to_np(table)[:, s["rem"]].any()  # the columns of R hold zero: the carry loses nothing
            n2 = eng.apply_vertices(remove=s["rem"], add_labels=s["add"])[0]
            assert n2 == s["g"]["n"]
            carried = torch.zeros((nq, n2), dtype=torch.int64, device=table.device)
            torch.cuda.synchronize()
            eng.carry_vertices(table, carried, nq, 8)
            table = carried
            eng.vde(want=False)
            eng.filter_support_delta(plan, s["T2"], +1, table)
            after = check_tables(eng, s["g"], vde_of(oracle, s["g"], e), plan, table, e, ("vertices", k, i))
            moves.step(before, after, s["col_map"])
            before = after
        eng.close()
    moves.check()


# ---- 5b. the slices of an anchor's row -----------------------------------------------------------------------------------------------

_SPARSE = {}
SPARSE_N, SPARSE_CORE, SPARSE_HUB_DEG = 350000, 600, 300


def sparse_hub_graph():
    """350 000 vertices, all but the first 600 isolated: G(600, 900) with four labels, vertex 300 (label 1) joined to 300 of the
    others -- a row of five chunks of 64 lanes.  The yardstick's path join drops the isolated vertices at its first step."""
    if not _SPARSE:
        from gnnpe_amd import synth
        g0 = synth.gnm_graph(SPARSE_CORE, 900, n_labels=NL, seed=13)
        rng = np.random.default_rng(14)
        edges = {(int(a), int(b)) for a, b in zip(g0["eu"], g0["ev"])}
        others = np.setdiff1d(np.arange(SPARSE_CORE), [HUB])
        keep = {e for e in edges if HUB not in e}
        keep |= {(min(int(v), HUB), max(int(v), HUB)) for v in rng.choice(others, SPARSE_HUB_DEG, replace=False)}
        labels = np.concatenate([g0["labels"], rng.integers(0, NL, SPARSE_N - SPARSE_CORE)]).astype(np.uint32)
        labels[HUB] = 1
        core = graph_of(SPARSE_CORE, keep, labels[:SPARSE_CORE])  # (the CSR of the core, then 349 400 empty rows)
        offsets = np.concatenate([core["offsets"], np.full(SPARSE_N - SPARSE_CORE, core["offsets"][-1], np.uint32)])
        _SPARSE["g"] = dict(core, n=SPARSE_N, offsets=offsets, labels=labels)
    return _SPARSE["g"]


def sparse_vde(oracle, g, e):
    """the oracle's embeddings of sparse_hub_graph in milliseconds: an embedding is made of the vertex' label and its row, so an
    isolated vertex has the embedding of its label.  The oracle runs on the core with one isolated vertex per label appended, and
    the 349 400 isolated vertices take the row of their label (equal to the oracle's run on the whole graph bit for bit; that run
    takes more than a second)"""
    C = SPARSE_CORE
    offs = np.concatenate([g["offsets"][:C + 1], np.full(NL, g["offsets"][C], np.uint32)])
    small = oracle.gen_vde(offs, g["nbrs"], np.concatenate([g["labels"][:C], np.arange(NL)]).astype(np.uint32), e)[2]
    vde = small[C:][g["labels"]]
    vde[:C] = small[:C]
    return vde


@pytest.mark.gpu
@pytest.mark.parametrize("want_slices", [3, 2])
@pytest.mark.parametrize("l", [2, 3])
def test_gpu_delta_slices_stride_over_a_long_row(oracle, tmp_path, l, want_slices):
    """k_support_walk cuts the anchor's own row into slices: slice s of n_slices takes the chunks s, s + n_slices, ...  With a list
    of more than 2^18 ids the host gives every item 2 or 3 slices (about 2^20 waves in all), and the hub's row of 300 entries has
    five chunks: a slice takes a SECOND chunk, n_slices lanes-of-64 further on.  Every other test has at most 301 items (64 slices)
    and rows of at most 150 entries, so there the stride never ran.  S_T against np_support, sign +1 and back with -1.
    Wall time on one MI355X (pytest --durations, call phase, the cases in the order of this file, beside test_gpu_counts_loop_
    against_brute_force of tests/test_standing_counts.py, whose slowest case took 0.22 - 0.34 s): [2-3] 0.08 s, [2-2] 0.07 s, [3-3]
    0.20 s, [3-2] 0.09 s; no case may take more than twice that test's slowest case.  (Run as the first GPU test of a process, a
    case also pays the start-up of the runtime, about 0.4 s, as any first test does.)"""
    from gnnpe_amd import binding
    e = 2
    g = sparse_hub_graph()
    n, deg = g["n"], np.diff(g["offsets"].astype(np.int64))
    assert deg[HUB] == SPARSE_HUB_DEG and (deg[SPARSE_CORE:] == 0).all()
    vde = sparse_vde(oracle, g, e)
    eng = open_engine(g, e)
    assert eng.rows_held()[2] >= 1, "no hub row: the host would not slice"
    qp = str(tmp_path / "star.graph")
    _write_query(qp, 4, {(0, 1), (0, 2), (0, 3)}, [1, 0, 2, 1])
    P = fields.path_index(g, l + 1).P
    through = P[(P == HUB).any(axis=1)]
    rng = np.random.default_rng(15)
    picked = through[rng.choice(len(through), 3, replace=False)]
    assert len(set(np.argmax(through == HUB, axis=1).tolist())) == l + 1  # the hub at every position: every anchor J walks its row
    plans = [binding.host_query_plan_exact(qp, e, l), fields.make_plan(l, e, [fields._case(g, vde, r) for r in picked], [])]
    row = nbrs_of(g, HUB)
    isolated = np.arange(SPARSE_CORE, n)
    if want_slices == 3:
        T = np.concatenate([isolated[:(1 << 18) + 60], [HUB], row[::7], [5, 9]])
    else:
        T = np.concatenate([isolated, [HUB], row[::3], np.arange(0, SPARSE_CORE, 2)])
    T = np.unique(T)
    n_slices = min(64, max(1, (1 << 20) // len(T)))  # the host's rule for a list on a graph with hub rows
    assert len(T) > 1 << 18 and n_slices == want_slices, (len(T), n_slices)
    assert deg[HUB] > n_slices * 64, "no slice would take a second chunk"
    assert HUB in T and np.isin(row, T).any() and not np.isin(row, T).all()
    for k, plan in enumerate(plans):
        nq = int(plan["n_vertices"])
        want = np_support(g, vde, plan, T)
        assert want[:, HUB].any() and want[:, row[n_slices * 64:]].any(), (l, k, "the yardstick has nothing behind the first chunks")
        table, pat = pattern(nq, n)
        eng.filter_support_delta(plan, T, +1, table)
        got = to_np(table) - pat  # wrapping
        assert np.array_equal(got, want), (l, k, n_slices, int((got != want).sum()), int(got.sum()), int(want.sum()))
        eng.filter_support_delta(plan, T, -1, table)
        assert np.array_equal(to_np(table), pat), (l, k, n_slices, "restored")
    eng.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_refusals_leave_the_table_alone(oracle, tmp_path):
    import ctypes as C
    from gnnpe_amd import binding
    e, l = 2, 3
    g = make_graph()
    eng = open_engine(g, e)
    plan = make_plans(g, e, l, tmp_path, 21)[0]
    nq, n = int(plan["n_vertices"]), g["n"]
    table, pat = pattern(nq, n)
    bad = lambda **kw: dict(plan, **kw)
    part = lambda name, **kw: dict(plan[name], **kw)
    v_big = plan["main"]["vids"].copy()
    v_big[0, 0] = nq
    zeros = lambda rows, width: dict(vids=np.zeros((rows, width), np.uint32), labels=np.zeros((rows, width), np.uint32),
                                     degrees=np.zeros((rows, width), np.uint32), pde=np.zeros((rows, width * e)))
    lone = zeros(nq + 1, 1)  # more single entries than query vertices
    tri_at_2 = dict(binding.host_query_plan_exact(str(tmp_path / "cut_3_2_21.graph"), e, 2), tri=zeros(1, 3))
    cases = [(bad(l=4), "2 or 3"), (tri_at_2, "complement paths at l = 2"), (bad(main=part("main", vids=v_big)), "query path vertex"),
             (bad(single=lone), "single query vertices")]
    for p, msg in cases:
        with pytest.raises(binding.GnnpeError, match=msg):
            eng.filter_support_exact(p, table=table)
        with pytest.raises(binding.GnnpeError, match=msg):
            eng.filter_support_delta(p, [1, 2], 1, table)
    for tb in (0, table.data_ptr() + 4):  # null, not 8-byte aligned
        with pytest.raises(binding.GnnpeError, match="dev_table"):
            eng.filter_support_exact(plan, table=tb)
        with pytest.raises(binding.GnnpeError, match="dev_table"):
            eng.filter_support_delta(plan, [1], 1, tb)
        with pytest.raises(binding.GnnpeError, match="dev_table"):
            eng.support_bitmap(tb, nq)
    for sign in (0, 2, -2):
        with pytest.raises(binding.GnnpeError, match="sign"):
            eng.filter_support_delta(plan, [1], sign, table)
    with pytest.raises(binding.GnnpeError, match="not a vertex"):
        eng.filter_support_delta(plan, [1, n], 1, table)
    # a null list with a count: the raw call
    lq, counts, v, lb, d, pde, nv = eng._exact_plan_args(plan)
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    ptr = lambda a, t: a.ctypes.data_as(t)
    rc = eng.lib.gnnpe_filter_support_exact_delta(eng.ctx, lq, counts, ptr(v, u32p), ptr(lb, u32p), ptr(d, u32p), ptr(pde, f64p), nv, EPS,
                                                  None, 3, 1, C.c_void_p(table.data_ptr()), None)
    assert rc == -1 and b"null vertex list" in eng.lib.gnnpe_last_error()
    assert np.array_equal(to_np(table), pat)
    # ... and the context still answers
    eng.filter_support_delta(plan, [HUB], 1, table)
    eng.filter_support_delta(plan, [HUB], -1, table)
    assert np.array_equal(to_np(table), pat)
    # no gnnpe_vde since the rows changed: what catches a caller who forgot it after an update
    a, b = sorted(g["edges"])[0]
    eng.apply_edges(delete=[(a, b)])
    for call in (lambda: eng.filter_support_exact(plan, table=table), lambda: eng.filter_support_delta(plan, [a, b], 1, table)):
        with pytest.raises(binding.GnnpeError, match="gnnpe_vde"):
            call()
    eng.vde(want=False)
    eng.filter_support_delta(plan, [a, b], 1, table)
    eng.filter_support_delta(plan, [a, b], -1, table)
    # the multigraph state
    g2 = apply_edges_np(g, [], [(a, b)])
    eng.set_multigraph_rows(g2["offsets"].astype(np.uint64), g2["nbrs"])
    for call in (lambda: eng.filter_support_exact(plan, table=table), lambda: eng.filter_support_delta(plan, [1], 1, table),
                 lambda: eng.support_bitmap(table, nq)):
        with pytest.raises(binding.GnnpeError, match=r"\[-3\].*simple graphs only"):
            call()
    eng.close()
    # a slab-only context
    eng = binding.Engine(0)
    rows = np.arange(n, dtype=np.uint32)
    eng.load_rows(n, g["labels"], rows, g["offsets"].astype(np.uint64), g["nbrs"])
    eng.set_label_table(binding.host_label_table(NL, e))
    eng.vde(want=False)
    for call in (lambda: eng.filter_support_exact(plan, table=table), lambda: eng.filter_support_delta(plan, [1], 1, table),
                 lambda: eng.support_bitmap(table, nq)):
        with pytest.raises(binding.GnnpeError, match=r"\[-3\].*whole graph"):
            call()
    eng.close()
    assert np.array_equal(to_np(table), pat)


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["--apply-edges", "--set-labels", "--apply-vertices"])
def test_gpu_cli_incremental_equals_the_plain_run(tmp_path, test_graph, flag):
    """gnnpe_main -m filter --exact and -m online -l 3 with an update file: --incremental reports the candidate sets (candidates.bin)
    and the answer of the same command without it"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    g = dict(n=len(test_graph["labels"]), offsets=test_graph["offsets"], nbrs=test_graph["nbrs"], labels=test_graph["labels"])
    rng = np.random.default_rng(81)
    deg = np.diff(g["offsets"].astype(np.int64))
    und = np.array([(v, int(w)) for v in range(g["n"]) for w in nbrs_of(g, v) if v < w])
    f = str(tmp_path / "batch.txt")
    if flag == "--apply-edges":
        have = {tuple(p) for p in und.tolist()}
        ins = set()
        while len(ins) < 10:
            a, b = sorted(int(x) for x in rng.choice(g["n"], 2, replace=False))
            if (a, b) not in have:
                ins.add((a, b))
        dele = und[rng.choice(len(und), 10, replace=False)]
        open(f, "w").write("".join(f"+ {a} {b}\n" for a, b in sorted(ins)) + "".join(f"- {a} {b}\n" for a, b in dele.tolist()))
    elif flag == "--set-labels":
        nl = int(g["labels"].max()) + 1
        S = np.unique(np.concatenate([[int(np.argmax(deg))], rng.choice(g["n"], 8, replace=False)]))
        open(f, "w").write("".join(f"{v} {(int(g['labels'][v]) + 1) % nl}\n" for v in S.tolist()))
    else:
        rem = np.unique(np.concatenate([[int(np.argmax(deg))], rng.choice(g["n"], 6, replace=False)]))
        open(f, "w").write("".join(f"- {v}\n" for v in rem.tolist()) + "+ 0\n+ 1\n")
    root = base._dataset(tmp_path, graph)
    qp = os.path.join(base.ONLINE, "q1.graph")
    strip = lambda s: [ln.split(" Query Time")[0] for ln in s.splitlines()]
    for tail in (["-m", "filter", "--exact"], ["-m", "online", "-l", "3"]):
        seen = []
        for extra in ([], ["--incremental"]):
            r = subprocess.run([CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", flag, f] + tail + extra, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
            cand = open(os.path.join(root, "gnn-pe", "candidates.bin"), "rb").read() if tail[1] == "filter" else b""
            seen.append((strip(r.stdout), cand))
        assert seen[0] == seen[1], (flag, tail)
        assert tail[1] == "filter" and len(seen[0][1]) > 8 or any(ln.startswith("Answer Number: ") for ln in seen[0][0])


def test_cli_refuses_incremental_without_an_update(tmp_path):
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = base._dataset(tmp_path, graph)
    qp = os.path.join(base.ONLINE, "q1.graph")
    r = subprocess.run([CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "filter", "--exact", "--incremental"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--incremental applies with" in r.stderr + r.stdout
