"""The exact online filter (gnnpe_filter_candidates_exact: k_filter_starts4, k_filter_starts with a doubled plan, k_filter_vertices)
field by field against brute force.

tests/test_online_exact.py feeds the filter planner plans of queries cut out of the data graph: their degrees and embeddings lie
strictly inside the data's, their plans hold a handful of paths, and no single field of a plan path ever decides a bit.  Here the
plans are written by hand: every plan path is a copy of one directed data path with ONE field moved onto, just inside or just outside
its threshold, and every plan path has query-vertex ids of its own, so that one launch decides hundreds of cases independently.

Yardstick: brute_exact_sets, the exact contract over every DIRECTED simple path, plan paths forwards only, in numpy -- no order, no
slab, none of the oracle's C.  That it equals the library's doubled plan over one-orientation enumeration is what is under test.
The prune stages of the path kernels ask whether ANY plan path still fits a prefix, so a field decides there only in a plan that holds
nothing else: the "solo" calls of test_gpu_one_field_decides and the plan-size test (fillers with an unknown label)."""
import numpy as np
import pytest

import test_online_exact as base
from test_online_exact import EPS, _check_sets, _write_query, oracle_exact_sets

CHUNK = 256  # plan paths per call: 512 with their reverses, the whole LDS plan


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

def directed_paths(offsets, nbrs, W):
    """every directed simple path of W vertices (P x W int64): the CSR rows joined W - 1 times, no vertex repeated"""
    offs = np.asarray(offsets, np.int64)
    nb = np.asarray(nbrs, np.int64)
    deg = np.diff(offs)
    P = np.arange(len(deg), dtype=np.int64)[:, None]
    for _ in range(W - 1):
        cnt = deg[P[:, -1]]
        rep = np.repeat(np.arange(len(P)), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        nxt = nb[offs[P[rep, -1]] + within]
        keep = np.all(P[rep] != nxt[:, None], axis=1)
        P = np.column_stack([P[rep][keep], nxt[keep]])
    return P


class PathIndex:
    """the directed W-paths of a graph grouped by their label tuple"""

    def __init__(self, g, W):
        lab = np.asarray(g["labels"], np.int64)
        self.nl = int(lab.max()) + 1 if len(lab) else 1
        P = directed_paths(g["offsets"], g["nbrs"], W)
        key = np.zeros(len(P), np.int64)
        for j in range(W):
            key = key * self.nl + lab[P[:, j]]
        order = np.argsort(key, kind="stable")
        self.P, key = P[order], key[order]
        uniq, first = np.unique(key, return_index=True)
        ends = list(first[1:]) + [len(key)]
        self.groups = {int(k): (int(a), int(b)) for k, a, b in zip(uniq, first, ends)}

    def with_labels(self, labels):
        key = 0
        for lb in labels:
            if int(lb) >= self.nl:
                return self.P[:0]
            key = key * self.nl + int(lb)
        a, b = self.groups.get(key, (0, 0))
        return self.P[a:b]


_INDEX = {}


def path_index(g, W):
    key = (W, g["offsets"].tobytes(), g["nbrs"].tobytes(), g["labels"].tobytes())
    if key not in _INDEX:
        if len(_INDEX) >= 6:
            _INDEX.pop(next(iter(_INDEX)))
        _INDEX[key] = PathIndex(g, W)
    return _INDEX[key]


def matching_paths(g, vde, labels, degrees, pde, eps):
    """the directed data paths that pass one plan path, in the orientation given: labels equal, query degree <= CSR degree, in no
    dimension q > d and |q - d| > eps, at every position"""
    W = len(labels)
    deg = np.diff(np.asarray(g["offsets"], np.int64))
    cand = path_index(g, W).with_labels(labels)
    cand = cand[np.all(deg[cand] >= np.asarray(degrees, np.int64)[None, :], axis=1)]
    q = np.asarray(pde, np.float64).reshape(1, W, -1)
    d = vde[cand]
    return cand[~np.any((q > d) & (np.abs(q - d) > eps), axis=(1, 2))]


def brute_exact_sets(g, vde, plan, eps=EPS):
    """candidate sets of the exact contract (sorted uint32 arrays, one per query vertex)"""
    nq = int(plan["n_vertices"])
    labels = np.asarray(g["labels"], np.int64)
    deg = np.diff(np.asarray(g["offsets"], np.int64))
    got = [[] for _ in range(nq)]
    for part in ("main", "tri"):
        p = plan[part]
        for k in range(len(p["vids"])):
            rows = matching_paths(g, vde, p["labels"][k], p["degrees"][k], p["pde"][k], eps)
            for j, u in enumerate(p["vids"][k]):
                got[int(u)].append(rows[:, j])
    s = plan["single"]
    for i in range(len(s["vids"])):
        q = np.asarray(s["pde"][i], np.float64)[None, :]
        ok = (labels == int(s["labels"][i, 0])) & (deg >= int(s["degrees"][i, 0]))
        ok &= ~np.any((q > vde) & (np.abs(q - vde) > eps), axis=1)
        got[int(s["vids"][i, 0])].append(np.flatnonzero(ok))
    return [np.unique(np.concatenate(x)).astype(np.uint32) if x else np.zeros(0, np.uint32) for x in got]


# ---- hand-written plans -------------------------------------------------------------------------------------------------------------

def _case(g, vde, src, kind="base", pos=None, what="base"):
    src = np.asarray(src, np.int64)
    deg = np.diff(np.asarray(g["offsets"], np.int64))
    return dict(src=src, labels=np.asarray(g["labels"], np.int64)[src].copy(), degrees=deg[src].copy(), pde=vde[src].copy(),
                kind=kind, pos=pos, what=what)


def mutations(g, vde, src, mode):
    """copies of the data path / vertex `src` with one field changed.  kind "outside": `src` must stop matching; "inside" and "base":
    it must still match.  mode "eps": the calls with the default epsilon; "zero": eps = 0.0; "one": eps = 1.0"""
    W, e = len(src), vde.shape[1]
    nl = max(int(g["labels"].max()) + 1, 2)
    out = []
    if mode != "one":
        out.append(_case(g, vde, src))  # every degree and every embedding value exactly equal
    for j in range(W):
        if mode == "eps":
            c = _case(g, vde, src, "outside", j, f"label@{j}")
            c["labels"][j] = (c["labels"][j] + 1) % nl
            out.append(c)
            c = _case(g, vde, src, "outside", j, f"degree+1@{j}")
            c["degrees"][j] += 1
            out.append(c)
        for t in range(e):
            d = vde[src[j], t]
            moves = {"eps": (("inside", d + 0.5 * EPS, "+eps/2"), ("outside", d + 2 * EPS, "+2eps")),
                     "zero": (("outside", np.nextafter(d, np.inf), "nextafter"), ("inside", d - 1e-3, "-1e-3")),
                     "one": (("inside", d + 0.5, "+0.5"), ("outside", d + 2.0, "+2.0"))}[mode]
            for kind, value, name in moves:
                c = _case(g, vde, src, kind, j, f"{name}@{j}.{t}")
                c["pde"][j, t] = value
                out.append(c)
    return out


MODE_EPS = {"eps": EPS, "zero": 0.0, "one": 1.0}


def _part(cases, W, e, first_id):
    k = len(cases)
    part = dict(vids=(first_id + np.arange(k * W)).reshape(k, W).astype(np.uint32),
                labels=np.array([c["labels"] for c in cases], np.uint32).reshape(k, W),
                degrees=np.array([c["degrees"] for c in cases], np.uint32).reshape(k, W),
                pde=np.array([c["pde"].ravel() for c in cases], np.float64).reshape(k, W * e))
    return part, first_id + k * W


def make_plan(l, e, main=(), tri=(), single=()):
    """a plan dict as host_query_plan_exact returns it; every path and every single entry gets query-vertex ids of its own"""
    plan = dict(l=l, e=e)
    plan["main"], o = _part(main, l + 1, e, 0)
    plan["tri"], o = _part(tri, 3, e, o)
    plan["single"], o = _part(single, 1, e, o)
    plan["n_vertices"] = max(o, 1)
    return plan


def make_plans(l, e, main=(), tri=()):
    """the cases split at CHUNK paths per call, main and tri side by side"""
    return [make_plan(l, e, main[i:i + CHUNK], tri[i:i + CHUNK]) for i in range(0, max(len(main), len(tri), 1), CHUNK)]


def assert_telling(g, vde, cases, eps):
    """on the yardstick alone: base and inside cases are matched by their own source path; an outside case is not, and its source
    vertex at the changed position leaves that position's set.  Returns the number of cases of each kind"""
    seen = {"base": 0, "inside": 0, "outside": 0}
    for c in cases:
        rows = matching_paths(g, vde, c["labels"], c["degrees"], c["pde"].ravel(), eps)
        hit = bool(np.any(np.all(rows == c["src"][None, :], axis=1)))
        if c["kind"] == "outside":
            j = c["pos"]
            assert not hit and c["src"][j] not in rows[:, j], (c["what"], c["src"])
        else:
            assert hit, (c["what"], c["src"])
        seen[c["kind"]] += 1
    return seen


def sample_sources(g, W, sn, rng, count):
    """`count` directed W-paths, half with their first vertex before their last in the processing order `sn` (the device walks them
    as given) and half after (the device walks them backwards and reaches the plan path through its reversed copy)"""
    P = path_index(g, W).P
    rank = np.empty(len(sn), np.int64)
    rank[np.asarray(sn, np.int64)] = np.arange(len(sn))
    fwd = rank[P[:, 0]] < rank[P[:, -1]]
    a, b = np.flatnonzero(fwd), np.flatnonzero(~fwd)
    assert len(a) >= count // 2 and len(b) >= count - count // 2  # both situations occur
    pick = np.concatenate([rng.choice(a, count // 2, replace=False), rng.choice(b, count - count // 2, replace=False)])
    return [P[i] for i in pick]


def field_graph(e):
    from gnnpe_amd import synth
    g = synth.gnm_graph(300, 1200, n_labels=3, seed=5 + e)
    return g, np.random.default_rng(50 + e).permutation(g["n"]).astype(np.uint32)


def field_cases(g, vde, W, e, sn, mode):
    rng = np.random.default_rng(1000 + 10 * e + W)
    return [c for src in sample_sources(g, W, sn, rng, 12) for c in mutations(g, vde, src, mode)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------

def test_brute_force_equals_the_oracle_on_planner_plans(oracle, tmp_path):
    """three random graphs, random orders, planner plans of cut queries, a star and a single edge, l = 2 and 3, e = 1, 2, 8:
    the numpy yardstick == oracle_exact_sets (the oracle's C leaf test over one-orientation paths and their reverses)"""
    from gnnpe_amd import binding, synth
    cut_query = base._cut_query()
    rng = np.random.default_rng(2024)
    compared = 0
    for trial, (n, nl) in enumerate(((150, 2), (220, 3), (300, 4))):
        g = synth.gnm_graph(n, int(n * rng.uniform(3, 4)), n_labels=nl, seed=900 + trial)
        sn = rng.permutation(n).astype(np.uint32)
        qpaths = []
        for k in range(2):
            qp = str(tmp_path / f"c{trial}_{k}.graph")
            open(qp, "w").write(cut_query(g["offsets"].astype(np.int64), g["nbrs"], g["labels"], int(rng.integers(4, 8)), rng))
            qpaths.append(qp)
        qp = str(tmp_path / f"star{trial}.graph")
        _write_query(qp, 4, {(0, 1), (0, 2), (0, 3)}, rng.integers(0, nl, 4))
        qpaths.append(qp)
        qp = str(tmp_path / f"edge{trial}.graph")
        _write_query(qp, 2, {(0, 1)}, rng.integers(0, nl, 2))
        qpaths.append(qp)
        cache = {}
        for e in (1, 2, 8):
            _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
            for qp in qpaths:
                for l in (2, 3):
                    plan = binding.host_query_plan_exact(qp, e, l)
                    want = oracle_exact_sets(oracle, g, sn, vde, plan, cache)
                    got = brute_exact_sets(g, vde, plan, EPS)
                    assert len(got) == len(want)
                    for u in range(len(want)):
                        assert np.array_equal(got[u], want[u]), (trial, e, qp, l, u)
                    compared += sum(len(w) > 0 for w in want)
    assert compared > 200


@pytest.mark.parametrize("e", [1, 2, 8])
@pytest.mark.parametrize("W", [3, 4])
def test_crafted_cases_are_telling(oracle, W, e):
    """before any device sees them: every base and inside case is matched by its own source path, every outside case (label,
    degree + 1, + 2 eps / nextafter / + 2.0 in one dimension of one position) is not and changes the set of the changed position"""
    g, sn = field_graph(e)
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    seen = assert_telling(g, vde, field_cases(g, vde, W, e, sn, "eps"), EPS)
    assert seen == {"base": 12, "inside": 12 * W * e, "outside": 12 * W * (2 + e)}
    seen = assert_telling(g, vde, field_cases(g, vde, W, e, sn, "zero"), 0.0)
    assert seen == {"base": 12, "inside": 12 * W * e, "outside": 12 * W * e}
    seen = assert_telling(g, vde, field_cases(g, vde, W, e, sn, "one"), 1.0)
    assert seen == {"base": 0, "inside": 12 * W * e, "outside": 12 * W * e}


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------

def _open(oracle, g, sn, e, slab=None):
    """an engine on (g, sn) whose embeddings are bit-equal to the oracle's: what fails afterwards is the filter"""
    from gnnpe_amd import binding
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    eng = base._engine(binding, g, sn, e, slab=slab)
    assert np.array_equal(eng.vde()[2], vde)
    return eng, vde


def _check(bm, want, n, what):
    assert bm.shape == (len(want), (n + 31) // 32), what
    if n % 32:
        assert not np.any(bm[:, -1] >> np.uint32(n % 32)), ("bits past n", what)
    _check_sets(bm, want, n, what)


def _run(eng, g, vde, plans, eps, what):
    n = len(g["labels"])
    for i, plan in enumerate(plans):
        _check(eng.filter_candidates_exact(plan, eps=eps)[0], brute_exact_sets(g, vde, plan, eps), n, (what, i))


@pytest.mark.gpu
@pytest.mark.parametrize("e", [1, 2, 8])
@pytest.mark.parametrize("l", [2, 3])
def test_gpu_one_field_decides(oracle, l, e):
    """12 source paths (6 walked as given, 6 backwards), every position and dimension: label, degree + 1, degree equal, + eps/2,
    + 2 eps; with eps = 0: equal, nextafter, - 1e-3; with eps = 1: + 0.5, + 2.  At l = 3 the 3-vertex part gets the same in the
    same calls.  Then solo calls, a plan of one path: all equal, and + eps/2 at the first and the last position (the prune stages
    and the (s) stage's epsilon decide only there)"""
    g, sn = field_graph(e)
    eng, vde = _open(oracle, g, sn, e)
    W = l + 1
    for mode, eps in MODE_EPS.items():
        main = field_cases(g, vde, W, e, sn, mode)
        tri = field_cases(g, vde, 3, e, sn, mode) if l == 3 else []
        _run(eng, g, vde, make_plans(l, e, main, tri), eps, (l, e, mode))
    for width in ((W, 3) if l == 3 else (W,)):
        for src in sample_sources(g, width, sn, np.random.default_rng(1000 + 10 * e + width), 12):
            solo = [c for c in mutations(g, vde, src, "eps")
                    if c["kind"] == "base" or (c["kind"] == "inside" and c["pos"] in (0, width - 1)
                                               and c["what"].endswith((".0", f".{e - 1}")))]
            for eps in (EPS, 0.0):
                for c in (solo if eps else solo[:1]):
                    assert_telling(g, vde, [c], eps)
                    plan = make_plan(l, e, [c], []) if width == W else make_plan(l, e, [], [c])
                    _run(eng, g, vde, [plan], eps, (l, e, "solo", width, c["what"], eps))
    eng.close()


def _filler(g, vde, src, bad_pos, bad_label):
    """the labels of `src` with one label the graph does not have; degrees and embeddings 0, so every other test passes"""
    c = _case(g, vde, src, "outside", bad_pos, f"filler@{bad_pos}")
    c["labels"][bad_pos] = bad_label
    c["degrees"][:] = 0
    c["pde"][:] = 0.0
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["l3", "l2", "tri"])
def test_gpu_every_plan_size(oracle, mode):
    """plans of 1 .. 256 paths (2 .. 512 in LDS): one path that can match, first or last, among fillers that die at position
    0, 1, 2 or W - 1; then 256 distinct data paths at once.  The (s) stage of k_filter_starts4 walks the doubled plan 64 at a time"""
    from gnnpe_amd import synth
    e = 2
    g = synth.gnm_graph(300, 1200, n_labels=3, seed=7)
    sn = np.random.default_rng(70).permutation(g["n"]).astype(np.uint32)
    eng, vde = _open(oracle, g, sn, e)
    l, W = (2, 3) if mode == "l2" else (3, 3 if mode == "tri" else 4)
    rng = np.random.default_rng(71)
    sources = sample_sources(g, W, sn, rng, 8)
    unknown = int(g["labels"].max()) + 1
    turn = 0
    for count in ((256,) if mode == "tri" else (1, 32, 33, 64, 65, 128, 129, 256)):
        for place in ("first", "last"):
            for bad_pos in (0, 1, 2, W - 1):
                src = sources[(turn + turn // len(sources)) % len(sources)]  # every situation meets every orientation
                turn += 1
                real = _case(g, vde, src)
                assert_telling(g, vde, [real], EPS)
                fill = [_filler(g, vde, src, bad_pos, unknown) for _ in range(count - 1)]
                cases = [real] + fill if place == "first" else fill + [real]
                plan = make_plan(l, e, [], cases) if mode == "tri" else make_plan(l, e, cases, [])
                _run(eng, g, vde, [plan], EPS, (mode, count, place, bad_pos))
    P = path_index(g, W).P
    cases = [_case(g, vde, P[i]) for i in rng.choice(len(P), CHUNK, replace=False)]
    plan = make_plan(l, e, [], cases) if mode == "tri" else make_plan(l, e, cases, [])
    _run(eng, g, vde, [plan], EPS, (mode, "256 distinct"))
    eng.close()


HUB_SIZES = (1, 62, 63, 64, 65, 127, 128, 129)


def gadget_graph():
    """one label, disjoint gadgets.  Family 1: a centre s with two neighbours b1 < b2, b1 with a and b2 with b further neighbours c,
    every c with one tail, every other tail with a pendant (so that within one row some fourth vertices pass a degree-2 embedding
    and some do not).  Each (a, b) twice: s the smallest id of its gadget (first in the rows of b1 and b2: a first ballot of 63
    survivors) and s the largest (last: 63 queued, then a ballot of 64 -- the fill of 127).  Family 2: pendant - s - b - c with
    1, 64, 65, 130 further neighbours of c, every other one with a pendant.  Returns (graph, centres)"""
    from gnnpe_amd import synth
    pairs = [(a, 64) for a in HUB_SIZES] + [(63, b) for b in HUB_SIZES] + [(129, 129), (1, 1), (127, 128), (65, 62)]
    edges, centres = [], []
    nxt = 0
    for a, b in pairs:
        for s_first in (True, False):
            size = 3 + sum(2 * k + (k + 1) // 2 for k in (a, b))
            ids = list(range(nxt, nxt + size))
            nxt += size
            s = ids.pop(0) if s_first else ids.pop()
            it = iter(ids)
            b1, b2 = next(it), next(it)
            edges += [(s, b1), (s, b2)]
            for hub, k in ((b1, a), (b2, b)):
                for i in range(k):
                    c, t = next(it), next(it)
                    edges += [(hub, c), (c, t)]
                    if i % 2 == 0:
                        edges.append((t, next(it)))
            assert next(it, None) is None
            centres.append(s)
    for k in (1, 64, 65, 130):
        s, pend, b, c = nxt, nxt + 1, nxt + 2, nxt + 3
        nxt += 4
        edges += [(s, pend), (s, b), (b, c)]
        for i in range(k):
            edges.append((c, nxt))
            nxt += 1
            if i % 2 == 0:
                edges.append((nxt - 1, nxt))
                nxt += 1
        centres.append(s)
    eu, ev = np.array(edges, np.int64).T
    offs, nbrs = synth._csr_from_edges(nxt, eu, ev)
    g = dict(n=nxt, m=len(edges), offsets=offs, nbrs=nbrs, labels=np.zeros(nxt, np.uint32), eu=eu, ev=ev)
    return g, np.array(centres, np.int64)


@pytest.mark.gpu
def test_gpu_prefix_queue_and_long_rows(oracle):
    """one 4-path plan with all degrees 0 and the embedding of a data path of four degree-2 vertices: every prefix survives the
    prune stages, the queue fills to 63, 64, 126, 127 ..., and the leaf test decides tail by tail.  Centres first (the wave of s
    queues) and the reverse order both give the yardstick's sets"""
    e = 2
    g, centres = gadget_graph()
    n = g["n"]
    deg = np.diff(g["offsets"].astype(np.int64))
    assert deg.max() >= 130
    rest = np.setdiff1d(np.arange(n), centres)
    order = np.concatenate([centres, rest]).astype(np.uint32)
    P = path_index(g, 4).P
    src = next(p for p in P if p[0] in centres and np.all(deg[p] == 2))
    plan = None
    for sn in (order, order[::-1].copy()):
        eng, vde = _open(oracle, g, sn, e)
        if plan is None:
            c = _case(g, vde, src)
            c["degrees"][:] = 0
            plan = make_plan(3, e, [c], [])
            full = matching_paths(g, vde, c["labels"], c["degrees"], c["pde"].ravel(), EPS)
            loose = c["pde"].copy()
            loose[3] = 0.0  # any fourth vertex
            assert 0 < len(full) < len(matching_paths(g, vde, c["labels"], c["degrees"], loose.ravel(), EPS))
        _run(eng, g, vde, [plan], EPS, ("gadgets", int(sn[0])))
        eng.close()


def _small_graph(n):
    """n vertices, about n edges among them, two labels, some vertices isolated"""
    from gnnpe_amd import synth
    rng = np.random.default_rng(300 + n)
    pairs = set()
    while n >= 4 and len(pairs) < n:
        a, b = sorted(int(x) for x in rng.choice(n - n // 8, 2, replace=False))  # the last n / 8 ids stay isolated
        pairs.add((a, b))
    eu, ev = (np.array(sorted(pairs), np.int64).T if pairs else (np.zeros(0, np.int64), np.zeros(0, np.int64)))
    offs, nbrs = synth._csr_from_edges(n, eu, ev)
    labels = rng.integers(0, 2, n).astype(np.uint32)
    labels[0] = 0
    return dict(n=n, m=len(pairs), offsets=offs, nbrs=nbrs, labels=labels, eu=eu, ev=ev), rng


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 96, 97, 129])
def test_gpu_vertex_kernel_at_the_word_edges(oracle, n):
    """k_filter_vertices writes two bitmap words per wave: graphs of 1 .. 129 vertices, single entries with one field changed,
    whole, one-vertex, middle and empty slabs, a three-slab split; then a query vertex fed by a path kernel AND the vertex kernel"""
    e = 2
    g, rng = _small_graph(n)
    sn = rng.permutation(n).astype(np.uint32)
    deg = np.diff(g["offsets"].astype(np.int64))
    assert (deg == 0).any()
    verts = sorted({0, n - 1, int(np.argmax(deg)), int(sn[0]), int(sn[-1])} | {int(v) for v in rng.choice(n, min(n, 4), replace=False)})
    eng, vde = _open(oracle, g, sn, e)
    single = [c for v in verts for c in mutations(g, vde, [v], "eps")]
    plan = make_plan(2, e, [], [], single)
    want = brute_exact_sets(g, vde, plan, EPS)
    for u, c in enumerate(single):  # telling, on the reference
        assert (int(c["src"][0]) in want[u]) == (c["kind"] != "outside"), c["what"]
    whole = eng.filter_candidates_exact(plan)[0]
    eng.close()
    _check(whole, want, n, ("whole", n))
    thirds = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    acc = np.zeros_like(whole)
    for k, (a, b) in enumerate([(0, 1), (n - 1, n), (n // 2, n // 2)] + thirds):
        eng, _ = _open(oracle, g, sn, e, slab=(a, b))
        bm = eng.filter_candidates_exact(plan)[0]
        eng.close()
        own = np.zeros(n, bool)
        own[sn[a:b].astype(np.int64)] = True  # a slab sets bits only for its own vertices: the whole's, restricted
        _check(bm, [w[own[w.astype(np.int64)]] for w in want], n, ("slab", n, a, b))
        if k >= 3:
            acc |= bm
    assert np.array_equal(acc, whole)
    # one query vertex on a plan path and in `single`: the union; the vertex kernel's plain OR keeps what the path kernel set
    for l in (2, 3):
        P = path_index(g, l + 1).P
        if len(P) == 0:
            assert n < 31
            continue
        eng, _ = _open(oracle, g, sn, e)
        for src in P[rng.choice(len(P), min(len(P), 4), replace=False)]:
            path = _case(g, vde, src)
            other = _case(g, vde, [src[1]])
            other["labels"][0] = 1 - other["labels"][0]  # every vertex of the other label: never src[1]
            other["degrees"][:] = 0
            other["pde"][:] = 0.0
            plan = make_plan(l, e, [path], [], [other])
            plan["single"]["vids"][0, 0] = plan["main"]["vids"][0, 1]
            plan["n_vertices"] -= 1
            want = brute_exact_sets(g, vde, plan, EPS)
            by_path = matching_paths(g, vde, path["labels"], path["degrees"], path["pde"].ravel(), EPS)[:, 1]
            by_vertex = np.flatnonzero(g["labels"] == other["labels"][0])
            assert int(src[1]) in by_path and len(by_vertex) and not np.intersect1d(by_path, by_vertex).size
            assert np.array_equal(want[1], np.union1d(by_path, by_vertex).astype(np.uint32))
            assert np.intersect1d(by_path >> 5, by_vertex >> 5).size  # both kernels write one word
            _check(eng.filter_candidates_exact(plan)[0], want, n, ("shared id", n, l))
        eng.close()


@pytest.mark.gpu
def test_gpu_order_and_slab_invariance(oracle):
    """one plan of test_gpu_one_field_decides (l = 3, both parts), three random orders, whole and as the OR of three slabs:
    always the yardstick's sets, which know no order"""
    e = 2
    g, sn0 = field_graph(e)
    n = g["n"]
    _, _, vde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    plan = make_plans(3, e, field_cases(g, vde, 4, e, sn0, "eps"), field_cases(g, vde, 3, e, sn0, "eps"))[0]
    want = brute_exact_sets(g, vde, plan, EPS)
    assert sum(len(w) > 0 for w in want) > 100
    rng = np.random.default_rng(9)
    for trial in range(3):
        sn = rng.permutation(n).astype(np.uint32)
        cuts = sorted(int(x) for x in rng.choice(np.arange(1, n), 2, replace=False))
        eng, _ = _open(oracle, g, sn, e)
        _check(eng.filter_candidates_exact(plan)[0], want, n, ("whole", trial))
        eng.close()
        acc = None
        for a, b in zip([0] + cuts, cuts + [n]):
            eng, _ = _open(oracle, g, sn, e, slab=(a, b))
            bm = eng.filter_candidates_exact(plan)[0]
            eng.close()
            acc = bm if acc is None else acc | bm
        _check(acc, want, n, ("slabs", trial, cuts))
