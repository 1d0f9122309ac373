"""The paged cursor's POLL suspend (csrc/gnnpe_refine_pages.hip, the `(++steps & 1023u) == 0` branch of k_refine_pages): a wave that
has walked 1024 loop steps looks at the page cursor and, if the page is full, saves its state where it stands -- any depth, unvisited
survivors pending at several depths, cbase[d] in the middle of a pivot row -- and carries on in a later launch.  The graphs of
test_refine_pages.py, test_refine_distinct.py and test_refine_induced.py have rows of at most 155 entries: their subtrees end long
before 1024 steps and every suspension they see is a LEAF suspend.  The graphs here are built so that the search tree is known:

  * a FINDER, the start candidate with the highest id, reaches M matches within its first steps, all in one last-depth chunk: with
    page_rows < M it fills every page at once and leaf-suspends with a leftover mask;
  * W WALKERS, start candidates with smaller ids (their first-level items have lower ticket numbers, so their tickets are taken
    before the finder's can be), walk several times 1024 steps before their first match, and their matches sit in the last chunk
    of the last row they visit: a state that is lost, shifted or replayed changes the row set.

Families: (a) comb, 3-vertex path, the poll lands at the last depth among chunks of duds; (b) comb, 4-vertex path, the poll lands at
depth 2 or 3 with survivors pending at depths 1 and 2; (c) hub wedge in the four modes (plain, distinct, induced, both), the poll
lands at depth 2 in a hub row that the distinct forms have trimmed.  In (a) walker j is adjacent to the LAST K[j] teeth (not the
first): every walker then ends on the one tooth that carries leaves, so every walker has matches at its very end and none before.

Yardsticks: a plain numpy backtracking enumerator over the bitmap sets (_enumerate), pinned on the CPU to the constructions' closed
forms and to the host forms gnnpe_host_refine_sets*; and a Python model of the `while (d >= 1)` loop of k_refine_pages (_walk) that
counts loop steps, so the tests do not need to know how long a step takes: at page_rows = 1 the finder fills every page while it has
rows, so a walker's k-th poll suspends it exactly before its work step 1023 k + 1 (a resumed wave restarts `steps` at 0 and the
polling step does no work).  Two constructions are tuned with that: in (a) walker 0's sixth poll and in (b) walker 0's fifteenth
stand exactly before the chunk that holds the walker's matches, so a cursor that resumes one chunk too far loses rows; and in (a)
walker 1's matches are the 6 x 1024th chunk it evaluates, for a poll that counted chunks and not loop steps."""
import sys

import numpy as np
import pytest

import test_online_exact as ex
import test_refine_pages as rp
import test_refine_sets as rs
import test_refine_sets_shapes as sh

POLL = 1024  # k_refine_pages looks at the cursor every POLL loop steps
MODES = {"R": dict(distinct=False, induced=False), "D": dict(distinct=True, induced=False),
         "I": dict(distinct=False, induced=True), "ID": dict(distinct=True, induced=True)}

# ---- the constructions ------------------------------------------------------------------------------------------------------
# (a): W walkers, walker j adjacent to the last K[j] of T teeth; every tooth but the last holds ND duds (with its 1-4 walkers: 111
# chunks), the last tooth ND_LAST duds and the E leaves (149 chunks, the leaves in the last); the finder has one neighbour with M leaves.
# A walker's matches are its loop step 113 (K - 1) + 150 and the chunk 111 (K - 1) + 150 it evaluates: K = 54 gives step 6 x 1023 + 1,
# K = 55 chunk 6 x 1024.  914 176 adjacency entries
COMB_LEAF = dict(W=4, K=(54, 55, 60, 64), T=64, ND=7100, ND_LAST=9525, E=3, M=6)
# (b): walker j adjacent to the last K[j] of T teeth, every tooth adjacent to NM mids, every mid's row = the T teeth; the last tooth also
# to `mtop` (the highest-id member of C(u2)) whose row is that tooth and the E leaves; finder - f1 - f2 - M leaves
COMB_INNER = dict(W=4, K=(5, 6, 7, 8), T=8, NM=1023, E=3, M=30)
# (c): W hubs with rows [12 of L | ND duds | 3 of L] (101 chunks) and a finder hub with F of L.  Inside L, per hub: the 12 are a clique
# and all of them but the 10th and the 12th (FREE) are adjacent to the 3: in the induced modes the item of a hub's first chunk walks the
# hub's row 9 times without a match (103 steps each), is polled at step 1024 in the 10th walk, whose matches come in its last chunk
# (step 1029), and finds the 12th's matches, which were pending at depth 1 when it was polled, at the very end
HUB_WEDGE = dict(W=3, NA=12, NB=3, ND=6400, F=8, FREE=(9, 11))


def _graph(n, edges):
    from gnnpe_amd import synth
    e = np.concatenate([np.asarray(x, np.int64).reshape(-1, 2) for x in edges])
    offs, nbrs = synth._csr_from_edges(n, e[:, 0], e[:, 1])
    assert len(nbrs) == 2 * len(e) and len(np.unique(nbrs.astype(np.int64) + (np.repeat(np.arange(n), np.diff(offs)) << 32))) == len(nbrs)
    return dict(n=n, offsets=offs, nbrs=nbrs, labels=np.zeros(n, np.uint32))


def _pairs(a, b):
    """every (x, y) with x of a and y of b"""
    a, b = np.atleast_1d(np.asarray(a, np.int64)), np.atleast_1d(np.asarray(b, np.int64))
    return np.stack([np.repeat(a, len(b)), np.tile(b, len(a))], axis=1)


class _Ids:
    """hands out blocks of consecutive vertex ids: a block taken later has higher ids and so stands later in every row"""

    def __init__(self):
        self.n = 0

    def take(self, k):
        out = np.arange(self.n, self.n + k, dtype=np.int64)
        self.n += k
        return out


def _case(g, qp, sets, **kw):
    n = g["n"]
    bm = np.stack([sh._row_of(s, n) for s in sets])
    return dict(g=g, qp=qp, sets=[np.sort(np.asarray(s, np.int64)) for s in sets], bm=bm, **kw)


_CASES = {}


def _tmp(tmp_path_factory):
    if "tmp" not in _CASES:
        _CASES["tmp"] = tmp_path_factory.mktemp("suspend")
    return _CASES["tmp"]


def _comb_leaf(tmp_path_factory):
    if "a" in _CASES:
        return _CASES["a"]
    p = COMB_LEAF
    W, K, T, E, M = p["W"], p["K"], p["T"], p["E"], p["M"]
    ids = _Ids()
    walkers, finder, teeth, f1, fleaves = ids.take(W), ids.take(1), ids.take(T), ids.take(1), ids.take(M)
    duds, leaves = ids.take(max(p["ND"], p["ND_LAST"])), ids.take(E)
    edges = [_pairs(walkers[j], teeth[T - K[j]:]) for j in range(W)]
    edges += [_pairs(teeth[:-1], duds[:p["ND"]]), _pairs(teeth[-1], duds[:p["ND_LAST"]]), _pairs(teeth[-1], leaves)]
    edges += [_pairs(finder, f1), _pairs(f1, fleaves)]
    g = _graph(ids.n, edges)
    sets = [np.concatenate([walkers, finder]), np.concatenate([teeth, f1]), np.concatenate([fleaves, leaves])]
    items = {s: sum(-(-k // (1 << s)) for k in K) + 1 for s in (0, 3, 6)}
    _CASES["a"] = _case(g, sh._path_file(_tmp(tmp_path_factory), 3), sets, closed={"R": W * E + M}, W=W, M={"R": M}, E=E,
                        walkers=walkers, finder=int(finder[0]), cands=W + 1, items=items)
    return _CASES["a"]


def _comb_inner(tmp_path_factory):
    if "b" in _CASES:
        return _CASES["b"]
    p = COMB_INNER
    W, K, T, E, M = p["W"], p["K"], p["T"], p["E"], p["M"]
    ids = _Ids()
    walkers, finder, teeth, f1 = ids.take(W), ids.take(1), ids.take(T), ids.take(1)
    mids, mtop, f2, fleaves, leaves = ids.take(p["NM"]), ids.take(1), ids.take(1), ids.take(M), ids.take(E)
    edges = [_pairs(walkers[j], teeth[T - K[j]:]) for j in range(W)]
    edges += [_pairs(teeth, mids), _pairs(teeth[-1], mtop), _pairs(mtop, leaves), _pairs(finder, f1), _pairs(f1, f2), _pairs(f2, fleaves)]
    g = _graph(ids.n, edges)
    sets = [np.concatenate([walkers, finder]), np.concatenate([teeth, f1]), np.concatenate([mids, mtop, f2]),
            np.concatenate([fleaves, leaves])]
    _CASES["b"] = _case(g, sh._path_file(_tmp(tmp_path_factory), 4), sets, closed={"R": W * E + M}, W=W, M={"R": M}, E=E,
                        walkers=walkers, finder=int(finder[0]), cands=W + 1, items={6: W + 1})
    return _CASES["b"]


def _hub_wedge(tmp_path_factory):
    if "c" in _CASES:
        return _CASES["c"]
    p = HUB_WEDGE
    W, NA, NB, F = p["W"], p["NA"], p["NB"], p["F"]
    ids = _Ids()
    hubs, hf = ids.take(W), ids.take(1)
    a_of = [ids.take(NA) for _ in range(W)]
    fl = ids.take(F)
    d_of = [ids.take(p["ND"]) for _ in range(W)]
    b_of = [ids.take(NB) for _ in range(W)]
    edges = [_pairs(hf, fl)]
    for h in range(W):
        edges += [_pairs(hubs[h], np.concatenate([a_of[h], d_of[h], b_of[h]])), _pairs(np.delete(a_of[h], p["FREE"]), b_of[h])]
        edges += [np.array([(x, y) for i, x in enumerate(a_of[h]) for y in a_of[h][i + 1:]], np.int64)]
    g = _graph(ids.n, edges)
    L = np.concatenate(a_of + [fl] + b_of)
    k = NA + NB
    non = NB * len(p["FREE"]) + NB * (NB - 1) // 2  # non-adjacent pairs inside a hub's part of L: FREE with the 3, the 3 among themselves
    closed = {"R": W * k * (k - 1) + F * (F - 1), "D": (W * k * (k - 1) + F * (F - 1)) // 2, "I": W * 2 * non + F * (F - 1),
              "ID": W * non + F * (F - 1) // 2}
    chunks = -(-(NA + p["ND"] + NB) // 64)
    _CASES["c"] = _case(g, sh._shape_file(_tmp(tmp_path_factory), "wedge"), [L, np.concatenate([hubs, hf]), L], closed=closed, W=W,
                        M={"R": F * (F - 1), "D": F * (F - 1) // 2, "I": F * (F - 1), "ID": F * (F - 1) // 2}, walkers=hubs,
                        finder=int(hf[0]), cands=W + 1, items={6: W * chunks + 1})
    return _CASES["c"]


# ---- the reference: plain backtracking over the bitmap sets ---------------------------------------------------------------------

def _query(qp):
    from gnnpe_amd import binding
    q = binding.host_load_graph(qp)
    adj = [set(int(x) for x in q["nbrs"][q["offsets"][u]:q["offsets"][u + 1]]) for u in range(q["n"])]
    return q, adj


def _enumerate(c, distinct=False, induced=False):
    """every map of the query into the graph with each image in its vertex's set, of the right label and at least the query vertex's
    degree, injective, edges on edges; distinct: f(a) < f(b) for the pairs of host_query_symmetry; induced: the pairs of
    host_query_nonedges on non-edges.  Query vertices in id order of a breadth-first walk from vertex 0 -- not the library's order"""
    from gnnpe_amd import binding
    g, qp = c["g"], c["qp"]
    q, adj = _query(qp)
    nq, n = q["n"], g["n"]
    offs, nbrs = g["offsets"].astype(np.int64), g["nbrs"].astype(np.int64)
    deg = np.diff(offs)
    inset = np.zeros((nq, n), bool)
    for u in range(nq):
        inset[u, c["sets"][u]] = True
        inset[u] &= (g["labels"] == q["labels"][u]) & (deg >= len(adj[u]))
    less = [(int(a), int(b)) for a, b in binding.host_query_symmetry(qp)[1]] if distinct else []
    non = [(int(a), int(b)) for a, b in binding.host_query_nonedges(qp)] if induced else []
    order = [0]
    while len(order) < nq:
        order += sorted(u for u in range(nq) if u not in order and adj[u] & set(order))[:1]
    row = lambda v: nbrs[offs[v]:offs[v + 1]]
    out, image = [], {}

    def rec(i):
        if i == nq:
            out.append([image[u] for u in range(nq)])
            return
        u = order[i]
        earlier = [w for w in order[:i] if w in adj[u]]
        cand = row(image[earlier[0]]) if earlier else np.nonzero(inset[u])[0]
        cand = cand[inset[u, cand]]
        for w in earlier[1:]:
            cand = cand[np.isin(cand, row(image[w]))]
        for w in order[:i]:
            cand = cand[cand != image[w]]
            if (w, u) in non or (u, w) in non:
                cand = cand[~np.isin(cand, row(image[w]))]
            if (w, u) in less:
                cand = cand[cand > image[w]]
            if (u, w) in less:
                cand = cand[cand < image[w]]
        for v in cand:
            image[u] = int(v)
            rec(i + 1)
        image.pop(u, None)

    rec(0)
    return np.asarray(out, np.uint32).reshape(-1, nq)


def _reference(c, mode="R"):
    """the enumerator's rows of a case in a mode, computed once"""
    key = ("rows", mode)
    if key not in c:
        c[key] = _enumerate(c, **MODES[mode])
        c[key].setflags(write=False)
    return c[key]


# ---- the step model: the `while (d >= 1)` loop of k_refine_pages ----------------------------------------------------------------

def _match_order(c):
    """build_match_order (host/refine.h): start = fewest candidates, then larger degree, then smaller id; then always the unvisited
    vertex with the most visited neighbours (smaller id on a tie), its pivot its first earlier neighbour in the order.  Returns
    (order, pivot position per position)"""
    q, adj = _query(c["qp"])
    cnt = [len(s) for s in c["sets"]]
    start = 0
    for u in range(1, q["n"]):
        if cnt[u] < cnt[start] or (cnt[u] == cnt[start] and len(adj[u]) > len(adj[start])):
            start = u
    order, pivot = [start], [0]
    while len(order) < q["n"]:
        links = {u: len(adj[u] & set(order)) for u in range(q["n"]) if u not in order}
        best = min(links, key=lambda u: (-links[u], u))
        pivot.append(min(order.index(w) for w in adj[best] if w in order))
        order.append(best)
    return order, pivot


def _walk(c, v0, c0, c1, mode="R"):
    """One first-level item (start candidate v0, entries [c0, c1) of its row) walked as k_refine_pages walks it, one list entry per
    loop step: (kind, depth, matches) with kind "C" a chunk evaluated (and, above the last depth, the descent into its first
    survivor in the same step), "D" a descent into a pending survivor, "U" a row exhausted.  Also returns the rows found.  The
    distinct modes trim a pivot row longer than a chunk to its bounds when the depth is entered, as sets_descend does."""
    from gnnpe_amd import binding
    g, qp = c["g"], c["qp"]
    q, adj = _query(qp)
    order, pivot = _match_order(c)
    nq, last = q["n"], q["n"] - 1
    offs, nbrs = g["offsets"].astype(np.int64), g["nbrs"].astype(np.int64)
    deg = np.diff(offs)
    pos = {u: i for i, u in enumerate(order)}
    inset = np.zeros((nq, g["n"]), bool)
    for i, u in enumerate(order):
        inset[i, c["sets"][u]] = True
        inset[i] &= deg >= len(adj[u])
    m = MODES[mode]
    less = [(pos[int(a)], pos[int(b)]) for a, b in binding.host_query_symmetry(qp)[1]] if m["distinct"] else []
    non = [(pos[int(a)], pos[int(b)]) for a, b in binding.host_query_nonedges(qp)] if m["induced"] else []
    back = [[pos[w] for w in adj[order[i]] if pos[w] < i and pos[w] != pivot[i]] for i in range(nq)]
    row = lambda v: nbrs[offs[v]:offs[v + 1]]

    def bounds(d, image):
        lo = max([image[a] + 1 for a, b in less if b == d and a < d] + [0])
        hi = min([image[b] for a, b in less if a == d and b < d] + [1 << 32])
        return lo, hi

    image, cbase, end, mask = {0: v0}, {1: c0 - 64}, {1: c1}, {1: []}
    d, steps, rows = 1, [], []
    while d >= 1:
        if not mask[d]:
            cb = cbase[d] + 64
            if end[d] - cb <= 0:
                steps.append(("U", d, 0))
                d -= 1
                continue
            cbase[d] = cb
            idx = np.arange(cb, min(cb + 64, end[d]))
            v = nbrs[idx]
            ok = inset[d, v]
            lo, hi = bounds(d, image)
            ok &= (v >= lo) & (v < hi)
            for i in range(d):
                ok &= v != image[i]
            for b in back[d]:
                ok &= np.isin(v, row(image[b]))
            for a, b in non:
                if max(a, b) == d:
                    ok &= ~np.isin(v, row(image[min(a, b)]))
            if d == last:
                steps.append(("C", d, int(ok.sum())))
                rows += [[image[pos[u]] if pos[u] < d else int(x) for u in range(nq)] for x in v[ok]]
                continue
            steps.append(("C", d, 0))
            mask[d] = list(idx[ok])
            if not mask[d]:
                continue
        else:
            steps.append(("D", d, 0))
        image[d] = int(nbrs[mask[d].pop(0)])
        d += 1
        rb = int(offs[image[pivot[d]]])
        re = rb + int(deg[image[pivot[d]]])
        if m["distinct"] and re - rb > 64:
            lo, hi = bounds(d, image)
            r = nbrs[rb:re]
            rb, re = rb + int(np.searchsorted(r, lo)), rb + int(np.searchsorted(r, hi))
        cbase[d], end[d], mask[d] = rb - 64, re, []
    return steps, np.asarray(rows, np.uint32).reshape(-1, nq)


def _items(c, v0, shift):
    """the first-level items of a start candidate: chunks of 1 << shift entries of its row"""
    s, e = int(c["g"]["offsets"][v0]), int(c["g"]["offsets"][v0 + 1])
    return [(a, min(a + (1 << shift), e)) for a in range(s, e, 1 << shift)]


def _first_match(steps):
    """the 1-based loop step of an item's first match, None if it has none"""
    return next((i + 1 for i, s in enumerate(steps) if s[2]), None)


def _polled_steps(steps, polls):
    """at page_rows = 1 with a page that is full at every poll: the work steps before which polls 1 .. `polls` suspend the wave"""
    return [steps[(POLL - 1) * k] for k in range(1, polls + 1) if (POLL - 1) * k < len(steps)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def _host_count(c, mode):
    from gnnpe_amd import binding
    return binding.host_refine_sets(c["g"], c["qp"], c["bm"], limit=10 ** 7, **MODES[mode])


@pytest.mark.parametrize("family", ["a", "b", "c"])
def test_reference_rows_equal_the_closed_form_and_the_host_form(tmp_path_factory, family):
    """the enumerator's count is the construction's closed form and the host form's in every mode of the family; the rows are valid
    embeddings inside the sets and pairwise different; no case has more than 2 000 matches, no graph more than about a million
    adjacency entries; in (c) R, D, I and ID are pairwise different"""
    c = {"a": _comb_leaf, "b": _comb_inner, "c": _hub_wedge}[family](tmp_path_factory)
    assert len(c["g"]["nbrs"]) <= 1_050_000
    counts = {}
    for mode in (MODES if family == "c" else ("R",)):
        rows = _reference(c, mode)
        rs._assert_rows_are_embeddings(c["g"], c["qp"], c["bm"], rows)
        counts[mode] = len(rows)
        assert len(rows) == c["closed"][mode] == _host_count(c, mode), (family, mode, len(rows), c["closed"][mode])
        assert c["M"][mode] < len(rows) <= 2000
    if family == "c":
        assert len(set(counts.values())) == 4, counts
        assert sh._row_set(_reference(c, "ID")) < sh._row_set(_reference(c, "I")) < sh._row_set(_reference(c, "R"))
        assert sh._row_set(_reference(c, "ID")) < sh._row_set(_reference(c, "D")) < sh._row_set(_reference(c, "R"))
    # the match order the constructions count on: the start vertex is the one whose set holds walkers and finder
    order, _ = _match_order(c)
    assert len(c["sets"][order[0]]) == c["cands"] and c["finder"] == c["sets"][order[0]].max()


@pytest.mark.parametrize("family", ["a", "b"])
def test_step_model_of_the_combs(tmp_path_factory, family):
    """shift 6, where a walker is one item: the model's rows are the enumerator's; every walker takes at least 4 x 1024 steps, and
    at least (M - 1) x 1024 in (a), before its first match, which is the last chunk it evaluates; the finder reaches its M matches,
    all in one chunk, within 8 steps; the walkers' step counts are pairwise different modulo 1024.  The tuned poll: in (a) walker 0's
    sixth and in (b) walker 0's fifteenth poll at page_rows = 1 stand before the chunk that holds (or leads to) the walker's matches,
    while the finder still has rows; in (a) the chunk with walker 1's matches is the 6 x 1024th it evaluates"""
    c = {"a": _comb_leaf, "b": _comb_inner}[family](tmp_path_factory)
    M, E = c["M"]["R"], c["E"]
    found, first, total = [], [], []
    for v0 in list(c["walkers"]) + [c["finder"]]:
        items = _items(c, int(v0), 6)
        assert len(items) == 1
        steps, rows = _walk(c, int(v0), *items[0])
        found.append(rows)
        first.append(_first_match(steps))
        total.append(len(steps))
        if v0 == c["finder"]:
            assert first[-1] <= 8 and len(rows) == M and [s[2] for s in steps if s[2]] == [M]
        else:
            assert len(rows) == E and [s[2] for s in steps if s[2]] == [E]
            assert first[-1] >= max(4, M - 1 if family == "a" else 4) * POLL, (family, first)
            assert all(s[0] == "U" for s in steps[first[-1]:]), "the matches come in the last chunk the walker evaluates"
    print(f"family {family}: loop steps per item {total}, first match at {first}")
    assert sh._row_set(np.concatenate(found)) == sh._row_set(_reference(c)) and sum(map(len, found)) == len(_reference(c))
    assert len({t % POLL for t in total[:-1]}) == c["W"], total
    walker, poll = (0, 6) if family == "a" else (0, 15)
    assert poll <= M
    steps, _ = _walk(c, int(c["walkers"][walker]), *_items(c, int(c["walkers"][walker]), 6)[0])
    polled = _polled_steps(steps, poll)
    last = len(c["sets"]) - 1
    if family == "a":
        assert polled[-1] == ("C", last, E), polled
        assert all(p == ("C", last, 0) for p in polled[:-1])
        steps, _ = _walk(c, int(c["walkers"][1]), *_items(c, int(c["walkers"][1]), 6)[0])
        assert [s[2] for s in steps if s[0] == "C"].index(E) + 1 == M * POLL
    else:
        # the last depth-2 chunk of the last tooth, the one that holds mtop: no other depth-2 chunk follows before the matches
        k, first = (POLL - 1) * poll, _first_match(steps)
        assert steps[k][:2] == ("C", 2) and k < first and not any(s[:2] == ("C", 2) for s in steps[k + 1:first]), steps[k]
        assert {p[1] for p in polled} == {2, 3}, "polls at both inner depths"


def test_step_model_of_the_comb_at_narrow_first_level_chunks(tmp_path_factory):
    """(a) at shifts 0 and 3: the walkers' rows are cut into items of 1 and 8 teeth, the items are as many as the construction says,
    and their rows taken together are the enumerator's.  An item of 8 teeth stays below 1024 steps: below shift 6 this graph can
    only leaf-suspend, and the device test asks for the row set alone there"""
    c = _comb_leaf(tmp_path_factory)
    for shift in (0, 3):
        found, n_items, longest = [], 0, 0
        for v0 in c["sets"][0]:
            for it in _items(c, int(v0), shift):
                steps, rows = _walk(c, int(v0), *it)
                found.append(rows)
                n_items += 1
                longest = max(longest, len(steps))
        assert n_items == c["items"][shift]
        assert longest < POLL
        assert sh._row_set(np.concatenate(found)) == sh._row_set(_reference(c))


@pytest.mark.parametrize("mode", list(MODES))
def test_step_model_of_the_hub_wedge(tmp_path_factory, mode):
    """shift 6: the items of all hubs give the enumerator's rows in every mode.  In the induced modes the item of a hub's first chunk
    walks more than 1024 steps before its first match (its first 9 survivors find nothing), so at page_rows = 1 it is poll-suspended
    at depth 2, in the walk that ends with its first matches (the depth-2 state counts), with survivors pending at depth 1 of which
    the last has the item's last matches (the depth-1 mask counts).  In the distinct modes that depth-2 row is trimmed: it starts
    after the image of `a`, not at the row's first entry"""
    c = _hub_wedge(tmp_path_factory)
    found, n_items = [], 0
    for v0 in c["sets"][1]:
        for k, it in enumerate(_items(c, int(v0), 6)):
            steps, rows = _walk(c, int(v0), *it, mode=mode)
            found.append(rows)
            n_items += 1
            if k == 0 and v0 != c["finder"] and MODES[mode]["induced"]:
                first = _first_match(steps)
                assert first > POLL and steps[POLL - 1][:2] == ("C", 2), (mode, first)
                assert not any(s[:2] == ("D", 1) for s in steps[POLL - 1:first]), "polled in the walk that finds the first matches"
                pending = [i for i, s in enumerate(steps) if s[:2] == ("D", 1) and i > first]
                assert len(pending) == 2 and any(s[2] for s in steps[pending[-1]:]), "survivors pending at depth 1, the last with matches"
            if v0 == c["finder"]:
                assert _first_match(steps) <= 8
    assert n_items == c["items"][6]
    assert sh._row_set(np.concatenate(found)) == sh._row_set(_reference(c, mode)) and sum(map(len, found)) == len(_reference(c, mode))


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def pages_lines(monkeypatch, capfd):
    """contexts created while this fixture is active print one `[refine_pages]` line per cursor that launches (GNNPE_DEBUG=1 is read
    when a context is created); the returned callable gives the lines since it was last called as dicts of integers"""
    monkeypatch.setenv("GNNPE_DEBUG", "1")
    capfd.readouterr()

    def take():
        sys.stderr.flush()
        err = capfd.readouterr().err
        return [{k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])}
                for ln in err.splitlines() if ln.startswith("[refine_pages] ")]
    return take


def _open_engine(c, monkeypatch, shift):
    from gnnpe_amd import binding, synth
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    return ex._engine(binding, c["g"], synth.degree_order(c["g"]["offsets"]), 2)


def _assert_the_reference_set(c, mode, rows):
    want = _reference(c, mode)
    assert len(rows) == len(want), (mode, len(rows), len(want))
    assert sh._row_set(rows) == sh._row_set(want), mode


def _drain_all_page_sizes(eng, c, mode, shift, pages_lines):
    """cursors with page_rows 1, 5, 64 and M + 1 drained through test_refine_pages._drain (page shape, end state): each delivers the
    enumerator's set, no row lost and none twice; the library's line shows the order and the items the construction counts on.
    Returns the info after the first page per page size"""
    firsts = {}
    for page_rows in (1, 5, 64, c["M"][mode] + 1):
        with eng.open_match_cursor(c["qp"], c["bm"], page_rows, **MODES[mode]) as cur:
            line = pages_lines()
            assert len(line) == 1 and line[0]["shift"] == shift and line[0]["forced"] == 1, line
            assert line[0]["cands"] == c["cands"] and line[0]["items"] == c["items"][shift], (line, c["cands"], c["items"])
            assert line[0]["slots"] > c["items"][shift], "every item finds a wave of its own"
            rows, n_pages, firsts[page_rows] = rp._drain(cur, page_rows)
        _assert_the_reference_set(c, mode, rows)
        firsts[page_rows]["n_pages"] = n_pages
    print(f"mode {mode} shift {shift}: after the first page, by page_rows: {firsts}")
    return firsts


def _suspensions_per_page(eng, c, mode):
    """page_rows = 1: `suspended_waves` after every page, with the rows"""
    out, pages = [], []
    with eng.open_match_cursor(c["qp"], c["bm"], 1, **MODES[mode]) as cur:
        done = False
        while not done:
            rows, done = cur.next()
            info = cur.info()
            if not out:
                assert info["items_left"] == 0, info
            out.append(info["suspended_waves"] if not done else 0)
            pages.append(rows)
            assert len(pages) <= 4000
    return out, np.concatenate(pages)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 3, 6])
def test_gpu_comb_polls_at_the_last_depth(tmp_path_factory, monkeypatch, pages_lines, shift):
    """(a) at first-level shifts 0, 3 and 6: the enumerator's set at every page size.  At shift 6 a walker is one item of more than
    5 x 1024 matchless steps: with page_rows = 1 every item is taken in the first launch, and after every page for which the finder
    still has rows W + 1 waves are suspended -- the finder at its leaf, and the W walkers, which hold no match, by the poll: each
    walker was resumed and suspended again M - 1 = 5 times"""
    c = _comb_leaf(tmp_path_factory)
    eng = _open_engine(c, monkeypatch, shift)
    try:
        firsts = _drain_all_page_sizes(eng, c, "R", shift, pages_lines)
        if shift == 6:
            W, M = c["W"], c["M"]["R"]
            assert firsts[1]["items_left"] == 0 and firsts[1]["suspended_waves"] == W + 1, firsts[1]
            per_page, rows = _suspensions_per_page(eng, c, "R")
            print(f"suspended after each page: {per_page}")
            _assert_the_reference_set(c, "R", rows)
            assert per_page[:M - 1] == [W + 1] * (M - 1), per_page
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_comb_polls_at_the_inner_depths(tmp_path_factory, monkeypatch, pages_lines):
    """(b), shift 6: the enumerator's set at every page size; with page_rows = 1 every item is taken in the first launch and W + 1
    waves are suspended after it, and after every later page until the first walker reaches its matches (page 15 at the earliest):
    the walkers by the poll, at depths 2 and 3 with survivors pending at depths 1 and 2"""
    c = _comb_inner(tmp_path_factory)
    eng = _open_engine(c, monkeypatch, 6)
    try:
        firsts = _drain_all_page_sizes(eng, c, "R", 6, pages_lines)
        W = c["W"]
        assert firsts[1]["items_left"] == 0 and firsts[1]["suspended_waves"] == W + 1, firsts[1]
        per_page, rows = _suspensions_per_page(eng, c, "R")
        print(f"suspended after each page: {per_page}")
        _assert_the_reference_set(c, "R", rows)
        assert per_page[:14] == [W + 1] * 14, per_page
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_hub_wedge_in_every_mode(tmp_path_factory, monkeypatch, pages_lines, mode):
    """(c), shift 6, the four instantiations of k_refine_pages: the enumerator's set at every page size, and at least 2 waves
    suspended after the first page of 1 row.  In the induced modes exactly 1 + 2 W: the finder; per hub the item of its last chunk,
    whose survivors find a match within two steps (leaf); and per hub the item of its first chunk, which finds none in its first
    1024 steps (poll, at depth 2, in the distinct form inside a trimmed row) and has matches both in the walk it was polled in and
    behind a survivor that was pending at depth 1"""
    c = _hub_wedge(tmp_path_factory)
    eng = _open_engine(c, monkeypatch, 6)
    try:
        firsts = _drain_all_page_sizes(eng, c, mode, 6, pages_lines)
        assert firsts[1]["suspended_waves"] >= 2 and firsts[1]["items_left"] == 0, firsts[1]
        if MODES[mode]["induced"]:
            assert firsts[1]["suspended_waves"] == 1 + 2 * c["W"], firsts[1]
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_a_limit_ends_the_cursor_while_walkers_are_suspended(tmp_path_factory, monkeypatch):
    """(a), shift 6, page_rows = 1, limit = M - 1: the cursor says `done` with the limit's rows while W walkers and the finder hold
    saved states; info() then shows nothing suspended and no item left and a further next() launches nothing (_drain).  A new cursor
    on the same engine delivers the full set: the slots belong to the cursor"""
    c = _comb_leaf(tmp_path_factory)
    eng = _open_engine(c, monkeypatch, 6)
    try:
        limit = c["M"]["R"] - 1
        with eng.open_match_cursor(c["qp"], c["bm"], 1, limit=limit) as cur:
            rows, n_pages, first = rp._drain(cur, 1)
            assert first["suspended_waves"] == c["W"] + 1 and n_pages == limit == cur.info()["pages"], (first, n_pages)
        assert len(rows) == limit and sh._row_set(rows) <= sh._row_set(_reference(c)) and len(sh._row_set(rows)) == limit
        rows, _, _ = rp._all_rows(eng, c["qp"], c["bm"], 1)
        _assert_the_reference_set(c, "R", rows)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_two_cursors_with_poll_suspended_waves(tmp_path_factory, monkeypatch):
    """(c), shift 6: an induced and an induced-distinct cursor on one engine, pages of 1 and 5 rows alternating, each with
    poll-suspended waves from its first page on: both deliver their mode's set"""
    c = _hub_wedge(tmp_path_factory)
    eng = _open_engine(c, monkeypatch, 6)
    try:
        page = {"I": 1, "ID": 5}
        cur = {m: eng.open_match_cursor(c["qp"], c["bm"], page[m], **MODES[m]) for m in page}
        got, done = {m: [] for m in page}, {m: False for m in page}
        while not all(done.values()):
            for m in page:
                if not done[m]:
                    rows, done[m] = cur[m].next()
                    assert done[m] or len(rows) == page[m]
                    if not got[m]:
                        assert cur[m].info()["suspended_waves"] >= 1 + c["W"], (m, cur[m].info())
                    got[m].append(rows)
        for m in page:
            _assert_the_reference_set(c, m, np.concatenate(got[m]))
            cur[m].close()
    finally:
        eng.close()


def _tables(c, rows):
    """the per-vertex and per-edge count tables tallied from rows (include/gnnpe_online.h, V(C) and E(C))"""
    from gnnpe_amd import binding
    g = c["g"]
    offs, nbrs = g["offsets"].astype(np.int64), g["nbrs"].astype(np.int64)
    rows = rows.astype(np.int64)
    vt = np.zeros((rows.shape[1], g["n"]), np.uint64)
    for u in range(rows.shape[1]):
        np.add.at(vt[u], rows[:, u], 1)
    qe = binding.host_query_edges(c["qp"])
    et = np.zeros((len(qe), len(nbrs)), np.uint64)
    for k, (a, b) in enumerate(qe):
        for x, y in zip(rows[:, a], rows[:, b]):
            j = offs[x] + np.searchsorted(nbrs[offs[x]:offs[x + 1]], y)
            assert nbrs[j] == y
            et[k, j] += 1
    return vt, et


@pytest.mark.gpu
def test_gpu_one_shot_walkers_hear_of_the_limit(tmp_path_factory, monkeypatch):
    """(a), shift 6, the one-shot kernels, whose walk polls the total every 1024 steps as well (sets_walk, EXIT 3): refine_sets with
    limits 1, M, count - 1, count and count + 1 returns min(count, limit) and as many valid, different rows of the enumerator's set;
    the vertex and edge count tables are incomplete for every limit up to the count and, for count + 1, complete and equal to the
    tables tallied from the enumerator's rows"""
    c = _comb_leaf(tmp_path_factory)
    ref = _reference(c)
    count, M = len(ref), c["M"]["R"]
    vt, et = _tables(c, ref)
    eng = _open_engine(c, monkeypatch, 6)
    try:
        for limit in (1, M, count - 1, count, count + 1):
            got, _, rows = eng.refine_sets(c["qp"], c["bm"], limit=limit, matches_cap=count + 1)
            assert got == min(count, limit) == len(rows), (limit, got, len(rows))
            assert len(sh._row_set(rows)) == got and sh._row_set(rows) <= sh._row_set(ref), limit
            got, complete, table, _ = eng.refine_sets_vertex_counts(c["qp"], c["bm"], limit=limit)
            assert got == min(count, limit) and complete == (limit > count), (limit, got, complete)
            if complete:
                assert np.array_equal(table, vt)
            got, complete, table, _ = eng.refine_sets_edge_counts(c["qp"], c["bm"], limit=limit)
            assert got == min(count, limit) and complete == (limit > count), (limit, got, complete)
            if complete:
                assert np.array_equal(table, et)
    finally:
        eng.close()
