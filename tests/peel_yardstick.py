"""The yardstick of the peel tests (tests/test_standing_peel.py, tests/test_host_peel.py): a Python peel that recounts every match
of the current numpy graph each round and deletes all edges below the threshold at once.  It shares no code with the library:
the matches come from `embeddings` of tests/test_standing_query.py (joins of CSR rows in numpy), the support of an edge is counted
from them with np.unique, and the levels are found by peeling from the whole graph for every t from 0 up to the largest support.

Support.  A map of the query is injective, so the query edges of one map land on different data edges: the sum over the query edges
and the two directions of an edge's cells is the number of maps whose image holds the edge.  With `distinct` a match is an orbit of
maps under the query's automorphisms, each orbit n_aut maps with the same image, so the support is that number divided by n_aut."""
import numpy as np

from test_standing_query import automorphisms, embeddings


def graph_from(n, edges, labels):
    """a compact CSR dict from undirected pairs (any orientation); works without edges"""
    und = sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in edges})
    both = np.array(und + [(b, a) for a, b in und], np.int64).reshape(-1, 2)
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    offsets = np.zeros(n + 1, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(both[:, 0], minlength=n))
    return dict(n=n, m=len(und), offsets=offsets, nbrs=both[:, 1].astype(np.uint32), labels=np.asarray(labels, np.uint32).copy(), edges=set(und))


def supports(g, query, distinct):
    """{(x, y) with x < y: support} for every edge of g"""
    rows = embeddings(g, query, False) if g["m"] else np.zeros((0, query[0]), np.int64)
    n = g["n"]
    keys = [np.minimum(rows[:, a], rows[:, b]) * n + np.maximum(rows[:, a], rows[:, b]) for a, b in query[1]]
    k, c = np.unique(np.concatenate(keys), return_counts=True) if len(rows) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    div = len(automorphisms(query)) if distinct else 1
    assert (c % div == 0).all()
    sup = {e: 0 for e in g["edges"]}
    for kk, cc in zip(k.tolist(), c.tolist()):
        assert (kk // n, kk % n) in sup, "a match runs over a pair that is no edge"
        sup[kk // n, kk % n] = cc // div
    return sup


def peel(g, query, distinct, t, max_rounds=0):
    """(the graph left, removed edges in removal order, their rounds from 1, [rounds, removed, edges left, converged])"""
    cur, removed, rounds, r, converged = g, [], [], 0, 0
    while not (max_rounds and r == max_rounds):
        sup = supports(cur, query, distinct)
        low = sorted(e for e, s in sup.items() if s < t)
        if not low:
            converged = 1
            break
        r += 1
        removed += low
        rounds += [r] * len(low)
        cur = graph_from(cur["n"], cur["edges"] - set(low), cur["labels"])
    return cur, removed, rounds, [r, len(removed), cur["m"], converged]


def levels(g, query, distinct):
    """{edge: the largest t whose (Q, t)-truss holds it}: one peel of the whole graph per t, no jumping"""
    top = max(supports(g, query, distinct).values(), default=0)
    level = {}
    for t in range(top + 2):
        truss = peel(g, query, distinct, t)[0]
        for e in truss["edges"]:
            level[e] = t
        if not truss["m"]:
            break
    assert set(level) == g["edges"] and all(v <= top for v in level.values())
    return level


def cascade_graph(tail=12):
    """A K5 (vertices 0..4) with a strip of triangles hanging off it: the path 1 - 6 - 7 - ... under the two apexes 0 (of the K5) and
    5, which are not adjacent.  Every strip edge lies in two triangles except those at the free end, which lie in one; taking them
    away leaves the next ones with one, and so on: with the triangle and t = 2 the strip unravels a step per round and the K5
    (three triangles on every edge) stays.  All labels 1, the label of the triangle query."""
    n = 6 + tail
    edges = {(a, b) for a in range(5) for b in range(a + 1, 5)}
    path = [1] + list(range(6, n))
    edges |= {(min(a, b), max(a, b)) for a, b in zip(path, path[1:])}
    edges |= {(min(h, q), max(h, q)) for h in (0, 5) for q in path if h != q}
    assert n <= 64
    return graph_from(n, edges, np.ones(n, np.uint32))


K5 = {(a, b) for a in range(5) for b in range(a + 1, 5)}


def gnm(n, m, seed, n_labels=2):
    """G(n, m) with random labels"""
    rng = np.random.default_rng(seed)
    edges = set()
    while len(edges) < m:
        a, b = sorted(int(v) for v in rng.choice(n, 2, replace=False))
        edges.add((a, b))
    return graph_from(n, edges, rng.integers(0, n_labels, n))
