"""A numpy model of the slab halo and embedding exchange (TEST INFRASTRUCTURE: no GPU, no engine).

The multi-GPU path cuts the processing order into contiguous slabs, one per rank (gnn-pe_amd/dist.py).  A rank owns the
adjacency rows of its slab's vertices and fetches, hop by hop, the rows those rows refer to; the last hop's rows are
installed truncated to the entries ranked at or after the slab's first position.  `SlabModel` says what every C-ABI
helper of that exchange has to produce -- need lists, owners, truncated rows, the held state after every hop -- from
the whole graph, so that tests/test_gpu_slab_helpers.py compares each primitive with numpy and never with another
primitive.  tests/test_slab_model.py holds the model itself to the oracle's enumeration and to tests/fake_engine.py.
"""
import numpy as np

HUB_DEGREE = 64  # a row longer than this is a hub row of the enumeration (kHubDegree of the engine)

PLANTED_DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 129, 200)  # vertex i < 10 has exactly PLANTED_DEGREES[i] neighbours


def build_graph(n=600, m=2400, n_labels=5, seed=2):
    """G(n, m) with the planted vertices 0..9 of PLANTED_DEGREES (around the 16-lane row loops, the 64-lane compaction and
    the hub limit), `n_labels` labels and a RANDOM processing order, so that ranks are mixed inside every row.  Planted
    vertices are joined to unplanted ones only, so their degrees are exact."""
    from gnnpe_amd import synth
    rng = np.random.default_rng(seed)
    k = len(PLANTED_DEGREES)
    eu, ev = [], []
    for v, d in enumerate(PLANTED_DEGREES):
        eu.append(np.full(d, v, np.int64))
        ev.append(k + rng.choice(n - k, size=d, replace=False).astype(np.int64))
    have = sum(PLANTED_DEGREES)
    seen = set()
    ru, rv = [], []
    while have + len(ru) < m:
        a, b = (int(x) for x in rng.integers(k, n, size=2))
        if a == b or (min(a, b), max(a, b)) in seen:
            continue
        seen.add((min(a, b), max(a, b)))
        ru.append(min(a, b))
        rv.append(max(a, b))
    eu = np.concatenate(eu + [np.array(ru, np.int64)])
    ev = np.concatenate(ev + [np.array(rv, np.int64)])
    offsets, nbrs = synth._csr_from_edges(n, eu, ev)
    deg = np.diff(offsets.astype(np.int64))
    assert tuple(deg[:k]) == PLANTED_DEGREES and len(nbrs) == 2 * m
    assert deg[k:].max() <= HUB_DEGREE  # the planted rows are the only hub rows
    return dict(n=n, m=m, offsets=offsets, nbrs=nbrs, labels=rng.integers(0, n_labels, size=n).astype(np.uint32),
                n_labels=n_labels, sorted_nodes=rng.permutation(n).astype(np.uint32), membership=np.zeros(n, np.uint32))


def build_small_graph(n=10, seed=5):
    """Ten vertices for 64 ranks: most slabs are empty and n < n_ranks."""
    from gnnpe_amd import synth
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    pick = rng.choice(len(pairs), size=18, replace=False)
    eu = np.array([pairs[i][0] for i in pick], np.int64)
    ev = np.array([pairs[i][1] for i in pick], np.int64)
    offsets, nbrs = synth._csr_from_edges(n, eu, ev)
    return dict(n=n, m=len(pick), offsets=offsets, nbrs=nbrs, labels=rng.integers(0, 5, size=n).astype(np.uint32),
                n_labels=5, sorted_nodes=rng.permutation(n).astype(np.uint32), membership=np.zeros(n, np.uint32))


def bounds_sets(n):
    """The slab bounds every test runs over, for the graph of build_graph (n vertices)."""
    return {
        "R1": np.array([0, n], np.uint32),
        "R2": np.array([0, 257, n], np.uint32),
        "R3_empty_middle": np.array([0, 211, 211, n], np.uint32),
        "R5_empty_ends": np.array([0, 0, 190, 401, n, n], np.uint32),
        "R64": ((np.arange(65, dtype=np.int64) * n) // 64).astype(np.uint32),
    }


def small_bounds(n):
    """64 ranks over the graph of build_small_graph."""
    return ((np.arange(65, dtype=np.int64) * n) // 64).astype(np.uint32)


class Held:
    """Rows on one rank: vertex -> row as installed, in installation order (owned rows in slab order, then the halo)."""

    def __init__(self):
        self.rows = {}
        self.n_owned = 0

    def ids(self):
        return np.fromiter(self.rows.keys(), np.int64, len(self.rows))

    def halo_ids(self):
        return self.ids()[self.n_owned:]

    def stats(self):
        """(rows, neighbour entries, hub rows) as gnnpe_rows_held reports them: hub rows counted on the installed degrees."""
        lens = [len(r) for r in self.rows.values()]
        return len(lens), int(sum(lens)), int(sum(1 for d in lens if d > HUB_DEGREE))

    def pairs(self):
        """Every held adjacency entry (v -> u) as v << 32 | u."""
        out = [(np.int64(v) << 32) | r.astype(np.int64) for v, r in self.rows.items() if len(r)]
        return np.concatenate(out) if out else np.zeros(0, np.int64)


class SlabModel:
    def __init__(self, offsets, nbrs, sorted_nodes, bounds):
        self.offs = np.asarray(offsets, np.int64)
        self.nbrs = np.asarray(nbrs, np.uint32)
        self.sorted = np.asarray(sorted_nodes, np.int64)
        self.bounds = np.asarray(bounds, np.int64)
        self.n = len(self.offs) - 1
        self.R = len(self.bounds) - 1
        assert self.bounds[0] == 0 and self.bounds[-1] == self.n and np.all(np.diff(self.bounds) >= 0)
        self.rank = np.empty(self.n, np.int64)
        self.rank[self.sorted] = np.arange(self.n)
        self.deg = np.diff(self.offs)

    def row(self, v):
        return self.nbrs[self.offs[v]:self.offs[v + 1]]

    def owned(self, r):
        """Vertices of slab r, in slab order."""
        return self.sorted[self.bounds[r]:self.bounds[r + 1]]

    def owner(self, v):
        """The largest r with bounds[r] <= rank[v]: empty slabs own nothing."""
        return np.searchsorted(self.bounds[1:], self.rank[np.asarray(v, np.int64)], side="right")

    def truncate(self, row, min_rank):
        """The entries ranked >= min_rank, order kept."""
        row = np.asarray(row, np.uint32)
        return row[self.rank[row.astype(np.int64)] >= min_rank]

    def concat_rows(self, ids):
        """(degrees, the whole rows back to back) of `ids`: what their owner packs."""
        ids = np.asarray(ids, np.int64)
        rows = [self.row(v) for v in ids]
        return self.deg[ids].astype(np.int64), (np.concatenate(rows) if rows else np.zeros(0, np.uint32))

    def owned_csr(self, r):
        """rows u32, row_offsets u64, row_nbrs u32 of slab r: the arguments of gnnpe_load_rows."""
        ids = self.owned(r)
        deg, rn = self.concat_rows(ids)
        roff = np.zeros(len(ids) + 1, np.uint64)
        np.cumsum(deg, out=roff[1:])
        return ids.astype(np.uint32), roff, rn.astype(np.uint32)

    def start(self, r):
        h = Held()
        for v in self.owned(r):
            h.rows[int(v)] = self.row(v)
        h.n_owned = len(h.rows)
        return h

    def need(self, held):
        """(ids, counts): the vertices that held rows refer to and that are not held, grouped by owner, ascending by id
        inside a group; counts[o] = how many owner o is asked for."""
        ref = np.zeros(self.n, bool)
        for row in held.rows.values():
            ref[row.astype(np.int64)] = True
        ref[held.ids()] = False
        ids = np.flatnonzero(ref)
        own = self.owner(ids)
        order = np.argsort(own, kind="stable")
        return ids[order], np.bincount(own, minlength=self.R).astype(np.int64)[:self.R]

    def install(self, held, ids, min_rank=0):
        """The rows of `ids` arrive from their owners (whole) and are installed truncated at min_rank."""
        for v in np.asarray(ids, np.int64):
            assert int(v) not in held.rows
            held.rows[int(v)] = self.truncate(self.row(v), min_rank)
        return held

    def hops(self, r, l, truncate=True):
        """Held state of rank r after the l - 1 hops of dist.SlabBuild.install_halo: the last hop truncated at bounds[r],
        earlier hops whole.  Returns (held, [the need list of every hop])."""
        held, lists = self.start(r), []
        for hop in range(l - 1):
            ids, counts = self.need(held)
            lists.append((ids, counts))
            last = hop == l - 2
            self.install(held, ids, int(self.bounds[r]) if (truncate and last) else 0)
        return held, lists

    def in_some_halo(self, v):
        """True when some rank that does not own v asks for its row on the first hop."""
        o = int(self.owner(v))
        return any(r != o and v in set(self.need(self.start(r))[0].tolist()) for r in range(self.R))

    def slab_paths(self, paths, r):
        """The rows of an enumeration in processing order whose start vertex lies in slab r."""
        rk = self.rank[paths[:, 0].astype(np.int64)]
        return paths[(rk >= self.bounds[r]) & (rk < self.bounds[r + 1])]
