"""A numpy model of an update session on the resident graph and a deterministic generator of such sessions (no GPU, no library
call): what tests/test_dynamic_sessions.py replays on an engine.

The model is the graph dict of tests/test_filter_support.py (n, sorted CSR, labels, edge set) moved on by fs.apply_edges_np and
fs.apply_vertices_np, together with the ids of the hub and of the isolated vertex as vertex batches renumber them, and two tag
tables a caller would keep: one cell per vertex and one per adjacency entry (found BY KEY x * n + y), 0 where a carry through the
library's maps must leave 0 (an added vertex, an inserted entry) and a fresh tag afterwards.

session(kind, seed) -> dict(g0, hub, iso, qname, bent, steps): STEPS steps, each drawn against the model graph as it then is.
Every step holds its kind, its arguments, and the model AFTER it: g, hub, iso, vtags / etags (what a carry must deliver) and
vtags_new / etags_new (with the fresh tags the caller then writes).  The step kinds:
    edges      1 .. 40 mixed insertions and deletions away from the hub and the isolated vertex; the pairs carry the labels of an
               edge of the session's query where the graph has such pairs (deletions fall back to any edge when they run out)
    edges_hub  one edge at the hub: inserted while its row has <= 64 entries, deleted otherwise (64 -> 65, 65 -> 64)
    vertices   0 .. 20 removed and 0 .. 20 added (never 0 and 0), sometimes a hub neighbour, the hub itself from step 6 on, the
               isolated vertex, vertex 0 and vertex n - 1
    relabel    1 .. 15 vertices to another label, sometimes a hub neighbour and the hub
    empty      the empty edge batch
    refused    `why` in ("id": an id >= n, "dup": an insertion that is an edge, "non": a deletion that is none -- each beside a
               valid pair --, "all": every vertex removed) with the text the library must name; the model stays as it is
    offline    set_order(degree_order), label table, vde, count_paths(2), fill_paths on the current graph
    kind "A" only: refresh, open, close (the third handle), keep_counts

A session has a bent drawn from its seed: "grow" (edge batches insert, vertex batches add), "shrink" (edge batches delete, vertex
batches remove the longest rows: the entries fall under 1024) or "none" (an edge batch pushes the entries to the other side of
2048).  Starting graphs: fs.make_graph's construction -- G(300, m) with four labels, vertex 17 isolated, vertex 300 a hub of exactly
64 entries -- with m near 940, so that the directed entries start between 1 960 and 2 040, just under one 2048-entry tile."""
import numpy as np

import test_filter_support as fs
import test_standing_query as sqt

NL, E, STEPS = fs.NL, 2, 10
STRUCT = ("edges", "vertices", "relabel", "offline")
QNAMES = ("wedge", "triangle", "path3", "c4")
BENTS = ("none", "grow", "shrink", "none")
WEIGHTS = dict(edges=3.0, edges_hub=1.5, vertices=2.5, relabel=2.0, offline=1.5, empty=1.0, refused=1.2)
WEIGHTS_A = dict(WEIGHTS, refresh=1.0, open=0.8, close=1.2, keep_counts=0.8)


def deg_of(g):
    return np.diff(g["offsets"].astype(np.int64))


def keys_of(g):
    """x * n + y of every adjacency entry in entry order (ascending: the rows are sorted)"""
    return np.repeat(np.arange(g["n"], dtype=np.int64), deg_of(g)) * g["n"] + g["nbrs"].astype(np.int64)


def start_graph(seed):
    from gnnpe_amd import synth
    g0 = synth.gnm_graph(300, 938 + 3 * (seed % 5), n_labels=NL, seed=500 + seed)
    edges = {(int(a), int(b)) for a, b in zip(g0["eu"], g0["ev"]) if fs.ISOLATED not in (int(a), int(b))}
    rng = np.random.default_rng(9000 + seed)
    others = np.setdiff1d(np.arange(300), [fs.ISOLATED])
    edges |= {(int(v), fs.HUB) for v in rng.choice(others, 64, replace=False)}
    g = fs.graph_of(301, edges, np.concatenate([g0["labels"], [1]]))
    d = deg_of(g)
    assert d[fs.HUB] == 64 and d[fs.ISOLATED] == 0 and 1960 <= len(g["nbrs"]) <= 2040, len(g["nbrs"])
    return g


def carry_tags(g_old, etags, g_new, new_id=None):
    """the entry tags of g_old in the entries of g_new by key, 0 for an entry g_old has not; new_id: of a vertex batch"""
    n_old, n_new = g_old["n"], g_new["n"]
    ko = keys_of(g_old)
    x, y = ko // n_old, ko % n_old
    if new_id is not None:
        live = (new_id[x] >= 0) & (new_id[y] >= 0)
        ko, etags = new_id[x[live]] * n_new + new_id[y[live]], etags[live]
        assert (np.diff(ko) > 0).all()  # the survivors keep their order
    kn = keys_of(g_new)
    out = np.zeros(len(kn), np.uint64)
    if len(ko):
        pos = np.minimum(np.searchsorted(ko, kn), len(ko) - 1)
        hit = ko[pos] == kn
        out[hit] = etags[pos[hit]]
    return out


class _Gen:
    def __init__(self, kind, seed):
        self.kind, self.seed = kind, seed
        self.rng = np.random.default_rng([{"A": 1, "B": 2}[kind], seed])
        self.g = start_graph(seed)
        self.hub, self.iso = fs.HUB, fs.ISOLATED
        self.qname = QNAMES[seed % 4]
        q = sqt.QUERIES[self.qname]
        self.edge_labels = {(q[2][a], q[2][b]) for a, b in q[1]} | {(q[2][b], q[2][a]) for a, b in q[1]}
        self.bent = BENTS[seed % 4] if kind == "B" else BENTS[(seed // 4 + seed) % 4]
        self.next_tag = 1
        self.vtags, self.etags = self.fresh(np.zeros(self.g["n"], np.uint64)), self.fresh(np.zeros(len(self.g["nbrs"]), np.uint64))
        self.third, self.batches = False, 0

    def fresh(self, tags):
        """a fresh tag in every zero cell"""
        out = tags.copy()
        z = np.flatnonzero(out == 0)
        out[z] = self.next_tag + np.arange(len(z), dtype=np.uint64)
        self.next_tag += len(z)
        return out

    # ---- the draws ------------------------------------------------------------------------------------------------------------

    def pairs(self, k_ins, k_del):
        g, rng = self.g, self.rng
        lab, avoid = g["labels"], {self.hub, self.iso}
        fit = lambda a, b: (int(lab[a]), int(lab[b])) in self.edge_labels
        have = [e for e in sorted(g["edges"]) if not avoid & set(e)]
        good, rest = [e for e in have if fit(*e)], [e for e in have if not fit(*e)]
        pick = lambda pool, k: [pool[int(i)] for i in rng.choice(len(pool), k, replace=False)] if k else []
        k_del = min(k_del, len(have))
        dele = pick(good, min(k_del, len(good)))
        dele += pick(rest, k_del - len(dele))
        ins, tries = set(), 0
        while len(ins) < k_ins:
            a, b = sorted(int(x) for x in rng.choice(g["n"], 2, replace=False))
            tries += 1
            if (a, b) in g["edges"] or a in avoid or b in avoid:
                continue
            if fit(a, b) or tries > 400 * k_ins:
                ins.add((a, b))
        return sorted(ins), sorted(dele)

    def draw_edges(self):
        rng, entries = self.rng, len(self.g["nbrs"])
        if self.bent == "none" and rng.random() < 0.25:
            k_ins, k_del = int(rng.integers(0, 6)), int(rng.integers(0, 6))
            k_ins += k_ins + k_del == 0
        else:
            up = self.bent == "grow" or (self.bent == "none" and entries < 2048)
            big, small = int(rng.integers(25, 38)), int(rng.integers(0, 3))
            k_ins, k_del = (big, small) if up else (small, big)
        ins, dele = self.pairs(k_ins, k_del)
        return dict(kind="edges", ins=ins, dele=dele)

    def draw_edges_hub(self):
        g, hub = self.g, self.hub
        if deg_of(g)[hub] <= 64:
            free = [v for v in range(g["n"]) if v not in (hub, self.iso) and (min(v, hub), max(v, hub)) not in g["edges"]]
            v = free[int(self.rng.integers(len(free)))]
            return dict(kind="edges_hub", ins=[(min(v, hub), max(v, hub))], dele=[])
        w = int(self.rng.choice(fs.nbrs_of(g, hub)))
        return dict(kind="edges_hub", ins=[], dele=[(min(w, hub), max(w, hub))])

    def draw_vertices(self, i):
        g, rng, hub = self.g, self.rng, self.hub
        n, d = g["n"], deg_of(g)
        mode = self.bent if self.bent != "none" else ("grow", "shrink", "mixed")[int(rng.integers(3))]
        if mode == "grow":
            k_rem, k_add = int(rng.integers(0, 3)), int(rng.integers(15, 21))
        elif mode == "shrink":
            k_rem, k_add = int(rng.integers(15, 21)), int(rng.integers(0, 3))
        else:
            k_rem, k_add = int(rng.integers(0, 21)), int(rng.integers(0, 21))
            k_add += k_rem + k_add == 0
        k_rem = min(k_rem, n - 1)
        special = []
        if hub >= 0 and d[hub] and rng.random() < (0.8 if d[hub] == 65 else 0.3):
            special.append(int(rng.choice(fs.nbrs_of(g, hub))))
        if hub >= 0 and i >= 6 and rng.random() < 0.3:
            special.append(hub)
        if self.iso >= 0 and rng.random() < 0.3:
            special.append(self.iso)
        for v in (0, n - 1):
            if rng.random() < 0.3:
                special.append(v)
        rem = list(dict.fromkeys(special))[:k_rem]
        pool = np.setdiff1d(np.arange(n), rem + [hub])
        if self.bent == "shrink":
            pool = pool[np.argsort(-d[pool], kind="stable")][:k_rem]  # the longest rows
        rem += [int(v) for v in rng.choice(pool, k_rem - len(rem), replace=False)]
        return dict(kind="vertices", rem=sorted(rem), add=[int(x) for x in rng.integers(0, NL, k_add)])

    def draw_relabel(self):
        g, rng, hub = self.g, self.rng, self.hub
        d = deg_of(g)
        R = []
        if hub >= 0 and d[hub] and rng.random() < (0.9 if d[hub] > 64 else 0.4):
            R.append(int(rng.choice(fs.nbrs_of(g, hub))))
        if hub >= 0 and rng.random() < 0.3:
            R.append(hub)
        k = int(rng.integers(1, 16))
        R = list(dict.fromkeys(R + [int(v) for v in rng.choice(g["n"], k, replace=False)]))[:k]
        labels = [(int(g["labels"][v]) + int(rng.integers(1, NL))) % NL for v in R]
        return dict(kind="relabel", R=R, labels=labels)

    def draw_refused(self):
        g, rng = self.g, self.rng
        n = g["n"]
        why = ("id", "dup", "non", "all")[int(rng.integers(4))]
        ins, dele = self.pairs(1, 1)
        have = sorted(g["edges"])
        if why == "id":
            return dict(kind="refused", why=why, ins=ins + [(3, n)], dele=dele, msg=str(n))
        if why == "dup":
            return dict(kind="refused", why=why, ins=ins + [have[int(rng.integers(len(have)))]], dele=[], msg="already an edge")
        if why == "non":
            return dict(kind="refused", why=why, ins=[], dele=dele + ins, msg="not an edge")
        return dict(kind="refused", why=why, rem=list(range(n)), add=[], msg="leaves no vertex")

    # ---- the model moves on -----------------------------------------------------------------------------------------------------

    def apply(self, step):
        g = self.g
        kind = step["kind"]
        vt = et = None
        if kind in ("edges", "edges_hub"):
            g2 = fs.apply_edges_np(g, step["ins"], step["dele"])
            vt, et = self.vtags, carry_tags(g, self.etags, g2)
            self.batches += 1
        elif kind == "vertices":
            g2, new_id = fs.apply_vertices_np(g, step["rem"], step["add"])
            step["new_id"] = new_id
            vt = np.zeros(g2["n"], np.uint64)
            vt[new_id[new_id >= 0]] = self.vtags[new_id >= 0]
            et = carry_tags(g, self.etags, g2, new_id)
            self.hub = int(new_id[self.hub]) if self.hub >= 0 else -1
            self.iso = int(new_id[self.iso]) if self.iso >= 0 else -1
        elif kind == "relabel":
            labels = g["labels"].copy()
            labels[step["R"]] = step["labels"]
            g2 = fs.graph_of(g["n"], g["edges"], labels)
        else:
            g2 = g
        if vt is None:
            vt, et = self.vtags, self.etags
        self.g, self.vtags, self.etags = g2, self.fresh(vt), self.fresh(et)
        step.update(g=g2, hub=self.hub, iso=self.iso, vtags=vt, etags=et, vtags_new=self.vtags, etags_new=self.etags)
        return step

    def steps(self):
        out = []
        for i in range(STEPS):
            w = dict(WEIGHTS_A if self.kind == "A" else WEIGHTS)
            if self.hub < 0:
                w.pop("edges_hub")
            if self.kind == "A":
                w.pop("open" if self.third else "close")
                if not self.batches:
                    w.pop("keep_counts")
            names = sorted(w)
            p = np.array([w[k] for k in names])
            kind = names[int(self.rng.choice(len(names), p=p / p.sum()))]
            draw = dict(edges=self.draw_edges, edges_hub=self.draw_edges_hub, relabel=self.draw_relabel, refused=self.draw_refused)
            step = draw[kind]() if kind in draw else self.draw_vertices(i) if kind == "vertices" else dict(kind=kind)
            if kind in ("open", "close"):
                self.third = kind == "open"
            if kind == "vertices" and self.third and len(step["rem"]) != len(step["add"]):
                self.third = False  # the caller's bitmap was made for another n: the refresh is refused and the handle closed
            out.append(self.apply(step))
        return out


_SESSIONS = {}


def session(kind, seed):
    if (kind, seed) not in _SESSIONS:
        gen = _Gen(kind, seed)
        first = dict(g0=gen.g, hub=gen.hub, iso=gen.iso, qname=gen.qname, bent=gen.bent, vtags=gen.vtags, etags=gen.etags)
        _SESSIONS[kind, seed] = dict(first, steps=gen.steps())
    return _SESSIONS[kind, seed]


# ---- what a set of sessions covers, from the model alone --------------------------------------------------------------------------------

def crossed(a, b, edge):
    """+1 / -1 where a value went from below `edge` to at or above it / the other way, else 0"""
    return int(a < edge <= b) - int(b < edge <= a)


def coverage(sessions):
    """the graph-shaped facts of the issue over a list of sessions: a dict of counters (the telling ones, which need the brute
    force, are counted by the test)"""
    c = dict(pairs=set(), then=set(), hub_up=0, hub_down=0, hub_down_by_removal=0, relabel_at_long_row=0, n32_up=0, n32_down=0,
             n_320_or_288=0, e2048_up=0, e2048_down=0, e1024_down=0)
    for s in sessions:
        g, hub = s["g0"], s["hub"]
        prev = None
        for st in s["steps"]:
            k = "edges" if st["kind"] == "edges_hub" else st["kind"]
            if prev in STRUCT and k in STRUCT:
                c["pairs"].add((prev, k))
            if prev in STRUCT and k in ("refused", "empty"):
                c["then"].add((prev, k))
            prev = k
            g2 = st["g"]
            d, d2 = deg_of(g), deg_of(g2)
            if hub >= 0 and st["hub"] >= 0:
                a, b = int(d[hub]), int(d2[st["hub"]])
                if st["kind"] in ("edges", "edges_hub"):
                    c["hub_up"] += (a, b) == (64, 65)
                    c["hub_down"] += (a, b) == (65, 64)
                if st["kind"] == "vertices":
                    c["hub_down_by_removal"] += (a, b) == (65, 64)
            if st["kind"] == "relabel":
                c["relabel_at_long_row"] += any(d[w] > 64 for v in st["R"] for w in fs.nbrs_of(g, v))
            for edge in range(32, 640, 32):
                x = crossed(g["n"], g2["n"], edge)
                c["n32_up"] += x > 0
                c["n32_down"] += x < 0
                c["n_320_or_288"] += x != 0 and edge in (288, 320)
            x = crossed(len(g["nbrs"]), len(g2["nbrs"]), 2048)
            c["e2048_up"] += x > 0
            c["e2048_down"] += x < 0
            c["e1024_down"] += crossed(len(g["nbrs"]), len(g2["nbrs"]), 1024) < 0
            g, hub = g2, st["hub"]
    return c
