"""Large label alphabets: the label table's row count n_labels picks the code path in the embedding, index and auxiliary-index
kernels, and the rest of the suite never passes a table of more than 64 rows.  Every case here sits on one side of a threshold
read off the code (engine through the C-ABI against the oracle, bit for bit, as tests/test_gpu_fuzz.py):

  n_labels * e <= 4096            k_vde / k_vde_hubs: the table in LDS, else read from global memory (kVdeTabMax)
  n_labels * e <= 448             k_pack_leaves_pairs with the auxiliary rows: 16-bit ranks and sorted values in LDS, else global
  n_labels <= 65536               the table's rank form exists and the one-pass auxiliary build is allowed, else the generic pass
  bits(max degree) + bits(max label) <= 26   build_raux: the {degree, label} word inside a record's id bits, else 8-byte words
  lb = ceil(log2 n_labels) <= 21  ensure_vkey: 32- or 64-bit path keys, narrow or wide vertex words, zb = 0 .. 4 Z-order bits
  bits(p) + 3 lb + zb 3e <= 64    build_triple_order (l = 3): the vertex words' own widths, else a key without its low bits

The table's row count is a free parameter of set_label_table: the graph's labels are redrawn uniformly below it, the rows of
the labels that occur are the oracle's gen_vde_x rows (so oracle.gen_vde stays the reference) and every other row is positive
noise -- a table of 2^21 + 5 rows costs one numpy call.  Label 0 and label n_labels - 1 are pinned on the two highest-degree
vertices and on two low-degree ones: the first and the last row of the table and the top label bit are read."""
import numpy as np
import pytest

from gnnpe_amd import synth

pytestmark = pytest.mark.gpu

KVDE_STAGE, KVDE_TAB_MAX, HUB_DEGREE = 6144, 4096, 64  # gnnpe_kernels.hip.h: labels staged per pass, table doubles in LDS, hub rows


def _graph(name):
    if name == "gnm512":  # a 256-row block's adjacency range (~8000) exceeds one stage: the staging loop runs more than once
        return synth.gnm_graph(512, 8000)
    if name == "pl1500":  # hub rows: k_vde_hubs at e = 1, 2, 4, 8, the single-thread walk at e = 3, 5; largest degree: 9 bits
        return synth.powerlaw_graph(1500, 9000, exponent=2.0, max_degree=400)
    if name == "gnm600":
        return synth.gnm_graph(600, 3000)
    if name == "pl800":  # hub units of the pair-major build
        return synth.powerlaw_graph(800, 2500, exponent=2.1, max_degree=250)
    if name == "gnm400":  # ~1e5 four-vertex paths
        return synth.gnm_graph(400, 1600)
    raise KeyError(name)


def _deg(g):
    return np.diff(g["offsets"].astype(np.int64))


def _block_ranges(g):
    """Adjacency entries under every 256-row block of k_vde (rows in id order)."""
    offs = g["offsets"].astype(np.int64)
    return np.array([offs[min(r + 256, g["n"])] - offs[r] for r in range(0, g["n"], 256)])


def _relabel(g, n_labels, seed):
    """The graph with labels uniform in [0, n_labels); n_labels - 1 on the highest-degree vertex and on the lowest-degree
    vertex that has a neighbour, 0 on the second of each."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_labels, size=g["n"], dtype=np.int64).astype(np.uint32)
    deg = _deg(g)
    by_deg = np.argsort(deg, kind="stable")
    low = by_deg[deg[by_deg] >= 1]
    assert len(low) >= 4 and deg[low[-1]] > deg[low[1]]
    labels[low[-1]] = labels[low[0]] = n_labels - 1
    labels[low[-2]] = labels[low[1]] = 0
    out = dict(g)
    out["labels"] = labels
    return out


def _table(oracle, labels, n_labels, e, seed):
    t = 1.0 - np.random.default_rng(seed).random((n_labels, e))  # (0, 1]: positive, as the embeddings must be
    for lab in np.unique(labels):
        t[lab] = oracle.gen_vde_x(int(lab), e)
    return t


def _engine(oracle, g, n_labels, e, sn, mem, p):
    from gnnpe_amd import binding
    eng = binding.Engine(0)
    eng.load_csr(g["offsets"], g["nbrs"], g["labels"])
    eng.set_order(sn, mem, p)
    eng.set_label_table(_table(oracle, g["labels"], n_labels, e, 7 * n_labels + e))
    return eng


_PATHS = {}  # (graph, vertices per path) -> the oracle's enumeration in degree order: labels do not enter it


def _paths(oracle, name, L):
    if (name, L) not in _PATHS:
        g = _graph(name)
        _PATHS[name, L] = oracle.enumerate_closed(g["offsets"], g["nbrs"], synth.degree_order(g["offsets"]), L)
        _PATHS[name, L].setflags(write=False)
    return _PATHS[name, L]


# ---- group 1: embeddings on both sides of 4096 table doubles ---------------------------------------------------------
@pytest.mark.parametrize("side", ["lds", "global"])
@pytest.mark.parametrize("e", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("name", ["gnm512", "pl1500"])
def test_embeddings_on_both_sides_of_the_lds_table(oracle, name, e, side):
    """x, nx and vde with the largest table k_vde keeps in LDS (4096 // e rows) and with one row more (the table read from global
    memory through the kernels' second loop)."""
    n_labels = KVDE_TAB_MAX // e + (side == "global")
    assert (n_labels * e <= KVDE_TAB_MAX) == (side == "lds") and (n_labels - (side == "global")) * e <= KVDE_TAB_MAX
    g = _relabel(_graph(name), n_labels, 31 * e + (side == "global"))
    deg = _deg(g)
    if name == "gnm512":
        assert _block_ranges(g).max() > KVDE_STAGE and deg.max() <= HUB_DEGREE
    else:
        assert (deg > HUB_DEGREE).sum() >= 8 and g["labels"][np.argmax(deg)] == n_labels - 1
    assert g["labels"].max() == n_labels - 1 and g["labels"].min() == 0
    sn = synth.degree_order(g["offsets"])
    eng = _engine(oracle, g, n_labels, e, sn, np.zeros(g["n"], np.uint32), 1)
    x, nx, vde = eng.vde()
    eng.close()
    ox, onx, ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    assert np.array_equal(x, ox) and np.array_equal(nx, onx) and np.array_equal(vde, ovde)


@pytest.mark.parametrize("name", ["gnm512", "pl1500"])
def test_embeddings_and_path_rows_at_70000_labels(oracle, name):
    """e = 2 with 70000 rows (no rank form, 17 label bits): the embeddings, and the path rows' pde and pde_label at l = 2 (all
    rows) and l = 3 (the first, the middle and the last 100 000 of 7.8e6 / 2.1e7 rows) against ovde[want] and ox[want]."""
    e, n_labels = 2, 70000
    g = _relabel(_graph(name), n_labels, 5)
    sn = synth.degree_order(g["offsets"])
    eng = _engine(oracle, g, n_labels, e, sn, np.zeros(g["n"], np.uint32), 1)
    x, nx, vde = eng.vde()
    ox, onx, ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    assert np.array_equal(x, ox) and np.array_equal(nx, onx) and np.array_equal(vde, ovde)
    for l in (2, 3):
        L = l + 1
        want = _paths(oracle, name, L)
        total = eng.count_paths(l)
        assert total == len(want) > 200_000
        k = 100_000
        for a in ((0,) if l == 2 else (0, total // 2 - k // 2, total - k)):
            b = total if l == 2 else a + k
            ids, pde, pdl = eng.fill_paths(a, b, pde=True, pde_label=True)
            assert np.array_equal(ids, want[a:b]), (l, a)
            assert np.array_equal(pde, ovde[want[a:b]].reshape(b - a, L * e)), (l, a)
            assert np.array_equal(pdl, ox[want[a:b]].reshape(b - a, L * e)), (l, a)
    eng.close()


# ---- groups 2 - 4: partition images and their auxiliary index ---------------------------------------------------------
def _check_partitions(oracle, eng, g, mem, p, want, L, e, ox, ovde):
    """Every partition's image straight from the enumeration state (pair-major at l = 2, triple-major at l = 3): valid, every path
    of the partition once with son = its index inside the partition, lo = hi = its pde row; the auxiliary index of the generic pass
    and of the one-pass entry point (same image bytes, same three arrays) against the oracle's walk of that image."""
    import torch
    dev = torch.device("cuda:0")
    D = L * e
    F = min((4096 - 5) // (16 * D + 4) - 1, 64)  # both builds fill a leaf to capacity - 1, the tuple-array build to capacity - 2
    deg = _deg(g).astype(np.uint32)
    part_of = mem[want[:, 0]]
    assert np.bincount(part_of, minlength=p).min() > 0
    for pid in range(p):
        mine = want[part_of == pid]
        k = len(mine)
        img, nbytes, hdr = eng.build_index_partition_device(pid)
        raw = eng.copy_to_host(img, nbytes).tobytes()
        d = oracle.index_validate(raw)
        assert d["dim"] == D and d["num_data"] == k == hdr[3] and d["dnodes"] == -(-k // F), (pid, d["dnodes"])
        order = np.argsort(d["leaf_son"], kind="stable")
        assert np.array_equal(d["leaf_son"][order], np.arange(k)), pid
        assert np.array_equal(d["leaf_pt"][order], ovde[mine].reshape(k, D)), pid
        tup = torch.from_numpy(np.ascontiguousarray(mine).view(np.int32)).to(dev)
        aux = eng.aux_index_device(img, nbytes, k, L, tup)
        key, adeg, ambr = oracle.aux_index(raw, L, deg[mine].reshape(k, L), ox[mine].reshape(k, D))
        assert np.array_equal(aux["key"].view(np.uint64), key.view(np.uint64)), pid
        assert np.array_equal(aux["degrees"], adeg) and np.array_equal(aux["label_mbr"].view(np.uint64), ambr.view(np.uint64)), pid
        img2, nbytes2, hdr2, fkey, fdeg, fmbr, fn = eng.build_index_partition_aux_device(pid, fetch=True)
        assert nbytes2 == nbytes and eng.copy_to_host(img2, nbytes2).tobytes() == raw, pid
        assert fn == len(key) and np.array_equal(fkey.view(np.uint64), key.view(np.uint64)), pid
        assert np.array_equal(fdeg, adeg) and np.array_equal(fmbr.view(np.uint64), ambr.view(np.uint64)), pid


def _partition_case(oracle, g, want, l, e, n_labels, p, seed):
    sn = synth.degree_order(g["offsets"])
    mem = np.random.default_rng(seed).integers(0, p, size=g["n"]).astype(np.uint32)
    eng = _engine(oracle, g, n_labels, e, sn, mem, p)
    x, nx, vde = eng.vde()
    ox, onx, ovde = oracle.gen_vde(g["offsets"], g["nbrs"], g["labels"], e)
    assert np.array_equal(x, ox) and np.array_equal(vde, ovde)
    assert eng.count_paths(l) == len(want)
    _check_partitions(oracle, eng, g, mem, p, want, l + 1, e, ox, ovde)
    eng.close()


# 448 = the ranks and sorted values that ride in the leaf kernel's LDS; 65536 = the last table with 16-bit ranks
@pytest.mark.parametrize("e,n_labels", [(2, 224), (2, 225), (2, 2049), (2, 65536), (2, 65537), (2, 2 ** 21 + 5),
                                         (8, 56), (8, 57), (8, 600), (8, 65537)])
@pytest.mark.parametrize("name", ["gnm600", "pl800"])
def test_pair_major_images_and_aux_across_the_label_thresholds(oracle, name, e, n_labels):
    """l = 2, p = 3, random membership, degree order.  Above 65536 labels the one-pass entry point has no rank form to reduce and
    must return the same arrays through the generic pass."""
    g = _relabel(_graph(name), n_labels, n_labels % 1000 + e)
    deg = _deg(g)
    assert (deg.max() <= HUB_DEGREE) if name == "gnm600" else ((deg > HUB_DEGREE).sum() >= 4)
    _partition_case(oracle, g, _paths(oracle, name, 3), 2, e, n_labels, 3, 17 + e)


def _star_graph(hub_degree):
    """G(1100, 1500) with vertex 0 rewired to exactly `hub_degree` neighbours: the largest degree is the case's parameter."""
    base = synth.gnm_graph(1100, 1500)
    keep = (base["eu"] != 0) & (base["ev"] != 0)
    eu = np.concatenate([base["eu"][keep].astype(np.int64), np.zeros(hub_degree, np.int64)])
    ev = np.concatenate([base["ev"][keep].astype(np.int64), np.arange(1, hub_degree + 1, dtype=np.int64)])
    src, dst = np.concatenate([eu, ev]), np.concatenate([ev, eu])
    o = np.lexsort((dst, src))
    offsets = np.searchsorted(src[o], np.arange(base["n"] + 1)).astype(np.uint32)
    return dict(n=base["n"], m=len(eu), offsets=offsets, nbrs=dst[o].astype(np.uint32), labels=base["labels"])


@pytest.mark.parametrize("e", [2, 8])
@pytest.mark.parametrize("hub_degree", [1023, 1024])
def test_compact_aux_word_at_its_limit(oracle, monkeypatch, hub_degree, e):
    """The one-pass build keeps the {degree, label} word in a record's 26 id bits while bits(max degree) + bits(max label) fit.
    It runs with 16-bit labels at most (65536 rows), so the limit is reached through the degree: a hub of 1023 neighbours under
    label 65535 is the word with all 26 bits set, a hub of 1024 switches the build to 8-byte words by the data alone."""
    monkeypatch.delenv("GNNPE_AUX_WIDE", raising=False)
    n_labels = 65536
    g = _relabel(_star_graph(hub_degree), n_labels, hub_degree + e)
    deg = _deg(g)
    assert deg.max() == deg[0] == hub_degree and np.sort(deg)[-2] < 64
    assert g["labels"][0] == n_labels - 1 and (g["labels"][deg < 4] == n_labels - 1).any()
    assert (int(deg.max()).bit_length() + int(g["labels"].max()).bit_length() <= 26) == (hub_degree == 1023)
    sn = synth.degree_order(g["offsets"])
    want = oracle.enumerate_closed(g["offsets"], g["nbrs"], sn, 3)
    _partition_case(oracle, g, want, 2, e, n_labels, 2, 3)


@pytest.mark.parametrize("e", [2, 8])
@pytest.mark.parametrize("max_label", [131071, 131072])
def test_aux_index_with_17_and_18_bit_labels_under_a_9_bit_degree(oracle, monkeypatch, max_label, e):
    """Largest degree 9 bits, largest label 17 bits (26 bits together) and 18 bits (27).  Tables of this size have no rank form, so
    the one-pass entry point answers through the generic pass on both sides; the arrays must be the oracle's all the same."""
    monkeypatch.delenv("GNNPE_AUX_WIDE", raising=False)
    n_labels = max_label + 1
    g = _relabel(_graph("pl1500"), n_labels, max_label % 100 + e)
    deg = _deg(g)
    assert 256 <= deg.max() <= 511
    assert g["labels"].max() == max_label == g["labels"][np.argmax(deg)] and (g["labels"][deg < 4] == max_label).any()
    _partition_case(oracle, g, _paths(oracle, "pl1500", 3), 2, e, n_labels, 3, 23 + e)


# ---- group 4: the l = 3 partition index across the key-width boundary ------------------------------------------------
def _triple_key_bits(e, n_labels, p):
    """ensure_vkey's widths restated: (bits of the three labels and the Z-order levels, bits of the partition field on top)."""
    lb = 1
    while lb < 21 and (1 << lb) < n_labels:
        lb += 1
    D = 3 * e
    zb_cap = 0
    while zb_cap < 4 and zb_cap * D + e <= 32:
        zb_cap += 1
    zb = min(2, zb_cap)
    while zb > 0 and 3 * lb + zb * D > 64:
        zb -= 1
    passes, width = (3 * lb + zb * D + 7) // 8, 32 if 3 * lb + zb * D <= 32 else 64
    while zb < zb_cap and (3 * lb + (zb + 1) * D + 7) // 8 == passes and 3 * lb + (zb + 1) * D <= width:
        zb += 1
    return 3 * lb + zb * D, int(p).bit_length()  # (the value p itself is the key of an empty unit)


FITS = [(8, 16, 2), (8, 33, 2), (2, 8193, 3)]
TOO_WIDE = [(8, 17, 2), (8, 32, 3), (8, 16, 16), (4, 4097, 2), (2, 16385, 3), (2, 65537, 2), (1, 65537, 2), (2, 2 ** 20 + 1, 2)]


@pytest.mark.parametrize("e,n_labels,p", FITS + TOO_WIDE)
def test_triple_major_images_across_the_key_width_boundary(oracle, e, n_labels, p):
    """l = 3 where the vertex words' key and the partition field fit in 64 bits, and where they do not (17 .. 32 labels at e = 8
    and two partitions: 63 + 2 bits): the build must not refuse -- the key is a packing order only -- and the images and their
    auxiliary index hold exactly the partition's paths either way."""
    vbits, pbits = _triple_key_bits(e, n_labels, p)
    assert (vbits + pbits <= 64) == ((e, n_labels, p) in FITS), (vbits, pbits)
    g = _relabel(_graph("gnm400"), n_labels, n_labels % 1000 + e + p)
    assert _deg(g).max() <= HUB_DEGREE
    want = _paths(oracle, "gnm400", 4)
    assert len(want) > 100_000
    _partition_case(oracle, g, want, 3, e, n_labels, p, 41 + p)
