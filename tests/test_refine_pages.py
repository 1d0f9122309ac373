"""Paged match enumeration (include/gnnpe_online.h "ABI version 10", csrc/gnnpe_refine_pages.hip): a cursor over the embeddings
gnnpe_refine_sets counts.  Every page except the last is exactly full, and across the pages every embedding inside the sets comes
out exactly once, up to the limit, whatever the page size.

Yardstick for "the right set": the rows are valid embeddings inside the sets and pairwise different
(test_refine_sets._assert_rows_are_embeddings) and as many as the host form gnnpe_host_refine_sets counts; where networkx's rows
exist (test_refine_sets._small_cases) the row sets are compared directly."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import test_online_exact as ex
import test_refine_sets as rs
import test_refine_sets_shapes as sh

FULL = (1 << 64) - 1
CLI = rs.CLI
ONLINE = rs.ONLINE
FUZZ_PAGE_ROWS = (1, 3, 64, 257, 5000)
FUZZ_MAX_COUNT = 2_000_000


def _drain(cur, page_rows):
    """every page of an open cursor: (all rows, number of next() calls up to `done`, info after the first page).  Checks the
    page shape on the way: every page before the last holds exactly page_rows rows; after `done` nothing is suspended, no item
    is left, and a further next() gives 0 rows, `done`, and no launch (the page count stands)"""
    pages, first = [], None
    while True:
        rows, done = cur.next()
        if first is None:
            first = cur.info()
        assert rows.dtype == np.uint32 and rows.ndim == 2
        pages.append(rows)
        if done:
            break
        assert len(rows) == page_rows, (len(pages), len(rows), page_rows)
        assert len(pages) < 10 ** 6
    assert len(pages[-1]) <= page_rows
    end = cur.info()
    assert end["suspended_waves"] == 0 and end["items_left"] == 0, end
    assert end["rows"] == sum(len(p) for p in pages)
    again, done = cur.next()
    assert done and len(again) == 0 and cur.info()["pages"] == end["pages"]
    return np.concatenate(pages), len(pages), first


def _all_rows(eng, qp, bm, page_rows, limit=FULL):
    with eng.open_match_cursor(qp, bm, page_rows, limit=limit) as cur:
        return _drain(cur, page_rows)


def _assert_the_right_set(g, qp, bm, rows, want):
    assert len(rows) == want, (len(rows), want)
    rs._assert_rows_are_embeddings(g, qp, bm, rows)


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_cli_refuses_the_paging_flags_where_they_do_not_apply(tmp_path):
    """each refusal exits non-zero with its message before the graph is read or a GPU is touched"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    q = os.path.join(ONLINE, "q1.graph")
    mf = str(tmp_path / "m.txt")
    base = [CLI, "-f", root, "-d", graph, "-q", q, "-p", "2", "-m", "online", "--exact", "--refine", "sets"]
    for extra, msg in ((["--all-matches"], "--all-matches needs --matches"),
                       (["--matches", mf, "--match-page", "50"], "--match-page needs --all-matches"),
                       (["--matches", mf, "--all-matches", "--match-page", "0"], "--match-page must be an integer of at least 1")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "Answer Number" not in r.stdout, extra
    assert not os.path.exists(mf)


def test_fuzz_cases_fit_the_paged_test(tmp_path_factory):
    """the 24 fuzz cases of test_refine_sets_shapes before any device sees them: at least 20 have no more than 2 000 000
    embeddings, so the device test below runs on at least 20"""
    counts = [sh._fuzz_case(s, tmp_path_factory)["count"] for s in sh.FUZZ_SEEDS]
    assert sum(k <= FUZZ_MAX_COUNT for k in counts) >= 20, counts


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_one_row_per_page(tmp_path_factory):
    """1. page_rows = 1 on the 12 small cases, label/degree and thinned bitmaps: the row set is networkx's filtered set, the
    pages are the count plus at most one empty last page, every page before the last holds 1 row.  Every last-depth chunk with
    two survivors straddles a page end here."""
    from gnnpe_amd import binding
    total = 0
    for t, c in enumerate(rs._small_cases(tmp_path_factory)):
        eng = ex._engine(binding, c["g"], c["sn"], 2)
        for name in ("bm", "sub"):
            emb = c["emb"][rs._in_sets(c[name], c["emb"])]
            rows, n_pages, _ = _all_rows(eng, c["qp"], c[name], 1)
            assert sh._row_set(rows) == sh._row_set(emb) and len(rows) == len(emb), (t, name)
            assert len(emb) <= n_pages <= len(emb) + 1 and n_pages >= 1, (t, name, n_pages, len(emb))
            total += len(emb) if name == "bm" else 0
        eng.close()
    assert total == 1079


H1_RUNS = (("triangle", "thin", 7), ("triangle", "thin", 63), ("triangle", "thin", 64), ("triangle", "thin", 65),
           ("K4", "ld", 1000), ("K4", "ld", 4096), ("edge", "ld", 100), ("vertex", "ld", 1), ("vertex", "ld", 64),
           ("vertex", "ld", 100))
H1_COUNTS = {("triangle", "thin"): 11882, ("K4", "ld"): 109224, ("edge", "ld"): 11386, ("vertex", "ld"): 2000}


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 6])
def test_gpu_page_sizes_around_the_wave_width_on_h1(tmp_path_factory, monkeypatch, shift):
    """2. H1 with single-entry first-level items (shift 0) and with 64-entry chunks (shift 6): pages of 7, 63, 64 and 65 rows of
    the thinned triangle, 1 000 and 4 096 of K4, 100 of the edge (the leaf is the item's own chunk), 1, 64 and 100 of the
    vertex.  The right set, every page before the last exactly full; at shift 0 with pages of at most 1 000 rows some wave is
    suspended after the first page, so the suspend path ran"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={shift}")
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name, b, page_rows in H1_RUNS:
            want = h["want"][name, b]
            assert want == H1_COUNTS[name, b]
            rows, n_pages, first = _all_rows(eng, h["q"][name], h["bm"][name][b], page_rows)
            print(f"shift {shift} {name} {b} page {page_rows}: {n_pages} pages, {first['suspended_waves']} of {first['slots']} waves "
                  f"suspended after the first")
            _assert_the_right_set(g, h["q"][name], h["bm"][name][b], rows, want)
            assert -(-want // page_rows) <= n_pages <= -(-want // page_rows) + 1
            if shift == 0 and page_rows <= 1000:
                assert first["suspended_waves"] >= 1 and first["pages"] == 1 and first["rows"] == page_rows, first
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_limits(tmp_path_factory):
    """3. triangle on H1's label/degree bitmap (28 446 embeddings), pages of 1 000 rows: min(28 446, limit) valid different
    rows, and no launch once the limit is met (_drain: the page count stands on a further next())"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, qp, bm, count = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"], h["want"]["triangle", "ld"]
    assert count == 28446
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for limit in (0, 1, 999, 1000, 1001, 28445, 28446, 28447, FULL):
            with eng.open_match_cursor(qp, bm, 1000, limit=limit) as cur:
                rows, n_pages, _ = _drain(cur, 1000)
                want = min(count, limit)
                _assert_the_right_set(g, qp, bm, rows, want)
                launches = cur.info()["pages"]
                assert launches <= -(-want // 1000) + (1 if limit > count else 0), (limit, launches)
                if limit <= count:  # the page that meets the limit says `done` itself
                    assert launches == -(-want // 1000) and n_pages == max(launches, 1), (limit, launches, n_pages)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_one_page_holds_everything(tmp_path_factory):
    """4. a page larger than the count: one page, `done` with it, and the row set of Engine.refine_sets(matches_cap=count).  A
    page of exactly the count is a count that is a multiple of page_rows: one full page, then at most one empty last page."""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        for name in ("triangle", "K4", "vertex"):
            qp, bm, count = h["q"][name], h["bm"][name]["ld"], h["want"][name, "ld"]
            got, _, ref = eng.refine_sets(qp, bm, limit=sh.H1_LIMIT, matches_cap=count)
            assert got == count == len(ref)
            for page_rows in (count + 1, count + 1000, 2 * count):
                with eng.open_match_cursor(qp, bm, page_rows) as cur:
                    rows, done = cur.next()
                    assert done and len(rows) == count and cur.info()["pages"] == 1, (name, page_rows, len(rows))
                    assert sh._row_set(rows) == sh._row_set(ref), (name, page_rows)
            rows, n_pages, _ = _all_rows(eng, qp, bm, count)
            assert n_pages in (1, 2) and sh._row_set(rows) == sh._row_set(ref) and len(rows) == count, (name, n_pages)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_cursors_are_independent(tmp_path_factory):
    """5. two cursors (triangle, K4) on one engine with their pages alternating, Engine.refine_sets and the exact filter
    between the pages: both sets are right.  A cursor closed after its first page leaves nothing behind: a new cursor on the same
    query delivers the full set."""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g = h["g"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        names = ("triangle", "K4")
        q = {k: h["q"][k] for k in names}
        bm = {k: h["bm"][k]["ld"] for k in names}
        page = {"triangle": 3000, "K4": 10000}
        plan = binding.host_query_plan_exact(q["triangle"], 2, 2)
        cur = {k: eng.open_match_cursor(q[k], bm[k], page[k]) for k in names}
        got, done = {k: [] for k in names}, {k: False for k in names}
        step = 0
        while not all(done.values()):
            for k in names:
                if not done[k]:
                    rows, done[k] = cur[k].next()
                    assert done[k] or len(rows) == page[k]
                    got[k].append(rows)
            if step < 3:
                assert eng.refine_sets(q["K4"], bm["K4"], limit=sh.H1_LIMIT)[0] == h["want"]["K4", "ld"]
                assert eng.refine_sets(q["triangle"], h["bm"]["triangle"]["thin"], limit=sh.H1_LIMIT, matches_cap=100)[0] == \
                    h["want"]["triangle", "thin"]
                fbm, _ = eng.filter_candidates_exact(plan)
                assert fbm.shape == bm["triangle"].shape
            step += 1
        for k in names:
            _assert_the_right_set(g, q[k], bm[k], np.concatenate(got[k]), h["want"][k, "ld"])
            cur[k].close()
        first = eng.open_match_cursor(q["triangle"], bm["triangle"], 500)
        rows, done = first.next()
        assert len(rows) == 500 and not done
        first.close()
        rows, _, _ = _all_rows(eng, q["triangle"], bm["triangle"], 500)
        _assert_the_right_set(g, q["triangle"], bm["triangle"], rows, h["want"]["triangle", "ld"])
        # the generator form closes its cursor itself
        pages = list(eng.match_pages(q["triangle"], bm["triangle"], 5000))
        assert [len(p) for p in pages[:-1]] == [5000] * (len(pages) - 1) and not eng._cursors
        _assert_the_right_set(g, q["triangle"], bm["triangle"], np.concatenate(pages), h["want"]["triangle", "ld"])
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_device_pages(tmp_path_factory):
    """6. device=True: no host buffer is passed; torch.as_tensor of every page, taken together, is the host-copy run's set"""
    import torch
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, qp, bm, count = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"], h["want"]["triangle", "ld"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        host_rows, _, _ = _all_rows(eng, qp, bm, 4096)
        _assert_the_right_set(g, qp, bm, host_rows, count)
        pages = []
        with eng.open_match_cursor(qp, bm, 4096, device=True) as cur:
            done = False
            while not done:
                view, done = cur.next()
                assert done or view.shape == (4096, 3)
                if view.shape[0]:
                    t = torch.as_tensor(view, device="cuda:0")
                    assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == view.shape
                    assert t.data_ptr() == view.__cuda_array_interface__["data"][0]
                    pages.append(t.cpu().numpy().astype(np.uint32))  # (copied off the page before the next next())
                    del t
        dev_rows = np.concatenate(pages)
        assert len(dev_rows) == count and sh._row_set(dev_rows) == sh._row_set(host_rows)
        pages = [torch.as_tensor(p, device="cuda:0").cpu().numpy() for p in eng.match_pages(qp, bm, 10000, device=True)]
        assert sh._row_set(np.concatenate(pages).astype(np.uint32)) == sh._row_set(host_rows)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path_factory, tmp_path):
    """7. page_rows = 0, a 33-vertex query, a disconnected query and a multigraph context are refused by open; a cursor whose
    engine loaded another graph raises on next() and the engine goes on answering"""
    from gnnpe_amd import binding, synth
    h = sh._h1(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        with pytest.raises(binding.GnnpeError, match="page_rows must be at least 1"):
            eng.open_match_cursor(qp, bm, 0)
        with pytest.raises(binding.GnnpeError, match=r"1\.\.32"):
            eng.open_match_cursor(sh._path_file(tmp_path, 33), sh._ones(33, g["n"]), 10)
        disc = str(tmp_path / "pair.graph")
        ex._write_query(disc, 2, set(), [0, 0])
        with pytest.raises(binding.GnnpeError, match="not connected"):
            eng.open_match_cursor(disc, sh._ones(2, g["n"]), 10)
        assert not eng._cursors
        cur = eng.open_match_cursor(qp, bm, 100)
        rows, done = cur.next()
        assert len(rows) == 100 and not done
        other = sh._cycle_graph(40)
        eng.load_csr(other["offsets"], other["nbrs"], other["labels"])
        with pytest.raises(binding.GnnpeError, match="after the cursor was opened"):
            cur.next()
        assert cur.info()["pages"] == 1
        cur.close()
        p2 = sh._path_file(tmp_path, 2)
        assert eng.refine_sets(p2, sh._ones(2, 40))[0] == 80
        rows, _, _ = _all_rows(eng, p2, sh._ones(2, 40), 7)
        _assert_the_right_set(other, p2, sh._ones(2, 40), rows, 80)
        # the same rows handed over as the stored rows of a multigraph: the context is in the multigraph state
        eng.set_multigraph_rows(other["offsets"].astype(np.uint64), other["nbrs"])
        with pytest.raises(binding.GnnpeError, match="simple graphs only"):
            eng.open_match_cursor(p2, sh._ones(2, 40), 7)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_empty_outcomes(tmp_path_factory):
    """8. an empty set for one query vertex, and sets without an embedding (every query vertex held to the same single data
    vertex): `done` with 0 rows on the first next()"""
    from gnnpe_amd import binding
    h = sh._h1(tmp_path_factory)
    g, qp, bm = h["g"], h["q"]["triangle"], h["bm"]["triangle"]["ld"]
    eng = ex._engine(binding, g, h["sn"], 2)
    try:
        empty = bm.copy()
        empty[2] = 0
        hub = int(np.argmax(h["deg"]))
        single = np.repeat(sh._row_of([hub], g["n"])[None, :], 3, axis=0)
        assert binding.host_refine_sets(g, qp, single) == 0 == binding.host_refine_sets(g, qp, empty)
        for b in (empty, single):
            for page_rows in (1, 1000):
                with eng.open_match_cursor(qp, b, page_rows) as cur:
                    rows, done = cur.next()
                    assert done and rows.shape == (0, 3)
                    info = cur.info()
                    assert info["rows"] == 0 and info["suspended_waves"] == 0 and info["items_left"] == 0
    finally:
        eng.close()


_FUZZ_RAN = []


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sh.FUZZ_SEEDS)
def test_gpu_random_case_pages_equal_the_host_form(tmp_path_factory, monkeypatch, seed):
    """9. the 24 random cases of test_refine_sets_shapes (graph, query, bitmap, forced first-level shift), page_rows drawn per
    seed from 1, 3, 64, 257, 5 000: the right set against the host form's count.  A seed is skipped only if it has more than
    2 000 000 embeddings; at least 20 of the 24 run (asserted with the last seed, and on the CPU by
    test_fuzz_cases_fit_the_paged_test)"""
    from gnnpe_amd import binding, synth
    c = sh._fuzz_case(seed, tmp_path_factory)
    page_rows = int(np.random.default_rng(7000 + seed).choice(FUZZ_PAGE_ROWS))
    if c["count"] <= FUZZ_MAX_COUNT:
        g = c["g"]
        if c["shift"] is not None:
            monkeypatch.setenv("GNNPE_TESTING", f"sets_first_shift={c['shift']}")
        eng = ex._engine(binding, g, synth.degree_order(g["offsets"]), 2)
        try:
            rows, n_pages, _ = _all_rows(eng, c["qp"], c["bm"], page_rows)
            print(f"seed {seed}: {c['count']} embeddings, pages of {page_rows}: {n_pages}")
            _assert_the_right_set(g, c["qp"], c["bm"], rows, c["count"])
        finally:
            eng.close()
        _FUZZ_RAN.append(seed)
    if seed == sh.FUZZ_SEEDS[-1] and len(set(_FUZZ_RAN) | {seed}) > 1:  # (the whole parametrised test ran, not one seed of it)
        assert len(_FUZZ_RAN) >= 20, _FUZZ_RAN
    if c["count"] > FUZZ_MAX_COUNT:
        pytest.skip(f"{c['count']} embeddings")


@pytest.mark.gpu
def test_gpu_cli_all_matches(tmp_path, test_graph):
    """10. gnnpe_main --all-matches --match-page 50 on the golden Test graph with q1 (266 exact answers): 266 distinct valid
    lines in 6 or 7 pages and the answer line of a run without the flag; with -n 120 exactly 120 lines"""
    graph = os.path.join(GOLDEN, "test_graph", "data_graph.graph")
    root = ex._dataset(tmp_path, graph)
    qp = os.path.join(ONLINE, "q1.graph")
    want = json.load(open(os.path.join(ONLINE, "exact_answers.json")))["q1"]["exact"]
    assert want == 266
    base = [CLI, "-f", root, "-d", graph, "-q", qp, "-p", "2", "-m", "online", "--timing", "--exact", "--refine", "sets"]
    mf = str(tmp_path / "all.txt")
    r = subprocess.run(base + ["--matches", mf, "--all-matches", "--match-page", "50"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    answer = lambda out: [ln.split(" Query Time")[0] for ln in out.splitlines() if ln.startswith("Answer Number:")]
    assert answer(r.stdout) == answer(plain.stdout) == [f"Answer Number: {want}"]
    t = json.loads(r.stderr.strip().splitlines()[-1])
    assert t["refine"] == "sets" and t["matches_written"] == want and t["match_pages"] in (6, 7), t
    assert "match_pages" not in json.loads(plain.stderr.strip().splitlines()[-1])
    rows = np.loadtxt(mf, dtype=np.int64, ndmin=2)
    assert len(rows) == want
    rs._assert_rows_are_embeddings(test_graph, qp, ex._ld_bitmap(test_graph, qp), rows)
    mf = str(tmp_path / "n120.txt")
    r = subprocess.run(base + ["--matches", mf, "--all-matches", "--match-page", "50", "-n", "120"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "Answer Number: 120 " in r.stdout, r.stderr
    rows = np.loadtxt(mf, dtype=np.int64, ndmin=2)
    assert len(rows) == 120 and json.loads(r.stderr.strip().splitlines()[-1])["match_pages"] == 3
    rs._assert_rows_are_embeddings(test_graph, qp, ex._ld_bitmap(test_graph, qp), rows)
