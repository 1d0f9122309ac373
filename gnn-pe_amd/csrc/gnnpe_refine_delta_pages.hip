// gnnpe_refine_delta_pages.hip -- the delta matches as CURSORS: gnnpe_refine_pages_open_delta, _open_delta_nonedges and
// _open_delta_vertices of include/gnnpe_online.h.  They hand out the gnnpe_match_cursor of gnnpe_refine_pages.hip, whose _next,
// _device_ptr, _info and _close serve them; across the pages of a cursor every map of Dset_m(C, F), Nset_m(C, F) or Sset_m(C, S)
// comes out exactly once.
//
// The searches are the one-shot ones -- one launch per ANCHOR (query edge: gnnpe_refine_delta.hip; non-adjacent query pair:
// gnnpe_refine_delta_nonedges.hip; query vertex: gnnpe_refine_delta_vertices.hip), the same items, item decodes and charging rules,
// used as they are -- under the loop, leaf, suspend and resume of k_refine_pages.  sets_walk cannot suspend, and k_refine_pages'
// loop knows one launch, one ticket and a floor of depth 1: the loop of these kernels is a COPY of it (delta_pages_run,
// gnnpe_refine_pages.hip.h) with a decode hook, a test hook ANDed onto the lane test's result before the ballot, and a floor depth.
// k_refine_pages was left as it is rather than made an instantiation of the copy: its protocol differs in three places (a wave
// loads its slot whatever the page holds; `suspended` is per launch; one ticket word), and its resource line is pinned.
//
//   * FLOOR.  The non-edge item fixes positions 0 and 1 and enters depth 2; its depth-1 words are never written.  The item ends when
//     the depth falls below the depth it entered at, which is the kernel's constant: a resumed wave needs no word for it.
//   * THE EDGE ITEM holds depth 1 to the chunk [j, j + 1) through cbase[1] = j - 64, end[1] = j + 1: the loop's next-chunk step
//     makes cb = j, one lane tests y, and the step after finds cb = j + 64 past the end.  Under a two-vertex query that chunk is the
//     leaf, and a leftover mask of it is bit 0.
//   * SEVERAL LAUNCHES, ONE PAGE, ONE WAIT.  The counter block (DeltaPagesCounters) is followed by one ticket word per anchor, all
//     zeroed when the cursor is opened.  A page zeroes the row cursor alone and queues the launch of the first unfinished anchor and
//     of every later one, back to back on the context's stream, then copies the block back: one wait.  A kernel first reads the row
//     cursor: with the page full it returns before it touches a slot or a ticket.  So
//       - a wave suspends only when it saw the page full, and the row cursor only grows inside a page: a launch that ends with room
//         in the page was never full, every one of its waves looked at its slot and resumed (and cleared) a valid one, and none
//         suspended.  It leaves NO valid slot, and it ends only when its tickets are past its items: the anchor is finished, and the
//         next launch owns the slots.
//       - the launch that fills the page is the only one of the page that suspends; the launches behind it return at once.
//       - hence all valid slots belong to one anchor at any time: `owner`, written with every suspend.  `valid` counts them (+1 a
//         suspend, -1 a resume) and is never zeroed: a slot whose wave came too late to look at it stays valid and stays counted.
//     After the wait the host takes the first unfinished anchor from it: `owner` if valid != 0, else the first anchor whose
//     ticket is below its item count.  The slot carries its anchor; a wave that meets another launch's slot raises `mismatch` and
//     leaves, and the host refuses the page (cursor bookkeeping, not a device assert).
//   * THE GRID of every launch of a cursor is the same, since wave w owns slot w: sets_grid_blocks over the largest item count.
//   * nothing waits on anything inside a kernel: a wave works, suspends or leaves.
//   * THE CURSOR OWNS ITS MEMORY: counters and tickets, its copy of the bitmap, F as keys, pairs and entries or S as a bitmap, the
//     candidate lists, chunk counts and item offsets of every launch (vertices), the slots and one page; the staging helpers of the
//     one-shot calls take these buffers in the place of the context's.  Every chunk count and scan runs in open, so a page queues
//     search launches only.  A pair of F that is (not) an edge is found by k_delta_entries inside open's wait.
// Resources of the twelve instantiations and the measurement: profiles/online_delta_pages.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_pages.hip.h"
#include "gnnpe_refine_delta_vertices.hip.h"

namespace gnnpe {

#define GNNPE_DELTA_PAGES_WAVE                                                                \
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];                                           \
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];                                          \
    volatile uint32_t *Sw = reinterpret_cast<volatile uint32_t *>(&s_wave[threadIdx.x >> 6]); \
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};                    \
    PagesSlot *slot = slots + ((size_t)blockIdx.x * kSetsWavesPerBlock + (threadIdx.x >> 6))

// Three kernels, four instantiations each, as k_refine_pages: plain, SetsOrder (distinct), SetsNon (induced), both.
// anchored at a query edge: the items are the 2 |F| directed entries.  nq >= 2.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_pages(SetsPlan P, SetsDelta D, uint32_t n_items, const uint32_t *__restrict__ pairs,
                                                              const uint32_t *__restrict__ ent, const unsigned long long *__restrict__ keys,
                                                              uint32_t n_keys, const uint32_t *__restrict__ adj_start,
                                                              const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                              const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                              uint64_t words, DeltaPagesCounters *ctr, uint32_t anchor, PagesSlot *slots,
                                                              uint32_t *__restrict__ page, unsigned long long page_rows, Ord... ord)
{
    GNNPE_DELTA_PAGES_WAVE;
    delta_pages_run<kOrdered, 1u, false>(
        P, S, Sw, G, 0u, nullptr, n_items, anchor, ctr, slot, page, page_rows, [&](uint32_t q) { return delta_item_decode(P, S, G, pairs, ent, q); },
        [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); }, ord...);
}

// anchored at a non-adjacent query pair: the items are the 2 |F| directed pairs, the floor is depth 2.  nq >= 3.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_nonedges_pages(SetsPlan P, SetsDelta D, uint32_t n_items,
                                                                       const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent,
                                                                       const unsigned long long *__restrict__ keys, uint32_t n_keys,
                                                                       const uint32_t *__restrict__ adj_start,
                                                                       const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                                       const uint32_t *__restrict__ labels,
                                                                       const uint32_t *__restrict__ bitmap, uint64_t words,
                                                                       DeltaPagesCounters *ctr, uint32_t anchor, PagesSlot *slots,
                                                                       uint32_t *__restrict__ page, unsigned long long page_rows, Ord... ord)
{
    GNNPE_DELTA_PAGES_WAVE;
    const uint32_t lane = threadIdx.x & 63u;
    delta_pages_run<kOrdered, 2u, false>(
        P, S, Sw, G, 0u, nullptr, n_items, anchor, ctr, slot, page, page_rows,
        [&](uint32_t q) { return nonedge_item_decode<kOrdered>(P, S, G, pairs, ent, q, lane, ord...); },
        [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); }, ord...);
}

// anchored at a query vertex: the items are the first-level chunks of S n C(u), or 64 candidates each under a single-vertex query
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_vertices_pages(SetsPlan P, uint32_t earlier, const uint32_t *__restrict__ sbits,
                                                                       uint32_t n_cand, const uint32_t *__restrict__ cand,
                                                                       const uint32_t *__restrict__ item_off, uint32_t n_items,
                                                                       uint32_t w_shift, const uint32_t *__restrict__ adj_start,
                                                                       const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                                       const uint32_t *__restrict__ labels,
                                                                       const uint32_t *__restrict__ bitmap, uint64_t words,
                                                                       DeltaPagesCounters *ctr, uint32_t anchor, PagesSlot *slots,
                                                                       uint32_t *__restrict__ page, unsigned long long page_rows, Ord... ord)
{
    GNNPE_DELTA_PAGES_WAVE;
    delta_pages_run<kOrdered, 1u, true>(
        P, S, Sw, G, n_cand, cand, n_items, anchor, ctr, slot, page, page_rows,
        [&](uint32_t q) { return sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q); },
        [&](uint32_t d, uint32_t v) { return ((earlier >> d) & 1u) == 0 || !vset_has(sbits, v); }, ord...);
}

#undef GNNPE_DELTA_PAGES_WAVE

}  // namespace gnnpe

using namespace gnnpe;

namespace {

enum { kAnchorEdges = 1, kAnchorNonedges = 2, kAnchorVertices = 3 };

size_t ctrs_bytes(size_t n_launch) { return sizeof(DeltaPagesCounters) + n_launch * 4; }

struct CursorGuard {  // every early return of an open closes the cursor unless it was handed out
    gnnpe_match_cursor *p;
    ~CursorGuard() { gnnpe_refine_pages_close(p); }
};

// what every open does before its anchor's own staging
gnnpe_match_cursor *cursor_new(gnnpe_ctx *c, int kind, uint64_t limit, uint64_t page_rows)
{
    gnnpe_match_cursor *cur = new gnnpe_match_cursor();
    cur->c = c;
    cur->graph_gen = c->graph_gen;
    cur->anchor_kind = kind;
    cur->limit = limit;
    cur->page_rows = page_rows;
    cur->page_cap = std::min(page_rows, limit);
    return cur;
}

// after the launches are known (L, with n_cand where the grid depends on it): the grid, the slots, the page, the counters with the
// tickets, the pinned block and the events.  Zeroes the counters and the slots on the stream.
int cursor_reserve(const char *who, gnnpe_match_cursor *cur, uint32_t grid_items)
{
    gnnpe_ctx *c = cur->c;
    const uint32_t nq = cur->Q.nq;
    const size_t n_launch = cur->L.size();
    cur->blocks = sets_grid_blocks(c, nq, grid_items);  // the same for every launch
    const size_t slot_bytes = (size_t)cur->blocks * kSetsWavesPerBlock * sizeof(PagesSlot);
    GNNPE_REQUIRE(cur->page_cap <= (~(size_t)0 >> 1) / ((size_t)nq * 4), GNNPE_ERR_RANGE, "%s: a page of %llu rows does not fit an allocation", who,
                  (unsigned long long)cur->page_cap);
    int rc;
    if ((rc = cur->slots.reserve(slot_bytes)) || (rc = cur->page.reserve((size_t)cur->page_cap * nq * 4)) ||
        (rc = cur->ctrs.reserve(ctrs_bytes(n_launch))))
        return rc;
    // (the pinned block also takes the item counts of a vertices cursor's launches during open)
    GNNPE_HIP_TRY(hipHostMalloc((void **)&cur->h_ctrs, ctrs_bytes(n_launch) + n_launch * 4));
    GNNPE_HIP_TRY(hipEventCreate(&cur->ev0));
    GNNPE_HIP_TRY(hipEventCreate(&cur->ev1));
    GNNPE_HIP_TRY(hipMemsetAsync(cur->ctrs.p, 0, ctrs_bytes(n_launch), c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(cur->slots.p, 0, slot_bytes, c->stream));  // no slot is valid
    return GNNPE_OK;
}

void cursor_items_left(gnnpe_match_cursor *cur, const uint32_t *tickets)
{
    cur->items_left = 0;
    for (size_t k = cur->first; k < cur->L.size(); k++)
        cur->items_left += cur->L[k].n_items - std::min(tickets ? tickets[k] : 0u, cur->L[k].n_items);
}

// gnnpe_refine_pages_open_delta and gnnpe_refine_pages_open_delta_nonedges
int open_pairs(const char *who, bool nonedges, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *pairs,
               uint64_t n_pairs, uint64_t limit, uint64_t page_rows, uint32_t mode, gnnpe_match_cursor **out)
{
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && out && (pairs || n_pairs == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    GNNPE_REQUIRE(page_rows > 0, GNNPE_ERR_ARG, "%s: page_rows must be at least 1", who);
    if (nonedges) {
        GNNPE_REQUIRE((mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) == 0, GNNPE_ERR_ARG, "%s: unknown mode bits 0x%x", who, mode);
        GNNPE_REQUIRE((mode & GNNPE_MATCH_INDUCED) != 0, GNNPE_ERR_ARG, "%s: the mode must contain GNNPE_MATCH_INDUCED", who);
    }
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, &q);
    if (rc) return rc;
    DeltaPlans D;
    if ((rc = delta_plans(who, c, Q, q, pairs, n_pairs, mode, &D, nonedges))) return rc;
    gnnpe_match_cursor *cur = cursor_new(c, nonedges ? kAnchorNonedges : kAnchorEdges, limit, page_rows);
    CursorGuard guard{cur};
    cur->Q = std::move(Q);
    if (D.nothing) {  // nothing to launch: a cursor that is done before its first page; the pairs are not looked up
        cur->done = true;
        guard.p = nullptr;
        *out = cur;
        return GNNPE_OK;
    }
    const uint32_t nq = cur->Q.nq;
    const size_t n_keys = cur->n_keys = D.keys.size();
    cur->L.resize(D.plans.size());
    for (size_t k = 0; k < D.plans.size(); k++) {
        cur->L[k].K = std::move(D.plans[k]);
        cur->L[k].older = D.older[k];
        cur->L[k].n_items = D.n_items;
    }
    if ((rc = cur->bitmap.reserve((size_t)nq * cur->Q.words * 4)) || (rc = cur->fset.reserve(DeltaBuf::bytes(n_keys))) ||
        (rc = cursor_reserve(who, cur, D.n_items)))
        return rc;
    SetsCall call(who, c, false);
    // F and the bitmap go up and k_delta_entries looks the pairs up; the staging zeroes the block's first 32 bytes once more
    delta_stage(call, c, cur->Q, D, candidate_bitmap, nonedges, &cur->ctrs, &cur->bitmap, &cur->fset);
    call.wait(cur->ctrs.p, sizeof(DeltaPagesCounters));  // (the caller's arrays may go)
    if (call.ok() && reinterpret_cast<const DeltaPagesCounters *>(c->h_pinned)->bad) {
        set_error(nonedges ? "%s: a pair is an edge of the graph" : "%s: a delta edge is not an edge of the graph", who);
        call.rc = GNNPE_ERR_ARG;
    }
    if ((rc = call.finish(nullptr))) return rc;
    cursor_items_left(cur, nullptr);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta_pages] kind=%d keys=%zu items=%u launches=%zu slots=%u\n", cur->anchor_kind, n_keys, D.n_items, cur->L.size(),
                cur->blocks * kSetsWavesPerBlock);
    guard.p = nullptr;
    *out = cur;
    return GNNPE_OK;
}

}  // namespace

extern "C" {

int gnnpe_refine_pages_open_delta(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *delta_edges,
                                  uint64_t n_delta, uint64_t limit, uint64_t page_rows, uint32_t mode, gnnpe_match_cursor **out)
{
    return open_pairs("gnnpe_refine_pages_open_delta", false, c, query_graph_path, candidate_bitmap, delta_edges, n_delta, limit, page_rows, mode,
                      out);
}

int gnnpe_refine_pages_open_delta_nonedges(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *pairs,
                                           uint64_t n_pairs, uint64_t limit, uint64_t page_rows, uint32_t mode, gnnpe_match_cursor **out)
{
    return open_pairs("gnnpe_refine_pages_open_delta_nonedges", true, c, query_graph_path, candidate_bitmap, pairs, n_pairs, limit, page_rows,
                      mode, out);
}

int gnnpe_refine_pages_open_delta_vertices(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *vertices,
                                           uint64_t n_vertices, uint64_t limit, uint64_t page_rows, uint32_t mode, gnnpe_match_cursor **out)
{
    const char *who = "gnnpe_refine_pages_open_delta_vertices";
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && out && (vertices || n_vertices == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    GNNPE_REQUIRE(page_rows > 0, GNNPE_ERR_ARG, "%s: page_rows must be at least 1", who);
    VerticesPlans V;
    int rc = vertices_plans(who, c, query_graph_path, candidate_bitmap, vertices, n_vertices, limit, mode, &V);
    if (rc) return rc;
    gnnpe_match_cursor *cur = cursor_new(c, kAnchorVertices, limit, page_rows);
    CursorGuard guard{cur};
    std::vector<uint32_t>().swap(V.Q.cand);  // (the launches have their own lists)
    cur->Q = V.Q;
    if (V.nothing) {  // nothing to launch: a cursor that is done before its first page
        cur->done = true;
        guard.p = nullptr;
        *out = cur;
        return GNNPE_OK;
    }
    const uint32_t nq = cur->Q.nq;
    const size_t n_launch = V.L.size();
    cur->n_cand_all = V.cand_all.size();
    cur->L.resize(n_launch);
    uint32_t grid_items = 0;
    for (size_t k = 0; k < n_launch; k++) {
        DeltaPagesLaunch &l = cur->L[k];
        l.K = std::move(V.L[k].K);
        l.earlier = V.L[k].earlier;
        l.n_cand = V.L[k].n_cand;
        l.w_shift = V.L[k].w_shift;
        l.cand_at = V.L[k].cand_at;
        l.off_at = V.L[k].off_at;
        l.n_items = (l.n_cand + 63u) / 64u;  // a single-vertex query; otherwise the scan's total, below
        grid_items = std::max(grid_items, l.n_cand);
    }
    // the cursor's own work areas of every launch, bitmap, S and scan storage, all before the first launch
    if ((rc = vertices_reserve(c, &V, &cur->work, &cur->bitmap, &cur->fset, &cur->tmp)) || (rc = cursor_reserve(who, cur, grid_items))) return rc;
    SetsCall call(who, c, false);
    vertices_stage(call, c, V, candidate_bitmap, nullptr, 0, &cur->work, &cur->bitmap);
    const VerticesWork W(cur->work, cur->n_cand_all, n_launch);
    uint32_t *h_items = cur->h_ctrs + ctrs_bytes(n_launch) / 4;
    for (size_t k = 0; k < n_launch && nq > 1; k++) {
        const DeltaPagesLaunch &l = cur->L[k];
        uint32_t *cand = W.cand + l.cand_at, *item_off = W.item_off + l.off_at, *chunks = W.chunks + l.off_at;
        call.launch([&] {
            hipLaunchKernelGGL(k_sets_cand_chunks, dim3((l.n_cand + 256) / 256), dim3(256), 0, c->stream, l.n_cand, cand, c->adj_deg.as<uint32_t>(),
                               l.w_shift, chunks);
        });
        size_t tb = cur->tmp.bytes;
        if (call.ok()) call.he = hipcub::DeviceScan::ExclusiveSum(cur->tmp.p, tb, chunks, item_off, (int)(l.n_cand + 1), c->stream);
        if (call.ok()) call.he = hipMemcpyAsync(h_items + k, item_off + l.n_cand, 4, hipMemcpyDeviceToHost, c->stream);
    }
    call.wait(cur->ctrs.p, 8);  // (the caller's arrays may go)
    if ((rc = call.finish(nullptr))) return rc;
    for (size_t k = 0; k < n_launch && nq > 1; k++) cur->L[k].n_items = h_items[k];
    cursor_items_left(cur, nullptr);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta_pages] kind=3 vertices=%zu launches=%zu cands=%zu items=%llu slots=%u\n", V.ids.size(), n_launch,
                cur->n_cand_all, (unsigned long long)cur->items_left, cur->blocks * kSetsWavesPerBlock);
    guard.p = nullptr;
    *out = cur;
    return GNNPE_OK;
}

}  // extern "C"

// One page: the row cursor is zeroed, the launches of the first unfinished anchor and of every later one are queued, the counters
// come back -- the one wait of a page -- and the first unfinished anchor is worked out from them.
int gnnpe_delta_pages_next(gnnpe_match_cursor *cur, uint32_t *host_rows, uint64_t *n_rows, int *done, double *device_ms)
{
    gnnpe_ctx *c = cur->c;
    const uint64_t rows_now = std::min(cur->page_rows, cur->limit - cur->delivered);  // >= 1: a met limit sets done
    const SetsQuery &Q = cur->Q;
    const size_t n_launch = cur->L.size();
    DeltaPagesCounters *d_ctr = cur->ctrs.as<DeltaPagesCounters>();
    const uint32_t *adj_start = c->adj_start.as<uint32_t>(), *adj_deg = c->adj_deg.as<uint32_t>(), *nbrs = c->nbrs.as<uint32_t>(),
                   *labels = c->labels.as<uint32_t>(), *bitmap = cur->bitmap.as<uint32_t>();
    PagesSlot *slots = cur->slots.as<PagesSlot>();
    uint32_t *page = cur->page.as<uint32_t>();
    GNNPE_HIP_TRY(hipMemsetAsync(&d_ctr->cursor, 0, 8, c->stream));
    GNNPE_HIP_TRY(hipEventRecord(cur->ev0, c->stream));
    for (size_t k = cur->first; k < n_launch; k++) {
        const DeltaPagesLaunch &l = cur->L[k];
        const uint32_t anchor = (uint32_t)k;
        if (cur->anchor_kind == kAnchorVertices) {
            const VerticesWork W(cur->work, cur->n_cand_all, n_launch);
            const uint32_t *sbits = cur->fset.as<uint32_t>();
            sets_dispatch(l.K, [&](auto... ord) {
                hipLaunchKernelGGL((k_refine_delta_vertices_pages<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(cur->blocks), dim3(kBlock), 0,
                                   c->stream, l.K.P, l.earlier, sbits, l.n_cand, W.cand + l.cand_at, W.item_off + l.off_at, l.n_items, l.w_shift,
                                   adj_start, adj_deg, nbrs, labels, bitmap, Q.words, d_ctr, anchor, slots, page, (unsigned long long)rows_now,
                                   ord...);
            });
        } else {
            const DeltaBuf F(cur->fset, cur->n_keys);
            const uint32_t n_keys = (uint32_t)cur->n_keys;
            sets_dispatch(l.K, [&](auto... ord) {
                if (cur->anchor_kind == kAnchorEdges)
                    hipLaunchKernelGGL((k_refine_delta_pages<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(cur->blocks), dim3(kBlock), 0,
                                       c->stream, l.K.P, l.older, l.n_items, F.pairs, F.ent, F.keys, n_keys, adj_start, adj_deg, nbrs, labels, bitmap,
                                       Q.words, d_ctr, anchor, slots, page, (unsigned long long)rows_now, ord...);
                else
                    hipLaunchKernelGGL((k_refine_delta_nonedges_pages<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(cur->blocks),
                                       dim3(kBlock), 0, c->stream, l.K.P, l.older, l.n_items, F.pairs, F.ent, F.keys, n_keys, adj_start, adj_deg, nbrs,
                                       labels, bitmap, Q.words, d_ctr, anchor, slots, page, (unsigned long long)rows_now, ord...);
            });
        }
        GNNPE_HIP_TRY(hipGetLastError());
    }
    GNNPE_HIP_TRY(hipEventRecord(cur->ev1, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(cur->h_ctrs, d_ctr, ctrs_bytes(n_launch), hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait of a page
    const DeltaPagesCounters &h = *reinterpret_cast<const DeltaPagesCounters *>(cur->h_ctrs);
    const uint32_t *tickets = cur->h_ctrs + sizeof(DeltaPagesCounters) / 4;
    // the cursor's bookkeeping: every valid slot belongs to one anchor, which no finished launch is
    GNNPE_REQUIRE(!h.mismatch && (h.valid == 0 || (h.owner >= cur->first && h.owner < n_launch)), GNNPE_ERR_HIP,
                  "gnnpe_refine_pages_next: a suspend slot of anchor %u met another launch (first unfinished %u)", h.owner, cur->first);
    const uint64_t got = std::min<uint64_t>(h.cursor, rows_now);
    if (got && host_rows) GNNPE_HIP_TRY(hipMemcpy(host_rows, cur->page.p, (size_t)got * Q.nq * 4, hipMemcpyDeviceToHost));
    if (device_ms) {
        float ms = 0.f;
        GNNPE_HIP_TRY(hipEventElapsedTime(&ms, cur->ev0, cur->ev1));
        *device_ms = ms;
    }
    cur->suspended = h.valid;
    if (h.valid) {
        cur->first = h.owner;
    } else {
        while (cur->first < n_launch && tickets[cur->first] >= cur->L[cur->first].n_items) cur->first++;
    }
    cursor_items_left(cur, tickets);
    cur->pages++;
    cur->delivered += got;
    // over: every anchor finished -- or the limit is met, and what the slots hold is never asked for
    if (cur->first >= n_launch || cur->delivered >= cur->limit) {
        cur->done = true;
        cur->suspended = 0;
        cur->items_left = 0;
    }
    *n_rows = got;
    *done = cur->done ? 1 : 0;
    return GNNPE_OK;
}
