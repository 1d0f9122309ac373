// gnnpe_refine_pages.hip -- the set-restricted refinement as a CURSOR over its embeddings: gnnpe_refine_pages_* of
// include/gnnpe_online.h.  Every launch of k_refine_pages fills one page of at most page_rows embeddings; across the launches of
// a cursor every embedding inside the sets comes out exactly once.
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip): one wave per first-level item taken from a ticket counter by a resident
// grid, the whole wave on every row chunk, the set bit, label, degree, injectivity and back-edge tests.  The two kernels share
// every step of it through gnnpe_refine_sets.hip.h -- lane test, descent, item decode, single-vertex item; the host shares the
// preparation of the query and the staging of the items -- and each keeps its own loop, leaf and polling
// (profiles/online_shared_steps.txt compares the gfx950 code with the copies they were).  What is this kernel's own:
//
//   * page cursor: the counters hold a page-relative row cursor, zeroed before every launch, and the ticket, zeroed when the
//     cursor is opened.  At the last depth one atomic add reserves popcount(survivors) rows; a survivor whose row is below
//     page_rows stores it, so every row below min(cursor, page_rows) is written by exactly one lane.  The kernel knows no
//     limit: the host passes min(page_rows, limit - delivered) as the page size.
//   * suspend: a wave whose reservation reaches past the page end stores the survivors that fit and keeps the others as the
//     survivor mask of the last depth -- the LEFTOVER LEAF MASK is stored, the chunk is not evaluated again.  It then writes
//     depth, item and the SetsWave words up to that depth into slot `global wave id` of the slot array, marks the slot valid
//     and leaves.  A single-vertex query keeps its item and the mask (depth 0).  A wave also looks at the cursor every 1024
//     chunks and suspends where it stands once the page is full, so a page does not last as long as a matchless subtree.
//   * resume: the grid is the same for every launch of a cursor and wave w owns slot w.  A wave whose slot is valid loads it
//     and clears it; at the last depth a non-empty mask is emitted from the mask (the lanes read their entries of the chunk
//     again; nothing is tested again).  Only then does the wave take tickets, and before every ticket it reads the cursor: with
//     the page full it takes none.
//   * nothing waits on anything: a wave works, suspends or leaves.
// A launch ends with the page exactly full, or with every item taken and no slot valid: the enumeration is over.
//
// Resources (gfx950, -O3): 53 VGPRs (k_refine_sets: 30), no scratch, 896 B of LDS per wave (3 584 B per workgroup) as
// k_refine_sets; a suspend slot is 912 B of global memory per resident wave (3.6 MiB on 256 CUs).  The ordered instantiation
// (gnnpe_refine_pages_open_distinct) has 58 VGPRs and no scratch; slot and LDS are the same.  The two induced instantiations
// (gnnpe_refine_pages_open_mode with GNNPE_MATCH_INDUCED): profiles/online_induced.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_pages.hip.h"

namespace gnnpe {

struct PagesCounters {  // one 32-byte block, copied back once per page
    unsigned long long cursor;  // rows reserved in this page (may pass page_rows); zeroed before every launch
    uint32_t suspended, pad0;   // waves that saved their state in this launch; zeroed before every launch
    uint32_t ticket, pad1[3];   // first-level items handed out; zeroed when the cursor is opened
};
static_assert(sizeof(PagesCounters) == SetsWork::kCtrBytes, "the counters of the work buffer");
constexpr size_t kPagesPerLaunchBytes = 16;  // the part of PagesCounters zeroed before every launch

// One kernel, four instantiations.  k_refine_pages<false> is the plain search: the parameter pack is empty, nothing below that is
// `if constexpr (kOrdered)` exists (here and in the shared steps), and the code is what it was before the ordered form existed.
// k_refine_pages<true, SetsOrder> is the ordered search (D(C, limit): one embedding per distinct subgraph): one more by-value
// argument, the bounds of SetsOrder in every chunk's test, and the long pivot rows trimmed to them.  The bounds are
// derived from the images, which a suspended wave saves and restores: the slot holds nothing new.
// k_refine_pages<false, SetsNon> and k_refine_pages<true, SetsOrder, SetsNon> add the induced test of sets_lane_test (SetsNon, the
// last by-value argument).  It reads the images too, so the slot is the same again, and the leftover leaf mask of a resumed wave
// holds lanes that passed it: they are emitted without a test, as ever.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_pages(SetsPlan P, uint32_t n_cand, const uint32_t *__restrict__ cand,
                                                        const uint32_t *__restrict__ item_off, uint32_t n_items, uint32_t w_shift,
                                                        const uint32_t *__restrict__ adj_start,
                                                        const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                        const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                        uint64_t words, PagesCounters *ctr, PagesSlot *slots,
                                                        uint32_t *__restrict__ page, unsigned long long page_rows, Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    volatile uint32_t *Sw = reinterpret_cast<volatile uint32_t *>(&s_wave[threadIdx.x >> 6]);
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nq = P.nq, last = nq - 1;
    PagesSlot *slot = slots + ((size_t)blockIdx.x * kSetsWavesPerBlock + (threadIdx.x >> 6));

    // the survivors `m` of a chunk at the last depth (lane's entry v): reserve their rows, store the ones inside the page;
    // returns the survivors whose row lies past the page end
    auto emit = [&](uint32_t d, unsigned long long m, uint32_t v) -> unsigned long long {
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(&ctr->cursor, (unsigned long long)__popcll(m));
        at = uni64(at) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        const bool mine = ((m >> lane) & 1ull) != 0;
        if (mine && at < page_rows) {
            uint32_t *row = page + at * nq;
            for (uint32_t i = 0; i < d; i++) row[P.qv[i]] = S.image[i];
            row[P.qv[d]] = v;
        }
        return __ballot(mine && at >= page_rows);
    };
    // save depth, item and the state words of depths 0 .. d; the wave leaves after it.  The words are wave-uniform and every
    // lane holds what it wrote itself: one lane stores them, and a resuming wave has every lane write every word again, so
    // that no lane ever reads LDS that only another lane wrote (as in k_refine_sets)
    auto suspend = [&](uint32_t d, uint32_t q) {
        if (lane == 0) {
#pragma unroll 1
            for (uint32_t a = 0; a < kWaveWords; a += (uint32_t)kSetsMaxQ)
#pragma unroll 1
                for (uint32_t i = 0; i <= d; i++) slot->w[a + i] = Sw[a + i];
            slot->depth = d;
            slot->item = q;
            slot->valid = 1u;
            atomicAdd(&ctr->suspended, 1u);
        }
    };

    uint32_t q = 0, d = 0;
    bool resumed = uni(slot->valid) != 0;
    if (resumed) {
        d = uni(slot->depth);
        q = uni(slot->item);
#pragma unroll 1
        for (uint32_t a = 0; a < kWaveWords; a += (uint32_t)kSetsMaxQ)
#pragma unroll 1
            for (uint32_t i = 0; i <= d; i++) Sw[a + i] = slot->w[a + i];
        if (lane == 0) slot->valid = 0u;
    }

    for (;; resumed = false) {
        if (!resumed) {
            // the page is full: no ticket; every item is taken: none either (the ticket never runs far past the items)
            if (__hip_atomic_load(&ctr->cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= page_rows) return;
            if (__hip_atomic_load(&ctr->ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_items) return;
            if (lane == 0) q = atomicAdd(&ctr->ticket, 1u);
            q = uni(q);
            if (q >= n_items) return;
        }

        if (nq == 1) {
            // item q = 64 start candidates; the mask of depth 0 holds the ones not yet delivered
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            unsigned long long m;
            if (resumed)
                m = ((unsigned long long)uni(S.mask_hi[0]) << 32) | uni(S.mask_lo[0]);
            else
                m = __ballot(sets_single_test(P, G, n_cand, i, v));
            if (m == 0) continue;
            m = emit(0, m, v);
            if (m) {
                S.mask_lo[0] = (uint32_t)m;
                S.mask_hi[0] = (uint32_t)(m >> 32);
                suspend(0, q);
                return;
            }
            continue;
        }

        if (!resumed) {
            if (!sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) continue;
            d = 1;
        }
        uint32_t steps = 0;
        while (d >= 1) {
            // a subtree that finds little still hears of the page's end: a look at the cursor every 1024 chunks
            if ((++steps & 1023u) == 0 && __hip_atomic_load(&ctr->cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= page_rows) {
                suspend(d, q);
                return;
            }
            unsigned long long m = ((unsigned long long)uni(S.mask_hi[d]) << 32) | uni(S.mask_lo[d]);
            if (m == 0) {
                // next chunk of the pivot row
                const uint32_t cb = uni(S.cbase[d]) + 64u, ce = uni(S.end[d]);
                if ((int32_t)(ce - cb) <= 0) {
                    d--;
                    continue;
                }
                S.cbase[d] = cb;
                uint32_t v;
                const bool ok = sets_lane_test<kOrdered>(P, S, G, d, cb, ce, lane, v, ord...);
                m = __ballot(ok);
                if (m == 0) continue;
                if (d == last) {
                    m = emit(d, m, v);
                    if (m) {
                        S.mask_lo[d] = (uint32_t)m;
                        S.mask_hi[d] = (uint32_t)(m >> 32);
                        suspend(d, q);
                        return;
                    }
                    continue;
                }
            } else if (d == last) {
                // (after a resume only) the survivors a full page left behind: their entries again, no test again
                const uint32_t v = ((m >> lane) & 1ull) ? nbrs[uni(S.cbase[d]) + lane] : 0u;
                m = emit(d, m, v);
                S.mask_lo[d] = (uint32_t)m;
                S.mask_hi[d] = (uint32_t)(m >> 32);
                if (m) {
                    suspend(d, q);
                    return;
                }
                continue;
            }
            sets_descend<kOrdered>(P, S, G, d, m, lane, ord...);
        }
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// The cursor object is in gnnpe_refine_pages.hip.h: the delta cursors of gnnpe_refine_delta_pages.hip are served by the calls below too.
extern "C" {

void gnnpe_refine_pages_close(gnnpe_match_cursor *cur)
{
    if (!cur) return;
    (void)hipSetDevice(cur->c->device);
    (void)hipStreamSynchronize(cur->c->stream);
    if (cur->ev0) (void)hipEventDestroy(cur->ev0);
    if (cur->ev1) (void)hipEventDestroy(cur->ev1);
    if (cur->h_ctrs) (void)hipHostFree(cur->h_ctrs);
    delete cur;  // the buffers free themselves
}

}  // extern "C"

// gnnpe_refine_pages_open (mode 0), gnnpe_refine_pages_open_distinct (GNNPE_MATCH_DISTINCT) and gnnpe_refine_pages_open_mode
static int refine_pages_open(const char *who, uint32_t mode, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                             uint64_t limit, uint64_t page_rows, gnnpe_match_cursor **out)
{
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && out, GNNPE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    GNNPE_REQUIRE(page_rows > 0, GNNPE_ERR_ARG, "%s: page_rows must be at least 1", who);
    SetsQuery Q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q);
    if (rc) return rc;
    gnnpe_match_cursor *cur = new gnnpe_match_cursor();
    struct Guard {  // every early return below closes the cursor unless it was handed out
        gnnpe_match_cursor *p;
        ~Guard() { gnnpe_refine_pages_close(p); }
    } guard{cur};
    cur->c = c;
    cur->graph_gen = c->graph_gen;
    cur->Q = std::move(Q);
    cur->limit = limit;
    cur->page_rows = page_rows;
    cur->page_cap = std::min(page_rows, limit);
    if (cur->Q.empty) {  // limit 0 or an empty set: a cursor that is done before its first page
        cur->done = true;
        guard.p = nullptr;
        *out = cur;
        return GNNPE_OK;
    }
    const uint32_t nq = cur->Q.nq, n_cand = cur->Q.n_cand;

    cur->blocks = sets_grid_blocks(c, nq, n_cand);  // the same for every launch
    const size_t slot_bytes = (size_t)cur->blocks * kSetsWavesPerBlock * sizeof(PagesSlot);
    GNNPE_REQUIRE(cur->page_cap <= (~(size_t)0 >> 1) / ((size_t)nq * 4), GNNPE_ERR_RANGE,
                  "%s: a page of %llu rows does not fit an allocation", who, (unsigned long long)cur->page_cap);
    if ((rc = cur->slots.reserve(slot_bytes)) || (rc = cur->page.reserve((size_t)cur->page_cap * nq * 4))) return rc;
    GNNPE_HIP_TRY(hipEventCreate(&cur->ev0));
    GNNPE_HIP_TRY(hipEventCreate(&cur->ev1));
    if ((rc = sets_stage_items(c, &cur->Q, candidate_bitmap, cur->work, cur->bitmap, cur->tmp))) return rc;
    GNNPE_HIP_TRY(hipMemsetAsync(cur->slots.p, 0, slot_bytes, c->stream));  // no slot is valid
    cur->n_items = (n_cand + 63u) / 64u;
    // the item count comes to the host once, here: the info call and the end test want it
    if (nq > 1)
        GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, SetsWork(cur->work, n_cand).item_off + n_cand, 4, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // (the start candidates and the caller's bitmap may go)
    std::vector<uint32_t>().swap(cur->Q.cand);
    if (nq > 1) cur->n_items = (uint32_t)c->h_pinned[0];
    if (c->sw.debug)
        fprintf(stderr, "[refine_pages] shift=%u forced=%d cands=%u items=%u slots=%u\n", cur->Q.w_shift, (int)cur->Q.forced, n_cand,
                cur->n_items, cur->blocks * kSetsWavesPerBlock);
    guard.p = nullptr;
    *out = cur;
    return GNNPE_OK;
}

extern "C" {

int gnnpe_refine_pages_open(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                            uint64_t page_rows, gnnpe_match_cursor **out)
{
    return refine_pages_open("gnnpe_refine_pages_open", 0u, c, query_graph_path, candidate_bitmap, limit, page_rows, out);
}

int gnnpe_refine_pages_open_distinct(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                                     uint64_t page_rows, gnnpe_match_cursor **out)
{
    return refine_pages_open("gnnpe_refine_pages_open_distinct", GNNPE_MATCH_DISTINCT, c, query_graph_path, candidate_bitmap, limit,
                             page_rows, out);
}

int gnnpe_refine_pages_open_mode(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                                 uint64_t page_rows, uint32_t mode, gnnpe_match_cursor **out)
{
    return refine_pages_open("gnnpe_refine_pages_open_mode", mode, c, query_graph_path, candidate_bitmap, limit, page_rows, out);
}

int gnnpe_refine_pages_next(gnnpe_match_cursor *cur, uint32_t *host_rows, uint64_t *n_rows, int *done, double *device_ms)
{
    GNNPE_REQUIRE(cur && n_rows && done, GNNPE_ERR_ARG, "gnnpe_refine_pages_next: null argument");
    gnnpe_ctx *c = cur->c;
    *n_rows = 0;
    *done = cur->done ? 1 : 0;
    if (device_ms) *device_ms = 0.0;
    if (cur->done) return GNNPE_OK;
    GNNPE_REQUIRE(cur->graph_gen == c->graph_gen && c->have_graph && c->rows_identity && !c->multigraph, GNNPE_ERR_ARG,
                  "gnnpe_refine_pages_next: the context's graph was loaded or changed after the cursor was opened; close the cursor");
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if (cur->anchor_kind) return gnnpe_delta_pages_next(cur, host_rows, n_rows, done, device_ms);
    const uint64_t rows_now = std::min(cur->page_rows, cur->limit - cur->delivered);  // >= 1: a met limit sets done
    const SetsQuery &Q = cur->Q;
    const SetsWork W(cur->work, Q.n_cand);
    PagesCounters *d_ctr = static_cast<PagesCounters *>(W.ctr);
    GNNPE_HIP_TRY(hipMemsetAsync(d_ctr, 0, kPagesPerLaunchBytes, c->stream));
    GNNPE_HIP_TRY(hipEventRecord(cur->ev0, c->stream));
    sets_dispatch(Q, [&](auto... ord) {
        hipLaunchKernelGGL((k_refine_pages<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(cur->blocks), dim3(kBlock), 0, c->stream, Q.P, Q.n_cand,
                           W.cand, W.item_off, cur->n_items, Q.w_shift, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), cur->bitmap.as<uint32_t>(), Q.words, d_ctr,
                           cur->slots.as<PagesSlot>(), cur->page.as<uint32_t>(), (unsigned long long)rows_now, ord...);
    });
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipEventRecord(cur->ev1, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, d_ctr, sizeof(PagesCounters), hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait of a page
    const uint32_t *h32 = reinterpret_cast<const uint32_t *>(c->h_pinned);
    const uint64_t got = std::min<uint64_t>(c->h_pinned[0], rows_now);
    cur->suspended = h32[2];
    cur->ticket = h32[4];
    if (got && host_rows) GNNPE_HIP_TRY(hipMemcpy(host_rows, cur->page.p, (size_t)got * Q.nq * 4, hipMemcpyDeviceToHost));
    if (device_ms) {
        float ms = 0.f;
        GNNPE_HIP_TRY(hipEventElapsedTime(&ms, cur->ev0, cur->ev1));
        *device_ms = ms;
    }
    cur->pages++;
    cur->delivered += got;
    // over: every item taken and no wave holds a state -- or the limit is met, and what the slots hold is never asked for
    if ((cur->suspended == 0 && cur->ticket >= cur->n_items) || cur->delivered >= cur->limit) {
        cur->done = true;
        cur->suspended = 0;
        cur->ticket = cur->n_items;
    }
    *n_rows = got;
    *done = cur->done ? 1 : 0;
    return GNNPE_OK;
}

int gnnpe_refine_pages_device_ptr(gnnpe_match_cursor *cur, void **dev_rows, uint32_t *n_query_vertices)
{
    GNNPE_REQUIRE(cur && dev_rows, GNNPE_ERR_ARG, "gnnpe_refine_pages_device_ptr: null argument");
    *dev_rows = cur->page.p;
    if (n_query_vertices) *n_query_vertices = cur->Q.nq;
    return GNNPE_OK;
}

int gnnpe_refine_pages_info(gnnpe_match_cursor *cur, uint64_t info[5])
{
    GNNPE_REQUIRE(cur && info, GNNPE_ERR_ARG, "gnnpe_refine_pages_info: null argument");
    info[0] = cur->pages;
    info[1] = cur->delivered;
    info[2] = cur->suspended;
    info[3] = cur->anchor_kind ? cur->items_left : cur->n_items - std::min(cur->ticket, cur->n_items);
    info[4] = (uint64_t)cur->blocks * kSetsWavesPerBlock;
    return GNNPE_OK;
}

}  // extern "C"
