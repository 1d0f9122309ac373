// gnnpe_refine_pages.hip -- the set-restricted refinement as a CURSOR over its embeddings: gnnpe_refine_pages_* of
// include/gnnpe_online.h.  Every launch of k_refine_pages fills one page of at most page_rows embeddings; across the launches of
// a cursor every embedding inside the sets comes out exactly once.
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip; the plan, the wave state and the first-level items are shared through
// gnnpe_refine_sets.hip.h): one wave per first-level item taken from a ticket counter by a resident grid, the whole wave on every
// row chunk, the set bit, label, degree, injectivity and back-edge tests.  The kernel is a second kernel, not a shared body:
// k_refine_sets' code is what it was.  What differs:
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
// (gnnpe_refine_pages_open_distinct) has 58 VGPRs and no scratch; slot and LDS are the same.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/gnnpe_online.h"
#include "../host/graph_loader.h"
#include "../host/query_symmetry.h"
#include "../host/refine.h"
#include "gnnpe_common.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

struct PagesCounters {  // one 32-byte block, copied back once per page
    unsigned long long cursor;  // rows reserved in this page (may pass page_rows); zeroed before every launch
    uint32_t suspended, pad0;   // waves that saved their state in this launch; zeroed before every launch
    uint32_t ticket, pad1[3];   // first-level items handed out; zeroed when the cursor is opened
};
constexpr size_t kPagesPerLaunchBytes = 16;  // the part of PagesCounters zeroed before every launch

constexpr uint32_t kWaveWords = sizeof(SetsWave) / 4;  // 7 arrays of kSetsMaxQ words: word a * kSetsMaxQ + i belongs to depth i

struct PagesSlot {  // saved state of one wave
    uint32_t valid, depth, item, pad;
    uint32_t w[kWaveWords];  // the SetsWave words of depths 0 .. depth
};

// One kernel, two instantiations.  k_refine_pages<false> is the plain search: the parameter pack is empty, nothing below that is
// `if constexpr (kOrdered)` exists, and the code is instruction for instruction what it was before the ordered form existed.
// k_refine_pages<true, SetsOrder> is the ordered search (D(C, limit): one embedding per distinct subgraph): one more by-value
// argument, the bounds of SetsOrder in every chunk's test, and the long pivot rows trimmed to them.  The bounds are
// derived from the images, which a suspended wave saves and restores: the slot holds nothing new.
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
            const uint32_t i = q * 64u + lane;
            const uint32_t v = i < n_cand ? cand[i] : 0u;
            unsigned long long m;
            if (resumed)
                m = ((unsigned long long)uni(S.mask_hi[0]) << 32) | uni(S.mask_lo[0]);
            else
                m = __ballot(i < n_cand && labels[v] == P.label[0] && adj_deg[v] >= P.degree[0]);
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
            // item -> (start candidate, chunk of its row): largest ci with item_off[ci] <= q
            uint32_t lo = 0, hi = n_cand;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (item_off[mid] <= q) lo = mid; else hi = mid;
            }
            lo = uni(lo);
            const uint32_t v0 = uni(cand[lo]);
            const uint32_t s0 = uni(adj_start[v0]), d0 = uni(adj_deg[v0]);
            if (uni(labels[v0]) != P.label[0] || d0 < P.degree[0]) continue;
            S.image[0] = v0;
            S.istart[0] = s0;
            S.ideg[0] = d0;
            // depth 1 (its pivot is position 0) is held to this item's chunk
            const uint32_t c0 = s0 + ((q - uni(item_off[lo])) << w_shift);
            S.cbase[1] = c0 - 64u;
            S.end[1] = min(c0 + (1u << w_shift), s0 + d0);
            S.mask_lo[1] = 0;
            S.mask_hi[1] = 0;
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
                const uint32_t idx = cb + lane;
                bool ok = idx < ce;
                const uint32_t v = ok ? nbrs[idx] : 0u;
                const uint32_t word = bitmap[(uint64_t)P.qv[d] * words + (v >> 5)], lab = labels[v], dv = adj_deg[v];
                ok = ok & (((word >> (v & 31u)) & 1u) != 0) & (lab == P.label[d]) & (dv >= P.degree[d]);
                if constexpr (kOrdered) {
                    uint32_t lo, hi;
                    order_bounds(sets_order(ord...), S, d, lo, hi);
                    ok = ok & (v >= lo) & (v < hi);
                }
                for (uint32_t i = 0; i < d; i++) ok &= S.image[i] != v;
                if (ok && P.back_off[d] < P.back_off[d + 1]) {
                    const uint32_t vs = adj_start[v];
                    for (uint32_t j = P.back_off[d]; j < P.back_off[d + 1] && ok; j++) {
                        const uint32_t b = P.back[j], w = S.image[b], ws = S.istart[b], dw = S.ideg[b];
                        ok = dv <= dw ? row_has(nbrs, vs, dv, w) : row_has(nbrs, ws, dw, v);
                    }
                }
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
            // descend into the next survivor of this chunk
            const uint32_t bit = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            S.mask_lo[d] = (uint32_t)m;
            S.mask_hi[d] = (uint32_t)(m >> 32);
            const uint32_t v = uni(nbrs[uni(S.cbase[d]) + bit]);
            S.image[d] = v;
            S.istart[d] = uni(adj_start[v]);
            S.ideg[d] = uni(adj_deg[v]);
            d++;
            const uint32_t p = P.pivot[d], ps = uni(S.istart[p]);
            if constexpr (kOrdered) {
                uint32_t rb = ps, re = ps + uni(S.ideg[p]);
                if (sets_order(ord...).trim) {
                    uint32_t lo, hi;
                    order_bounds(sets_order(ord...), S, d, lo, hi);
                    order_trim(nbrs, lo, hi, lane, rb, re);
                }
                S.cbase[d] = rb - 64u;
                S.end[d] = re;
            } else {
                S.cbase[d] = ps - 64u;
                S.end[d] = ps + uni(S.ideg[p]);
            }
            S.mask_lo[d] = 0;
            S.mask_hi[d] = 0;
        }
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// A cursor owns everything its launches write or read besides the graph: two cursors, the one-shot gnnpe_refine_sets and the
// filters interleave freely on one context.
struct gnnpe_match_cursor {
    gnnpe_ctx *c = nullptr;
    uint64_t graph_gen = 0;  // the context's graph when the cursor was opened
    SetsPlan P = {};
    SetsOrder O = {};  // of a distinct cursor
    uint32_t n_pairs = 0;  // 0: the plain kernel
    uint32_t nq = 0, n_cand = 0, n_items = 0, w_shift = 6, blocks = 0;
    uint64_t words = 0, limit = 0, page_rows = 0, page_cap = 0;  // page_cap: rows the page buffer holds, min(page_rows, limit)
    uint64_t delivered = 0, pages = 0;
    uint32_t suspended = 0, ticket = 0;  // of the last page
    bool done = false;
    // work: [counters 32 B | item_off u32 x (n_cand + 1) | cand u32 x n_cand | chunks u32 x (n_cand + 1)]
    DevBuf work, bitmap, slots, page, tmp;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

extern "C" {

void gnnpe_refine_pages_close(gnnpe_match_cursor *cur)
{
    if (!cur) return;
    (void)hipSetDevice(cur->c->device);
    (void)hipStreamSynchronize(cur->c->stream);
    if (cur->ev0) (void)hipEventDestroy(cur->ev0);
    if (cur->ev1) (void)hipEventDestroy(cur->ev1);
    delete cur;  // the buffers free themselves
}

}  // extern "C"

// gnnpe_refine_pages_open (distinct = false) and gnnpe_refine_pages_open_distinct
static int refine_pages_open(const char *who, bool distinct, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                             uint64_t limit, uint64_t page_rows, gnnpe_match_cursor **out)
{
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && out, GNNPE_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    GNNPE_REQUIRE(page_rows > 0, GNNPE_ERR_ARG, "%s: page_rows must be at least 1", who);
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    gnnpe_host::StaticGraph q;
    std::string err;
    int rc = q.load(query_graph_path, &err);
    if (rc != 0) {
        set_error("%s", err.c_str());
        return rc;
    }
    const uint32_t nq = q.n;
    GNNPE_REQUIRE(nq >= 1 && nq <= (uint32_t)kSetsMaxQ, GNNPE_ERR_UNSUPPORTED, "query graphs of 1..%d vertices (got %u)", kSetsMaxQ, nq);
    const uint64_t words = ((uint64_t)c->n + 31) / 32;
    std::vector<uint64_t> cnt(nq, 0);
    for (uint32_t u = 0; u < nq; u++)
        for (uint64_t w = 0; w < words; w++) cnt[u] += (uint64_t)__builtin_popcount(candidate_bitmap[(size_t)u * words + w]);
    gnnpe_host::MatchOrder mo;
    if (gnnpe_host::build_match_order(q, cnt, &mo, &err) != 0) {
        set_error("%s", err.c_str());
        return GNNPE_ERR_ARG;
    }
    // plan by position in the order
    gnnpe_match_cursor *cur = new gnnpe_match_cursor();
    struct Guard {  // every early return below closes the cursor unless it was handed out
        gnnpe_match_cursor *p;
        ~Guard() { gnnpe_refine_pages_close(p); }
    } guard{cur};
    cur->c = c;
    cur->graph_gen = c->graph_gen;
    cur->nq = nq;
    cur->words = words;
    cur->limit = limit;
    cur->page_rows = page_rows;
    cur->page_cap = std::min(page_rows, limit);
    SetsPlan &P = cur->P;
    P.nq = nq;
    std::vector<uint32_t> pos_of(nq, 0);
    for (uint32_t i = 0; i < nq; i++) pos_of[mo.order[i]] = i;
    GNNPE_REQUIRE(mo.back.size() <= sizeof(P.back), GNNPE_ERR_UNSUPPORTED, "query graph too dense");
    for (uint32_t i = 0; i < nq; i++) {
        P.label[i] = q.labels[mo.order[i]];
        P.degree[i] = q.degree(mo.order[i]);
        P.qv[i] = (uint8_t)mo.order[i];
        P.pivot[i] = (uint8_t)pos_of[mo.pivot[i]];
        P.back_off[i] = (uint16_t)mo.back_off[i];
    }
    P.back_off[nq] = (uint16_t)mo.back_off[nq];
    for (size_t j = 0; j < mo.back.size(); j++) P.back[j] = (uint8_t)pos_of[mo.back[j]];
    // the ordering constraints by position; a query without symmetry has none and runs the plain kernel
    if (distinct) cur->n_pairs = sets_order_from_pairs(gnnpe_host::query_symmetry(q).pairs, pos_of, c->sw.sets_trim, &cur->O);
    // start candidates; limit 0 or an empty set anywhere: a cursor that is done before its first page
    std::vector<uint32_t> cand;
    bool empty = limit == 0;
    for (uint32_t u = 0; u < nq; u++) empty |= cnt[u] == 0;
    if (!empty) {
        const uint32_t start = mo.order[0];
        cand.reserve(cnt[start]);
        for (uint64_t w = 0; w < words; w++)
            for (uint32_t bits = candidate_bitmap[(size_t)start * words + w]; bits; bits &= bits - 1) {
                const uint64_t v = w * 32 + __builtin_ctz(bits);
                if (v < c->n) cand.push_back((uint32_t)v);
            }
    }
    const uint32_t n_cand = (uint32_t)cand.size();
    cur->n_cand = n_cand;
    if (n_cand == 0) {
        cur->done = true;
        guard.p = nullptr;
        *out = cur;
        return GNNPE_OK;
    }

    // a resident grid, the same for every launch; a single-vertex query needs no more waves than it has items
    uint64_t blocks = (uint64_t)std::max(c->num_cus, 1) * kSetsBlocksPerCu;
    if (nq == 1) blocks = std::min<uint64_t>(blocks, ((uint64_t)(n_cand + 63) / 64 + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
    cur->blocks = (uint32_t)blocks;
    const size_t bm_bytes = (size_t)nq * words * 4, slot_bytes = (size_t)blocks * kSetsWavesPerBlock * sizeof(PagesSlot);
    GNNPE_REQUIRE(cur->page_cap <= (~(size_t)0 >> 1) / ((size_t)nq * 4), GNNPE_ERR_RANGE,
                  "%s: a page of %llu rows does not fit an allocation", who, (unsigned long long)cur->page_cap);
    if ((rc = cur->work.reserve(sizeof(PagesCounters) + ((size_t)n_cand * 3 + 2) * 4 + 64)) || (rc = cur->bitmap.reserve(bm_bytes)) ||
        (rc = cur->slots.reserve(slot_bytes)) || (rc = cur->page.reserve((size_t)cur->page_cap * nq * 4)))
        return rc;
    PagesCounters *d_ctr = cur->work.as<PagesCounters>();
    uint32_t *item_off = reinterpret_cast<uint32_t *>(d_ctr + 1), *d_cand = item_off + n_cand + 1, *d_chunks = d_cand + n_cand;
    GNNPE_HIP_TRY(hipEventCreate(&cur->ev0));
    GNNPE_HIP_TRY(hipEventCreate(&cur->ev1));
    GNNPE_HIP_TRY(hipMemcpyAsync(d_cand, cand.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(cur->bitmap.p, candidate_bitmap, bm_bytes, hipMemcpyHostToDevice, c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(PagesCounters), c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(cur->slots.p, 0, slot_bytes, c->stream));  // no slot is valid
    // GNNPE_TESTING=sets_first_shift=K stands in for the heuristic; the 32-bit item offsets still come first
    const bool forced = c->sw.sets_first_shift >= 0 && c->nbr_used + c->n < (1ull << 32);
    cur->w_shift = forced ? (uint32_t)c->sw.sets_first_shift : sets_first_level_shift(n_cand, c->nbr_used, c->n, c->num_cus, c->n_hub);
    cur->n_items = (n_cand + 63u) / 64u;
    if (nq > 1) {
        hipLaunchKernelGGL(k_sets_cand_chunks, dim3((n_cand + 256) / 256), dim3(256), 0, c->stream, n_cand, d_cand,
                           c->adj_deg.as<uint32_t>(), cur->w_shift, d_chunks);
        size_t tb = 0;
        GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_chunks, item_off, (int)(n_cand + 1), c->stream));
        if ((rc = cur->tmp.reserve(tb))) return rc;
        GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cur->tmp.p, tb, d_chunks, item_off, (int)(n_cand + 1), c->stream));
        // the item count comes to the host once, here: the info call and the end test want it
        GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, item_off + n_cand, 4, hipMemcpyDeviceToHost, c->stream));
    }
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // (cand and the caller's bitmap may go)
    if (nq > 1) cur->n_items = (uint32_t)c->h_pinned[0];
    if (c->sw.debug)
        fprintf(stderr, "[refine_pages] shift=%u forced=%d cands=%u items=%u slots=%u\n", cur->w_shift, (int)forced, n_cand,
                cur->n_items, cur->blocks * kSetsWavesPerBlock);
    guard.p = nullptr;
    *out = cur;
    return GNNPE_OK;
}

extern "C" {

int gnnpe_refine_pages_open(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                            uint64_t page_rows, gnnpe_match_cursor **out)
{
    return refine_pages_open("gnnpe_refine_pages_open", false, c, query_graph_path, candidate_bitmap, limit, page_rows, out);
}

int gnnpe_refine_pages_open_distinct(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                                     uint64_t page_rows, gnnpe_match_cursor **out)
{
    return refine_pages_open("gnnpe_refine_pages_open_distinct", true, c, query_graph_path, candidate_bitmap, limit, page_rows, out);
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
    const uint64_t rows_now = std::min(cur->page_rows, cur->limit - cur->delivered);  // >= 1: a met limit sets done
    PagesCounters *d_ctr = cur->work.as<PagesCounters>();
    uint32_t *item_off = reinterpret_cast<uint32_t *>(d_ctr + 1), *d_cand = item_off + cur->n_cand + 1;
    GNNPE_HIP_TRY(hipMemsetAsync(d_ctr, 0, kPagesPerLaunchBytes, c->stream));
    GNNPE_HIP_TRY(hipEventRecord(cur->ev0, c->stream));
    if (cur->n_pairs)
        hipLaunchKernelGGL((k_refine_pages<true, SetsOrder>), dim3(cur->blocks), dim3(kBlock), 0, c->stream, cur->P, cur->n_cand, d_cand,
                           item_off, cur->n_items, cur->w_shift, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), cur->bitmap.as<uint32_t>(), cur->words, d_ctr,
                           cur->slots.as<PagesSlot>(), cur->page.as<uint32_t>(), (unsigned long long)rows_now, cur->O);
    else
        hipLaunchKernelGGL((k_refine_pages<false>), dim3(cur->blocks), dim3(kBlock), 0, c->stream, cur->P, cur->n_cand, d_cand, item_off,
                           cur->n_items, cur->w_shift, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(),
                           c->labels.as<uint32_t>(), cur->bitmap.as<uint32_t>(), cur->words, d_ctr, cur->slots.as<PagesSlot>(),
                           cur->page.as<uint32_t>(), (unsigned long long)rows_now);
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipEventRecord(cur->ev1, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, d_ctr, sizeof(PagesCounters), hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait of a page
    const uint32_t *h32 = reinterpret_cast<const uint32_t *>(c->h_pinned);
    const uint64_t got = std::min<uint64_t>(c->h_pinned[0], rows_now);
    cur->suspended = h32[2];
    cur->ticket = h32[4];
    if (got && host_rows) GNNPE_HIP_TRY(hipMemcpy(host_rows, cur->page.p, (size_t)got * cur->nq * 4, hipMemcpyDeviceToHost));
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
    if (n_query_vertices) *n_query_vertices = cur->nq;
    return GNNPE_OK;
}

int gnnpe_refine_pages_info(gnnpe_match_cursor *cur, uint64_t info[5])
{
    GNNPE_REQUIRE(cur && info, GNNPE_ERR_ARG, "gnnpe_refine_pages_info: null argument");
    info[0] = cur->pages;
    info[1] = cur->delivered;
    info[2] = cur->suspended;
    info[3] = cur->n_items - std::min(cur->ticket, cur->n_items);
    info[4] = (uint64_t)cur->blocks * kSetsWavesPerBlock;
    return GNNPE_OK;
}

}  // extern "C"
