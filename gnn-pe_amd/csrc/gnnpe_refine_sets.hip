// gnnpe_refine_sets.hip -- the SET-RESTRICTED refinement on the device: R(C, limit) of include/gnnpe_online.h.
//
// gnnpe_refine.hip (frozen) restates the reference: the start vertex is taken from its candidate set, every other level
// walks a whole adjacency row with one thread.  Here every level is restricted to its set, and a whole WAVE works on
// every row:
//
//   * a work item is (start candidate, 64-entry chunk of its row); a resident grid takes items from a ticket counter and a
//     wave leaves when the counter passes the item count (nothing spins).  The item offsets are scanned on the device and
//     the kernel reads their total there, so the host waits once, at the end.  On a graph with rows longer than a chunk, where
//     the subtrees below one entry differ by orders of magnitude, a start set so small that 64-entry chunks would leave
//     most of the resident waves without an item is cut into chunks of 32, 16, ... 1 entries instead
//     (sets_first_level_shift): the items are all the balancing there is.
//   * at depth d the wave reads the pivot image's row in chunks of 64, one entry per lane, coalesced.  A lane tests its v:
//     bit v of C(order[d]), label, degree, not in the image, every back edge by binary search in the SHORTER of the two
//     rows.  __ballot gives the survivors; at the last depth the wave adds their number (and writes their rows), above it
//     it descends into them one at a time.
//   * the search state is wave-uniform -- per depth the chunk base, the row end and the survivor mask, plus the image with
//     its rows' start and length -- and lives in LDS (896 bytes per wave); nothing is a dynamically indexed per-lane array.
//   * limit: a wave adds its finds to the total at the end of an item and at least every 1024 finds, reads the total before
//     an item, with each of those adds and every 1024 chunks, and leaves once the total has reached the limit.
//   * matches: at the last depth one atomic add on a row cursor reserves popcount(mask) rows; lanes whose row is below the
//     cap store image + own v in query-vertex order.
//   * ordered form (gnnpe_refine_sets_distinct: D(C, limit), one embedding per distinct subgraph): the pairs of
//     host/query_symmetry.h become, per position, two masks of earlier positions whose images bound this one from below and
//     from above (SetsOrder).  Per chunk the wave derives the two bounds from the images in LDS and every lane adds
//     lo <= v < hi to its test; when a depth is entered over a pivot row longer than a chunk, the row is first cut to the
//     part that can hold such ids by a wave-wide search (row_lower_bound: 64 probes and a ballot per step).  31 VGPRs, no
//     scratch; the plain instantiation has none of it (30 VGPRs).
//   * induced form (gnnpe_refine_sets_mode with GNNPE_MATCH_INDUCED: I(C, limit) and ID(C, limit)): per position a mask of the
//     earlier positions that are no query neighbours (SetsNon).  A lane that passed every other test searches each of their
//     images' rows, or its own, whichever is shorter, and fails if the edge is there: a subtree is cut at its first wrong vertex.
//     Two more instantiations, plain and ordered; the two above hold none of it.  Figures: profiles/online_induced.txt.
// host/refine_sets.cpp is the host form.  The paged form of this search (gnnpe_refine_pages.hip) takes the same steps, and every
// step exists once, in gnnpe_refine_sets.hip.h: the lane test of a chunk, the descent, the item decode and the single-vertex item
// on the device; the preparation of a query and the staging of its items on the host.  This file keeps what is the one-shot
// call's own: the kernel's loop, its leaf (total, flush, limit) and its polling; the events and the single wait of the host.
// The gfx950 code of both kernels against the copies they were: profiles/online_shared_steps.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

struct SetsCounters {  // one 32-byte block, zeroed before every launch
    unsigned long long total, cursor;
    uint32_t ticket, pad[3];
};
static_assert(sizeof(SetsCounters) == SetsWork::kCtrBytes, "the counters of the work buffer");

// One kernel, four instantiations.  k_refine_sets<false> is the plain search: the parameter pack is empty, nothing below that is
// `if constexpr (kOrdered)` exists (here and in the shared steps), and the code is what it was before the ordered form existed.
// k_refine_sets<true, SetsOrder> is the ordered search (D(C, limit): one embedding per distinct subgraph): one more by-value
// argument, the bounds of SetsOrder in every chunk's test, and the long pivot rows trimmed to them.
// k_refine_sets<false, SetsNon> and k_refine_sets<true, SetsOrder, SetsNon> are the two with the induced test: SetsNon is the last
// by-value argument, and all it adds is inside sets_lane_test.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_sets(SetsPlan P, uint32_t n_cand, const uint32_t *__restrict__ cand,
                                                       const uint32_t *__restrict__ item_off, uint32_t w_shift,
                                                       const uint32_t *__restrict__ adj_start,
                                                       const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                       const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                       uint64_t words, unsigned long long limit, SetsCounters *ctr,
                                                       uint32_t *__restrict__ matches, unsigned long long matches_cap, Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nq = P.nq, last = nq - 1;
    // a single-vertex query has one item per 64 start candidates; otherwise the scan's total
    const uint32_t n_items = nq == 1 ? (n_cand + 63u) / 64u : item_off[n_cand];
    bool rows_full = matches == nullptr;  // no row left to reserve

    for (;;) {
        if (__hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= limit) return;
        uint32_t q = 0;
        if (lane == 0) q = atomicAdd(&ctr->ticket, 1u);
        q = uni(q);
        if (q >= n_items) return;

        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;

        // the chunk of survivors at the last depth: count them, store their rows
        auto leaf = [&](uint32_t d, bool ok, uint32_t v) {
            const unsigned long long m = __ballot(ok);
            const uint32_t cnt = (uint32_t)__popcll(m);
            if (cnt == 0) return;
            if (!rows_full) {
                unsigned long long slot = 0;
                if (lane == 0) slot = atomicAdd(&ctr->cursor, (unsigned long long)cnt);
                slot = uni64(slot);
                if (slot >= matches_cap) rows_full = true;
                slot += (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
                if (ok && slot < matches_cap) {
                    uint32_t *row = matches + slot * nq;
                    for (uint32_t i = 0; i < d; i++) row[P.qv[i]] = S.image[i];
                    row[P.qv[d]] = v;
                }
            }
            pending += cnt;
            if (pending >= 1024ull) {
                unsigned long long before = 0;
                if (lane == 0) before = atomicAdd(&ctr->total, pending);
                before = uni64(before);
                stop = before + pending >= limit;
                pending = 0;
            }
        };

        if (nq == 1) {
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            leaf(0, sets_single_test(P, G, n_cand, i, v), v);
        } else if (sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) {
            uint32_t d = 1, steps = 0;
            while (d >= 1 && !stop) {
                // a subtree that finds little still hears of the limit: a look at the total every 1024 chunks
                if ((++steps & 1023u) == 0 &&
                    __hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + pending >= limit)
                    break;
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
                    if (d == last) {
                        leaf(d, ok, v);
                        continue;
                    }
                    m = __ballot(ok);
                    if (m == 0) continue;
                }
                sets_descend<kOrdered>(P, S, G, d, m, lane, ord...);
            }
        }
        if (pending && lane == 0) atomicAdd(&ctr->total, pending);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// gnnpe_refine_sets (mode 0: R), gnnpe_refine_sets_distinct (GNNPE_MATCH_DISTINCT: D, the ordered kernel unless the query has no
// symmetry) and gnnpe_refine_sets_mode (any mode; GNNPE_MATCH_INDUCED: I or ID, an induced kernel unless the query has no non-edge)
static int refine_sets_run(const char *who, uint32_t mode, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                           uint64_t limit, uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && answers, GNNPE_ERR_ARG, "%s: null argument", who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    SetsQuery Q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q);
    if (rc || Q.empty) return rc;  // limit 0 or an empty set: no answers
    const uint32_t nq = Q.nq, n_cand = Q.n_cand;
    if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);

    // context-owned, grow-only: the work buffer, the bitmap, the rows
    if (matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))) return rc;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t he = hipSuccess;
    if (device_ms) he = hipEventCreate(&ev0);
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev1);
    if (he == hipSuccess) rc = sets_stage_items(c, &Q, candidate_bitmap, c->q_work, c->q_bitmap, c->q_tmp, ev0);
    if (c->sw.debug) {
        char pairs[32] = "", non[32] = "";  // a distinct call appends pairs=K, an induced one nonedges=K
        if (mode & GNNPE_MATCH_DISTINCT) snprintf(pairs, sizeof pairs, " pairs=%u", Q.n_pairs);
        if (mode & GNNPE_MATCH_INDUCED) snprintf(non, sizeof non, " nonedges=%u", Q.n_non);
        fprintf(stderr, "[refine_sets] shift=%u forced=%d cands=%u hubs=%u cus=%d%s%s\n", Q.w_shift, (int)Q.forced, n_cand, c->n_hub,
                c->num_cus, pairs, non);
    }
    uint32_t *d_rows = matches_cap ? c->q_matches.as<uint32_t>() : nullptr;
    if (he == hipSuccess && !rc) {
        const SetsWork W(c->q_work, n_cand);
        auto launch = [&](auto... ord) {
            hipLaunchKernelGGL((k_refine_sets<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(sets_grid_blocks(c, nq, n_cand)), dim3(kBlock), 0,
                               c->stream, Q.P, n_cand, W.cand, W.item_off, Q.w_shift, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                               c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->q_bitmap.as<uint32_t>(), Q.words,
                               (unsigned long long)limit, static_cast<SetsCounters *>(W.ctr), d_rows, (unsigned long long)matches_cap,
                               ord...);
        };
        if (Q.n_non)
            Q.n_pairs ? launch(Q.O, Q.N) : launch(Q.N);
        else
            Q.n_pairs ? launch(Q.O) : launch();
        he = hipGetLastError();
        if (he == hipSuccess && device_ms) he = hipEventRecord(ev1, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(c->h_pinned, W.ctr, 16, hipMemcpyDeviceToHost, c->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(c->stream);  // the one wait of a counting call
    }
    if (he == hipSuccess && !rc) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        // every find reserved a row, so the first min(cursor, cap) rows are written
        const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
        if (n_rows) he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
    }
    if (he == hipSuccess && !rc && device_ms) {
        float ms = 0.f;
        he = hipEventElapsedTime(&ms, ev0, ev1);
        *device_ms = ms;
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipStreamSynchronize(c->stream);
    if (!rc && he != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(he));
        rc = GNNPE_ERR_HIP;
    }
    return rc;
}

extern "C" {

int gnnpe_refine_sets(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                      uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_sets_run("gnnpe_refine_sets", 0u, c, query_graph_path, candidate_bitmap, limit, answers, matches, matches_cap,
                           device_ms);
}

int gnnpe_refine_sets_distinct(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                               uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_sets_run("gnnpe_refine_sets_distinct", GNNPE_MATCH_DISTINCT, c, query_graph_path, candidate_bitmap, limit, answers,
                           matches, matches_cap, device_ms);
}

int gnnpe_refine_sets_mode(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                           uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_sets_run("gnnpe_refine_sets_mode", mode, c, query_graph_path, candidate_bitmap, limit, answers, matches, matches_cap,
                           device_ms);
}

}  // extern "C"
