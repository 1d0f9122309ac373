// gnnpe_refine_vcount.hip -- PER-VERTEX MATCH COUNTS of the set-restricted refinement: V_m(C) of include/gnnpe_online.h,
// V[u][v] = the number of maps the mode counts that send query vertex u to data vertex v (nq x n uint64, row-major).
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip): the same resident grid, tickets and first-level items, and from
// gnnpe_refine_sets.hip.h the ticket take (sets_limit_reached, sets_take_ticket), the loop over the shared steps (sets_walk), the `pending` / total flush
// every 1024 finds (sets_found) and the 1024-chunk poll.  It writes no rows.  What is this file's own is the table -- the leaf and
// flush below, hooked into the walk at the last depth, before d-- and before the descent -- and the entry point:
//
//   * adding 1 to the nq cells of every find would cost nq atomics per match.  Instead the wave TALLIES PER DEPTH AND FLUSHES ON
//     THE WAY UP: tally[d], d = 0 .. nq-2, is the number of finds below the CURRENT image of position d -- wave-uniform, 64-bit,
//     in an LDS array beside SetsWave (SetsTally of the shared header: two words per depth; SetsWave is untouched).  The conventions of the
//     shared state hold: every lane writes every word, every read goes through uni().
//   * leaf (depth nq-1, a chunk with survivor ballot m): every surviving lane does one 64-bit atomic add of 1 on
//     counts[qv[last] * n + its v] -- the addresses of a chunk are different entries of one row -- and tally[last-1] += popcount(m).
//   * flush(d): if tally[d] != 0, lane 0 adds it to counts[qv[d] * n + image[d]], then tally[d-1] += tally[d] (d >= 1) and
//     tally[d] = 0.  It runs immediately before sets_descend at depth d (the previous sibling's subtree is complete, and the
//     descent overwrites image[d]), before d-- out of depth d (the pivot row is exhausted), and for d = 0 at the end of an item.
//     Several items share one start candidate, so cell [qv[0]][v0] is added to by several waves: every add is an atomic.
//   * so a find costs one atomic for the last position, and every visited image with at least one find below it costs one more.
//   * plain 64-bit integer atomics, no returned value but the ticket's and the total's, which the loop already takes.
//   * a wave counts its flushes and adds their number to the second counter word at the end of an item; with GNNPE_DEBUG=1 the
//     host prints it beside the finds, which is how scripts/online_vertex_counts_measure.py knows the atomics per find.
//
// limit is a GUARD, not a cut: a wave that hears of the limit (the three exits marked EXIT 1, 2 and 3 in gnnpe_refine_sets.hip.h:
// sets_limit_reached, sets_found, sets_walk -- the only places where a wave reads the total against the limit, and this kernel's hooks
// add none) leaves without flushing its tallies, and the table is unspecified.  *complete = 1 iff |M| < limit, computed on the host from the total.  Why that is
// enough: `total` only ever receives finds, each once, so at every moment total + (any wave's pending) <= |M|.  Exit 1 needs
// total >= limit, exit 2 needs before + pending >= limit, exit 3 needs total + pending >= limit: with |M| < limit none of the
// three can be taken, every wave walks every item to its end, every tally is flushed, and the final total is |M| < limit.
// Conversely a final total >= limit is |M| >= limit (the total never exceeds |M|), and the host says *complete = 0.
// The host side after sets_prepare is sets_count_call of the shared header, with the edge counts: the table's zeroing, the empty
// set's zero answer, `complete`, the copy back.
// Resources of the four instantiations and the measurement: profiles/online_vertex_counts.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_sets: plain, SetsOrder (distinct), SetsNon (induced), both.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_vcount(SetsPlan P, uint32_t n_cand, const uint32_t *__restrict__ cand,
                                                         const uint32_t *__restrict__ item_off, uint32_t w_shift,
                                                         const uint32_t *__restrict__ adj_start,
                                                         const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                         const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                         uint64_t words, unsigned long long limit, SetsCounters *ctr,
                                                         unsigned long long *__restrict__ counts, uint32_t n, Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    __shared__ SetsTally s_tally[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    volatile SetsTally &T = s_tally[threadIdx.x >> 6];
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nq = P.nq, last = nq - 1;
    // a single-vertex query has one item per 64 start candidates; otherwise the scan's total
    const uint32_t n_items = nq == 1 ? (n_cand + 63u) / 64u : item_off[n_cand];

    for (;;) {
        if (sets_limit_reached(ctr, limit)) return;
        const uint32_t q = sets_take_ticket(ctr, lane);
        if (q >= n_items) return;
        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;
        uint32_t flushed = 0;  // adds of flush() in this item: one more add per item for the GNNPE_DEBUG line, nothing reads it back
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);

        // the chunk of survivors at the last depth: one add per survivor on its own cell, their number to the depth above
        auto leaf = [&](uint32_t d, uint32_t, bool ok, uint32_t v) {
            const unsigned long long m = __ballot(ok);
            const uint32_t cnt = (uint32_t)__popcll(m);
            if (cnt == 0) return;
            if (ok) atomicAdd(&counts[(uint64_t)P.qv[d] * n + v], 1ull);
            if (d >= 1) tally_set(T, d - 1, tally_get(T, d - 1) + cnt);
            sets_found(ctr, limit, lane, cnt, pending, stop);
        };
        // the subtree of position d's current image is complete: its finds to the image's cell and to the depth above
        auto flush = [&](uint32_t d, unsigned long long = 0) {
            const unsigned long long t = tally_get(T, d);
            if (t == 0) return;
            if (lane == 0) atomicAdd(&counts[(uint64_t)P.qv[d] * n + uni(S.image[d])], t);
            if (d >= 1) tally_set(T, d - 1, tally_get(T, d - 1) + t);
            tally_set(T, d, 0ull);
            flushed++;
        };

        if (nq == 1) {
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            leaf(0, 0, sets_single_test(P, G, n_cand, i, v), v);
        } else if (sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) {
            // flush: the last sibling of a depth when its row is exhausted; the previous sibling before the descent overwrites image[d]
            sets_walk<kOrdered>(P, S, G, ctr, limit, lane, pending, stop, last, 1, SetsNoHook{}, leaf, flush, flush, ord...);
            flush(0);
        }
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// the body of gnnpe_refine_sets_vertex_counts; `res` (a standing query, gnnpe_standing.hip): the sets are on the device already and
// the table is the handle's `dev_table` (nq x n uint64)
static int refine_vcount_run(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                             uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts, double *device_ms,
                             const SetsResident *res = nullptr, void *dev_table = nullptr)
{
    const char *who = "gnnpe_refine_sets_vertex_counts";
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && complete, GNNPE_ERR_ARG, "%s: null argument", who);
    *answers = 0;
    *complete = 0;
    if (dev_counts) *dev_counts = nullptr;
    if (device_ms) *device_ms = 0.0;
    SetsQuery Q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, nullptr, res);
    if (rc || limit == 0) return rc;  // limit 0: nothing is launched, and nothing is complete
    const uint32_t nq = Q.nq, n_cand = Q.n_cand, n = c->n;
    // context-owned, grow-only: the table beside the work buffer and the bitmap
    if (!dev_table && (rc = c->q_vcounts.reserve((size_t)nq * n * 8))) return rc;
    unsigned long long *d_counts = dev_table ? static_cast<unsigned long long *>(dev_table) : c->q_vcounts.as<unsigned long long>();
    const uint32_t *d_bitmap = res ? res->d_bitmap : nullptr;  // (q_bitmap is reserved by the staging)
    return sets_count_call(
        who, c, &Q, candidate_bitmap, limit, d_counts, (size_t)nq * n, answers, complete, host_counts, dev_counts, device_ms,
        [&] {
            fprintf(stderr, "[refine_vcount] shift=%u forced=%d cands=%u hubs=%u cus=%d pairs=%u nonedges=%u\n", Q.w_shift, (int)Q.forced,
                    n_cand, c->n_hub, c->num_cus, Q.n_pairs, Q.n_non);
        },
        [&](const SetsWork &W, auto... ord) {
            hipLaunchKernelGGL((k_refine_vcount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(sets_grid_blocks(c, nq, n_cand)),
                               dim3(kBlock), 0, c->stream, Q.P, n_cand, W.cand, W.item_off, Q.w_shift, c->adj_start.as<uint32_t>(),
                               c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                               d_bitmap ? d_bitmap : c->q_bitmap.as<uint32_t>(), Q.words, (unsigned long long)limit,
                               static_cast<SetsCounters *>(W.ctr), d_counts, n, ord...);
        },
        [&](unsigned long long finds, unsigned long long flush_adds) {  // every atomic on the table: one leaf add per find, and the flushes
            fprintf(stderr, "[refine_vcount] finds=%llu flush_adds=%llu complete=%d\n", finds, flush_adds, *complete);
        },
        res);
}

extern "C" int gnnpe_refine_sets_vertex_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                               uint64_t limit, uint32_t mode, uint64_t *answers, int *complete, uint64_t *host_counts,
                                               void **dev_counts, double *device_ms)
{
    return refine_vcount_run(c, query_graph_path, candidate_bitmap, limit, mode, answers, complete, host_counts, dev_counts, device_ms);
}

// the same on resident sets into the caller's table, limit 2^64 - 1, for gnnpe_standing.hip (declared there)
namespace gnnpe {
int refine_vcount_resident(gnnpe_ctx *c, uint32_t mode, uint64_t *answers, const SetsResident *res, void *dev_table, double *device_ms)
{
    int complete = 0;
    return refine_vcount_run(c, nullptr, nullptr, ~0ull, mode, answers, &complete, nullptr, nullptr, device_ms, res, dev_table);
}
}  // namespace gnnpe
