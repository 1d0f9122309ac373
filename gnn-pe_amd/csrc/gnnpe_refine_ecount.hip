// gnnpe_refine_ecount.hip -- PER-EDGE MATCH COUNTS of the set-restricted refinement: E_m(C) of include/gnnpe_online.h,
// E[k][j] = the number of maps the mode counts that send query edge k = (a_k, b_k) onto the adjacency entry j = (f(a_k) -> f(b_k))
// of the loaded CSR (nqe x entries uint64, row-major).
//
// The search is k_refine_vcount's (gnnpe_refine_vcount.hip), which is k_refine_sets': the same resident grid, tickets and
// first-level items, and from gnnpe_refine_sets.hip.h the ticket take, the loop over the shared steps (sets_walk), the `pending` /
// total flush every 1024 finds, the 1024-chunk poll and the three exits, the tallies (SetsTally) and on the host the table
// handling (sets_count_call).  It writes no rows.  What is this file's own is the table, one level finer than the per-vertex one
// -- the plan edges, ient[], the leaf and flush below, hooked into the walk where k_refine_vcount's are -- and the entry point:
//
//   * every plan edge -- the pivot edge of position d >= 1 and each of its back edges -- carries a word (k << 1) | flip from the
//     host (EcountEdges, by value beside the plan).  k is the query edge's number; flip = 1 when the EARLIER position's query
//     vertex is b_k: the entry to credit then runs from the image of d to the earlier image.
//   * per wave in LDS (EcountWave, this kernel's own; SetsWave is untouched): tally[d], the finds below the current image of
//     position d (the shared SetsTally), and ient[d], the CSR index of the entry (image of pivot[d] -> image of d): cbase[d] + ctz(m),
//     taken immediately before sets_descend at depth d.  Every lane writes every word.  Reads go through uni(), but for the
//     lanes of flush(), which each read the image and the row of THEIR edge's earlier position.
//   * flush(d), d >= 1, tally t != 0: lane i takes the i-th edge of position d (lane 0 the pivot edge, then the back edges: at
//     most 31).  The pivot edge's entry is ient[d].  A back edge's entry is found by binary search in the SHORTER of the two
//     rows.  Where flip asks for the opposite entry, or the search ran in the other row, the reverse of entry j = (x -> y) is
//     adj_start[y] + revpos[j]: the context builds revpos when the rows are loaded (k_revpos), and in the state this call
//     requires (gnnpe_load_csr, no multigraph rows) every row is owned, so every entry of an undirected graph has one.  An entry
//     without a reverse (a CSR that is not symmetric) is skipped.  One 64-bit atomic add of t per lane, nothing returned.  Then
//     tally[d-1] += t and tally[d] = 0.  Position 0 has no edge: flush(0) only clears.  It runs where k_refine_vcount's does.
//   * leaf (a chunk with survivors): every surviving lane adds 1 for its pivot entry cb + lane (flipped: that entry's reverse)
//     and 1 per back edge of the last position, at the entry it finds by search; tally[last-1] += popcount.
//   * so a find costs deg_Q(last position) atomics, and every visited image with a find below it one per query edge to its
//     earlier positions.  A wave counts the adds of its flushes into the second counter word (GNNPE_DEBUG=1 prints it).
//
// limit is a GUARD exactly as in k_refine_vcount: a wave that hears of the limit leaves without flushing, the table is then
// unspecified, and *complete = 1 iff |M| < limit (the argument is written out in gnnpe_refine_vcount.hip).
// EcountEdges, EcountWave, the entry searches and the adds of the leaf and of a flush are in gnnpe_refine_ecount.hip.h, which
// k_refine_delta_ecount (gnnpe_refine_delta_counts.hip) includes as well.
// Resources of the four instantiations and the measurement: profiles/online_edge_counts.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_ecount.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_sets: plain, SetsOrder (distinct), SetsNon (induced), both.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_ecount(SetsPlan P, EcountEdges X, uint32_t n_cand, const uint32_t *__restrict__ cand,
                                                         const uint32_t *__restrict__ item_off, uint32_t w_shift,
                                                         const uint32_t *__restrict__ adj_start,
                                                         const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                         const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                         uint64_t words, const uint32_t *__restrict__ revpos, unsigned long long limit,
                                                         SetsCounters *ctr, unsigned long long *__restrict__ counts, uint64_t entries,
                                                         Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    __shared__ EcountWave s_tally[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    volatile EcountWave &E = s_tally[threadIdx.x >> 6];
    volatile SetsTally &T = E.tally;
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

        // cnt finds more: to the depth above the last and to the total
        auto found = [&](uint32_t cnt) {
            if (last >= 1) tally_set(T, last - 1, tally_get(T, last - 1) + cnt);
            sets_found(ctr, limit, lane, cnt, pending, stop);
        };
        // the chunk [cb, ..) of survivors at the last depth: every survivor adds 1 to the entry of each query edge of the last
        // position -- its own pivot entry cb + lane and one per back edge --, their number goes to the depth above
        auto leaf = [&](uint32_t, uint32_t cb, bool ok, uint32_t v) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
            if (cnt == 0) return;
            if (ok) ecount_leaf_adds(P, X, S, G, revpos, counts, entries, lane, last, cb, v, 1ull);
            found(cnt);
        };
        // the subtree of position d's current image is complete: its finds to the entries of the position's query edges, one
        // lane each, and to the depth above
        auto flush = [&](uint32_t d) {
            const unsigned long long t = tally_get(T, d);
            if (t == 0) return;
            if (d >= 1) {
                const uint32_t nb = (uint32_t)P.back_off[d + 1] - P.back_off[d];
                if (lane <= nb) ecount_flush_adds(P, X, S, E, G, revpos, counts, entries, lane, d, t);
                tally_set(T, d - 1, tally_get(T, d - 1) + t);
                flushed += nb + 1u;
            }
            tally_set(T, d, 0ull);
        };

        if (nq == 1) {  // no edge, no table: the finds alone
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            const uint32_t cnt = (uint32_t)__popcll(__ballot(sets_single_test(P, G, n_cand, i, v)));
            if (cnt) found(cnt);
        } else if (sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) {
            sets_walk<kOrdered>(
                P, S, G, ctr, limit, lane, pending, stop, last, 1, SetsNoHook{}, leaf,
                flush,  // the last sibling of this depth
                [&](uint32_t d, unsigned long long m) {
                    flush(d);  // the previous sibling, before the descent overwrites image[d]
                    E.ient[d] = uni(S.cbase[d]) + (uint32_t)__builtin_ctzll(m);  // the entry the descent takes
                },
                ord...);
            flush(0);
        }
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// the body of gnnpe_refine_sets_edge_counts; `res` (a standing query, gnnpe_standing.hip): the sets are on the device already and
// the table is the handle's `dev_table` (query edges x entries uint64)
static int refine_ecount_run(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                             uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts, double *device_ms,
                             const SetsResident *res = nullptr, void *dev_table = nullptr)
{
    const char *who = "gnnpe_refine_sets_edge_counts";
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && complete, GNNPE_ERR_ARG, "%s: null argument", who);
    *answers = 0;
    *complete = 0;
    if (dev_counts) *dev_counts = nullptr;
    if (device_ms) *device_ms = 0.0;
    SetsQuery Q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, nullptr, res);
    if (rc || limit == 0) return rc;  // limit 0: nothing is launched, and nothing is complete
    const uint32_t nq = Q.nq, n_cand = Q.n_cand;
    const uint64_t entries = c->nbr_used;  // offsets[n] of gnnpe_load_csr: adj_start[x] = offsets[x], nbrs as handed over
    // the query edges by number and the words of the plan edges: sets_prepare read a simple graph or its repeats count once here as well
    EcountEdges X = {};
    uint32_t nqe = 0, flips = 0, backflips = 0;
    if (!Q.empty) {
        nqe = ecount_edges_from_plan(Q.P, &X, &flips, &backflips);
    } else if (nq > 1) {
        // an empty set: the table's height still has to be known for the zeros
        gnnpe_host::StaticGraph q;
        std::string err;
        if (!res && q.load(query_graph_path, &err) != 0) {
            set_error("%s", err.c_str());
            return GNNPE_ERR_ARG;
        }
        nqe = (uint32_t)gnnpe_host::query_edges(res ? *res->query : q).size();
    }
    const size_t cells = (size_t)nqe * entries;
    unsigned long long *d_counts = nullptr;
    if (cells && dev_table) {
        d_counts = static_cast<unsigned long long *>(dev_table);
    } else if (cells) {
        // context-owned, grow-only, of its own: a vertex-count call in between leaves it alone
        if ((rc = c->q_ecounts.reserve(cells * 8))) return rc;
        d_counts = c->q_ecounts.as<unsigned long long>();
    }
    const uint32_t *d_bitmap = res ? res->d_bitmap : nullptr;  // (q_bitmap is reserved by the staging)
    return sets_count_call(
        who, c, &Q, candidate_bitmap, limit, d_counts, cells, answers, complete, host_counts, dev_counts, device_ms,
        [&] {
            fprintf(stderr, "[refine_ecount] shift=%u forced=%d cands=%u edges=%u flips=%u backflips=%u lastflip=%u hubs=%u cus=%d pairs=%u "
                            "nonedges=%u\n", Q.w_shift, (int)Q.forced, n_cand, nqe, flips, backflips, nq > 1 ? X.pivot[nq - 1] & 1u : 0u,
                    c->n_hub, c->num_cus, Q.n_pairs, Q.n_non);
        },
        [&](const SetsWork &W, auto... ord) {
            hipLaunchKernelGGL((k_refine_ecount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(sets_grid_blocks(c, nq, n_cand)),
                               dim3(kBlock), 0, c->stream, Q.P, X, n_cand, W.cand, W.item_off, Q.w_shift, c->adj_start.as<uint32_t>(),
                               c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                               d_bitmap ? d_bitmap : c->q_bitmap.as<uint32_t>(), Q.words, c->revpos.as<uint32_t>(),
                               (unsigned long long)limit, static_cast<SetsCounters *>(W.ctr), d_counts, entries, ord...);
        },
        [&](unsigned long long finds, unsigned long long flush_adds) {
            // every atomic on the table: deg_Q(last position) leaf adds per find, and the flushes
            const uint32_t leaf_deg = nq > 1 ? 1u + Q.P.back_off[nq] - Q.P.back_off[nq - 1] : 0u;
            fprintf(stderr, "[refine_ecount] finds=%llu flush_adds=%llu leaf_adds=%llu complete=%d\n", finds, flush_adds, finds * leaf_deg,
                    *complete);
        },
        res);
}

extern "C" int gnnpe_refine_sets_edge_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                             uint64_t limit, uint32_t mode, uint64_t *answers, int *complete, uint64_t *host_counts,
                                             void **dev_counts, double *device_ms)
{
    return refine_ecount_run(c, query_graph_path, candidate_bitmap, limit, mode, answers, complete, host_counts, dev_counts, device_ms);
}

// the same on resident sets into the caller's table, limit 2^64 - 1, for gnnpe_standing.hip (declared there)
namespace gnnpe {
int refine_ecount_resident(gnnpe_ctx *c, uint32_t mode, uint64_t *answers, const SetsResident *res, void *dev_table, double *device_ms)
{
    int complete = 0;
    return refine_ecount_run(c, nullptr, nullptr, ~0ull, mode, answers, &complete, nullptr, nullptr, device_ms, res, dev_table);
}
}  // namespace gnnpe
