// gnnpe_refine_delta_nonedges_counts.hip -- COUNT TABLES OF THE INDUCED MATCHES ON A SET OF NON-EDGES: VN_m(C, F) and EN_m(C, F) of
// include/gnnpe_online.h (ABI 19), the tables of gnnpe_refine_sets_vertex_counts / _edge_counts over the maps
// gnnpe_refine_sets_delta_nonedges counts.  With them and the tables of gnnpe_refine_delta_counts.hip an INDUCED table is maintained
// on the device across gnnpe_csr_apply_edges:
//     insertion of F:  T -= tables of Nset(G, F);  apply;  T += tables of Dset(G', F)
//     deletion  of D:  T -= tables of Dset(G, D);  apply;  T += tables of Nset(G', D)
// and nothing per match leaves the device.
//
// Nothing of the search is this file's own.  k_refine_delta_nonedges_vcount and k_refine_delta_nonedges_ecount are compositions:
//   * from k_refine_delta_nonedges (gnnpe_refine_delta_nonedges.hip): one launch per non-adjacent query pair k in the order of
//     build_match_order_from_pair against one counter block, one item per directed pair of F (nonedge_item_decode: positions 0 and 1
//     are the item's, depth 2 is entered), sets_walk with first = 2, and the charging rule as the walk's `test` hook (delta_older_ok).
//   * from k_refine_delta_vcount / k_refine_delta_ecount (gnnpe_refine_delta_counts.hip): the per-depth tallies in LDS (SetsTally,
//     EcountWave), the leaf as the `leaf` hook, flush(d) as the `up` and `down` hooks, one = sign mod 2^64, the look at the error flag
//     before a wave's first item (delta_refused), flush_adds in the second counter word.  Everything said there about one plan per
//     launch, one table for all launches, the added value, the counters, a refused call and the limit as a guard holds here with N in
//     the place of Delta; the host's side of the call is the same function (delta_counts_call, gnnpe_refine_delta_counts.hip.h).
// What the composition has to get right -- both because the items of those kernels fix one position and these fix two:
//   * POSITION 1 BELONGS TO THE ITEM, NOT TO THE WALK.  The walk starts at depth 2 and never calls `up` or `down` for depth 1, so at
//     the end of an item the kernels run flush(1) and then flush(0): flush(1) adds tally[1] to the cell (qv[1], image[1]) and carries
//     it to tally[0], flush(0) adds that to (qv[0], image[0]).  For a 3-vertex query depth 2 is the leaf, and the leaf tallies into
//     tally[1].  The tallies of the depths 0 .. last - 1 are zeroed per item.
//   * POSITION 1 HAS A PIVOT IN THE PLAN AND NO EDGE IN THE QUERY.  build_match_order_from_pair names position 0 as position 1's
//     pivot only so that the plan is well-formed.  ecount_edges_from_plan leaves that pseudo-pivot out (anchor_pair): counted as an
//     edge it would give nqe + 1 edges and shift every edge number above the anchor's.  In the edge kernel flush(1) therefore makes
//     no add -- there is no entry (image[0] -> image[1]), ient[1] is never written -- it only carries tally[1] to tally[0] and does
//     not count into flush_adds.  A position >= 2 whose pivot is position 1 is ordinary: ient[d] = cbase[d] + ctz(m) is an entry of
//     image[1]'s row.  In the ordered form nonedge_item_decode has trimmed that row, so cbase[2] need not be 64-aligned; it is still
//     the index of the chunk's first entry, as it is after sets_descend.
// Every add to a table is a 64-bit atomic whose result is not used.
// Resources of the eight instantiations and the measurement: profiles/online_delta_nonedges_counts.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_delta_counts.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_delta_nonedges: plain (the anchor is the query's only non-adjacent pair), SetsOrder,
// SetsNon, both.  nq >= 3.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_nonedges_vcount(SetsPlan P, SetsDelta D, uint32_t n_items,
                                                                        const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent,
                                                                        const unsigned long long *__restrict__ keys, uint32_t n_keys,
                                                                        const uint32_t *__restrict__ adj_start,
                                                                        const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                                        const uint32_t *__restrict__ labels,
                                                                        const uint32_t *__restrict__ bitmap, uint64_t words,
                                                                        unsigned long long limit, SetsCounters *ctr,
                                                                        unsigned long long *__restrict__ counts, uint32_t n,
                                                                        unsigned long long one, Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    __shared__ SetsTally s_tally[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    volatile SetsTally &T = s_tally[threadIdx.x >> 6];
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t last = P.nq - 1;
    if (delta_refused(ctr)) return;

    for (;;) {
        if (sets_limit_reached(ctr, limit)) return;
        const uint32_t q = sets_take_ticket(ctr, lane);
        if (q >= n_items) return;
        // item q -> the directed pair (x, y): positions 0 and 1, depth 2 entered
        if (!nonedge_item_decode<kOrdered>(P, S, G, pairs, ent, q, lane, ord...)) continue;
        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;
        uint32_t flushed = 0;  // adds of flush() in this item, for the GNNPE_DEBUG line
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);

        // k_refine_delta_vcount's leaf and flush
        auto leaf = [&](uint32_t d, uint32_t, bool ok, uint32_t v) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
            if (cnt == 0) return;
            if (ok) atomicAdd(&counts[(uint64_t)P.qv[d] * n + v], one);
            tally_set(T, d - 1, tally_get(T, d - 1) + cnt);
            sets_found(ctr, limit, lane, cnt, pending, stop);
        };
        auto flush = [&](uint32_t d, unsigned long long = 0) {
            const unsigned long long t = tally_get(T, d);
            if (t == 0) return;
            if (lane == 0) atomicAdd(&counts[(uint64_t)P.qv[d] * n + uni(S.image[d])], one * t);
            if (d >= 1) tally_set(T, d - 1, tally_get(T, d - 1) + t);
            tally_set(T, d, 0ull);
            flushed++;
        };

        sets_walk<kOrdered>(
            P, S, G, ctr, limit, lane, pending, stop, last, 2,
            [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); },  // the charging rule
            leaf, flush, flush, ord...);
        flush(1);  // position 1 is the item's: the walk never leaves it
        flush(0);
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_nonedges_ecount(SetsPlan P, SetsDelta D, EcountEdges X, uint32_t n_items,
                                                                        const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent,
                                                                        const unsigned long long *__restrict__ keys, uint32_t n_keys,
                                                                        const uint32_t *__restrict__ adj_start,
                                                                        const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                                        const uint32_t *__restrict__ labels,
                                                                        const uint32_t *__restrict__ bitmap, uint64_t words,
                                                                        const uint32_t *__restrict__ revpos, unsigned long long limit,
                                                                        SetsCounters *ctr, unsigned long long *__restrict__ counts,
                                                                        uint64_t entries, unsigned long long one, Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    __shared__ EcountWave s_tally[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    volatile EcountWave &E = s_tally[threadIdx.x >> 6];
    volatile SetsTally &T = E.tally;
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t last = P.nq - 1;
    if (delta_refused(ctr)) return;

    for (;;) {
        if (sets_limit_reached(ctr, limit)) return;
        const uint32_t q = sets_take_ticket(ctr, lane);
        if (q >= n_items) return;
        // item q -> the directed pair (x, y): positions 0 and 1, depth 2 entered
        if (!nonedge_item_decode<kOrdered>(P, S, G, pairs, ent, q, lane, ord...)) continue;
        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;
        uint32_t flushed = 0;  // adds of flush() in this item, for the GNNPE_DEBUG line
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);

        // k_refine_delta_ecount's leaf; its flush with position 1 as a position without an edge of its own
        auto leaf = [&](uint32_t, uint32_t cb, bool ok, uint32_t v) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
            if (cnt == 0) return;
            if (ok) ecount_leaf_adds(P, X, S, G, revpos, counts, entries, lane, last, cb, v, one);
            tally_set(T, last - 1, tally_get(T, last - 1) + cnt);
            sets_found(ctr, limit, lane, cnt, pending, stop);
        };
        auto flush = [&](uint32_t d) {
            const unsigned long long t = tally_get(T, d);
            if (t == 0) return;
            if (d >= 2) {
                const uint32_t nb = (uint32_t)P.back_off[d + 1] - P.back_off[d];
                if (lane <= nb) ecount_flush_adds(P, X, S, E, G, revpos, counts, entries, lane, d, one * t);
                flushed += nb + 1u;
            }
            if (d >= 1) tally_set(T, d - 1, tally_get(T, d - 1) + t);  // (d == 1: the carry alone -- no entry joins the anchor's images)
            tally_set(T, d, 0ull);
        };

        sets_walk<kOrdered>(
            P, S, G, ctr, limit, lane, pending, stop, last, 2,
            [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); },  // the charging rule
            leaf,
            flush,  // the last sibling of this depth
            [&](uint32_t d, unsigned long long m) {
                flush(d);  // the previous sibling, before the descent overwrites image[d]
                E.ient[d] = uni(S.cbase[d]) + (uint32_t)__builtin_ctzll(m);  // the entry the descent takes, in the row of image[pivot[d]]
            },
            ord...);
        flush(1);  // position 1 is the item's: the walk never leaves it
        flush(0);
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

// Both entry points after their names: delta_counts_call with F of non-edges, and the kernel a launch starts.
static int nonedges_counts_call(const char *who, const char *tag, bool edge_table, gnnpe_ctx *c, const char *query_graph_path,
                                const uint32_t *candidate_bitmap, const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts, void *dev_accum, int sign,
                                double *device_ms, const SetsResident *res = nullptr)
{
    return delta_counts_call(
        who, tag, edge_table, true, &gnnpe_ctx::q_nvcounts, &gnnpe_ctx::q_necounts, c, query_graph_path, candidate_bitmap, pairs, n_pairs,
        limit, mode, answers, complete, host_counts, dev_counts, dev_accum, sign, device_ms,
        [&](gnnpe_ctx *c, const DeltaCountsLaunch &A, const SetsQuery &K, auto... ord) {
            if (edge_table)
                hipLaunchKernelGGL((k_refine_delta_nonedges_ecount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(A.blocks),
                                   dim3(kBlock), 0, c->stream, K.P, *A.older, *A.X, A.n_items, A.F.pairs, A.F.ent, A.F.keys, A.n_keys,
                                   c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                                   A.bitmap, A.words, c->revpos.as<uint32_t>(), A.limit, A.ctr, A.table, A.entries, A.one,
                                   ord...);
            else
                hipLaunchKernelGGL((k_refine_delta_nonedges_vcount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(A.blocks),
                                   dim3(kBlock), 0, c->stream, K.P, *A.older, A.n_items, A.F.pairs, A.F.ent, A.F.keys, A.n_keys,
                                   c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                                   A.bitmap, A.words, A.limit, A.ctr, A.table, A.n, A.one, ord...);
        },
        res);
}

// the same on resident sets, adding sign * counts to the caller's table, limit 2^64 - 1, for gnnpe_standing.hip (declared there)
int refine_delta_nonedges_counts_resident(gnnpe_ctx *c, bool edge_table, const uint32_t *pairs, uint64_t n_pairs, uint32_t mode,
                                          uint64_t *answers, const SetsResident *res, void *dev_accum, int sign, double *device_ms)
{
    int complete = 0;
    return edge_table ? nonedges_counts_call("gnnpe_refine_sets_delta_nonedges_edge_counts", "refine_delta_nonedges_ecount", true, c, nullptr, nullptr,
                                             pairs, n_pairs, ~0ull, mode, answers, &complete, nullptr, nullptr, dev_accum, sign, device_ms, res)
                      : nonedges_counts_call("gnnpe_refine_sets_delta_nonedges_vertex_counts", "refine_delta_nonedges_vcount", false, c, nullptr,
                                             nullptr, pairs, n_pairs, ~0ull, mode, answers, &complete, nullptr, nullptr, dev_accum, sign, device_ms,
                                             res);
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_refine_sets_delta_nonedges_vertex_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                              const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                              uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                              void *dev_accum, int sign, double *device_ms)
{
    return nonedges_counts_call("gnnpe_refine_sets_delta_nonedges_vertex_counts", "refine_delta_nonedges_vcount", false, c, query_graph_path,
                                candidate_bitmap, pairs, n_pairs, limit, mode, answers, complete, host_counts, dev_counts, dev_accum, sign,
                                device_ms);
}

extern "C" int gnnpe_refine_sets_delta_nonedges_edge_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                            const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                            uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                            void *dev_accum, int sign, double *device_ms)
{
    return nonedges_counts_call("gnnpe_refine_sets_delta_nonedges_edge_counts", "refine_delta_nonedges_ecount", true, c, query_graph_path,
                                candidate_bitmap, pairs, n_pairs, limit, mode, answers, complete, host_counts, dev_counts, dev_accum, sign,
                                device_ms);
}
