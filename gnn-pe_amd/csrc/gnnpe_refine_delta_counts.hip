// gnnpe_refine_delta_counts.hip -- COUNT TABLES OF THE MATCHES THROUGH A SET OF DATA EDGES: VDelta_m(C, F) and EDelta_m(C, F) of
// include/gnnpe_online.h, the tables of gnnpe_refine_sets_vertex_counts / _edge_counts over the maps gnnpe_refine_sets_delta counts.
// With them a table is maintained on the device across gnnpe_csr_apply_edges: T -= tables of Delta(G, D), apply, T += tables of
// Delta(G', I); nothing per match leaves the device.
//
// Nothing of the search is this file's own.  k_refine_delta_vcount and k_refine_delta_ecount are compositions:
//   * from k_refine_delta (gnnpe_refine_delta.hip.h): one launch per query edge k in the order of build_match_order_from_edge against
//     one counter block, one item per directed entry of F with depth 1 held to [j, j + 1) (delta_item_decode), and the charging rule
//     as the walk's `test` hook (delta_older_ok): a match is found in the launch of its lowest-numbered query edge in F only.
//   * from k_refine_vcount / k_refine_ecount (gnnpe_refine_sets.hip.h, gnnpe_refine_ecount.hip.h): the per-depth tallies in LDS
//     (SetsTally, EcountWave), the leaf as the `leaf` hook, flush(d) as the `up` and `down` hooks, flush(0) at the end of an item.
// What the composition has to get right:
//   * ONE PLAN PER LAUNCH.  P.qv differs from launch to launch, and the cells are addressed by query vertex id (P.qv[d]), so every
//     launch adds to the same rows.  For the edge table the words (k << 1) | flip of the plan edges (EcountEdges) are built per launch
//     from that launch's plan, as the `older` masks are.
//   * ONE TABLE FOR ALL LAUNCHES OF A CALL, and many items share cells: every add is an atomic, 64-bit, nothing returned.
//   * THE ITEM'S OWN ENTRY.  Depth 1 runs on the chunk [j, j + 1) with cbase[1] = j - 64: the walk steps to cbase[1] = j, the only
//     survivor is lane 0, and `down` takes ient[1] = cbase[1] + ctz(1) = j.  With nq = 2 the leaf runs at depth 1 on that chunk, and
//     its pivot entry cb + lane is j.
//   * THE ADDED VALUE is `one` at the leaf and one * tally in the flushes, one = sign mod 2^64 (1, or 2^64 - 1 for sign -1): the adds
//     wrap, and a cell ends at old + sign * c mod 2^64.
//   * THE COUNTERS.  The kernels write no rows: the second counter word carries flush_adds as in the count kernels (GNNPE_DEBUG=1
//     prints it), and goes on across the launches with the total.
//   * A REFUSED CALL ADDS NOTHING.  k_delta_entries has finished, in stream order, before the first search launch starts, so `bad` is
//     final when a wave of these kernels reads it, before its first item; a wave that finds it set leaves.  A caller's accumulated
//     table is then byte for byte what it was.
// limit is a GUARD exactly as in k_refine_vcount, with Delta in the place of |M|, shared across the launches through `total`: a wave
// that hears of it leaves without flushing, the table is then unspecified, and *complete = 1 iff Delta < limit, decided on the host
// from the total.  The argument written out in gnnpe_refine_vcount.hip carries over unchanged: the launches find disjoint sets of
// maps whose union is the set of the definition, so `total` only ever receives finds, each once, and total + pending <= Delta at
// every moment of every launch; the three exits are still the only places where a wave reads the total against the limit.
// Resources of the eight instantiations and the measurement: profiles/online_delta_counts.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_delta_counts.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_sets: plain, SetsOrder (distinct), SetsNon (induced), both.  nq >= 2.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_vcount(SetsPlan P, SetsDelta D, uint32_t n_items, const uint32_t *__restrict__ pairs,
                                                               const uint32_t *__restrict__ ent,
                                                               const unsigned long long *__restrict__ keys, uint32_t n_keys,
                                                               const uint32_t *__restrict__ adj_start,
                                                               const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                               const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                               uint64_t words, unsigned long long limit, SetsCounters *ctr,
                                                               unsigned long long *__restrict__ counts, uint32_t n, unsigned long long one,
                                                               Ord... ord)
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
        if (!delta_item_decode(P, S, G, pairs, ent, q)) continue;
        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;
        uint32_t flushed = 0;  // adds of flush() in this item, for the GNNPE_DEBUG line
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);

        // k_refine_vcount's leaf and flush, adding `one` for 1
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
            P, S, G, ctr, limit, lane, pending, stop, last, 1,
            [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); },  // the charging rule
            leaf, flush, flush, ord...);
        flush(0);
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_ecount(SetsPlan P, SetsDelta D, EcountEdges X, uint32_t n_items,
                                                               const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent,
                                                               const unsigned long long *__restrict__ keys, uint32_t n_keys,
                                                               const uint32_t *__restrict__ adj_start,
                                                               const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                               const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                               uint64_t words, const uint32_t *__restrict__ revpos, unsigned long long limit,
                                                               SetsCounters *ctr, unsigned long long *__restrict__ counts, uint64_t entries,
                                                               unsigned long long one, Ord... ord)
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
        if (!delta_item_decode(P, S, G, pairs, ent, q)) continue;
        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;
        uint32_t flushed = 0;  // adds of flush() in this item, for the GNNPE_DEBUG line
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);

        // k_refine_ecount's leaf and flush, adding `one` for 1
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
            if (d >= 1) {
                const uint32_t nb = (uint32_t)P.back_off[d + 1] - P.back_off[d];
                if (lane <= nb) ecount_flush_adds(P, X, S, E, G, revpos, counts, entries, lane, d, one * t);
                tally_set(T, d - 1, tally_get(T, d - 1) + t);
                flushed += nb + 1u;
            }
            tally_set(T, d, 0ull);
        };

        sets_walk<kOrdered>(
            P, S, G, ctr, limit, lane, pending, stop, last, 1,
            [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); },  // the charging rule
            leaf,
            flush,  // the last sibling of this depth
            [&](uint32_t d, unsigned long long m) {
                flush(d);  // the previous sibling, before the descent overwrites image[d]
                E.ient[d] = uni(S.cbase[d]) + (uint32_t)__builtin_ctzll(m);  // the entry the descent takes; at depth 1 the item's own j
            },
            ord...);
        flush(0);
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

// Both entry points after their names: the host's side is delta_counts_call (gnnpe_refine_delta_counts.hip.h), shared with the tables
// over a set of non-edges; this file's part of it is the kernel a launch starts.
static int delta_edges_counts_call(const char *who, const char *tag, bool edge_table, gnnpe_ctx *c, const char *query_graph_path,
                                   const uint32_t *candidate_bitmap, const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit,
                                   uint32_t mode, uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts, void *dev_accum,
                                   int sign, double *device_ms, const SetsResident *res = nullptr)
{
    return delta_counts_call(
        who, tag, edge_table, false, &gnnpe_ctx::q_dvcounts, &gnnpe_ctx::q_decounts, c, query_graph_path, candidate_bitmap, delta_edges,
        n_delta, limit, mode, answers, complete, host_counts, dev_counts, dev_accum, sign, device_ms,
        [&](gnnpe_ctx *c, const DeltaCountsLaunch &A, const SetsQuery &K, auto... ord) {
            if (edge_table)
                hipLaunchKernelGGL((k_refine_delta_ecount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(A.blocks), dim3(kBlock), 0,
                                   c->stream, K.P, *A.older, *A.X, A.n_items, A.F.pairs, A.F.ent, A.F.keys, A.n_keys,
                                   c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                                   A.bitmap, A.words, c->revpos.as<uint32_t>(), A.limit, A.ctr, A.table, A.entries, A.one,
                                   ord...);
            else
                hipLaunchKernelGGL((k_refine_delta_vcount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(A.blocks), dim3(kBlock), 0,
                                   c->stream, K.P, *A.older, A.n_items, A.F.pairs, A.F.ent, A.F.keys, A.n_keys, c->adj_start.as<uint32_t>(),
                                   c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), A.bitmap,
                                   A.words, A.limit, A.ctr, A.table, A.n, A.one, ord...);
        },
        res);
}

// the same on resident sets, adding sign * counts to the caller's table, limit 2^64 - 1, for gnnpe_standing.hip (declared there)
int refine_delta_counts_resident(gnnpe_ctx *c, bool edge_table, const uint32_t *edges, uint64_t n_edges, uint32_t mode, uint64_t *answers,
                                 const SetsResident *res, void *dev_accum, int sign, double *device_ms)
{
    int complete = 0;
    return edge_table ? delta_edges_counts_call("gnnpe_refine_sets_delta_edge_counts", "refine_delta_ecount", true, c, nullptr, nullptr, edges, n_edges,
                                                ~0ull, mode, answers, &complete, nullptr, nullptr, dev_accum, sign, device_ms, res)
                      : delta_edges_counts_call("gnnpe_refine_sets_delta_vertex_counts", "refine_delta_vcount", false, c, nullptr, nullptr, edges,
                                                n_edges, ~0ull, mode, answers, &complete, nullptr, nullptr, dev_accum, sign, device_ms, res);
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_refine_sets_delta_vertex_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                     const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                                     uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                     void *dev_accum, int sign, double *device_ms)
{
    return delta_edges_counts_call("gnnpe_refine_sets_delta_vertex_counts", "refine_delta_vcount", false, c, query_graph_path,
                                   candidate_bitmap, delta_edges, n_delta, limit, mode, answers, complete, host_counts, dev_counts, dev_accum,
                                   sign, device_ms);
}

extern "C" int gnnpe_refine_sets_delta_edge_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                   const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                                   uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                   void *dev_accum, int sign, double *device_ms)
{
    return delta_edges_counts_call("gnnpe_refine_sets_delta_edge_counts", "refine_delta_ecount", true, c, query_graph_path,
                                   candidate_bitmap, delta_edges, n_delta, limit, mode, answers, complete, host_counts, dev_counts, dev_accum,
                                   sign, device_ms);
}
