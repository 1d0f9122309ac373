// gnnpe_refine_delta_vertices_counts.hip -- COUNT TABLES OF THE MATCHES THROUGH A SET OF DATA VERTICES: VV_m(C, S) and EV_m(C, S) of
// include/gnnpe_online.h, the tables of gnnpe_refine_sets_vertex_counts / _edge_counts over the maps gnnpe_refine_sets_delta_vertices
// counts.  With them a table is maintained on the device across a relabel: T -= tables of Sset(G, C, S), gnnpe_set_vertex_labels,
// T += tables of Sset(G', C', S); and across a removal of E(S).  Nothing per match leaves the device.
//
// Nothing of the search is this file's own.  k_refine_delta_vertices_vcount and k_refine_delta_vertices_ecount are compositions:
//   * from k_refine_delta_vertices (gnnpe_refine_delta_vertices.hip): one launch per query vertex u with a candidate in S against
//     one counter block, the first-level chunks of S n C(u) as items (sets_item_decode, the per-launch w_shift), sets_walk with
//     first = 1, the charging rule (`earlier` and vset_has) as the walk's `test` hook, and the single-vertex item.
//   * from k_refine_vcount / k_refine_ecount and their delta forms (gnnpe_refine_vcount.hip, gnnpe_refine_ecount.hip,
//     gnnpe_refine_delta_counts.hip): the per-depth tallies in LDS (SetsTally, EcountWave), the leaf as the `leaf` hook, flush(d) as
//     the `up` and `down` hooks, ient[d] taken before the descent, ecount_leaf_adds / ecount_flush_adds, one = sign mod 2^64
//     multiplied into every add, flush_adds in the second counter word; every table add is a 64-bit atomic whose result is not used.
// What the composition has to get right:
//   * POSITION 0 IS A DIFFERENT QUERY VERTEX IN EVERY LAUNCH.  The vertex-table row of depth d is P.qv[d] of that launch's plan;
//     qv[0] = u, not 0.  The cells are addressed by query vertex id, so every launch adds to the same rows.
//   * ONE EcountEdges PER LAUNCH, built by ecount_edges_from_plan from that launch's plan: an order anchored at u != 0 flips other
//     edges than the order anchored at 0 does.  Every launch's count must equal nqe; the host refuses otherwise.
//   * SEVERAL ITEMS SHARE ONE START CANDIDATE.  A row in S longer than a chunk is cut into several first-level items, so flush(0)
//     runs at the end of every item and adds atomically to the shared cell, and the tallies of depths 0 .. last - 1 are zeroed per
//     item.
//   * THE TICKET MEMSET BETWEEN LAUNCHES CLEARS THE TICKET ONLY.  The total and flush_adds run on across the launches.
//   * THE LIMIT IS A GUARD ACROSS ALL LAUNCHES, exactly as in k_refine_vcount with DeltaV in the place of |M|: the total is shared,
//     a wave that hears of the limit leaves without flushing, the table is then unspecified, and *complete = 1 iff DeltaV < limit,
//     decided on the host from the total.  The argument written out in gnnpe_refine_vcount.hip carries over unchanged: the charging
//     rule makes the launches' finds disjoint and their union the set of the definition, so `total` only ever receives finds, each
//     once, and total + pending <= DeltaV at every moment of every launch; the three exits are still the only places where a wave
//     reads the total against the limit.
//   * nq = 1.  The vertex kernel's leaf adds `one` at [0][v] and touches no tally.  The edge kernel counts the finds only: there is
//     no table, *dev_counts is NULL and *answers = DeltaV.
//   * A REFUSED CALL ADDS NOTHING: every refusal is the host's, before anything is launched.
// Resources of the eight instantiations and the measurement: profiles/online_delta_vertices_counts.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_delta_vertices.hip.h"
#include "gnnpe_refine_ecount.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_sets: plain, SetsOrder (distinct), SetsNon (induced), both.  `earlier` as in
// k_refine_delta_vertices.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_vertices_vcount(SetsPlan P, uint32_t earlier, const uint32_t *__restrict__ sbits,
                                                                        uint32_t n_cand, const uint32_t *__restrict__ cand,
                                                                        const uint32_t *__restrict__ item_off, uint32_t w_shift,
                                                                        const uint32_t *__restrict__ adj_start,
                                                                        const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                                        const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                                        uint64_t words, unsigned long long limit, SetsCounters *ctr,
                                                                        unsigned long long *__restrict__ counts, uint32_t n,
                                                                        unsigned long long one, Ord... ord)
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
        uint32_t flushed = 0;  // adds of flush() in this item, for the GNNPE_DEBUG line
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);  // per item: several items share a start candidate

        // k_refine_vcount's leaf and flush, adding `one` for 1; the row is the launch's P.qv[d]
        auto leaf = [&](uint32_t d, uint32_t, bool ok, uint32_t v) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
            if (cnt == 0) return;
            if (ok) atomicAdd(&counts[(uint64_t)P.qv[d] * n + v], one);
            if (d >= 1) tally_set(T, d - 1, tally_get(T, d - 1) + cnt);
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

        if (nq == 1) {
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            leaf(0, 0, sets_single_test(P, G, n_cand, i, v), v);
        } else if (sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) {
            sets_walk<kOrdered>(
                P, S, G, ctr, limit, lane, pending, stop, last, 1,
                // the charging rule: a query vertex numbered below this launch's must not land in S
                [&](uint32_t d, uint32_t v) { return ((earlier >> d) & 1u) == 0 || !vset_has(sbits, v); }, leaf, flush, flush, ord...);
            flush(0);  // the item's share of the start candidate's cell
        }
        sets_item_end(ctr, lane, pending);
        if (flushed && lane == 0) atomicAdd(&ctr->flush_adds, (unsigned long long)flushed);
        if (stop) return;
    }
}

template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_vertices_ecount(SetsPlan P, EcountEdges X, uint32_t earlier,
                                                                        const uint32_t *__restrict__ sbits, uint32_t n_cand,
                                                                        const uint32_t *__restrict__ cand,
                                                                        const uint32_t *__restrict__ item_off, uint32_t w_shift,
                                                                        const uint32_t *__restrict__ adj_start,
                                                                        const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                                        const uint32_t *__restrict__ labels, const uint32_t *__restrict__ bitmap,
                                                                        uint64_t words, const uint32_t *__restrict__ revpos,
                                                                        unsigned long long limit, SetsCounters *ctr,
                                                                        unsigned long long *__restrict__ counts, uint64_t entries,
                                                                        unsigned long long one, Ord... ord)
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
        uint32_t flushed = 0;  // adds of flush() in this item, for the GNNPE_DEBUG line
        for (uint32_t d = 0; d < last; d++) tally_set(T, d, 0ull);  // per item: several items share a start candidate

        // k_refine_ecount's leaf and flush, adding `one` for 1, with the launch's own words of the plan edges
        auto found = [&](uint32_t cnt) {
            if (last >= 1) tally_set(T, last - 1, tally_get(T, last - 1) + cnt);
            sets_found(ctr, limit, lane, cnt, pending, stop);
        };
        auto leaf = [&](uint32_t, uint32_t cb, bool ok, uint32_t v) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
            if (cnt == 0) return;
            if (ok) ecount_leaf_adds(P, X, S, G, revpos, counts, entries, lane, last, cb, v, one);
            found(cnt);
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

        if (nq == 1) {  // no edge, no table: the finds alone
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            const uint32_t cnt = (uint32_t)__popcll(__ballot(sets_single_test(P, G, n_cand, i, v)));
            if (cnt) found(cnt);
        } else if (sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) {
            sets_walk<kOrdered>(
                P, S, G, ctr, limit, lane, pending, stop, last, 1,
                // the charging rule: a query vertex numbered below this launch's must not land in S
                [&](uint32_t d, uint32_t v) { return ((earlier >> d) & 1u) == 0 || !vset_has(sbits, v); }, leaf,
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

// Both entry points after their names.  The staging is that of gnnpe_refine_sets_delta_vertices (gnnpe_refine_delta_vertices.hip.h);
// the table -- the context's own, zeroed on the stream before the first launch, or the caller's, untouched until a search kernel
// adds to it --, `one`, *complete and the copy back follow delta_counts_call (gnnpe_refine_delta_counts.hip.h), which is tied to the
// launches over a set of edges.
static int vertices_counts_call(const char *who, const char *tag, bool edge_table, gnnpe_ctx *c, const char *query_graph_path,
                                const uint32_t *candidate_bitmap, const uint32_t *vertices, uint64_t n_vertices, uint64_t limit,
                                uint32_t mode, uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts, void *dev_accum,
                                int sign, double *device_ms, const SetsResident *res = nullptr)
{
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && complete && (vertices || n_vertices == 0), GNNPE_ERR_ARG,
                  "%s: null argument", who);
    *answers = 0;
    *complete = 0;
    if (dev_counts) *dev_counts = nullptr;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(sign == 1 || (sign == -1 && dev_accum), GNNPE_ERR_ARG, "%s: sign must be +1, or -1 with dev_accum (got %d)", who, sign);
    GNNPE_REQUIRE(!(dev_accum && host_counts), GNNPE_ERR_ARG, "%s: host_counts must be NULL with dev_accum", who);
    VerticesPlans V;
    int rc = vertices_plans(who, c, query_graph_path, candidate_bitmap, vertices, n_vertices, limit, mode, &V, res);
    if (rc || limit == 0) return rc;  // limit 0: nothing is launched, and nothing is complete
    const uint32_t nq = V.Q.nq, n = c->n, nqe = (uint32_t)gnnpe_host::query_edges(V.q).size();
    const uint64_t entries = c->nbr_used;  // offsets[n] of gnnpe_load_csr
    const size_t cells = edge_table ? (size_t)nqe * entries : (size_t)nq * n, table_bytes = cells * 8;
    unsigned long long *table = cells ? static_cast<unsigned long long *>(dev_accum) : nullptr;  // a single-vertex query has no edge table
    if (!dev_accum && cells) {
        // context-owned, grow-only, of its own: the views of the other count calls are not disturbed
        DevBuf &own = edge_table ? c->q_evcounts : c->q_vvcounts;
        if ((rc = own.reserve(table_bytes))) return rc;
        table = own.as<unsigned long long>();
    }
    if (dev_counts) *dev_counts = table;
    if (V.nothing) {  // an empty set, an empty S, no vertex of S in any set: a zero table is the whole answer; a caller's table stays as it is
        if (!dev_accum && table_bytes) {
            GNNPE_HIP_TRY(hipMemsetAsync(table, 0, table_bytes, c->stream));
            GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
            if (host_counts) std::fill(host_counts, host_counts + cells, 0ull);
        }
        *complete = 1;
        return GNNPE_OK;
    }
    // the words of the plan edges, per launch as the plans are
    std::vector<EcountEdges> X(edge_table && nq > 1 ? V.L.size() : 0);
    uint32_t flips = 0, backflips = 0;
    for (size_t k = 0; k < X.size(); k++) {
        const uint32_t got = ecount_edges_from_plan(V.L[k].K.P, &X[k], &flips, &backflips);
        GNNPE_REQUIRE(got == nqe, GNNPE_ERR_ARG, "%s: the plan of launch %zu has %u query edges, the query %u", who, k, got, nqe);
    }
    if ((rc = vertices_reserve(c, &V, nullptr, nullptr, nullptr, nullptr, res))) return rc;
    SetsCounters *ctr = c->q_work.as<SetsCounters>();
    const unsigned long long one = sign == 1 ? 1ull : ~0ull;
    const uint64_t words = V.Q.words;
    const uint32_t *d_bitmap = res ? res->d_bitmap : c->q_bitmap.as<uint32_t>();  // (a standing query's sets are on the device already)
    SetsCall call(who, c, device_ms != nullptr);
    vertices_stage(call, c, V, candidate_bitmap, table, dev_accum ? 0 : table_bytes, nullptr, nullptr, res);
    if (c->sw.debug)
        fprintf(stderr, "[%s] vertices=%zu launches=%zu cands=%zu shift=%u hubs=%u pairs=%u nonedges=%u accum=%d sign=%d\n", tag, V.ids.size(),
                V.L.size(), V.cand_all.size(), V.L[0].w_shift, c->n_hub, V.L[0].K.n_pairs, V.L[0].K.n_non, dev_accum != nullptr, sign);
    vertices_launches(call, c, V, [&](size_t k, const VerticesLaunch &l, uint32_t blocks, uint32_t *cand, uint32_t *item_off, auto... ord) {
        if (edge_table)
            hipLaunchKernelGGL((k_refine_delta_vertices_ecount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0,
                               c->stream, l.K.P, nq > 1 ? X[k] : EcountEdges{}, l.earlier, V.sbits, l.n_cand, cand, item_off, l.w_shift,
                               c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                               d_bitmap, words, c->revpos.as<uint32_t>(), (unsigned long long)limit, ctr, table, entries, one,
                               ord...);
        else
            hipLaunchKernelGGL((k_refine_delta_vertices_vcount<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0,
                               c->stream, l.K.P, l.earlier, V.sbits, l.n_cand, cand, item_off, l.w_shift, c->adj_start.as<uint32_t>(),
                               c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), d_bitmap, words,
                               (unsigned long long)limit, ctr, table, n, one, ord...);
    });
    call.wait(ctr, 16);
    if (call.ok()) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        *complete = c->h_pinned[0] < limit ? 1 : 0;
        if (c->sw.debug)
            fprintf(stderr, "[%s] finds=%llu flush_adds=%llu complete=%d\n", tag, (unsigned long long)c->h_pinned[0],
                    (unsigned long long)c->h_pinned[1], *complete);
        if (host_counts && *complete && table_bytes) call.he = hipMemcpy(host_counts, table, table_bytes, hipMemcpyDeviceToHost);
    }
    return call.finish(device_ms);
}

// the two on resident sets, for gnnpe_standing.hip (declared there): sign * (the table over S) added to the handle's scratch table
int refine_delta_vertices_counts_resident(gnnpe_ctx *c, bool edge_table, const uint32_t *vertices, uint64_t n_vertices, uint32_t mode,
                                          uint64_t *answers, const SetsResident *res, void *dev_accum, int sign, double *device_ms)
{
    int complete = 0;
    return vertices_counts_call(edge_table ? "gnnpe_refine_sets_delta_vertices_edge_counts" : "gnnpe_refine_sets_delta_vertices_vertex_counts",
                                edge_table ? "refine_delta_vertices_ecount" : "refine_delta_vertices_vcount", edge_table, c, nullptr, nullptr, vertices,
                                n_vertices, ~0ull, mode, answers, &complete, nullptr, nullptr, dev_accum, sign, device_ms, res);
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_refine_sets_delta_vertices_vertex_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                              const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                              uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                              void *dev_accum, int sign, double *device_ms)
{
    return vertices_counts_call("gnnpe_refine_sets_delta_vertices_vertex_counts", "refine_delta_vertices_vcount", false, c, query_graph_path,
                                candidate_bitmap, vertices, n_vertices, limit, mode, answers, complete, host_counts, dev_counts, dev_accum,
                                sign, device_ms);
}

extern "C" int gnnpe_refine_sets_delta_vertices_edge_counts(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                            const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                            uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                            void *dev_accum, int sign, double *device_ms)
{
    return vertices_counts_call("gnnpe_refine_sets_delta_vertices_edge_counts", "refine_delta_vertices_ecount", true, c, query_graph_path,
                                candidate_bitmap, vertices, n_vertices, limit, mode, answers, complete, host_counts, dev_counts, dev_accum,
                                sign, device_ms);
}
