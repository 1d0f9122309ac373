// gnnpe_refine_delta.hip -- THE MATCHES THROUGH A SET OF DATA EDGES, each once: Delta_m(C, F, limit) of include/gnnpe_online.h,
// the primitive of incremental subgraph matching (the new matches after an insertion, the vanishing ones before a deletion).
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip): the same resident grid and tickets, and from gnnpe_refine_sets.hip.h the
// ticket take (sets_limit_reached, sets_take_ticket), the loop over the shared steps (sets_walk), the leaf (sets_leaf_rows: total, rows through the
// cursor, the flush every 1024 finds) and the polling; on the host the events, the wait and the error translation (SetsCall).
// What is this file's own:
//
//   * ONE LAUNCH PER QUERY EDGE k = (a_k, b_k), all on the context's stream against one counter block (total, cursor, ticket;
//     the ticket is cleared by a 4-byte memset between launches), and one wait at the end.  The plan of launch k comes from
//     build_match_order_from_edge(q, a_k, b_k): position 0 is a_k, position 1 is b_k.  Because the total is shared, a launch that
//     starts after the limit was reached returns at its first look.
//   * AN ITEM IS A DIRECTED DELTA ENTRY x -> y: the host de-duplicates F, sorts its keys (min << 32) | max and uploads them once
//     with the 2|F| directed pairs; k_delta_entries finds the entry index j of y in x's row, one lane per pair.  A pair that is no
//     edge raises `bad` in the counter block and gets no entry; the search kernels skip it, and the host refuses the call after
//     its single wait.  The item decode tests x as position 0 (bit x of C(a_k), label, degree), makes it image[0] and holds depth 1
//     to the chunk [j, j + 1): y gets its whole test from sets_lane_test like any other entry.
//   * EVERY MATCH IS CHARGED TO ONE (query edge, delta entry) PAIR.  A match whose query edges k1 < k2 < ... land in F would be
//     found in each of those launches.  It is kept in launch k1 only: SetsDelta::older[d] holds the positions i < d that are
//     query neighbours of position d by a query edge numbered below k, and a lane that passed sets_lane_test with candidate v
//     fails if {v, image[i]} is a key of F for one of them.  So launch k finds exactly the maps f with {f(a_k), f(b_k)} in F
//     and no lower-numbered query edge in F; the item is the entry f(a_k) -> f(b_k), which exists once.  The union over k is
//     the set of the definition, every map once, and a subtree that belongs to an earlier launch is cut at its first vertex.
//   * one item per entry is all the balancing there is: a single delta edge between two hubs under a large query runs on one
//     wave.
// The shared device code is used as it is; the test above is this kernel's `test` hook of the walk, ANDed onto the lane test's
// result.
// The key search, k_delta_entries, the item decode, the charging rule and the host's staging and launches are in
// gnnpe_refine_delta.hip.h, which the table kernels of gnnpe_refine_delta_counts.hip include as well.
// Resources of the four instantiations and the measurement: profiles/online_delta.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_delta.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_sets: plain, SetsOrder (distinct), SetsNon (induced), both.  nq >= 2.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta(SetsPlan P, SetsDelta D, uint32_t n_items, const uint32_t *__restrict__ pairs,
                                                        const uint32_t *__restrict__ ent,
                                                        const unsigned long long *__restrict__ keys, uint32_t n_keys,
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
    const uint32_t last = P.nq - 1;
    bool rows_full = matches == nullptr;  // no row left to reserve

    for (;;) {
        if (sets_limit_reached(ctr, limit)) return;
        const uint32_t q = sets_take_ticket(ctr, lane);
        if (q >= n_items) return;
        // item q -> the directed entry x -> y at index j of the CSR; x is tested as position 0, depth 1 is held to [j, j + 1)
        if (!delta_item_decode(P, S, G, pairs, ent, q)) continue;  // (no edge of the graph: the call is refused)

        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;

        sets_walk<kOrdered>(
            P, S, G, ctr, limit, lane, pending, stop, last, 1,
            // the charging rule: a query edge numbered below this launch's must not land in F
            [&](uint32_t d, uint32_t v) { return delta_older_ok(D, S, keys, n_keys, d, v); },
            // the chunk of survivors at the last depth: count them, store their rows
            [&](uint32_t d, uint32_t, bool ok, uint32_t v) {
                sets_leaf_rows(P, S, ctr, limit, matches, matches_cap, rows_full, lane, d, ok, v, pending, stop);
            },
            SetsNoHook{}, SetsNoHook{}, ord...);
        sets_item_end(ctr, lane, pending);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// the body of gnnpe_refine_sets_delta; `res` (a standing query, gnnpe_standing.hip): the sets are on the device already and the rows stay there
static int refine_delta_run(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                       const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode, uint64_t *answers,
                                       uint32_t *matches, uint64_t matches_cap, double *device_ms, SetsResident *res = nullptr)
{
    const char *who = "gnnpe_refine_sets_delta";
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && (delta_edges || n_delta == 0), GNNPE_ERR_ARG, "%s: null argument",
                  who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    if (res) res->rows_held = 0;
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, &q, res);
    if (rc) return rc;
    // F as ascending keys and directed pairs, the plan of every launch; a loop or an id the graph does not have is refused here
    DeltaPlans D;
    if ((rc = delta_plans(who, c, Q, q, delta_edges, n_delta, mode, &D))) return rc;
    if (D.nothing) return GNNPE_OK;  // limit 0, an empty set, no F, a single-vertex query: nothing is launched
    const size_t n_keys = D.keys.size();
    const uint32_t nq = Q.nq, n_items = D.n_items;
    if (res) matches_cap = res->rows_cap;
    else if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);

    // context-owned, grow-only: the counters, the bitmap, F, the rows
    if ((rc = c->q_work.reserve(SetsWork::kCtrBytes)) || (!res && (rc = c->q_bitmap.reserve((size_t)nq * Q.words * 4))) ||
        (rc = c->q_delta.reserve(DeltaBuf::bytes(n_keys))) || (!res && matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))))
        return rc;
    SetsCounters *ctr = c->q_work.as<SetsCounters>();
    const DeltaBuf F(c->q_delta, n_keys);
    uint32_t *d_rows = !matches_cap ? nullptr : res ? res->d_rows : c->q_matches.as<uint32_t>();
    const uint32_t *d_bitmap = res ? res->d_bitmap : c->q_bitmap.as<uint32_t>();
    SetsCall call(who, c, device_ms != nullptr);
    const uint32_t blocks = delta_stage(call, c, Q, D, candidate_bitmap, false, nullptr, nullptr, nullptr, res);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta] edges=%zu items=%u launches=%zu blocks=%u pairs=%u nonedges=%u\n", n_keys, n_items, D.plans.size(), blocks,
                D.plans[0].n_pairs, D.plans[0].n_non);
    delta_launches(call, c, D, [&](size_t k, const SetsQuery &K, auto... ord) {
        hipLaunchKernelGGL((k_refine_delta<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0, c->stream, K.P,
                           D.older[k], n_items, F.pairs, F.ent, F.keys, (uint32_t)n_keys, c->adj_start.as<uint32_t>(),
                           c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), d_bitmap, Q.words,
                           (unsigned long long)limit, ctr, d_rows, (unsigned long long)matches_cap, ord...);
    });
    call.wait(ctr, sizeof(SetsCounters));  // all of it: `bad` is in the second half
    if (call.ok()) {
        if (reinterpret_cast<const SetsCounters *>(c->h_pinned)->bad) {
            set_error("%s: a delta edge is not an edge of the graph", who);
            call.rc = GNNPE_ERR_ARG;
        } else {
            *answers = std::min<uint64_t>(c->h_pinned[0], limit);
            // every find reserved a row, so the first min(cursor, cap) rows are written
            const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
            if (res) res->rows_held = n_rows;
            else if (n_rows) call.he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
        }
    }
    return call.finish(device_ms);
}

extern "C" int gnnpe_refine_sets_delta(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                       const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode, uint64_t *answers,
                                       uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_delta_run(c, query_graph_path, candidate_bitmap, delta_edges, n_delta, limit, mode, answers, matches, matches_cap, device_ms);
}

// the same on resident sets, for gnnpe_standing.hip (declared there)
namespace gnnpe {
int refine_delta_resident(gnnpe_ctx *c, const uint32_t *edges, uint64_t n_edges, uint32_t mode, uint64_t *answers, SetsResident *res, double *device_ms)
{
    return refine_delta_run(c, nullptr, nullptr, edges, n_edges, ~0ull, mode, answers, nullptr, 0, device_ms, res);
}
}  // namespace gnnpe
