// gnnpe_refine_delta_nonedges.hip -- THE INDUCED MATCHES THAT PUT A NON-ADJACENT QUERY PAIR ON ONE OF A SET OF DATA VERTEX PAIRS, each
// once: N_m(C, F, limit) of include/gnnpe_online.h (ABI 18), the mirror image of gnnpe_refine_delta.hip.  F holds NON-edges of the
// loaded graph: asked before F is inserted these are the induced matches the insertion destroys, asked after F was deleted the ones
// the deletion created.
//
// The search is k_refine_delta's with "query edge" replaced by "non-adjacent query pair": the same resident grid, tickets, walk
// (sets_walk), leaf (sets_leaf_rows), polling, staging (delta_plans, delta_stage, delta_launches) and charging rule
// (delta_older_ok), all used as they are.  What is this file's own:
//
//   * ONE LAUNCH PER NON-ADJACENT QUERY PAIR k = (a_k, b_k), numbered as gnnpe_host_query_nonedges numbers them, all on the context's
//     stream against one counter block, and one wait at the end.  The plan of launch k comes from build_match_order_from_pair(q,
//     a_k, b_k): position 0 is a_k, position 1 is b_k.  Position 1 has NO pivot -- b_k is reached through no adjacency row -- and the
//     query is connected, so every position >= 2 has a pivot among the earlier positions (possibly position 1).
//   * AN ITEM IS A DIRECTED PAIR (x, y) OF F, 2 |F| items.  k_delta_entries looks the pairs up with its sense inverted: a pair that
//     HAS an entry raises `bad` and is skipped by the search kernels, and the host refuses the call after its single wait.  The decode
//     (nonedge_item_decode, in gnnpe_refine_delta.hip.h: the table kernels of gnnpe_refine_delta_nonedges_counts.hip share it)
//     tests x as position 0 and y as position 1, wave-uniformly -- bit of C, label, degree, x != y, and in the ordered form the
//     bounds of position 1 -- makes them image[0] and image[1], and enters depth 2 the way sets_descend enters a depth: over the
//     pivot's row, cut to the bounds in the ordered form.  The walk starts at depth 2 and ends when depth 2 is exhausted (sets_walk's
//     `first`); for a wedge depth 2 is already the leaf.
//   * THE ANCHOR'S OWN NON-ADJACENCY IS F'S VALIDATION, not a lane test: the plan's SetsNon leaves positions (0, 1) out
//     (sets_plan_from_order sees the anchor as position 1's pivot), so a query whose only non-adjacent pair is the anchor (wedge,
//     diamond) runs the instantiation without SetsNon.  Every other non-adjacent pair is tested as in k_refine_sets.
//   * EVERY MATCH IS CHARGED TO ONE (non-adjacent pair, item) PAIR.  A map whose non-adjacent pairs k1 < k2 < ... land in F would be
//     found in each of those launches.  It is kept in launch k1 only: SetsDelta::older[d] holds the positions i < d that form with d a
//     non-adjacent query pair numbered below k, and a lane that passed sets_lane_test with candidate v fails if {v, image[i]} is a
//     key of F for one of them.  So launch k finds exactly the induced maps f with {f(a_k), f(b_k)} in F and no lower-numbered
//     non-adjacent pair in F; the item is the directed pair (f(a_k), f(b_k)), which exists once.  The union over k is the set of the
//     definition, every map once, and a subtree that belongs to an earlier launch is cut at its first vertex.  (Positions 0 and 1
//     are the launch's own pair k, never an older one.)
//   * one item per directed pair is all the balancing there is, and a query with many non-adjacent pairs has as many launches: the
//     32-vertex path 465.
// Resources of the four instantiations and the measurement: profiles/online_delta_nonedges.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_delta.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_delta: plain (the anchor is the query's only non-adjacent pair), SetsOrder, SetsNon,
// both.  nq >= 3: a connected query with a non-adjacent pair has a third vertex.
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_nonedges(SetsPlan P, SetsDelta D, uint32_t n_items,
                                                                 const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent,
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
        // item q -> the directed pair (x, y): positions 0 and 1, depth 2 entered
        if (!nonedge_item_decode<kOrdered>(P, S, G, pairs, ent, q, lane, ord...)) continue;

        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;

        sets_walk<kOrdered>(
            P, S, G, ctr, limit, lane, pending, stop, last, 2,
            // the charging rule: a non-adjacent query pair numbered below this launch's must not land in F
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

// the body of gnnpe_refine_sets_delta_nonedges; `res` (a standing query, gnnpe_standing.hip): the sets are on the device already and the rows stay there
static int refine_delta_nonedges_run(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode, uint64_t *answers,
                                                uint32_t *matches, uint64_t matches_cap, double *device_ms, SetsResident *res = nullptr)
{
    const char *who = "gnnpe_refine_sets_delta_nonedges";
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && (pairs || n_pairs == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    if (res) res->rows_held = 0;
    GNNPE_REQUIRE((mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) == 0, GNNPE_ERR_ARG, "%s: unknown mode bits 0x%x", who, mode);
    GNNPE_REQUIRE((mode & GNNPE_MATCH_INDUCED) != 0, GNNPE_ERR_ARG, "%s: the mode must contain GNNPE_MATCH_INDUCED", who);
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, &q, res);
    if (rc) return rc;
    // F as ascending keys and directed pairs, the plan of every launch; a loop or an id the graph does not have is refused here
    DeltaPlans D;
    if ((rc = delta_plans(who, c, Q, q, pairs, n_pairs, mode, &D, true))) return rc;
    if (D.nothing) return GNNPE_OK;  // limit 0, an empty set, no F, a query without a non-adjacent pair: nothing is launched
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
    const uint32_t blocks = delta_stage(call, c, Q, D, candidate_bitmap, true, nullptr, nullptr, nullptr, res);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta_nonedges] pairs=%zu items=%u launches=%zu blocks=%u ordering=%u nonedges=%u pivot2=%u\n", n_keys, n_items,
                D.plans.size(), blocks, D.plans[0].n_pairs, D.plans[0].n_non, (uint32_t)D.plans[0].P.pivot[2]);
    delta_launches(call, c, D, [&](size_t k, const SetsQuery &K, auto... ord) {
        hipLaunchKernelGGL((k_refine_delta_nonedges<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0, c->stream,
                           K.P, D.older[k], n_items, F.pairs, F.ent, F.keys, (uint32_t)n_keys, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), d_bitmap, Q.words, (unsigned long long)limit,
                           ctr, d_rows, (unsigned long long)matches_cap, ord...);
    });
    call.wait(ctr, sizeof(SetsCounters));  // all of it: `bad` is in the second half
    if (call.ok()) {
        if (reinterpret_cast<const SetsCounters *>(c->h_pinned)->bad) {
            set_error("%s: a pair is an edge of the graph", who);
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

extern "C" int gnnpe_refine_sets_delta_nonedges(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode, uint64_t *answers,
                                                uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_delta_nonedges_run(c, query_graph_path, candidate_bitmap, pairs, n_pairs, limit, mode, answers, matches, matches_cap, device_ms);
}

// the same on resident sets, for gnnpe_standing.hip (declared there)
namespace gnnpe {
int refine_delta_nonedges_resident(gnnpe_ctx *c, const uint32_t *edges, uint64_t n_edges, uint32_t mode, uint64_t *answers, SetsResident *res, double *device_ms)
{
    return refine_delta_nonedges_run(c, nullptr, nullptr, edges, n_edges, ~0ull, mode, answers, nullptr, 0, device_ms, res);
}
}  // namespace gnnpe
