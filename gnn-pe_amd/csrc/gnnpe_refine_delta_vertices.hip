// gnnpe_refine_delta_vertices.hip -- THE MATCHES THROUGH A SET OF DATA VERTICES, each once: DeltaV_m(C, S, limit) of
// include/gnnpe_online.h, the question behind a vertex removal, a relabel (gnnpe_set_vertex_labels of include/gnnpe_hip.h) and an
// ego query.
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip): the same resident grid and tickets, the first-level chunks of the start
// candidates as items (k_sets_cand_chunks, the scan, sets_item_decode), the loop over the shared steps (sets_walk), the row leaf
// (sets_leaf_rows) and the single-vertex item; on the host the events, the wait and the error translation (SetsCall).  The host's
// staging of a call is in gnnpe_refine_delta_vertices.hip.h, shared with the table kernels of gnnpe_refine_delta_vertices_counts.hip.
// What is this search's own:
//
//   * ONE LAUNCH PER QUERY VERTEX u = 0 .. nq - 1, all on the context's stream against one counter block (total, cursor, ticket; the
//     ticket is cleared by a 4-byte memset between launches), and one wait at the end.  The plan of launch u comes from
//     build_match_order_from_vertex(q, u): position 0 is u.  Because the total is shared, a launch that starts after the limit was
//     reached returns at its first look.
//   * THE START CANDIDATES OF LAUNCH u ARE S n C(u), ascending, which the host takes from S and its bitmap.  They are cut into
//     first-level chunks exactly as gnnpe_refine_sets cuts C(order[0]): chunks of 1 << w_shift entries with the w_shift of
//     sets_first_level_shift (or of GNNPE_TESTING=sets_first_shift=K), so a hub in S is spread over the grid where the
//     edge-anchored emulation (one item per directed entry of E(S), the whole subtree behind it) puts single entries on single waves.
//     Every launch has its own candidate list, chunk counts and item offsets in the work buffer; all of them, and the scan's
//     temporary storage for the longest list, are reserved before the first launch, so no buffer moves under a queued kernel.
//   * EVERY MATCH IS CHARGED TO ONE QUERY VERTEX.  A map whose images at query vertices u1 < u2 < ... lie in S would be found in
//     each of those launches.  It is kept in launch u1 only: `earlier` holds the positions d >= 1 of the launch's order whose query
//     vertex P.qv[d] is numbered below u, and a lane that passed sets_lane_test with candidate v at such a position fails if v is
//     in S.  So launch u finds exactly the maps with f(u) in S and f(u') not in S for every u' < u; the union over u is Sset of the
//     definition, every map once, and a subtree that belongs to an earlier launch is cut at its first vertex.
//   * S ON THE DEVICE IS A BITMAP of ceil(n / 32) words in the context's q_delta buffer (grow-only), zeroed and filled once per call
//     by k_vset_scatter from the de-duplicated ids: one load per charged test.  The host has refused every id >= n, the scatter
//     checks it again, and the test is only reached by a lane that passed sets_lane_test, whose v is an entry of a validated row.
//   * a single-vertex query is one launch over S n C(0) with the single-vertex item of k_refine_sets.
// The shared device code is used as it is; the test above is this kernel's `test` hook of the walk.
// Resources of the four instantiations and the measurement: profiles/online_delta_vertices.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_delta_vertices.hip.h"

namespace gnnpe {

// One kernel, four instantiations, as k_refine_sets: plain, SetsOrder (distinct), SetsNon (induced), both.  `earlier`: bit d set =
// the query vertex of position d is numbered below this launch's (position 0 is the launch's own and never set).
template <bool kOrdered, class... Ord>
__global__ __launch_bounds__(kBlock) void k_refine_delta_vertices(SetsPlan P, uint32_t earlier, const uint32_t *__restrict__ sbits,
                                                                 uint32_t n_cand, const uint32_t *__restrict__ cand,
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
        if (sets_limit_reached(ctr, limit)) return;
        const uint32_t q = sets_take_ticket(ctr, lane);
        if (q >= n_items) return;
        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;
        // the chunk of survivors at the last depth: count them, store their rows
        auto leaf = [&](uint32_t d, uint32_t, bool ok, uint32_t v) {
            sets_leaf_rows(P, S, ctr, limit, matches, matches_cap, rows_full, lane, d, ok, v, pending, stop);
        };
        if (nq == 1) {
            const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
            leaf(0, 0, sets_single_test(P, G, n_cand, i, v), v);
        } else if (sets_item_decode(P, S, G, n_cand, cand, item_off, w_shift, q)) {
            sets_walk<kOrdered>(
                P, S, G, ctr, limit, lane, pending, stop, last, 1,
                // the charging rule: a query vertex numbered below this launch's must not land in S
                [&](uint32_t d, uint32_t v) { return ((earlier >> d) & 1u) == 0 || !vset_has(sbits, v); }, leaf, SetsNoHook{},
                SetsNoHook{}, ord...);
        }
        sets_item_end(ctr, lane, pending);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// The entry and its form on resident sets.  With `res` (gnnpe_standing.hip) neither the query file nor a host bitmap is read: the
// kernels read res->d_bitmap, the rows stay in res->d_rows and res->rows_held says how many were written.
static int refine_delta_vertices_run(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *vertices,
                                     uint64_t n_vertices, uint64_t limit, uint32_t mode, uint64_t *answers, uint32_t *matches,
                                     uint64_t matches_cap, double *device_ms, SetsResident *res = nullptr)
{
    const char *who = "gnnpe_refine_sets_delta_vertices";
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && (vertices || n_vertices == 0), GNNPE_ERR_ARG,
                  "%s: null argument", who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    if (res) res->rows_held = 0;
    // the staging is vertices_plans / _reserve / _stage / _launches of the shared header; this entry's own are the rows
    VerticesPlans V;
    int rc = vertices_plans(who, c, query_graph_path, candidate_bitmap, vertices, n_vertices, limit, mode, &V, res);
    if (rc || V.nothing) return rc;  // limit 0, an empty set, no S, no vertex of S in any set: nothing is launched
    const uint32_t nq = V.Q.nq;
    const uint64_t words = V.Q.words;
    const std::vector<VerticesLaunch> &L = V.L;
    if (res) matches_cap = res->rows_cap;
    else if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);
    if ((rc = vertices_reserve(c, &V, nullptr, nullptr, nullptr, nullptr, res)) ||
        (!res && matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))))
        return rc;
    SetsCounters *ctr = c->q_work.as<SetsCounters>();
    uint32_t *d_rows = !matches_cap ? nullptr : res ? res->d_rows : c->q_matches.as<uint32_t>();
    const uint32_t *d_bitmap = res ? res->d_bitmap : c->q_bitmap.as<uint32_t>();
    SetsCall call(who, c, device_ms != nullptr);
    vertices_stage(call, c, V, candidate_bitmap, nullptr, 0, nullptr, nullptr, res);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta_vertices] vertices=%zu launches=%zu cands=%zu shift=%u hubs=%u pairs=%u nonedges=%u\n", V.ids.size(),
                L.size(), V.cand_all.size(), L[0].w_shift, c->n_hub, L[0].K.n_pairs, L[0].K.n_non);
    vertices_launches(call, c, V, [&](size_t, const VerticesLaunch &l, uint32_t blocks, uint32_t *cand, uint32_t *item_off, auto... ord) {
        hipLaunchKernelGGL((k_refine_delta_vertices<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0, c->stream,
                           l.K.P, l.earlier, V.sbits, l.n_cand, cand, item_off, l.w_shift, c->adj_start.as<uint32_t>(),
                           c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), d_bitmap, words,
                           (unsigned long long)limit, ctr, d_rows, (unsigned long long)matches_cap, ord...);
    });
    call.wait(ctr, 16);
    if (call.ok()) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        // every find reserved a row, so the first min(cursor, cap) rows are written
        const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
        if (res) res->rows_held = n_rows;
        else if (n_rows) call.he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
    }
    return call.finish(device_ms);
}

extern "C" int gnnpe_refine_sets_delta_vertices(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_delta_vertices_run(c, query_graph_path, candidate_bitmap, vertices, n_vertices, limit, mode, answers, matches, matches_cap,
                                     device_ms);
}

// the same on resident sets, for gnnpe_standing.hip (declared there)
namespace gnnpe {
int refine_delta_vertices_resident(gnnpe_ctx *c, const uint32_t *vertices, uint64_t n_vertices, uint32_t mode, uint64_t *answers, SetsResident *res,
                                   double *device_ms)
{
    return refine_delta_vertices_run(c, nullptr, nullptr, vertices, n_vertices, ~0ull, mode, answers, nullptr, 0, device_ms, res);
}
}  // namespace gnnpe
