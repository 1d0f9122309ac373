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
// host/refine_sets.cpp is the host form.  Almost all of the above exists once, in gnnpe_refine_sets.hip.h, because other kernels
// take it too.  The steps -- the lane test of a chunk, the descent, the item decode, the single-vertex item -- and on the host the
// preparation of a query and the staging of its items are also the paged search's (gnnpe_refine_pages.hip;
// profiles/online_shared_steps.txt).  The ticket take, the find accounting and the limit, the loop that drives the steps
// (sets_walk) and the row-writing leaf, and on the host the events, the single wait and the error translation of a call (SetsCall),
// are also those of the per-vertex and per-edge counts and of the delta matches (gnnpe_refine_vcount.hip, _ecount.hip, _delta.hip;
// profiles/online_one_walk.txt).  What is this file's own: the kernel's signature and item setup with a leaf that is the shared
// row leaf and no other hook, and the three entry points of the call.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

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
            sets_walk<kOrdered>(P, S, G, ctr, limit, lane, pending, stop, last, 1, SetsNoHook{}, leaf, SetsNoHook{}, SetsNoHook{}, ord...);
        }
        sets_item_end(ctr, lane, pending);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// gnnpe_refine_sets (mode 0: R), gnnpe_refine_sets_distinct (GNNPE_MATCH_DISTINCT: D, the ordered kernel unless the query has no
// symmetry) and gnnpe_refine_sets_mode (any mode; GNNPE_MATCH_INDUCED: I or ID, an induced kernel unless the query has no non-edge)
// `res` (a standing query, gnnpe_standing.hip): the sets are on the device already and the rows stay there
static int refine_sets_run(const char *who, uint32_t mode, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                           uint64_t limit, uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms,
                           SetsResident *res = nullptr)
{
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers, GNNPE_ERR_ARG, "%s: null argument", who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    if (res) res->rows_held = 0;
    SetsQuery Q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, nullptr, res);
    if (rc || Q.empty) return rc;  // limit 0 or an empty set: no answers
    const uint32_t nq = Q.nq, n_cand = Q.n_cand;
    if (res) matches_cap = res->rows_cap;
    else if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);

    // context-owned, grow-only: the work buffer, the bitmap, the rows
    if (!res && matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))) return rc;
    SetsCall call(who, c, device_ms != nullptr);
    if (call.ok()) call.rc = sets_stage_items(c, &Q, candidate_bitmap, c->q_work, c->q_bitmap, c->q_tmp, call.ev0, res);
    if (c->sw.debug) {
        char pairs[32] = "", non[32] = "";  // a distinct call appends pairs=K, an induced one nonedges=K
        if (mode & GNNPE_MATCH_DISTINCT) snprintf(pairs, sizeof pairs, " pairs=%u", Q.n_pairs);
        if (mode & GNNPE_MATCH_INDUCED) snprintf(non, sizeof non, " nonedges=%u", Q.n_non);
        fprintf(stderr, "[refine_sets] shift=%u forced=%d cands=%u hubs=%u cus=%d%s%s\n", Q.w_shift, (int)Q.forced, n_cand, c->n_hub,
                c->num_cus, pairs, non);
    }
    uint32_t *d_rows = !matches_cap ? nullptr : res ? res->d_rows : c->q_matches.as<uint32_t>();
    const uint32_t *d_bitmap = res ? res->d_bitmap : c->q_bitmap.as<uint32_t>();
    call.launch([&] {
        const SetsWork W(c->q_work, n_cand);
        sets_dispatch(Q, [&](auto... ord) {
            hipLaunchKernelGGL((k_refine_sets<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(sets_grid_blocks(c, nq, n_cand)), dim3(kBlock), 0,
                               c->stream, Q.P, n_cand, W.cand, W.item_off, Q.w_shift, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                               c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), d_bitmap, Q.words,
                               (unsigned long long)limit, static_cast<SetsCounters *>(W.ctr), d_rows, (unsigned long long)matches_cap,
                               ord...);
        });
    });
    call.wait(c->q_work.p, 16);
    if (call.ok()) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        // every find reserved a row, so the first min(cursor, cap) rows are written
        const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
        if (res) res->rows_held = n_rows;
        else if (n_rows) call.he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
    }
    return call.finish(device_ms);
}

// gnnpe_refine_sets_mode on resident sets, for gnnpe_standing.hip (declared there)
namespace gnnpe {
int refine_sets_resident(gnnpe_ctx *c, uint32_t mode, uint64_t limit, uint64_t *answers, SetsResident *res, double *device_ms)
{
    return refine_sets_run("gnnpe_standing", mode, c, nullptr, nullptr, limit, answers, nullptr, 0, device_ms, res);
}
}  // namespace gnnpe

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
