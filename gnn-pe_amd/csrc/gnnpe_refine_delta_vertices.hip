// gnnpe_refine_delta_vertices.hip -- THE MATCHES THROUGH A SET OF DATA VERTICES, each once: DeltaV_m(C, S, limit) of
// include/gnnpe_online.h, the question behind a vertex removal, a relabel (gnnpe_set_vertex_labels of include/gnnpe_hip.h) and an
// ego query.
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip): the same resident grid and tickets, the first-level chunks of the start
// candidates as items (k_sets_cand_chunks, the scan, sets_item_decode), the loop over the shared steps (sets_walk), the row leaf
// (sets_leaf_rows) and the single-vertex item; on the host the events, the wait and the error translation (SetsCall).  What is this
// file's own:
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
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

// bit v of the set's bitmap; v < n
__device__ __forceinline__ bool vset_has(const uint32_t *__restrict__ sbits, uint32_t v) { return ((sbits[v >> 5] >> (v & 31u)) & 1u) != 0; }

// one lane per id of S (each once): its bit
static __global__ void k_vset_scatter(uint32_t n_ids, const uint32_t *__restrict__ ids, uint32_t n, uint32_t *__restrict__ sbits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ids) return;
    const uint32_t v = ids[i];
    if (v < n) atomicOr(&sbits[v >> 5], 1u << (v & 31u));
}

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

// the work buffer of a call: [counters 32 B | cand of every launch | item_off of every launch (n_cand + 1 each) | chunks, the same]
struct VerticesWork {
    SetsCounters *ctr;
    uint32_t *cand, *item_off, *chunks;
    static size_t bytes(size_t n_cand_all, size_t n_launch) { return SetsWork::kCtrBytes + (3 * n_cand_all + 2 * n_launch) * 4 + 64; }
    VerticesWork(const DevBuf &b, size_t n_cand_all, size_t n_launch)
        : ctr(b.as<SetsCounters>()), cand(reinterpret_cast<uint32_t *>(b.as<char>() + SetsWork::kCtrBytes)), item_off(cand + n_cand_all),
          chunks(item_off + n_cand_all + n_launch)
    {
    }
};

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_refine_sets_delta_vertices(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    const char *who = "gnnpe_refine_sets_delta_vertices";
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && answers && (vertices || n_vertices == 0), GNNPE_ERR_ARG, "%s: null argument",
                  who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, &q);
    if (rc) return rc;
    // S as ascending ids, each once; an id the graph does not have is refused here, before anything is launched
    std::vector<uint32_t> ids;
    std::string err;
    if (gnnpe_host::delta_vertex_ids(c->n, vertices, n_vertices, &ids, &err) != 0) {
        set_error("%s: %s", who, err.c_str());
        return GNNPE_ERR_ARG;
    }
    if (Q.empty || ids.empty()) return GNNPE_OK;  // limit 0, an empty set, no S: nothing is launched
    const uint32_t nq = Q.nq, n = c->n;
    const uint64_t words = Q.words;
    const bool distinct = (mode & GNNPE_MATCH_DISTINCT) != 0, induced = (mode & GNNPE_MATCH_INDUCED) != 0;

    // the launches: per query vertex u with a start candidate the plan in the order anchored at u, the positions of the
    // lower-numbered query vertices, and S n C(u)
    struct Launch {
        SetsQuery K;
        uint32_t earlier = 0, n_cand = 0, w_shift = 6;
        size_t cand_at = 0, off_at = 0;  // where its candidates / its item offsets and chunk counts begin
    };
    std::vector<Launch> L;
    std::vector<uint32_t> cand_all;
    for (uint32_t u = 0; u < nq; u++) {
        const size_t before = cand_all.size();
        for (uint32_t s : ids)
            if ((candidate_bitmap[(size_t)u * words + (s >> 5)] >> (s & 31u)) & 1u) cand_all.push_back(s);
        if (cand_all.size() == before) continue;
        gnnpe_host::MatchOrder mo;
        if (gnnpe_host::build_match_order_from_vertex(q, u, &mo, &err) != 0) {
            set_error("%s: %s", who, err.c_str());
            return GNNPE_ERR_ARG;
        }
        L.emplace_back();
        Launch &l = L.back();
        sets_plan_from_order(q, mo, distinct, induced, c->sw.sets_trim, &l.K);
        for (uint32_t d = 1; d < nq; d++)
            if (l.K.P.qv[d] < u) l.earlier |= 1u << d;
        l.n_cand = (uint32_t)(cand_all.size() - before);
        l.cand_at = before;
        l.off_at = before + (L.size() - 1);
        // the first-level chunk width, as sets_stage_items chooses it
        const bool forced = c->sw.sets_first_shift >= 0 && c->nbr_used + n < (1ull << 32);
        l.w_shift = forced ? (uint32_t)c->sw.sets_first_shift : sets_first_level_shift(l.n_cand, c->nbr_used, n, c->num_cus, c->n_hub);
    }
    if (L.empty()) return GNNPE_OK;  // no vertex of S is in any set
    const size_t n_cand_all = cand_all.size(), n_launch = L.size(), n_ids = ids.size();
    if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);

    // context-owned, grow-only: the work areas of every launch, the bitmap, S (its bitmap, then its ids), the scan's temporary
    // storage for the longest list, the rows -- all before the first launch
    size_t tmp_bytes = 0;
    for (const Launch &l : L) {
        size_t tb = 0;
        GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(l.n_cand + 1), c->stream));
        tmp_bytes = std::max(tmp_bytes, tb);
    }
    if ((rc = c->q_work.reserve(VerticesWork::bytes(n_cand_all, n_launch))) || (rc = c->q_bitmap.reserve((size_t)nq * words * 4)) ||
        (rc = c->q_delta.reserve((words + n_ids) * 4)) || (nq > 1 && (rc = c->q_tmp.reserve(tmp_bytes))) ||
        (matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))))
        return rc;
    const VerticesWork W(c->q_work, n_cand_all, n_launch);
    uint32_t *sbits = c->q_delta.as<uint32_t>(), *d_ids = sbits + words;
    uint32_t *d_rows = matches_cap ? c->q_matches.as<uint32_t>() : nullptr;
    SetsCall call(who, c, device_ms != nullptr);
    if (call.ok()) call.he = hipMemcpyAsync(W.cand, cand_all.data(), n_cand_all * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemcpyAsync(d_ids, ids.data(), n_ids * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemcpyAsync(c->q_bitmap.p, candidate_bitmap, (size_t)nq * words * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemsetAsync(W.ctr, 0, SetsWork::kCtrBytes, c->stream);
    if (call.ok() && call.ev0) call.he = hipEventRecord(call.ev0, c->stream);
    if (call.ok()) call.he = hipMemsetAsync(sbits, 0, words * 4, c->stream);
    call.launch([&] {
        hipLaunchKernelGGL(k_vset_scatter, dim3((uint32_t)((n_ids + 255) / 256)), dim3(256), 0, c->stream, (uint32_t)n_ids, d_ids, n, sbits);
    });
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta_vertices] vertices=%zu launches=%zu cands=%zu shift=%u hubs=%u pairs=%u nonedges=%u\n", n_ids, n_launch,
                n_cand_all, L[0].w_shift, c->n_hub, L[0].K.n_pairs, L[0].K.n_non);
    for (size_t k = 0; k < n_launch; k++) {
        const Launch &l = L[k];
        uint32_t *cand = W.cand + l.cand_at, *item_off = W.item_off + l.off_at, *chunks = W.chunks + l.off_at;
        if (k && call.ok()) call.he = hipMemsetAsync(&W.ctr->ticket, 0, 4, c->stream);  // the next launch's tickets
        if (nq > 1) {
            call.launch([&] {
                hipLaunchKernelGGL(k_sets_cand_chunks, dim3((l.n_cand + 256) / 256), dim3(256), 0, c->stream, l.n_cand, cand,
                                   c->adj_deg.as<uint32_t>(), l.w_shift, chunks);
            });
            size_t tb = c->q_tmp.bytes;
            if (call.ok()) call.he = hipcub::DeviceScan::ExclusiveSum(c->q_tmp.p, tb, chunks, item_off, (int)(l.n_cand + 1), c->stream);
        }
        // a resident grid; without hub rows a start candidate has at most 64 >> w_shift chunks, and a launch needs no more waves than items
        uint64_t blocks = sets_grid_blocks(c, nq, l.n_cand);
        if (nq > 1 && c->n_hub == 0)
            blocks = std::min<uint64_t>(blocks, (((uint64_t)l.n_cand << (6 - std::min(l.w_shift, 6u))) + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
        call.launch([&] {
            sets_dispatch(l.K, [&](auto... ord) {
                hipLaunchKernelGGL((k_refine_delta_vertices<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3((uint32_t)blocks), dim3(kBlock),
                                   0, c->stream, l.K.P, l.earlier, sbits, l.n_cand, cand, item_off, l.w_shift, c->adj_start.as<uint32_t>(),
                                   c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->q_bitmap.as<uint32_t>(),
                                   words, (unsigned long long)limit, W.ctr, d_rows, (unsigned long long)matches_cap, ord...);
            });
        });
    }
    call.wait(W.ctr, 16);
    if (call.ok()) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        // every find reserved a row, so the first min(cursor, cap) rows are written
        const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
        if (n_rows) call.he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
    }
    return call.finish(device_ms);
}
