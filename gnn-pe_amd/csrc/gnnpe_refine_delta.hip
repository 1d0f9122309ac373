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
// Resources of the four instantiations and the measurement: profiles/online_delta.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

struct SetsDelta {  // by position: bit i < d of older[d] = positions i and d are joined by a query edge numbered below the launch's
    uint32_t older[kSetsMaxQ];
};

constexpr uint32_t kDeltaNoEntry = 0xFFFFFFFFu;

// is `key` among the ascending keys[0 .. n)?
__device__ __forceinline__ bool delta_has(const unsigned long long *__restrict__ keys, uint32_t n, unsigned long long key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const unsigned long long x = keys[mid];
        if (x == key) return true;
        if (x < key) lo = mid + 1; else hi = mid;
    }
    return false;
}

// one lane per directed pair (x, y), both below n: the index of y in x's row, or kDeltaNoEntry and the error flag
static __global__ void k_delta_entries(uint32_t n_pairs, const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ adj_start,
                                       const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                       uint32_t *__restrict__ ent, SetsCounters *ctr)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const uint32_t x = pairs[2 * i], y = pairs[2 * i + 1];
    const uint32_t st = adj_start[x];
    uint32_t lo = 0, hi = adj_deg[x], j = kDeltaNoEntry;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t w = nbrs[st + mid];
        if (w == y) {
            j = st + mid;
            break;
        }
        if (w < y) lo = mid + 1; else hi = mid;
    }
    ent[i] = j;
    if (j == kDeltaNoEntry) atomicOr(&ctr->bad, 1u);
}

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
        const uint32_t j = uni(ent[q]);
        if (j == kDeltaNoEntry) continue;  // no edge of the graph: the call is refused
        const uint32_t x = uni(pairs[2 * q]);
        const uint32_t s0 = uni(adj_start[x]), d0 = uni(adj_deg[x]);
        const uint32_t word = uni(bitmap[(uint64_t)P.qv[0] * words + (x >> 5)]);
        if (((word >> (x & 31u)) & 1u) == 0 || uni(labels[x]) != P.label[0] || d0 < P.degree[0]) continue;
        S.image[0] = x;
        S.istart[0] = s0;
        S.ideg[0] = d0;
        S.cbase[1] = j - 64u;
        S.end[1] = j + 1u;
        S.mask_lo[1] = 0;
        S.mask_hi[1] = 0;

        unsigned long long pending = 0;  // finds not yet added to the total
        bool stop = false;

        sets_walk<kOrdered>(
            P, S, G, ctr, limit, lane, pending, stop, last,
            // the charging rule: a query edge numbered below this launch's must not land in F
            [&](uint32_t d, uint32_t v) {
                bool ok = true;
                for (uint32_t o = uni(D.older[d]); o && ok; o &= o - 1u) {
                    const uint32_t w = uni(S.image[__builtin_ctz(o)]);
                    ok = !delta_has(keys, n_keys, ((unsigned long long)min(v, w) << 32) | max(v, w));
                }
                return ok;
            },
            // the chunk of survivors at the last depth: count them, store their rows
            [&](uint32_t d, uint32_t, bool ok, uint32_t v) {
                sets_leaf_rows(P, S, ctr, limit, matches, matches_cap, rows_full, lane, d, ok, v, pending, stop);
            },
            SetsNoHook{}, SetsNoHook{}, ord...);
        sets_item_end(ctr, lane, pending);
        if (stop) return;
    }
}

// the buffer of F on the device: [keys u64 x n_keys | pairs u32 x 2 x 2 n_keys | ent u32 x 2 n_keys]
struct DeltaBuf {
    unsigned long long *keys;
    uint32_t *pairs, *ent;
    static size_t bytes(size_t n_keys) { return n_keys * (8 + 16 + 8); }
    DeltaBuf(const DevBuf &b, size_t n_keys)
        : keys(b.as<unsigned long long>()), pairs(reinterpret_cast<uint32_t *>(keys + n_keys)), ent(pairs + 4 * n_keys)
    {
    }
};

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_refine_sets_delta(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                       const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode, uint64_t *answers,
                                       uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    const char *who = "gnnpe_refine_sets_delta";
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && answers && (delta_edges || n_delta == 0), GNNPE_ERR_ARG, "%s: null argument",
                  who);
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, &q);
    if (rc) return rc;
    // F as ascending keys, each edge once; a loop or an id the graph does not have is refused here, before anything is launched
    std::vector<uint64_t> keys;
    std::string err;
    if (gnnpe_host::delta_edge_keys(c->n, delta_edges, n_delta, &keys, &err) != 0) {
        set_error("%s: %s", who, err.c_str());
        return GNNPE_ERR_ARG;
    }
    const std::vector<std::pair<uint32_t, uint32_t>> qe = gnnpe_host::query_edges(q);
    if (Q.empty || keys.empty() || qe.empty()) return GNNPE_OK;  // limit 0, an empty set, no F, a single-vertex query: nothing is launched
    const size_t n_keys = keys.size();
    GNNPE_REQUIRE(2 * (uint64_t)n_keys < (1ull << 32), GNNPE_ERR_ARG, "%s: %zu different delta edges, the items are 32-bit", who, n_keys);
    const uint32_t nq = Q.nq, n_items = (uint32_t)(2 * n_keys);
    std::vector<uint32_t> pairs(4 * n_keys);
    for (size_t i = 0; i < n_keys; i++) {
        const uint32_t lo = (uint32_t)(keys[i] >> 32), hi = (uint32_t)keys[i];
        pairs[4 * i] = pairs[4 * i + 3] = lo;
        pairs[4 * i + 1] = pairs[4 * i + 2] = hi;
    }
    // the plan of every launch: the order anchored at the query edge, and the earlier neighbours by a lower-numbered edge
    const bool distinct = (mode & GNNPE_MATCH_DISTINCT) != 0, induced = (mode & GNNPE_MATCH_INDUCED) != 0;
    std::vector<SetsQuery> plans(qe.size());
    std::vector<SetsDelta> older(qe.size(), SetsDelta{});
    for (size_t k = 0; k < qe.size(); k++) {
        gnnpe_host::MatchOrder mo;
        if (gnnpe_host::build_match_order_from_edge(q, qe[k].first, qe[k].second, &mo, &err) != 0) {
            set_error("%s: %s", who, err.c_str());
            return GNNPE_ERR_ARG;
        }
        const std::vector<uint32_t> pos_of = sets_plan_from_order(q, mo, distinct, induced, c->sw.sets_trim, &plans[k]);
        for (size_t e = 0; e < k; e++) {
            const uint32_t pa = pos_of[qe[e].first], pb = pos_of[qe[e].second];
            older[k].older[std::max(pa, pb)] |= 1u << std::min(pa, pb);
        }
    }
    if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);

    // context-owned, grow-only: the counters, the bitmap, F, the rows
    const size_t bm_bytes = (size_t)nq * Q.words * 4;
    if ((rc = c->q_work.reserve(SetsWork::kCtrBytes)) || (rc = c->q_bitmap.reserve(bm_bytes)) ||
        (rc = c->q_delta.reserve(DeltaBuf::bytes(n_keys))) || (matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))))
        return rc;
    SetsCounters *ctr = c->q_work.as<SetsCounters>();
    const DeltaBuf F(c->q_delta, n_keys);
    uint32_t *d_rows = matches_cap ? c->q_matches.as<uint32_t>() : nullptr;
    SetsCall call(who, c, device_ms != nullptr);
    if (call.ok()) call.he = hipMemcpyAsync(F.keys, keys.data(), n_keys * 8, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemcpyAsync(F.pairs, pairs.data(), n_keys * 16, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemcpyAsync(c->q_bitmap.p, candidate_bitmap, bm_bytes, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemsetAsync(ctr, 0, SetsWork::kCtrBytes, c->stream);
    if (call.ok() && call.ev0) call.he = hipEventRecord(call.ev0, c->stream);
    // a resident grid, or as many waves as there are items
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(sets_grid_blocks(c, nq, n_items), (n_items + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta] edges=%zu items=%u launches=%zu blocks=%u pairs=%u nonedges=%u\n", n_keys, n_items, qe.size(), blocks,
                plans[0].n_pairs, plans[0].n_non);
    call.launch([&] {
        hipLaunchKernelGGL(k_delta_entries, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, n_items, F.pairs, c->adj_start.as<uint32_t>(),
                           c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), F.ent, ctr);
    });
    for (size_t k = 0; k < qe.size(); k++) {
        const SetsQuery &K = plans[k];
        if (k && call.ok()) call.he = hipMemsetAsync(&ctr->ticket, 0, 4, c->stream);  // the next launch's tickets; total and cursor go on
        // (the pairs and the non-edges are the query's, whatever the order: every launch runs the same instantiation)
        call.launch([&] {
            sets_dispatch(K, [&](auto... ord) {
                hipLaunchKernelGGL((k_refine_delta<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0, c->stream,
                                   K.P, older[k], n_items, F.pairs, F.ent, F.keys, (uint32_t)n_keys, c->adj_start.as<uint32_t>(),
                                   c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->q_bitmap.as<uint32_t>(),
                                   Q.words, (unsigned long long)limit, ctr, d_rows, (unsigned long long)matches_cap, ord...);
            });
        });
    }
    call.wait(ctr, sizeof(SetsCounters));  // all of it: `bad` is in the second half
    if (call.ok()) {
        if (reinterpret_cast<const SetsCounters *>(c->h_pinned)->bad) {
            set_error("%s: a delta edge is not an edge of the graph", who);
            call.rc = GNNPE_ERR_ARG;
        } else {
            *answers = std::min<uint64_t>(c->h_pinned[0], limit);
            // every find reserved a row, so the first min(cursor, cap) rows are written
            const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
            if (n_rows) call.he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
        }
    }
    return call.finish(device_ms);
}
