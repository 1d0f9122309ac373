// gnnpe_refine_delta.hip -- THE MATCHES THROUGH A SET OF DATA EDGES, each once: Delta_m(C, F, limit) of include/gnnpe_online.h,
// the primitive of incremental subgraph matching (the new matches after an insertion, the vanishing ones before a deletion).
//
// The search is k_refine_sets' (gnnpe_refine_sets.hip): the same resident grid and tickets, the same loop over the shared steps
// of gnnpe_refine_sets.hip.h (sets_lane_test, sets_descend), the same leaf (total, rows through the cursor, the flush every 1024
// finds) and the same polling.  What is this file's own:
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
// The shared device code is used as it is; the test above is ANDed onto its result here.
// Resources of the four instantiations and the measurement: profiles/online_delta.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

struct DeltaCounters {  // one 32-byte block, zeroed once per call; the ticket alone is cleared between the launches
    unsigned long long total, cursor;
    uint32_t ticket, bad, pad[2];  // bad != 0: a pair of F is no edge of the graph
};
static_assert(sizeof(DeltaCounters) == SetsWork::kCtrBytes, "the counters of the work buffer");

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
                                       uint32_t *__restrict__ ent, DeltaCounters *ctr)
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
                                                        uint64_t words, unsigned long long limit, DeltaCounters *ctr,
                                                        uint32_t *__restrict__ matches, unsigned long long matches_cap, Ord... ord)
{
    __shared__ SetsWave s_wave[kSetsWavesPerBlock];
    volatile SetsWave &S = s_wave[threadIdx.x >> 6];
    const SetsGraph G = {adj_start, adj_deg, nbrs, labels, bitmap, words};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nq = P.nq, last = nq - 1;
    bool rows_full = matches == nullptr;  // no row left to reserve

    for (;;) {
        if (__hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= limit) return;
        uint32_t q = 0;
        if (lane == 0) q = atomicAdd(&ctr->ticket, 1u);
        q = uni(q);
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

        // the chunk of survivors at the last depth: count them, store their rows
        auto leaf = [&](uint32_t d, bool ok, uint32_t v) {
            const unsigned long long m = __ballot(ok);
            const uint32_t cnt = (uint32_t)__popcll(m);
            if (cnt == 0) return;
            if (!rows_full) {
                unsigned long long slot = 0;
                if (lane == 0) slot = atomicAdd(&ctr->cursor, (unsigned long long)cnt);
                slot = uni64(slot);
                if (slot >= matches_cap) rows_full = true;
                slot += (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
                if (ok && slot < matches_cap) {
                    uint32_t *row = matches + slot * nq;
                    for (uint32_t i = 0; i < d; i++) row[P.qv[i]] = S.image[i];
                    row[P.qv[d]] = v;
                }
            }
            pending += cnt;
            if (pending >= 1024ull) {
                unsigned long long before = 0;
                if (lane == 0) before = atomicAdd(&ctr->total, pending);
                before = uni64(before);
                stop = before + pending >= limit;
                pending = 0;
            }
        };

        uint32_t d = 1, steps = 0;
        while (d >= 1 && !stop) {
            // a subtree that finds little still hears of the limit: a look at the total every 1024 chunks
            if ((++steps & 1023u) == 0 &&
                __hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + pending >= limit)
                break;
            unsigned long long m = ((unsigned long long)uni(S.mask_hi[d]) << 32) | uni(S.mask_lo[d]);
            if (m == 0) {
                // next chunk of the pivot row
                const uint32_t cb = uni(S.cbase[d]) + 64u, ce = uni(S.end[d]);
                if ((int32_t)(ce - cb) <= 0) {
                    d--;
                    continue;
                }
                S.cbase[d] = cb;
                uint32_t v;
                bool ok = sets_lane_test<kOrdered>(P, S, G, d, cb, ce, lane, v, ord...);
                // the charging rule: a query edge numbered below this launch's must not land in F
                if (ok) {
                    for (uint32_t o = uni(D.older[d]); o && ok; o &= o - 1u) {
                        const uint32_t w = uni(S.image[__builtin_ctz(o)]);
                        ok = !delta_has(keys, n_keys, ((unsigned long long)min(v, w) << 32) | max(v, w));
                    }
                }
                if (d == last) {
                    leaf(d, ok, v);
                    continue;
                }
                m = __ballot(ok);
                if (m == 0) continue;
            }
            sets_descend<kOrdered>(P, S, G, d, m, lane, ord...);
        }
        if (pending && lane == 0) atomicAdd(&ctr->total, pending);
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
    DeltaCounters *ctr = c->q_work.as<DeltaCounters>();
    const DeltaBuf F(c->q_delta, n_keys);
    uint32_t *d_rows = matches_cap ? c->q_matches.as<uint32_t>() : nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t he = hipSuccess;
    if (device_ms) he = hipEventCreate(&ev0);
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev1);
    if (he == hipSuccess) he = hipMemcpyAsync(F.keys, keys.data(), n_keys * 8, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(F.pairs, pairs.data(), n_keys * 16, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(c->q_bitmap.p, candidate_bitmap, bm_bytes, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemsetAsync(ctr, 0, SetsWork::kCtrBytes, c->stream);
    if (he == hipSuccess && device_ms) he = hipEventRecord(ev0, c->stream);
    // a resident grid, or as many waves as there are items
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(sets_grid_blocks(c, nq, n_items), (n_items + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
    if (c->sw.debug)
        fprintf(stderr, "[refine_delta] edges=%zu items=%u launches=%zu blocks=%u pairs=%u nonedges=%u\n", n_keys, n_items, qe.size(), blocks,
                plans[0].n_pairs, plans[0].n_non);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_delta_entries, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, n_items, F.pairs, c->adj_start.as<uint32_t>(),
                           c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), F.ent, ctr);
        he = hipGetLastError();
    }
    for (size_t k = 0; k < qe.size() && he == hipSuccess; k++) {
        const SetsQuery &K = plans[k];
        auto launch = [&](auto... ord) {
            hipLaunchKernelGGL((k_refine_delta<kSetsOrdered<decltype(ord)...>, decltype(ord)...>), dim3(blocks), dim3(kBlock), 0, c->stream, K.P,
                               older[k], n_items, F.pairs, F.ent, F.keys, (uint32_t)n_keys, c->adj_start.as<uint32_t>(),
                               c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->q_bitmap.as<uint32_t>(), Q.words,
                               (unsigned long long)limit, ctr, d_rows, (unsigned long long)matches_cap, ord...);
        };
        if (k) he = hipMemsetAsync(&ctr->ticket, 0, 4, c->stream);  // the next launch's tickets; total and cursor go on
        if (he != hipSuccess) break;
        // (the pairs and the non-edges are the query's, whatever the order: every launch runs the same instantiation)
        if (K.n_non)
            K.n_pairs ? launch(K.O, K.N) : launch(K.N);
        else
            K.n_pairs ? launch(K.O) : launch();
        he = hipGetLastError();
    }
    if (he == hipSuccess && device_ms) he = hipEventRecord(ev1, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(c->h_pinned, ctr, sizeof(DeltaCounters), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);  // the one wait of the call
    if (he == hipSuccess) {
        const uint32_t bad = reinterpret_cast<const uint32_t *>(c->h_pinned)[5];
        if (bad) {
            set_error("%s: a delta edge is not an edge of the graph", who);
            rc = GNNPE_ERR_ARG;
        } else {
            *answers = std::min<uint64_t>(c->h_pinned[0], limit);
            // every find reserved a row, so the first min(cursor, cap) rows are written
            const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
            if (n_rows) he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
        }
    }
    if (he == hipSuccess && !rc && device_ms) {
        float ms = 0.f;
        he = hipEventElapsedTime(&ms, ev0, ev1);
        *device_ms = ms;
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipStreamSynchronize(c->stream);
    if (!rc && he != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(he));
        rc = GNNPE_ERR_HIP;
    }
    return rc;
}
