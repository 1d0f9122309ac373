// gnnpe_refine_delta.hip.h -- what the searches anchored at the entries of a set F of data edges share: k_refine_delta
// (gnnpe_refine_delta.hip, Delta_m(C, F, limit) and its rows) and k_refine_delta_vcount / k_refine_delta_ecount
// (gnnpe_refine_delta_counts.hip, the tables of the same matches) -- and, anchored at the pairs of a set of NON-edges,
// k_refine_delta_nonedges (gnnpe_refine_delta_nonedges.hip) and k_refine_delta_nonedges_vcount / _ecount
// (gnnpe_refine_delta_nonedges_counts.hip), which take the lookup with its sense inverted, the charging rule, the buffer of F and the
// host's side as they are and share their own item decode (nonedge_item_decode).  On the device the key search, the entries of the
// pairs, the two decodes of an item and the charging rule; on the host F as keys and pairs, the plan of every launch, the staging and the launches.  The
// text that explains them is at the head of gnnpe_refine_delta.hip; a kernel keeps its leaf and its other hooks.
#pragma once

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

// one lane per directed pair (x, y), both below n: the index of y in x's row, or kDeltaNoEntry.  The error flag is raised by a pair
// without an entry where F must hold edges (want_entry != 0), and by a pair WITH one where it must hold non-edges (want_entry == 0,
// gnnpe_refine_delta_nonedges.hip)
static __global__ void k_delta_entries(uint32_t n_pairs, const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ adj_start,
                                       const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                       uint32_t *__restrict__ ent, SetsCounters *ctr, uint32_t want_entry)
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
    if ((j == kDeltaNoEntry) == (want_entry != 0u)) atomicOr(&ctr->bad, 1u);
}

// item q -> the directed entry x -> y at index j of the CSR; x is tested as position 0 (bit x of C, label, degree) and becomes
// image[0], depth 1 is held to the chunk [j, j + 1).  False: a pair that is no edge of the graph (the call is refused), or an x that
// fails.
__device__ __forceinline__ bool delta_item_decode(const SetsPlan &P, volatile SetsWave &S, const SetsGraph &G,
                                                  const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent, uint32_t q)
{
    const uint32_t j = uni(ent[q]);
    if (j == kDeltaNoEntry) return false;
    const uint32_t x = uni(pairs[2 * q]);
    const uint32_t s0 = uni(G.adj_start[x]), d0 = uni(G.adj_deg[x]);
    const uint32_t word = uni(G.bitmap[(uint64_t)P.qv[0] * G.words + (x >> 5)]);
    if (((word >> (x & 31u)) & 1u) == 0 || uni(G.labels[x]) != P.label[0] || d0 < P.degree[0]) return false;
    S.image[0] = x;
    S.istart[0] = s0;
    S.ideg[0] = d0;
    S.cbase[1] = j - 64u;
    S.end[1] = j + 1u;
    S.mask_lo[1] = 0;
    S.mask_hi[1] = 0;
    return true;
}

// item q -> the directed pair (x, y) of F, both below n.  x is tested as position 0 and y as position 1; they become image[0] and
// image[1], and depth 2 is entered over its pivot's row.  False: a pair that is an edge of the graph (the call is refused), or an x
// or y that fails.
template <bool kOrdered, class... Ord>
__device__ __forceinline__ bool nonedge_item_decode(const SetsPlan &P, volatile SetsWave &S, const SetsGraph &G,
                                                    const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ ent, uint32_t q,
                                                    uint32_t lane, const Ord &...ord)
{
    if (uni(ent[q]) != kDeltaNoEntry) return false;
    const uint32_t x = uni(pairs[2 * q]), y = uni(pairs[2 * q + 1]);
    const uint32_t sx = uni(G.adj_start[x]), dx = uni(G.adj_deg[x]), sy = uni(G.adj_start[y]), dy = uni(G.adj_deg[y]);
    const uint32_t wx = uni(G.bitmap[(uint64_t)P.qv[0] * G.words + (x >> 5)]), wy = uni(G.bitmap[(uint64_t)P.qv[1] * G.words + (y >> 5)]);
    if (x == y || ((wx >> (x & 31u)) & 1u) == 0 || ((wy >> (y & 31u)) & 1u) == 0) return false;
    if (uni(G.labels[x]) != P.label[0] || dx < P.degree[0] || uni(G.labels[y]) != P.label[1] || dy < P.degree[1]) return false;
    S.image[0] = x;
    S.istart[0] = sx;
    S.ideg[0] = dx;
    if constexpr (kOrdered) {
        uint32_t lo, hi;
        order_bounds(sets_order(ord...), S, 1, lo, hi);
        if (y < lo || y >= hi) return false;
    }
    S.image[1] = y;
    S.istart[1] = sy;
    S.ideg[1] = dy;
    const uint32_t p = P.pivot[2], ps = uni(S.istart[p]);
    uint32_t rb = ps, re = ps + uni(S.ideg[p]);
    if constexpr (kOrdered) {
        if (sets_order(ord...).trim) {
            uint32_t lo, hi;
            order_bounds(sets_order(ord...), S, 2, lo, hi);
            order_trim(G.nbrs, lo, hi, lane, rb, re);
        }
    }
    S.cbase[2] = rb - 64u;
    S.end[2] = re;
    S.mask_lo[2] = 0;
    S.mask_hi[2] = 0;
    return true;
}

// the charging rule, the `test` hook of the walk: for a lane that passed sets_lane_test with candidate v at depth d, a query edge
// numbered below this launch's must not land in F
__device__ __forceinline__ bool delta_older_ok(const SetsDelta &D, const volatile SetsWave &S, const unsigned long long *__restrict__ keys,
                                               uint32_t n_keys, uint32_t d, uint32_t v)
{
    bool ok = true;
    for (uint32_t o = uni(D.older[d]); o && ok; o &= o - 1u) {
        const uint32_t w = uni(S.image[__builtin_ctz(o)]);
        ok = !delta_has(keys, n_keys, ((unsigned long long)min(v, w) << 32) | max(v, w));
    }
    return ok;
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

// ---- the host's side of a delta call -----------------------------------------------------------------------------------------
// F and the launches of a call, after sets_prepare: F as ascending keys and as the 2 |F| directed pairs (the items), the query edges,
// and per query edge k the plan in the order anchored at it, the earlier neighbours by a lower-numbered edge and pos_of[query
// vertex] of that order.
struct DeltaPlans {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> pairs;
    std::vector<std::pair<uint32_t, uint32_t>> qe;  // the anchors of the launches: the query edges (or the non-adjacent query pairs)
    std::vector<SetsQuery> plans;
    std::vector<SetsDelta> older;
    std::vector<std::vector<uint32_t>> pos_of;
    bool nothing = false;  // limit 0, an empty set, no F, a single-vertex query: nothing is launched
    uint32_t n_items = 0;
};

// Fills D.  A loop or an id the graph does not have is refused here, before anything is launched; with D->nothing the pairs and the
// plans are not built.  With `nonedges` (gnnpe_refine_delta_nonedges.hip) the anchors `qe` of the launches are the query's
// non-adjacent pairs in the place of its edges, each with the order of build_match_order_from_pair; `older` then holds the earlier
// positions joined to a position by a lower-numbered non-adjacent pair.
static inline int delta_plans(const char *who, gnnpe_ctx *c, const SetsQuery &Q, const gnnpe_host::StaticGraph &q, const uint32_t *delta_edges,
                              uint64_t n_delta, uint32_t mode, DeltaPlans *D, bool nonedges = false)
{
    std::string err;
    if (gnnpe_host::delta_edge_keys(c->n, delta_edges, n_delta, &D->keys, &err) != 0) {
        set_error("%s: %s", who, err.c_str());
        return GNNPE_ERR_ARG;
    }
    D->qe = nonedges ? gnnpe_host::query_nonedges(q) : gnnpe_host::query_edges(q);
    D->nothing = Q.empty || D->keys.empty() || D->qe.empty();
    if (D->nothing) return GNNPE_OK;
    const size_t n_keys = D->keys.size();
    GNNPE_REQUIRE(2 * (uint64_t)n_keys < (1ull << 32), GNNPE_ERR_ARG, "%s: %zu different delta edges, the items are 32-bit", who, n_keys);
    D->n_items = (uint32_t)(2 * n_keys);
    D->pairs.resize(4 * n_keys);
    for (size_t i = 0; i < n_keys; i++) {
        const uint32_t lo = (uint32_t)(D->keys[i] >> 32), hi = (uint32_t)D->keys[i];
        D->pairs[4 * i] = D->pairs[4 * i + 3] = lo;
        D->pairs[4 * i + 1] = D->pairs[4 * i + 2] = hi;
    }
    // the plan of every launch: the order anchored at the query edge, and the earlier neighbours by a lower-numbered edge
    const bool distinct = (mode & GNNPE_MATCH_DISTINCT) != 0, induced = (mode & GNNPE_MATCH_INDUCED) != 0;
    const size_t nqe = D->qe.size();
    D->plans.assign(nqe, SetsQuery{});
    D->older.assign(nqe, SetsDelta{});
    D->pos_of.resize(nqe);
    for (size_t k = 0; k < nqe; k++) {
        gnnpe_host::MatchOrder mo;
        if ((nonedges ? gnnpe_host::build_match_order_from_pair : gnnpe_host::build_match_order_from_edge)(q, D->qe[k].first, D->qe[k].second, &mo,
                                                                                                             &err) != 0) {
            set_error("%s: %s", who, err.c_str());
            return GNNPE_ERR_ARG;
        }
        D->pos_of[k] = sets_plan_from_order(q, mo, distinct, induced, c->sw.sets_trim, &D->plans[k]);
        for (size_t e = 0; e < k; e++) {
            const uint32_t pa = D->pos_of[k][D->qe[e].first], pb = D->pos_of[k][D->qe[e].second];
            D->older[k].older[std::max(pa, pb)] |= 1u << std::min(pa, pb);
        }
    }
    return GNNPE_OK;
}

// The staging of a call whose buffers (q_work, q_bitmap, q_delta) are reserved, on the context's stream: F and the bitmap go up, the
// counters are zeroed, ev0 is recorded and k_delta_entries looks the pairs up -- each must be an edge of the graph, or with
// `nonedges` none of them may be.  Returns the blocks of a search launch: a resident grid, or as many waves as there are items.
// (A cursor hands in its own reserved buffers in the place of the context's: `work` begins with the counter block.)  With `res` the
// bitmap is not uploaded: the search reads res->d_bitmap.
static inline uint32_t delta_stage(SetsCall &call, gnnpe_ctx *c, const SetsQuery &Q, const DeltaPlans &D, const uint32_t *bitmap,
                                   bool nonedges = false, const DevBuf *work = nullptr, const DevBuf *bm = nullptr, const DevBuf *fset = nullptr,
                                   const SetsResident *res = nullptr)
{
    const size_t n_keys = D.keys.size();
    SetsCounters *ctr = (work ? *work : c->q_work).as<SetsCounters>();
    const DeltaBuf F(fset ? *fset : c->q_delta, n_keys);
    void *d_bitmap = (bm ? *bm : c->q_bitmap).p;
    if (call.ok()) call.he = hipMemcpyAsync(F.keys, D.keys.data(), n_keys * 8, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemcpyAsync(F.pairs, D.pairs.data(), n_keys * 16, hipMemcpyHostToDevice, c->stream);
    if (call.ok() && !res) call.he = hipMemcpyAsync(d_bitmap, bitmap, (size_t)Q.nq * Q.words * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemsetAsync(ctr, 0, SetsWork::kCtrBytes, c->stream);
    if (call.ok() && call.ev0) call.he = hipEventRecord(call.ev0, c->stream);
    call.launch([&] {
        hipLaunchKernelGGL(k_delta_entries, dim3((D.n_items + 255) / 256), dim3(256), 0, c->stream, D.n_items, F.pairs,
                           c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), F.ent, ctr, nonedges ? 0u : 1u);
    });
    return (uint32_t)std::min<uint64_t>(sets_grid_blocks(c, Q.nq, D.n_items), (D.n_items + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
}

// One launch per anchor (query edge, or non-adjacent query pair) against the one counter block: launch(k, plan of k, ord...) starts
// the kernel of launch k in the instantiation the plan asks for; the ticket is cleared in between, total and the second counter word
// go on.
// (the pairs and the non-edges are the query's, whatever the order: every launch runs the same instantiation -- also where the
// anchor is a non-adjacent pair and left out of the plan's non-edges, since every launch then tests one pair fewer than the query has)
template <class Launch>
static inline void delta_launches(SetsCall &call, gnnpe_ctx *c, const DeltaPlans &D, Launch &&launch)
{
    SetsCounters *ctr = c->q_work.as<SetsCounters>();
    for (size_t k = 0; k < D.plans.size(); k++) {
        const SetsQuery &K = D.plans[k];
        if (k && call.ok()) call.he = hipMemsetAsync(&ctr->ticket, 0, 4, c->stream);  // the next launch's tickets
        call.launch([&] { sets_dispatch(K, [&](auto... ord) { launch(k, K, ord...); }); });
    }
}

}  // namespace gnnpe
