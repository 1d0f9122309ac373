// gnnpe_refine_ecount.hip.h -- what the kernels that fill a per-edge table share: k_refine_ecount (gnnpe_refine_ecount.hip, E_m(C)),
// k_refine_delta_ecount (gnnpe_refine_delta_counts.hip, EDelta_m(C, F)) and k_refine_delta_nonedges_ecount
// (gnnpe_refine_delta_nonedges_counts.hip, EN_m(C, F)).  The words of the plan edges and how the host derives them
// from a plan, the per-wave state, the entry searches, and the adds of the leaf and of a flush.  The text that explains them is at
// the head of gnnpe_refine_ecount.hip; a kernel keeps its tallies' bookkeeping and its hooks.
#pragma once

#include "gnnpe_records.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

struct EcountEdges {  // (k << 1) | flip of every plan edge: 64 + 992 bytes by value
    uint16_t pivot[kSetsMaxQ];                            // of position d's pivot edge (d >= 1)
    uint16_t back[kSetsMaxQ * (kSetsMaxQ - 1) / 2];       // of P.back[j]
};

struct EcountWave {  // per wave in LDS, wave-uniform
    SetsTally tally;            // finds below the current image of a position
    uint32_t ient[kSetsMaxQ];   // CSR index of the entry (image of pivot[d] -> image of d)
};

// index in nbrs of `target` in the ascending row [st, st + d), kNoEdge if it is not there
__device__ __forceinline__ uint32_t row_pos(const uint32_t *__restrict__ nbrs, uint32_t st, uint32_t d, uint32_t target)
{
    uint32_t lo = 0, hi = d;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t x = nbrs[st + mid];
        if (x == target) return st + mid;
        if (x < target) lo = mid + 1; else hi = mid;
    }
    return kNoEdge;
}

// the reverse (y -> x) of entry j = (x -> y), ys = adj_start[y]; kNoEdge if row y does not hold x
__device__ __forceinline__ uint32_t entry_reverse(const uint32_t *__restrict__ revpos, uint32_t j, uint32_t ys)
{
    const uint32_t r = revpos[j];
    return r == kNoEdge ? kNoEdge : ys + r;
}

// The entry of the data edge between an earlier image w (row ws, dw) and a later image v (row vs, dv): (w -> v), or with `flip`
// (v -> w).  Searched in the shorter row, as the back-edge test does, and reversed if that is the other one.
__device__ __forceinline__ uint32_t back_entry(const uint32_t *__restrict__ nbrs, const uint32_t *__restrict__ revpos, uint32_t w,
                                               uint32_t ws, uint32_t dw, uint32_t v, uint32_t vs, uint32_t dv, bool flip)
{
    const bool in_v = dv <= dw;                                       // the search gives (v -> w), else (w -> v)
    const uint32_t j = in_v ? row_pos(nbrs, vs, dv, w) : row_pos(nbrs, ws, dw, v);
    if (j == kNoEdge || in_v == flip) return j;
    return entry_reverse(revpos, j, in_v ? ws : vs);
}

// The adds of the leaf, for a lane that survived the chunk [cb, ..) at the last position with candidate v: `add` to the entry of each
// query edge of the last position -- its own pivot entry cb + lane and one per back edge
__device__ __forceinline__ void ecount_leaf_adds(const SetsPlan &P, const EcountEdges &X, const volatile SetsWave &S, const SetsGraph &G,
                                                 const uint32_t *__restrict__ revpos, unsigned long long *__restrict__ counts,
                                                 uint64_t entries, uint32_t lane, uint32_t last, uint32_t cb, uint32_t v,
                                                 unsigned long long add)
{
    const uint32_t vs = G.adj_start[v], dv = G.adj_deg[v];
    const uint32_t pw = X.pivot[last];
    uint32_t j = cb + lane;
    if (pw & 1u) j = entry_reverse(revpos, j, vs);
    if (j != kNoEdge) atomicAdd(&counts[(uint64_t)(pw >> 1) * entries + j], add);
    for (uint32_t e = P.back_off[last]; e < P.back_off[last + 1]; e++) {
        const uint32_t b = P.back[e], bw = X.back[e];
        j = back_entry(G.nbrs, revpos, uni(S.image[b]), uni(S.istart[b]), uni(S.ideg[b]), v, vs, dv, (bw & 1u) != 0);
        if (j != kNoEdge) atomicAdd(&counts[(uint64_t)(bw >> 1) * entries + j], add);
    }
}

// The adds of flush(d), d >= 1, for the lanes 0 .. nb (nb = the back edges of position d): `add` to the entry of the lane's edge of
// the position, lane 0 the pivot edge (its entry is ient[d]), then the back edges
__device__ __forceinline__ void ecount_flush_adds(const SetsPlan &P, const EcountEdges &X, const volatile SetsWave &S,
                                                  const volatile EcountWave &E, const SetsGraph &G, const uint32_t *__restrict__ revpos,
                                                  unsigned long long *__restrict__ counts, uint64_t entries, uint32_t lane, uint32_t d,
                                                  unsigned long long add)
{
    const uint32_t v = uni(S.image[d]), vs = uni(S.istart[d]), dv = uni(S.ideg[d]);
    uint32_t j, w16;
    if (lane == 0) {
        w16 = X.pivot[d];
        j = uni(E.ient[d]);
        if (w16 & 1u) j = entry_reverse(revpos, j, vs);
    } else {
        const uint32_t e = P.back_off[d] + lane - 1u, b = P.back[e];
        w16 = X.back[e];
        j = back_entry(G.nbrs, revpos, S.image[b], S.istart[b], S.ideg[b], v, vs, dv, (w16 & 1u) != 0);
    }
    if (j != kNoEdge) atomicAdd(&counts[(uint64_t)(w16 >> 1) * entries + j], add);
}

// The words of a plan's edges: the query edges by number -- from the plan, where repeats of the query file count once as in
// gnnpe_host::query_edges -- and for every plan edge (k << 1) | flip, flip = the earlier position's query vertex is b_k.  Returns nqe;
// *flips counts the flipped plan edges, *backflips those among them that are back edges.  With `anchor_pair` the plan is one of
// build_match_order_from_pair: positions 0 and 1 are a NON-adjacent pair, position 1 names position 0 as its pivot only so that the
// plan is well-formed, and that pseudo-pivot is left out -- it is no query edge, and X->pivot[1] stays 0 and is never read.
static inline uint32_t ecount_edges_from_plan(const SetsPlan &P, EcountEdges *X, uint32_t *flips, uint32_t *backflips,
                                              bool anchor_pair = false)
{
    *X = EcountEdges{};
    *flips = *backflips = 0;
    const uint32_t nq = P.nq;
    std::vector<std::pair<uint32_t, uint32_t>> qe;
    auto norm = [&](uint32_t early, uint32_t late) {
        const uint32_t a = P.qv[early], b = P.qv[late];
        return std::make_pair(std::min(a, b), std::max(a, b));
    };
    for (uint32_t d = 1; d < nq; d++) {
        if (d > 1 || !anchor_pair) qe.push_back(norm(P.pivot[d], d));
        for (uint32_t j = P.back_off[d]; j < P.back_off[d + 1]; j++) qe.push_back(norm(P.back[j], d));
    }
    std::sort(qe.begin(), qe.end());
    qe.erase(std::unique(qe.begin(), qe.end()), qe.end());
    auto word = [&](uint32_t early, uint32_t late, uint32_t *n_flip) {
        const uint32_t k = (uint32_t)(std::lower_bound(qe.begin(), qe.end(), norm(early, late)) - qe.begin());
        const uint32_t flip = P.qv[early] > P.qv[late] ? 1u : 0u;  // the earlier position's query vertex is b_k
        *n_flip += flip;
        return (uint16_t)((k << 1) | flip);
    };
    for (uint32_t d = 1; d < nq; d++) {
        if (d > 1 || !anchor_pair) X->pivot[d] = word(P.pivot[d], d, flips);
        for (uint32_t j = P.back_off[d]; j < P.back_off[d + 1]; j++) X->back[j] = word(P.back[j], d, backflips);
    }
    *flips += *backflips;
    return (uint32_t)qe.size();
}

}  // namespace gnnpe
