// gnnpe_refine_sets.hip.h -- what the two set-restricted wave searches share: the one-shot k_refine_sets (gnnpe_refine_sets.hip)
// and the paged k_refine_pages (gnnpe_refine_pages.hip).  The plan by position in the matching order, the per-wave search
// state in LDS, the row search, the first-level items.
#pragma once

#include <algorithm>

#include "gnnpe_common.h"

namespace gnnpe {

constexpr int kSetsMaxQ = 32;
constexpr int kSetsWavesPerBlock = kBlock / 64;
constexpr int kSetsBlocksPerCu = 4;  // 16 waves per CU; LDS and registers admit more, the tickets balance whatever is resident

struct SetsPlan {  // indexed by POSITION in the matching order
    uint32_t nq;
    uint32_t label[kSetsMaxQ], degree[kSetsMaxQ];
    uint8_t qv[kSetsMaxQ], pivot[kSetsMaxQ];   // query vertex id of a position; position of its pivot
    uint16_t back_off[kSetsMaxQ + 1];
    uint8_t back[kSetsMaxQ * (kSetsMaxQ - 1) / 2];  // positions of the other earlier neighbours
};

struct SetsWave {  // per-wave search state in LDS; every word is wave-uniform
    uint32_t image[kSetsMaxQ], istart[kSetsMaxQ], ideg[kSetsMaxQ];  // image of a position, its row
    uint32_t cbase[kSetsMaxQ], end[kSetsMaxQ];                      // current chunk of the pivot row, the row's end
    uint32_t mask_lo[kSetsMaxQ], mask_hi[kSetsMaxQ];                // survivors of the current chunk not yet visited
};

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long x)
{
    return ((unsigned long long)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x);
}

// is `target` in the ascending row [st, st + d)?
__device__ __forceinline__ bool row_has(const uint32_t *__restrict__ nbrs, uint32_t st, uint32_t d, uint32_t target)
{
    uint32_t lo = 0, hi = d;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t x = nbrs[st + mid];
        if (x == target) return true;
        if (x < target) lo = mid + 1; else hi = mid;
    }
    return false;
}

// ---- the ORDERED searches (D(C, limit) of include/gnnpe_online.h: one embedding per distinct subgraph) ------------------------
// The pairs (a, b) of host/query_symmetry.h ask for f(a) < f(b).  By position in the matching order every pair binds the LATER
// of its two positions to the image of the earlier one: bit i of gt[d] = the image of position d must be greater than the image
// of position i < d, bit i of lt[d] = smaller.  Position 0 has no bound.  The ordered kernels take this by value beside the plan.
struct SetsOrder {
    uint32_t gt[kSetsMaxQ], lt[kSetsMaxQ];
    uint32_t trim;  // != 0: a pivot row longer than a chunk is cut to the ids inside the bounds when its depth is entered
};

// pos_of[query vertex] = position; returns the number of pairs
template <class Pairs, class PosOf>
static inline uint32_t sets_order_from_pairs(const Pairs &pairs, const PosOf &pos_of, bool trim, SetsOrder *O)
{
    *O = SetsOrder{};
    O->trim = trim ? 1u : 0u;
    for (const auto &ab : pairs) {
        const uint32_t pa = pos_of[ab.first], pb = pos_of[ab.second];
        if (pa < pb) O->gt[pb] |= 1u << pa; else O->lt[pa] |= 1u << pb;
    }
    return (uint32_t)pairs.size();
}

// the one argument of an ordered kernel's parameter pack
__device__ __forceinline__ const SetsOrder &sets_order(const SetsOrder &o) { return o; }

// the bounds of position d from the images of the earlier positions: an image v passes if lo <= v < hi.  Wave-uniform.
__device__ __forceinline__ void order_bounds(const SetsOrder &O, const volatile SetsWave &S, uint32_t d, uint32_t &lo, uint32_t &hi)
{
    lo = 0u;
    hi = 0xFFFFFFFFu;  // (no vertex has this id: a graph has fewer than 2^32 - 1 vertices)
    for (uint32_t g = uni(O.gt[d]); g; g &= g - 1u) lo = max(lo, uni(S.image[__builtin_ctz(g)]) + 1u);
    for (uint32_t l = uni(O.lt[d]); l; l &= l - 1u) hi = min(hi, uni(S.image[__builtin_ctz(l)]));
}

// first index in [b, e) of an ascending row whose entry is >= x, e if there is none.  The whole wave searches: 64 probes spread
// over the range and one ballot leave a 64th of it, so a row of 4 096 entries takes two loads.  b, e, x and the result are
// wave-uniform; no lane reads outside [b, e).
__device__ __forceinline__ uint32_t row_lower_bound(const uint32_t *__restrict__ nbrs, uint32_t b, uint32_t e, uint32_t x, uint32_t lane)
{
    while (e - b > 64u) {
        const uint32_t step = (e - b + 63u) >> 6;  // >= 2
        const uint32_t idx = b + lane * step;
        const bool below = idx < e && nbrs[idx] < x;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(below));  // the row ascends: the probes below x are the first cnt
        if (cnt == 0) return b;
        e = min(e, b + cnt * step);
        b += (cnt - 1u) * step + 1u;
    }
    const uint32_t idx = b + lane;
    const bool below = idx < e && nbrs[idx] < x;
    return b + (uint32_t)__popcll(__ballot(below));
}

// the part [b, e) of a pivot row that can hold ids in [lo, hi); only a row longer than a chunk is searched -- a shorter one is one
// chunk whatever is cut from it, and the lanes' own compare does the rest
__device__ __forceinline__ void order_trim(const uint32_t *__restrict__ nbrs, uint32_t lo, uint32_t hi, uint32_t lane, uint32_t &b, uint32_t &e)
{
    if (e - b <= 64u) return;
    if (lo != 0u) b = row_lower_bound(nbrs, b, e, lo, lane);
    if (hi != 0xFFFFFFFFu && e - b > 0u) e = row_lower_bound(nbrs, b, e, hi, lane);
}

// first-level chunks (of 1 << w_shift entries) in every start candidate's row: the scan's input; entry n_cand = 0 so that the
// scan's last output is the total
static __global__ void k_sets_cand_chunks(uint32_t n_cand, const uint32_t *__restrict__ cand, const uint32_t *__restrict__ adj_deg,
                                          uint32_t w_shift, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_cand) out[i] = i < n_cand ? (adj_deg[cand[i]] + (1u << w_shift) - 1u) >> w_shift : 0u;
}

// log2 of the first-level chunk width: 64 entries unless the graph has hub rows (longer than 64) and the resident grid would
// be short of items.  The host knows the start set's size and the graph's mean degree, not the candidates' own degrees; the
// aim is eight items per resident wave.  Every item costs a ticket, and the tickets of a launch are atomics on one word:
// without hub rows the subtrees are small and alike, and the 24 000 single-entry items of a G(n,m) query took 0.9 ms
// where its 1 200 chunks take 0.1.
static inline uint32_t sets_first_level_shift(uint32_t n_cand, uint64_t entries, uint32_t n, int num_cus, uint32_t n_hub)
{
    if (n_hub == 0 || entries + n >= (1ull << 32)) return 6;  // (the item offsets are 32-bit)
    const uint64_t est = (uint64_t)n_cand * std::max<uint64_t>(1, entries / std::max<uint32_t>(n, 1));
    const uint64_t target = 8ull * (uint64_t)std::max(num_cus, 1) * kSetsBlocksPerCu * kSetsWavesPerBlock;
    uint32_t shift = 6;
    while (shift > 0 && (est >> shift) < target) shift--;
    return shift;
}

}  // namespace gnnpe
