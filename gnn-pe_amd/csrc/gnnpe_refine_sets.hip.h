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
