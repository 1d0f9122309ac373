// gnnpe_refine_sets.hip.h -- what the set-restricted wave searches share: the one-shot k_refine_sets (gnnpe_refine_sets.hip),
// k_refine_vcount, k_refine_ecount and k_refine_delta (the files of those names), k_refine_delta_vcount and k_refine_delta_ecount
// (gnnpe_refine_delta_counts.hip), k_refine_delta_nonedges (gnnpe_refine_delta_nonedges.hip), k_refine_delta_nonedges_vcount and
// k_refine_delta_nonedges_ecount (gnnpe_refine_delta_nonedges_counts.hip), k_refine_delta_vertices (the file of that name) and the paged k_refine_pages (gnnpe_refine_pages.hip).
//   * All of them, on the device: the plan by position in the matching order, the per-wave search state in LDS and every STEP of the
//     search: a chunk's lane test, the descent into a survivor, the decode of a first-level item, the single-vertex item.  On the
//     host the preparation of a query (sets_prepare), the staging of its first-level items (sets_stage_items) and the choice of
//     the instantiation (sets_dispatch).
//   * The one-shot kernels, on the device: the counter block, the ticket take, the find accounting and the limit, the loop
//     that drives the steps (sets_walk), the row-writing leaf of two of them and the tallies of the others.  A kernel keeps
//     its item setup and its hooks.  On the host the events, the single wait and the error translation of a call (SetsCall) and
//     the table handling of the two count calls (sets_count_call).
// k_refine_pages keeps its own loop, leaf and polling.
#pragma once

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../host/graph_loader.h"
#include "../host/query_symmetry.h"
#include "../host/refine.h"
#include "../host/refine_sets.h"
#include "../../include/gnnpe_online.h"
#include "gnnpe_common.h"
#include "gnnpe_touched.hip.h"

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

// ---- the INDUCED searches (I(C, limit) and ID(C, limit) of include/gnnpe_online.h: query non-edges land on data non-edges) ------
// By position in the matching order: bit i < d of non[d] = positions i and d are NOT adjacent in the query, i.e. i is neither the
// pivot of d nor one of its back neighbours.  The induced kernels take this by value beside the plan, after the SetsOrder of an
// ordered one: 128 bytes.
struct SetsNon {
    uint32_t non[kSetsMaxQ];
};

// what a kernel's parameter pack holds: nothing (plain), SetsOrder (ordered), SetsNon (induced), or SetsOrder and SetsNon
template <class... Ext>
constexpr bool kSetsOrdered = (std::is_same_v<Ext, SetsOrder> || ...);
template <class... Ext>
constexpr bool kSetsInduced = (std::is_same_v<Ext, SetsNon> || ...);

// the SetsOrder of an ordered kernel's parameter pack, the SetsNon of an induced one's
__device__ __forceinline__ const SetsOrder &sets_order(const SetsOrder &o) { return o; }
__device__ __forceinline__ const SetsOrder &sets_order(const SetsOrder &o, const SetsNon &) { return o; }
__device__ __forceinline__ const SetsNon &sets_non(const SetsNon &n) { return n; }
__device__ __forceinline__ const SetsNon &sets_non(const SetsOrder &, const SetsNon &n) { return n; }

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

// ---- the steps of the search ---------------------------------------------------------------------------------------------------
// Every kernel builds a SetsGraph from their own parameters and keep the conventions of the state: S is read and written through
// `volatile SetsWave &`, every word read from it goes through uni(), and no lane reads LDS that another lane alone wrote (every
// lane writes every word).  The ordered instantiations pass their SetsOrder as the trailing pack, the induced ones their SetsNon
// (after the SetsOrder, if both), the plain ones nothing.
struct SetsGraph {
    const uint32_t *__restrict__ adj_start, *__restrict__ adj_deg, *__restrict__ nbrs, *__restrict__ labels, *__restrict__ bitmap;
    uint64_t words;
};

// the lane's entry v of the chunk [cb, ce) of depth d's pivot row and its test: set bit, label, degree, the ordered bounds, not in
// the image, every back edge by binary search in the SHORTER of the two rows; in the induced form, for the lanes still standing,
// every earlier image that is no query neighbour by the same search, which must NOT find it
template <bool kOrdered, class... Ord>
__device__ __forceinline__ bool sets_lane_test(const SetsPlan &P, const volatile SetsWave &S, const SetsGraph &G, uint32_t d, uint32_t cb,
                                               uint32_t ce, uint32_t lane, uint32_t &v, const Ord &...ord)
{
    const uint32_t idx = cb + lane;
    bool ok = idx < ce;
    v = ok ? G.nbrs[idx] : 0u;
    const uint32_t word = G.bitmap[(uint64_t)P.qv[d] * G.words + (v >> 5)], lab = G.labels[v], dv = G.adj_deg[v];
    ok = ok & (((word >> (v & 31u)) & 1u) != 0) & (lab == P.label[d]) & (dv >= P.degree[d]);
    if constexpr (kOrdered) {
        uint32_t lo, hi;
        order_bounds(sets_order(ord...), S, d, lo, hi);
        ok = ok & (v >= lo) & (v < hi);
    }
    for (uint32_t i = 0; i < d; i++) ok &= S.image[i] != v;
    if (ok && P.back_off[d] < P.back_off[d + 1]) {
        const uint32_t vs = G.adj_start[v];
        for (uint32_t j = P.back_off[d]; j < P.back_off[d + 1] && ok; j++) {
            const uint32_t b = P.back[j], w = S.image[b], ws = S.istart[b], dw = S.ideg[b];
            ok = dv <= dw ? row_has(G.nbrs, vs, dv, w) : row_has(G.nbrs, ws, dw, v);
        }
    }
    if constexpr (kSetsInduced<Ord...>) {
        if (ok) {
            const uint32_t vs = G.adj_start[v];
            for (uint32_t m = uni(sets_non(ord...).non[d]); m && ok; m &= m - 1u) {
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                const uint32_t w = uni(S.image[i]), ws = uni(S.istart[i]), dw = uni(S.ideg[i]);
                ok = !(dv <= dw ? row_has(G.nbrs, vs, dv, w) : row_has(G.nbrs, ws, dw, v));
            }
        }
    }
    return ok;
}

// descend into the lowest survivor of depth d's chunk: the others stay as its mask, the survivor becomes the image of d, and
// d + 1 is entered over its pivot's row (in the ordered form cut to the bounds) with no survivors yet
template <bool kOrdered, class... Ord>
__device__ __forceinline__ void sets_descend(const SetsPlan &P, volatile SetsWave &S, const SetsGraph &G, uint32_t &d, unsigned long long m,
                                             uint32_t lane, const Ord &...ord)
{
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    m &= m - 1;
    S.mask_lo[d] = (uint32_t)m;
    S.mask_hi[d] = (uint32_t)(m >> 32);
    const uint32_t v = uni(G.nbrs[uni(S.cbase[d]) + bit]);
    S.image[d] = v;
    S.istart[d] = uni(G.adj_start[v]);
    S.ideg[d] = uni(G.adj_deg[v]);
    d++;
    const uint32_t p = P.pivot[d], ps = uni(S.istart[p]);
    if constexpr (kOrdered) {
        uint32_t rb = ps, re = ps + uni(S.ideg[p]);
        if (sets_order(ord...).trim) {
            uint32_t lo, hi;
            order_bounds(sets_order(ord...), S, d, lo, hi);
            order_trim(G.nbrs, lo, hi, lane, rb, re);
        }
        S.cbase[d] = rb - 64u;
        S.end[d] = re;
    } else {
        S.cbase[d] = ps - 64u;
        S.end[d] = ps + uni(S.ideg[p]);
    }
    S.mask_lo[d] = 0;
    S.mask_hi[d] = 0;
}

// item q -> (start candidate, chunk of its row): the largest ci with item_off[ci] <= q.  A start candidate of the right label
// and degree becomes the image of position 0 and depth 1 (its pivot is position 0) is held to the item's chunk; false otherwise.
__device__ __forceinline__ bool sets_item_decode(const SetsPlan &P, volatile SetsWave &S, const SetsGraph &G, uint32_t n_cand,
                                                 const uint32_t *__restrict__ cand, const uint32_t *__restrict__ item_off, uint32_t w_shift,
                                                 uint32_t q)
{
    uint32_t lo = 0, hi = n_cand;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (item_off[mid] <= q) lo = mid; else hi = mid;
    }
    lo = uni(lo);
    const uint32_t v0 = uni(cand[lo]);
    const uint32_t s0 = uni(G.adj_start[v0]), d0 = uni(G.adj_deg[v0]);
    if (uni(G.labels[v0]) != P.label[0] || d0 < P.degree[0]) return false;
    S.image[0] = v0;
    S.istart[0] = s0;
    S.ideg[0] = d0;
    const uint32_t c0 = s0 + ((q - uni(item_off[lo])) << w_shift);
    S.cbase[1] = c0 - 64u;
    S.end[1] = min(c0 + (1u << w_shift), s0 + d0);
    S.mask_lo[1] = 0;
    S.mask_hi[1] = 0;
    return true;
}

// a single-vertex query: an item is 64 start candidates, lane's index i; its candidate, and the whole test of it
__device__ __forceinline__ uint32_t sets_single_cand(uint32_t n_cand, const uint32_t *__restrict__ cand, uint32_t i)
{
    return i < n_cand ? cand[i] : 0u;
}
__device__ __forceinline__ bool sets_single_test(const SetsPlan &P, const SetsGraph &G, uint32_t n_cand, uint32_t i, uint32_t v)
{
    return i < n_cand && G.labels[v] == P.label[0] && G.adj_deg[v] >= P.degree[0];
}

// ---- the walk of the one-shot kernels ------------------------------------------------------------------------------------------
// k_refine_sets, k_refine_vcount, k_refine_ecount, k_refine_delta and k_refine_delta_nonedges are one search: a wave takes a ticket, walks the item's subtree
// chunk by chunk and leaves when the total has reached the limit.  That protocol exists once, here; a kernel adds its item setup and
// the hooks of sets_walk.  (k_refine_pages suspends and resumes and has no limit: it keeps its own loop over the same steps.)
// The three places where a wave hears of the limit are marked EXIT 1, 2 and 3; the proof in gnnpe_refine_vcount.hip that a count
// table is complete iff total < limit rests on these three being the only ones.
struct SetsCounters {  // the 32-byte block at the head of the work buffer (SetsWork), zeroed before every call
    unsigned long long total;  // finds, each added once
    union {
        unsigned long long cursor;      // k_refine_sets, k_refine_delta: rows reserved
        unsigned long long flush_adds;  // the kernels that fill a table: the atomic adds of their flushes (GNNPE_DEBUG prints it)
    };
    uint32_t ticket;  // the next item
    uint32_t bad;     // k_delta_entries: a pair of F is no edge of the graph (the delta table kernels leave when it is set)
    uint32_t pad[2];
};

// the head of a wave's outer loop: the look at the total before an item, and the item's ticket.  A wave whose ticket is not below
// the item count leaves as well.  (Two functions and the two returns in the kernel: one function with one result costs every
// kernel a flag and a branch more per item.)
__device__ __forceinline__ bool sets_limit_reached(const SetsCounters *ctr, unsigned long long limit)
{
    return __hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= limit;  // EXIT 1
}
__device__ __forceinline__ uint32_t sets_take_ticket(SetsCounters *ctr, uint32_t lane)
{
    uint32_t q = 0;
    if (lane == 0) q = atomicAdd(&ctr->ticket, 1u);
    return uni(q);
}

// cnt finds more: `pending` holds a wave's finds not yet added to the total and goes there every 1024; `stop` = that add reached
// the limit.  Both are registers of the calling kernel.
__device__ __forceinline__ void sets_found(SetsCounters *ctr, unsigned long long limit, uint32_t lane, uint32_t cnt, unsigned long long &pending,
                                           bool &stop)
{
    pending += cnt;
    if (pending >= 1024ull) {
        unsigned long long before = 0;
        if (lane == 0) before = atomicAdd(&ctr->total, pending);
        before = uni64(before);
        stop = before + pending >= limit;  // EXIT 2 (sets_walk and the kernel's `if (stop) return` act on it)
        pending = 0;
    }
}

// the end of an item: what is left of `pending`
__device__ __forceinline__ void sets_item_end(SetsCounters *ctr, uint32_t lane, unsigned long long pending)
{
    if (pending && lane == 0) atomicAdd(&ctr->total, pending);
}

// the leaf of the kernels that write rows: the survivors `ok` of a chunk at the last position d, lane's candidate v.  One atomic add
// on the row cursor reserves a row each; lanes whose row is below the cap store image + own v in query-vertex order.
__device__ __forceinline__ void sets_leaf_rows(const SetsPlan &P, const volatile SetsWave &S, SetsCounters *ctr, unsigned long long limit,
                                               uint32_t *__restrict__ matches, unsigned long long matches_cap, bool &rows_full, uint32_t lane,
                                               uint32_t d, bool ok, uint32_t v, unsigned long long &pending, bool &stop)
{
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
            uint32_t *row = matches + slot * P.nq;
            for (uint32_t i = 0; i < d; i++) row[P.qv[i]] = S.image[i];
            row[P.qv[d]] = v;
        }
    }
    sets_found(ctr, limit, lane, cnt, pending, stop);
}

// the tallies of the kernels that fill a table: per wave in LDS, wave-uniform, the finds below the current image of a position, low
// and high word.  The conventions of SetsWave hold: every lane writes every word, every read goes through uni().
struct SetsTally {
    uint32_t lo[kSetsMaxQ], hi[kSetsMaxQ];
};
__device__ __forceinline__ unsigned long long tally_get(const volatile SetsTally &T, uint32_t d)
{
    return ((unsigned long long)uni(T.hi[d]) << 32) | uni(T.lo[d]);
}
__device__ __forceinline__ void tally_set(volatile SetsTally &T, uint32_t d, unsigned long long x)
{
    T.lo[d] = (uint32_t)x;
    T.hi[d] = (uint32_t)(x >> 32);
}

// a hook of sets_walk that a kernel does not need: it does nothing, and as a test it passes.  (By value: a reference to the walk's d
// or to a lane's ok would keep them in memory until the inlining is done, and the code that comes out holds more registers.)
struct SetsNoHook {
    template <class... A>
    __device__ __forceinline__ bool operator()(A...) const
    {
        return true;
    }
};

// The walk of an item below depth `first`, which sets_item_decode (or a kernel's own decode) has entered: per step the next chunk of the
// current depth's pivot row, its lane test, the leaf at the last depth and the descent into a survivor above it; up when a row is
// exhausted, done when depth `first` is.  A kernel's own work is four inlined callables:
//   test(d, v)          for a lane that passed sets_lane_test with candidate v at depth d: false fails it
//   leaf(d, cb, ok, v)  the chunk [cb, ..) at the last depth d: counts the survivors `ok` (sets_found) and does with them what the
//                       kernel is for
//   up(d)               the row of depth d < last is exhausted (the subtree of the last image of d is complete), before d--
//   down(d, m)          before the descent into the lowest survivor of m at depth d
// `pending` and `stop` are the kernel's registers, which its leaf passes to sets_found; the walk only reads them.  `last` is the last
// position, nq - 1, which every kernel holds already.  `first` is the depth the decode has entered and the walk ends below: the
// literal 1 for every kernel whose item fixes position 0, 2 for k_refine_delta_nonedges and the two table kernels over non-edges,
// whose item fixes positions 0 and 1 (so `up` and `down` are never called for depth 1: those kernels flush it themselves).
template <bool kOrdered, class Test, class Leaf, class Up, class Down, class... Ord>
__device__ __forceinline__ void sets_walk(const SetsPlan &P, volatile SetsWave &S, const SetsGraph &G, const SetsCounters *ctr,
                                          unsigned long long limit, uint32_t lane, const unsigned long long &pending, const bool &stop, uint32_t last,
                                          uint32_t first, Test &&test, Leaf &&leaf, Up &&up, Down &&down, const Ord &...ord)
{
    uint32_t d = first, steps = 0;
    while (d >= first && !stop) {
        // a subtree that finds little still hears of the limit: a look at the total every 1024 chunks
        if ((++steps & 1023u) == 0 && __hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + pending >= limit)
            break;  // EXIT 3
        unsigned long long m = ((unsigned long long)uni(S.mask_hi[d]) << 32) | uni(S.mask_lo[d]);
        if (m == 0) {
            // next chunk of the pivot row
            const uint32_t cb = uni(S.cbase[d]) + 64u, ce = uni(S.end[d]);
            if ((int32_t)(ce - cb) <= 0) {
                if (d < last) up(d);
                d--;
                continue;
            }
            S.cbase[d] = cb;
            uint32_t v;
            const bool ok = sets_lane_test<kOrdered>(P, S, G, d, cb, ce, lane, v, ord...) && test(d, v);
            if (d == last) {
                leaf(d, cb, ok, v);
                continue;
            }
            m = __ballot(ok);
            if (m == 0) continue;
        }
        down(d, m);
        sets_descend<kOrdered>(P, S, G, d, m, lane, ord...);
    }
}

// ---- the host's side of the calls ------------------------------------------------------------------------------------------
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

// A query as both calls launch it: the plan and the ordering constraints by position, the start candidates.
struct SetsQuery {
    SetsPlan P = {};
    SetsOrder O = {};      // of a distinct call
    uint32_t n_pairs = 0;  // 0: no ordered kernel (a call that is not distinct, or a query without symmetry)
    SetsNon N = {};        // of an induced call
    uint32_t n_non = 0;    // non-adjacent pairs; 0: no induced kernel (a call that is not induced, or a query without a non-edge)
    uint32_t nq = 0, n_cand = 0;
    uint64_t words = 0;
    std::vector<uint32_t> cand;    // C(start vertex) below n, ascending; sets_stage_items uploads it
    bool empty = false;            // limit 0 or an empty set: there is nothing to launch
    uint32_t w_shift = 6;          // log2 of the first-level chunk width (sets_stage_items)
    bool forced = false;           // ... taken from GNNPE_TESTING=sets_first_shift=K, not from the heuristic
};

// The plan of a matching order by position, with the ordering constraints of a distinct call and the non-edges of an induced one:
// what sets_prepare launches for the order of build_match_order, and gnnpe_refine_sets_delta for the order anchored at each query
// edge.  Fills Q->P, Q->O, Q->n_pairs, Q->N and Q->n_non; returns pos_of[query vertex] = position.
static inline std::vector<uint32_t> sets_plan_from_order(const gnnpe_host::StaticGraph &q, const gnnpe_host::MatchOrder &mo, bool distinct,
                                                         bool induced, bool trim, SetsQuery *Q)
{
    const uint32_t nq = q.n;
    // plan by position in the order.  P.back holds every query edge: 32 vertices have at most 496 edges, back leaves out the 31
    // pivot edges, and sizeof(P.back) is 496
    SetsPlan &P = Q->P;
    static_assert(sizeof(P.back) == kSetsMaxQ * (kSetsMaxQ - 1) / 2, "one byte per possible query edge");
    P = SetsPlan{};
    P.nq = nq;
    std::vector<uint32_t> pos_of(nq, 0);
    for (uint32_t i = 0; i < nq; i++) pos_of[mo.order[i]] = i;
    for (uint32_t i = 0; i < nq; i++) {
        P.label[i] = q.labels[mo.order[i]];
        P.degree[i] = q.degree(mo.order[i]);
        P.qv[i] = (uint8_t)mo.order[i];
        P.pivot[i] = (uint8_t)pos_of[mo.pivot[i]];
        P.back_off[i] = (uint16_t)mo.back_off[i];
    }
    P.back_off[nq] = (uint16_t)mo.back_off[nq];
    for (size_t j = 0; j < mo.back.size(); j++) P.back[j] = (uint8_t)pos_of[mo.back[j]];
    // the ordering constraints by position; a query without symmetry has none and runs the plain kernel
    Q->O = SetsOrder{};
    Q->n_pairs = distinct ? sets_order_from_pairs(gnnpe_host::query_symmetry(q).pairs, pos_of, trim, &Q->O) : 0u;
    // the non-edges by position: every earlier position but the pivot and the back neighbours; a query without one (1 or 2
    // vertices, K_n) runs the kernel it would run without the flag
    Q->N = SetsNon{};
    Q->n_non = 0;
    for (uint32_t d = 1; induced && d < nq; d++) {
        uint32_t m = ((1u << d) - 1u) & ~(1u << P.pivot[d]);
        for (uint32_t j = P.back_off[d]; j < P.back_off[d + 1]; j++) m &= ~(1u << P.back[j]);
        Q->N.non[d] = m;
        Q->n_non += (uint32_t)__builtin_popcount(m);
    }
    return pos_of;
}

// "The sets are already on the device": what a standing exact query (gnnpe_standing.hip) hands sets_prepare, sets_stage_items and
// delta_stage in the place of the query file and the host bitmap.  The query graph was parsed once; d_bitmap is the handle's own
// nq x words bitmap; sizes[u] = |C(u)| are on the host already (k_sets_sizes, read in a wait the handle had anyway); the start
// candidates are written on the device by k_sets_members.  With it the three skip the file, the host walk over the sets and the two
// uploads; the kernels read d_bitmap.  d_rows / rows_cap: the rows of the call stay on the device, in the handle's buffer, and
// rows_held says how many were written; nothing per match comes to the host.
struct SetsResident {
    const gnnpe_host::StaticGraph *query = nullptr;
    const uint32_t *d_bitmap = nullptr;
    const uint64_t *sizes = nullptr;
    uint32_t *d_rows = nullptr;
    uint64_t rows_cap = 0;
    uint64_t rows_held = 0;  // out
};

// (sets_members_launch, which writes the start candidates of a resident row: gnnpe_touched.hip.h)

// Everything between a call's own argument checks and the device: the state of the context, the query graph, the set sizes and the
// matching order -- a disconnected query is refused whatever the limit -- then the plan, the pairs and the start candidates.
// `query`, if given, receives the loaded query graph (gnnpe_refine_sets_delta builds its own orders from it).  With `res` the query
// graph and the set sizes are the handle's, Q->cand stays empty (sets_stage_items has the device write the candidates) and
// query_graph_path and bitmap are not read.
static inline int sets_prepare(const char *who, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *bitmap, uint32_t mode,
                               uint64_t limit, SetsQuery *Q, gnnpe_host::StaticGraph *query = nullptr, const SetsResident *res = nullptr)
{
    GNNPE_REQUIRE((mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) == 0, GNNPE_ERR_ARG, "%s: unknown mode bits 0x%x", who, mode);
    const bool distinct = (mode & GNNPE_MATCH_DISTINCT) != 0, induced = (mode & GNNPE_MATCH_INDUCED) != 0;
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    gnnpe_host::StaticGraph q_own;
    gnnpe_host::StaticGraph &q = query ? *query : q_own;
    std::string err;
    const int rc = res ? 0 : q.load(query_graph_path, &err);
    if (rc != 0) {
        set_error("%s", err.c_str());
        return rc;
    }
    if (res) q = *res->query;
    const uint32_t nq = Q->nq = q.n;
    GNNPE_REQUIRE(nq >= 1 && nq <= (uint32_t)kSetsMaxQ, GNNPE_ERR_UNSUPPORTED, "query graphs of 1..%d vertices (got %u)", kSetsMaxQ, nq);
    const uint64_t words = Q->words = ((uint64_t)c->n + 31) / 32;
    const std::vector<uint64_t> cnt = res ? std::vector<uint64_t>(res->sizes, res->sizes + nq) : gnnpe_host::set_sizes(bitmap, words, nq);
    gnnpe_host::MatchOrder mo;
    if (gnnpe_host::build_match_order(q, cnt, &mo, &err) != 0) {
        set_error("%s", err.c_str());
        return GNNPE_ERR_ARG;
    }
    Q->empty = limit == 0 || std::find(cnt.begin(), cnt.end(), 0u) != cnt.end();  // an empty set anywhere means no embedding
    if (Q->empty) return GNNPE_OK;
    sets_plan_from_order(q, mo, distinct, induced, c->sw.sets_trim, Q);
    if (!res) Q->cand = gnnpe_host::set_members(bitmap, words, mo.order[0], c->n);
    Q->n_cand = res ? (uint32_t)cnt[mo.order[0]] : (uint32_t)Q->cand.size();  // (a resident row has no bit at or above n)
    Q->empty = Q->n_cand == 0;
    return GNNPE_OK;
}

// the work buffer of a call or a cursor: [counters 32 B | item_off u32 x (n_cand + 1) | cand u32 x n_cand | chunks u32 x (n_cand + 1)]
struct SetsWork {
    void *ctr;
    uint32_t *item_off, *cand, *chunks;
    static constexpr size_t kCtrBytes = 32;
    static size_t bytes(uint32_t n_cand) { return kCtrBytes + ((size_t)n_cand * 3 + 2) * 4 + 64; }
    SetsWork(const DevBuf &b, uint32_t n_cand)
        : ctr(b.p), item_off(reinterpret_cast<uint32_t *>(b.as<char>() + kCtrBytes)), cand(item_off + n_cand + 1), chunks(cand + n_cand)
    {
    }
};
static_assert(sizeof(SetsCounters) == SetsWork::kCtrBytes, "the counters of the work buffer");

// a resident grid; a single-vertex query needs no more waves than it has items
static inline uint32_t sets_grid_blocks(const gnnpe_ctx *c, uint32_t nq, uint32_t n_cand)
{
    uint64_t blocks = (uint64_t)std::max(c->num_cus, 1) * kSetsBlocksPerCu;
    if (nq == 1) blocks = std::min<uint64_t>(blocks, ((uint64_t)(n_cand + 63) / 64 + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
    return (uint32_t)blocks;
}

// Puts a prepared query on the device, on the context's stream, in the buffers it is handed (the context's for the one-shot call,
// a cursor's own): the start candidates, the bitmap, zeroed counters, and for nq > 1 the offsets of the first-level items
// (k_sets_cand_chunks and a scan; item_off[n_cand] is their number).  Chooses Q->w_shift first.  `uploaded`, if given, is recorded
// between the copies and the kernels.  Waits for nothing.  With `res` nothing is uploaded: k_sets_members writes the start
// candidates from the resident row of the start vertex (P.qv[0]), and `bm` is neither reserved nor written.
static inline int sets_stage_items(gnnpe_ctx *c, SetsQuery *Q, const uint32_t *bitmap, DevBuf &work, DevBuf &bm, DevBuf &tmp,
                                   hipEvent_t uploaded = nullptr, const SetsResident *res = nullptr)
{
    // GNNPE_TESTING=sets_first_shift=K stands in for the heuristic; the 32-bit item offsets still come first
    Q->forced = c->sw.sets_first_shift >= 0 && c->nbr_used + c->n < (1ull << 32);
    Q->w_shift = Q->forced ? (uint32_t)c->sw.sets_first_shift : sets_first_level_shift(Q->n_cand, c->nbr_used, c->n, c->num_cus, c->n_hub);
    const uint32_t n_cand = Q->n_cand;
    const size_t bm_bytes = (size_t)Q->nq * Q->words * 4;
    int rc;
    if ((rc = work.reserve(SetsWork::bytes(n_cand))) || (!res && (rc = bm.reserve(bm_bytes)))) return rc;
    const SetsWork W(work, n_cand);
    if (res) {
        GNNPE_HIP_TRY(sets_members_launch(c->stream, res->d_bitmap + (uint64_t)Q->P.qv[0] * Q->words, Q->words, c->n, W.cand, n_cand, nullptr));
    } else {
        GNNPE_HIP_TRY(hipMemcpyAsync(W.cand, Q->cand.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, c->stream));
        GNNPE_HIP_TRY(hipMemcpyAsync(bm.p, bitmap, bm_bytes, hipMemcpyHostToDevice, c->stream));
    }
    GNNPE_HIP_TRY(hipMemsetAsync(W.ctr, 0, SetsWork::kCtrBytes, c->stream));
    if (uploaded) GNNPE_HIP_TRY(hipEventRecord(uploaded, c->stream));
    if (Q->nq == 1) return GNNPE_OK;
    hipLaunchKernelGGL(k_sets_cand_chunks, dim3((n_cand + 256) / 256), dim3(256), 0, c->stream, n_cand, W.cand, c->adj_deg.as<uint32_t>(),
                       Q->w_shift, W.chunks);
    size_t tb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, W.chunks, W.item_off, (int)(n_cand + 1), c->stream));
    if ((rc = tmp.reserve(tb))) return rc;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, W.chunks, W.item_off, (int)(n_cand + 1), c->stream));
    return GNNPE_OK;
}

// the instantiation a query runs: f(), f(Q.O), f(Q.N) or f(Q.O, Q.N), as its pairs and non-edges ask
template <class F>
static inline void sets_dispatch(const SetsQuery &Q, F &&f)
{
    if (Q.n_non)
        Q.n_pairs ? f(Q.O, Q.N) : f(Q.N);
    else
        Q.n_pairs ? f(Q.O) : f();
}

// A one-shot call from "arguments checked" to "rc returned": the two events of a timed call, the single wait, the error translation.
// Between the constructor and finish() the call stages (ev0 is recorded where its uploads end), launches and reads h_pinned; every
// such step runs only while ok(), and leaves its failure in rc (a code whose message is set) or he (a HIP error, translated at the
// end).
struct SetsCall {
    const char *who;
    gnnpe_ctx *c;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // null unless the call is timed
    hipError_t he = hipSuccess;
    int rc = GNNPE_OK;
    SetsCall(const char *who_, gnnpe_ctx *c_, bool timed) : who(who_), c(c_)
    {
        if (timed) he = hipEventCreate(&ev0);
        if (he == hipSuccess && timed) he = hipEventCreate(&ev1);
    }
    bool ok() const { return he == hipSuccess && !rc; }
    // the launches of f
    template <class F>
    void launch(F &&f)
    {
        if (!ok()) return;
        f();
        he = hipGetLastError();
    }
    // after the last launch: the end of the timed span, the first `bytes` of the counters to h_pinned, and the one wait of the call
    void wait(const void *ctr, size_t bytes)
    {
        if (ok() && ev1) he = hipEventRecord(ev1, c->stream);
        if (ok()) he = hipMemcpyAsync(c->h_pinned, ctr, bytes, hipMemcpyDeviceToHost, c->stream);
        if (ok()) he = hipStreamSynchronize(c->stream);
    }
    // the device time of a call that succeeded, and the call's return code
    int finish(double *device_ms)
    {
        if (ok() && device_ms) {
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
};

// What the two count calls (vertex table, edge table) do after sets_prepare with a table of `cells` uint64 reserved at d_counts
// (null if cells == 0).  An empty set or no start candidate: a zeroed table is the whole answer.  Otherwise the table is zeroed on
// the stream, launch(W, ord...) starts the kernel, and after the wait *complete = total < limit; the table comes back to
// host_counts only where it is asked for and means something.  With GNNPE_DEBUG staged() prints the call's line after the staging
// and done(finds, flush_adds) its line after the wait.  With `res` (a standing query that keeps its count tables) the sets are on
// the device already: nothing is uploaded, and launch() hands its kernel res->d_bitmap.
template <class Staged, class Launch, class Done>
static inline int sets_count_call(const char *who, gnnpe_ctx *c, SetsQuery *Q, const uint32_t *bitmap, uint64_t limit,
                                  unsigned long long *d_counts, size_t cells, uint64_t *answers, int *complete, uint64_t *host_counts,
                                  void **dev_counts, double *device_ms, Staged &&staged, Launch &&launch, Done &&done,
                                  const SetsResident *res = nullptr)
{
    const size_t table_bytes = cells * 8;
    if (dev_counts) *dev_counts = d_counts;
    if (Q->empty) {
        if (table_bytes) {
            GNNPE_HIP_TRY(hipMemsetAsync(d_counts, 0, table_bytes, c->stream));
            GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
            if (host_counts) std::fill(host_counts, host_counts + cells, 0ull);
        }
        *complete = 1;
        return GNNPE_OK;
    }
    SetsCall call(who, c, device_ms != nullptr);
    if (call.ok()) call.rc = sets_stage_items(c, Q, bitmap, c->q_work, c->q_bitmap, c->q_tmp, call.ev0, res);
    if (c->sw.debug) staged();
    if (call.ok() && table_bytes) call.he = hipMemsetAsync(d_counts, 0, table_bytes, c->stream);
    call.launch([&] {
        const SetsWork W(c->q_work, Q->n_cand);
        sets_dispatch(*Q, [&](auto... ord) { launch(W, ord...); });
    });
    call.wait(c->q_work.p, 16);
    if (call.ok()) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        *complete = c->h_pinned[0] < limit ? 1 : 0;
        if (c->sw.debug) done((unsigned long long)c->h_pinned[0], (unsigned long long)c->h_pinned[1]);
        if (host_counts && *complete && table_bytes) call.he = hipMemcpy(host_counts, d_counts, table_bytes, hipMemcpyDeviceToHost);
    }
    return call.finish(device_ms);
}

}  // namespace gnnpe
