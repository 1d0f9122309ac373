// gnnpe_refine_sets.hip.h -- what the two set-restricted wave searches share: the one-shot k_refine_sets (gnnpe_refine_sets.hip)
// and the paged k_refine_pages (gnnpe_refine_pages.hip).  On the device the plan by position in the matching order, the
// per-wave search state in LDS and every STEP of the search: a chunk's lane test, the descent into a survivor, the decode of a
// first-level item, the single-vertex item.  Each kernel keeps its own loop, leaf and polling.  On the host the preparation
// of a query (sets_prepare) and the staging of its first-level items on the device (sets_stage_items).
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
// Both kernels build a SetsGraph from their own parameters and keep the conventions of the state: S is read and written through
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

// ---- the host's side of both calls -----------------------------------------------------------------------------------------
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

// Everything between a call's own argument checks and the device: the state of the context, the query graph, the set sizes and the
// matching order -- a disconnected query is refused whatever the limit -- then the plan, the pairs and the start candidates.
// `query`, if given, receives the loaded query graph (gnnpe_refine_sets_delta builds its own orders from it).
static inline int sets_prepare(const char *who, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *bitmap, uint32_t mode,
                               uint64_t limit, SetsQuery *Q, gnnpe_host::StaticGraph *query = nullptr)
{
    GNNPE_REQUIRE((mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) == 0, GNNPE_ERR_ARG, "%s: unknown mode bits 0x%x", who, mode);
    const bool distinct = (mode & GNNPE_MATCH_DISTINCT) != 0, induced = (mode & GNNPE_MATCH_INDUCED) != 0;
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    gnnpe_host::StaticGraph q_own;
    gnnpe_host::StaticGraph &q = query ? *query : q_own;
    std::string err;
    const int rc = q.load(query_graph_path, &err);
    if (rc != 0) {
        set_error("%s", err.c_str());
        return rc;
    }
    const uint32_t nq = Q->nq = q.n;
    GNNPE_REQUIRE(nq >= 1 && nq <= (uint32_t)kSetsMaxQ, GNNPE_ERR_UNSUPPORTED, "query graphs of 1..%d vertices (got %u)", kSetsMaxQ, nq);
    const uint64_t words = Q->words = ((uint64_t)c->n + 31) / 32;
    const std::vector<uint64_t> cnt = gnnpe_host::set_sizes(bitmap, words, nq);
    gnnpe_host::MatchOrder mo;
    if (gnnpe_host::build_match_order(q, cnt, &mo, &err) != 0) {
        set_error("%s", err.c_str());
        return GNNPE_ERR_ARG;
    }
    Q->empty = limit == 0 || std::find(cnt.begin(), cnt.end(), 0u) != cnt.end();  // an empty set anywhere means no embedding
    if (Q->empty) return GNNPE_OK;
    sets_plan_from_order(q, mo, distinct, induced, c->sw.sets_trim, Q);
    Q->cand = gnnpe_host::set_members(bitmap, words, mo.order[0], c->n);
    Q->n_cand = (uint32_t)Q->cand.size();
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
// between the copies and the kernels.  Waits for nothing.
static inline int sets_stage_items(gnnpe_ctx *c, SetsQuery *Q, const uint32_t *bitmap, DevBuf &work, DevBuf &bm, DevBuf &tmp,
                                   hipEvent_t uploaded = nullptr)
{
    // GNNPE_TESTING=sets_first_shift=K stands in for the heuristic; the 32-bit item offsets still come first
    Q->forced = c->sw.sets_first_shift >= 0 && c->nbr_used + c->n < (1ull << 32);
    Q->w_shift = Q->forced ? (uint32_t)c->sw.sets_first_shift : sets_first_level_shift(Q->n_cand, c->nbr_used, c->n, c->num_cus, c->n_hub);
    const uint32_t n_cand = Q->n_cand;
    const size_t bm_bytes = (size_t)Q->nq * Q->words * 4;
    int rc;
    if ((rc = work.reserve(SetsWork::bytes(n_cand))) || (rc = bm.reserve(bm_bytes))) return rc;
    const SetsWork W(work, n_cand);
    GNNPE_HIP_TRY(hipMemcpyAsync(W.cand, Q->cand.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(bm.p, bitmap, bm_bytes, hipMemcpyHostToDevice, c->stream));
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

}  // namespace gnnpe
