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
//     scratch; the plain instantiation is instruction for instruction the kernel it was (30 VGPRs).
// host/refine_sets.cpp is the host form.  The plan, the wave state and the first-level items are in gnnpe_refine_sets.hip.h, shared with
// the paged form of this search (gnnpe_refine_pages.hip).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/gnnpe_online.h"
#include "../host/graph_loader.h"
#include "../host/query_symmetry.h"
#include "../host/refine.h"
#include "gnnpe_common.h"
#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

struct SetsCounters {  // one 32-byte block, zeroed before every launch
    unsigned long long total, cursor;
    uint32_t ticket, pad[3];
};

// One kernel, two instantiations.  k_refine_sets<false> is the plain search: the parameter pack is empty, nothing below that is
// `if constexpr (kOrdered)` exists, and the code is instruction for instruction what it was before the ordered form existed.
// k_refine_sets<true, SetsOrder> is the ordered search (D(C, limit): one embedding per distinct subgraph): one more by-value
// argument, the bounds of SetsOrder in every chunk's test, and the long pivot rows trimmed to them.
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
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nq = P.nq, last = nq - 1;
    // a single-vertex query has one item per 64 start candidates; otherwise the scan's total
    const uint32_t n_items = nq == 1 ? (n_cand + 63u) / 64u : item_off[n_cand];
    bool rows_full = matches == nullptr;  // no row left to reserve

    for (;;) {
        if (__hip_atomic_load(&ctr->total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= limit) return;
        uint32_t q = 0;
        if (lane == 0) q = atomicAdd(&ctr->ticket, 1u);
        q = uni(q);
        if (q >= n_items) return;

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

        if (nq == 1) {
            const uint32_t i = q * 64u + lane;
            const uint32_t v = i < n_cand ? cand[i] : 0u;
            const bool ok = i < n_cand && labels[v] == P.label[0] && adj_deg[v] >= P.degree[0];
            leaf(0, ok, v);
        } else {
            // item -> (start candidate, chunk of its row): largest ci with item_off[ci] <= q
            uint32_t lo = 0, hi = n_cand;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (item_off[mid] <= q) lo = mid; else hi = mid;
            }
            lo = uni(lo);
            const uint32_t v0 = uni(cand[lo]);
            const uint32_t s0 = uni(adj_start[v0]), d0 = uni(adj_deg[v0]);
            if (uni(labels[v0]) == P.label[0] && d0 >= P.degree[0]) {
                S.image[0] = v0;
                S.istart[0] = s0;
                S.ideg[0] = d0;
                // depth 1 (its pivot is position 0) is held to this item's chunk
                const uint32_t c0 = s0 + ((q - uni(item_off[lo])) << w_shift);
                S.cbase[1] = c0 - 64u;
                S.end[1] = min(c0 + (1u << w_shift), s0 + d0);
                S.mask_lo[1] = 0;
                S.mask_hi[1] = 0;
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
                        const uint32_t idx = cb + lane;
                        bool ok = idx < ce;
                        const uint32_t v = ok ? nbrs[idx] : 0u;
                        const uint32_t word = bitmap[(uint64_t)P.qv[d] * words + (v >> 5)], lab = labels[v], dv = adj_deg[v];
                        ok = ok & (((word >> (v & 31u)) & 1u) != 0) & (lab == P.label[d]) & (dv >= P.degree[d]);
                        if constexpr (kOrdered) {
                            uint32_t lo, hi;
                            order_bounds(sets_order(ord...), S, d, lo, hi);
                            ok = ok & (v >= lo) & (v < hi);
                        }
                        for (uint32_t i = 0; i < d; i++) ok &= S.image[i] != v;
                        if (ok && P.back_off[d] < P.back_off[d + 1]) {
                            const uint32_t vs = adj_start[v];
                            for (uint32_t j = P.back_off[d]; j < P.back_off[d + 1] && ok; j++) {
                                const uint32_t b = P.back[j], w = S.image[b], ws = S.istart[b], dw = S.ideg[b];
                                ok = dv <= dw ? row_has(nbrs, vs, dv, w) : row_has(nbrs, ws, dw, v);
                            }
                        }
                        if (d == last) {
                            leaf(d, ok, v);
                            continue;
                        }
                        m = __ballot(ok);
                        if (m == 0) continue;
                    }
                    // descend into the next survivor of this chunk
                    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    S.mask_lo[d] = (uint32_t)m;
                    S.mask_hi[d] = (uint32_t)(m >> 32);
                    const uint32_t v = uni(nbrs[uni(S.cbase[d]) + bit]);
                    S.image[d] = v;
                    S.istart[d] = uni(adj_start[v]);
                    S.ideg[d] = uni(adj_deg[v]);
                    d++;
                    const uint32_t p = P.pivot[d], ps = uni(S.istart[p]);
                    if constexpr (kOrdered) {
                        uint32_t rb = ps, re = ps + uni(S.ideg[p]);
                        if (sets_order(ord...).trim) {
                            uint32_t lo, hi;
                            order_bounds(sets_order(ord...), S, d, lo, hi);
                            order_trim(nbrs, lo, hi, lane, rb, re);
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
            }
        }
        if (pending && lane == 0) atomicAdd(&ctr->total, pending);
        if (stop) return;
    }
}

}  // namespace gnnpe

using namespace gnnpe;

// gnnpe_refine_sets (distinct = false: R) and gnnpe_refine_sets_distinct (D: the ordered kernel, unless the query has no symmetry)
static int refine_sets_run(const char *who, bool distinct, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                           uint64_t limit, uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    GNNPE_REQUIRE(c && query_graph_path && candidate_bitmap && answers, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    *answers = 0;
    if (device_ms) *device_ms = 0.0;
    gnnpe_host::StaticGraph q;
    std::string err;
    int rc = q.load(query_graph_path, &err);
    if (rc != 0) {
        set_error("%s", err.c_str());
        return rc;
    }
    const uint32_t nq = q.n;
    GNNPE_REQUIRE(nq >= 1 && nq <= (uint32_t)kSetsMaxQ, GNNPE_ERR_UNSUPPORTED, "query graphs of 1..%d vertices (got %u)", kSetsMaxQ, nq);
    const uint64_t words = ((uint64_t)c->n + 31) / 32;
    std::vector<uint64_t> cnt(nq, 0);
    for (uint32_t u = 0; u < nq; u++)
        for (uint64_t w = 0; w < words; w++) cnt[u] += (uint64_t)__builtin_popcount(candidate_bitmap[(size_t)u * words + w]);
    gnnpe_host::MatchOrder mo;
    if (gnnpe_host::build_match_order(q, cnt, &mo, &err) != 0) {
        set_error("%s", err.c_str());
        return GNNPE_ERR_ARG;
    }
    if (limit == 0) return GNNPE_OK;
    if (!matches) matches_cap = 0;
    matches_cap = std::min(matches_cap, limit);
    // plan by position in the order
    SetsPlan P = {};
    P.nq = nq;
    std::vector<uint32_t> pos_of(nq, 0);
    for (uint32_t i = 0; i < nq; i++) pos_of[mo.order[i]] = i;
    GNNPE_REQUIRE(mo.back.size() <= sizeof(P.back), GNNPE_ERR_UNSUPPORTED, "query graph too dense");
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
    SetsOrder O = {};
    const uint32_t n_pairs = distinct ? sets_order_from_pairs(gnnpe_host::query_symmetry(q).pairs, pos_of, c->sw.sets_trim, &O) : 0u;
    // start candidates; an empty set anywhere means no embedding
    for (uint32_t u = 0; u < nq; u++)
        if (cnt[u] == 0) return GNNPE_OK;
    const uint32_t start = mo.order[0];
    std::vector<uint32_t> cand;
    cand.reserve(cnt[start]);
    for (uint64_t w = 0; w < words; w++)
        for (uint32_t bits = candidate_bitmap[(size_t)start * words + w]; bits; bits &= bits - 1) {
            const uint64_t v = w * 32 + __builtin_ctz(bits);
            if (v < c->n) cand.push_back((uint32_t)v);
        }
    const uint32_t n_cand = (uint32_t)cand.size();
    if (n_cand == 0) return GNNPE_OK;

    // context-owned, grow-only: [counters 32 B | item_off u32 x (n_cand + 1) | cand u32 x n_cand | chunks u32 x (n_cand + 1)],
    // the bitmap, the rows
    const size_t bm_bytes = (size_t)nq * words * 4;
    if ((rc = c->q_work.reserve(sizeof(SetsCounters) + ((size_t)n_cand * 3 + 2) * 4 + 64)) || (rc = c->q_bitmap.reserve(bm_bytes)) ||
        (matches_cap && (rc = c->q_matches.reserve((size_t)matches_cap * nq * 4))))
        return rc;
    SetsCounters *d_ctr = c->q_work.as<SetsCounters>();
    uint32_t *item_off = reinterpret_cast<uint32_t *>(d_ctr + 1), *d_cand = item_off + n_cand + 1, *d_chunks = d_cand + n_cand;
    uint32_t *d_bm = c->q_bitmap.as<uint32_t>(), *d_rows = matches_cap ? c->q_matches.as<uint32_t>() : nullptr;
    hipError_t he = hipMemcpyAsync(d_cand, cand.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_bm, candidate_bitmap, bm_bytes, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemsetAsync(d_ctr, 0, sizeof(SetsCounters), c->stream);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev0);
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev1);
    if (he == hipSuccess && device_ms) he = hipEventRecord(ev0, c->stream);
    // GNNPE_TESTING=sets_first_shift=K stands in for the heuristic; the 32-bit item offsets still come first
    const bool forced = c->sw.sets_first_shift >= 0 && c->nbr_used + c->n < (1ull << 32);
    const uint32_t w_shift = forced ? (uint32_t)c->sw.sets_first_shift
                                    : sets_first_level_shift(n_cand, c->nbr_used, c->n, c->num_cus, c->n_hub);
    if (c->sw.debug && distinct)
        fprintf(stderr, "[refine_sets] shift=%u forced=%d cands=%u hubs=%u cus=%d pairs=%u\n", w_shift, (int)forced, n_cand, c->n_hub,
                c->num_cus, n_pairs);
    else if (c->sw.debug)
        fprintf(stderr, "[refine_sets] shift=%u forced=%d cands=%u hubs=%u cus=%d\n", w_shift, (int)forced, n_cand, c->n_hub, c->num_cus);
    if (he == hipSuccess && nq > 1) {
        hipLaunchKernelGGL(k_sets_cand_chunks, dim3((n_cand + 256) / 256), dim3(256), 0, c->stream, n_cand, d_cand,
                           c->adj_deg.as<uint32_t>(), w_shift, d_chunks);
        size_t tb = 0;
        he = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_chunks, item_off, (int)(n_cand + 1), c->stream);
        if (he == hipSuccess && (rc = c->q_tmp.reserve(tb)) == 0)
            he = hipcub::DeviceScan::ExclusiveSum(c->q_tmp.p, tb, d_chunks, item_off, (int)(n_cand + 1), c->stream);
    }
    if (he == hipSuccess && !rc) {
        // a resident grid; a single-vertex query needs no more waves than it has items
        uint64_t blocks = (uint64_t)std::max(c->num_cus, 1) * kSetsBlocksPerCu;
        if (nq == 1) blocks = std::min<uint64_t>(blocks, ((uint64_t)(n_cand + 63) / 64 + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
        if (n_pairs)
            hipLaunchKernelGGL((k_refine_sets<true, SetsOrder>), dim3((uint32_t)blocks), dim3(kBlock), 0, c->stream, P, n_cand, d_cand, item_off,
                               w_shift, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(),
                               c->labels.as<uint32_t>(), d_bm, words, (unsigned long long)limit, d_ctr, d_rows,
                               (unsigned long long)matches_cap, O);
        else
            hipLaunchKernelGGL((k_refine_sets<false>), dim3((uint32_t)blocks), dim3(kBlock), 0, c->stream, P, n_cand, d_cand, item_off, w_shift,
                               c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(),
                               c->labels.as<uint32_t>(), d_bm, words, (unsigned long long)limit, d_ctr, d_rows,
                               (unsigned long long)matches_cap);
        he = hipGetLastError();
    }
    if (he == hipSuccess && !rc && device_ms) he = hipEventRecord(ev1, c->stream);
    if (he == hipSuccess && !rc) he = hipMemcpyAsync(c->h_pinned, d_ctr, 16, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess && !rc) he = hipStreamSynchronize(c->stream);  // the one wait of a counting call
    if (he == hipSuccess && !rc) {
        *answers = std::min<uint64_t>(c->h_pinned[0], limit);
        // every find reserved a row, so the first min(cursor, cap) rows are written
        const uint64_t n_rows = std::min<uint64_t>(c->h_pinned[1], matches_cap);
        if (n_rows) he = hipMemcpy(matches, d_rows, (size_t)n_rows * nq * 4, hipMemcpyDeviceToHost);
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

extern "C" {

int gnnpe_refine_sets(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                      uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_sets_run("gnnpe_refine_sets", false, c, query_graph_path, candidate_bitmap, limit, answers, matches, matches_cap,
                           device_ms);
}

int gnnpe_refine_sets_distinct(gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                               uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms)
{
    return refine_sets_run("gnnpe_refine_sets_distinct", true, c, query_graph_path, candidate_bitmap, limit, answers, matches,
                           matches_cap, device_ms);
}

}  // extern "C"
