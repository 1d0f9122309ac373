// gnnpe_refine_pages.hip.h -- what the two families of cursors share: the plain cursor over the whole match set (k_refine_pages,
// gnnpe_refine_pages.hip) and the cursors over the delta matches (gnnpe_refine_delta_pages.hip: the matches through a set of data
// edges, on a set of non-edges, through a set of data vertices).  On the device the suspend slot of a wave; on the host the cursor
// object, which gnnpe_refine_pages_next, _device_ptr, _info and _close (gnnpe_refine_pages.hip) serve whatever opened it.  And the
// loop of the delta cursors' kernels, delta_pages_run: the loop, leaf, suspend and resume of k_refine_pages with an anchored item
// decode, a charging test and a floor depth, and with the hand-over between the launches of one page (the text at the head of
// gnnpe_refine_delta_pages.hip).
#pragma once

#include <cstddef>

#include "gnnpe_refine_sets.hip.h"
#include "gnnpe_refine_delta.hip.h"

namespace gnnpe {

constexpr uint32_t kWaveWords = sizeof(SetsWave) / 4;  // 7 arrays of kSetsMaxQ words: word a * kSetsMaxQ + i belongs to depth i

struct PagesSlot {  // saved state of one wave
    uint32_t valid, depth, item;
    uint32_t anchor;  // a delta cursor: the launch (anchor index) that wrote the slot; the plain cursor leaves it alone
    uint32_t w[kWaveWords];  // the SetsWave words of depths 0 .. depth
};

// The counters of a delta cursor: this block, then one ticket word per launch (anchor).  Only `cursor` is zeroed before a page; the
// rest lives as long as the cursor.  `bad` lies where SetsCounters has it: k_delta_entries raises it during open.
struct DeltaPagesCounters {
    unsigned long long cursor;  // rows reserved in this page (may pass page_rows)
    uint32_t valid;             // slots that hold a state: a suspend adds one, a resume takes one
    uint32_t owner;             // the anchor of the launch that suspended last: every valid slot is its
    uint32_t mismatch;          // a wave met a slot of another anchor (never, by the hand-over's argument; the host refuses the page)
    uint32_t bad;               // k_delta_entries
    uint32_t pad[2];
};
static_assert(sizeof(DeltaPagesCounters) == SetsWork::kCtrBytes && offsetof(DeltaPagesCounters, bad) == offsetof(SetsCounters, bad),
              "k_delta_entries takes the block for a SetsCounters");

// One wave of a launch of a delta cursor.  `decode(q)` enters item q at depth kFloor (false: the item holds nothing), `test(d, v)`
// is the charging rule for a lane that passed sets_lane_test with candidate v at depth d.  kFloor is the depth the decode enters and
// the item ends below: 1 where the item fixes position 0, 2 where it fixes positions 0 and 1 (whose depth-1 words are never written
// and never read).  It is the kernel's constant, so a resumed wave has it back without a word in the slot.  kSingle: the kernel
// also serves a single-vertex query (an item is 64 start candidates of `cand`).
template <bool kOrdered, uint32_t kFloor, bool kSingle, class Decode, class Test, class... Ord>
__device__ __forceinline__ void delta_pages_run(const SetsPlan &P, volatile SetsWave &S, volatile uint32_t *Sw, const SetsGraph &G, uint32_t n_cand,
                                                const uint32_t *__restrict__ cand, uint32_t n_items, uint32_t anchor, DeltaPagesCounters *ctr,
                                                PagesSlot *slot, uint32_t *__restrict__ page, unsigned long long page_rows, Decode &&decode,
                                                Test &&test, const Ord &...ord)
{
    // the page is full (an earlier launch of this page filled it): away, before a slot or a ticket is touched
    if (__hip_atomic_load(&ctr->cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= page_rows) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nq = P.nq, last = nq - 1;
    uint32_t *ticket = reinterpret_cast<uint32_t *>(ctr + 1) + anchor;

    // as in k_refine_pages: reserve the survivors' rows, store the ones inside the page, return the ones past its end
    auto emit = [&](uint32_t d, unsigned long long m, uint32_t v) -> unsigned long long {
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(&ctr->cursor, (unsigned long long)__popcll(m));
        at = uni64(at) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        const bool mine = ((m >> lane) & 1ull) != 0;
        if (mine && at < page_rows) {
            uint32_t *row = page + at * nq;
            for (uint32_t i = 0; i < d; i++) row[P.qv[i]] = S.image[i];
            row[P.qv[d]] = v;
        }
        return __ballot(mine && at >= page_rows);
    };
    // as in k_refine_pages, and the slot is marked with the launch it belongs to
    auto suspend = [&](uint32_t d, uint32_t q) {
        if (lane == 0) {
#pragma unroll 1
            for (uint32_t a = 0; a < kWaveWords; a += (uint32_t)kSetsMaxQ)
#pragma unroll 1
                for (uint32_t i = 0; i <= d; i++) slot->w[a + i] = Sw[a + i];
            slot->depth = d;
            slot->item = q;
            slot->anchor = anchor;
            slot->valid = 1u;
            ctr->owner = anchor;
            atomicAdd(&ctr->valid, 1u);
        }
    };

    uint32_t q = 0, d = 0;
    bool resumed = uni(slot->valid) != 0;
    if (resumed) {
        if (uni(slot->anchor) != anchor) {
            if (lane == 0) atomicOr(&ctr->mismatch, 1u);
            return;
        }
        d = uni(slot->depth);
        q = uni(slot->item);
#pragma unroll 1
        for (uint32_t a = 0; a < kWaveWords; a += (uint32_t)kSetsMaxQ)
#pragma unroll 1
            for (uint32_t i = 0; i <= d; i++) Sw[a + i] = slot->w[a + i];
        if (lane == 0) {
            slot->valid = 0u;
            atomicSub(&ctr->valid, 1u);
        }
    }

    for (;; resumed = false) {
        if (!resumed) {
            if (__hip_atomic_load(&ctr->cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= page_rows) return;
            if (__hip_atomic_load(ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_items) return;
            if (lane == 0) q = atomicAdd(ticket, 1u);
            q = uni(q);
            if (q >= n_items) return;
        }

        if constexpr (kSingle) {
            if (nq == 1) {
                const uint32_t i = q * 64u + lane, v = sets_single_cand(n_cand, cand, i);
                unsigned long long m;
                if (resumed)
                    m = ((unsigned long long)uni(S.mask_hi[0]) << 32) | uni(S.mask_lo[0]);
                else
                    m = __ballot(sets_single_test(P, G, n_cand, i, v));
                if (m == 0) continue;
                m = emit(0, m, v);
                if (m) {
                    S.mask_lo[0] = (uint32_t)m;
                    S.mask_hi[0] = (uint32_t)(m >> 32);
                    suspend(0, q);
                    return;
                }
                continue;
            }
        }

        if (!resumed) {
            if (!decode(q)) continue;
            d = kFloor;
        }
        uint32_t steps = 0;
        while (d >= kFloor) {
            if ((++steps & 1023u) == 0 && __hip_atomic_load(&ctr->cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= page_rows) {
                suspend(d, q);
                return;
            }
            unsigned long long m = ((unsigned long long)uni(S.mask_hi[d]) << 32) | uni(S.mask_lo[d]);
            if (m == 0) {
                // next chunk of the pivot row (the edge item's depth 1: the one chunk [j, j + 1), then the end)
                const uint32_t cb = uni(S.cbase[d]) + 64u, ce = uni(S.end[d]);
                if ((int32_t)(ce - cb) <= 0) {
                    d--;
                    continue;
                }
                S.cbase[d] = cb;
                uint32_t v;
                const bool ok = sets_lane_test<kOrdered>(P, S, G, d, cb, ce, lane, v, ord...) && test(d, v);
                m = __ballot(ok);
                if (m == 0) continue;
                if (d == last) {
                    m = emit(d, m, v);
                    if (m) {
                        S.mask_lo[d] = (uint32_t)m;
                        S.mask_hi[d] = (uint32_t)(m >> 32);
                        suspend(d, q);
                        return;
                    }
                    continue;
                }
            } else if (d == last) {
                // (after a resume only) the survivors a full page left behind: their entries again, no test again
                const uint32_t v = ((m >> lane) & 1ull) ? G.nbrs[uni(S.cbase[d]) + lane] : 0u;
                m = emit(d, m, v);
                S.mask_lo[d] = (uint32_t)m;
                S.mask_hi[d] = (uint32_t)(m >> 32);
                if (m) {
                    suspend(d, q);
                    return;
                }
                continue;
            }
            sets_descend<kOrdered>(P, S, G, d, m, lane, ord...);
        }
    }
}

// one launch of a delta cursor: an anchor (query edge, non-adjacent query pair, or query vertex), its plan and its items
struct DeltaPagesLaunch {
    SetsQuery K;               // the plan and its packs (no candidates)
    SetsDelta older = {};      // edges, non-edges: the charging rule
    uint32_t earlier = 0;      // vertices: the charging rule
    uint32_t n_cand = 0, w_shift = 6, n_items = 0;
    size_t cand_at = 0, off_at = 0;  // vertices: where its candidates / item offsets begin in the cursor's work buffer
};

}  // namespace gnnpe

// A cursor owns everything its launches write or read besides the graph: cursors of any kind, the one-shot calls and the filters
// interleave freely on one context.
struct gnnpe_match_cursor {
    gnnpe_ctx *c = nullptr;
    uint64_t graph_gen = 0;  // the context's graph when the cursor was opened
    gnnpe::SetsQuery Q;      // (its host copy of the start candidates is dropped once they are on the device)
    uint32_t n_items = 0, blocks = 0;
    uint64_t limit = 0, page_rows = 0, page_cap = 0;  // page_cap: rows the page buffer holds, min(page_rows, limit)
    uint64_t delivered = 0, pages = 0;
    uint32_t suspended = 0, ticket = 0;  // of the last page
    bool done = false;
    gnnpe::DevBuf work, bitmap, slots, page, tmp;  // work: SetsWork (a vertices cursor: VerticesWork)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // a delta cursor (gnnpe_refine_delta_pages.hip)
    int anchor_kind = 0;  // 0: the plain cursor; 1 edges, 2 non-edges, 3 vertices
    std::vector<gnnpe::DeltaPagesLaunch> L;
    uint32_t first = 0;       // the first launch that is not finished
    uint64_t items_left = 0;  // first-level items not yet taken, of launch `first` and all later ones
    size_t n_keys = 0, n_cand_all = 0;
    gnnpe::DevBuf ctrs, fset;  // DeltaPagesCounters and the tickets; F as keys, pairs and entries, or S as a bitmap and ids
    uint32_t *h_ctrs = nullptr;  // pinned: the counters come here once per page
};

// gnnpe_refine_pages_next for a delta cursor, after its checks (gnnpe_refine_delta_pages.hip)
int gnnpe_delta_pages_next(gnnpe_match_cursor *cur, uint32_t *host_rows, uint64_t *n_rows, int *done, double *device_ms);
