// gnnpe_edges_below.hip -- gnnpe_csr_edges_below of include/gnnpe_hip.h: the undirected edges of the resident graph whose support in
// a per-entry count table lies below a threshold, as ascending (x, y) pairs, and the smallest support among the others.
//
// Who calls it: every round of gnnpe_standing_peel (csrc/gnnpe_standing.hip), with the table E a standing exact query keeps.  The
// support of the edge {x, y} is the sum over the table's rows of the cells of its two entries j = (x -> y) and r = (y -> x), mod 2^64.
// The table stays on the device: a round moves 8 bytes per selected edge to the host where the loop over gnnpe_standing_counts moved
// n_rows x entries cells.
//
// Shape: the two passes over fixed tiles of gnnpe_table_fold.hip -- no atomics, no block waits for another.
//   One lane per entry j: y = nbrs[j], r = adj_start[y] + revpos[j] (the context's reverse positions), x = nbrs[r].  The lane of the
//   direction x > y is idle; the lane with x < y reads the 2 x n_rows cells.  The cells at j stream, the cells at r are gathers of
//   8 bytes: the pass is bound by requests, not by bandwidth (profiles/online_standing_peel.txt).
//   1. k_below_count: per tile of kBelowTile entries the selected edges (a DPP wave sum, the four wave sums through LDS) and the
//      smallest support among the edges that are not selected (a DPP wave minimum on two dwords, four LDS words).
//   2. hipcub ExclusiveSum over the tile counts: tile_base[t] = selected edges in front of tile t, tile_base[tiles] = all of them;
//      hipcub Reduce (minimum) over the tile minima.  The two words are what the host waits for.
//   3. k_below_write: a tile whose count is 0 is left without a read of the graph or the table.  Otherwise the supports are computed
//      again and the selected lanes are ranked as k_fold_apply ranks its nonzero cells: by step, then wave, then lane, which is
//      ascending j; the pair (x, y) goes to tile_base[t] + rank if that is below cap.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) and the measurement: profiles/online_standing_peel.txt.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "gnnpe_common.h"
#include "gnnpe_dpp.hip.h"

namespace gnnpe {

constexpr uint32_t kBelowTile = 2048;  // entries per block and step (tests mirror it): kFoldTile's 8 per lane
constexpr uint32_t kBelowPerLane = kBelowTile / kBlock, kBelowWaves = kBlock / 64, kBelowSlots = kBelowPerLane * kBelowWaves;
constexpr uint32_t kBelowNoEdge = 0xFFFFFFFFu;  // k_revpos: the row of the other end is not held (never on a whole graph)
static_assert(kBelowSlots <= 64, "one wave scans the (step, wave) totals");

struct BelowGraph {
    const uint32_t *__restrict__ adj_start, *__restrict__ nbrs, *__restrict__ revpos;
    uint32_t entries;
};

__device__ __forceinline__ unsigned long long below_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v)
{
    const uint32_t lo = dpp_u32<CTRL, ROW_MASK>((uint32_t)v), hi = dpp_u32<CTRL, ROW_MASK>((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)  // a skipped row keeps its own value: the identity
{
    GNNPE_DPP_REDUCE(unsigned long long, dpp_u64, below_min)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// Entry j = (x -> y): false for the idle lanes (j outside the graph, x > y); otherwise x, y and the support of {x, y}.  Every index
// is below `entries` where it is used: r is checked before nbrs[r] and the table are read at it.
__device__ __forceinline__ bool below_support(const BelowGraph &G, const unsigned long long *__restrict__ table, uint32_t n_rows, uint64_t j,
                                              uint32_t *x, uint32_t *y, unsigned long long *sup)
{
    if (j >= G.entries) return false;
    const uint32_t yy = G.nbrs[j], rp = G.revpos[j];
    if (rp == kBelowNoEdge) return false;
    const uint64_t r = (uint64_t)G.adj_start[yy] + rp;
    if (r >= G.entries) return false;
    const uint32_t xx = G.nbrs[r];
    if (xx >= yy) return false;
    unsigned long long s = 0;
    for (uint32_t k = 0; k < n_rows; k++) {
        const unsigned long long *__restrict__ row = table + (uint64_t)k * G.entries;
        s += row[j] + row[r];
    }
    *x = xx, *y = yy, *sup = s;
    return true;
}

// tile_cnt[t] = the selected edges of tile t, tile_cnt[tiles] = 0 (the scan runs over tiles + 1 words); tile_min[t] = the smallest
// support of its edges that are not selected, 2^64 - 1 without one
static __global__ __launch_bounds__(kBlock) void k_below_count(BelowGraph G, uint64_t tiles, const unsigned long long *__restrict__ table, uint32_t n_rows,
                                                               unsigned long long threshold, unsigned long long *__restrict__ tile_cnt,
                                                               unsigned long long *__restrict__ tile_min)
{
    __shared__ uint32_t wsum[kBelowWaves];
    __shared__ unsigned long long wmin[kBelowWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_cnt[tiles] = 0ull;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t a = t * kBelowTile;
        uint32_t cnt = 0;
        unsigned long long mn = ~0ull;
#pragma unroll
        for (uint32_t i = 0; i < kBelowPerLane; i++) {
            uint32_t x, y;
            unsigned long long sup;
            if (!below_support(G, table, n_rows, a + i * kBlock + threadIdx.x, &x, &y, &sup)) continue;
            if (sup < threshold) cnt++;
            else mn = below_min(mn, sup);
        }
        const uint32_t sum = wave_sum_u32(cnt);
        const unsigned long long low = wave_min_u64(mn);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = sum, wmin[threadIdx.x >> 6] = low;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            unsigned long long m = ~0ull;
            for (uint32_t w = 0; w < kBelowWaves; w++) s += wsum[w], m = below_min(m, wmin[w]);
            tile_cnt[t] = s;
            tile_min[t] = m;
        }
        __syncthreads();
    }
}

// The select (the file's head, step 3).  No pair is stored at or behind `cap`.
static __global__ __launch_bounds__(kBlock) void k_below_write(BelowGraph G, uint64_t tiles, const unsigned long long *__restrict__ table, uint32_t n_rows,
                                                               unsigned long long threshold, const unsigned long long *__restrict__ tile_cnt,
                                                               const unsigned long long *__restrict__ tile_base, uint32_t *__restrict__ pairs,
                                                               unsigned long long cap)
{
    __shared__ uint32_t wcnt[kBelowSlots], wpre[kBelowSlots];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        if (tile_cnt[t] == 0ull) continue;  // (uniform) no edge of this tile is selected
        const uint64_t a = t * kBelowTile;
        const unsigned long long base = tile_base[t];
        if (base >= cap) continue;  // (uniform) every pair of the tile lies behind cap
        uint32_t x[kBelowPerLane], y[kBelowPerLane], rank[kBelowPerLane];
        bool sel[kBelowPerLane];
#pragma unroll
        for (uint32_t i = 0; i < kBelowPerLane; i++) {
            unsigned long long sup = 0;
            x[i] = y[i] = 0;
            sel[i] = below_support(G, table, n_rows, a + i * kBlock + threadIdx.x, &x[i], &y[i], &sup) && sup < threshold;
        }
#pragma unroll
        for (uint32_t i = 0; i < kBelowPerLane; i++) {
            const unsigned long long mask = __ballot(sel[i]);
            rank[i] = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[i * kBelowWaves + wave] = (uint32_t)__popcll(mask);
        }
        __syncthreads();
        if (wave == 0) {  // the entries run by step, then wave, then lane
            const uint32_t c = lane < kBelowSlots ? wcnt[lane] : 0u;
            const uint32_t incl = wave_scan_add(c);
            if (lane < kBelowSlots) wpre[lane] = incl - c;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kBelowPerLane; i++) {
            if (!sel[i]) continue;
            const unsigned long long o = base + wpre[i * kBelowWaves + wave] + rank[i];
            if (o < cap) {
                pairs[2 * o] = x[i];
                pairs[2 * o + 1] = y[i];
            }
        }
        __syncthreads();  // wcnt and wpre are written again in the next step
    }
}

struct BelowMin {
    __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a < b ? a : b; }
};

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_csr_edges_below(gnnpe_ctx *c, const void *dev_table, uint32_t n_rows, uint64_t threshold, void *dev_pairs, uint64_t cap,
                                     uint64_t *n_selected, uint64_t *min_kept, double *device_ms)
{
    const char *who = "gnnpe_csr_edges_below";
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && dev_table && n_selected && min_kept, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(cap == 0 || dev_pairs, GNNPE_ERR_ARG, "%s: cap %llu without dev_pairs", who, (unsigned long long)cap);
    GNNPE_REQUIRE(n_rows != 0, GNNPE_ERR_ARG, "%s: a table without rows", who);
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_ARG, "%s: the whole graph must be on the device (gnnpe_load_csr), not a slab", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_ARG, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    GNNPE_REQUIRE((uintptr_t)dev_table % 8 == 0, GNNPE_ERR_ARG, "%s: dev_table is not aligned to its 8-byte cells", who);
    GNNPE_REQUIRE(!dev_pairs || (uintptr_t)dev_pairs % 4 == 0, GNNPE_ERR_ARG, "%s: dev_pairs is not aligned to its 4-byte words", who);
    const uint64_t entries = c->nbr_used;
    // no more room than pairs can come out: every edge has two entries
    const uint64_t room = std::min(cap, entries / 2);
    {
        const uintptr_t t = (uintptr_t)dev_table, p = (uintptr_t)dev_pairs;
        const uint64_t tb = (uint64_t)n_rows * entries * 8, pb = room * 8;
        GNNPE_REQUIRE(!tb || !pb || t + tb <= p || p + pb <= t, GNNPE_ERR_ARG, "%s: dev_pairs and dev_table overlap", who);
    }
    *n_selected = 0;
    *min_kept = ~0ull;
    if (entries == 0) return GNNPE_OK;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint64_t tiles = (entries + kBelowTile - 1) / kBelowTile;
    // [tile_cnt, tiles + 1 | tile_base, tiles + 1 | tile_min, tiles | the minimum]
    int rc = c->below_tiles.reserve((size_t)(3 * tiles + 3) * 8);
    if (rc) return rc;
    unsigned long long *tile_cnt = c->below_tiles.as<unsigned long long>(), *tile_base = tile_cnt + tiles + 1, *tile_min = tile_base + tiles + 1,
                       *d_min = tile_min + tiles;
    size_t tb = 0, rb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, tile_cnt, tile_base, (int64_t)tiles + 1, c->stream));
    GNNPE_HIP_TRY(hipcub::DeviceReduce::Reduce(nullptr, rb, tile_min, d_min, (int64_t)tiles, BelowMin(), ~0ull, c->stream));
    if ((rc = c->cub_tmp.reserve(std::max<size_t>(std::max(tb, rb), 1)))) return rc;
    tb = rb = c->cub_tmp.bytes;
    struct Events {  // of a timed call
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Events()
        {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } E;
    if (device_ms) {
        GNNPE_HIP_TRY(hipEventCreate(&E.ev[0]));
        GNNPE_HIP_TRY(hipEventCreate(&E.ev[1]));
        GNNPE_HIP_TRY(hipEventRecord(E.ev[0], c->stream));
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)std::max(c->num_cus, 1) * 8);
    const BelowGraph G = {c->adj_start.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->revpos.as<uint32_t>(), (uint32_t)entries};
    const unsigned long long *table = static_cast<const unsigned long long *>(dev_table);
    hipLaunchKernelGGL(k_below_count, dim3(grid), dim3(kBlock), 0, c->stream, G, tiles, table, n_rows, (unsigned long long)threshold, tile_cnt, tile_min);
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tb, tile_cnt, tile_base, (int64_t)tiles + 1, c->stream));
    GNNPE_HIP_TRY(hipcub::DeviceReduce::Reduce(c->cub_tmp.p, rb, tile_min, d_min, (int64_t)tiles, BelowMin(), ~0ull, c->stream));
    if (room && threshold) {
        hipLaunchKernelGGL(k_below_write, dim3(grid), dim3(kBlock), 0, c->stream, G, tiles, table, n_rows, (unsigned long long)threshold, tile_cnt,
                           tile_base, static_cast<uint32_t *>(dev_pairs), (unsigned long long)room);
        GNNPE_HIP_TRY(hipGetLastError());
    }
    if (device_ms) GNNPE_HIP_TRY(hipEventRecord(E.ev[1], c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, tile_base + tiles, 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned + 1, d_min, 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait of the call
    *n_selected = c->h_pinned[0];
    *min_kept = c->h_pinned[1];
    if (device_ms) {
        float ms = 0.f;
        GNNPE_HIP_TRY(hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
        *device_ms = ms;
    }
    return GNNPE_OK;
}
