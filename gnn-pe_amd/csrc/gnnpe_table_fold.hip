// gnnpe_table_fold.hip -- gnnpe_table_fold of include/gnnpe_hip.h: table += delta, delta = 0, and the list of the cells that changed,
// in one pass over the scratch table.
//
// Who calls it: a standing exact query that keeps its count tables (csrc/gnnpe_standing.hip).  The delta count kernels of a batch add
// into a scratch table D of the table's size, the fold moves D into the table T at the end of the batch.  Why a scratch table and
// not T itself: the zeroing of D happens here, so no batch pays a memset of nq x n cells; a refused batch is rolled back by one
// memset of D while T was never touched; and the cells a batch changed -- with created and destroyed parts that cancel left out --
// come out of the same pass, where a consumer of T alone would have to compare nq x n cells on the host.
//
// Shape: the two passes over fixed tiles of gnnpe_update_vertices.hip, not a decoupled look-back -- no block waits for another.
//   1. k_fold_count: the nonzero cells of D per tile of kFoldTile cells (a DPP wave sum, the four wave sums through LDS).
//   2. hipcub ExclusiveSum over the tile counts (64-bit: a table can hold more than 2^32 cells): tile_base[t] = changed cells in
//      front of tile t, tile_base[tiles] = all of them, which is the one word the host waits for.
//   3. k_fold_apply: a tile whose count is 0 is left without a read of T or D -- after a small batch that is almost every tile, and
//      the pass then reads the tile counts only.  Otherwise the cells of the tile run by step, then wave, then lane (consecutive
//      lanes on consecutive cells, 8 bytes per lane, kFoldPerLane steps): the rank of a nonzero cell inside its (step, wave) is the
//      popcount of the ballot below its lane, the 32 (step, wave) totals go through LDS and one wave turns them into their
//      exclusive prefix with wave_scan_add; then T[j] += D[j], the pair (j, D[j]) goes to tile_base[t] + rank if that is below cap,
//      and D[j] = 0.  Every cell is owned by one lane: no atomics.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) and the measurement: profiles/online_standing_counts.txt.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "gnnpe_common.h"
#include "gnnpe_dpp.hip.h"

namespace gnnpe {

constexpr uint32_t kFoldTile = 2048;  // cells per block and step (tests mirror it), chosen as kVertTile was: 8 cells per lane
constexpr uint32_t kFoldPerLane = kFoldTile / kBlock, kFoldWaves = kBlock / 64, kFoldSlots = kFoldPerLane * kFoldWaves;
static_assert(kFoldSlots <= 64, "one wave scans the (step, wave) totals");

// tile_cnt[t] = the nonzero cells of tile t; tile_cnt[tiles] = 0 (the scan runs over tiles + 1 words)
static __global__ __launch_bounds__(kBlock) void k_fold_count(uint64_t cells, uint64_t tiles, const unsigned long long *__restrict__ delta,
                                                              unsigned long long *__restrict__ tile_cnt)
{
    __shared__ uint32_t wsum[kFoldWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_cnt[tiles] = 0ull;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t a = t * kFoldTile;
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t i = 0; i < kFoldPerLane; i++) {
            const uint64_t j = a + i * kBlock + threadIdx.x;
            cnt += j < cells && delta[j] != 0ull;
        }
        const uint32_t sum = wave_sum_u32(cnt);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < kFoldWaves; w++) s += wsum[w];
            tile_cnt[t] = s;
        }
        __syncthreads();
    }
}

// The fold (the file's head, step 3).  No pair is stored at or behind `cap`; a cell index is below `cells` wherever it is used.
static __global__ __launch_bounds__(kBlock) void k_fold_apply(uint64_t cells, uint64_t tiles, unsigned long long *__restrict__ table,
                                                              unsigned long long *__restrict__ delta,
                                                              const unsigned long long *__restrict__ tile_cnt,
                                                              const unsigned long long *__restrict__ tile_base,
                                                              unsigned long long *__restrict__ out_cells, long long *__restrict__ out_deltas,
                                                              unsigned long long cap)
{
    __shared__ uint32_t wcnt[kFoldSlots], wpre[kFoldSlots];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        if (tile_cnt[t] == 0ull) continue;  // (uniform) nothing of this tile changed
        const uint64_t a = t * kFoldTile;
        const unsigned long long base = tile_base[t];
        unsigned long long d[kFoldPerLane];
        uint32_t rank[kFoldPerLane];
#pragma unroll
        for (uint32_t i = 0; i < kFoldPerLane; i++) {
            const uint64_t j = a + i * kBlock + threadIdx.x;
            d[i] = j < cells ? delta[j] : 0ull;
        }
#pragma unroll
        for (uint32_t i = 0; i < kFoldPerLane; i++) {
            const unsigned long long mask = __ballot(d[i] != 0ull);
            rank[i] = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[i * kFoldWaves + wave] = (uint32_t)__popcll(mask);
        }
        __syncthreads();
        if (wave == 0) {  // the cells run by step, then wave, then lane
            const uint32_t c = lane < kFoldSlots ? wcnt[lane] : 0u;
            const uint32_t incl = wave_scan_add(c);
            if (lane < kFoldSlots) wpre[lane] = incl - c;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kFoldPerLane; i++) {
            if (d[i] == 0ull) continue;
            const uint64_t j = a + i * kBlock + threadIdx.x;  // below cells: a cell outside the table read as 0
            table[j] += d[i];
            delta[j] = 0ull;
            const unsigned long long o = base + wpre[i * kFoldWaves + wave] + rank[i];
            if (o < cap) {
                out_cells[o] = j;
                out_deltas[o] = (long long)d[i];
            }
        }
        __syncthreads();  // wcnt and wpre are written again in the next step
    }
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_table_fold(gnnpe_ctx *c, void *dev_table, void *dev_delta, uint64_t cells, void *dev_change_cells, void *dev_change_deltas,
                                uint64_t cap, uint64_t *n_changes, double *device_ms)
{
    const char *who = "gnnpe_table_fold";
    if (n_changes) *n_changes = 0;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && n_changes, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(cap == 0 || (dev_change_cells && dev_change_deltas), GNNPE_ERR_ARG, "%s: cap %llu without the change arrays", who,
                  (unsigned long long)cap);
    if (cells == 0) return GNNPE_OK;
    GNNPE_REQUIRE(dev_table && dev_delta, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(cells <= (1ull << 56) && cap <= (1ull << 56), GNNPE_ERR_ARG, "%s: %llu cells, cap %llu", who, (unsigned long long)cells,
                  (unsigned long long)cap);
    // no more room than pairs can come out
    const uint64_t room = std::min(cap, cells);
    const struct {
        const void *p;
        uint64_t bytes;
        const char *name;
    } R[4] = {{dev_table, cells * 8, "dev_table"}, {dev_delta, cells * 8, "dev_delta"}, {dev_change_cells, room * 8, "dev_change_cells"},
              {dev_change_deltas, room * 8, "dev_change_deltas"}};
    for (int i = 0; i < 4; i++) {
        if (!R[i].bytes) continue;
        GNNPE_REQUIRE((uintptr_t)R[i].p % 8 == 0, GNNPE_ERR_ARG, "%s: %s is not aligned to its 8-byte cells", who, R[i].name);
        for (int k = 0; k < i; k++) {
            if (!R[k].bytes) continue;
            const uintptr_t x = (uintptr_t)R[i].p, y = (uintptr_t)R[k].p;
            GNNPE_REQUIRE(x + R[i].bytes <= y || y + R[k].bytes <= x, GNNPE_ERR_ARG, "%s: %s and %s overlap", who, R[k].name, R[i].name);
        }
    }
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint64_t tiles = (cells + kFoldTile - 1) / kFoldTile;
    int rc = c->fold_tiles.reserve((size_t)(tiles + 1) * 16);
    if (rc) return rc;
    unsigned long long *tile_cnt = c->fold_tiles.as<unsigned long long>(), *tile_base = tile_cnt + tiles + 1;
    size_t tb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, tile_cnt, tile_base, (int64_t)tiles + 1, c->stream));
    if ((rc = c->cub_tmp.reserve(std::max<size_t>(tb, 1)))) return rc;
    tb = c->cub_tmp.bytes;
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
    unsigned long long *table = static_cast<unsigned long long *>(dev_table), *delta = static_cast<unsigned long long *>(dev_delta);
    hipLaunchKernelGGL(k_fold_count, dim3(grid), dim3(kBlock), 0, c->stream, cells, tiles, delta, tile_cnt);
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tb, tile_cnt, tile_base, (int64_t)tiles + 1, c->stream));
    hipLaunchKernelGGL(k_fold_apply, dim3(grid), dim3(kBlock), 0, c->stream, cells, tiles, table, delta, tile_cnt, tile_base,
                       static_cast<unsigned long long *>(dev_change_cells), static_cast<long long *>(dev_change_deltas),
                       (unsigned long long)room);
    GNNPE_HIP_TRY(hipGetLastError());
    if (device_ms) GNNPE_HIP_TRY(hipEventRecord(E.ev[1], c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, tile_base + tiles, 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait of the call
    *n_changes = c->h_pinned[0];
    if (device_ms) {
        float ms = 0.f;
        GNNPE_HIP_TRY(hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
        *device_ms = ms;
    }
    return GNNPE_OK;
}
