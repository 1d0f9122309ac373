// gnnpe_update_vertices.hip -- A BATCH OF VERTEX REMOVALS AND ADDITIONS APPLIED TO THE RESIDENT GRAPH: gnnpe_csr_apply_vertices of
// include/gnnpe_hip.h.  (gnnpe_csr_carry_vertices, the gather of a per-vertex table through the vertex map this call leaves, is
// k_carry_entries of gnnpe_update.hip under another stride and lives there.)
//
// Survivors keep their order and rows keep their inner order, so the new neighbour array is the stream compaction of the old one
// over "both ends survive" with every kept word mapped through the new id, and the new start of a surviving row is the number of
// kept entries in front of its old start.  Everything runs on the context's stream from the few words of the batch, with one wait
// before the decision:
//
//   1. the host checks the ids, sorts and de-duplicates R and uploads R and the labels of A.  n' is known here;
//   2. k_vert_mark, one wave per removed vertex, lanes over its row: the vertex' bit in a bitmap of ceil(n / 32) words (atomicOr:
//      two removed vertices may share a word), a byte flag on each of its entries and, through revpos, on the mirrored entry in the
//      neighbour's row (the access pattern of k_set_labels; plain byte stores: two removed neighbours mark different bytes, and
//      both ends of a removed edge store the same 1).  The work is the sum of the removed degrees, not a test of every entry;
//   3. hipcub ExclusiveSum over the popcounts of the bitmap words: below[w] = removed vertices in front of word w.  The new id of a
//      vertex is v - below[v >> 5] - popc(bits[v >> 5] & lower bits): two tables of n / 8 bytes each under the random lookups of
//      the compaction, where a table of new ids would be 4 n bytes;
//   4. the kept-prefix by TWO passes over fixed tiles of kVertTile old entries, not by a decoupled look-back: k_vert_tile_counts
//      counts the kept entries of every tile from the flags alone (one byte per entry, an eighth of the compaction's traffic),
//      hipcub ExclusiveSum turns the counts into tile bases, and no block ever waits for another -- a spin on a neighbour's status
//      word is the one way such a pass can hang, and a byte of flags per entry is what avoiding it costs;
//   5. k_vert_compact<kMap>, one block per tile and step: word and flag of kVertPerLane consecutive-dword loads per lane, the rank
//      of a kept entry from wave ballots and a 32-word LDS scan, new_nbrs[base + rank] = newid(word) and, under kMap, the entry
//      map's word (the old index) at the same position.  The block then takes the rows whose old start lies in its tile (two
//      wave-uniform binary searches in the old starts) and stores new_start[newid(x)] = base + kept entries of the tile in front of
//      the old start, read from the LDS prefix the ranks came from;
//   6. k_vert_map (a lane per old vertex: vertex_map[newid(v)] = v) and k_vert_tail (a lane per new vertex: the degree as the
//      difference of two starts, the label gathered through the vertex map; the added vertices get the constant tail -- start =
//      entries', degree 0, their label, GNNPE_NO_VERTEX in the map);
//   7. the wait: entries' and the number of removed bits come back.  GNNPE_ERR_RANGE is decided here from the exact entries', with
//      nothing but spare buffers written.  Otherwise start / degree / neighbour / label / presence arrays are swapped with the
//      spare ones and the tail of gnnpe_load_csr runs as gnnpe_csr_apply_edges runs it.
//
// The floor is one read of the old neighbour array and its flags plus one write of the new array (and of the map where wanted).
// No LDS beyond the tile's prefix (4 KB), no scratch, vector memory operations only.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "gnnpe_common.h"
#include "gnnpe_update.hip.h"

namespace gnnpe {

constexpr uint32_t kVertTile = 2048;  // old entries per block and step (tests mirror it)
constexpr uint32_t kVertPerLane = kVertTile / kBlock, kVertWaves = kBlock / 64;

struct PopcountOp {
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (uint32_t)__builtin_popcount(w); }
};

__device__ __forceinline__ bool vert_removed(const uint32_t *__restrict__ bits, uint32_t v) { return (bits[v >> 5] >> (v & 31u)) & 1u; }

// the id of a surviving vertex in G'
__device__ __forceinline__ uint32_t vert_new_id(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ below, uint32_t v)
{
    const uint32_t w = v >> 5;
    return v - below[w] - (uint32_t)__popc(bits[w] & ((1u << (v & 31u)) - 1u));
}

// first x in [0, n) with start[x] >= key (the old starts ascend: the rows of a whole graph lie back to back)
__device__ __forceinline__ uint32_t start_lower_bound(const uint32_t *__restrict__ start, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (start[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per removed vertex (each listed once, ids below n).  A reverse position outside the neighbour's row (an entry without
// its mirror) is skipped: no store leaves the row it belongs to, and every row lies inside the flag array.
static __global__ __launch_bounds__(kBlock) void k_vert_mark(uint32_t count, const uint32_t *__restrict__ verts, const uint32_t *__restrict__ adj_start,
                                                             const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                             const uint32_t *__restrict__ revpos, uint32_t *__restrict__ bits, uint8_t *__restrict__ flag)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * kVertWaves;
    for (uint32_t t = blockIdx.x * kVertWaves + (threadIdx.x >> 6); t < count; t += waves) {
        const uint32_t v = verts[t];
        const uint32_t st = adj_start[v], d = adj_deg[v];
        if (lane == 0) atomicOr(&bits[v >> 5], 1u << (v & 31u));
        for (uint32_t i = lane; i < d; i += 64) {
            const uint32_t u = nbrs[st + i], r = revpos[st + i];
            flag[st + i] = 1;
            if (r < adj_deg[u]) flag[adj_start[u] + r] = 1;
        }
    }
}

// kept entries of every tile
static __global__ __launch_bounds__(kBlock) void k_vert_tile_counts(uint32_t entries, uint32_t tiles, const uint8_t *__restrict__ flag,
                                                                    uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t wsum[kVertWaves];
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t a = (uint64_t)t * kVertTile;
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t i = 0; i < kVertPerLane; i++) {
            const uint64_t j = a + i * kBlock + threadIdx.x;
            cnt += j < entries && flag[j] == 0;
        }
        for (uint32_t off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < kVertWaves; w++) s += wsum[w];
            tile_cnt[t] = s;
        }
        __syncthreads();
    }
}

// The compaction (the file's head, step 5).  tile_base[t]: kept entries in front of tile t.  kMap: every store of a neighbour word
// also stores the entry map's word for the same new entry, under the same guard.  A store index is checked against the size of the
// array it goes to (the new arrays have at most `entries` words and n_after starts) whatever the tables say.
template <bool kMap>
__global__ __launch_bounds__(kBlock) void k_vert_compact(uint32_t n, uint32_t entries, uint32_t tiles, uint32_t n_surv,
                                                        const uint32_t *__restrict__ adj_start, const uint32_t *__restrict__ nbrs,
                                                        const uint8_t *__restrict__ flag, const uint32_t *__restrict__ bits,
                                                        const uint32_t *__restrict__ below, const uint32_t *__restrict__ tile_base,
                                                        uint32_t *__restrict__ new_start, uint32_t *__restrict__ new_nbrs, uint32_t *__restrict__ map)
{
    __shared__ uint16_t pre[kVertTile + 1];  // kept entries of the tile in front of entry a + i; [kVertTile]: all of them
    __shared__ uint32_t wcnt[kVertPerLane * kVertWaves], wpre[kVertPerLane * kVertWaves + 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t a = (uint64_t)t * kVertTile;
        const uint32_t base = tile_base[t];
        uint32_t word[kVertPerLane], rank[kVertPerLane];
        bool keep[kVertPerLane];
#pragma unroll
        for (uint32_t i = 0; i < kVertPerLane; i++) {
            const uint64_t j = a + i * kBlock + threadIdx.x;
            const bool in = j < entries;
            word[i] = in ? nbrs[j] : 0u;
            keep[i] = in && flag[j] == 0;
        }
#pragma unroll
        for (uint32_t i = 0; i < kVertPerLane; i++) {
            const unsigned long long mask = __ballot(keep[i]);
            rank[i] = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[i * kVertWaves + wave] = (uint32_t)__popcll(mask);
        }
        __syncthreads();
        if (threadIdx.x <= kVertPerLane * kVertWaves) {  // the entries run by step, then wave, then lane
            uint32_t s = 0;
            for (uint32_t q = 0; q < threadIdx.x; q++) s += wcnt[q];
            wpre[threadIdx.x] = s;
            if (threadIdx.x == kVertPerLane * kVertWaves) pre[kVertTile] = (uint16_t)s;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kVertPerLane; i++) {
            const uint32_t idx = i * kBlock + threadIdx.x, pos = wpre[i * kVertWaves + wave] + rank[i];
            pre[idx] = (uint16_t)pos;
            const uint32_t o = base + pos;
            if (keep[i] && o < entries) {
                new_nbrs[o] = vert_new_id(bits, below, word[i]);
                if (kMap) map[o] = (uint32_t)(a + idx);
            }
        }
        __syncthreads();
        // the rows whose old start lies in [a, a + kVertTile); the last tile also takes the empty rows at the array's end
        const uint32_t r0 = start_lower_bound(adj_start, n, a);
        const uint32_t r1 = t + 1 == tiles ? n : start_lower_bound(adj_start, n, a + kVertTile);
        for (uint32_t x = r0 + threadIdx.x; x < r1; x += kBlock) {
            if (vert_removed(bits, x)) continue;
            const uint64_t off = (uint64_t)adj_start[x] - a;
            const uint32_t nx = vert_new_id(bits, below, x);
            if (nx < n_surv && off <= kVertTile) new_start[nx] = base + pre[off];
        }
        __syncthreads();
    }
}

// one lane per vertex of G: where it went
static __global__ void k_vert_map(uint32_t n, uint32_t n_surv, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ below,
                                  uint32_t *__restrict__ vmap)
{
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
        if (vert_removed(bits, (uint32_t)v)) continue;
        const uint32_t nv = vert_new_id(bits, below, (uint32_t)v);
        if (nv < n_surv) vmap[nv] = (uint32_t)v;
    }
}

// one lane per vertex of G' (and the word behind the last, which the loader leaves zero): degree, label, presence; the constant
// tail of the added vertices.  *total: entries'.  A survivor reads the start of the next SURVIVOR only, a tail lane writes tail
// words only: nothing is ordered.
static __global__ void k_vert_tail(uint32_t n_before, uint32_t n_surv, uint32_t n_after, const uint32_t *__restrict__ total,
                                   const uint32_t *__restrict__ old_labels, const uint32_t *__restrict__ add_labels, uint32_t *__restrict__ new_start,
                                   uint32_t *__restrict__ new_deg, uint32_t *__restrict__ new_labels, uint8_t *__restrict__ present,
                                   uint32_t *__restrict__ vmap)
{
    const uint32_t m2 = *total;
    for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x <= n_after; x += (uint64_t)gridDim.x * blockDim.x) {
        if (x == n_after) {
            new_start[x] = 0;
            new_deg[x] = 0;
            present[x] = 0;
        } else if (x < n_surv) {
            const uint32_t next = x + 1 < n_surv ? new_start[x + 1] : m2, old = vmap[x];
            new_deg[x] = next - new_start[x];
            new_labels[x] = old < n_before ? old_labels[old] : 0u;
            present[x] = 1;
        } else {
            new_start[x] = m2;
            new_deg[x] = 0;
            new_labels[x] = add_labels[x - n_surv];
            present[x] = 1;
            vmap[x] = GNNPE_NO_VERTEX;
        }
    }
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_csr_apply_vertices(gnnpe_ctx *c, const uint32_t *remove, uint64_t n_remove, const uint32_t *add_labels, uint64_t n_add,
                                        uint32_t *n_after, uint64_t *n_entries_before, uint64_t *n_entries_after, void **dev_vertex_map,
                                        void **dev_entry_map, double *device_ms)
{
    const char *who = "gnnpe_csr_apply_vertices";
    if (dev_vertex_map) *dev_vertex_map = nullptr;
    if (dev_entry_map) *dev_entry_map = nullptr;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c, GNNPE_ERR_ARG, "%s: null argument", who);
    if (n_after) *n_after = c->n;
    if (n_entries_before) *n_entries_before = c->nbr_used;
    if (n_entries_after) *n_entries_after = c->nbr_used;
    c->map_valid = c->vmap_valid = false;  // whatever happens below, the maps of an earlier batch are gone
    GNNPE_REQUIRE((remove || n_remove == 0) && (add_labels || n_add == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = require_whole_graph(who, c);
    if (rc) return rc;
    const bool want_map = dev_entry_map != nullptr;
    const uint32_t n = c->n;
    const uint64_t entries = c->nbr_used;
    std::vector<uint32_t> rem(remove, remove + n_remove);
    for (uint32_t v : rem) GNNPE_REQUIRE(v < n, GNNPE_ERR_ARG, "%s: vertex %u is not a vertex of the graph (n = %u)", who, v, n);
    std::sort(rem.begin(), rem.end());
    rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
    const uint32_t k = (uint32_t)rem.size(), n_surv = n - k;
    GNNPE_REQUIRE(n_add < 0xFFFFFFFFull, GNNPE_ERR_RANGE, "%s: %llu added vertices exceed 32-bit ids", who, (unsigned long long)n_add);
    const uint64_t n2_64 = (uint64_t)n_surv + n_add;
    GNNPE_REQUIRE(n2_64 != 0, GNNPE_ERR_ARG, "%s: the batch leaves no vertex", who);
    GNNPE_REQUIRE(n2_64 < 0xFFFFFFFFull, GNNPE_ERR_RANGE, "%s: %llu vertices exceed 32-bit ids", who, (unsigned long long)n2_64);
    const uint32_t n2 = (uint32_t)n2_64;
    GNNPE_HIP_TRY(hipSetDevice(c->device));

    if (k == 0 && n_add == 0) {  // nothing changes: the identity maps, the generation stays
        if ((rc = c->upd_vmap.reserve(((size_t)n + 1) * 4)) || (want_map && (rc = c->upd_map.reserve((entries + 1) * 4)))) return rc;
        LaunchTimer timer;
        if ((rc = timer.begin(device_ms, c->stream))) return rc;
        hipLaunchKernelGGL(k_map_identity, dim3(std::min<int>(grid_for(n), c->num_cus * 8)), dim3(kBlock), 0, c->stream, n, c->upd_vmap.as<uint32_t>());
        if (want_map && entries)
            hipLaunchKernelGGL(k_map_identity, dim3(std::min<int>(grid_for(entries), c->num_cus * 8)), dim3(kBlock), 0, c->stream, (uint32_t)entries,
                               c->upd_map.as<uint32_t>());
        GNNPE_HIP_TRY(hipGetLastError());
        if ((rc = timer.end(c->stream))) return rc;
        c->vmap_valid = true;
        c->vmap_gen = c->graph_gen;
        c->vmap_before = c->vmap_after = n;
        if (want_map) {
            c->map_valid = true;
            c->map_gen = c->graph_gen;
            c->map_before = c->map_after = entries;
            *dev_entry_map = c->upd_map.p;
        }
        if (dev_vertex_map) *dev_vertex_map = c->upd_vmap.p;
        return GNNPE_OK;
    }

    // the spare arrays of G' and the batch's work area: [R | A | bits | below | tile counts | tile bases | flags]
    const uint32_t words = n / 32 + 1;  // ceil(n / 32) words hold a bit, one more behind them for the scan's total
    const uint32_t tiles = (uint32_t)std::max<uint64_t>(1, (entries + kVertTile - 1) / kVertTile);
    const size_t work_words = (size_t)k + n_add + 2 * ((size_t)words + 1) + 2 * ((size_t)tiles + 1);
    if ((rc = c->upd_start.reserve(((size_t)n2 + 1) * 4)) || (rc = c->upd_deg.reserve(((size_t)n2 + 1) * 4)) ||
        (rc = c->upd_labels.reserve(((size_t)n2 + 1) * 4)) || (rc = c->upd_present.reserve((size_t)n2 + 1)) ||
        (rc = c->upd_vmap.reserve(((size_t)n2 + 1) * 4)) || (rc = c->upd_nbrs.reserve((entries + 1) * 4)) ||
        (rc = c->upd_work.reserve(work_words * 4 + entries + 64)) || (want_map && (rc = c->upd_map.reserve((entries + 1) * 4))))
        return rc;
    DevBuf fresh_owned;  // has to grow with n: allocated aside, so that a refusal by the device loses nothing
    if ((rc = grow_aside(c->owned, fresh_owned, (size_t)n2 + 1))) return rc;
    uint32_t *d_rem = c->upd_work.as<uint32_t>(), *d_add = d_rem + k, *bits = d_add + n_add, *below = bits + words + 1;
    uint32_t *tile_cnt = below + words + 1, *tile_base = tile_cnt + tiles + 1;
    uint8_t *flag = reinterpret_cast<uint8_t *>(tile_base + tiles + 1);
    size_t tb = 0, tb2 = 0;
    hipcub::TransformInputIterator<uint32_t, PopcountOp, const uint32_t *> popc(bits, PopcountOp());
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, popc, below, (int64_t)words + 1, c->stream));
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, tile_cnt, tile_base, (int64_t)tiles + 1, c->stream));
    if ((rc = c->cub_tmp.reserve(std::max<size_t>(std::max(tb, tb2), 1)))) return rc;

    UpdateEvents E;
    const bool timed = device_ms != nullptr || c->sw.debug;
    if (timed)
        for (hipEvent_t &e : E.ev) GNNPE_HIP_TRY(hipEventCreate(&e));
    if (k) GNNPE_HIP_TRY(hipMemcpyAsync(d_rem, rem.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
    if (n_add) GNNPE_HIP_TRY(hipMemcpyAsync(d_add, add_labels, (size_t)n_add * 4, hipMemcpyHostToDevice, c->stream));
    if (timed) GNNPE_HIP_TRY(hipEventRecord(E.ev[0], c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(bits, 0, ((size_t)words + 1) * 4, c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(tile_cnt, 0, ((size_t)tiles + 1) * 4, c->stream));
    if (entries) GNNPE_HIP_TRY(hipMemsetAsync(flag, 0, entries, c->stream));
    if (k)
        hipLaunchKernelGGL(k_vert_mark, dim3((uint32_t)std::min<uint64_t>((k + kVertWaves - 1) / kVertWaves, (uint64_t)c->num_cus * 16)), dim3(kBlock), 0,
                           c->stream, k, d_rem, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(),
                           c->revpos.as<uint32_t>(), bits, flag);
    GNNPE_HIP_TRY(hipGetLastError());
    tb = c->cub_tmp.bytes;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tb, popc, below, (int64_t)words + 1, c->stream));
    const uint32_t tile_grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)c->num_cus * 8);
    hipLaunchKernelGGL(k_vert_tile_counts, dim3(tile_grid), dim3(kBlock), 0, c->stream, (uint32_t)entries, tiles, flag, tile_cnt);
    GNNPE_HIP_TRY(hipGetLastError());
    tb = c->cub_tmp.bytes;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tb, tile_cnt, tile_base, (int64_t)tiles + 1, c->stream));
    hipLaunchKernelGGL(k_vert_map, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, n, n_surv, bits, below, c->upd_vmap.as<uint32_t>());
    if (want_map)
        hipLaunchKernelGGL(k_vert_compact<true>, dim3(tile_grid), dim3(kBlock), 0, c->stream, n, (uint32_t)entries, tiles, n_surv,
                           c->adj_start.as<uint32_t>(), c->nbrs.as<uint32_t>(), flag, bits, below, tile_base, c->upd_start.as<uint32_t>(),
                           c->upd_nbrs.as<uint32_t>(), c->upd_map.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_vert_compact<false>, dim3(tile_grid), dim3(kBlock), 0, c->stream, n, (uint32_t)entries, tiles, n_surv,
                           c->adj_start.as<uint32_t>(), c->nbrs.as<uint32_t>(), flag, bits, below, tile_base, c->upd_start.as<uint32_t>(),
                           c->upd_nbrs.as<uint32_t>(), (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_vert_tail, dim3(grid_for((uint64_t)n2 + 1)), dim3(kBlock), 0, c->stream, n, n_surv, n2, tile_base + tiles,
                       c->labels.as<uint32_t>(), d_add, c->upd_start.as<uint32_t>(), c->upd_deg.as<uint32_t>(), c->upd_labels.as<uint32_t>(),
                       c->upd_present.as<uint8_t>(), c->upd_vmap.as<uint32_t>());
    GNNPE_HIP_TRY(hipGetLastError());
    if (timed) GNNPE_HIP_TRY(hipEventRecord(E.ev[1], c->stream));
    // the call's wait: the decision is taken here, before anything of the context changes
    uint32_t *h_words = reinterpret_cast<uint32_t *>(c->h_pinned);
    GNNPE_HIP_TRY(hipMemcpyAsync(h_words, tile_base + tiles, 4, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(h_words + 1, below + words, 4, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t m2 = h_words[0];
    GNNPE_REQUIRE(h_words[1] == k && m2 <= entries, GNNPE_ERR_HIP, "%s: internal error: %u of %u vertices marked, %llu of %llu entries kept", who,
                  h_words[1], k, (unsigned long long)m2, (unsigned long long)entries);
    GNNPE_REQUIRE(m2 + n2 < (1ull << 32), GNNPE_ERR_RANGE, "%s: %llu entries + %u vertices exceed 32-bit addressing", who, (unsigned long long)m2, n2);

    // the swap, then exactly the tail of gnnpe_load_csr
    c->graph_gen++;
    c->vmap_valid = true;
    c->vmap_gen = c->graph_gen;
    c->vmap_before = n;
    c->vmap_after = n2;
    if (want_map) {
        c->map_valid = true;
        c->map_gen = c->graph_gen;
        c->map_before = entries;
        c->map_after = m2;
    }
    swap_buffers(c->adj_start, c->upd_start);
    swap_buffers(c->adj_deg, c->upd_deg);
    swap_buffers(c->nbrs, c->upd_nbrs);
    swap_buffers(c->labels, c->upd_labels);
    swap_buffers(c->present, c->upd_present);
    if (fresh_owned.p) swap_buffers(c->owned, fresh_owned);
    if (timed) GNNPE_HIP_TRY(hipEventRecord(E.ev[2], c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->owned.p, c->present.p, n2, hipMemcpyDeviceToDevice, c->stream));
    c->have_graph = false;
    c->n = n2;
    c->n_rows = c->n_held = n2;
    c->nbr_used = c->nbr_owned = m2;
    c->nbr_cap = c->nbrs.bytes / 4;
    if ((rc = finish_rows(c, n2, nullptr))) return rc;
    if (m2)
        hipLaunchKernelGGL(k_gather_u32, dim3(grid_for(m2)), dim3(kBlock), 0, c->stream, m2, c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                           c->nbr_label.as<uint32_t>());
    GNNPE_HIP_TRY(hipGetLastError());
    c->have_graph = true;
    c->slab_begin = 0;
    c->slab_end = n2;
    c->slab_set = false;
    c->have_order = false;
    invalidate_derived(c);
    if (n_after) *n_after = n2;
    if (n_entries_after) *n_entries_after = m2;
    if (dev_vertex_map) *dev_vertex_map = c->upd_vmap.p;
    if (want_map) *dev_entry_map = c->upd_map.p;
    if (timed) {
        GNNPE_HIP_TRY(hipEventRecord(E.ev[3], c->stream));
        GNNPE_HIP_TRY(hipEventSynchronize(E.ev[3]));
        float all = 0.f, build = 0.f, rebuild = 0.f;
        GNNPE_HIP_TRY(hipEventElapsedTime(&all, E.ev[0], E.ev[3]));
        GNNPE_HIP_TRY(hipEventElapsedTime(&build, E.ev[0], E.ev[1]));
        GNNPE_HIP_TRY(hipEventElapsedTime(&rebuild, E.ev[2], E.ev[3]));
        if (device_ms) *device_ms = all;
        // build: the marks to the tail kernel; wait: the two words' read-back and the host's decision; rebuild: owned, finish_rows, the labels
        if (c->sw.debug)
            fprintf(stderr, "[apply_vertices] removed=%u added=%llu n=%u->%u entries=%llu->%llu device_ms=%.4f build_ms=%.4f wait_ms=%.4f rebuild_ms=%.4f\n",
                    k, (unsigned long long)n_add, n, n2, (unsigned long long)entries, (unsigned long long)m2, all, build, all - build - rebuild, rebuild);
    }
    return GNNPE_OK;
}
