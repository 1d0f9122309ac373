// gnnpe_touched.hip -- TOUCHED VERTEX SETS ON THE DEVICE: gnnpe_csr_closed_neighbourhood and gnnpe_csr_carry_vertex_set of
// include/gnnpe_hip.h ("touched sets"), and the ordered compaction k_sets_members both end with.
//
// The support loops of a relabel and of a vertex batch need T = R u N_G(R) and, behind a vertex batch, T' = the new ids of T's
// survivors together with the added vertices.  A caller with a host copy of the rows builds them there; the standing exact query
// (gnnpe_standing.hip) has none, and nothing proportional to n or m may cross to the host per batch.  Here both are made from the
// resident rows and the resident vertex map, as a bitmap and as ascending ids -- the two forms gnnpe_filter_support_exact_delta_device
// takes.
//
// k_touched_mark: one wave per vertex of R, lanes over its row 64 entries at a time, atomicOr into a zeroed bitmap (two vertices of
//   R may share a neighbour, two neighbours a word); R's own bit by lane 0.  The work is the sum of R's degrees.
// k_touched_carry: one lane per vertex of G', the wave's 64 answers one __ballot stored as two words by lane 0 -- one writer per
//   word, every word written, the bits at and above n' zero: the shape of k_support_bitmap.
// k_sets_members: an ORDERED stream compaction, no atomics, so that the ids come out ascending as gnnpe_host::set_members gives
//   them.  One workgroup walks the row tile by tile (kMembersTile words = 8192 vertices): a lane's word, its popcount, the
//   inclusive DPP scan of the wave (wave_scan_add of gnnpe_dpp.hip.h), the four wave totals through LDS, and the lane expands its
//   word into the tile's ids in LDS at its exclusive offset; then the workgroup stores the tile's ids to carry + i with consecutive
//   lanes on consecutive words (the expansion's scattered stores stay in LDS), and the carry moves on by the tile's total.  The last
//   word of the row is masked to the bits below n.  (It came here from gnnpe_standing.hip unchanged: that library links this one.)
#include <algorithm>

#include "gnnpe_dpp.hip.h"
#include "gnnpe_touched.hip.h"
#include "gnnpe_launch_timer.hip.h"

namespace gnnpe {

constexpr uint32_t kMembersTile = kBlock;  // words of a row per step of k_sets_members: one per lane

// out[0 .. min(cap, k)) = the first ids of the k set bits below n of `row`, ascending; *total = k (total may be null: the walk then
// ends with the tile that fills cap).  One workgroup of kBlock lanes.
static __global__ __launch_bounds__(kBlock) void k_sets_members(const uint32_t *__restrict__ row, uint64_t words, uint32_t n,
                                                                uint32_t *__restrict__ out, uint64_t cap, unsigned long long *__restrict__ total)
{
    __shared__ uint32_t s_ids[kMembersTile * 32];  // the ids of one tile: 32 KiB
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint64_t carry = 0;  // ids of the tiles before this one
    for (uint64_t w0 = 0; w0 < words; w0 += kMembersTile) {
        if (!total && carry >= cap) break;  // (uniform)
        const uint64_t w = w0 + t;
        uint32_t x = w < words ? sets_word_below_n(row[w], w, words, n) : 0u;
        const uint32_t c = (uint32_t)__popc(x);
        const uint32_t incl = wave_scan_add(c);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile_total = 0;
#pragma unroll
        for (uint32_t i = 0; i < kBlock / 64; i++) {
            const uint32_t v = s_wave[i];
            before += i < wave ? v : 0u;
            tile_total += v;
        }
        uint32_t o = before + incl - c;  // at most kMembersTile * 32 - c: the expansion stays inside s_ids
        for (; x; x &= x - 1u) s_ids[o++] = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)x) - 1u;
        __syncthreads();
        for (uint32_t i = t; i < tile_total; i += kBlock)
            if (carry + i < cap) out[carry + i] = s_ids[i];
        carry += tile_total;
        __syncthreads();  // s_wave and s_ids are written again in the next step
    }
    if (t == 0 && total) *total = carry;
}

hipError_t sets_members_launch(hipStream_t stream, const uint32_t *d_row, uint64_t words, uint32_t n, uint32_t *d_out, uint64_t cap,
                               unsigned long long *d_total)
{
    hipLaunchKernelGGL(k_sets_members, dim3(1), dim3(kBlock), 0, stream, d_row, words, n, d_out, cap, d_total);
    return hipGetLastError();
}

// one wave per listed vertex (ids below n: the host has checked; a repeated id sets the same bits again)
static __global__ __launch_bounds__(kBlock) void k_touched_mark(uint32_t count, const uint32_t *__restrict__ verts, const uint32_t *__restrict__ adj_start,
                                                                const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs, uint32_t n,
                                                                uint32_t *__restrict__ bits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (kBlock / 64);
    for (uint32_t t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < count; t += waves) {
        const uint32_t v = verts[t];
        const uint32_t st = adj_start[v], d = adj_deg[v];
        if (lane == 0) atomicOr(&bits[v >> 5], 1u << (v & 31u));
        for (uint32_t i = lane; i < d; i += 64) {
            const uint32_t u = nbrs[st + i];
            if (u < n) atomicOr(&bits[u >> 5], 1u << (u & 31u));  // (a word of a whole simple graph is below n: no store leaves the bitmap)
        }
    }
}

// bit v' of new_bits = vmap[v'] is a vertex of old_bits (n_before vertices), or with_added and vmap[v'] == GNNPE_NO_VERTEX
static __global__ __launch_bounds__(kBlock) void k_touched_carry(uint32_t n_before, uint32_t n_after, const uint32_t *__restrict__ vmap,
                                                                 const uint32_t *__restrict__ old_bits, uint32_t with_added, uint64_t words_after,
                                                                 uint32_t *__restrict__ new_bits)
{
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t chunks = ((uint64_t)n_after + 63) / 64;
    uint64_t c = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; c < chunks; c += nw) {  // wave-uniform: every lane reaches the __ballot
        const uint64_t v = c * 64 + lane;
        bool in = false;
        if (v < n_after) {
            const uint32_t old = vmap[v];
            in = old == GNNPE_NO_VERTEX ? with_added != 0 : old < n_before && ((old_bits[old >> 5] >> (old & 31u)) & 1u) != 0;
        }
        const uint64_t m = __ballot(in);
        if (lane == 0) {
            new_bits[2 * c] = (uint32_t)m;
            if (2 * c + 1 < words_after) new_bits[2 * c + 1] = (uint32_t)(m >> 32);
        }
    }
}

// the end of both calls: the ids of the `words`-word bitmap over n vertices, the count to the host in the call's one wait
static int touched_ids(const char *who, gnnpe_ctx *c, LaunchTimer &timer, const uint32_t *bits, uint64_t words, uint32_t n, void *dev_ids,
                       uint64_t ids_cap, unsigned long long *d_total, uint64_t *n_ids)
{
    GNNPE_HIP_TRY(sets_members_launch(c->stream, bits, words, n, static_cast<uint32_t *>(dev_ids), dev_ids ? ids_cap : 0, d_total));
    int rc = timer.end(c->stream);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    *n_ids = c->h_pinned[0];
    GNNPE_REQUIRE(dev_ids ? *n_ids <= ids_cap : *n_ids == 0, GNNPE_ERR_ARG, "%s: the set has %llu vertices, ids_cap is %llu (the bitmap is written)",
                  who, (unsigned long long)*n_ids, (unsigned long long)(dev_ids ? ids_cap : 0));
    return GNNPE_OK;
}

static int touched_pointers(const char *who, const void *dev_bits, const void *dev_ids, uint64_t ids_cap)
{
    GNNPE_REQUIRE(dev_bits && (reinterpret_cast<uintptr_t>(dev_bits) & 3u) == 0, GNNPE_ERR_ARG, "%s: the bitmap must be a 4-byte aligned device pointer", who);
    GNNPE_REQUIRE((dev_ids || ids_cap == 0) && (reinterpret_cast<uintptr_t>(dev_ids) & 3u) == 0, GNNPE_ERR_ARG,
                  "%s: dev_ids must be a 4-byte aligned device pointer of ids_cap words", who);
    return GNNPE_OK;
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" int gnnpe_csr_closed_neighbourhood(gnnpe_ctx *c, const uint32_t *vertices, uint64_t n_vertices, void *dev_bits, void *dev_ids,
                                              uint64_t ids_cap, uint64_t *n_ids, double *device_ms)
{
    const char *who = "gnnpe_csr_closed_neighbourhood";
    if (n_ids) *n_ids = 0;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && n_ids && (vertices || n_vertices == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = require_whole_graph(who, c);
    if (rc || (rc = touched_pointers(who, dev_bits, dev_ids, ids_cap))) return rc;
    const uint32_t n = c->n;
    GNNPE_REQUIRE(n_vertices < (1ull << 32), GNNPE_ERR_ARG, "%s: %llu ids, the list is 32-bit", who, (unsigned long long)n_vertices);
    for (uint64_t i = 0; i < n_vertices; i++)
        GNNPE_REQUIRE(vertices[i] < n, GNNPE_ERR_ARG, "%s: vertex %u is not a vertex of the graph (n = %u)", who, vertices[i], n);
    const uint64_t words = ((uint64_t)n + 31) / 32;
    const uint32_t k = (uint32_t)n_vertices;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    // the work area: [the count | R]
    if ((rc = c->upd_work.reserve(8 + (size_t)k * 4))) return rc;
    unsigned long long *d_total = c->upd_work.as<unsigned long long>();
    uint32_t *d_verts = reinterpret_cast<uint32_t *>(d_total + 1), *bits = static_cast<uint32_t *>(dev_bits);
    if (k) GNNPE_HIP_TRY(hipMemcpyAsync(d_verts, vertices, (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
    LaunchTimer timer;
    if ((rc = timer.begin(device_ms, c->stream))) return rc;
    if (words) GNNPE_HIP_TRY(hipMemsetAsync(bits, 0, words * 4, c->stream));
    if (k) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)k + kBlock / 64 - 1) / (kBlock / 64), (uint64_t)c->num_cus * 16);
        hipLaunchKernelGGL(k_touched_mark, dim3(grid), dim3(kBlock), 0, c->stream, k, d_verts, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), n, bits);
        GNNPE_HIP_TRY(hipGetLastError());
    }
    return touched_ids(who, c, timer, bits, words, n, dev_ids, ids_cap, d_total, n_ids);  // (`vertices` is read until the wait inside)
}

extern "C" int gnnpe_csr_carry_vertex_set(gnnpe_ctx *c, const void *dev_bits_old, int with_added, void *dev_bits_new, void *dev_ids, uint64_t ids_cap,
                                          uint64_t *n_ids, double *device_ms)
{
    const char *who = "gnnpe_csr_carry_vertex_set";
    if (n_ids) *n_ids = 0;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && n_ids, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(c->vmap_valid && c->vmap_gen == c->graph_gen && c->have_graph, GNNPE_ERR_ARG,
                  "%s: the context has no valid vertex map (gnnpe_csr_apply_vertices makes one; loading or changing the rows ends it)", who);
    int rc = touched_pointers(who, dev_bits_new, dev_ids, ids_cap);
    if (rc) return rc;
    GNNPE_REQUIRE(dev_bits_old && (reinterpret_cast<uintptr_t>(dev_bits_old) & 3u) == 0, GNNPE_ERR_ARG,
                  "%s: the bitmap must be a 4-byte aligned device pointer", who);
    const uint32_t n_before = (uint32_t)c->vmap_before, n_after = (uint32_t)c->vmap_after;
    const uint64_t words_before = ((uint64_t)n_before + 31) / 32, words_after = ((uint64_t)n_after + 31) / 32;
    const uintptr_t s = (uintptr_t)dev_bits_old, d = (uintptr_t)dev_bits_new;
    GNNPE_REQUIRE(s + words_before * 4 <= d || d + words_after * 4 <= s, GNNPE_ERR_ARG, "%s: the two bitmaps overlap", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->upd_work.reserve(8))) return rc;
    unsigned long long *d_total = c->upd_work.as<unsigned long long>();
    uint32_t *bits = static_cast<uint32_t *>(dev_bits_new);
    LaunchTimer timer;
    if ((rc = timer.begin(device_ms, c->stream))) return rc;
    hipLaunchKernelGGL(k_touched_carry, dim3(grid_for(((uint64_t)n_after + 63) / 64 * 64)), dim3(kBlock), 0, c->stream, n_before, n_after,
                       c->upd_vmap.as<uint32_t>(), static_cast<const uint32_t *>(dev_bits_old), with_added ? 1u : 0u, words_after, bits);
    GNNPE_HIP_TRY(hipGetLastError());
    return touched_ids(who, c, timer, bits, words_after, n_after, dev_ids, ids_cap, d_total, n_ids);
}
