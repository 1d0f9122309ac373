// gnnpe_update.hip -- A BATCH OF EDGE INSERTIONS AND DELETIONS APPLIED TO THE RESIDENT GRAPH: gnnpe_csr_apply_edges and
// gnnpe_csr_download of include/gnnpe_hip.h (ABI 16); gnnpe_csr_apply_edges_map and gnnpe_csr_carry_entries (ABI 20): the same
// call leaving the entry map of the batch on the device, and the kernel that moves a caller's per-entry table through it.  The step between two gnnpe_refine_sets_delta calls: delta over the
// deletions, apply, delta over the insertions.
//
// Everything runs on the context's stream from the few kilobytes of the batch, with one wait before the decision:
//
//   1. the host turns every pair into its two directed keys (x << 32) | y and uploads them; hipcub sorts each list and keeps the
//      first key of every run (DeviceRadixSort::SortKeys, DeviceSelect::Unique: the unique counts stay on the device);
//   2. k_update_check, one lane per unique key: a lower bound in old row x gives the key's position there and whether y is
//      present.  An insert must be absent, a delete present, and no insert key may be among the delete keys.  An offender goes
//      into the counter block with atomicMin on the key (the lists are ascending: the smallest key is the smallest index), so
//      the message names the same pair on every run;
//   3. k_update_degrees, one lane per vertex: deg' = deg + (insert keys of the row) - (delete keys of the row), two lower bounds
//      per list, and a flag for the rows the batch touches; DeviceScan::ExclusiveSum gives the offsets of G',
//      k_offsets_to_start_deg (as the loader uses it) the spare adj_start / adj_deg, DeviceSelect::Flagged the ascending list
//      of touched rows;
//   4. k_csr_merge writes the spare neighbour array:
//      - between two touched rows both arrays hold one contiguous stretch that moves by a constant.  The first blocks of the
//        grid stream the OLD array in tiles of kMergeTile entries: the wave looks up the tile's first touched row once (a
//        binary search among the touched rows' old ends, wave-uniform, in a list that sits in L2), a lane then only steps over
//        the touched rows that begin inside its tile.  Loads and stores are consecutive dwords per wave; entries of touched
//        rows are skipped here;
//      - the remaining blocks give one wave to every touched row, in chunks of 64: an old entry finds its rank among the row's
//        insert and delete keys (two short binary searches among the few keys of the row) and lands at
//        position + inserts below - deletes below unless it is a delete key itself; an insert key lands at (its position in
//        the old row, from step 2) + (its rank among the row's inserts) - (deletes below it).  No lane reads outside its
//        row, nothing is staged in LDS or scratch.
//      Its floor is one read of the old array and one write of the new.  A batch with an offender never reaches the merge's
//      stores (the kernel reads the counter block first): garbage degrees cannot send a store out of bounds.
//   5. the wait; a refusal returns here, with nothing but the spare buffers written.  Otherwise the three arrays are swapped
//      with the spare ones and the tail of gnnpe_load_csr runs: owned from present, finish_rows (validation, revpos, hub list),
//      the neighbour labels, the resets, graph_gen++.  The rebuild is whole on purpose: "the state of a fresh load" holds by
//      construction (DESIGN.md section 3.7 has its share of the time).
//
// The entry map (ABI 20) is written by the merge itself, at its three store sites: the streaming part knows the old entry j of the
// word it moves, the stay-loop of a touched row knows st + p, an insert has none.  k_carry_entries (below) is a gather through it.
//
// Transient memory: a second neighbour array (and second adj_start / adj_deg); they stay with the context as the next call's spare.
//
// gnnpe_set_vertex_labels and gnnpe_labels_download (at the end) are the vertex half: new labels on a few vertices, with the rows,
// the reverse positions and the hub list left standing.  k_set_labels patches labels[v] and, through revpos, the copy of v's label in
// every neighbour's row; the host then runs the resets of gnnpe_load_csr's tail.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "gnnpe_common.h"
#include "gnnpe_update.hip.h"

namespace gnnpe {

typedef unsigned long long ukey;
constexpr ukey kNoKey = ~0ull;
constexpr uint32_t kMergeTile = 2048;  // entries of the old array per block and step: 8 consecutive-dword loads per lane

struct UpdateCounters {  // one block, read back in the call's single wait
    uint32_t n_ins, n_del;  // unique directed keys of the two lists
    uint32_t n_touched, entries_after;
    ukey bad_insert, bad_delete, bad_both;  // smallest offending key of each kind, kNoKey = none
};

// first index in keys[0 .. n) whose key is >= key
__device__ __forceinline__ uint32_t key_lower_bound(const ukey *__restrict__ keys, uint32_t lo, uint32_t hi, ukey key)
{
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one lane per unique key of either list (inserts first): its position in the old row of x, and the three refusals
static __global__ void k_update_check(uint32_t cap_ins, uint32_t cap_del, const ukey *__restrict__ ikeys, const ukey *__restrict__ dkeys,
                                      const uint32_t *__restrict__ adj_start, const uint32_t *__restrict__ adj_deg,
                                      const uint32_t *__restrict__ nbrs, uint32_t *__restrict__ ipos, UpdateCounters *ctr)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_ins = ctr->n_ins, n_del = ctr->n_del;
    const bool ins = t < cap_ins;
    const uint32_t i = ins ? t : t - cap_ins;
    if (ins ? i >= n_ins : (i >= n_del || i >= cap_del)) return;
    const ukey key = ins ? ikeys[i] : dkeys[i];
    const uint32_t x = (uint32_t)(key >> 32), y = (uint32_t)key;
    const uint32_t st = adj_start[x];
    uint32_t lo = 0, hi = adj_deg[x];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (nbrs[st + mid] < y) lo = mid + 1; else hi = mid;
    }
    const bool present = lo < adj_deg[x] && nbrs[st + lo] == y;
    if (ins) {
        ipos[i] = lo;
        if (present) atomicMin(&ctr->bad_insert, key);
        const uint32_t k = key_lower_bound(dkeys, 0, n_del, key);
        if (k < n_del && dkeys[k] == key) atomicMin(&ctr->bad_both, key);
    } else if (!present) {
        atomicMin(&ctr->bad_delete, key);
    }
}

// one lane per vertex: the new degree (cnt[n] = 0 for the scan) and whether the batch touches the row
static __global__ void k_update_degrees(uint32_t n, const uint32_t *__restrict__ adj_deg, const ukey *__restrict__ ikeys,
                                        const ukey *__restrict__ dkeys, const UpdateCounters *__restrict__ ctr, uint32_t *__restrict__ cnt,
                                        uint8_t *__restrict__ touched)
{
    const uint32_t n_ins = ctr->n_ins, n_del = ctr->n_del;
    for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x <= n; x += (uint64_t)gridDim.x * blockDim.x) {
        if (x == n) {
            cnt[x] = 0;
            continue;
        }
        const uint32_t ia = key_lower_bound(ikeys, 0, n_ins, (ukey)x << 32), ib = key_lower_bound(ikeys, ia, n_ins, (ukey)(x + 1) << 32);
        const uint32_t da = key_lower_bound(dkeys, 0, n_del, (ukey)x << 32), db = key_lower_bound(dkeys, da, n_del, (ukey)(x + 1) << 32);
        cnt[x] = adj_deg[x] + (ib - ia) - (db - da);
        touched[x] = (ib - ia) + (db - da) != 0;
    }
}

// the scan's total beside the other counters
static __global__ void k_update_total(uint32_t n, const uint32_t *__restrict__ offs, UpdateCounters *ctr) { ctr->entries_after = offs[n]; }

// The new neighbour array from the old one and the two key lists (the file's head, step 4).  Blocks [0, copy_blocks) stream
// the stretches between touched rows, the others merge the touched rows, one wave each.  kMap: every store of a neighbour word
// also stores the entry map's word for the same new entry (the old entry it came from, GNNPE_NO_ENTRY for an insert), under
// the same guard; without it `map` is not looked at and the code is the one of before the map existed.
template <bool kMap>
__global__ __launch_bounds__(kBlock) void k_csr_merge(uint32_t copy_blocks, uint32_t entries, const uint32_t *__restrict__ adj_start,
                                                     const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                     const uint32_t *__restrict__ new_start, const uint32_t *__restrict__ new_deg,
                                                     uint32_t *__restrict__ new_nbrs, const uint32_t *__restrict__ rows,
                                                     const ukey *__restrict__ ikeys, const ukey *__restrict__ dkeys,
                                                     const uint32_t *__restrict__ ipos, const UpdateCounters *__restrict__ ctr,
                                                     uint32_t *__restrict__ map)
{
    if ((ctr->bad_insert & ctr->bad_delete & ctr->bad_both) != kNoKey) return;  // refused: the degrees mean nothing
    const uint32_t nt = ctr->n_touched, entries_after = ctr->entries_after;
    if (blockIdx.x < copy_blocks) {
        for (uint64_t a = (uint64_t)blockIdx.x * kMergeTile; a < entries; a += (uint64_t)copy_blocks * kMergeTile) {
            // the first touched row that ends behind the tile's first entry: once per tile, the same in every lane
            uint32_t lo = 0, hi = nt;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1, r = rows[mid];
                if (adj_start[r] + adj_deg[r] <= (uint32_t)a) lo = mid + 1; else hi = mid;
            }
            uint32_t k = lo, r_beg = entries, r_end = entries, shift = entries_after - entries;  // behind the last touched row
            if (k < nt) {
                const uint32_t r = rows[k];
                r_beg = adj_start[r];
                r_end = r_beg + adj_deg[r];
                shift = new_start[r] - r_beg;
            }
            const uint64_t stop = min(a + kMergeTile, (uint64_t)entries);
            for (uint64_t j64 = a + threadIdx.x; j64 < stop; j64 += kBlock) {
                const uint32_t j = (uint32_t)j64;
                while (k < nt && j >= r_end) {  // a touched row began and ended before j: the next stretch
                    k++;
                    if (k < nt) {
                        const uint32_t r = rows[k];
                        r_beg = adj_start[r];
                        r_end = r_beg + adj_deg[r];
                        shift = new_start[r] - r_beg;
                    } else {
                        r_beg = r_end = entries;
                        shift = entries_after - entries;
                    }
                }
                if (k < nt && j >= r_beg) continue;  // inside a touched row: the row's wave writes it
                const uint32_t o = j + shift;
                if (o < entries_after) {
                    new_nbrs[o] = nbrs[j];
                    if (kMap) map[o] = j;
                }
            }
        }
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_ins = ctr->n_ins, n_del = ctr->n_del;
    const uint32_t waves = (gridDim.x - copy_blocks) * (kBlock / 64);
    for (uint32_t t = (blockIdx.x - copy_blocks) * (kBlock / 64) + (threadIdx.x >> 6); t < nt; t += waves) {
        const uint32_t x = rows[t];
        const uint32_t st = adj_start[x], d = adj_deg[x], nst = new_start[x], nd = new_deg[x];
        const ukey kx = (ukey)x << 32;
        const uint32_t ia = key_lower_bound(ikeys, 0, n_ins, kx), ib = key_lower_bound(ikeys, ia, n_ins, kx + (1ull << 32));
        const uint32_t da = key_lower_bound(dkeys, 0, n_del, kx), db = key_lower_bound(dkeys, da, n_del, kx + (1ull << 32));
        for (uint32_t base = 0; base < d; base += 64) {  // the old entries that stay
            const uint32_t p = base + lane;
            if (p >= d) continue;
            const uint32_t v = nbrs[st + p];
            const uint32_t ri = key_lower_bound(ikeys, ia, ib, kx | v), rd = key_lower_bound(dkeys, da, db, kx | v);
            if (rd < db && dkeys[rd] == (kx | v)) continue;  // deleted
            const uint32_t o = p + (ri - ia) - (rd - da);
            if (o < nd) {
                new_nbrs[nst + o] = v;
                if (kMap) map[nst + o] = st + p;
            }
        }
        for (uint32_t base = ia; base < ib; base += 64) {  // the inserts
            const uint32_t i = base + lane;
            if (i >= ib) continue;
            const ukey key = ikeys[i];
            const uint32_t rd = key_lower_bound(dkeys, da, db, key);
            const uint32_t o = ipos[i] + (i - ia) - (rd - da);
            if (o < nd) {
                new_nbrs[nst + o] = (uint32_t)key;
                if (kMap) map[nst + o] = GNNPE_NO_ENTRY;
            }
        }
    }
}

// gnnpe_csr_carry_entries: dst[r][j'] = src[r][map[j']], 0 where the map says GNNPE_NO_ENTRY.  A block takes kCarryTile
// consecutive new entries per step, lane t the entries a + t, a + kBlock + t, ...: consecutive lanes hold consecutive j', and
// between two touched rows map[j'] - j' is constant, so the loads of a wave are as consecutive as its stores (one 256- or
// 512-byte run per wave instruction).  The map words are read once and kept in registers across the n_rows rows; the kCarryTile
// / kBlock loads of a row are issued before the first store.  No LDS, no scratch.  A map word >= entries_before never occurs in
// a valid map; it is treated as GNNPE_NO_ENTRY so that no read leaves src.
constexpr uint32_t kCarryPerLane = 4, kCarryTile = kCarryPerLane * kBlock;
template <class T>
__global__ __launch_bounds__(kBlock) void k_carry_entries(uint32_t n_rows, uint32_t entries_before, uint32_t entries_after,
                                                         const uint32_t *__restrict__ map, const T *__restrict__ src, T *__restrict__ dst)
{
    for (uint64_t a = (uint64_t)blockIdx.x * kCarryTile; a < entries_after; a += (uint64_t)gridDim.x * kCarryTile) {
        uint32_t m[kCarryPerLane];
#pragma unroll
        for (uint32_t i = 0; i < kCarryPerLane; i++) {
            const uint64_t j = a + i * kBlock + threadIdx.x;
            m[i] = j < entries_after ? map[j] : GNNPE_NO_ENTRY;
            if (m[i] >= entries_before) m[i] = GNNPE_NO_ENTRY;
        }
        for (uint32_t r = 0; r < n_rows; r++) {
            const T *__restrict__ s = src + (uint64_t)r * entries_before;
            T *__restrict__ d = dst + (uint64_t)r * entries_after;
            T v[kCarryPerLane];
#pragma unroll
            for (uint32_t i = 0; i < kCarryPerLane; i++) v[i] = m[i] != GNNPE_NO_ENTRY ? s[m[i]] : (T)0;
#pragma unroll
            for (uint32_t i = 0; i < kCarryPerLane; i++) {
                const uint64_t j = a + i * kBlock + threadIdx.x;
                if (j < entries_after) d[j] = v[i];
            }
        }
    }
}

// gnnpe_set_vertex_labels: one wave per changed vertex v (each listed once, ids below n), lanes over its row.  labels[v] = the new
// label, and for every entry q = (v -> u) of the row the copy of v's label in u's row: the entry (u -> v) sits at
// adj_start[u] + revpos[q].  Two changed vertices that are neighbours write different words, so nothing is ordered.  A reverse
// position outside u's row (an entry without its mirror) is skipped: no store leaves the row it belongs to.
static __global__ __launch_bounds__(kBlock) void k_set_labels(uint32_t count, const uint32_t *__restrict__ verts,
                                                              const uint32_t *__restrict__ new_labels, const uint32_t *__restrict__ adj_start,
                                                              const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                              const uint32_t *__restrict__ revpos, uint32_t *__restrict__ labels,
                                                              uint32_t *__restrict__ nbr_label)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (kBlock / 64);
    for (uint32_t t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < count; t += waves) {
        const uint32_t v = verts[t], lab = new_labels[t];
        const uint32_t st = adj_start[v], d = adj_deg[v];
        if (lane == 0) labels[v] = lab;
        for (uint32_t i = lane; i < d; i += 64) {
            const uint32_t u = nbrs[st + i], r = revpos[st + i];
            if (r < adj_deg[u]) nbr_label[adj_start[u] + r] = lab;
        }
    }
}

// pairs -> the two directed keys of each; a loop or an id >= n is refused
static int directed_keys(const char *who, const char *what, uint32_t n, const uint32_t *edges, uint64_t n_edges, std::vector<ukey> *keys)
{
    keys->resize(2 * n_edges);
    for (uint64_t i = 0; i < n_edges; i++) {
        const uint32_t x = edges[2 * i], y = edges[2 * i + 1];
        GNNPE_REQUIRE(x != y, GNNPE_ERR_ARG, "%s: %s (%u, %u) is a loop", who, what, x, y);
        GNNPE_REQUIRE(x < n && y < n, GNNPE_ERR_ARG, "%s: %s (%u, %u) names a vertex the graph does not have (n = %u)", who, what, x, y, n);
        (*keys)[2 * i] = ((ukey)x << 32) | y;
        (*keys)[2 * i + 1] = ((ukey)y << 32) | x;
    }
    return GNNPE_OK;
}

// sorted and unique on the stream: in -> out (tmp: a list of the same length), the unique count to *d_count
static int sort_unique(gnnpe_ctx *c, ukey *in, ukey *tmp, ukey *out, uint32_t count, uint32_t *d_count)
{
    if (count == 0) return GNNPE_OK;  // (the counter block was cleared)
    size_t tb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, in, tmp, (int)count, 0, 64, c->stream));
    int rc = c->cub_tmp.reserve(tb);
    if (rc) return rc;
    tb = c->cub_tmp.bytes;
    GNNPE_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->cub_tmp.p, tb, in, tmp, (int)count, 0, 64, c->stream));
    tb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, tb, tmp, out, d_count, (int)count, c->stream));
    if ((rc = c->cub_tmp.reserve(tb))) return rc;
    tb = c->cub_tmp.bytes;
    GNNPE_HIP_TRY(hipcub::DeviceSelect::Unique(c->cub_tmp.p, tb, tmp, out, d_count, (int)count, c->stream));
    return GNNPE_OK;
}

}  // namespace gnnpe

using namespace gnnpe;

// The body of gnnpe_csr_apply_edges and gnnpe_csr_apply_edges_map.  want_map: the merge also writes the entry map into
// c->upd_map and a success marks it valid for the new rows; the empty batch writes the identity map.
static int apply_edges(gnnpe_ctx *c, const char *who, bool want_map, const uint32_t *insert_edges, uint64_t n_insert, const uint32_t *delete_edges,
                       uint64_t n_delete, uint64_t *n_entries_after, double *device_ms)
{
    GNNPE_REQUIRE(c && (insert_edges || n_insert == 0) && (delete_edges || n_delete == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    if (device_ms) *device_ms = 0.0;
    int rc = require_whole_graph(who, c);
    if (rc) return rc;
    const uint32_t n = c->n;
    const uint64_t entries = c->nbr_used;
    if (n_entries_after) *n_entries_after = entries;
    if (n_insert == 0 && n_delete == 0) {  // nothing changes; without the map nothing is launched
        if (!want_map) return GNNPE_OK;
        GNNPE_HIP_TRY(hipSetDevice(c->device));
        if ((rc = c->upd_map.reserve((entries + 1) * 4))) return rc;
        LaunchTimer timer;
        if ((rc = timer.begin(device_ms, c->stream))) return rc;
        if (entries) {
            hipLaunchKernelGGL(k_map_identity, dim3(std::min<int>(grid_for(entries), c->num_cus * 8)), dim3(kBlock), 0, c->stream, (uint32_t)entries,
                               c->upd_map.as<uint32_t>());
            GNNPE_HIP_TRY(hipGetLastError());
        }
        if ((rc = timer.end(c->stream))) return rc;
        c->map_valid = true;
        c->map_gen = c->graph_gen;
        c->map_before = c->map_after = entries;
        return GNNPE_OK;
    }
    GNNPE_REQUIRE(n_insert < (1ull << 30) && n_delete < (1ull << 30), GNNPE_ERR_ARG, "%s: %llu + %llu pairs, the key lists are 32-bit", who,
                  (unsigned long long)n_insert, (unsigned long long)n_delete);
    std::vector<ukey> hi, hd;
    if ((rc = directed_keys(who, "insertion", n, insert_edges, n_insert, &hi)) || (rc = directed_keys(who, "deletion", n, delete_edges, n_delete, &hd)))
        return rc;
    const uint32_t cap_ins = (uint32_t)hi.size(), cap_del = (uint32_t)hd.size();
    // the bound of the 32-bit offsets and of sets_first_level_shift.  Repeats aside the new graph has entries + cap_ins - (unique
    // delete keys) entries; only where the cheap bound fails is the exact number worked out here (a refused batch is refused below)
    uint64_t most = entries + cap_ins;
    if (most + n >= (1ull << 32)) {
        std::vector<ukey> ui(hi), ud(hd);
        std::sort(ui.begin(), ui.end());
        std::sort(ud.begin(), ud.end());
        most = entries + (std::unique(ui.begin(), ui.end()) - ui.begin()) - std::min<uint64_t>(entries, std::unique(ud.begin(), ud.end()) - ud.begin());
        GNNPE_REQUIRE(most + n < (1ull << 32), GNNPE_ERR_RANGE, "%s: %llu entries + %u vertices exceed 32-bit addressing", who,
                      (unsigned long long)most, n);
        most = entries + cap_ins;
    }
    GNNPE_HIP_TRY(hipSetDevice(c->device));

    // the spare arrays and the batch's work area: [counters | keys in, sorted, unique: 3 lists each | ipos | cnt | offs | rows | touched]
    const size_t n_rows_cap = std::min<uint64_t>(n, (uint64_t)cap_ins + cap_del);
    const size_t work_bytes = 64 + 3 * 8 * ((size_t)cap_ins + cap_del) + 4 * (size_t)cap_ins + 2 * 4 * ((size_t)n + 1) + 4 * (n_rows_cap + 1) + n + 1;
    if ((rc = c->upd_start.reserve(((size_t)n + 1) * 4)) || (rc = c->upd_deg.reserve(((size_t)n + 1) * 4)) ||
        (rc = c->upd_nbrs.reserve((most + 1) * 4)) || (rc = c->upd_work.reserve(work_bytes)) || (want_map && (rc = c->upd_map.reserve((most + 1) * 4))))
        return rc;
    DevBuf fresh_revpos, fresh_label;  // a buffer that has to grow: allocated aside, so that a refusal by the device loses nothing
    if ((rc = grow_aside(c->revpos, fresh_revpos, (most + 1) * 4)) || (rc = grow_aside(c->nbr_label, fresh_label, (most + 1) * 4))) return rc;
    UpdateCounters *ctr = c->upd_work.as<UpdateCounters>();
    static_assert(sizeof(UpdateCounters) <= 64, "the counter block is the work area's first 64 bytes");
    ukey *ik_in = reinterpret_cast<ukey *>(c->upd_work.as<char>() + 64), *ik_tmp = ik_in + cap_ins, *ikeys = ik_tmp + cap_ins;
    ukey *dk_in = ikeys + cap_ins, *dk_tmp = dk_in + cap_del, *dkeys = dk_tmp + cap_del;
    uint32_t *ipos = reinterpret_cast<uint32_t *>(dkeys + cap_del), *cnt = ipos + cap_ins, *offs = cnt + n + 1, *rows = offs + n + 1;
    uint8_t *touched = reinterpret_cast<uint8_t *>(rows + n_rows_cap + 1);

    UpdateEvents E;
    const bool timed = device_ms != nullptr || c->sw.debug;
    if (timed)
        for (hipEvent_t &e : E.ev) GNNPE_HIP_TRY(hipEventCreate(&e));
    if (cap_ins) GNNPE_HIP_TRY(hipMemcpyAsync(ik_in, hi.data(), (size_t)cap_ins * 8, hipMemcpyHostToDevice, c->stream));
    if (cap_del) GNNPE_HIP_TRY(hipMemcpyAsync(dk_in, hd.data(), (size_t)cap_del * 8, hipMemcpyHostToDevice, c->stream));
    if (timed) GNNPE_HIP_TRY(hipEventRecord(E.ev[0], c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(ctr, 0, 16, c->stream));
    GNNPE_HIP_TRY(hipMemsetAsync(&ctr->bad_insert, 0xFF, 24, c->stream));
    if ((rc = sort_unique(c, ik_in, ik_tmp, ikeys, cap_ins, &ctr->n_ins)) || (rc = sort_unique(c, dk_in, dk_tmp, dkeys, cap_del, &ctr->n_del))) return rc;
    hipLaunchKernelGGL(k_update_check, dim3((cap_ins + cap_del + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, cap_ins, cap_del, ikeys, dkeys,
                       c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), ipos, ctr);
    hipLaunchKernelGGL(k_update_degrees, dim3(grid_for((uint64_t)n + 1)), dim3(kBlock), 0, c->stream, n, c->adj_deg.as<uint32_t>(), ikeys, dkeys,
                       ctr, cnt, touched);
    GNNPE_HIP_TRY(hipGetLastError());
    size_t tb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, offs, (int64_t)n + 1, c->stream));
    if ((rc = c->cub_tmp.reserve(tb))) return rc;
    tb = c->cub_tmp.bytes;
    GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tb, cnt, offs, (int64_t)n + 1, c->stream));
    hipLaunchKernelGGL(k_update_total, dim3(1), dim3(1), 0, c->stream, n, offs, ctr);
    // (present is 1 for every vertex of a whole graph: the kernel writes what is there)
    hipLaunchKernelGGL(k_offsets_to_start_deg, dim3(grid_for(n)), dim3(kBlock), 0, c->stream, n, offs, c->upd_start.as<uint32_t>(),
                       c->upd_deg.as<uint32_t>(), c->present.as<uint8_t>());
    GNNPE_HIP_TRY(hipGetLastError());
    hipcub::CountingInputIterator<uint32_t> ids(0);
    tb = 0;
    GNNPE_HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, tb, ids, touched, rows, &ctr->n_touched, (int)n, c->stream));
    if ((rc = c->cub_tmp.reserve(tb))) return rc;
    tb = c->cub_tmp.bytes;
    GNNPE_HIP_TRY(hipcub::DeviceSelect::Flagged(c->cub_tmp.p, tb, ids, touched, rows, &ctr->n_touched, (int)n, c->stream));
    // a third of the resident grid streams the stretches; a wave per touched row
    const uint32_t copy_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((entries + kMergeTile - 1) / kMergeTile, (uint64_t)c->num_cus * 8));
    const uint32_t row_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_rows_cap + kBlock / 64 - 1) / (kBlock / 64), (uint64_t)c->num_cus * 16));
    if (want_map)
        hipLaunchKernelGGL(k_csr_merge<true>, dim3(copy_blocks + row_blocks), dim3(kBlock), 0, c->stream, copy_blocks, (uint32_t)entries,
                           c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->upd_start.as<uint32_t>(),
                           c->upd_deg.as<uint32_t>(), c->upd_nbrs.as<uint32_t>(), rows, ikeys, dkeys, ipos, ctr, c->upd_map.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_csr_merge<false>, dim3(copy_blocks + row_blocks), dim3(kBlock), 0, c->stream, copy_blocks, (uint32_t)entries,
                           c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->upd_start.as<uint32_t>(),
                           c->upd_deg.as<uint32_t>(), c->upd_nbrs.as<uint32_t>(), rows, ikeys, dkeys, ipos, ctr, (uint32_t *)nullptr);
    GNNPE_HIP_TRY(hipGetLastError());
    if (timed) GNNPE_HIP_TRY(hipEventRecord(E.ev[1], c->stream));
    // the call's wait: the decision is taken here, before anything of the context changes
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, ctr, sizeof(UpdateCounters), hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    const UpdateCounters R = *reinterpret_cast<const UpdateCounters *>(c->h_pinned);
    GNNPE_REQUIRE(R.bad_both == kNoKey, GNNPE_ERR_ARG, "%s: edge (%u, %u) is in both lists", who, (uint32_t)(R.bad_both >> 32), (uint32_t)R.bad_both);
    GNNPE_REQUIRE(R.bad_insert == kNoKey, GNNPE_ERR_ARG, "%s: insertion (%u, %u) is already an edge of the graph", who,
                  (uint32_t)(R.bad_insert >> 32), (uint32_t)R.bad_insert);
    GNNPE_REQUIRE(R.bad_delete == kNoKey, GNNPE_ERR_ARG, "%s: deletion (%u, %u) is not an edge of the graph", who,
                  (uint32_t)(R.bad_delete >> 32), (uint32_t)R.bad_delete);
    const uint64_t m2 = R.entries_after;
    GNNPE_REQUIRE(m2 == entries + R.n_ins - R.n_del && m2 <= most, GNNPE_ERR_HIP, "%s: internal error: %llu entries after %llu + %u - %u", who,
                  (unsigned long long)m2, (unsigned long long)entries, R.n_ins, R.n_del);

    // the swap, then exactly the tail of gnnpe_load_csr
    c->graph_gen++;
    if (want_map) {  // (the map's words are in place: the wait above was behind the merge)
        c->map_valid = true;
        c->map_gen = c->graph_gen;
        c->map_before = entries;
        c->map_after = m2;
    }
    swap_buffers(c->adj_start, c->upd_start);
    swap_buffers(c->adj_deg, c->upd_deg);
    swap_buffers(c->nbrs, c->upd_nbrs);
    if (fresh_revpos.p) swap_buffers(c->revpos, fresh_revpos);
    if (fresh_label.p) swap_buffers(c->nbr_label, fresh_label);
    if (timed) GNNPE_HIP_TRY(hipEventRecord(E.ev[2], c->stream));
    if (n) GNNPE_HIP_TRY(hipMemcpyAsync(c->owned.p, c->present.p, n, hipMemcpyDeviceToDevice, c->stream));
    c->have_graph = false;
    c->nbr_used = c->nbr_owned = m2;
    c->nbr_cap = c->nbrs.bytes / 4;
    if ((rc = finish_rows(c, n, nullptr))) return rc;
    if (m2)
        hipLaunchKernelGGL(k_gather_u32, dim3(grid_for(m2)), dim3(kBlock), 0, c->stream, m2, c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(),
                           c->nbr_label.as<uint32_t>());
    GNNPE_HIP_TRY(hipGetLastError());
    c->have_graph = true;
    c->slab_begin = 0;
    c->slab_end = n;
    c->slab_set = false;
    c->have_order = false;
    invalidate_derived(c);
    if (n_entries_after) *n_entries_after = m2;
    if (timed) {
        GNNPE_HIP_TRY(hipEventRecord(E.ev[3], c->stream));
        GNNPE_HIP_TRY(hipEventSynchronize(E.ev[3]));
        float all = 0.f, build = 0.f, rebuild = 0.f;
        GNNPE_HIP_TRY(hipEventElapsedTime(&all, E.ev[0], E.ev[3]));
        GNNPE_HIP_TRY(hipEventElapsedTime(&build, E.ev[0], E.ev[1]));
        GNNPE_HIP_TRY(hipEventElapsedTime(&rebuild, E.ev[2], E.ev[3]));
        if (device_ms) *device_ms = all;
        // build: the keys to the merge; wait: the counters' read-back and the host's decision; rebuild: owned, finish_rows, the labels
        if (c->sw.debug)
            fprintf(stderr, "[apply_edges] keys=%u+%u touched=%u entries=%llu->%llu device_ms=%.4f build_ms=%.4f wait_ms=%.4f rebuild_ms=%.4f\n",
                    R.n_ins, R.n_del, R.n_touched, (unsigned long long)entries, (unsigned long long)m2, all, build, all - build - rebuild, rebuild);
    }
    return GNNPE_OK;
}

extern "C" int gnnpe_csr_apply_edges(gnnpe_ctx *c, const uint32_t *insert_edges, uint64_t n_insert, const uint32_t *delete_edges,
                                     uint64_t n_delete, uint64_t *n_entries_after, double *device_ms)
{
    if (c) c->map_valid = false;  // the entry map belongs to gnnpe_csr_apply_edges_map's batch
    return apply_edges(c, "gnnpe_csr_apply_edges", false, insert_edges, n_insert, delete_edges, n_delete, n_entries_after, device_ms);
}

extern "C" int gnnpe_csr_apply_edges_map(gnnpe_ctx *c, const uint32_t *insert_edges, uint64_t n_insert, const uint32_t *delete_edges,
                                         uint64_t n_delete, uint64_t *n_entries_before, uint64_t *n_entries_after, void **dev_map,
                                         double *device_ms)
{
    const char *who = "gnnpe_csr_apply_edges_map";
    if (dev_map) *dev_map = nullptr;
    if (c) {
        c->map_valid = false;  // whatever happens below, the map of an earlier batch is gone
        if (n_entries_before) *n_entries_before = c->nbr_used;
        if (n_entries_after) *n_entries_after = c->nbr_used;
    }
    GNNPE_REQUIRE(c && dev_map, GNNPE_ERR_ARG, "%s: null argument", who);
    const int rc = apply_edges(c, who, true, insert_edges, n_insert, delete_edges, n_delete, n_entries_after, device_ms);
    if (rc) {
        c->map_valid = false;
        return rc;
    }
    if (n_entries_before) *n_entries_before = c->map_before;
    *dev_map = c->upd_map.p;
    return GNNPE_OK;
}

// The body of gnnpe_csr_carry_entries and gnnpe_csr_carry_vertices: the same gather, through the entry map or the vertex map
// (`before` / `after`: the columns of src / dst; a map word of 0xFFFFFFFF -- GNNPE_NO_ENTRY, GNNPE_NO_VERTEX -- gives 0).
static int carry_through(gnnpe_ctx *c, const char *who, const uint32_t *map, uint64_t before, uint64_t after, uint32_t n_rows, uint32_t elem_bytes,
                         const void *dev_src, void *dev_dst, double *device_ms)
{
    GNNPE_REQUIRE(elem_bytes == 4 || elem_bytes == 8, GNNPE_ERR_ARG, "%s: elem_bytes %u, 4 or 8 expected", who, elem_bytes);
    if (n_rows == 0 || after == 0) return GNNPE_OK;
    const uint64_t src_bytes = (uint64_t)n_rows * before * elem_bytes, dst_bytes = (uint64_t)n_rows * after * elem_bytes;
    GNNPE_REQUIRE(dev_dst && (dev_src || src_bytes == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    const uintptr_t s = (uintptr_t)dev_src, d = (uintptr_t)dev_dst;
    GNNPE_REQUIRE(s % elem_bytes == 0 && d % elem_bytes == 0, GNNPE_ERR_ARG, "%s: a table is not aligned to its %u-byte cells", who, elem_bytes);
    GNNPE_REQUIRE(src_bytes == 0 || s + src_bytes <= d || d + dst_bytes <= s, GNNPE_ERR_ARG, "%s: src and dst overlap", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    LaunchTimer timer;
    int rc = timer.begin(device_ms, c->stream);
    if (rc) return rc;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((after + kCarryTile - 1) / kCarryTile, (uint64_t)c->num_cus * 8);
    if (elem_bytes == 8)
        hipLaunchKernelGGL(k_carry_entries<uint64_t>, dim3(grid), dim3(kBlock), 0, c->stream, n_rows, (uint32_t)before, (uint32_t)after,
                           map, static_cast<const uint64_t *>(dev_src), static_cast<uint64_t *>(dev_dst));
    else
        hipLaunchKernelGGL(k_carry_entries<uint32_t>, dim3(grid), dim3(kBlock), 0, c->stream, n_rows, (uint32_t)before, (uint32_t)after,
                           map, static_cast<const uint32_t *>(dev_src), static_cast<uint32_t *>(dev_dst));
    GNNPE_HIP_TRY(hipGetLastError());
    return timer.end(c->stream);
}

extern "C" int gnnpe_csr_carry_entries(gnnpe_ctx *c, uint32_t n_rows, uint32_t elem_bytes, const void *dev_src, void *dev_dst, double *device_ms)
{
    const char *who = "gnnpe_csr_carry_entries";
    GNNPE_REQUIRE(c, GNNPE_ERR_ARG, "%s: null argument", who);
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c->map_valid && c->map_gen == c->graph_gen && c->have_graph, GNNPE_ERR_ARG,
                  "%s: the context has no valid entry map (gnnpe_csr_apply_edges_map makes one; loading or changing the rows ends it)", who);
    return carry_through(c, who, c->upd_map.as<uint32_t>(), c->map_before, c->map_after, n_rows, elem_bytes, dev_src, dev_dst, device_ms);
}

// (the vertex map of csrc/gnnpe_update_vertices.hip; the kernel is k_carry_entries: a vertex table has n columns where an entry
// table has offsets[n])
extern "C" int gnnpe_csr_carry_vertices(gnnpe_ctx *c, uint32_t n_rows, uint32_t elem_bytes, const void *dev_src, void *dev_dst, double *device_ms)
{
    const char *who = "gnnpe_csr_carry_vertices";
    GNNPE_REQUIRE(c, GNNPE_ERR_ARG, "%s: null argument", who);
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c->vmap_valid && c->vmap_gen == c->graph_gen && c->have_graph, GNNPE_ERR_ARG,
                  "%s: the context has no valid vertex map (gnnpe_csr_apply_vertices makes one; loading or changing the rows ends it)", who);
    return carry_through(c, who, c->upd_vmap.as<uint32_t>(), c->vmap_before, c->vmap_after, n_rows, elem_bytes, dev_src, dev_dst, device_ms);
}

extern "C" int gnnpe_set_vertex_labels(gnnpe_ctx *c, const uint32_t *vertices, const uint32_t *labels, uint64_t count, double *device_ms)
{
    const char *who = "gnnpe_set_vertex_labels";
    GNNPE_REQUIRE(c && ((vertices && labels) || count == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    if (device_ms) *device_ms = 0.0;
    int rc = require_whole_graph(who, c);
    if (rc) return rc;
    if (count == 0) return GNNPE_OK;  // nothing changes and nothing is launched
    const uint32_t n = c->n;
    // every (vertex, label) pair once; a vertex with two labels is refused
    std::vector<ukey> pairs(count);
    for (uint64_t i = 0; i < count; i++) {
        GNNPE_REQUIRE(vertices[i] < n, GNNPE_ERR_ARG, "%s: vertex %u is not a vertex of the graph (n = %u)", who, vertices[i], n);
        pairs[i] = ((ukey)vertices[i] << 32) | labels[i];
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const size_t k = pairs.size();
    std::vector<uint32_t> up(2 * k);
    for (size_t i = 0; i < k; i++) {
        GNNPE_REQUIRE(i == 0 || (uint32_t)(pairs[i] >> 32) != (uint32_t)(pairs[i - 1] >> 32), GNNPE_ERR_ARG,
                      "%s: vertex %u is listed with the labels %u and %u", who, (uint32_t)(pairs[i] >> 32), (uint32_t)pairs[i - 1], (uint32_t)pairs[i]);
        up[i] = (uint32_t)(pairs[i] >> 32);
        up[k + i] = (uint32_t)pairs[i];
    }
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->upd_work.reserve(2 * k * 4))) return rc;
    uint32_t *d_verts = c->upd_work.as<uint32_t>(), *d_labels = d_verts + k;
    GNNPE_HIP_TRY(hipMemcpyAsync(d_verts, up.data(), 2 * k * 4, hipMemcpyHostToDevice, c->stream));
    LaunchTimer timer;
    if ((rc = timer.begin(device_ms, c->stream))) return rc;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((k + kBlock / 64 - 1) / (kBlock / 64), (uint64_t)c->num_cus * 16);
    hipLaunchKernelGGL(k_set_labels, dim3(grid), dim3(kBlock), 0, c->stream, (uint32_t)k, d_verts, d_labels, c->adj_start.as<uint32_t>(),
                       c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), c->revpos.as<uint32_t>(), c->labels.as<uint32_t>(),
                       c->nbr_label.as<uint32_t>());
    GNNPE_HIP_TRY(hipGetLastError());
    if ((rc = timer.end(c->stream))) return rc;
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // (the host lists go out of scope)
    // exactly the tail of gnnpe_load_csr; the rows, the reverse positions and the hub list stand
    c->graph_gen++;
    c->slab_begin = 0;
    c->slab_end = n;
    c->slab_set = false;
    c->have_order = false;
    invalidate_derived(c);
    return GNNPE_OK;
}

extern "C" int gnnpe_labels_download(gnnpe_ctx *c, uint32_t *host_labels)
{
    const char *who = "gnnpe_labels_download";
    GNNPE_REQUIRE(c && host_labels, GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = require_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if (c->n) GNNPE_HIP_TRY(hipMemcpyAsync(host_labels, c->labels.p, (size_t)c->n * 4, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    return GNNPE_OK;
}

extern "C" int gnnpe_csr_download(gnnpe_ctx *c, uint32_t *host_offsets, uint32_t *host_nbrs, uint64_t nbrs_cap, uint64_t *n_entries)
{
    const char *who = "gnnpe_csr_download";
    GNNPE_REQUIRE(c && host_offsets && n_entries && (host_nbrs || nbrs_cap == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    *n_entries = 0;
    int rc = require_whole_graph(who, c);
    if (rc) return rc;
    *n_entries = c->nbr_used;
    GNNPE_REQUIRE(c->nbr_used <= nbrs_cap, GNNPE_ERR_ARG, "%s: %llu entries, room for %llu", who, (unsigned long long)c->nbr_used,
                  (unsigned long long)nbrs_cap);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = c->n;
    // the rows of a whole graph lie back to back: offsets[x] = adj_start[x], offsets[n] = the entries
    if (n) GNNPE_HIP_TRY(hipMemcpyAsync(host_offsets, c->adj_start.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (c->nbr_used) GNNPE_HIP_TRY(hipMemcpyAsync(host_nbrs, c->nbrs.p, c->nbr_used * 4, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    host_offsets[n] = (uint32_t)c->nbr_used;
    return GNNPE_OK;
}
