// gnnpe_refine_delta_vertices.hip.h -- what the searches anchored at a set S of data vertices share: k_refine_delta_vertices
// (gnnpe_refine_delta_vertices.hip: the rows of Sset_m(C, S) of include/gnnpe_online.h) and k_refine_delta_vertices_vcount /
// k_refine_delta_vertices_ecount (gnnpe_refine_delta_vertices_counts.hip: its tables VV_m and EV_m).  On the device S as a bitmap;
// on the host the staging of a call, once: the launch list with S n C(u) and the orders anchored at u, the work buffer, the
// reserves, the uploads, and per launch the chunks, the scan and the grid.  An entry adds the kernel a launch starts and what it does
// with the counters.  The text that explains the launches and the charging rule is at the head of gnnpe_refine_delta_vertices.hip.
#pragma once

#include "gnnpe_refine_sets.hip.h"

namespace gnnpe {

// bit v of the set's bitmap; v < n
__device__ __forceinline__ bool vset_has(const uint32_t *__restrict__ sbits, uint32_t v) { return ((sbits[v >> 5] >> (v & 31u)) & 1u) != 0; }

// one lane per id of S (each once): its bit
static __global__ void k_vset_scatter(uint32_t n_ids, const uint32_t *__restrict__ ids, uint32_t n, uint32_t *__restrict__ sbits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ids) return;
    const uint32_t v = ids[i];
    if (v < n) atomicOr(&sbits[v >> 5], 1u << (v & 31u));
}

// Which ids of a list are in which resident set: one lane per (query vertex u, id), the wave's 64 answers one __ballot.
// out[u * chunks + c] = the ids c * 64 .. c * 64 + 63 of the list (every id < n) that are in row u of the bitmap.  grid: a wave per
// (u, c), one writer per word.
static __global__ __launch_bounds__(kBlock) void k_vset_member_of(uint32_t n_ids, const uint32_t *__restrict__ ids, uint32_t nq, uint64_t words,
                                                                  const uint32_t *__restrict__ bitmap, unsigned long long *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t chunks = ((uint64_t)n_ids + 63) / 64, items = chunks * nq;
    uint64_t w = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; w < items; w += nw) {  // wave-uniform: every lane reaches the __ballot
        const uint64_t u = w / chunks, i = (w - u * chunks) * 64 + lane;
        bool in = false;
        if (i < n_ids) {
            const uint32_t v = ids[i];
            in = ((bitmap[u * words + (v >> 5)] >> (v & 31u)) & 1u) != 0;
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) out[w] = m;
    }
}

// the work buffer of a call: [counters 32 B | cand of every launch | item_off of every launch (n_cand + 1 each) | chunks, the same]
struct VerticesWork {
    SetsCounters *ctr;
    uint32_t *cand, *item_off, *chunks;
    static size_t bytes(size_t n_cand_all, size_t n_launch) { return SetsWork::kCtrBytes + (3 * n_cand_all + 2 * n_launch) * 4 + 64; }
    VerticesWork(const DevBuf &b, size_t n_cand_all, size_t n_launch)
        : ctr(b.as<SetsCounters>()), cand(reinterpret_cast<uint32_t *>(b.as<char>() + SetsWork::kCtrBytes)), item_off(cand + n_cand_all),
          chunks(item_off + n_cand_all + n_launch)
    {
    }
};

// one launch: the query vertex u with a start candidate in S, its plan in the order anchored at u, the positions of the
// lower-numbered query vertices, and S n C(u)
struct VerticesLaunch {
    SetsQuery K;
    uint32_t earlier = 0, n_cand = 0, w_shift = 6;
    size_t cand_at = 0, off_at = 0;  // where its candidates / its item offsets and chunk counts begin
};

// a call up to its launch list
struct VerticesPlans {
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    std::vector<uint32_t> ids;       // S ascending, each once
    std::vector<uint32_t> cand_all;  // S n C(u) of every launch, one after the other
    std::vector<VerticesLaunch> L;
    bool nothing = false;  // limit 0, an empty set, an empty S, no vertex of S in any set: nothing is launched
    uint32_t *sbits = nullptr, *d_ids = nullptr;  // S on the device (vertices_reserve)
};

// The resident form of "S n C(u)": the k ids of S go up, k_vset_member_of answers for every (u, id), and nq x ceil(k / 64) words
// come back in one wait -- nothing proportional to n crosses.  The ids and the answers live in the context's q_delta, which
// vertices_reserve sizes again afterwards (grow-only: the call's S lands where these ids were).
static inline int vset_members_resident(gnnpe_ctx *c, const std::vector<uint32_t> &ids, uint32_t nq, uint64_t words, const uint32_t *d_bitmap,
                                        std::vector<unsigned long long> *in_set)
{
    const size_t k = ids.size(), chunks = (k + 63) / 64, ids_bytes = (k * 4 + 7) & ~(size_t)7;
    in_set->assign(chunks * nq, 0ull);
    if (!k) return GNNPE_OK;
    int rc = c->q_delta.reserve(ids_bytes + chunks * nq * 8);
    if (rc) return rc;
    uint32_t *d_ids = c->q_delta.as<uint32_t>();
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(c->q_delta.as<char>() + ids_bytes);
    GNNPE_HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), k * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_vset_member_of, dim3(grid_for((uint64_t)chunks * nq * 64)), dim3(kBlock), 0, c->stream, (uint32_t)k, d_ids, nq, words, d_bitmap,
                       d_out);
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipMemcpyAsync(in_set->data(), d_out, chunks * nq * 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    return GNNPE_OK;
}

// sets_prepare, S as ascending ids -- an id the graph does not have is refused here, before anything is launched -- and the launches
// With `res` (a standing query: the sets are on the device) S n C(u) comes from vset_members_resident and neither the file nor the
// host bitmap is read.
static inline int vertices_plans(const char *who, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                 const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode, VerticesPlans *V,
                                 const SetsResident *res = nullptr)
{
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &V->Q, &V->q, res);
    if (rc) return rc;
    std::string err;
    if (gnnpe_host::delta_vertex_ids(c->n, vertices, n_vertices, &V->ids, &err) != 0) {
        set_error("%s: %s", who, err.c_str());
        return GNNPE_ERR_ARG;
    }
    V->nothing = V->Q.empty || V->ids.empty();
    if (V->nothing) return GNNPE_OK;
    const uint32_t nq = V->Q.nq, n = c->n;
    const uint64_t words = V->Q.words;
    const bool distinct = (mode & GNNPE_MATCH_DISTINCT) != 0, induced = (mode & GNNPE_MATCH_INDUCED) != 0;
    std::vector<unsigned long long> in_set;  // of a resident call: the answers of k_vset_member_of
    const size_t chunks = (V->ids.size() + 63) / 64;
    if (res && (rc = vset_members_resident(c, V->ids, nq, words, res->d_bitmap, &in_set))) return rc;
    for (uint32_t u = 0; u < nq; u++) {
        const size_t before = V->cand_all.size();
        for (size_t i = 0; i < V->ids.size(); i++) {
            const uint32_t s = V->ids[i];
            if (res ? (in_set[u * chunks + i / 64] >> (i & 63u)) & 1ull : (candidate_bitmap[(size_t)u * words + (s >> 5)] >> (s & 31u)) & 1u)
                V->cand_all.push_back(s);
        }
        if (V->cand_all.size() == before) continue;
        gnnpe_host::MatchOrder mo;
        if (gnnpe_host::build_match_order_from_vertex(V->q, u, &mo, &err) != 0) {
            set_error("%s: %s", who, err.c_str());
            return GNNPE_ERR_ARG;
        }
        V->L.emplace_back();
        VerticesLaunch &l = V->L.back();
        sets_plan_from_order(V->q, mo, distinct, induced, c->sw.sets_trim, &l.K);
        for (uint32_t d = 1; d < nq; d++)
            if (l.K.P.qv[d] < u) l.earlier |= 1u << d;
        l.n_cand = (uint32_t)(V->cand_all.size() - before);
        l.cand_at = before;
        l.off_at = before + (V->L.size() - 1);
        // the first-level chunk width, as sets_stage_items chooses it
        const bool forced = c->sw.sets_first_shift >= 0 && c->nbr_used + n < (1ull << 32);
        l.w_shift = forced ? (uint32_t)c->sw.sets_first_shift : sets_first_level_shift(l.n_cand, c->nbr_used, n, c->num_cus, c->n_hub);
    }
    V->nothing = V->L.empty();  // no vertex of S is in any set
    return GNNPE_OK;
}

// context-owned, grow-only: the work areas of every launch, the bitmap, S (its bitmap, then its ids), the scan's temporary storage
// for the longest list -- all before the first launch (an entry reserves its rows or its table beside them)
// (a cursor hands in its own buffers in the place of the context's q_work, q_bitmap, q_delta and q_tmp)
static inline int vertices_reserve(gnnpe_ctx *c, VerticesPlans *V, DevBuf *work = nullptr, DevBuf *bm = nullptr, DevBuf *fset = nullptr,
                                   DevBuf *tmp = nullptr, const SetsResident *res = nullptr)
{
    DevBuf &b_work = work ? *work : c->q_work, &b_bm = bm ? *bm : c->q_bitmap, &b_set = fset ? *fset : c->q_delta, &b_tmp = tmp ? *tmp : c->q_tmp;
    const uint32_t nq = V->Q.nq;
    const uint64_t words = V->Q.words;
    size_t tmp_bytes = 0;
    for (const VerticesLaunch &l : V->L) {
        size_t tb = 0;
        GNNPE_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(l.n_cand + 1), c->stream));
        tmp_bytes = std::max(tmp_bytes, tb);
    }
    int rc;
    if ((rc = b_work.reserve(VerticesWork::bytes(V->cand_all.size(), V->L.size()))) || (!res && (rc = b_bm.reserve((size_t)nq * words * 4))) ||
        (rc = b_set.reserve((words + V->ids.size()) * 4)) || (nq > 1 && (rc = b_tmp.reserve(tmp_bytes))))
        return rc;
    V->sbits = b_set.as<uint32_t>();
    V->d_ids = V->sbits + words;
    return GNNPE_OK;
}

// the uploads, the zeroed counters, the start of the timed span, then inside it the zeroing of `zero` (a context-owned table; may
// be null) and S as a bitmap.  With `res` the sets are on the device already and no bitmap goes up.
static inline void vertices_stage(SetsCall &call, gnnpe_ctx *c, const VerticesPlans &V, const uint32_t *candidate_bitmap, void *zero = nullptr,
                                  size_t zero_bytes = 0, const DevBuf *work = nullptr, const DevBuf *bm = nullptr, const SetsResident *res = nullptr)
{
    const size_t n_cand_all = V.cand_all.size(), n_ids = V.ids.size();
    const uint64_t words = V.Q.words;
    const VerticesWork W(work ? *work : c->q_work, n_cand_all, V.L.size());
    uint32_t *sbits = V.sbits, *d_ids = V.d_ids;
    if (call.ok()) call.he = hipMemcpyAsync(W.cand, V.cand_all.data(), n_cand_all * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemcpyAsync(d_ids, V.ids.data(), n_ids * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok() && !res) call.he = hipMemcpyAsync((bm ? *bm : c->q_bitmap).p, candidate_bitmap, (size_t)V.Q.nq * words * 4, hipMemcpyHostToDevice, c->stream);
    if (call.ok()) call.he = hipMemsetAsync(W.ctr, 0, SetsWork::kCtrBytes, c->stream);
    if (call.ok() && call.ev0) call.he = hipEventRecord(call.ev0, c->stream);
    if (call.ok() && zero_bytes) call.he = hipMemsetAsync(zero, 0, zero_bytes, c->stream);  // once per call, before the first launch
    if (call.ok()) call.he = hipMemsetAsync(sbits, 0, words * 4, c->stream);
    const uint32_t n = c->n;
    call.launch([&] {
        hipLaunchKernelGGL(k_vset_scatter, dim3((uint32_t)((n_ids + 255) / 256)), dim3(256), 0, c->stream, (uint32_t)n_ids, d_ids, n, sbits);
    });
}

// the launches, all against one counter block: per launch the chunks, the scan and the grid, then
// launch(k, l, blocks, cand, item_off, ord...) starts the entry's kernel with the plan l.K.P and its pack
template <class Launch>
static inline void vertices_launches(SetsCall &call, gnnpe_ctx *c, const VerticesPlans &V, Launch &&launch)
{
    const uint32_t nq = V.Q.nq;
    const VerticesWork W(c->q_work, V.cand_all.size(), V.L.size());
    for (size_t k = 0; k < V.L.size(); k++) {
        const VerticesLaunch &l = V.L[k];
        uint32_t *cand = W.cand + l.cand_at, *item_off = W.item_off + l.off_at, *chunks = W.chunks + l.off_at;
        if (k && call.ok()) call.he = hipMemsetAsync(&W.ctr->ticket, 0, 4, c->stream);  // the next launch's tickets, and nothing else
        if (nq > 1) {
            call.launch([&] {
                hipLaunchKernelGGL(k_sets_cand_chunks, dim3((l.n_cand + 256) / 256), dim3(256), 0, c->stream, l.n_cand, cand,
                                   c->adj_deg.as<uint32_t>(), l.w_shift, chunks);
            });
            size_t tb = c->q_tmp.bytes;
            if (call.ok()) call.he = hipcub::DeviceScan::ExclusiveSum(c->q_tmp.p, tb, chunks, item_off, (int)(l.n_cand + 1), c->stream);
        }
        // a resident grid; without hub rows a start candidate has at most 64 >> w_shift chunks, and a launch needs no more waves than items
        uint64_t blocks = sets_grid_blocks(c, nq, l.n_cand);
        if (nq > 1 && c->n_hub == 0)
            blocks = std::min<uint64_t>(blocks, (((uint64_t)l.n_cand << (6 - std::min(l.w_shift, 6u))) + kSetsWavesPerBlock - 1) / kSetsWavesPerBlock);
        call.launch([&] { sets_dispatch(l.K, [&](auto... ord) { launch(k, l, (uint32_t)blocks, cand, item_off, ord...); }); });
    }
}

}  // namespace gnnpe
