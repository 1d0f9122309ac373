// gnnpe_filter.hip -- SURVEY 8(f) row 4: the online FILTER, data side.
//
// The reference answers a query by walking each partition's R*-tree best-first (Partition::query,
// GNN-PE/include/custom.h:366-489); the traversal only prunes -- what it reports is defined by its leaf test
// (custom.h:404-431): data path p matches query path j iff, position by position, labels are equal and the query
// degree does not exceed the data degree, and in no embedding dimension the query's pde exceeds the data pde by
// more than epsilon; each match inserts p's vertices into the candidate sets of j's vertices (custom.h:429-432),
// and the sets of all partitions are united (main.cpp:165-171).  On the GPU the index is unnecessary: the test
// is applied to every enumerated path, 2e8 paths against a plan of a few query paths in a few milliseconds,
// with no files, no R-tree and no 100-second text re-parse (custom.h:546-572) in between -- and without emitting a
// single path: the test is fused into the enumeration itself (k_filter_starts).
// Candidate sets are bitmaps: row u (query vertex) x ceil(n/32) words, bit v = data vertex v is a candidate.
#include "gnnpe_common.h"

namespace gnnpe {

constexpr int kMaxPlan = 512;  // query paths held in LDS

// One wave per start vertex s of the slab.  A pair (s, b) is dropped as soon as no plan path begins with
// (label s, label b) within the two degrees -- with |labels|^2 label pairs and a handful of plan paths that is almost
// every pair, before the row of b is touched.  Only the surviving pairs scan N(b): c is kept iff rank[c] > rank[s]
// (the enumeration's rule, custom.h:66-92 in closed form), then the full leaf test runs.  Needs the CSR rows of the
// slab and its 1-hop halo, labels, ranks, vde and every vertex' degree; no counts, no records, any degree, any e.
__global__ __launch_bounds__(256) void k_filter_starts(uint32_t slab_begin, uint32_t slab_len,
                                                       const uint32_t *__restrict__ sorted,
                                                       const uint32_t *__restrict__ adj_start,
                                                       const uint32_t *__restrict__ adj_deg,
                                                       const uint32_t *__restrict__ nbrs,
                                                       const uint32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ rank, const uint32_t *__restrict__ deg,
                                                       const double *__restrict__ vde, uint32_t e, uint32_t n_qp,
                                                       const uint32_t *__restrict__ q_vids,
                                                       const uint32_t *__restrict__ q_labels,
                                                       const uint32_t *__restrict__ q_deg,
                                                       const double *__restrict__ q_pde, double eps, uint64_t words,
                                                       uint32_t *__restrict__ bitmap)
{
    __shared__ uint32_t s_lab[kMaxPlan * 3], s_deg[kMaxPlan * 3], s_vid[kMaxPlan * 3];
    for (uint32_t i = threadIdx.x; i < n_qp * 3; i += blockDim.x) {
        s_lab[i] = q_labels[i];
        s_deg[i] = q_deg[i];
        s_vid[i] = q_vids[i];
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    uint64_t w = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; w < slab_len; w += nw) {
        const uint32_t thr = slab_begin + (uint32_t)w, s = sorted[thr];
        const uint32_t a_s = adj_start[s], ds = adj_deg[s], ls = labels[s];
        bool any = false;  // wave-uniform: does any plan path start like s?
        for (uint32_t j = 0; j < n_qp && !any; j++) any = s_lab[j * 3] == ls && s_deg[j * 3] <= ds;
        if (!any) continue;
        for (uint32_t k0 = 0; k0 < ds; k0 += 64) {
            const uint32_t k = k0 + lane;
            uint32_t b = 0, lb = 0, db = 0;
            bool hit = false;
            if (k < ds) {
                b = nbrs[a_s + k];
                lb = labels[b];
                db = deg[b];
                for (uint32_t j = 0; j < n_qp && !hit; j++)
                    hit = s_lab[j * 3] == ls && s_lab[j * 3 + 1] == lb && s_deg[j * 3] <= ds && s_deg[j * 3 + 1] <= db;
            }
            uint64_t live = __ballot(hit);
            while (live) {  // surviving pairs, one at a time, the row of b over the lanes
                const int kk = __ffsll((long long)live) - 1;
                live &= live - 1;
                const uint32_t bb = (uint32_t)__builtin_amdgcn_readlane((int)b, kk);
                const uint32_t lbb = (uint32_t)__builtin_amdgcn_readlane((int)lb, kk);
                const uint32_t dbb = (uint32_t)__builtin_amdgcn_readlane((int)db, kk);
                const uint32_t b_st = adj_start[bb], b_d = adj_deg[bb];
                for (uint32_t j0 = 0; j0 < b_d; j0 += 64) {
                    if (j0 + lane >= b_d) continue;
                    const uint32_t c = nbrs[b_st + j0 + lane];
                    if (rank[c] <= thr) continue;  // not emitted from s: c == s, or the path belongs to start c
                    const uint32_t lc = labels[c];
                    for (uint32_t q = 0; q < n_qp; q++) {
                        if (s_lab[q * 3] != ls || s_lab[q * 3 + 1] != lbb || s_lab[q * 3 + 2] != lc) continue;  // custom.h:410
                        if (s_deg[q * 3] > ds || s_deg[q * 3 + 1] > dbb || s_deg[q * 3 + 2] > deg[c]) continue;
                        bool ok = true;
                        const double *qp = q_pde + (uint64_t)q * 3 * e;
                        for (uint32_t t = 0; t < e && ok; t++) {                                              // custom.h:420-426
                            const double a0 = vde[(uint64_t)s * e + t], a1 = vde[(uint64_t)bb * e + t], a2 = vde[(uint64_t)c * e + t];
                            if (qp[t] > a0 && fabs(qp[t] - a0) > eps) ok = false;
                            if (qp[e + t] > a1 && fabs(qp[e + t] - a1) > eps) ok = false;
                            if (qp[2 * e + t] > a2 && fabs(qp[2 * e + t] - a2) > eps) ok = false;
                        }
                        if (!ok) continue;
                        atomicOr(&bitmap[s_vid[q * 3] * words + (s >> 5)], 1u << (s & 31u));                // custom.h:429-432
                        atomicOr(&bitmap[s_vid[q * 3 + 1] * words + (bb >> 5)], 1u << (bb & 31u));
                        atomicOr(&bitmap[s_vid[q * 3 + 2] * words + (c >> 5)], 1u << (c & 31u));
                    }
                }
            }
        }
    }
}

// ---- exact mode: the orientation-complete filter ----------------------------------------------------------
// The reference keeps every simple path in one orientation, on both sides (custom.h:66-92, :94-119), and compares position by
// position: a query path (A, B, C) whose image in the data graph is stored as (c, b, a) never matches it.  Exact mode tests
// every plan path in both orientations (gnnpe_filter_candidates_exact adds the reverses), so that C(u), the union over the plan
// paths through u of the data vertices at u's position in a passing data path, holds f(u) for EVERY embedding f:
//   - f maps the query path (u0 .. uk) onto a simple data path (f(u0) .. f(uk)); it is enumerated in one of its orientations,
//     and the plan holds the query path in that same orientation;
//   - labels are equal, and f maps N(u) injectively into N(f(u)), so deg(u) <= deg(f(u));
//   - gen_vde_x is non-negative (custom.h:492-511: uniform [0, 1) draws, L1-normalised), so vde(f(u)) = x(f(u)) + the sum of x
//     over N(f(u)) is at least vde(u) = x(u) + the sum over f(N(u)), dimension by dimension: the leaf test
//     (q > d && |q - d| > eps rejects) passes at every position.
// A query vertex on no plan path gets the same three tests on its own (k_filter_vertices).
constexpr int kPrefixQueue = 128;  // (b, c) prefixes queued per wave; drained from 64 on, so one ballot's survivors always fit

__device__ __forceinline__ void set_candidate(uint32_t *bitmap, uint64_t words, uint32_t u, uint32_t v)
{
    uint32_t *p = bitmap + u * words + (v >> 5);
    const uint32_t bit = 1u << (v & 31u);
    if (!(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(p, bit);  // most bits are set already
}

// 4-vertex paths (l = 3).  One wave per start vertex s of the slab, pruned level by level so that a row is read only for a
// prefix some plan path still matches:
//   (s)        lanes over the plan: label, degree and vde of s against position 0
//   (s, b)     lanes over N(s): labels and degrees of positions 0-1; survivors ballot-compacted, taken one at a time
//   (s, b, c)  lanes over N(b), c != s: labels and degrees of positions 0-2; survivors queued in LDS (per wave)
//   d in N(c)  lanes over the row, d not in {s, b}, rank[d] > rank[s]: the full leaf test (custom.h:404-431) at 4 positions
// Orientation: the plan holds every query path and its reverse, and the enumeration keeps its one-orientation rule (a simple
// path is visited from the end that comes first in the processing order, the closed form of the DFS + hash set at depth 3).
// Visiting every simple 4-walk from both ends instead would be the same work with half the plan, but the rule is what lets a
// slab context hold truncated halo rows: the rows of c need no entry ranked below the slab (gnnpe_rows_append's min_rank).
// Reads the rows of the slab and of its 2-hop halo, the vde of every vertex up to three hops out (d), labels, ranks and every
// vertex' degree; any degree (rows > 64 entries are walked 64 at a time at every level), any e.
__global__ __launch_bounds__(256) void k_filter_starts4(uint32_t slab_begin, uint32_t slab_len,
                                                        const uint32_t *__restrict__ sorted,
                                                        const uint32_t *__restrict__ adj_start,
                                                        const uint32_t *__restrict__ adj_deg,
                                                        const uint32_t *__restrict__ nbrs,
                                                        const uint32_t *__restrict__ labels,
                                                        const uint32_t *__restrict__ rank, const uint32_t *__restrict__ deg,
                                                        const double *__restrict__ vde, uint32_t e, uint32_t n_qp,
                                                        const uint32_t *__restrict__ q_vids,
                                                        const uint32_t *__restrict__ q_labels,
                                                        const uint32_t *__restrict__ q_deg,
                                                        const double *__restrict__ q_pde, double eps, uint64_t words,
                                                        uint32_t *__restrict__ bitmap)
{
    __shared__ uint32_t s_lab[kMaxPlan * 4], s_deg[kMaxPlan * 4], s_vid[kMaxPlan * 4];
    __shared__ uint32_t s_qb[kBlock / 64][kPrefixQueue], s_qc[kBlock / 64][kPrefixQueue];
    for (uint32_t i = threadIdx.x; i < n_qp * 4; i += blockDim.x) {
        s_lab[i] = q_labels[i];
        s_deg[i] = q_deg[i];
        s_vid[i] = q_vids[i];
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    uint32_t *qb = s_qb[threadIdx.x >> 6], *qc = s_qc[threadIdx.x >> 6];
    uint64_t w = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; w < slab_len; w += nw) {
        const uint32_t thr = slab_begin + (uint32_t)w, s = sorted[thr];
        const uint32_t a_s = adj_start[s], ns = adj_deg[s], ls = labels[s], ds = deg[s];
        const double *vs = vde + (uint64_t)s * e;
        bool any = false;  // (s), wave-uniform
        for (uint32_t j0 = 0; j0 < n_qp && !any; j0 += 64) {
            const uint32_t j = j0 + lane;
            bool ok = j < n_qp && s_lab[j * 4] == ls && s_deg[j * 4] <= ds;
            const double *qp = q_pde + (uint64_t)j * 4 * e;
            for (uint32_t t = 0; t < e && ok; t++)
                if (qp[t] > vs[t] && fabs(qp[t] - vs[t]) > eps) ok = false;
            any = __ballot(ok) != 0;
        }
        if (!any) continue;
        // the leaf level over the queued prefixes; lanes independent (no cross-lane operation inside)
        auto drain = [&](uint32_t qn) {
            __builtin_amdgcn_wave_barrier();  // the queue was written by other lanes of this wave
            for (uint32_t i = 0; i < qn; i++) {
                const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)qb[i]);
                const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)qc[i]);
                const uint32_t lb = labels[b], db = deg[b], lc = labels[c], dc = deg[c];
                const uint32_t c_st = adj_start[c], nc = adj_deg[c];
                for (uint32_t k = lane; k < nc; k += 64) {
                    const uint32_t d = nbrs[c_st + k];
                    if (d == s || d == b || rank[d] <= thr) continue;  // not simple, or the path belongs to start d
                    const uint32_t ld = labels[d], dd = deg[d];
                    for (uint32_t q = 0; q < n_qp; q++) {
                        const uint32_t *ql = s_lab + q * 4, *qd = s_deg + q * 4;
                        if (ql[0] != ls || ql[1] != lb || ql[2] != lc || ql[3] != ld) continue;  // custom.h:410
                        if (qd[0] > ds || qd[1] > db || qd[2] > dc || qd[3] > dd) continue;
                        bool ok = true;
                        const double *qp = q_pde + (uint64_t)q * 4 * e;
                        for (uint32_t t = 0; t < e && ok; t++) {  // custom.h:420-426
                            const double a0 = vs[t], a1 = vde[(uint64_t)b * e + t], a2 = vde[(uint64_t)c * e + t],
                                         a3 = vde[(uint64_t)d * e + t];
                            if (qp[t] > a0 && fabs(qp[t] - a0) > eps) ok = false;
                            if (qp[e + t] > a1 && fabs(qp[e + t] - a1) > eps) ok = false;
                            if (qp[2 * e + t] > a2 && fabs(qp[2 * e + t] - a2) > eps) ok = false;
                            if (qp[3 * e + t] > a3 && fabs(qp[3 * e + t] - a3) > eps) ok = false;
                        }
                        if (!ok) continue;
                        set_candidate(bitmap, words, s_vid[q * 4], s);
                        set_candidate(bitmap, words, s_vid[q * 4 + 1], b);
                        set_candidate(bitmap, words, s_vid[q * 4 + 2], c);
                        set_candidate(bitmap, words, s_vid[q * 4 + 3], d);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();  // every lane has read the queue before it is written again
        };
        uint32_t qn = 0;  // queued prefixes, wave-uniform
        for (uint32_t k0 = 0; k0 < ns; k0 += 64) {
            const uint32_t k = k0 + lane;
            uint32_t b = 0, lb = 0, db = 0;
            bool hit = false;
            if (k < ns) {
                b = nbrs[a_s + k];
                lb = labels[b];
                db = deg[b];
                for (uint32_t j = 0; j < n_qp && !hit; j++)
                    hit = s_lab[j * 4] == ls && s_lab[j * 4 + 1] == lb && s_deg[j * 4] <= ds && s_deg[j * 4 + 1] <= db;
            }
            uint64_t live = __ballot(hit);
            while (live) {  // surviving (s, b), one at a time, the row of b over the lanes
                const int kk = __ffsll((long long)live) - 1;
                live &= live - 1;
                const uint32_t bb = (uint32_t)__builtin_amdgcn_readlane((int)b, kk);
                const uint32_t lbb = (uint32_t)__builtin_amdgcn_readlane((int)lb, kk);
                const uint32_t dbb = (uint32_t)__builtin_amdgcn_readlane((int)db, kk);
                const uint32_t b_st = adj_start[bb], nb = adj_deg[bb];
                for (uint32_t j0 = 0; j0 < nb; j0 += 64) {
                    const uint32_t jj = j0 + lane;
                    uint32_t c = 0;
                    bool ok = false;
                    if (jj < nb) {
                        c = nbrs[b_st + jj];
                        if (c != s) {
                            const uint32_t lc = labels[c], dc = deg[c];
                            for (uint32_t q = 0; q < n_qp && !ok; q++)
                                ok = s_lab[q * 4] == ls && s_lab[q * 4 + 1] == lbb && s_lab[q * 4 + 2] == lc &&
                                     s_deg[q * 4] <= ds && s_deg[q * 4 + 1] <= dbb && s_deg[q * 4 + 2] <= dc;
                        }
                    }
                    const uint64_t m = __ballot(ok);
                    if (ok) {
                        const uint32_t slot =
                            qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        qb[slot] = bb;
                        qc[slot] = c;
                    }
                    qn += (uint32_t)__popcll(m);
                    if (qn >= 64) {
                        drain(qn);
                        qn = 0;
                    }
                }
            }
        }
        if (qn) drain(qn);
    }
}

// Query vertices on no plan path: label, degree and vde dominance (the leaf test at one position), one lane per data vertex of
// the slab (rank in [slab_begin, slab_end): a slab context holds the vde of its own vertices).  The wave's 64 results for a query
// vertex are one __ballot OR-ed into two bitmap words by lane 0: one writer per word, as in k_pge_filter.
__global__ __launch_bounds__(256) void k_filter_vertices(uint32_t n, uint32_t slab_begin, uint32_t slab_end,
                                                         const uint32_t *__restrict__ rank,
                                                         const uint32_t *__restrict__ labels,
                                                         const uint32_t *__restrict__ deg, const double *__restrict__ vde,
                                                         uint32_t e, uint32_t n_qv, const uint32_t *__restrict__ q_vids,
                                                         const uint32_t *__restrict__ q_labels,
                                                         const uint32_t *__restrict__ q_deg,
                                                         const double *__restrict__ q_vde, double eps, uint64_t words,
                                                         uint32_t *__restrict__ bitmap)
{
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t chunks = ((uint64_t)n + 63) / 64;
    uint64_t c = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; c < chunks; c += nw) {  // wave-uniform: every lane reaches each __ballot
        const uint64_t v = c * 64 + lane;
        const uint32_t r = v < n ? rank[v] : 0u;
        const bool in = v < n && r >= slab_begin && r < slab_end;
        const uint32_t lv = in ? labels[v] : 0u, dv = in ? deg[v] : 0u;
        for (uint32_t u = 0; u < n_qv; u++) {
            bool ok = in && lv == q_labels[u] && q_deg[u] <= dv;
            const double *qv = q_vde + (uint64_t)u * e, *dvde = vde + v * e;
            for (uint32_t t = 0; t < e && ok; t++)
                if (qv[t] > dvde[t] && fabs(qv[t] - dvde[t]) > eps) ok = false;
            const uint64_t m = __ballot(ok);
            if (lane == 0 && m) {
                uint32_t *row = bitmap + (uint64_t)q_vids[u] * words;
                row[2 * c] |= (uint32_t)m;
                if (2 * c + 1 < words) row[2 * c + 1] |= (uint32_t)(m >> 32);
            }
        }
    }
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" {

int gnnpe_set_degrees(gnnpe_ctx *c, const uint32_t *host_degrees)
{
    GNNPE_REQUIRE(c && host_degrees && c->have_graph, GNNPE_ERR_ARG, "gnnpe_set_degrees: load the rows first");
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->deg_all.reserve(((size_t)c->n + 1) * 4))) return rc;
    GNNPE_HIP_TRY(hipMemcpyAsync(c->deg_all.p, host_degrees, (size_t)c->n * 4, hipMemcpyHostToDevice, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_deg_all = true;
    c->aux_vdl_valid = false;
    return GNNPE_OK;
}

int gnnpe_filter_candidates(gnnpe_ctx *c, uint32_t n_paths, const uint32_t *q_vids, const uint32_t *q_labels,
                            const uint32_t *q_degrees, const double *q_pde, uint32_t n_query_vertices, double epsilon,
                            uint32_t *host_bitmap, double *device_ms)
{
    GNNPE_REQUIRE(c && host_bitmap && n_query_vertices, GNNPE_ERR_ARG, "gnnpe_filter_candidates: null argument");
    GNNPE_REQUIRE(n_paths == 0 || (q_vids && q_labels && q_degrees && q_pde), GNNPE_ERR_ARG, "null query plan");
    GNNPE_REQUIRE(n_paths <= (uint32_t)kMaxPlan, GNNPE_ERR_UNSUPPORTED, "query plan of %u paths (limit %d)", n_paths, kMaxPlan);
    GNNPE_REQUIRE(c->have_graph && c->have_order && c->have_vde, GNNPE_ERR_ARG,
                  "gnnpe_filter_candidates: needs the graph, the order (gnnpe_set_order) and gnnpe_vde");
    GNNPE_REQUIRE(c->rows_identity || c->have_deg_all, GNNPE_ERR_UNSUPPORTED,
                  "the filter needs every vertex' degree: load the whole graph (gnnpe_load_csr) or call gnnpe_set_degrees");
    for (uint32_t i = 0; i < n_paths * 3; i++)
        GNNPE_REQUIRE(q_vids[i] < n_query_vertices, GNNPE_ERR_ARG, "query path vertex %u >= %u", q_vids[i], n_query_vertices);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint32_t e = c->e;
    const uint64_t words = ((uint64_t)c->n + 31) / 32, bm_bytes = (uint64_t)n_query_vertices * words * 4;
    DevBuf &plan = c->q_plan, &bm = c->q_bitmap;  // context-owned: a query allocates nothing new
    int rc;
    const size_t np3 = (size_t)n_paths * 3;
    if ((rc = plan.reserve(np3 * 12 + np3 * e * 8 + 64)) || (rc = bm.reserve(std::max<uint64_t>(bm_bytes, 4)))) return rc;
    double *d_pde = plan.as<double>();  // doubles first (alignment), then the three uint32 arrays
    uint32_t *d_vids = reinterpret_cast<uint32_t *>(d_pde + np3 * e), *d_lab = d_vids + np3, *d_deg = d_lab + np3;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t he = hipSuccess;
    if (np3) {
        he = hipMemcpyAsync(d_pde, q_pde, np3 * e * 8, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(d_vids, q_vids, np3 * 4, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(d_lab, q_labels, np3 * 4, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(d_deg, q_degrees, np3 * 4, hipMemcpyHostToDevice, c->stream);
    }
    if (he == hipSuccess) he = hipMemsetAsync(bm.p, 0, std::max<uint64_t>(bm_bytes, 4), c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);  // the plan arrays are caller memory
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev0);
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev1);
    if (he == hipSuccess && device_ms) he = hipEventRecord(ev0, c->stream);
    rc = GNNPE_OK;
    const uint32_t len = c->slab_end - c->slab_begin;
    if (he == hipSuccess && n_paths && len) {
        hipLaunchKernelGGL(k_filter_starts, dim3(grid_for((uint64_t)len * 64)), dim3(256), 0, c->stream, c->slab_begin, len,
                           c->sorted.as<uint32_t>(), c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->rank.as<uint32_t>(),
                           c->have_deg_all ? c->deg_all.as<uint32_t>() : c->adj_deg.as<uint32_t>(), c->vde.as<double>(), e,
                           n_paths, d_vids, d_lab, d_deg, d_pde, epsilon, words, bm.as<uint32_t>());
        he = hipGetLastError();
    }
    if (he == hipSuccess && !rc && device_ms) he = hipEventRecord(ev1, c->stream);
    if (he == hipSuccess && !rc) he = hipMemcpyAsync(host_bitmap, bm.p, bm_bytes, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess && !rc) he = hipStreamSynchronize(c->stream);
    if (he == hipSuccess && !rc && device_ms) {
        float ms = 0.f;
        he = hipEventElapsedTime(&ms, ev0, ev1);
        *device_ms = ms;
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipStreamSynchronize(c->stream);
    if (!rc && he != hipSuccess) {
        set_error("gnnpe_filter_candidates: %s", hipGetErrorString(he));
        rc = GNNPE_ERR_HIP;
    }
    return rc;
}


int gnnpe_filter_candidates_exact(gnnpe_ctx *c, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                                  const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                                  uint32_t n_query_vertices, double epsilon, uint32_t *host_bitmap, double *device_ms)
{
    GNNPE_REQUIRE(c && counts && host_bitmap && n_query_vertices, GNNPE_ERR_ARG, "gnnpe_filter_candidates_exact: null argument");
    GNNPE_REQUIRE(l == 2 || l == 3, GNNPE_ERR_UNSUPPORTED, "gnnpe_filter_candidates_exact: l = %u (2 or 3)", l);
    GNNPE_REQUIRE(l == 3 || counts[1] == 0, GNNPE_ERR_ARG, "gnnpe_filter_candidates_exact: 3-vertex complement paths at l = 2");
    const uint32_t W = l + 1;
    const uint64_t n_in = (uint64_t)counts[0] * W + (uint64_t)counts[1] * 3 + counts[2];
    GNNPE_REQUIRE(n_in == 0 || (q_vids && q_labels && q_degrees && q_pde), GNNPE_ERR_ARG, "null query plan");
    // both orientations of every path: the limit of the kernels' LDS plan holds after doubling
    GNNPE_REQUIRE(2ull * counts[0] <= (uint64_t)kMaxPlan && 2ull * counts[1] <= (uint64_t)kMaxPlan, GNNPE_ERR_UNSUPPORTED,
                  "exact query plan of %u + %u paths, %u + %u with their reverses (limit %d per width)", counts[0], counts[1],
                  2 * counts[0], 2 * counts[1], kMaxPlan);
    GNNPE_REQUIRE(counts[2] <= n_query_vertices, GNNPE_ERR_ARG, "%u single query vertices of %u", counts[2], n_query_vertices);
    GNNPE_REQUIRE(c->have_graph && c->have_order && c->have_vde, GNNPE_ERR_ARG,
                  "gnnpe_filter_candidates_exact: needs the graph, the order (gnnpe_set_order) and gnnpe_vde");
    GNNPE_REQUIRE(c->rows_identity || c->have_deg_all, GNNPE_ERR_UNSUPPORTED,
                  "the filter needs every vertex' degree: load the whole graph (gnnpe_load_csr) or call gnnpe_set_degrees");
    for (uint64_t i = 0; i < n_in; i++)
        GNNPE_REQUIRE(q_vids[i] < n_query_vertices, GNNPE_ERR_ARG, "query path vertex %u >= %u", q_vids[i], n_query_vertices);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint32_t e = c->e;
    // the doubled plan on the host: part 0 (width W), its reverses, part 1 (width 3), its reverses, then the single vertices;
    // a reversed path lists its positions backwards, each position's e pde values in their order
    const uint32_t n0 = 2 * counts[0], n1 = 2 * counts[1], n2 = counts[2];
    const size_t T = (size_t)n0 * W + (size_t)n1 * 3 + n2;
    std::vector<uint32_t> hv(T), hl(T), hd(T);
    std::vector<double> hp(T * e);
    size_t o = 0;
    const uint64_t in1 = (uint64_t)counts[0] * W, in2 = in1 + (uint64_t)counts[1] * 3;
    auto put = [&](uint64_t src) {  // one position of the caller's plan
        hv[o] = q_vids[src];
        hl[o] = q_labels[src];
        hd[o] = q_degrees[src];
        memcpy(&hp[o * e], q_pde + src * e, (size_t)e * 8);
        o++;
    };
    for (int rev = 0; rev < 2; rev++)
        for (uint32_t p = 0; p < counts[0]; p++)
            for (uint32_t j = 0; j < W; j++) put((uint64_t)p * W + (rev ? W - 1 - j : j));
    for (int rev = 0; rev < 2; rev++)
        for (uint32_t p = 0; p < counts[1]; p++)
            for (uint32_t j = 0; j < 3; j++) put(in1 + (uint64_t)p * 3 + (rev ? 2 - j : j));
    for (uint32_t i = 0; i < n2; i++) put(in2 + i);
    const uint64_t words = ((uint64_t)c->n + 31) / 32, bm_bytes = (uint64_t)n_query_vertices * words * 4;
    DevBuf &plan = c->q_plan, &bm = c->q_bitmap;
    int rc;
    if ((rc = plan.reserve(T * 12 + T * e * 8 + 64)) || (rc = bm.reserve(std::max<uint64_t>(bm_bytes, 4)))) return rc;
    double *d_pde = plan.as<double>();  // doubles first (alignment), then the three uint32 arrays
    uint32_t *d_vids = reinterpret_cast<uint32_t *>(d_pde + T * e), *d_lab = d_vids + T, *d_deg = d_lab + T;
    const size_t off1 = (size_t)n0 * W, off2 = off1 + (size_t)n1 * 3;  // first entry of parts 1 and 2
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t he = hipSuccess;
    if (T) {
        he = hipMemcpyAsync(d_pde, hp.data(), T * e * 8, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(d_vids, hv.data(), T * 4, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(d_lab, hl.data(), T * 4, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(d_deg, hd.data(), T * 4, hipMemcpyHostToDevice, c->stream);
    }
    if (he == hipSuccess) he = hipMemsetAsync(bm.p, 0, std::max<uint64_t>(bm_bytes, 4), c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);  // the host arrays are locals
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev0);
    if (he == hipSuccess && device_ms) he = hipEventCreate(&ev1);
    if (he == hipSuccess && device_ms) he = hipEventRecord(ev0, c->stream);
    const uint32_t len = c->slab_end - c->slab_begin;
    const uint32_t *deg = c->have_deg_all ? c->deg_all.as<uint32_t>() : c->adj_deg.as<uint32_t>();
    // the launches share the bitmap on one stream: the path kernels' atomics, then the single vertices' OR-ed words
    if (he == hipSuccess && len && n0 && l == 2) {
        hipLaunchKernelGGL(k_filter_starts, dim3(grid_for((uint64_t)len * 64)), dim3(256), 0, c->stream, c->slab_begin, len,
                           c->sorted.as<uint32_t>(), c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->rank.as<uint32_t>(), deg, c->vde.as<double>(), e,
                           n0, d_vids, d_lab, d_deg, d_pde, epsilon, words, bm.as<uint32_t>());
        he = hipGetLastError();
    }
    if (he == hipSuccess && len && n0 && l == 3) {
        hipLaunchKernelGGL(k_filter_starts4, dim3(grid_for((uint64_t)len * 64)), dim3(256), 0, c->stream, c->slab_begin, len,
                           c->sorted.as<uint32_t>(), c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->rank.as<uint32_t>(), deg, c->vde.as<double>(), e,
                           n0, d_vids, d_lab, d_deg, d_pde, epsilon, words, bm.as<uint32_t>());
        he = hipGetLastError();
    }
    if (he == hipSuccess && len && n1) {
        hipLaunchKernelGGL(k_filter_starts, dim3(grid_for((uint64_t)len * 64)), dim3(256), 0, c->stream, c->slab_begin, len,
                           c->sorted.as<uint32_t>(), c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(),
                           c->nbrs.as<uint32_t>(), c->labels.as<uint32_t>(), c->rank.as<uint32_t>(), deg, c->vde.as<double>(), e,
                           n1, d_vids + off1, d_lab + off1, d_deg + off1, d_pde + off1 * e, epsilon, words, bm.as<uint32_t>());
        he = hipGetLastError();
    }
    if (he == hipSuccess && len && n2) {
        hipLaunchKernelGGL(k_filter_vertices, dim3(grid_for(((uint64_t)c->n + 63) / 64 * 64)), dim3(256), 0, c->stream, c->n,
                           c->slab_begin, c->slab_end, c->rank.as<uint32_t>(), c->labels.as<uint32_t>(), deg,
                           c->vde.as<double>(), e, n2, d_vids + off2, d_lab + off2, d_deg + off2, d_pde + off2 * e, epsilon,
                           words, bm.as<uint32_t>());
        he = hipGetLastError();
    }
    if (he == hipSuccess && device_ms) he = hipEventRecord(ev1, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(host_bitmap, bm.p, bm_bytes, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if (he == hipSuccess && device_ms) {
        float ms = 0.f;
        he = hipEventElapsedTime(&ms, ev0, ev1);
        *device_ms = ms;
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipStreamSynchronize(c->stream);
    if (he != hipSuccess) {
        set_error("gnnpe_filter_candidates_exact: %s", hipGetErrorString(he));
        return GNNPE_ERR_HIP;
    }
    return GNNPE_OK;
}

}  // extern "C"
