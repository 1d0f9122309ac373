// gnnpe_filter_support.hip -- the support table of the exact online filter (include/gnnpe_hip.h, "filter support tables").
//
// gnnpe_filter_candidates_exact (gnnpe_filter.hip) sets bit v of row u when SOME passing data path puts v at a position of u: a
// union, which an update of the graph cannot patch -- a deletion may take the last path away.  S[u][v] counts those paths, and a
// count can be patched: the paths whose existence or test result an update changes all contain a touched vertex, so
//     S -= S_T(G);  update;  gnnpe_vde;  S += S_T(G');  bitmap = (S != 0)
// with T the touched vertices keeps S exact (the three loops and why their T suffices: the header).
//
// What is counted: DIRECTED simple data paths against the plan AS LISTED (no reverses).  An undirected path in one orientation
// against the plan doubled with its reverses -- what k_filter_starts / k_filter_starts4 enumerate -- is the same multiset of
// (plan path, position, data vertex) triples, so S[u][v] != 0 exactly where the filter sets the bit; and directed paths need no
// processing order: nothing here reads c->sorted or c->rank.
//
// The charging rule that counts every path of S_T once: a path is charged to the SMALLEST position j with P[j] in T.  A work item
// is (t, j), t in T, one wave: it walks the paths with P[j] = t, to the right of j over any vertex, to the left of j over vertices
// outside T only.  With T = V (the full table) only j = 0 finds anything, and the host launches only that, over all vertices.
// On a graph with rows longer than 64 entries an item is cut into slices: slice s of S takes the chunks s, s + S, ... of t's own
// row (the first position filled), so that a hub in T is walked by up to 64 waves instead of one.
#include "gnnpe_common.h"

#include <algorithm>
#include <type_traits>

namespace gnnpe {

constexpr int kSupportPlan = 256;  // plan paths of one width held in LDS, as listed: the exact filter's 512 after doubling

// the leaf test of gnnpe_filter_candidates in one dimension (custom.h:420-426): does the query's value reject the data's?
__device__ __forceinline__ bool support_dim_rejects(double q, double d, double eps) { return q > d && fabs(q - d) > eps; }

// bit v of T's bitmap, v < n (the idiom of csrc/gnnpe_refine_delta_vertices.hip.h, which belongs to the other library)
__device__ __forceinline__ bool support_in_set(const uint32_t *__restrict__ tbits, uint32_t v) { return ((tbits[v >> 5] >> (v & 31u)) & 1u) != 0; }

// one lane per id of T (each once, every id < n: the host has checked): its bit
__global__ void k_support_set_scatter(uint32_t n_ids, const uint32_t *__restrict__ ids, uint32_t *__restrict__ tbits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ids) atomicOr(&tbits[ids[i] >> 5], 1u << (ids[i] & 31u));
}

// the k-th position an item anchored at J fills: J, then rightwards to W - 1, then leftwards from J - 1 to 0
template <int W, int J> __host__ __device__ constexpr int support_pos(int k) { return k <= W - 1 - J ? J + k : W - 1 - k; }

// what a wave carries through the walk; P / L / D: vertex, label and degree of the positions filled so far, wave-uniform
template <int W> struct SupportWalk {
    const uint32_t *adj_start, *adj_deg, *nbrs, *labels, *tbits;
    const double *vde, *q_pde;
    const uint32_t *s_lab, *s_deg, *s_vid;  // the plan part in LDS
    unsigned long long *cnt;                // this wave's passing paths per plan path (LDS): the anchor's cells
    uint32_t e, n_qp;
    double eps;
    uint64_t n, sign;
    unsigned long long *table;
    unsigned lane;
    uint32_t slice, n_slices;  // of the anchor's own row (the first position filled): this wave takes every n_slices-th chunk
    uint32_t P[W], L[W], D[W];
};

// Fills position support_pos(K) from the row of its filled neighbour position, lanes over the row 64 entries at a time.  A vertex
// already on the path is dropped, and to the left of the anchor a vertex of T (the path belongs to that vertex' item).  Before
// the last position: the candidate is kept iff some plan path still fits the labels and degrees chosen so far -- before its row
// is read -- and the survivors of a __ballot are taken one at a time.  At the last position: the leaf test against every plan path;
// the cells of the wave-uniform positions get the number of passing lanes once (the anchor's: into `cnt`, flushed per item).
template <int W, int J, int K> __device__ __forceinline__ void support_extend(SupportWalk<W> &S)
{
    constexpr int pos = support_pos<W, J>(K), src = pos > J ? pos - 1 : pos + 1;
    constexpr bool left = pos < J, last = K == W - 1;
    const uint32_t a = S.adj_start[S.P[src]], d = S.D[src];
    const uint32_t first = K == 1 ? S.slice * 64 : 0, step = K == 1 ? S.n_slices * 64 : 64;
    for (uint32_t k0 = first; k0 < d; k0 += step) {
        const uint32_t k = k0 + S.lane;
        uint32_t x = 0, lx = 0, dx = 0;
        bool ok = k < d;
        if (ok) {
            x = S.nbrs[a + k];
#pragma unroll
            for (int i = 0; i < K; i++) ok = ok && x != S.P[support_pos<W, J>(i)];
            if (left) ok = ok && !support_in_set(S.tbits, x);
            if (ok) {
                lx = S.labels[x];
                dx = S.adj_deg[x];
            }
        }
        if constexpr (!last) {
            if (ok) {
                bool hit = false;
                for (uint32_t q = 0; q < S.n_qp && !hit; q++) {
                    hit = S.s_lab[q * W + pos] == lx && S.s_deg[q * W + pos] <= dx;
#pragma unroll
                    for (int i = 0; i < K; i++) {
                        const int p = support_pos<W, J>(i);
                        hit = hit && S.s_lab[q * W + p] == S.L[p] && S.s_deg[q * W + p] <= S.D[p];
                    }
                }
                ok = hit;
            }
            uint64_t live = __ballot(ok);
            while (live) {
                const int kk = __ffsll((long long)live) - 1;
                live &= live - 1;
                S.P[pos] = (uint32_t)__builtin_amdgcn_readlane((int)x, kk);
                S.L[pos] = (uint32_t)__builtin_amdgcn_readlane((int)lx, kk);
                S.D[pos] = (uint32_t)__builtin_amdgcn_readlane((int)dx, kk);
                support_extend<W, J, K + 1>(S);
            }
        } else {
            for (uint32_t q = 0; q < S.n_qp; q++) {  // wave-uniform: every lane reaches each __ballot
                bool uni = true;                     // the positions filled before: the same answer in every lane
#pragma unroll
                for (int i = 0; i < K; i++) {
                    const int p = support_pos<W, J>(i);
                    uni = uni && S.s_lab[q * W + p] == S.L[p] && S.s_deg[q * W + p] <= S.D[p];
                }
                if (!uni) continue;
                const double *qp = S.q_pde + (uint64_t)q * W * S.e;
#pragma unroll
                for (int i = 0; i < K; i++) {
                    const int p = support_pos<W, J>(i);
                    for (uint32_t t = 0; t < S.e && uni; t++)
                        if (support_dim_rejects(qp[p * S.e + t], S.vde[(uint64_t)S.P[p] * S.e + t], S.eps)) uni = false;
                }
                if (!uni) continue;
                bool pass = ok && S.s_lab[q * W + pos] == lx && S.s_deg[q * W + pos] <= dx;
                for (uint32_t t = 0; t < S.e && pass; t++)
                    if (support_dim_rejects(qp[pos * S.e + t], S.vde[(uint64_t)x * S.e + t], S.eps)) pass = false;
                const uint64_t m = __ballot(pass);
                if (!m) continue;
                const uint64_t c = (uint64_t)__popcll(m);
                if (S.lane == 0) {
#pragma unroll
                    for (int i = 1; i < K; i++) {
                        const int p = support_pos<W, J>(i);
                        atomicAdd(S.table + (uint64_t)S.s_vid[q * W + p] * S.n + S.P[p], (unsigned long long)(S.sign * c));
                    }
                    S.cnt[q] += c;
                }
                if (pass) atomicAdd(S.table + (uint64_t)S.s_vid[q * W + pos] * S.n + x, (unsigned long long)S.sign);
            }
        }
    }
}

// One wave per item and slice: t = ids[item] (ids == nullptr: t = item, the full table's launch) anchored at position J of a path
// of W vertices.  table[u * n + v] += sign * (the paths charged to the item that pass a plan path with u at the position of v).
// Rows of any length, any e; reads rows, labels, degrees and vde of the whole graph, no order.
template <int W, int J>
__global__ __launch_bounds__(256) void k_support_walk(uint32_t n_items, uint32_t n_slices, const uint32_t *__restrict__ ids,
                                                      const uint32_t *__restrict__ tbits, const uint32_t *__restrict__ adj_start,
                                                      const uint32_t *__restrict__ adj_deg, const uint32_t *__restrict__ nbrs,
                                                      const uint32_t *__restrict__ labels, const double *__restrict__ vde, uint32_t e,
                                                      uint32_t n_qp, const uint32_t *__restrict__ q_vids,
                                                      const uint32_t *__restrict__ q_labels, const uint32_t *__restrict__ q_deg,
                                                      const double *__restrict__ q_pde, double eps, uint64_t n, uint64_t sign,
                                                      unsigned long long *__restrict__ table)
{
    __shared__ uint32_t s_lab[kSupportPlan * W], s_deg[kSupportPlan * W], s_vid[kSupportPlan * W];
    __shared__ unsigned long long s_cnt[kBlock / 64][kSupportPlan];
    for (uint32_t i = threadIdx.x; i < n_qp * W; i += blockDim.x) {
        s_lab[i] = q_labels[i];
        s_deg[i] = q_deg[i];
        s_vid[i] = q_vids[i];
    }
    for (uint32_t i = threadIdx.x; i < (kBlock / 64) * kSupportPlan; i += blockDim.x) (&s_cnt[0][0])[i] = 0;
    __syncthreads();
    SupportWalk<W> S;
    S.adj_start = adj_start, S.adj_deg = adj_deg, S.nbrs = nbrs, S.labels = labels, S.tbits = tbits;
    S.vde = vde, S.q_pde = q_pde;
    S.s_lab = s_lab, S.s_deg = s_deg, S.s_vid = s_vid;
    S.cnt = s_cnt[threadIdx.x >> 6];
    S.e = e, S.n_qp = n_qp, S.eps = eps, S.n = n, S.sign = sign, S.table = table;
    S.lane = threadIdx.x & 63u;
    S.n_slices = n_slices;
    uint64_t w = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; w < (uint64_t)n_items * n_slices; w += nw) {  // the slices of an item side by side
        const uint64_t item = w / n_slices;
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ids ? ids[item] : (uint32_t)item));
        S.slice = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w - item * n_slices));
        S.P[J] = t;
        S.L[J] = labels[t];
        S.D[J] = adj_deg[t];
        if ((uint64_t)S.slice * 64 >= S.D[J]) continue;  // no chunk of t's row for this slice (a vertex without a neighbour: no path)
        bool any = false;  // wave-uniform: does t pass position J of any plan path?
        for (uint32_t q0 = 0; q0 < n_qp && !any; q0 += 64) {
            const uint32_t q = q0 + S.lane;
            bool ok = q < n_qp && s_lab[q * W + J] == S.L[J] && s_deg[q * W + J] <= S.D[J];
            const double *qp = q_pde + ((uint64_t)q * W + J) * e;
            for (uint32_t k = 0; k < e && ok; k++)
                if (support_dim_rejects(qp[k], vde[(uint64_t)t * e + k], eps)) ok = false;
            any = __ballot(ok) != 0;
        }
        if (!any) continue;
        support_extend<W, J, 1>(S);
        // the anchor's cells, once per item and plan path; lane 0 wrote the counters
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t q = S.lane; q < n_qp; q += 64) {
            const uint64_t c = S.cnt[q];
            if (c) {
                S.cnt[q] = 0;
                atomicAdd(table + (uint64_t)s_vid[q * W + J] * n + t, (unsigned long long)(sign * c));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// The single entries of the plan: one lane per item t, the leaf test at one position (what k_filter_vertices applies).
__global__ __launch_bounds__(256) void k_support_singles(uint32_t n_items, const uint32_t *__restrict__ ids,
                                                         const uint32_t *__restrict__ labels, const uint32_t *__restrict__ adj_deg,
                                                         const double *__restrict__ vde, uint32_t e, uint32_t n_qv,
                                                         const uint32_t *__restrict__ q_vids, const uint32_t *__restrict__ q_labels,
                                                         const uint32_t *__restrict__ q_deg, const double *__restrict__ q_vde,
                                                         double eps, uint64_t n, uint64_t sign, unsigned long long *__restrict__ table)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t t = ids ? ids[i] : (uint32_t)i;
        const uint32_t lt = labels[t], dt = adj_deg[t];
        for (uint32_t u = 0; u < n_qv; u++) {
            bool ok = lt == q_labels[u] && q_deg[u] <= dt;
            for (uint32_t k = 0; k < e && ok; k++)
                if (support_dim_rejects(q_vde[(uint64_t)u * e + k], vde[(uint64_t)t * e + k], eps)) ok = false;
            if (ok) atomicAdd(table + (uint64_t)q_vids[u] * n + t, (unsigned long long)sign);
        }
    }
}

// bitmap[u][v] = (table[u][v] != 0): a lane per vertex, the wave's 64 answers for a query vertex are one __ballot stored as two
// words by lane 0 -- one writer per word, every word of the bitmap written (k_filter_vertices' shape, stores instead of ORs)
__global__ __launch_bounds__(256) void k_support_bitmap(uint32_t n, uint32_t n_qv, const unsigned long long *__restrict__ table,
                                                        uint64_t words, uint32_t *__restrict__ bitmap)
{
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t chunks = ((uint64_t)n + 63) / 64;
    uint64_t c = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (; c < chunks; c += nw) {  // wave-uniform: every lane reaches each __ballot
        const uint64_t v = c * 64 + lane;
        for (uint32_t u = 0; u < n_qv; u++) {
            const uint64_t m = __ballot(v < n && table[(uint64_t)u * n + v] != 0);
            if (lane == 0) {
                uint32_t *row = bitmap + (uint64_t)u * words;
                row[2 * c] = (uint32_t)m;
                if (2 * c + 1 < words) row[2 * c + 1] = (uint32_t)(m >> 32);
            }
        }
    }
}

// the state the update calls ask for too (gnnpe_update.hip.h): the whole simple graph on the device
static int support_whole_graph(const char *who, gnnpe_ctx *c)
{
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    return GNNPE_OK;
}

// the plan of a call on the device: the caller's arrays as they are (each path once), pde first
struct SupportPlan {
    uint32_t W = 0, n0 = 0, n1 = 0, n2 = 0, e = 0;
    size_t in1 = 0, in2 = 0, total = 0;  // first entry of parts 1 and 2, entries
    double *d_pde = nullptr;
    uint32_t *d_vids = nullptr, *d_lab = nullptr, *d_deg = nullptr;
};

// the refusals of gnnpe_filter_support_exact[_delta] that concern the plan and the context: the plan checks of
// gnnpe_filter_candidates_exact, then the table, the whole simple graph and gnnpe_vde.  Nothing is launched or reserved here.
static int support_check(const char *who, gnnpe_ctx *c, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                         const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde, uint32_t n_query_vertices,
                         const void *dev_table, SupportPlan *P)
{
    GNNPE_REQUIRE(c && counts && n_query_vertices, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(l == 2 || l == 3, GNNPE_ERR_UNSUPPORTED, "%s: l = %u (2 or 3)", who, l);
    GNNPE_REQUIRE(l == 3 || counts[1] == 0, GNNPE_ERR_ARG, "%s: 3-vertex complement paths at l = 2", who);
    const uint32_t W = l + 1;
    const uint64_t n_in = (uint64_t)counts[0] * W + (uint64_t)counts[1] * 3 + counts[2];
    GNNPE_REQUIRE(n_in == 0 || (q_vids && q_labels && q_degrees && q_pde), GNNPE_ERR_ARG, "null query plan");
    // the exact filter's limit, which holds after doubling there: the same plans are accepted and refused
    GNNPE_REQUIRE(2ull * counts[0] <= 2ull * kSupportPlan && 2ull * counts[1] <= 2ull * kSupportPlan, GNNPE_ERR_UNSUPPORTED,
                  "exact query plan of %u + %u paths, %u + %u with their reverses (limit %d per width)", counts[0], counts[1],
                  2 * counts[0], 2 * counts[1], 2 * kSupportPlan);
    GNNPE_REQUIRE(counts[2] <= n_query_vertices, GNNPE_ERR_ARG, "%u single query vertices of %u", counts[2], n_query_vertices);
    for (uint64_t i = 0; i < n_in; i++)
        GNNPE_REQUIRE(q_vids[i] < n_query_vertices, GNNPE_ERR_ARG, "query path vertex %u >= %u", q_vids[i], n_query_vertices);
    GNNPE_REQUIRE(dev_table && (reinterpret_cast<uintptr_t>(dev_table) & 7u) == 0, GNNPE_ERR_ARG,
                  "%s: dev_table must be an 8-byte aligned device pointer", who);
    int rc = support_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_REQUIRE(c->have_table && c->have_vde, GNNPE_ERR_ARG,
                  "%s: needs the label table and gnnpe_vde since the last change of the rows or the labels", who);
    P->W = W, P->n0 = counts[0], P->n1 = counts[1], P->n2 = counts[2], P->e = c->e;
    P->in1 = (size_t)counts[0] * W, P->in2 = P->in1 + (size_t)counts[1] * 3, P->total = (size_t)n_in;
    return GNNPE_OK;
}

// the plan into the context's grow-only buffer; the arrays are the caller's and stay valid until the call's one wait
static hipError_t support_upload(gnnpe_ctx *c, SupportPlan *P, const uint32_t *q_vids, const uint32_t *q_labels,
                                 const uint32_t *q_degrees, const double *q_pde)
{
    const size_t T = P->total, e = P->e;
    P->d_pde = c->q_plan.as<double>();  // doubles first (alignment), then the three uint32 arrays
    P->d_vids = reinterpret_cast<uint32_t *>(P->d_pde + T * e), P->d_lab = P->d_vids + T, P->d_deg = P->d_lab + T;
    if (!T) return hipSuccess;
    hipError_t he = hipMemcpyAsync(P->d_pde, q_pde, T * e * 8, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(P->d_vids, q_vids, T * 4, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(P->d_lab, q_labels, T * 4, hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(P->d_deg, q_degrees, T * 4, hipMemcpyHostToDevice, c->stream);
    return he;
}

template <int W, int J>
static hipError_t support_launch_walk(gnnpe_ctx *c, uint32_t n_items, uint32_t n_slices, const uint32_t *d_ids, const uint32_t *d_tbits,
                                      uint32_t n_qp, size_t off, const SupportPlan &P, double eps, uint64_t sign, unsigned long long *table)
{
    hipLaunchKernelGGL((k_support_walk<W, J>), dim3(grid_for((uint64_t)n_items * n_slices * 64)), dim3(kBlock), 0, c->stream, n_items,
                       n_slices, d_ids, d_tbits, c->adj_start.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(),
                       c->labels.as<uint32_t>(), c->vde.as<double>(), P.e, n_qp, P.d_vids + off, P.d_lab + off, P.d_deg + off,
                       P.d_pde + off * P.e, eps, (uint64_t)c->n, sign, table);
    return hipGetLastError();
}

// every launch of a call: the items (t, j) of each width's part -- anchors [0, n_anchor) -- and the single entries
static hipError_t support_launches(gnnpe_ctx *c, const SupportPlan &P, uint32_t n_items, const uint32_t *d_ids, const uint32_t *d_tbits,
                                   bool all_anchors, double eps, uint64_t sign, unsigned long long *table)
{
    hipError_t he = hipSuccess;
    if (!n_items) return he;
    // slices per item: only where a row can have a second chunk, only for a list (the full table has a wave per vertex to spread
    // its hubs over), and no more than about a million waves, most of which find no chunk and leave at once
    const uint32_t n_slices = d_ids && c->n_hub ? std::min<uint32_t>(64u, std::max<uint32_t>(1u, (1u << 20) / n_items)) : 1u;
    auto go = [&](auto w, auto j, uint32_t n_qp, size_t off) {
        if (he == hipSuccess && n_qp && (all_anchors || decltype(j)::value == 0))
            he = support_launch_walk<decltype(w)::value, decltype(j)::value>(c, n_items, n_slices, d_ids, d_tbits, n_qp, off, P, eps, sign,
                                                                             table);
    };
    using std::integral_constant;
    if (P.W == 3) {
        go(integral_constant<int, 3>{}, integral_constant<int, 0>{}, P.n0, 0);
        go(integral_constant<int, 3>{}, integral_constant<int, 1>{}, P.n0, 0);
        go(integral_constant<int, 3>{}, integral_constant<int, 2>{}, P.n0, 0);
    } else {
        go(integral_constant<int, 4>{}, integral_constant<int, 0>{}, P.n0, 0);
        go(integral_constant<int, 4>{}, integral_constant<int, 1>{}, P.n0, 0);
        go(integral_constant<int, 4>{}, integral_constant<int, 2>{}, P.n0, 0);
        go(integral_constant<int, 4>{}, integral_constant<int, 3>{}, P.n0, 0);
        go(integral_constant<int, 3>{}, integral_constant<int, 0>{}, P.n1, P.in1);  // the 3-vertex complement paths
        go(integral_constant<int, 3>{}, integral_constant<int, 1>{}, P.n1, P.in1);
        go(integral_constant<int, 3>{}, integral_constant<int, 2>{}, P.n1, P.in1);
    }
    if (he == hipSuccess && P.n2) {
        hipLaunchKernelGGL(k_support_singles, dim3(grid_for(n_items)), dim3(kBlock), 0, c->stream, n_items, d_ids,
                           c->labels.as<uint32_t>(), c->adj_deg.as<uint32_t>(), c->vde.as<double>(), P.e, P.n2, P.d_vids + P.in2,
                           P.d_lab + P.in2, P.d_deg + P.in2, P.d_pde + P.in2 * P.e, eps, (uint64_t)c->n, sign, table);
        he = hipGetLastError();
    }
    return he;
}

// the end of a call: the closing event, an optional copy to the host, the ONE host wait, the device time
struct SupportTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~SupportTimer()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    hipError_t begin(bool want, hipStream_t s)
    {
        if (!want) return hipSuccess;
        hipError_t he = hipEventCreate(&ev0);
        if (he == hipSuccess) he = hipEventCreate(&ev1);
        if (he == hipSuccess) he = hipEventRecord(ev0, s);
        return he;
    }
    hipError_t end(hipError_t he, hipStream_t s, double *device_ms, void *host_dst = nullptr, const void *dev_src = nullptr, size_t bytes = 0)
    {
        if (he == hipSuccess && ev1) he = hipEventRecord(ev1, s);
        if (he == hipSuccess && bytes) he = hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s);
        const hipError_t hw = hipStreamSynchronize(s);  // also on an error: the caller's arrays may still be read
        if (he == hipSuccess) he = hw;
        if (he == hipSuccess && ev1) {
            float ms = 0.f;
            he = hipEventElapsedTime(&ms, ev0, ev1);
            *device_ms = ms;
        }
        return he;
    }
};

static int support_result(const char *who, hipError_t he)
{
    if (he == hipSuccess) return GNNPE_OK;
    set_error("%s: %s", who, hipGetErrorString(he));
    return GNNPE_ERR_HIP;
}

// The body of gnnpe_filter_support_exact_delta and gnnpe_filter_support_exact_delta_device after their checks and reserves: the
// plan's upload, then table += sign * S_T with T as the bitmap d_tbits and the ascending ids d_ids.  With host_ids (the host-list call)
// T is put on the device first, into the context's buffers the two pointers name: the upload, a zeroed bitmap, a bit per id.
static int support_delta_run(const char *who, gnnpe_ctx *c, SupportPlan &P, const uint32_t *q_vids, const uint32_t *q_labels,
                             const uint32_t *q_degrees, const double *q_pde, double eps, const uint32_t *host_ids, const uint32_t *d_tbits,
                             const uint32_t *d_ids, uint32_t n_ids, int sign, void *dev_table, double *device_ms)
{
    SupportTimer timer;
    hipError_t he = support_upload(c, &P, q_vids, q_labels, q_degrees, q_pde);
    if (host_ids) {
        const uint64_t words = ((uint64_t)c->n + 31) / 32;
        if (he == hipSuccess) he = hipMemcpyAsync(const_cast<uint32_t *>(d_ids), host_ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) he = timer.begin(device_ms != nullptr, c->stream);
        if (he == hipSuccess) he = hipMemsetAsync(const_cast<uint32_t *>(d_tbits), 0, words * 4, c->stream);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(k_support_set_scatter, dim3((n_ids + 255) / 256), dim3(256), 0, c->stream, n_ids, d_ids, const_cast<uint32_t *>(d_tbits));
            he = hipGetLastError();
        }
    } else if (he == hipSuccess)
        he = timer.begin(device_ms != nullptr, c->stream);
    if (he == hipSuccess)
        he = support_launches(c, P, n_ids, d_ids, d_tbits, true, eps, (uint64_t)(int64_t)sign, static_cast<unsigned long long *>(dev_table));
    return support_result(who, timer.end(he, c->stream, device_ms));
}

}  // namespace gnnpe

using namespace gnnpe;

extern "C" {

int gnnpe_filter_support_exact(gnnpe_ctx *c, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids, const uint32_t *q_labels,
                               const uint32_t *q_degrees, const double *q_pde, uint32_t n_query_vertices, double epsilon,
                               void *dev_table, double *device_ms)
{
    const char *who = "gnnpe_filter_support_exact";
    SupportPlan P;
    int rc = support_check(who, c, l, counts, q_vids, q_labels, q_degrees, q_pde, n_query_vertices, dev_table, &P);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->q_plan.reserve(P.total * 12 + P.total * P.e * 8 + 64))) return rc;
    if (device_ms) *device_ms = 0.0;
    SupportTimer timer;
    hipError_t he = support_upload(c, &P, q_vids, q_labels, q_degrees, q_pde);
    if (he == hipSuccess) he = timer.begin(device_ms != nullptr, c->stream);
    const size_t bytes = (size_t)n_query_vertices * c->n * 8;
    if (he == hipSuccess && bytes) he = hipMemsetAsync(dev_table, 0, bytes, c->stream);
    // T = V: only the items anchored at position 0 can find a path, over all vertices, without a list
    if (he == hipSuccess) he = support_launches(c, P, c->n, nullptr, nullptr, false, epsilon, 1, static_cast<unsigned long long *>(dev_table));
    return support_result(who, timer.end(he, c->stream, device_ms));
}

int gnnpe_filter_support_exact_delta(gnnpe_ctx *c, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                                     const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                                     uint32_t n_query_vertices, double epsilon, const uint32_t *vertices, uint64_t n_vertices, int sign,
                                     void *dev_table, double *device_ms)
{
    const char *who = "gnnpe_filter_support_exact_delta";
    SupportPlan P;
    int rc = support_check(who, c, l, counts, q_vids, q_labels, q_degrees, q_pde, n_query_vertices, dev_table, &P);
    if (rc) return rc;
    GNNPE_REQUIRE(sign == 1 || sign == -1, GNNPE_ERR_ARG, "%s: sign = %d (+1 or -1)", who, sign);
    GNNPE_REQUIRE(vertices || n_vertices == 0, GNNPE_ERR_ARG, "%s: null vertex list of %llu ids", who, (unsigned long long)n_vertices);
    for (uint64_t i = 0; i < n_vertices; i++)
        GNNPE_REQUIRE(vertices[i] < c->n, GNNPE_ERR_ARG, "%s: vertex %u is not a vertex of the graph (n = %u)", who, vertices[i], c->n);
    if (device_ms) *device_ms = 0.0;
    if (n_vertices == 0) return GNNPE_OK;  // nothing is launched, the table's bytes stay
    std::vector<uint32_t> ids(vertices, vertices + n_vertices);  // a repeated id means the vertex once
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const uint32_t n_ids = (uint32_t)ids.size();
    const uint64_t words = ((uint64_t)c->n + 31) / 32;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->q_plan.reserve(P.total * 12 + P.total * P.e * 8 + 64)) || (rc = c->q_work.reserve((words + n_ids) * 4))) return rc;
    uint32_t *d_tbits = c->q_work.as<uint32_t>(), *d_ids = d_tbits + words;
    // T from the host list: its upload, a zeroed bitmap and a bit per id; then the launches the device form makes
    return support_delta_run(who, c, P, q_vids, q_labels, q_degrees, q_pde, epsilon, ids.data(), d_tbits, d_ids, n_ids, sign, dev_table,
                             device_ms);  // `ids` lives until the wait inside
}

int gnnpe_filter_support_exact_delta_device(gnnpe_ctx *c, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                                            const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                                            uint32_t n_query_vertices, double epsilon, const void *dev_bits, const void *dev_ids,
                                            uint64_t n_ids, int sign, void *dev_table, double *device_ms)
{
    const char *who = "gnnpe_filter_support_exact_delta_device";
    SupportPlan P;
    int rc = support_check(who, c, l, counts, q_vids, q_labels, q_degrees, q_pde, n_query_vertices, dev_table, &P);
    if (rc) return rc;
    GNNPE_REQUIRE(sign == 1 || sign == -1, GNNPE_ERR_ARG, "%s: sign = %d (+1 or -1)", who, sign);
    GNNPE_REQUIRE(n_ids <= c->n, GNNPE_ERR_ARG, "%s: %llu ids, the graph has %u vertices", who, (unsigned long long)n_ids, c->n);
    if (device_ms) *device_ms = 0.0;
    if (n_ids == 0) return GNNPE_OK;  // nothing is launched, the table's bytes stay
    GNNPE_REQUIRE(dev_bits && dev_ids && ((reinterpret_cast<uintptr_t>(dev_bits) | reinterpret_cast<uintptr_t>(dev_ids)) & 3u) == 0, GNNPE_ERR_ARG,
                  "%s: dev_bits and dev_ids must be 4-byte aligned device pointers", who);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->q_plan.reserve(P.total * 12 + P.total * P.e * 8 + 64))) return rc;
    return support_delta_run(who, c, P, q_vids, q_labels, q_degrees, q_pde, epsilon, nullptr, static_cast<const uint32_t *>(dev_bits),
                             static_cast<const uint32_t *>(dev_ids), (uint32_t)n_ids, sign, dev_table, device_ms);
}

int gnnpe_filter_support_bitmap(gnnpe_ctx *c, uint32_t n_query_vertices, const void *dev_table, uint32_t *host_bitmap, double *device_ms)
{
    const char *who = "gnnpe_filter_support_bitmap";
    GNNPE_REQUIRE(c && host_bitmap && n_query_vertices, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(dev_table && (reinterpret_cast<uintptr_t>(dev_table) & 7u) == 0, GNNPE_ERR_ARG,
                  "%s: dev_table must be an 8-byte aligned device pointer", who);
    int rc = support_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint64_t words = ((uint64_t)c->n + 31) / 32, bm_bytes = (uint64_t)n_query_vertices * words * 4;
    if ((rc = c->q_bitmap.reserve(std::max<uint64_t>(bm_bytes, 4)))) return rc;
    if (device_ms) *device_ms = 0.0;
    SupportTimer timer;
    hipError_t he = timer.begin(device_ms != nullptr, c->stream);
    if (he == hipSuccess && c->n) {
        hipLaunchKernelGGL(k_support_bitmap, dim3(grid_for(((uint64_t)c->n + 63) / 64 * 64)), dim3(kBlock), 0, c->stream, c->n,
                           n_query_vertices, static_cast<const unsigned long long *>(dev_table), words, c->q_bitmap.as<uint32_t>());
        he = hipGetLastError();
    }
    return support_result(who, timer.end(he, c->stream, device_ms, host_bitmap, c->q_bitmap.p, bm_bytes));
}

// the same kernel into the caller's device buffer, on the context's stream; waits for nothing unless the call is timed (the two
// events of *device_ms need their wait).  k_support_bitmap writes every word of every row and leaves the bits at positions >= n of
// a row's last word zero (its __ballot is taken under v < n).
int gnnpe_filter_support_bitmap_device(gnnpe_ctx *c, uint32_t n_query_vertices, const void *dev_table, void *dev_bitmap, double *device_ms)
{
    const char *who = "gnnpe_filter_support_bitmap_device";
    GNNPE_REQUIRE(c && n_query_vertices, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(dev_table && (reinterpret_cast<uintptr_t>(dev_table) & 7u) == 0, GNNPE_ERR_ARG,
                  "%s: dev_table must be an 8-byte aligned device pointer", who);
    GNNPE_REQUIRE(dev_bitmap && (reinterpret_cast<uintptr_t>(dev_bitmap) & 3u) == 0, GNNPE_ERR_ARG,
                  "%s: dev_bitmap must be a 4-byte aligned device pointer", who);
    int rc = support_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint64_t words = ((uint64_t)c->n + 31) / 32;
    if (device_ms) *device_ms = 0.0;
    SupportTimer timer;
    hipError_t he = timer.begin(device_ms != nullptr, c->stream);
    if (he == hipSuccess && c->n) {
        hipLaunchKernelGGL(k_support_bitmap, dim3(grid_for(((uint64_t)c->n + 63) / 64 * 64)), dim3(kBlock), 0, c->stream, c->n,
                           n_query_vertices, static_cast<const unsigned long long *>(dev_table), words, static_cast<uint32_t *>(dev_bitmap));
        he = hipGetLastError();
    }
    if (!device_ms) return support_result(who, he);
    return support_result(who, timer.end(he, c->stream, device_ms));
}

}  // extern "C"
