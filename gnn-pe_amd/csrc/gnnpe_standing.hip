// gnnpe_standing.hip -- THE STANDING EXACT QUERY of include/gnnpe_online.h: a handle that keeps the parsed query, the support
// table S of the exact filter, the candidate bitmap C and the exact match count |M| on the device, and the one call that moves the
// resident graph and every open handle forward by an edge batch.
//
// The loop it runs was written out three times before (include/gnnpe_hip.h, `gnnpe_main --incremental`, the tests):
//     S -= S_T(G);  destroyed = Delta(G, C, D);  gnnpe_csr_apply_edges;  gnnpe_vde;  S += S_T(G');  C' = bitmap(S);
//     created = Delta(G', C', I);  |M'| = |M| + created - destroyed
// and every turn of it read and planned the query file again, walked the nq x ceil(n/32) words of C on the host, uploaded them
// for every delta call and downloaded them after every gnnpe_filter_support_bitmap.  Here the words of C never leave the device:
//   * gnnpe_filter_support_bitmap_device (gnnpe_filter_support.hip) writes C into the handle's buffer;
//   * k_sets_sizes gives |C(u)|, the 8 nq bytes the host needs for the matching order and the empty-set test;
//   * k_sets_members writes the start candidates of a full count (open, refresh) where sets_stage_items used to upload them;
//   * the searches are the kernels of gnnpe_refine_sets_mode, gnnpe_refine_sets_delta and gnnpe_refine_sets_delta_nonedges,
//     unchanged, reading the handle's bitmap: SetsResident of gnnpe_refine_sets.hip.h is the optional argument of sets_prepare,
//     sets_stage_items and delta_stage that says "the sets are already on the device".
//
// k_sets_sizes: one workgroup per bitmap row, lanes over the words, __popc, a DPP wave sum and four LDS words.
// k_sets_members (csrc/gnnpe_touched.hip, libgnnpe_hip.so, since the touched sets of a relabel or a vertex batch end with it too): the
//   ordered compaction of a bitmap row into ascending ids, one workgroup.  Here it writes the start candidates of a full count at
//   open and refresh, and gnnpe_standing_set_members.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) and the measurement: profiles/online_standing.txt.
//
// COUNT TABLES (gnnpe_standing_keep_counts): a handle can keep V (nq x n) and E (query edges x entries) exact across the batches.
// Per kept table it owns T, a scratch table D that is all zeros between batches, for E a spare for the out-of-place carry, and the
// change arrays.  A step runs the delta count kernels of the one-shot calls on the resident sets with D as dev_accum (sign -1 before
// the apply, +1 after it), the apply hands out the entry map where a handle on the context keeps E, T and D of E go through
// gnnpe_csr_carry_entries, and after the last step one gnnpe_table_fold per table does T += D, D = 0 and writes the change list
// (csrc/gnnpe_table_fold.hip says why D exists).  T, D and the spare of E take turns, so all three are sized for the largest graph
// of the batch before its first step (standing_size_edge_tables): nothing is allocated behind a swap.  profiles/online_standing_counts.txt.
//
// PEELING BY EDGE SUPPORT (gnnpe_standing_peel, gnnpe_standing_truss_levels): no kernel of their own.  A round is one
// gnnpe_csr_edges_below (csrc/gnnpe_edges_below.hip, libgnnpe_hip.so) on the kept E into c->below_pairs, the selected pairs to the host,
// and one gnnpe_standing_apply_edges with them as the deletions: the transaction, the other handles and the tables are that call's.
// profiles/online_standing_peel.txt.
#include "../../include/gnnpe_online.h"
#include "gnnpe_dpp.hip.h"
#include "gnnpe_refine_delta.hip.h"
#include "gnnpe_touched.hip.h"

#include <iterator>
#include <memory>

namespace gnnpe {

// sizes[u] = the set bits below n of row u; grid = nq workgroups
static __global__ __launch_bounds__(kBlock) void k_sets_sizes(const uint32_t *__restrict__ bitmap, uint64_t words, uint32_t n,
                                                              unsigned long long *__restrict__ sizes)
{
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t *__restrict__ row = bitmap + (uint64_t)blockIdx.x * words;
    uint32_t acc = 0;  // at most n < 2^32 in the whole row
    for (uint64_t w = threadIdx.x; w < words; w += kBlock) acc += (uint32_t)__popc(sets_word_below_n(row[w], w, words, n));
    const uint32_t sum = wave_sum_u32(acc);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < kBlock / 64; i++) total += s_wave[i];
        sizes[blockIdx.x] = total;
    }
}

// gnnpe_refine_sets.hip, gnnpe_refine_delta.hip, gnnpe_refine_delta_nonedges.hip: the three searches on resident sets, limit 2^64 - 1
int refine_sets_resident(gnnpe_ctx *c, uint32_t mode, uint64_t limit, uint64_t *answers, SetsResident *res, double *device_ms);
int refine_delta_resident(gnnpe_ctx *c, const uint32_t *edges, uint64_t n_edges, uint32_t mode, uint64_t *answers, SetsResident *res,
                          double *device_ms);
int refine_delta_nonedges_resident(gnnpe_ctx *c, const uint32_t *edges, uint64_t n_edges, uint32_t mode, uint64_t *answers,
                                   SetsResident *res, double *device_ms);
// gnnpe_refine_vcount.hip, gnnpe_refine_ecount.hip: the full count tables on resident sets into the handle's table; and
// gnnpe_refine_delta_counts.hip, gnnpe_refine_delta_nonedges_counts.hip: sign * (the tables over a set of edges / non-edges) added to
// the handle's scratch table (`edge_table`: the per-entry table, otherwise the per-vertex one)
int refine_vcount_resident(gnnpe_ctx *c, uint32_t mode, uint64_t *answers, const SetsResident *res, void *dev_table, double *device_ms);
int refine_ecount_resident(gnnpe_ctx *c, uint32_t mode, uint64_t *answers, const SetsResident *res, void *dev_table, double *device_ms);
int refine_delta_counts_resident(gnnpe_ctx *c, bool edge_table, const uint32_t *edges, uint64_t n_edges, uint32_t mode, uint64_t *answers,
                                 const SetsResident *res, void *dev_accum, int sign, double *device_ms);
int refine_delta_nonedges_counts_resident(gnnpe_ctx *c, bool edge_table, const uint32_t *pairs, uint64_t n_pairs, uint32_t mode,
                                          uint64_t *answers, const SetsResident *res, void *dev_accum, int sign, double *device_ms);

// gnnpe_refine_delta_vertices.hip, gnnpe_refine_delta_vertices_counts.hip: the search anchored at a set of data vertices and its two
// tables on resident sets -- S n C(u) by k_vset_member_of, no walk over C on the host
int refine_delta_vertices_resident(gnnpe_ctx *c, const uint32_t *vertices, uint64_t n_vertices, uint32_t mode, uint64_t *answers, SetsResident *res,
                                   double *device_ms);
int refine_delta_vertices_counts_resident(gnnpe_ctx *c, bool edge_table, const uint32_t *vertices, uint64_t n_vertices, uint32_t mode,
                                          uint64_t *answers, const SetsResident *res, void *dev_accum, int sign, double *device_ms);

// labels[i] = table[ids[i]]: the labels a relabel batch would replace (gnnpe_standing_set_labels)
static __global__ void k_standing_gather(uint32_t count, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ table, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = table[ids[i]];
}

// A count table a handle keeps (gnnpe_standing_keep_counts): T, the scratch table D the delta count kernels of a batch add into and
// gnnpe_table_fold empties, for the per-entry table the spare of the out-of-place carry, and the change list of the last batch.
struct StandingCounts {
    bool kept = false;
    DevBuf table, delta, spare, ch_cells, ch_deltas;
    uint64_t rows = 0, cols = 0;  // of T as it stands: nq x n, or query edges x entries of the current graph
    uint64_t n_changes = 0;       // of the last batch, whatever the change arrays hold
    uint64_t cells() const { return rows * cols; }
    static void swap(DevBuf &a, DevBuf &b)
    {
        std::swap(a.p, b.p);
        std::swap(a.bytes, b.bytes);
    }
    void swap_with(StandingCounts &o)
    {
        std::swap(kept, o.kept), std::swap(rows, o.rows), std::swap(cols, o.cols), std::swap(n_changes, o.n_changes);
        swap(table, o.table), swap(delta, o.delta), swap(spare, o.spare), swap(ch_cells, o.ch_cells), swap(ch_deltas, o.ch_deltas);
    }
};

constexpr size_t kStandingMax = 16;      // handles open on one context
constexpr uint64_t kStandingPoison = ~0ull;  // a generation no context has: the handle is stale whatever happens
constexpr uint32_t kMembersCanary = 16;   // words behind the ids of gnnpe_standing_set_members that must stay as they were

}  // namespace gnnpe

using namespace gnnpe;

struct gnnpe_standing {
    gnnpe_ctx *c = nullptr;
    uint32_t mode = 0, l = 0, nq = 0;
    double eps = 0.0;
    bool filter = false;  // gnnpe_standing_open: S is kept and C derived from it; gnnpe_standing_open_sets: C is the caller's
    gnnpe_host::StaticGraph query;  // parsed once
    // the exact plan of gnnpe_host_query_plan_exact (filter handles): the host arrays the support calls take
    uint32_t counts[3] = {0, 0, 0};
    uint32_t *qv = nullptr, *ql = nullptr, *qd = nullptr;
    double *qp = nullptr;
    std::string path;    // of the query file: read again only where a new label table changes e, which the plan depends on
    uint32_t plan_e = 0;
    uint32_t n = 0;      // the graph's vertices the buffers are sized for
    uint64_t words = 0;
    DevBuf table, bitmap, d_sizes, members;
    DevBuf table_spare;  // of the out-of-place carry of S through a vertex map: reserved at the first vertex batch
    DevBuf rows[2][2];  // [0 created, 1 destroyed][the kept rows, the batch being applied]
    int cur = 0;        // which of the two holds the kept rows
    uint64_t rows_cap = 0;
    std::vector<uint64_t> sizes;  // |C(u)|, from k_sets_sizes
    uint64_t count = 0, created = 0, destroyed = 0, held[2] = {0, 0};
    uint64_t graph_gen = 0, table_gen = 0;  // the state of the context the handle is exact for
    // the batch being applied, committed when every handle got through
    uint64_t p_created = 0, p_destroyed = 0, p_held[2] = {0, 0};
    // gnnpe_standing_keep_counts: [0] V (nq x n), [1] E (query edges x entries); changes_cap pairs of a batch's change list are held
    StandingCounts kc[2];
    uint32_t nqe = 0;  // the query's edges: the rows of E
    uint64_t changes_cap = 0;
    ~gnnpe_standing()
    {
        gnnpe_host_free(qv);
        gnnpe_host_free(ql);
        gnnpe_host_free(qd);
        gnnpe_host_free(qp);
    }
};

namespace {

bool standing_stale(const gnnpe_standing *h) { return h->graph_gen != h->c->graph_gen || h->table_gen != h->c->table_gen; }

#define STANDING_LIVE(who, h)                                                                                                          \
    do {                                                                                                                               \
        GNNPE_REQUIRE((h), GNNPE_ERR_ARG, "%s: null handle", who);                                                                     \
        GNNPE_REQUIRE(!standing_stale(h), GNNPE_ERR_ARG,                                                                               \
                      "%s: the graph, the labels or the label table changed behind the handle: gnnpe_standing_refresh brings it up to date", \
                      who);                                                                                                            \
    } while (0)

int standing_whole_graph(const char *who, gnnpe_ctx *c)
{
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    return GNNPE_OK;
}

SetsResident standing_sets(const gnnpe_standing *h)
{
    SetsResident R;
    R.query = &h->query;
    R.d_bitmap = h->bitmap.as<uint32_t>();
    R.sizes = h->sizes.data();
    return R;
}

// |C(u)| of the handle's bitmap to the host: k_sets_sizes, 8 nq bytes, one wait
int standing_sizes(gnnpe_standing *h)
{
    gnnpe_ctx *c = h->c;
    hipLaunchKernelGGL(k_sets_sizes, dim3(h->nq), dim3(kBlock), 0, c->stream, h->bitmap.as<uint32_t>(), h->words, h->n,
                       h->d_sizes.as<unsigned long long>());
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, h->d_sizes.p, (size_t)h->nq * 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    h->sizes.assign(c->h_pinned, c->h_pinned + h->nq);
    return GNNPE_OK;
}

// C = bitmap(S) on the device, then its sizes
int standing_derive(gnnpe_standing *h, double *ms)
{
    double ms1 = 0.0;
    int rc = gnnpe_filter_support_bitmap_device(h->c, h->nq, h->table.p, h->bitmap.p, ms ? &ms1 : nullptr);
    if (ms) *ms += ms1;
    return rc ? rc : standing_sizes(h);
}

int standing_support_delta(gnnpe_standing *h, const std::vector<uint32_t> &T, int sign, double *ms)
{
    double ms1 = 0.0;
    const int rc = gnnpe_filter_support_exact_delta(h->c, h->l, h->counts, h->qv, h->ql, h->qd, h->qp, h->nq, h->eps, T.data(), T.size(), sign,
                                                    h->table.p, ms ? &ms1 : nullptr);
    if (ms) *ms += ms1;
    return rc;
}

// A count table of the handle from the context's graph as it is, into K (the handle's own at a refresh, a local one in
// gnnpe_standing_keep_counts, which hands it over only when everything is in place): the buffers sized for the graph, D zeroed once,
// the change arrays of `cap` pairs, and T by the full count search on the resident sets.  The search's answer must be the count.
int standing_counts_build(const char *who, gnnpe_standing *h, bool edge, uint64_t cap, StandingCounts &K, double *ms)
{
    gnnpe_ctx *c = h->c;
    K.rows = edge ? h->nqe : h->nq;
    K.cols = edge ? c->nbr_used : c->n;
    const size_t bytes = std::max<uint64_t>(K.cells() * 8, 8), list = std::max<uint64_t>(cap * 8, 8);
    GNNPE_REQUIRE(cap <= (1ull << 40), GNNPE_ERR_ARG, "%s: changes_cap %llu", who, (unsigned long long)cap);
    int rc;
    if ((rc = K.table.reserve(bytes)) || (rc = K.delta.reserve(bytes)) || (edge && (rc = K.spare.reserve(bytes))) ||
        (rc = K.ch_cells.reserve(list)) || (rc = K.ch_deltas.reserve(list)))
        return rc;
    GNNPE_HIP_TRY(hipMemsetAsync(K.delta.p, 0, bytes, c->stream));
    const SetsResident R = standing_sets(h);
    uint64_t found = 0;
    double ms1 = 0.0;
    if ((rc = (edge ? refine_ecount_resident : refine_vcount_resident)(c, h->mode, &found, &R, K.table.p, ms ? &ms1 : nullptr))) return rc;
    if (ms) *ms += ms1;
    GNNPE_REQUIRE(found == h->count, GNNPE_ERR_HIP, "%s: internal error: the table's search found %llu matches, the count is %llu", who,
                  (unsigned long long)found, (unsigned long long)h->count);
    K.n_changes = 0;
    K.kept = true;
    return GNNPE_OK;
}

// S, C and |M| from the context's graph as it is: what open leaves, and refresh.  The buffers are sized for the graph's n.
int standing_compute(const char *who, gnnpe_standing *h, double *ms)
{
    gnnpe_ctx *c = h->c;
    int rc = standing_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    const uint64_t words = ((uint64_t)c->n + 31) / 32;
    if (!h->filter)
        GNNPE_REQUIRE(c->n == h->n, GNNPE_ERR_ARG, "%s: the graph has %u vertices, the caller's bitmap was made for %u: close the handle and open it again",
                      who, c->n, h->n);
    h->n = c->n;
    h->words = words;
    if ((rc = h->bitmap.reserve(std::max<uint64_t>((uint64_t)h->nq * words * 4, 4))) || (rc = h->d_sizes.reserve(((size_t)h->nq + 1) * 8))) return rc;
    if (h->filter) {
        GNNPE_REQUIRE(c->have_table, GNNPE_ERR_ARG, "%s: needs the label table and gnnpe_vde since the last change of the rows or the labels", who);
        if (h->plan_e != c->e) {
            gnnpe_host_free(h->qv), gnnpe_host_free(h->ql), gnnpe_host_free(h->qd), gnnpe_host_free(h->qp);
            h->qv = h->ql = h->qd = nullptr, h->qp = nullptr;
            uint32_t n_qv = 0;
            if ((rc = gnnpe_host_query_plan_exact(h->path.c_str(), c->e, h->l, &n_qv, h->counts, &h->qv, &h->ql, &h->qd, &h->qp))) return rc;
            h->plan_e = c->e;
        }
        if ((rc = h->table.reserve(std::max<uint64_t>((uint64_t)h->nq * c->n * 8, 8)))) return rc;
        double ms1 = 0.0;
        if ((rc = gnnpe_filter_support_exact(c, h->l, h->counts, h->qv, h->ql, h->qd, h->qp, h->nq, h->eps, h->table.p, ms ? &ms1 : nullptr))) return rc;
        if (ms) *ms += ms1;
        if ((rc = standing_derive(h, ms))) return rc;
    } else if ((rc = standing_sizes(h)))
        return rc;
    SetsResident R = standing_sets(h);
    double ms1 = 0.0;
    uint64_t count = 0;
    if ((rc = refine_sets_resident(c, h->mode, ~0ull, &count, &R, ms ? &ms1 : nullptr))) return rc;
    if (ms) *ms += ms1;
    h->count = count;
    h->created = h->destroyed = h->held[0] = h->held[1] = 0;
    // every kept count table again, with empty change lists
    for (int t = 0; t < 2; t++)
        if (h->kc[t].kept && (rc = standing_counts_build(who, h, t == 1, h->changes_cap, h->kc[t], ms))) return rc;
    h->graph_gen = c->graph_gen;
    h->table_gen = c->table_gen;
    return GNNPE_OK;
}

void standing_unregister(gnnpe_standing *h)
{
    auto &v = h->c->standing;
    v.erase(std::remove(v.begin(), v.end(), static_cast<void *>(h)), v.end());
}

void standing_close_all(gnnpe_ctx *c)
{
    const std::vector<void *> open(c->standing);
    c->standing.clear();
    for (void *p : open) delete static_cast<gnnpe_standing *>(p);
}

// what both opens share: the checks, the query graph, the handle and its row buffers; the bitmap comes from `host_bitmap` or, with
// l != 0, from the filter
int standing_open(const char *who, gnnpe_ctx *c, const char *query_graph_path, uint32_t l, double epsilon, uint32_t mode, uint64_t rows_cap,
                  const uint32_t *host_bitmap, gnnpe_standing **sq, uint64_t *count, double *device_ms)
{
    if (sq) *sq = nullptr;
    if (count) *count = 0;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && query_graph_path && sq && count, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE((mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) == 0, GNNPE_ERR_ARG, "%s: unknown mode bits 0x%x", who, mode);
    int rc = standing_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_REQUIRE(c->standing.size() < kStandingMax, GNNPE_ERR_ARG, "%s: %zu standing queries are open on the context already", who, kStandingMax);
    std::unique_ptr<gnnpe_standing> h(new gnnpe_standing);
    h->c = c;
    h->mode = mode;
    h->filter = host_bitmap == nullptr;
    h->l = l;
    h->eps = epsilon;
    h->rows_cap = rows_cap;
    std::string err;
    if ((rc = h->query.load(query_graph_path, &err)) != 0) {
        set_error("%s", err.c_str());
        return rc;
    }
    h->nq = h->query.n;
    h->nqe = (uint32_t)gnnpe_host::query_edges(h->query).size();
    GNNPE_REQUIRE(h->nq >= 1 && h->nq <= (uint32_t)kSetsMaxQ, GNNPE_ERR_UNSUPPORTED, "query graphs of 1..%d vertices (got %u)", kSetsMaxQ, h->nq);
    GNNPE_REQUIRE(rows_cap <= (1ull << 40) / ((uint64_t)h->nq * 4), GNNPE_ERR_ARG, "%s: rows_cap %llu", who, (unsigned long long)rows_cap);
    h->n = c->n;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    h->path = query_graph_path;
    if (!h->filter) {
        const uint64_t bytes = (uint64_t)h->nq * (((uint64_t)c->n + 31) / 32) * 4;
        if ((rc = h->bitmap.reserve(std::max<uint64_t>(bytes, 4)))) return rc;
        if (bytes) GNNPE_HIP_TRY(hipMemcpy(h->bitmap.p, host_bitmap, bytes, hipMemcpyHostToDevice));
    }
    for (int which = 0; which < 2 && rows_cap; which++)
        for (int b = 0; b < 2; b++)
            if ((rc = h->rows[which][b].reserve((size_t)rows_cap * h->nq * 4))) return rc;
    if ((rc = standing_compute(who, h.get(), device_ms))) return rc;
    c->standing.push_back(h.get());
    c->standing_close_all = standing_close_all;
    *count = h->count;
    *sq = h.release();
    return GNNPE_OK;
}

// one delta search of a handle on the graph as it is: Delta (nonedges false) or N (true) of `edges`, the rows behind the p_held[which]
// rows of the batch's buffer.  Adds to *sum.
// A handle that keeps count tables runs the table kernels of the same search with its scratch tables as dev_accum: sign -1 for what
// the step destroys (which == 1), +1 for what it creates.  Their answers are the search's, so with rows_cap == 0 the row search is
// left out and no match is searched twice; with rows it runs as well, and must agree.
// `items`: the pairs of the delta search (two words each), or with `vertices` the data vertices the search DeltaV is anchored at
// (gnnpe_standing_set_labels, gnnpe_standing_apply_vertices).  `who`: the entry the step belongs to, for its messages.
int standing_delta(const char *who, gnnpe_standing *h, bool nonedges, const std::vector<uint32_t> &items, int which, uint64_t *sum, double *ms,
                   bool vertices = false)
{
    if (items.empty()) return GNNPE_OK;
    const uint64_t n_items = vertices ? items.size() : items.size() / 2;
    uint64_t found = 0;
    bool have = false;
    for (int t = 0; t < 2; t++) {
        if (!h->kc[t].kept) continue;
        const SetsResident R = standing_sets(h);
        uint64_t got = 0;
        double ms1 = 0.0;
        const int rc = (vertices   ? refine_delta_vertices_counts_resident
                        : nonedges ? refine_delta_nonedges_counts_resident
                                   : refine_delta_counts_resident)(h->c, t == 1, items.data(), n_items, h->mode, &got, &R,
                                                                   h->kc[t].delta.p, which == 1 ? -1 : 1, ms ? &ms1 : nullptr);
        if (rc) return rc;
        if (ms) *ms += ms1;
        GNNPE_REQUIRE(!have || got == found, GNNPE_ERR_HIP, "%s: internal error: the two table searches found %llu and %llu matches", who,
                      (unsigned long long)found, (unsigned long long)got);
        found = got;
        have = true;
    }
    if (!have || h->rows_cap) {
        SetsResident R = standing_sets(h);
        const uint64_t at = h->p_held[which];
        if (h->rows_cap > at) {
            R.d_rows = h->rows[which][h->cur ^ 1].as<uint32_t>() + at * h->nq;
            R.rows_cap = h->rows_cap - at;
        }
        uint64_t rows_found = 0;
        double ms1 = 0.0;
        const int rc = (vertices   ? refine_delta_vertices_resident
                        : nonedges ? refine_delta_nonedges_resident
                                   : refine_delta_resident)(h->c, items.data(), n_items, h->mode, &rows_found, &R,
                                                            ms ? &ms1 : nullptr);
        if (rc) return rc;
        if (ms) *ms += ms1;
        GNNPE_REQUIRE(!have || rows_found == found, GNNPE_ERR_HIP, "%s: internal error: the row search found %llu matches, the table search %llu",
                      who, (unsigned long long)rows_found, (unsigned long long)found);
        found = rows_found;
        h->p_held[which] += R.rows_held;
    }
    *sum += found;
    return GNNPE_OK;
}

// D = 0 for every kept table of the handles: the roll-back of a step that was refused before its swap
int standing_zero_deltas(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H)
{
    bool any = false;
    for (gnnpe_standing *h : H)
        for (StandingCounts &K : h->kc)
            if (K.kept && K.cells()) {
                GNNPE_HIP_TRY(hipMemsetAsync(K.delta.p, 0, K.cells() * 8, c->stream));
                any = true;
            }
    if (any) GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    return GNNPE_OK;
}

// One apply of the context's graph with every handle carried through it (the header has the loop).  Returns the first failure; with
// *swapped false the graph is what it was and every S has been put back.
// `want_map` (a handle on the context keeps E): the apply is gnnpe_csr_apply_edges_map, and T and D of every kept E go through the
// entry map before the searches on the new graph add to D.
int standing_step(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H, const std::vector<uint32_t> &I, const std::vector<uint32_t> &D, bool *swapped,
                  double *ms, bool want_map)
{
    const char *who = "gnnpe_standing_apply_edges";
    *swapped = false;
    std::vector<uint32_t> T(I);  // the end vertices of the step, each once
    T.insert(T.end(), D.begin(), D.end());
    std::sort(T.begin(), T.end());
    T.erase(std::unique(T.begin(), T.end()), T.end());
    int rc = GNNPE_OK;
    std::vector<gnnpe_standing *> reduced;  // the handles whose S has lost S_T(G)
    for (size_t i = 0; i < H.size() && !rc; i++)
        if (H[i]->filter && !(rc = standing_support_delta(H[i], T, -1, ms))) reduced.push_back(H[i]);
    for (size_t i = 0; i < H.size() && !rc; i++) {
        gnnpe_standing *h = H[i];
        rc = standing_delta(who, h, false, D, 1, &h->p_destroyed, ms);
        if (!rc && (h->mode & GNNPE_MATCH_INDUCED)) rc = standing_delta(who, h, true, I, 1, &h->p_destroyed, ms);
    }
    double ms1 = 0.0;
    void *map = nullptr;
    if (!rc && want_map) rc = gnnpe_csr_apply_edges_map(c, I.data(), I.size() / 2, D.data(), D.size() / 2, nullptr, nullptr, &map, ms ? &ms1 : nullptr);
    else if (!rc) rc = gnnpe_csr_apply_edges(c, I.data(), I.size() / 2, D.data(), D.size() / 2, nullptr, ms ? &ms1 : nullptr);
    if (rc) {  // nothing of the context has changed: S is put back on the unchanged graph (the message of the failure is kept)
        const std::string why = gnnpe_last_error();
        for (gnnpe_standing *h : reduced)
            if (standing_support_delta(h, T, +1, nullptr)) h->graph_gen = kStandingPoison;
        if (standing_zero_deltas(c, H))  // the scratch tables lose what the searches on the unchanged graph subtracted
            for (gnnpe_standing *h : H) h->graph_gen = kStandingPoison;
        set_error("%s", why.c_str());
        return rc;
    }
    *swapped = true;
    if (ms) *ms += ms1;
    for (gnnpe_standing *h : H) {  // the buffers were sized for the batch before its first step (standing_size_edge_tables)
        StandingCounts &K = h->kc[1];
        if (!K.kept) continue;
        for (DevBuf *buf : {&K.table, &K.delta}) {
            if ((rc = gnnpe_csr_carry_entries(c, (uint32_t)K.rows, 8, buf->p, K.spare.p, ms ? &ms1 : nullptr))) return rc;
            if (ms) *ms += ms1;
            StandingCounts::swap(*buf, K.spare);
        }
        K.cols = c->nbr_used;
    }
    if (c->have_table && (rc = gnnpe_vde(c, nullptr, nullptr, nullptr))) return rc;
    for (size_t i = 0; i < H.size() && !rc; i++)
        if (H[i]->filter && !(rc = standing_support_delta(H[i], T, +1, ms))) rc = standing_derive(H[i], ms);
    for (size_t i = 0; i < H.size() && !rc; i++) {
        gnnpe_standing *h = H[i];
        rc = standing_delta(who, h, false, I, 0, &h->p_created, ms);
        if (!rc && (h->mode & GNNPE_MATCH_INDUCED)) rc = standing_delta(who, h, true, D, 0, &h->p_created, ms);
    }
    return rc;
}

// Before the first step of a batch: T, D and the spare of every kept E get room for the largest graph the batch passes through
// (`entries_max` entries), so that no carry needs an allocation behind a swap -- the three buffers take turns as the spare.  A spare
// holds nothing; D is all zeros between batches; T moves into the spare when it has to grow.  A refusal leaves every table intact.
int standing_size_edge_tables(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H, uint64_t entries_max)
{
    for (gnnpe_standing *h : H) {
        StandingCounts &K = h->kc[1];
        if (!K.kept) continue;
        const size_t need = std::max<uint64_t>(K.rows * entries_max * 8, 8);
        int rc = K.spare.reserve(need);
        if (rc) return rc;
        if (K.delta.bytes < need) {
            if ((rc = K.delta.reserve(need))) {
                h->graph_gen = kStandingPoison;  // (a refused reserve has given the old buffer back: the handle is without its D)
                return rc;
            }
            GNNPE_HIP_TRY(hipMemsetAsync(K.delta.p, 0, need, c->stream));
        }
        if (K.table.bytes < need) {
            GNNPE_HIP_TRY(hipMemcpyAsync(K.spare.p, K.table.p, K.cells() * 8, hipMemcpyDeviceToDevice, c->stream));
            GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
            StandingCounts::swap(K.table, K.spare);
            if ((rc = K.spare.reserve(need))) return rc;
        }
    }
    return GNNPE_OK;
}

// the refusals of a batch that are decided before anything changes: a loop, an id >= n, an edge in both lists (host); a deletion
// that is no edge, an insertion that is one (k_delta_entries, one wait).  The codes and the cases are gnnpe_csr_apply_edges'.
int standing_check_batch(const char *who, gnnpe_ctx *c, const std::vector<uint32_t> &I, const std::vector<uint32_t> &D)
{
    std::vector<uint64_t> ki, kd;
    std::string err;
    if (gnnpe_host::delta_edge_keys(c->n, I.data(), I.size() / 2, &ki, &err) != 0 || gnnpe_host::delta_edge_keys(c->n, D.data(), D.size() / 2, &kd, &err) != 0) {
        set_error("%s: %s", who, err.c_str());
        return GNNPE_ERR_ARG;
    }
    std::vector<uint64_t> both;
    std::set_intersection(ki.begin(), ki.end(), kd.begin(), kd.end(), std::back_inserter(both));
    GNNPE_REQUIRE(both.empty(), GNNPE_ERR_ARG, "%s: edge (%u, %u) is in both lists", who, (uint32_t)(both[0] >> 32), (uint32_t)both[0]);
    const size_t ni = ki.size(), nd = kd.size(), np = ni + nd;
    GNNPE_REQUIRE(np < (1ull << 31), GNNPE_ERR_ARG, "%s: %zu pairs, the items are 32-bit", who, np);
    std::vector<uint32_t> pairs(2 * np);
    for (size_t i = 0; i < np; i++) {
        const uint64_t k = i < ni ? ki[i] : kd[i - ni];
        pairs[2 * i] = (uint32_t)(k >> 32);
        pairs[2 * i + 1] = (uint32_t)k;
    }
    // [counters of the insertions | counters of the deletions | pairs | entries] in the buffer of F, which the delta calls fill afterwards
    int rc = c->q_delta.reserve(2 * sizeof(SetsCounters) + np * 12);
    if (rc) return rc;
    SetsCounters *ctr = c->q_delta.as<SetsCounters>();
    uint32_t *d_pairs = reinterpret_cast<uint32_t *>(ctr + 2), *d_ent = d_pairs + 2 * np;
    GNNPE_HIP_TRY(hipMemsetAsync(ctr, 0, 2 * sizeof(SetsCounters), c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), np * 8, hipMemcpyHostToDevice, c->stream));
    if (ni)
        hipLaunchKernelGGL(k_delta_entries, dim3((ni + 255) / 256), dim3(256), 0, c->stream, (uint32_t)ni, d_pairs, c->adj_start.as<uint32_t>(),
                           c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), d_ent, ctr, 0u);
    if (nd)
        hipLaunchKernelGGL(k_delta_entries, dim3((nd + 255) / 256), dim3(256), 0, c->stream, (uint32_t)nd, d_pairs + 2 * ni, c->adj_start.as<uint32_t>(),
                           c->adj_deg.as<uint32_t>(), c->nbrs.as<uint32_t>(), d_ent + ni, ctr + 1, 1u);
    GNNPE_HIP_TRY(hipGetLastError());
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, ctr, 2 * sizeof(SetsCounters), hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));  // (`pairs` lives until here)
    const SetsCounters *R = reinterpret_cast<const SetsCounters *>(c->h_pinned);
    GNNPE_REQUIRE(!R[0].bad, GNNPE_ERR_ARG, "%s: an insertion is already an edge of the graph", who);
    GNNPE_REQUIRE(!R[1].bad, GNNPE_ERR_ARG, "%s: a deletion is not an edge of the graph", who);
    return GNNPE_OK;
}


// ---- relabels and vertex batches through the handle ---------------------------------------------------------------------------

// The touched sets of a batch in c->q_touched, sized for `room` vertices (the larger of n and n'):
//   [ids of the batch, room words | their gathered labels, room words | T: bits, ids | T': bits, ids]
struct StandingTouched {
    uint32_t *batch = nullptr, *gathered = nullptr, *bits[2] = {nullptr, nullptr}, *ids[2] = {nullptr, nullptr};
    uint64_t n_ids[2] = {0, 0}, room = 0;
};

int standing_touched_reserve(gnnpe_ctx *c, uint64_t room, StandingTouched *T)
{
    const uint64_t words = (room + 31) / 32;
    const int rc = c->q_touched.reserve((2 * room + 2 * (words + room)) * 4 + 8);
    if (rc) return rc;
    T->room = room;
    T->batch = c->q_touched.as<uint32_t>();
    T->gathered = T->batch + room;
    T->bits[0] = T->gathered + room, T->ids[0] = T->bits[0] + words;
    T->bits[1] = T->ids[0] + room, T->ids[1] = T->bits[1] + words;
    return GNNPE_OK;
}

// S += sign * S_T of the handle, T from the device (set `w` of StandingTouched): no host list, no sort, no upload
int standing_support_delta_device(gnnpe_standing *h, const StandingTouched &T, int w, int sign, double *ms)
{
    double ms1 = 0.0;
    const int rc = gnnpe_filter_support_exact_delta_device(h->c, h->l, h->counts, h->qv, h->ql, h->qd, h->qp, h->nq, h->eps, T.bits[w], T.ids[w],
                                                           T.n_ids[w], sign, h->table.p, ms ? &ms1 : nullptr);
    if (ms) *ms += ms1;
    return rc;
}

// room for `need` bytes in a buffer whose first `used` bytes must survive: a larger one is made aside and takes them over
int standing_grow_keep(gnnpe_ctx *c, DevBuf &b, size_t need, size_t used)
{
    if (need <= b.bytes) return GNNPE_OK;
    DevBuf fresh;
    const int rc = fresh.reserve(need);
    if (rc) return rc;
    if (used) GNNPE_HIP_TRY(hipMemcpyAsync(fresh.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    StandingCounts::swap(b, fresh);
    return GNNPE_OK;
}

// Before a vertex batch changes anything: S, its spare, C, and T, D and the spare of every kept table get room for `n_max` vertices
// (the entries only shrink), so that nothing is allocated behind the swap.  The spares are made here, at the first vertex batch:
// a handle that only sees edge batches never owns them.  A refusal leaves every table intact (a scratch table without its zeros
// poisons the handle, as in standing_size_edge_tables).
int standing_size_for_vertices(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H, uint64_t n_max)
{
    for (gnnpe_standing *h : H) {
        const size_t s_need = std::max<uint64_t>((uint64_t)h->nq * n_max * 8, 8), c_need = std::max<uint64_t>((uint64_t)h->nq * ((n_max + 31) / 32) * 4, 4);
        int rc;
        if ((rc = h->table_spare.reserve(s_need)) || (rc = standing_grow_keep(c, h->table, s_need, (size_t)h->nq * h->n * 8)) ||
            (rc = standing_grow_keep(c, h->bitmap, c_need, (size_t)h->nq * h->words * 4)))
            return rc;
        for (int t = 0; t < 2; t++) {
            StandingCounts &K = h->kc[t];
            if (!K.kept) continue;
            const size_t need = std::max<uint64_t>(K.rows * (t == 1 ? K.cols : n_max) * 8, 8);
            if ((rc = K.spare.reserve(need)) || (rc = standing_grow_keep(c, K.table, need, K.cells() * 8))) return rc;
            if (K.delta.bytes < need) {
                if ((rc = K.delta.reserve(need))) {
                    h->graph_gen = kStandingPoison;
                    return rc;
                }
                GNNPE_HIP_TRY(hipMemsetAsync(K.delta.p, 0, need, c->stream));
            }
        }
    }
    return GNNPE_OK;
}

// after a refusal before the swap: S is put back on the unchanged graph, the scratch tables lose what the searches subtracted (the
// message of the failure is kept)
void standing_roll_back(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H, const std::vector<gnnpe_standing *> &reduced, const StandingTouched &T)
{
    const std::string why = gnnpe_last_error();
    for (gnnpe_standing *h : reduced)
        if (standing_support_delta_device(h, T, 0, +1, nullptr)) h->graph_gen = kStandingPoison;
    if (standing_zero_deltas(c, H))
        for (gnnpe_standing *h : H) h->graph_gen = kStandingPoison;
    set_error("%s", why.c_str());
}

// one gnnpe_table_fold per kept table: D into T, D = 0, the batch's change list in the cells of G'
int standing_fold_all(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H, double *device_ms)
{
    int rc = GNNPE_OK;
    for (size_t i = 0; i < H.size() && !rc; i++)
        for (StandingCounts &K : H[i]->kc) {
            if (!K.kept || rc) continue;
            double ms1 = 0.0;
            rc = gnnpe_table_fold(c, K.table.p, K.delta.p, K.cells(), K.ch_cells.p, K.ch_deltas.p, H[i]->changes_cap, &K.n_changes,
                                  device_ms ? &ms1 : nullptr);
            if (device_ms) *device_ms += ms1;
        }
    return rc;
}

// what a batch leaves in every handle once all of them got through (`moved`: the graph changed, the kept rows are the batch's)
void standing_commit(gnnpe_ctx *c, const std::vector<gnnpe_standing *> &H, bool moved)
{
    for (gnnpe_standing *h : H) {
        if (!moved) h->kc[0].n_changes = h->kc[1].n_changes = 0;  // the empty batch changes no cell
        h->created = h->p_created;
        h->destroyed = h->p_destroyed;
        h->count += h->p_created - h->p_destroyed;
        h->held[0] = h->p_held[0];
        h->held[1] = h->p_held[1];
        if (moved) h->cur ^= 1;
        h->graph_gen = c->graph_gen;
    }
}

// the live handles of the context, in a call's first lines
int standing_handles(const char *who, gnnpe_ctx *c, std::vector<gnnpe_standing *> *H)
{
    for (void *p : c->standing) {
        H->push_back(static_cast<gnnpe_standing *>(p));
        STANDING_LIVE(who, H->back());
    }
    return GNNPE_OK;
}

}  // namespace

extern "C" {

int gnnpe_standing_set_labels(gnnpe_ctx *c, const uint32_t *vertices, const uint32_t *labels, uint64_t count, double *device_ms)
{
    const char *who = "gnnpe_standing_set_labels";
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && ((vertices && labels) || count == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = standing_whole_graph(who, c);
    if (rc) return rc;
    std::vector<gnnpe_standing *> H;
    if ((rc = standing_handles(who, c, &H))) return rc;
    if (H.empty()) {  // a context without a handle gets the plain relabel (and gnnpe_vde): no gather, no touched set
        if ((rc = gnnpe_set_vertex_labels(c, vertices, labels, count, device_ms))) return rc;
        return count && c->have_table ? gnnpe_vde(c, nullptr, nullptr, nullptr) : GNNPE_OK;
    }
    bool filter = false;
    for (gnnpe_standing *h : H) filter = filter || h->filter;
    const uint32_t n = c->n;
    // every (vertex, label) pair once, as gnnpe_set_vertex_labels reads the lists; a label without a row in the table would fail
    // gnnpe_vde behind the change
    std::vector<uint64_t> pairs(count);
    for (uint64_t i = 0; i < count; i++) {
        GNNPE_REQUIRE(vertices[i] < n, GNNPE_ERR_ARG, "%s: vertex %u is not a vertex of the graph (n = %u)", who, vertices[i], n);
        GNNPE_REQUIRE(!(filter && c->have_table) || labels[i] < c->n_labels, GNNPE_ERR_ARG, "%s: label %u of vertex %u has no row in the %u-row label table",
                      who, labels[i], vertices[i], c->n_labels);
        pairs[i] = ((uint64_t)vertices[i] << 32) | labels[i];
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const size_t k = pairs.size();
    for (size_t i = 1; i < k; i++)
        GNNPE_REQUIRE((uint32_t)(pairs[i] >> 32) != (uint32_t)(pairs[i - 1] >> 32), GNNPE_ERR_ARG, "%s: vertex %u is listed with the labels %u and %u", who,
                      (uint32_t)(pairs[i] >> 32), (uint32_t)pairs[i - 1], (uint32_t)pairs[i]);
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    StandingTouched T;
    if ((rc = standing_touched_reserve(c, n, &T))) return rc;
    // R*: the pairs that change a label -- one gather of 4 k bytes says which
    std::vector<uint32_t> R, L;
    if (k) {
        std::vector<uint32_t> ids(k), now(k);
        for (size_t i = 0; i < k; i++) ids[i] = (uint32_t)(pairs[i] >> 32);
        GNNPE_HIP_TRY(hipMemcpyAsync(T.batch, ids.data(), k * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_standing_gather, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, c->stream, (uint32_t)k, T.batch, c->labels.as<uint32_t>(),
                           T.gathered);
        GNNPE_HIP_TRY(hipGetLastError());
        GNNPE_HIP_TRY(hipMemcpyAsync(now.data(), T.gathered, k * 4, hipMemcpyDeviceToHost, c->stream));
        GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < k; i++)
            if (now[i] != (uint32_t)pairs[i]) R.push_back(ids[i]), L.push_back((uint32_t)pairs[i]);
    }
    for (gnnpe_standing *h : H) h->p_created = h->p_destroyed = h->p_held[0] = h->p_held[1] = 0;
    if (R.empty()) {  // nothing changes: neither the graph nor its generation
        standing_commit(c, H, false);
        return GNNPE_OK;
    }
    double ms1 = 0.0;
    // T = R* u N(R*), once for every handle: the label of R* and the vde of its neighbours change
    if ((rc = gnnpe_csr_closed_neighbourhood(c, R.data(), R.size(), T.bits[0], T.ids[0], T.room, &T.n_ids[0], device_ms ? &ms1 : nullptr))) return rc;
    if (device_ms) *device_ms += ms1;
    std::vector<gnnpe_standing *> reduced;  // the handles whose S has lost S_T(G)
    for (size_t i = 0; i < H.size() && !rc; i++)
        if (H[i]->filter && !(rc = standing_support_delta_device(H[i], T, 0, -1, device_ms))) reduced.push_back(H[i]);
    for (size_t i = 0; i < H.size() && !rc; i++) rc = standing_delta(who, H[i], false, R, 1, &H[i]->p_destroyed, device_ms, true);
    if (!rc) rc = gnnpe_set_vertex_labels(c, R.data(), L.data(), R.size(), device_ms ? &ms1 : nullptr);
    if (rc) {  // nothing of the context has changed
        standing_roll_back(c, H, reduced, T);
        return rc;
    }
    if (device_ms) *device_ms += ms1;
    // behind the change: a failure leaves the graph moved on and the handles not
    if (c->have_table) rc = gnnpe_vde(c, nullptr, nullptr, nullptr);
    for (size_t i = 0; i < H.size() && !rc; i++)
        if (H[i]->filter && !(rc = standing_support_delta_device(H[i], T, 0, +1, device_ms))) rc = standing_derive(H[i], device_ms);
    for (size_t i = 0; i < H.size() && !rc; i++) rc = standing_delta(who, H[i], false, R, 0, &H[i]->p_created, device_ms, true);
    if (!rc) rc = standing_fold_all(c, H, device_ms);
    if (rc) {
        for (gnnpe_standing *h : H) h->graph_gen = kStandingPoison;
        return rc;
    }
    standing_commit(c, H, true);
    return GNNPE_OK;
}

int gnnpe_standing_apply_vertices(gnnpe_ctx *c, const uint32_t *remove, uint64_t n_remove, const uint32_t *add_labels, uint64_t n_add,
                                  uint32_t *n_after, double *device_ms)
{
    const char *who = "gnnpe_standing_apply_vertices";
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && (remove || n_remove == 0) && (add_labels || n_add == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    if (n_after) *n_after = c->n;
    int rc = standing_whole_graph(who, c);
    if (rc) return rc;
    std::vector<gnnpe_standing *> H;
    if ((rc = standing_handles(who, c, &H))) return rc;
    if (H.empty()) {  // a context without a handle gets the plain apply (and gnnpe_vde): no touched set, no carry
        const uint64_t gen = c->graph_gen;
        if ((rc = gnnpe_csr_apply_vertices(c, remove, n_remove, add_labels, n_add, n_after, nullptr, nullptr, nullptr, nullptr, device_ms))) return rc;
        return c->graph_gen != gen && c->have_table ? gnnpe_vde(c, nullptr, nullptr, nullptr) : GNNPE_OK;
    }
    bool want_map = false;  // a handle on the context keeps E: the apply hands out the entry map
    for (gnnpe_standing *h : H) {
        GNNPE_REQUIRE(h->filter, GNNPE_ERR_UNSUPPORTED,
                      "%s: a gnnpe_standing_open_sets handle is open on the context: its bitmap was made for %u vertices (close it first)", who, h->n);
        want_map = want_map || h->kc[1].kept;
    }
    // gnnpe_csr_apply_vertices' own refusals, decided here because S changes before the apply is asked
    const uint32_t n = c->n;
    std::vector<uint32_t> R(remove, remove + n_remove);
    for (uint32_t v : R) GNNPE_REQUIRE(v < n, GNNPE_ERR_ARG, "%s: vertex %u is not a vertex of the graph (n = %u)", who, v, n);
    std::sort(R.begin(), R.end());
    R.erase(std::unique(R.begin(), R.end()), R.end());
    const uint32_t n_surv = n - (uint32_t)R.size();
    GNNPE_REQUIRE(n_add < 0xFFFFFFFFull, GNNPE_ERR_RANGE, "%s: %llu added vertices exceed 32-bit ids", who, (unsigned long long)n_add);
    const uint64_t n2_64 = (uint64_t)n_surv + n_add;
    GNNPE_REQUIRE(n2_64 != 0, GNNPE_ERR_ARG, "%s: the batch leaves no vertex", who);
    GNNPE_REQUIRE(n2_64 < 0xFFFFFFFFull, GNNPE_ERR_RANGE, "%s: %llu vertices exceed 32-bit ids", who, (unsigned long long)n2_64);
    for (uint64_t i = 0; i < n_add && !H.empty() && c->have_table; i++)
        GNNPE_REQUIRE(add_labels[i] < c->n_labels, GNNPE_ERR_ARG, "%s: label %u of added vertex %llu has no row in the %u-row label table", who,
                      add_labels[i], (unsigned long long)i, c->n_labels);
    const uint32_t n2 = (uint32_t)n2_64;
    for (gnnpe_standing *h : H) h->p_created = h->p_destroyed = h->p_held[0] = h->p_held[1] = 0;
    if (R.empty() && n_add == 0) {  // the empty batch: neither the graph nor its generation changes
        standing_commit(c, H, false);
        return GNNPE_OK;
    }
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    StandingTouched T;
    const uint64_t n_max = std::max(n, n2);
    if ((rc = standing_touched_reserve(c, n_max, &T)) || (rc = standing_size_for_vertices(c, H, n_max))) return rc;
    double ms1 = 0.0;
    // T = R u N_G(R): what the removal takes from the paths of S (an empty R gives the empty set, which T' starts from)
    if ((rc = gnnpe_csr_closed_neighbourhood(c, R.data(), R.size(), T.bits[0], T.ids[0], T.room, &T.n_ids[0], device_ms ? &ms1 : nullptr))) return rc;
    if (device_ms) *device_ms += ms1;
    std::vector<gnnpe_standing *> reduced;
    for (size_t i = 0; i < H.size() && !rc; i++)
        if (!(rc = standing_support_delta_device(H[i], T, 0, -1, device_ms))) reduced.push_back(H[i]);
    for (size_t i = 0; i < H.size() && !rc; i++) rc = standing_delta(who, H[i], false, R, 1, &H[i]->p_destroyed, device_ms, true);
    void *vmap = nullptr, *emap = nullptr;
    if (!rc)
        rc = gnnpe_csr_apply_vertices(c, R.data(), R.size(), add_labels, n_add, nullptr, nullptr, nullptr, &vmap, want_map ? &emap : nullptr,
                                      device_ms ? &ms1 : nullptr);
    if (rc) {  // nothing of the context has changed
        standing_roll_back(c, H, reduced, T);
        return rc;
    }
    if (device_ms) *device_ms += ms1;
    if (n_after) *n_after = c->n;
    // behind the swap: S, V and its scratch table through the vertex map, E and its scratch table through the entry map.  The
    // columns of R and the entries at R hold what the searches above left there and are dropped: their cells are gone, not listed.
    auto carry = [&](bool entries, uint32_t rows, DevBuf &buf, DevBuf &spare) {
        const int r = (entries ? gnnpe_csr_carry_entries : gnnpe_csr_carry_vertices)(c, rows, 8, buf.p, spare.p, device_ms ? &ms1 : nullptr);
        if (!r) {
            if (device_ms) *device_ms += ms1;
            StandingCounts::swap(buf, spare);
        }
        return r;
    };
    for (size_t i = 0; i < H.size() && !rc; i++) {
        gnnpe_standing *h = H[i];
        rc = carry(false, h->nq, h->table, h->table_spare);
        for (int t = 0; t < 2 && !rc; t++) {
            StandingCounts &K = h->kc[t];
            if (!K.kept) continue;
            if (!(rc = carry(t == 1, (uint32_t)K.rows, K.table, K.spare))) rc = carry(t == 1, (uint32_t)K.rows, K.delta, K.spare);
            K.cols = t == 1 ? c->nbr_used : c->n;
        }
        h->n = c->n;
        h->words = ((uint64_t)c->n + 31) / 32;
    }
    // T' = the new ids of T's survivors together with the added vertices, through the same map, before gnnpe_vde
    if (!rc) rc = gnnpe_csr_carry_vertex_set(c, T.bits[0], 1, T.bits[1], T.ids[1], T.room, &T.n_ids[1], device_ms ? &ms1 : nullptr);
    if (!rc && device_ms) *device_ms += ms1;
    if (!rc && c->have_table) rc = gnnpe_vde(c, nullptr, nullptr, nullptr);
    for (size_t i = 0; i < H.size() && !rc; i++)
        if (!(rc = standing_support_delta_device(H[i], T, 1, +1, device_ms))) rc = standing_derive(H[i], device_ms);
    // an added vertex is isolated: it completes a match of a single-vertex query only, which the general search covers
    std::vector<uint32_t> A(n_add);
    for (uint64_t i = 0; i < n_add; i++) A[i] = n_surv + (uint32_t)i;
    for (size_t i = 0; i < H.size() && !rc; i++) rc = standing_delta(who, H[i], false, A, 0, &H[i]->p_created, device_ms, true);
    if (!rc) rc = standing_fold_all(c, H, device_ms);
    if (rc) {
        for (gnnpe_standing *h : H) h->graph_gen = kStandingPoison;
        return rc;
    }
    standing_commit(c, H, true);
    return GNNPE_OK;
}

int gnnpe_standing_open(gnnpe_ctx *c, const char *query_graph_path, uint32_t l, double epsilon, uint32_t mode, uint64_t rows_cap,
                        gnnpe_standing **sq, uint64_t *count, double *device_ms)
{
    const char *who = "gnnpe_standing_open";
    if (sq) *sq = nullptr;
    GNNPE_REQUIRE(l == 2 || l == 3, GNNPE_ERR_UNSUPPORTED, "%s: l = %u (2 or 3)", who, l);
    return standing_open(who, c, query_graph_path, l, epsilon, mode, rows_cap, nullptr, sq, count, device_ms);
}

int gnnpe_standing_open_sets(gnnpe_ctx *c, const char *query_graph_path, uint32_t mode, uint64_t rows_cap, const uint32_t *host_bitmap,
                             gnnpe_standing **sq, uint64_t *count, double *device_ms)
{
    const char *who = "gnnpe_standing_open_sets";
    if (sq) *sq = nullptr;
    GNNPE_REQUIRE(host_bitmap, GNNPE_ERR_ARG, "%s: null argument", who);
    return standing_open(who, c, query_graph_path, 0, 0.0, mode, rows_cap, host_bitmap, sq, count, device_ms);
}

int gnnpe_standing_set_bitmap(gnnpe_standing *h, const uint32_t *host_bitmap)
{
    const char *who = "gnnpe_standing_set_bitmap";
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(host_bitmap, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(!h->filter, GNNPE_ERR_ARG, "%s: the handle keeps its own sets (gnnpe_standing_open); only gnnpe_standing_open_sets handles take a bitmap", who);
    GNNPE_HIP_TRY(hipSetDevice(h->c->device));
    GNNPE_HIP_TRY(hipStreamSynchronize(h->c->stream));
    const uint64_t bytes = (uint64_t)h->nq * h->words * 4;
    if (bytes) GNNPE_HIP_TRY(hipMemcpy(h->bitmap.p, host_bitmap, bytes, hipMemcpyHostToDevice));
    h->graph_gen = kStandingPoison;  // until the count below is in place
    return standing_compute(who, h, nullptr);
}

int gnnpe_standing_apply_edges(gnnpe_ctx *c, const uint32_t *insert_edges, uint64_t n_insert, const uint32_t *delete_edges, uint64_t n_delete,
                               double *device_ms)
{
    const char *who = "gnnpe_standing_apply_edges";
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(c && (insert_edges || n_insert == 0) && (delete_edges || n_delete == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = standing_whole_graph(who, c);
    if (rc) return rc;
    std::vector<gnnpe_standing *> H;
    bool induced = false;
    for (void *p : c->standing) {
        H.push_back(static_cast<gnnpe_standing *>(p));
        STANDING_LIVE(who, H.back());
        induced = induced || (H.back()->mode & GNNPE_MATCH_INDUCED) != 0;
    }
    GNNPE_REQUIRE(n_insert < (1ull << 30) && n_delete < (1ull << 30), GNNPE_ERR_ARG, "%s: %llu + %llu pairs, the key lists are 32-bit", who,
                  (unsigned long long)n_insert, (unsigned long long)n_delete);
    const std::vector<uint32_t> I(insert_edges, insert_edges + 2 * n_insert), D(delete_edges, delete_edges + 2 * n_delete), none;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    if ((rc = standing_check_batch(who, c, I, D))) return rc;
    for (gnnpe_standing *h : H) h->p_created = h->p_destroyed = h->p_held[0] = h->p_held[1] = 0;
    if (n_insert || n_delete) {
        bool want_map = false;  // a handle on the context keeps E: the applies hand out the entry map
        for (gnnpe_standing *h : H) want_map = want_map || h->kc[1].kept;
        if (want_map && (rc = standing_size_edge_tables(c, H, c->nbr_used + 2 * I.size()))) return rc;  // (each pair of I is two words)
        // an induced handle and a mixed batch: D first, then I (the header says why); otherwise one apply
        const bool split = induced && n_insert && n_delete;
        bool swapped = false;
        rc = standing_step(c, H, split ? none : I, D, &swapped, device_ms, want_map);
        if (rc && !swapped) return rc;  // refused with everything as it was
        if (!rc && split) rc = standing_step(c, H, I, none, &swapped, device_ms, want_map);
        // the batch is through: one fold per kept table moves D into T and leaves the batch's change list, in the cells of G'
        if (!rc) rc = standing_fold_all(c, H, device_ms);
        if (rc) {  // a failure behind a swap: the graph has moved on and the handles have not
            for (gnnpe_standing *h : H) h->graph_gen = kStandingPoison;
            return rc;
        }
    }
    standing_commit(c, H, n_insert || n_delete);
    return GNNPE_OK;
}

int gnnpe_standing_result(gnnpe_standing *h, uint64_t out[6])
{
    const char *who = "gnnpe_standing_result";
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(out, GNNPE_ERR_ARG, "%s: null argument", who);
    out[0] = h->count, out[1] = h->created, out[2] = h->destroyed, out[3] = h->held[0], out[4] = h->held[1], out[5] = h->graph_gen;
    return GNNPE_OK;
}

int gnnpe_standing_rows(gnnpe_standing *h, int which, uint32_t *host_rows, uint64_t cap, uint64_t *n_rows)
{
    const char *who = "gnnpe_standing_rows";
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(n_rows && (which == 0 || which == 1) && (host_rows || cap == 0), GNNPE_ERR_ARG, "%s: bad argument", who);
    *n_rows = h->held[which];
    const uint64_t take = std::min(cap, h->held[which]);
    GNNPE_HIP_TRY(hipSetDevice(h->c->device));
    if (take) GNNPE_HIP_TRY(hipMemcpy(host_rows, h->rows[which][h->cur].p, (size_t)take * h->nq * 4, hipMemcpyDeviceToHost));
    return GNNPE_OK;
}

int gnnpe_standing_set_sizes(gnnpe_standing *h, uint64_t *sizes)
{
    const char *who = "gnnpe_standing_set_sizes";
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(sizes, GNNPE_ERR_ARG, "%s: null argument", who);
    std::copy(h->sizes.begin(), h->sizes.end(), sizes);
    return GNNPE_OK;
}

int gnnpe_standing_set_members(gnnpe_standing *h, uint32_t u, uint32_t *host_ids, uint64_t cap, uint64_t *n_ids)
{
    const char *who = "gnnpe_standing_set_members";
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(n_ids && (host_ids || cap == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_REQUIRE(u < h->nq, GNNPE_ERR_ARG, "%s: query vertex %u of %u", who, u, h->nq);
    gnnpe_ctx *c = h->c;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    // no more room than ids can come out; behind it words that the kernel must leave as they are
    const uint64_t room = std::min<uint64_t>(cap, h->n);
    int rc = h->members.reserve((room + kMembersCanary) * 4);
    if (rc) return rc;
    uint32_t *d_ids = h->members.as<uint32_t>();
    unsigned long long *d_total = h->d_sizes.as<unsigned long long>() + h->nq;
    GNNPE_HIP_TRY(hipMemsetAsync(d_ids + room, 0xFF, kMembersCanary * 4, c->stream));
    GNNPE_HIP_TRY(sets_members_launch(c->stream, h->bitmap.as<uint32_t>() + (uint64_t)u * h->words, h->words, h->n, d_ids, room, d_total));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipMemcpyAsync(c->h_pinned + 1, d_ids + room, kMembersCanary * 4, hipMemcpyDeviceToHost, c->stream));
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    *n_ids = c->h_pinned[0];
    for (uint32_t i = 0; i < kMembersCanary / 2; i++)
        GNNPE_REQUIRE(c->h_pinned[1 + i] == ~0ull, GNNPE_ERR_HIP, "%s: internal error: ids were written past the %llu asked for", who, (unsigned long long)room);
    const uint64_t take = std::min<uint64_t>(room, *n_ids);
    if (take) GNNPE_HIP_TRY(hipMemcpy(host_ids, d_ids, (size_t)take * 4, hipMemcpyDeviceToHost));
    return GNNPE_OK;
}

int gnnpe_standing_bitmap(gnnpe_standing *h, uint32_t *host_bitmap)
{
    const char *who = "gnnpe_standing_bitmap";
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(host_bitmap, GNNPE_ERR_ARG, "%s: null argument", who);
    GNNPE_HIP_TRY(hipSetDevice(h->c->device));
    GNNPE_HIP_TRY(hipStreamSynchronize(h->c->stream));
    const uint64_t bytes = (uint64_t)h->nq * h->words * 4;
    if (bytes) GNNPE_HIP_TRY(hipMemcpy(host_bitmap, h->bitmap.p, bytes, hipMemcpyDeviceToHost));
    return GNNPE_OK;
}

int gnnpe_standing_table(gnnpe_standing *h, void **dev_table)
{
    const char *who = "gnnpe_standing_table";
    if (dev_table) *dev_table = nullptr;
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(dev_table, GNNPE_ERR_ARG, "%s: null argument", who);
    *dev_table = h->filter ? h->table.p : nullptr;
    return GNNPE_OK;
}

int gnnpe_standing_keep_counts(gnnpe_standing *h, uint32_t which, uint64_t changes_cap, double *device_ms)
{
    const char *who = "gnnpe_standing_keep_counts";
    if (device_ms) *device_ms = 0.0;
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(which && (which & ~(GNNPE_STANDING_VERTEX_COUNTS | GNNPE_STANDING_EDGE_COUNTS)) == 0, GNNPE_ERR_ARG,
                  "%s: which = 0x%x (GNNPE_STANDING_VERTEX_COUNTS, GNNPE_STANDING_EDGE_COUNTS or both)", who, which);
    gnnpe_ctx *c = h->c;
    int rc = standing_whole_graph(who, c);
    if (rc) return rc;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    // everything is made aside and handed over at the end: a refusal leaves the handle as it was
    StandingCounts fresh[2];
    DevBuf lists[2][2];
    const size_t list = std::max<uint64_t>(changes_cap * 8, 8);
    GNNPE_REQUIRE(changes_cap <= (1ull << 40), GNNPE_ERR_ARG, "%s: changes_cap %llu", who, (unsigned long long)changes_cap);
    for (int t = 0; t < 2; t++) {
        if (!h->kc[t].kept && (which >> t & 1u)) {
            if ((rc = standing_counts_build(who, h, t == 1, changes_cap, fresh[t], device_ms))) return rc;
        } else if (h->kc[t].kept && changes_cap != h->changes_cap) {
            if ((rc = lists[t][0].reserve(list)) || (rc = lists[t][1].reserve(list))) return rc;
        }
    }
    GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
    for (int t = 0; t < 2; t++) {
        if (fresh[t].kept) {
            h->kc[t].swap_with(fresh[t]);
        } else if (lists[t][0].p) {  // a table kept before, under a new cap: new change arrays, and the last batch's list is gone
            StandingCounts::swap(h->kc[t].ch_cells, lists[t][0]);
            StandingCounts::swap(h->kc[t].ch_deltas, lists[t][1]);
            h->kc[t].n_changes = 0;
        }
    }
    h->changes_cap = changes_cap;
    return GNNPE_OK;
}

// the kept table a call names with exactly one bit of `which`
static int standing_kept(const char *who, gnnpe_standing *h, uint32_t which, StandingCounts **K)
{
    GNNPE_REQUIRE(which == GNNPE_STANDING_VERTEX_COUNTS || which == GNNPE_STANDING_EDGE_COUNTS, GNNPE_ERR_ARG,
                  "%s: which = 0x%x (GNNPE_STANDING_VERTEX_COUNTS or GNNPE_STANDING_EDGE_COUNTS)", who, which);
    *K = &h->kc[which == GNNPE_STANDING_EDGE_COUNTS ? 1 : 0];
    GNNPE_REQUIRE((*K)->kept, GNNPE_ERR_ARG, "%s: the handle does not keep that table (gnnpe_standing_keep_counts)", who);
    return GNNPE_OK;
}

int gnnpe_standing_counts(gnnpe_standing *h, uint32_t which, uint64_t *host_counts, void **dev_counts, uint64_t *n_rows, uint64_t *n_cols)
{
    const char *who = "gnnpe_standing_counts";
    if (dev_counts) *dev_counts = nullptr;
    if (n_rows) *n_rows = 0;
    if (n_cols) *n_cols = 0;
    STANDING_LIVE(who, h);
    StandingCounts *K = nullptr;
    const int rc = standing_kept(who, h, which, &K);
    if (rc) return rc;
    if (dev_counts) *dev_counts = K->cells() ? K->table.p : nullptr;
    if (n_rows) *n_rows = K->rows;
    if (n_cols) *n_cols = K->cols;
    if (host_counts && K->cells()) {
        GNNPE_HIP_TRY(hipSetDevice(h->c->device));
        GNNPE_HIP_TRY(hipStreamSynchronize(h->c->stream));
        GNNPE_HIP_TRY(hipMemcpy(host_counts, K->table.p, K->cells() * 8, hipMemcpyDeviceToHost));
    }
    return GNNPE_OK;
}

int gnnpe_standing_count_changes(gnnpe_standing *h, uint32_t which, uint64_t *host_cells, int64_t *host_deltas, uint64_t cap, uint64_t *n_changes)
{
    const char *who = "gnnpe_standing_count_changes";
    if (n_changes) *n_changes = 0;
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(n_changes && ((host_cells && host_deltas) || cap == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    StandingCounts *K = nullptr;
    const int rc = standing_kept(who, h, which, &K);
    if (rc) return rc;
    *n_changes = K->n_changes;
    const uint64_t take = std::min(std::min(cap, h->changes_cap), K->n_changes);
    if (take) {
        GNNPE_HIP_TRY(hipSetDevice(h->c->device));
        GNNPE_HIP_TRY(hipStreamSynchronize(h->c->stream));
        GNNPE_HIP_TRY(hipMemcpy(host_cells, K->ch_cells.p, take * 8, hipMemcpyDeviceToHost));
        GNNPE_HIP_TRY(hipMemcpy(host_deltas, K->ch_deltas.p, take * 8, hipMemcpyDeviceToHost));
    }
    return GNNPE_OK;
}

// ---- peeling by edge support (the header: "PEELING THE GRAPH BY EDGE SUPPORT") -------------------------------------------------------

// what gnnpe_standing_peel and gnnpe_standing_truss_levels refuse before anything changes
static int standing_peel_check(const char *who, gnnpe_standing *h)
{
    STANDING_LIVE(who, h);
    GNNPE_REQUIRE(!(h->mode & GNNPE_MATCH_INDUCED), GNNPE_ERR_UNSUPPORTED,
                  "%s: an induced handle: a deletion can create induced matches, so the peel has no unique fixpoint", who);
    GNNPE_REQUIRE(h->nqe != 0, GNNPE_ERR_ARG, "%s: a query without an edge has no per-edge table", who);
    GNNPE_REQUIRE(h->kc[1].kept, GNNPE_ERR_ARG, "%s: the handle does not keep E (gnnpe_standing_keep_counts with GNNPE_STANDING_EDGE_COUNTS)", who);
    std::vector<gnnpe_standing *> H;  // every handle on the context goes along: a stale one would refuse the first round
    return standing_handles(who, h->c, &H);
}

// The rounds of one threshold: select, stop if nothing is selected, delete the selection as one batch.  The pairs of every round are
// appended to *removed (and the round, counted from round_base + 1, once per pair to *round if it is given).  out as
// gnnpe_standing_peel's; *min_kept: of the last select.  A failure returns with out saying how far the loop came.
static int standing_peel_rounds(gnnpe_standing *h, uint64_t min_support, uint32_t max_rounds, std::vector<uint32_t> *removed, std::vector<uint32_t> *round,
                                uint32_t round_base, uint64_t out[4], uint64_t *min_kept, double *ms)
{
    gnnpe_ctx *c = h->c;
    out[0] = out[1] = out[3] = 0;
    out[2] = c->nbr_used / 2;
    *min_kept = ~0ull;
    GNNPE_HIP_TRY(hipSetDevice(c->device));
    while (max_rounds == 0 || out[0] < max_rounds) {
        const StandingCounts &K = h->kc[1];
        const uint64_t room = c->nbr_used / 2;
        int rc = c->below_pairs.reserve(std::max<uint64_t>(room * 8, 8));
        if (rc) return rc;
        uint64_t n_sel = 0;
        double ms1 = 0.0;
        if ((rc = gnnpe_csr_edges_below(c, K.table.p, (uint32_t)K.rows, min_support, c->below_pairs.p, room, &n_sel, min_kept, ms ? &ms1 : nullptr))) return rc;
        if (ms) *ms += ms1;
        if (n_sel == 0) {
            out[3] = 1;
            break;
        }
        GNNPE_REQUIRE(n_sel <= room, GNNPE_ERR_HIP, "gnnpe_standing_peel: internal error: %llu edges selected of %llu", (unsigned long long)n_sel,
                      (unsigned long long)room);
        const size_t at = removed->size();
        removed->resize(at + 2 * n_sel);
        GNNPE_HIP_TRY(hipMemcpy(removed->data() + at, c->below_pairs.p, n_sel * 8, hipMemcpyDeviceToHost));
        if ((rc = gnnpe_standing_apply_edges(c, nullptr, 0, removed->data() + at, n_sel, ms ? &ms1 : nullptr))) {
            removed->resize(at);  // the round was refused as a batch is: graph and handles are those of the round before
            return rc;
        }
        if (ms) *ms += ms1;
        out[0]++;
        out[1] += n_sel;
        out[2] = c->nbr_used / 2;
        if (round) round->insert(round->end(), n_sel, round_base + (uint32_t)out[0]);
    }
    return GNNPE_OK;
}

int gnnpe_standing_peel(gnnpe_standing *h, uint64_t min_support, uint32_t max_rounds, uint32_t *host_removed, uint32_t *host_round, uint64_t cap,
                        uint64_t out[4], double *device_ms)
{
    const char *who = "gnnpe_standing_peel";
    if (device_ms) *device_ms = 0.0;
    if (out) out[0] = out[1] = out[2] = out[3] = 0;
    GNNPE_REQUIRE(h && out && (host_removed || cap == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = standing_peel_check(who, h);
    if (rc) return rc;
    std::vector<uint32_t> removed, round;
    uint64_t min_kept = 0;
    rc = standing_peel_rounds(h, min_support, max_rounds, &removed, &round, 0, out, &min_kept, device_ms);
    const uint64_t take = std::min<uint64_t>(cap, removed.size() / 2);  // what was removed is reported after a failure too
    if (take) memcpy(host_removed, removed.data(), take * 8);
    if (take && host_round) memcpy(host_round, round.data(), take * 4);
    return rc;
}

int gnnpe_standing_truss_levels(gnnpe_standing *h, int restore, uint32_t *host_edges, uint64_t *host_levels, uint64_t cap, uint64_t out[4],
                                double *device_ms)
{
    const char *who = "gnnpe_standing_truss_levels";
    if (device_ms) *device_ms = 0.0;
    if (out) out[0] = out[1] = out[2] = out[3] = 0;
    GNNPE_REQUIRE(h && out && ((host_edges && host_levels) || cap == 0), GNNPE_ERR_ARG, "%s: null argument", who);
    int rc = standing_peel_check(who, h);
    if (rc) return rc;
    gnnpe_ctx *c = h->c;
    std::vector<uint32_t> removed;
    uint64_t part[4], t = 0, listed = 0;
    // the first level: the smallest support of the graph, from a select that selects nothing
    if ((rc = standing_peel_rounds(h, 0, 1, &removed, nullptr, 0, part, &t, device_ms))) return rc;
    while (c->nbr_used) {
        GNNPE_REQUIRE(t != ~0ull, GNNPE_ERR_RANGE, "%s: a support of 2^64 - 1 has no threshold above it", who);
        const uint64_t level = t;
        rc = standing_peel_rounds(h, level + 1, 0, &removed, nullptr, 0, part, &t, device_ms);
        out[0] += part[1];
        out[3] += part[0];
        if (part[1]) out[1]++, out[2] = level;
        for (; listed < removed.size() / 2 && listed < cap; listed++) host_levels[listed] = level;
        if (rc) break;
        GNNPE_REQUIRE(part[1] != 0, GNNPE_ERR_HIP, "%s: internal error: no edge has the smallest support %llu", who, (unsigned long long)level);
    }
    const uint64_t take = std::min<uint64_t>(cap, removed.size() / 2);
    if (take) memcpy(host_edges, removed.data(), take * 8);
    if (rc) return rc;
    if (restore && !removed.empty()) {
        double ms1 = 0.0;
        if ((rc = gnnpe_standing_apply_edges(c, removed.data(), removed.size() / 2, nullptr, 0, device_ms ? &ms1 : nullptr))) return rc;
        if (device_ms) *device_ms += ms1;
    }
    return GNNPE_OK;
}

int gnnpe_standing_refresh(gnnpe_standing *h, uint64_t *count, double *device_ms)
{
    const char *who = "gnnpe_standing_refresh";
    if (count) *count = 0;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(h && count, GNNPE_ERR_ARG, "%s: null argument", who);
    h->graph_gen = kStandingPoison;  // a refresh that fails leaves a stale handle
    // the rows belong to a batch of the graph before
    const int rc = standing_compute(who, h, device_ms);
    if (rc) return rc;
    *count = h->count;
    return GNNPE_OK;
}

int gnnpe_standing_close(gnnpe_standing *h)
{
    if (!h) return GNNPE_OK;
    (void)hipSetDevice(h->c->device);
    (void)hipStreamSynchronize(h->c->stream);
    standing_unregister(h);
    delete h;
    return GNNPE_OK;
}

}  // extern "C"
