// gnnpe_refine_delta_counts.hip.h -- what the kernels that fill a count table over a search anchored at a set F share:
// k_refine_delta_vcount / k_refine_delta_ecount (gnnpe_refine_delta_counts.hip: F of data edges, VD_m and ED_m of
// include/gnnpe_online.h) and k_refine_delta_nonedges_vcount / k_refine_delta_nonedges_ecount
// (gnnpe_refine_delta_nonedges_counts.hip: F of non-edges, VN_m and EN_m).  On the device the look at the error flag of the lookup; on
// the host the whole call but the kernel it launches.  The text that explains the call is at the head of
// gnnpe_refine_delta_counts.hip.
#pragma once

#include "gnnpe_refine_delta.hip.h"
#include "gnnpe_refine_ecount.hip.h"

namespace gnnpe {

// has k_delta_entries met a pair that must not be in F (no edge where F holds edges, an edge where it holds non-edges)?  Final before
// a search launch starts.
__device__ __forceinline__ bool delta_refused(const SetsCounters *ctr)
{
    return uni(__hip_atomic_load(&ctr->bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0;
}

// what the launch of a table kernel takes beside the plan of its launch and the plan's pack
struct DeltaCountsLaunch {
    uint32_t blocks;
    const SetsDelta *older;  // of this launch
    const EcountEdges *X;    // of this launch; null for the vertex table
    uint32_t n_items;
    DeltaBuf F;
    uint32_t n_keys;
    uint64_t words;
    unsigned long long limit;
    SetsCounters *ctr;
    unsigned long long *table;
    uint64_t entries;  // the width of the edge table
    uint32_t n;        // the width of the vertex table
    unsigned long long one;
    const uint32_t *bitmap;  // the sets the search reads: the call's upload, or a standing query's resident bitmap
};

// The four device entries that fill a table over F after their names: the argument checks, the preparation of
// gnnpe_refine_sets_delta (with `nonedges` of gnnpe_refine_sets_delta_nonedges: the mode must be an induced one, the anchors of the
// launches are the query's non-adjacent pairs and F must hold no edge), the table (the context's own -- `own_v` or `own_e`, zeroed
// on the stream before the first launch -- or the caller's, untouched until a search kernel adds to it), the launches, the single
// wait and what comes back.  launch(c, A, K, ord...) starts the table kernel of one launch with the plan K.P.  With `res` (a standing
// query that keeps its count tables, gnnpe_standing.hip) the sets are on the device already: query_graph_path and candidate_bitmap are
// not read, nothing of the sets is uploaded and the kernels read res->d_bitmap.
template <class Launch>
static int delta_counts_call(const char *who, const char *tag, bool edge_table, bool nonedges, DevBuf gnnpe_ctx::*own_v,
                             DevBuf gnnpe_ctx::*own_e, gnnpe_ctx *c, const char *query_graph_path, const uint32_t *candidate_bitmap,
                             const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode, uint64_t *answers, int *complete,
                             uint64_t *host_counts, void **dev_counts, void *dev_accum, int sign, double *device_ms, Launch &&launch,
                             const SetsResident *res = nullptr)
{
    GNNPE_REQUIRE(c && (res || (query_graph_path && candidate_bitmap)) && answers && complete && (delta_edges || n_delta == 0), GNNPE_ERR_ARG,
                  "%s: null argument", who);
    *answers = 0;
    *complete = 0;
    if (dev_counts) *dev_counts = nullptr;
    if (device_ms) *device_ms = 0.0;
    GNNPE_REQUIRE(sign == 1 || (sign == -1 && dev_accum), GNNPE_ERR_ARG, "%s: sign must be +1, or -1 with dev_accum (got %d)", who, sign);
    GNNPE_REQUIRE(!(dev_accum && host_counts), GNNPE_ERR_ARG, "%s: host_counts must be NULL with dev_accum", who);
    if (nonedges) {
        GNNPE_REQUIRE((mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) == 0, GNNPE_ERR_ARG, "%s: unknown mode bits 0x%x", who, mode);
        GNNPE_REQUIRE((mode & GNNPE_MATCH_INDUCED) != 0, GNNPE_ERR_ARG, "%s: the mode must contain GNNPE_MATCH_INDUCED", who);
    }
    SetsQuery Q;
    gnnpe_host::StaticGraph q;
    int rc = sets_prepare(who, c, query_graph_path, candidate_bitmap, mode, limit, &Q, &q, res);
    if (rc) return rc;
    DeltaPlans D;
    if ((rc = delta_plans(who, c, Q, q, delta_edges, n_delta, mode, &D, nonedges))) return rc;
    if (limit == 0) return GNNPE_OK;  // nothing is launched, and nothing is complete
    // the rows of the edge table are the query EDGES, whatever anchors the launches
    const uint32_t nq = Q.nq, n = c->n, nqe = (uint32_t)(nonedges ? gnnpe_host::query_edges(q).size() : D.qe.size());
    const uint64_t entries = c->nbr_used;  // offsets[n] of gnnpe_load_csr
    const size_t cells = edge_table ? (size_t)nqe * entries : (size_t)nq * n, table_bytes = cells * 8;
    unsigned long long *table = static_cast<unsigned long long *>(dev_accum);
    if (!dev_accum && cells) {
        // context-owned, grow-only, of its own: the views of the other count calls are not disturbed
        DevBuf &own = c->*(edge_table ? own_e : own_v);
        if ((rc = own.reserve(table_bytes))) return rc;
        table = own.as<unsigned long long>();
    }
    if (dev_counts) *dev_counts = table;
    if (D.nothing) {  // an empty set, no F, a query without an anchor: a zero table is the whole answer; a caller's table stays as it is
        if (!dev_accum && table_bytes) {
            GNNPE_HIP_TRY(hipMemsetAsync(table, 0, table_bytes, c->stream));
            GNNPE_HIP_TRY(hipStreamSynchronize(c->stream));
            if (host_counts) std::fill(host_counts, host_counts + cells, 0ull);
        }
        *complete = 1;
        return GNNPE_OK;
    }
    const size_t n_keys = D.keys.size();
    if ((rc = c->q_work.reserve(SetsWork::kCtrBytes)) || (!res && (rc = c->q_bitmap.reserve((size_t)nq * Q.words * 4))) ||
        (rc = c->q_delta.reserve(DeltaBuf::bytes(n_keys))))
        return rc;
    // the words of the plan edges, per launch as the plans are; position 1 of a plan anchored at a non-adjacent pair has no edge
    std::vector<EcountEdges> X(edge_table ? D.plans.size() : 0);
    uint32_t flips = 0, backflips = 0;
    for (size_t k = 0; k < X.size(); k++) {
        const uint32_t got = ecount_edges_from_plan(D.plans[k].P, &X[k], &flips, &backflips, nonedges);
        GNNPE_REQUIRE(got == nqe, GNNPE_ERR_ARG, "%s: the plan of launch %zu has %u query edges, the query %u", who, k, got, nqe);
    }
    SetsCounters *ctr = c->q_work.as<SetsCounters>();
    const unsigned long long one = sign == 1 ? 1ull : ~0ull;
    SetsCall call(who, c, device_ms != nullptr);
    const uint32_t blocks = delta_stage(call, c, Q, D, candidate_bitmap, nonedges, nullptr, nullptr, nullptr, res);
    const uint32_t *d_bitmap = res ? res->d_bitmap : c->q_bitmap.as<uint32_t>();
    if (c->sw.debug) {
        fprintf(stderr, "[%s] edges=%zu items=%u launches=%zu blocks=%u pairs=%u nonedges=%u accum=%d sign=%d", tag, n_keys, D.n_items,
                D.plans.size(), blocks, D.plans[0].n_pairs, D.plans[0].n_non, dev_accum != nullptr, sign);
        if (nonedges) fprintf(stderr, " pivot2=%u", (uint32_t)D.plans[0].P.pivot[2]);
        fprintf(stderr, "\n");
    }
    if (call.ok() && !dev_accum && table_bytes) call.he = hipMemsetAsync(table, 0, table_bytes, c->stream);  // once per call, before the first launch
    delta_launches(call, c, D, [&](size_t k, const SetsQuery &K, auto... ord) {
        const DeltaCountsLaunch A = {blocks, &D.older[k], edge_table ? &X[k] : nullptr, D.n_items, DeltaBuf(c->q_delta, n_keys),
                                     (uint32_t)n_keys, Q.words, (unsigned long long)limit, ctr, table, entries, n, one, d_bitmap};
        launch(c, A, K, ord...);
    });
    call.wait(ctr, sizeof(SetsCounters));  // all of it: `bad` is in the second half
    if (call.ok()) {
        if (reinterpret_cast<const SetsCounters *>(c->h_pinned)->bad) {
            if (nonedges) set_error("%s: a pair is an edge of the graph", who);
            else set_error("%s: a delta edge is not an edge of the graph", who);
            call.rc = GNNPE_ERR_ARG;
        } else {
            *answers = std::min<uint64_t>(c->h_pinned[0], limit);
            *complete = c->h_pinned[0] < limit ? 1 : 0;
            if (c->sw.debug)
                fprintf(stderr, "[%s] finds=%llu flush_adds=%llu complete=%d\n", tag, (unsigned long long)c->h_pinned[0],
                        (unsigned long long)c->h_pinned[1], *complete);
            if (host_counts && *complete && table_bytes) call.he = hipMemcpy(host_counts, table, table_bytes, hipMemcpyDeviceToHost);
        }
    }
    return call.finish(device_ms);
}

}  // namespace gnnpe
