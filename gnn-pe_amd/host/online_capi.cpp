// online_capi.cpp -- C-ABI of the host refinements (include/gnnpe_online.h).  Compiled into libgnnpe_online.so, which links
// against libgnnpe_hip.so for the loader and the error text.  Out of SURVEY section 8's scope (frozen).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gnnpe_online.h"
#include "graph_loader.h"
#include "refine.h"
#include "query_symmetry.h"
#include "refine_sets.h"

namespace gnnpe {
void set_error(const char *fmt, ...);
}

// load the query graph, or set the error text and return the loader's code
static int load_query(const char *path, gnnpe_host::StaticGraph *q)
{
    std::string err;
    const int rc = q->load(path, &err, true);
    if (rc != 0) gnnpe::set_error("%s", err.c_str());
    return rc;
}

static gnnpe_host::StaticGraph graph_from_csr(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels)
{
    gnnpe_host::StaticGraph g;
    g.n = n;
    g.offsets.assign(offsets, offsets + n + 1);
    g.neighbors.assign(nbrs, nbrs + offsets[n]);
    g.labels.assign(labels, labels + n);
    return g;
}

extern "C" {

int gnnpe_host_refine(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                      const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint64_t *answers)
{
    if (!offsets || !nbrs || !labels || !query_graph_path || !candidate_bitmap || !answers) {
        gnnpe::set_error("gnnpe_host_refine: null argument");
        return GNNPE_ERR_ARG;
    }
    gnnpe_host::StaticGraph q;
    std::string err;
    if (int rc = load_query(query_graph_path, &q)) return rc;
    const gnnpe_host::StaticGraph g = graph_from_csr(n, offsets, nbrs, labels);
    const uint64_t words = ((uint64_t)n + 31) / 32;
    std::vector<std::vector<uint32_t>> cand(q.n);
    for (uint32_t u = 0; u < q.n; u++)
        for (uint64_t w = 0; w < words; w++)
            for (uint32_t bits = candidate_bitmap[(size_t)u * words + w]; bits; bits &= bits - 1)
                cand[u].push_back((uint32_t)(w * 32 + __builtin_ctz(bits)));
    if (gnnpe_host::refine_count(g, q, cand, limit, answers, &err) != 0) {
        gnnpe::set_error("%s", err.c_str());
        return GNNPE_ERR_ARG;
    }
    return 0;
}

// The host entries of the set-restricted refinement are this one sequence: null checks, outputs cleared, unknown mode
// bits, query load, the search (gnnpe_host::refine_sets_run), its refusal as the error text.  An entry is its name, its table kind
// and whether it has F (`through`); what differs between them follows from those two:
//   null checks   offsets, nbrs, labels, query_graph_path, candidate_bitmap and answers always; complete with a table; counts with
//                 the vertex table only -- the edge table of a query without an edge is empty, so the search looks at counts once
//                 the query is known; delta_edges unless n_delta is 0
//   cleared       before the mode check *answers = 0 and *complete = 0 -- but not by the three entries with neither table nor F,
//                 which leave *answers alone until the search starts
//   refusal text  the search's own; with F behind "<who>: ".  A query that does not load returns the loader's code and text as
//                 they are, in all of them.  *answers is 0 after a refusal of the search.
// mode 0 and GNNPE_MATCH_DISTINCT are what gnnpe_host_refine_sets and gnnpe_host_refine_sets_distinct pass.
static int host_sets(const char *who, gnnpe_host::SetsJob::Table table, bool through, uint32_t n, const uint32_t *offsets,
                     const uint32_t *nbrs, const uint32_t *labels, const char *query_graph_path, const uint32_t *candidate_bitmap,
                     const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode, uint64_t *answers, int *complete,
                     uint64_t *counts, bool nonedges = false, bool vertices = false)
{
    const bool has_table = table != gnnpe_host::SetsJob::kNoTable;
    if (!offsets || !nbrs || !labels || !query_graph_path || !candidate_bitmap || !answers || (has_table && !complete) ||
        (table == gnnpe_host::SetsJob::kVertexTable && !counts) || (!delta_edges && n_delta)) {
        gnnpe::set_error("%s: null argument", who);
        return GNNPE_ERR_ARG;
    }
    if (has_table || through) *answers = 0;
    if (has_table) *complete = 0;
    if (mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) {
        gnnpe::set_error("%s: unknown mode bits 0x%x", who, mode);
        return GNNPE_ERR_ARG;
    }
    if (nonedges && !(mode & GNNPE_MATCH_INDUCED)) {
        gnnpe::set_error("%s: the mode must contain GNNPE_MATCH_INDUCED", who);
        return GNNPE_ERR_ARG;
    }
    gnnpe_host::StaticGraph q;
    if (int rc = load_query(query_graph_path, &q)) return rc;
    const gnnpe_host::StaticGraph g = graph_from_csr(n, offsets, nbrs, labels);
    gnnpe_host::QuerySymmetry sym;
    gnnpe_host::SetsJob job;
    if (mode & GNNPE_MATCH_DISTINCT) {
        sym = gnnpe_host::query_symmetry(q);
        job.pairs = &sym.pairs;
    }
    job.induced = (mode & GNNPE_MATCH_INDUCED) != 0;
    job.table = table;
    job.through = through && !vertices;
    job.nonedges = nonedges;
    job.delta_edges = vertices ? nullptr : delta_edges;
    job.n_delta = vertices ? 0 : n_delta;
    job.through_vertices = vertices;  // (S travels in the arguments of F: n_delta ids)
    job.vertices = vertices ? delta_edges : nullptr;
    job.n_vertices = vertices ? n_delta : 0;
    std::string err;
    bool done = false;
    if (gnnpe_host::refine_sets_run(g, q, candidate_bitmap, ((uint64_t)n + 31) / 32, limit, job, answers, &done, counts, &err) != 0) {
        if (through) gnnpe::set_error("%s: %s", who, err.c_str());
        else gnnpe::set_error("%s", err.c_str());
        return GNNPE_ERR_ARG;
    }
    if (has_table) *complete = done ? 1 : 0;
    return 0;
}

#define HOST_SETS(entry, table, through, delta_edges, n_delta, mode, complete, counts)                                              \
    host_sets(#entry, gnnpe_host::SetsJob::table, through, n, offsets, nbrs, labels, query_graph_path, candidate_bitmap, delta_edges, \
              n_delta, limit, mode, answers, complete, counts)

int gnnpe_host_refine_sets(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                           const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint64_t *answers)
{
    return HOST_SETS(gnnpe_host_refine_sets, kNoTable, false, nullptr, 0, 0u, nullptr, nullptr);
}

int gnnpe_host_refine_sets_distinct(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                    const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint64_t *answers)
{
    return HOST_SETS(gnnpe_host_refine_sets_distinct, kNoTable, false, nullptr, 0, GNNPE_MATCH_DISTINCT, nullptr, nullptr);
}

int gnnpe_host_refine_sets_mode(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                                uint64_t *answers)
{
    return HOST_SETS(gnnpe_host_refine_sets_mode, kNoTable, false, nullptr, 0, mode, nullptr, nullptr);
}

int gnnpe_host_refine_sets_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                         const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                                         uint64_t *answers, int *complete, uint64_t *counts)
{
    return HOST_SETS(gnnpe_host_refine_sets_vertex_counts, kVertexTable, false, nullptr, 0, mode, complete, counts);
}

int gnnpe_host_refine_sets_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                       const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                                       uint64_t *answers, int *complete, uint64_t *counts)
{
    return HOST_SETS(gnnpe_host_refine_sets_edge_counts, kEdgeTable, false, nullptr, 0, mode, complete, counts);
}

int gnnpe_host_refine_sets_delta(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                 const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *delta_edges,
                                 uint64_t n_delta, uint64_t limit, uint32_t mode, uint64_t *answers)
{
    return HOST_SETS(gnnpe_host_refine_sets_delta, kNoTable, true, delta_edges, n_delta, mode, nullptr, nullptr);
}

int gnnpe_host_refine_sets_delta_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                               const char *query_graph_path, const uint32_t *candidate_bitmap,
                                               const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                               uint64_t *answers, int *complete, uint64_t *counts)
{
    return HOST_SETS(gnnpe_host_refine_sets_delta_vertex_counts, kVertexTable, true, delta_edges, n_delta, mode, complete, counts);
}

int gnnpe_host_refine_sets_delta_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                             const char *query_graph_path, const uint32_t *candidate_bitmap,
                                             const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                             uint64_t *answers, int *complete, uint64_t *counts)
{
    return HOST_SETS(gnnpe_host_refine_sets_delta_edge_counts, kEdgeTable, true, delta_edges, n_delta, mode, complete, counts);
}
#undef HOST_SETS

// (the ninth entry of that sequence: F holds non-edges, the mode must be an induced one)
int gnnpe_host_refine_sets_delta_nonedges(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                          const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *pairs,
                                          uint64_t n_pairs, uint64_t limit, uint32_t mode, uint64_t *answers)
{
    return host_sets("gnnpe_host_refine_sets_delta_nonedges", gnnpe_host::SetsJob::kNoTable, true, n, offsets, nbrs, labels, query_graph_path,
                     candidate_bitmap, pairs, n_pairs, limit, mode, answers, nullptr, nullptr, true);
}

// (the tenth and the eleventh: the tables of those maps)
int gnnpe_host_refine_sets_delta_nonedges_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                        const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                        const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                        uint64_t *answers, int *complete, uint64_t *counts)
{
    return host_sets("gnnpe_host_refine_sets_delta_nonedges_vertex_counts", gnnpe_host::SetsJob::kVertexTable, true, n, offsets, nbrs, labels,
                     query_graph_path, candidate_bitmap, pairs, n_pairs, limit, mode, answers, complete, counts, true);
}

int gnnpe_host_refine_sets_delta_nonedges_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                      const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                      const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                      uint64_t *answers, int *complete, uint64_t *counts)
{
    return host_sets("gnnpe_host_refine_sets_delta_nonedges_edge_counts", gnnpe_host::SetsJob::kEdgeTable, true, n, offsets, nbrs, labels,
                     query_graph_path, candidate_bitmap, pairs, n_pairs, limit, mode, answers, complete, counts, true);
}

// (the twelfth: S, a set of data vertices, in the place of F)
int gnnpe_host_refine_sets_delta_vertices(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                          const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *vertices,
                                          uint64_t n_vertices, uint64_t limit, uint32_t mode, uint64_t *answers)
{
    return host_sets("gnnpe_host_refine_sets_delta_vertices", gnnpe_host::SetsJob::kNoTable, true, n, offsets, nbrs, labels, query_graph_path,
                     candidate_bitmap, vertices, n_vertices, limit, mode, answers, nullptr, nullptr, false, true);
}

// (the thirteenth and the fourteenth: the tables of those maps, VV_m(C, S) and EV_m(C, S); these two clear *answers and *complete
// before the null checks as well, so that every refusal leaves 0 in them)
int gnnpe_host_refine_sets_delta_vertices_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                        const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                        const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                        uint64_t *answers, int *complete, uint64_t *counts)
{
    if (answers) *answers = 0;
    if (complete) *complete = 0;
    return host_sets("gnnpe_host_refine_sets_delta_vertices_vertex_counts", gnnpe_host::SetsJob::kVertexTable, true, n, offsets, nbrs, labels,
                     query_graph_path, candidate_bitmap, vertices, n_vertices, limit, mode, answers, complete, counts, false, true);
}

int gnnpe_host_refine_sets_delta_vertices_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                      const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                      const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                      uint64_t *answers, int *complete, uint64_t *counts)
{
    if (answers) *answers = 0;
    if (complete) *complete = 0;
    return host_sets("gnnpe_host_refine_sets_delta_vertices_edge_counts", gnnpe_host::SetsJob::kEdgeTable, true, n, offsets, nbrs, labels,
                     query_graph_path, candidate_bitmap, vertices, n_vertices, limit, mode, answers, complete, counts, false, true);
}

int gnnpe_host_query_edges(const char *query_graph_path, uint32_t *edges, uint32_t cap, uint32_t *n_edges)
{
    if (!query_graph_path || !n_edges || (!edges && cap)) {
        gnnpe::set_error("gnnpe_host_query_edges: null argument");
        return GNNPE_ERR_ARG;
    }
    gnnpe_host::StaticGraph q;
    if (int rc = load_query(query_graph_path, &q)) return rc;
    const std::vector<std::pair<uint32_t, uint32_t>> qe = gnnpe_host::query_edges(q);
    *n_edges = (uint32_t)qe.size();
    if (qe.size() > cap) {
        gnnpe::set_error("gnnpe_host_query_edges: %zu edges, room for %u", qe.size(), cap);
        return GNNPE_ERR_ARG;
    }
    for (size_t k = 0; k < qe.size(); k++) {
        edges[2 * k] = qe[k].first;
        edges[2 * k + 1] = qe[k].second;
    }
    return 0;
}

int gnnpe_host_query_nonedges(const char *query_graph_path, uint32_t *pairs, uint32_t cap, uint32_t *n_pairs)
{
    if (!query_graph_path || !n_pairs || (!pairs && cap)) {
        gnnpe::set_error("gnnpe_host_query_nonedges: null argument");
        return GNNPE_ERR_ARG;
    }
    gnnpe_host::StaticGraph q;
    if (int rc = load_query(query_graph_path, &q)) return rc;
    const std::vector<std::pair<uint32_t, uint32_t>> qn = gnnpe_host::query_nonedges(q);
    *n_pairs = (uint32_t)qn.size();
    if (qn.size() > cap) {
        gnnpe::set_error("gnnpe_host_query_nonedges: %zu pairs, room for %u", qn.size(), cap);
        return GNNPE_ERR_ARG;
    }
    for (size_t k = 0; k < qn.size(); k++) {
        pairs[2 * k] = qn[k].first;
        pairs[2 * k + 1] = qn[k].second;
    }
    return 0;
}

// The host form of gnnpe_standing_truss_levels, and the library's own slow statement of the definition: every round counts the
// table E of the graph as it is from scratch (gnnpe_host_refine_sets_edge_counts), selects with gnnpe_host_csr_edges_below and
// rebuilds the CSR without the selected edges.
int gnnpe_host_truss_levels(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels, const char *query_graph_path,
                            const uint32_t *candidate_bitmap, uint32_t mode, uint32_t *edges, uint64_t *levels, uint64_t cap, uint64_t out[4])
{
    const char *who = "gnnpe_host_truss_levels";
    if (!offsets || (!nbrs && offsets[n]) || (!labels && n) || !query_graph_path || !candidate_bitmap || !out || ((!edges || !levels) && cap)) {
        gnnpe::set_error("%s: null argument", who);
        return GNNPE_ERR_ARG;
    }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (mode & ~(GNNPE_MATCH_DISTINCT | GNNPE_MATCH_INDUCED)) {
        gnnpe::set_error("%s: unknown mode bits 0x%x", who, mode);
        return GNNPE_ERR_ARG;
    }
    if (mode & GNNPE_MATCH_INDUCED) {
        gnnpe::set_error("%s: induced matching: a deletion can create matches, so the peel has no unique fixpoint", who);
        return GNNPE_ERR_UNSUPPORTED;
    }
    gnnpe_host::StaticGraph q;
    if (int rc = load_query(query_graph_path, &q)) return rc;
    const uint32_t nqe = (uint32_t)gnnpe_host::query_edges(q).size();
    if (nqe == 0) {
        gnnpe::set_error("%s: a query without an edge has no per-edge table", who);
        return GNNPE_ERR_ARG;
    }
    std::vector<uint32_t> off(offsets, offsets + n + 1), nb(nbrs, nbrs + offsets[n]), sel, off2, nb2;
    std::vector<uint64_t> table;
    uint64_t t = 0, n_out = 0;
    bool have_t = false, counted = false;
    while (!nb.empty()) {
        const uint64_t entries = nb.size();
        if (!counted) {
            table.assign((size_t)nqe * entries, 0);
            uint64_t answers = 0;
            int complete = 0;
            if (int rc = gnnpe_host_refine_sets_edge_counts(n, off.data(), nb.data(), labels, query_graph_path, candidate_bitmap, ~0ull, mode, &answers,
                                                            &complete, table.data()))
                return rc;
            counted = true;
        }
        uint64_t n_sel = 0, low = 0;
        sel.resize(entries);  // two words per undirected edge
        if (int rc = gnnpe_host_csr_edges_below(n, off.data(), nb.data(), table.data(), nqe, have_t ? t + 1 : 0, sel.data(), entries / 2, &n_sel, &low))
            return rc;
        if (n_sel == 0) {  // the level is peeled (or not known yet): the next one is the smallest support left
            if (low == ~0ull) {
                gnnpe::set_error("%s: a support of 2^64 - 1 has no threshold above it", who);
                return GNNPE_ERR_RANGE;
            }
            t = low;
            have_t = true;
            out[1]++;
            continue;
        }
        for (uint64_t i = 0; i < n_sel; i++, n_out++)
            if (n_out < cap) edges[2 * n_out] = sel[2 * i], edges[2 * n_out + 1] = sel[2 * i + 1], levels[n_out] = t;
        out[3]++;
        // the CSR without the selected edges: `sel` is ascending in (x, y)
        std::vector<uint64_t> gone;
        gone.reserve(2 * n_sel);
        for (uint64_t i = 0; i < n_sel; i++) {
            gone.push_back(((uint64_t)sel[2 * i] << 32) | sel[2 * i + 1]);
            gone.push_back(((uint64_t)sel[2 * i + 1] << 32) | sel[2 * i]);
        }
        std::sort(gone.begin(), gone.end());
        off2.assign((size_t)n + 1, 0);
        nb2.clear();
        for (uint32_t x = 0; x < n; x++) {
            for (uint32_t j = off[x]; j < off[x + 1]; j++)
                if (!std::binary_search(gone.begin(), gone.end(), ((uint64_t)x << 32) | nb[j])) nb2.push_back(nb[j]);
            off2[x + 1] = (uint32_t)nb2.size();
        }
        off.swap(off2);
        nb.swap(nb2);
        counted = false;
    }
    out[0] = n_out;
    out[2] = have_t ? t : 0;
    return 0;
}

int gnnpe_host_query_symmetry(const char *query_graph_path, uint64_t *n_automorphisms, uint32_t *pairs, uint32_t pairs_cap,
                              uint32_t *n_pairs)
{
    if (!query_graph_path || !n_automorphisms || !n_pairs || (!pairs && pairs_cap)) {
        gnnpe::set_error("gnnpe_host_query_symmetry: null argument");
        return GNNPE_ERR_ARG;
    }
    gnnpe_host::StaticGraph q;
    if (int rc = load_query(query_graph_path, &q)) return rc;
    const gnnpe_host::QuerySymmetry sym = gnnpe_host::query_symmetry(q);
    *n_automorphisms = sym.n_automorphisms;
    *n_pairs = (uint32_t)sym.pairs.size();
    if (sym.pairs.size() > pairs_cap) {
        gnnpe::set_error("gnnpe_host_query_symmetry: %zu pairs, room for %u", sym.pairs.size(), pairs_cap);
        return GNNPE_ERR_ARG;
    }
    for (size_t k = 0; k < sym.pairs.size(); k++) {
        pairs[2 * k] = sym.pairs[k].first;
        pairs[2 * k + 1] = sym.pairs[k].second;
    }
    return 0;
}

}  // extern "C"
