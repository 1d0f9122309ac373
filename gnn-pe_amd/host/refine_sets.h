// refine_sets.h -- the SET-RESTRICTED refinement on the host: the CPU yardstick of csrc/gnnpe_refine_sets.hip.
//
// M = the maps f from query vertices to data vertices that are injective, keep labels, have query degree <= data degree, map
// every query edge onto a data edge, and have f(u) in C(u) for EVERY query vertex u; R(C, limit) = min(limit, |M|)
// (include/gnnpe_online.h).  host/refine.h restricts the start vertex only, as the reference does; where every C(u) is
// complete the two agree, and both equal the true embedding count.  Plain backtracking in the order of
// build_match_order (refine.h); the count does not depend on the order.  One entry, refine_sets_run, serves every result kind
// of the header.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "graph_loader.h"

namespace gnnpe_host {

// cnt[u] = |C(u)|: the set bits of bitmap row u (rows of `words` uint32, as below)
inline std::vector<uint64_t> set_sizes(const uint32_t *bitmap, uint64_t words, uint32_t nq)
{
    std::vector<uint64_t> cnt(nq, 0);
    for (uint32_t u = 0; u < nq; u++)
        for (uint64_t w = 0; w < words; w++) cnt[u] += (uint64_t)__builtin_popcount(bitmap[(size_t)u * words + w]);
    return cnt;
}

// the members of C(u) below n, ascending (the last word of a row may carry bits past the graph)
inline std::vector<uint32_t> set_members(const uint32_t *bitmap, uint64_t words, uint32_t u, uint32_t n)
{
    std::vector<uint32_t> out;
    for (uint64_t w = 0; w < words; w++)
        for (uint32_t bits = bitmap[(size_t)u * words + w]; bits; bits &= bits - 1) {
            const uint64_t v = w * 32 + __builtin_ctz(bits);
            if (v < n) out.push_back((uint32_t)v);
        }
    return out;
}

// One search, two axes.  M is walked by the same backtracking whatever is asked; a SetsJob says
//   which of them count: `pairs` (only the maps with f(a) < f(b) for every pair (a, b) -- with the pairs of query_symmetry.h one
//       embedding per distinct subgraph), `induced` (only the maps that also send every two distinct, non-adjacent query vertices
//       to non-adjacent data vertices), and F = `delta_edges` where `through` is set (only the maps that put at least one query
//       edge on an edge of F, each once: one test at every find, nothing shared with the edge-anchored search of
//       csrc/gnnpe_refine_delta.hip, whose yardstick this is);
//   what every find that counts adds to: nothing, the vertex table (counts[u * data.n + v] += 1 for every query vertex u, v its
//       image) or the edge table (counts[k * data.offsets[data.n] + j] += 1 for every query edge k = (a_k, b_k) of query_edges, j
//       the adjacency entry f(a_k) -> f(b_k) of the data CSR, found by binary search in the row of f(a_k)).
// In the names of include/gnnpe_online.h:       no table            vertex table   edge table
//   all of M (through = false)                  R, D, I, ID         V_m(C)         E_m(C)
//   the maps through F (through = true)         Delta_m(C, F)       VDelta_m(C, F) EDelta_m(C, F)
//   ... F of non-edges (nonedges = true)        N_m(C, F)           VN_m(C, F)     EN_m(C, F)
//   the maps with an image in S (through_vertices)  DeltaV_m(C, S)  VV_m(C, S)     EV_m(C, S)
struct SetsJob {
    const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr;
    bool induced = false;
    enum Table { kNoTable, kVertexTable, kEdgeTable } table = kNoTable;
    bool through = false;
    bool nonedges = false;  // with `through` and `induced`: F holds NON-edges of the graph, and a map counts if it puts a
                            // non-adjacent query pair (query_nonedges) on one of them -- N_m(C, F) of include/gnnpe_online.h; a table
                            // is filled as for any other job (the rows of the edge table are still the query EDGES)
    const uint32_t *delta_edges = nullptr;  // F: n_delta pairs (x, y), either orientation, repeats tolerated; read where `through`
    uint64_t n_delta = 0;
    bool through_vertices = false;  // only the maps with at least one image in S = `vertices`, each once: DeltaV_m(C, S) of
                                    // include/gnnpe_online.h.  One test at every find against a byte mask of S; not with `through`
    const uint32_t *vertices = nullptr;  // S: n_vertices ids, repeats tolerated; read where `through_vertices`
    uint64_t n_vertices = 0;
};

// The query edges as include/gnnpe_online.h numbers them: (a_k, b_k) with a_k < b_k, lexicographically ascending, each once.
std::vector<std::pair<uint32_t, uint32_t>> query_edges(const StaticGraph &query);

// The non-adjacent pairs of the query as include/gnnpe_online.h numbers them: (a_k, b_k) with a_k < b_k, lexicographically ascending.
std::vector<std::pair<uint32_t, uint32_t>> query_nonedges(const StaticGraph &query);

// An undirected data edge {x, y} as one word: (min << 32) | max.
inline uint64_t delta_key(uint32_t x, uint32_t y) { return ((uint64_t)std::min(x, y) << 32) | std::max(x, y); }

// F of the delta calls as ascending keys, each edge once: delta_edges holds n_delta pairs (x, y), either orientation, repeats
// tolerated.  A loop or an id >= n returns <0 with *err; whether a pair is an edge of the graph is not looked at here.
int delta_edge_keys(uint32_t n, const uint32_t *delta_edges, uint64_t n_delta, std::vector<uint64_t> *keys, std::string *err);

// S of the vertex-anchored calls as ascending ids, each once: vertices holds n_vertices ids, repeats tolerated.  An id >= n returns
// <0 with *err.
int delta_vertex_ids(uint32_t n, const uint32_t *vertices, uint64_t n_vertices, std::vector<uint32_t> *ids, std::string *err);

// The cells of a job's table: query.n * data.n, query edges * adjacency entries, or 0 without a table.  A query without an edge
// has no edge table.
size_t sets_table_cells(const StaticGraph &data, const StaticGraph &query, SetsJob::Table table);

// bitmap: query.n rows of `words` = ceil(data.n / 32) uint32, bit v of row u set <=> v in C(u) (the layout
// gnnpe_filter_candidates writes).  Returns 0 with *answers = min(limit, the maps that count), or <0 with *err and *answers = 0.
// With a table, limit is a guard: *complete = the maps that count < limit (limit 0 walks nothing, and 0 < 0 is false), and the
// table is exact only where *complete (all zeros and complete where a set is empty); without one, complete may be null.  counts
// holds sets_table_cells cells and may be null where that is 0.
// In this order: a null complete, or a null counts with cells, is refused; then F -- a loop, an id >= data.n, a pair that is no
// edge of the graph (binary search in the data row; with `nonedges` a pair that IS one) -- with counts still untouched; then the table is zeroed; then the walk refuses
// a bitmap of other than `words` words per row, an ordering pair outside the query and a disconnected query graph, whatever the
// limit, leaving the zeroed table.  An empty F drops every find: the walk runs with limit 0 and still refuses what it refuses,
// *answers is 0 and *complete is 0 < limit.  S of a `through_vertices` job is checked where F is (an id >= data.n, or both flags set, is
// refused), and an empty S drops every find in the same way.
int refine_sets_run(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words, uint64_t limit,
                    const SetsJob &job, uint64_t *answers, bool *complete, uint64_t *counts, std::string *err);

}  // namespace gnnpe_host
