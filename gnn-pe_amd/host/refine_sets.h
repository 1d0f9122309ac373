// refine_sets.h -- the SET-RESTRICTED refinement on the host: the CPU yardstick of csrc/gnnpe_refine_sets.hip.
//
// R(C, limit) = min(limit, number of maps f from query vertices to data vertices that are injective, keep labels, have
// query degree <= data degree, map every query edge onto a data edge, and have f(u) in C(u) for EVERY query vertex u)
// (include/gnnpe_online.h).  host/refine.h restricts the start vertex only, as the reference does; where every C(u) is
// complete the two agree, and both equal the true embedding count.  Plain backtracking in the order of
// build_match_order (refine.h); the count does not depend on the order.
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

// bitmap: query.n rows of `words` = ceil(data.n / 32) uint32, bit v of row u set <=> v in C(u) (the layout
// gnnpe_filter_candidates writes).  Returns 0 and *answers, or <0 with *err (disconnected query graph).
// pairs (optional): only the maps with f(a) < f(b) for every pair (a, b) are counted -- with the pairs of query_symmetry.h this is
// D(C, limit), one embedding per distinct subgraph.
// induced: only the maps that also send every two distinct, non-adjacent query vertices to non-adjacent data vertices are counted
// -- I(C, limit), or with the pairs ID(C, limit).
int refine_sets_count(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                      uint64_t limit, uint64_t *answers, std::string *err,
                      const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr, bool induced = false);

// V_m(C) of include/gnnpe_online.h: counts[u * data.n + v] = the number of the maps refine_sets_count counts (same pairs, same
// induced) that send query vertex u to data vertex v.  limit is a guard: *answers = min(|M|, limit), *complete = |M| < limit, and
// the table is exact only where *complete (all zeros and complete where a set is empty).
int refine_sets_vertex_counts(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                              uint64_t limit, uint64_t *answers, bool *complete, uint64_t *counts, std::string *err,
                              const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr, bool induced = false);

// The query edges as include/gnnpe_online.h numbers them: (a_k, b_k) with a_k < b_k, lexicographically ascending, each once.
std::vector<std::pair<uint32_t, uint32_t>> query_edges(const StaticGraph &query);

// E_m(C) of include/gnnpe_online.h: counts[k * data.offsets[data.n] + j] = the number of the maps refine_sets_count counts (same
// pairs, same induced) that send query edge k = (a_k, b_k) onto the adjacency entry j = (f(a_k) -> f(b_k)) of the data CSR; j is
// found by binary search in the row of f(a_k).  limit and *complete as in refine_sets_vertex_counts.  A query without an edge has
// no table: counts may then be null.
int refine_sets_edge_counts(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                            uint64_t limit, uint64_t *answers, bool *complete, uint64_t *counts, std::string *err,
                            const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr, bool induced = false);

// An undirected data edge {x, y} as one word: (min << 32) | max.
inline uint64_t delta_key(uint32_t x, uint32_t y) { return ((uint64_t)std::min(x, y) << 32) | std::max(x, y); }

// F of the delta calls as ascending keys, each edge once: delta_edges holds n_delta pairs (x, y), either orientation, repeats
// tolerated.  A loop or an id >= n returns <0 with *err; whether a pair is an edge of the graph is not looked at here.
int delta_edge_keys(uint32_t n, const uint32_t *delta_edges, uint64_t n_delta, std::vector<uint64_t> *keys, std::string *err);

// Delta_m(C, F, limit) of include/gnnpe_online.h: min(limit, the maps refine_sets_count counts (same pairs, same induced) that put
// at least one query edge on an edge of F), each once.  The backtracking of refine_sets_count, unchanged, with one test at every
// find: it walks all of M and shares nothing with the edge-anchored search of csrc/gnnpe_refine_delta.hip, whose yardstick it is.
// A pair that is no edge of the graph is refused (<0 with *err) by a binary search in the data row.
int refine_sets_delta_count(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                            const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint64_t *answers, std::string *err,
                            const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr, bool induced = false);

// VDelta_m(C, F) and EDelta_m(C, F) of include/gnnpe_online.h: the tables of refine_sets_vertex_counts / refine_sets_edge_counts
// over the maps refine_sets_delta_count counts only.  The same unchanged backtracking over all of M, the F test at every find, then
// the cell increments.  limit and *complete as in refine_sets_vertex_counts with Delta in the place of |M|; refusals as
// refine_sets_delta_count.  A query without an edge has no edge table: counts may then be null.
int refine_sets_delta_vertex_counts(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                                    const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint64_t *answers, bool *complete,
                                    uint64_t *counts, std::string *err,
                                    const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr, bool induced = false);
int refine_sets_delta_edge_counts(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                                  const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint64_t *answers, bool *complete,
                                  uint64_t *counts, std::string *err,
                                  const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr, bool induced = false);

}  // namespace gnnpe_host
