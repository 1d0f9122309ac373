// refine.h -- the REFINEMENT half of the reference's `-m online` (host C++17), so that the filter's candidate
// sets can be turned into the answer count without the reference binary.
//
// What the reference computes (GNN-PE/include/custom.h:634-932, QuickSI-style exploration): the number of
// embeddings f of the query graph into the data graph -- injective, label(f(u)) = label(u),
// degree(u) <= degree(f(u)), every query edge mapped onto a data edge -- whose image of the START vertex lies in
// that vertex' candidate set; the other query vertices are extended through the data graph's adjacency and are
// NOT checked against their candidate sets (generateValidCandidates, custom.h:755-797).  The start vertex is the
// query vertex with the fewest candidates, ties to the larger query degree, then to the smaller id
// (selectGQLStartVertex, custom.h:634-654).  Counting stops at the answer limit (-n, custom.h:842-846).
// The count does not depend on the matching order, so this is an independent backtracking search over the same
// definition, not a transcription of the reference's loop; tests pin it to the reference's answers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "graph_loader.h"

namespace gnnpe_host {

// The matching order both refinements (host below, device in csrc/gnnpe_refine.hip) walk: order[0] = the start vertex
// (custom.h:634-654), then always the unvisited vertex with the most visited neighbours; pivot[i] = one earlier
// neighbour of order[i] (extension goes through the data neighbours of its image), back = the other earlier
// neighbours (edge checks), flattened with back_off[i]..back_off[i+1].
struct MatchOrder {
    std::vector<uint32_t> order, pivot, back, back_off;
};
int build_match_order(const StaticGraph &query, const std::vector<uint64_t> &candidate_counts, MatchOrder *out, std::string *err);

// The same order anchored at a query edge: order[0] = a, order[1] = b with pivot a, then the rule above with its ties, pivots and
// back lists.  (a, b) must be an edge of the query; a disconnected query is refused.
int build_match_order_from_edge(const StaticGraph &query, uint32_t a, uint32_t b, MatchOrder *out, std::string *err);

// The same order anchored at a NON-ADJACENT pair of the query: order[0] = a, order[1] = b, then the rule above.  b is reached through
// no adjacency row, so position 1 has no pivot: pivot[1] = a stands for the anchor itself (a plan built from this order therefore
// counts the anchor neither as an edge to test nor as a non-edge to test).  The query is connected, so every position >= 2 has a
// pivot among the earlier positions, which may be position 1.  (a, b) must be different and not adjacent; a disconnected query is
// refused.
int build_match_order_from_pair(const StaticGraph &query, uint32_t a, uint32_t b, MatchOrder *out, std::string *err);

// The same order anchored at a query VERTEX: order[0] = u, then the rule above with its ties, pivots and back lists (a single-vertex
// query is that position alone).  u must be a vertex of the query; a disconnected query is refused.
int build_match_order_from_vertex(const StaticGraph &query, uint32_t u, MatchOrder *out, std::string *err);

// candidates[u] = ascending data vertex ids of query vertex u.  Returns 0 and *answers, or <0 with *err
// (disconnected query graph, size mismatch).
int refine_count(const StaticGraph &data, const StaticGraph &query, const std::vector<std::vector<uint32_t>> &candidates,
                 uint64_t limit, uint64_t *answers, std::string *err);

}  // namespace gnnpe_host
