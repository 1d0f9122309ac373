// refine_sets.h -- the SET-RESTRICTED refinement on the host: the CPU yardstick of csrc/gnnpe_refine_sets.hip.
//
// R(C, limit) = min(limit, number of maps f from query vertices to data vertices that are injective, keep labels, have
// query degree <= data degree, map every query edge onto a data edge, and have f(u) in C(u) for EVERY query vertex u)
// (include/gnnpe_online.h).  host/refine.h restricts the start vertex only, as the reference does; where every C(u) is
// complete the two agree, and both equal the true embedding count.  Plain backtracking in the order of
// build_match_order (refine.h); the count does not depend on the order.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "graph_loader.h"

namespace gnnpe_host {

// bitmap: query.n rows of `words` = ceil(data.n / 32) uint32, bit v of row u set <=> v in C(u) (the layout
// gnnpe_filter_candidates writes).  Returns 0 and *answers, or <0 with *err (disconnected query graph).
// pairs (optional): only the maps with f(a) < f(b) for every pair (a, b) are counted -- with the pairs of query_symmetry.h this is
// D(C, limit), one embedding per distinct subgraph.
int refine_sets_count(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words,
                      uint64_t limit, uint64_t *answers, std::string *err,
                      const std::vector<std::pair<uint32_t, uint32_t>> *pairs = nullptr);

}  // namespace gnnpe_host
