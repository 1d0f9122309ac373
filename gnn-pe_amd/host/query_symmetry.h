// query_symmetry.h -- the symmetry of a query graph, as ordering constraints that leave one embedding per distinct subgraph.
//
// Aut(Q) = the permutations of the query vertices that keep labels and edges.  An embedding f and f o alpha, alpha in Aut(Q), have
// the same image subgraph, so a query reports every occurrence |Aut(Q)| times.  The Grochow-Kellis construction removes the
// repeats: walk the stabiliser chain in vertex-id order; for u = 0, 1, ... let O_u be the orbit of u under the automorphisms that
// fix 0 .. u-1 pointwise, and ask for f(u) < f(w) for every other w in O_u.  For any injective f exactly one of the maps
// {f o alpha} satisfies every pair, and |Aut(Q)| is the product of the |O_u| (orbit-stabiliser).
//
// The group is never listed: "is there an automorphism that fixes 0 .. u-1 and takes u to w" is one backtracking search with early
// exit per (u, w), over a query of a few dozen vertices.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "graph_loader.h"

namespace gnnpe_host {

struct QuerySymmetry {
    uint64_t n_automorphisms = 1;                     // saturated at 2^64 - 1
    std::vector<std::pair<uint32_t, uint32_t>> pairs;  // (a, b): require f(a) < f(b); by a, then b, ascending; a < b
};

QuerySymmetry query_symmetry(const StaticGraph &query);

}  // namespace gnnpe_host
