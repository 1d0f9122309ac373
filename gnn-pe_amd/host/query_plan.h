// query_plan.h -- query side of the online FILTER, host C++17.
//
// Restates what the reference does to a query graph before it touches the index (GNN-PE/src/main.cpp:136-151):
//   dfs_query        custom.h:94-119   every simple 3-vertex path of the query graph, from every vertex in id
//                                      order, neighbours ascending, kept unless it or its reverse was kept before
//   gen_vde          custom.h:513-544  x, nx, vde of the query vertices (same arithmetic as the data side)
//   gen_query_pde    custom.h:574-631  per path: vids, labels, degrees, weight = sum of degrees, pde; paths sorted by
//                                      weight (descending, std::sort) and taken greedily while they still cover a new
//                                      vertex, until every query vertex is covered
// The result is the query plan: the only query-side input of the filter (gnnpe_filter_candidates).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "graph_loader.h"

namespace gnnpe_host {

struct QueryPlan {
    uint32_t n_vertices = 0, L = 3, e = 0;
    std::vector<uint32_t> vids, labels, degrees;  // n_paths x L
    std::vector<double> pde, pde_label;           // n_paths x e*L
    uint32_t n_paths() const { return L ? (uint32_t)(vids.size() / L) : 0; }
};

// gen_vde (custom.h:513-544) of the query vertices: x (n x e) from the label table, vde = x + the neighbours' x summed in
// adjacency order.  0 = ok; <0 with *err set
int query_vde(const StaticGraph &query, uint32_t e, std::vector<double> *x, std::vector<double> *vde, std::string *err);

// GNN-PGE query side (GNN-PGE/src/main.cpp:253-329): per query vertex u the per-dimension [lo, hi] of [vde[u], vde[w]]
// (path_group) and of [x[u], x[w]] (path_label_group) over its 1-hop paths (u, w); n x 4e doubles each, laid out
// (lo0, hi0, lo1, hi1, ...) like the data side (gnnpe_pge_groups).
struct PgeQueryGroups {
    uint32_t n_vertices = 0, e = 0;
    std::vector<uint32_t> labels, degrees;  // n
    std::vector<double> pg, plg;            // n x 4e
};

// 0 = ok; -3 = a query vertex without an edge (no group: the reference's leaf test would read an empty vector); -2 otherwise
int build_pge_query_groups(const StaticGraph &query, uint32_t e, PgeQueryGroups *out, std::string *err);

// 0 = ok; <0 with *err set
int build_query_plan(const StaticGraph &query, uint32_t e, QueryPlan *out, std::string *err);

// Exact mode: the plan of the orientation-complete filter, where a query vertex's candidate set holds every
// data vertex some embedding maps it to.  Three parts, taken in this order by the gen_query_pde rule (a path is taken while
// it covers a vertex not covered yet):
//   main    l = 2: the reference's plan (build_query_plan), unchanged.  l = 3: every simple 4-vertex query path (dfs_query
//           rule at depth 3), sorted by degree weight, descending, with std::stable_sort
//   tri     l = 3 only: for the vertices no 4-vertex path covers, paths of the reference's 3-vertex plan, in its order
//   single  the vertices still uncovered, width 1: label, degree and vde (in `pde`), tested vertex by vertex
// The plan lists each path in one orientation; the filter (gnnpe_filter_candidates_exact) adds the reverses.
struct ExactPlan {
    QueryPlan main, tri, single;
};
// l = 2 or 3.  0 = ok; <0 with *err set
int build_query_plan_exact(const StaticGraph &query, uint32_t e, uint32_t l, ExactPlan *out, std::string *err);

}  // namespace gnnpe_host
