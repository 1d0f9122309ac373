/* gnnpe_online.h -- C-ABI of libgnnpe_online.so: the REFINEMENT half of the reference's online step (custom.h:634-932).
 *
 * gnnpe_host_refine / gnnpe_refine restate the reference (start vertex only) and are frozen: built in round 1 so that
 * `gnnpe_main -m online` can print the reference's answer line.  gnnpe_host_refine_sets / gnnpe_refine_sets (below) restrict
 * every query vertex to its set, for exact mode; the _distinct forms (ABI version 11) count and list every matching subgraph
 * once; the _mode forms (ABI version 12) add induced matching.  The library is kept out of libgnnpe_hip.so since round 6:
 * the offline hot path and its (f) rows link and load without it.  libgnnpe_online.so links against libgnnpe_hip.so (contexts, error text); `gnnpe_main` dlopen()s it for -m online
 * only.  Same conventions as gnnpe_hip.h: 0 = GNNPE_OK, gnnpe_last_error() for the text.
 */
#ifndef GNNPE_ONLINE_H
#define GNNPE_ONLINE_H

#include "gnnpe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Refinement half of the reference's online step (custom.h:634-932), host side: the number of embeddings of the
 * query graph in the data graph (injective, labels equal, query degree <= data degree, query edges on data edges)
 * whose START vertex -- fewest candidates, ties to the larger degree, then the smaller id (custom.h:634-654) -- maps
 * into its candidate set, counted up to `limit` (the reference's -n).  candidate_bitmap as written by
 * gnnpe_filter_candidates. */
int gnnpe_host_refine(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                      const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint64_t *answers);

/* The same count on the device: one thread per (start candidate, neighbour slot of its image), depth-first below that.
 * Needs the whole graph on the device (gnnpe_load_csr); query graphs of up to 32 vertices.  device_ms may be NULL. */
int gnnpe_refine(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                 uint64_t *answers, double *device_ms);

/* ---- ABI version 9: the set-restricted refinement ------------------------------------------------------------------
 * R(C, limit) = min(limit, number of maps f from query vertices to data vertices that are injective, keep labels, have
 * query degree <= data degree, map every query edge onto a data edge, AND have f(u) in C(u) for EVERY query vertex u),
 * with C the bitmap layout of gnnpe_filter_candidates (n_query_vertices x ceil(n / 32) uint32).
 *   - If every C(u) is complete -- exact-mode filter output (gnnpe_filter_candidates_exact), or a label/degree-only
 *     bitmap -- R(C, limit) equals what the two functions above return on the same bitmap, and equals the true count.
 *   - For arbitrary C it is the count of the embeddings that lie inside the sets.
 * The reference-mode filter's sets are NOT complete: there the functions above (start vertex only) give the reference's
 * answer and these give a smaller one.  The count does not depend on the matching order. */

/* Host form: plain backtracking that applies the set test at every level.  Arguments as gnnpe_host_refine.  It has no
 * limit on the query's size: a connected query of 33 or more vertices, which the device form refuses, is counted here. */
int gnnpe_host_refine_sets(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                           const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint64_t *answers);

/* Device form: one wave per search subtree, the whole wave on every adjacency row (csrc/gnnpe_refine_sets.hip).
 * Requirements as gnnpe_refine: whole simple graph on the device, connected query graph of up to 32 vertices; a context
 * in the multigraph state is refused.  *answers is clamped to limit; a count far above the limit costs no more time than
 * the limit does.  matches may be NULL; otherwise it is a host array of matches_cap x n_query_vertices uint32, and on
 * return its first min(*answers, matches_cap) rows are pairwise different embeddings, row k column u = f_k(u) (column =
 * query vertex id as in the query file).  Which embeddings are kept when there are more than matches_cap, and their
 * order, are unspecified; matches_cap > limit is treated as limit.  device_ms (may be NULL) covers the kernels, not the
 * uploads of the bitmap and the start candidates, as gnnpe_refine's does. */
int gnnpe_refine_sets(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                      uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms);

/* ---- ABI version 10: paged match enumeration -----------------------------------------------------------------------
 * A cursor over the embeddings gnnpe_refine_sets counts: every call of next delivers the next page of at most page_rows
 * embeddings, and across the pages every embedding inside the sets comes out exactly once, up to `limit`, whatever the
 * page size (csrc/gnnpe_refine_pages.hip: a wave that finds the page full stores its search state and the next launch
 * carries on from it; nothing is walked or counted twice).
 *
 * open: requirements and refusals as gnnpe_refine_sets -- the whole simple graph on the device, a connected query graph
 *   of 1..32 vertices, no multigraph state; page_rows == 0 is refused.  The cursor OWNS its device memory (its copy of
 *   the bitmap, start candidates, item offsets, counters, suspend slots, one page of min(page_rows, limit) rows), so
 *   two cursors may be open on one context with their pages interleaved, and gnnpe_refine_sets and the filters may run
 *   between two pages.  candidate_bitmap may be freed once open returns.
 * next: fills the device page and, unless host_rows (page_rows x n_query_vertices uint32) is NULL, copies its *n_rows
 *   rows there; row k column u = f_k(u), column = query vertex id as in the query file.  Every page except the last
 *   holds exactly page_rows rows.  *done = 1 with the last page; a page of 0 rows comes only together with *done = 1
 *   (limit == 0, an empty set, no embedding, or a count that is a multiple of page_rows).  After *done a call returns
 *   0 rows and *done = 1 and launches nothing.  The rows of all pages together are pairwise different embeddings
 *   inside the sets, min(R(C, 2^64 - 1), limit) of them; their order, and which embeddings come out when `limit`
 *   cuts, are unspecified.  device_ms (may be NULL) is the page's kernel time.  The small counter block comes back
 *   once per page, as in gnnpe_refine_sets.
 * device_ptr: the device page the last next filled (its first *n_rows rows), valid until the next call of next or
 *   close: the path for consumers on the device, who pass host_rows == NULL.
 * info: {pages delivered (launches), rows delivered, waves suspended at the end of the last page, first-level items not
 *   yet taken, suspend slots (resident waves)}.  After *done the third and fourth are 0.
 * Lifetime: loading or changing the context's rows (gnnpe_load_csr, gnnpe_load_rows, gnnpe_set_multigraph_rows,
 *   gnnpe_rows_append, gnnpe_rows_drop_halo) invalidates the open cursors: their next call of next returns GNNPE_ERR_ARG
 *   with a message and launches nothing; close still works.  Cursors MUST be closed before gnnpe_destroy.  close(NULL)
 *   does nothing. */
typedef struct gnnpe_match_cursor gnnpe_match_cursor;
int gnnpe_refine_pages_open(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                            uint64_t page_rows, gnnpe_match_cursor **cursor);
int gnnpe_refine_pages_next(gnnpe_match_cursor *cursor, uint32_t *host_rows, uint64_t *n_rows, int *done, double *device_ms);
int gnnpe_refine_pages_device_ptr(gnnpe_match_cursor *cursor, void **dev_rows, uint32_t *n_query_vertices);
int gnnpe_refine_pages_info(gnnpe_match_cursor *cursor, uint64_t info[5]);
void gnnpe_refine_pages_close(gnnpe_match_cursor *cursor);

/* ---- ABI version 11: one embedding per distinct subgraph ---------------------------------------------------------------
 * R counts EMBEDDINGS, so a query with symmetry reports every occurrence of the pattern |Aut(Q)| times (a triangle six
 * times, K4 24 times), Aut(Q) being the permutations of the query vertices that keep labels and edges.  The functions
 * below break the symmetry inside the search instead of leaving the duplicates to the caller.
 *
 * gnnpe_host_query_symmetry: |Aut(Q)| (saturated at 2^64 - 1) and the ordering pairs of the Grochow-Kellis construction:
 *   walk the stabiliser chain in query-vertex id order; for u = 0, 1, ... with O_u the orbit of u under the automorphisms
 *   that fix 0 .. u-1 pointwise, the pair (u, w) for every other w in O_u, ascending.  A pair (a, b) means "require
 *   f(a) < f(b)".  For any injective f exactly one of the maps {f o alpha : alpha in Aut(Q)} satisfies every pair, and
 *   |Aut(Q)| is the product of the |O_u|.  At most nq (nq - 1) / 2 pairs; pairs is pairs_cap x 2 uint32 and may be NULL
 *   with pairs_cap == 0; *n_pairs is the number of pairs, and with pairs_cap below it the call returns GNNPE_ERR_ARG
 *   (|Aut| and *n_pairs are still set).  No limit on the query's size; loader errors as from gnnpe_host_refine_sets.
 *
 * D(C, limit) = min(limit, number of maps counted by R(C, .) that also satisfy f(a) < f(b) for every such pair).
 *   - If C is closed under the query's automorphisms -- exact-mode filter output, label/degree bitmaps, all-ones bitmaps
 *     are -- the maps D counts are exactly one embedding per distinct image subgraph (the set of data edges the query
 *     edges land on), and D(C, 2^64 - 1) * |Aut(Q)| = R(C, 2^64 - 1).
 *   - For arbitrary C, D is the constrained count, nothing more: an occurrence whose one representative lies outside
 *     the sets is not counted although another of its embeddings lies inside.
 * A query without symmetry has no pairs: D = R, and the device forms run the kernels of the plain functions.
 *
 * gnnpe_host_refine_sets_distinct, gnnpe_refine_sets_distinct, gnnpe_refine_pages_open_distinct: arguments, requirements
 * and refusals of gnnpe_host_refine_sets, gnnpe_refine_sets and gnnpe_refine_pages_open, with D in the place of R; the
 * rows are the maps D counts.  On the device the compares run inside the search (an image outside its bounds is never
 * descended into, and a long adjacency row is cut to its bounds by a search before it is walked), so the symmetric part
 * of the search tree is not visited.  next, device_ptr, info and close serve both kinds of cursor. */
int gnnpe_host_query_symmetry(const char *query_graph_path, uint64_t *n_automorphisms, uint32_t *pairs, uint32_t pairs_cap,
                              uint32_t *n_pairs);
int gnnpe_host_refine_sets_distinct(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                    const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                                    uint64_t *answers);
int gnnpe_refine_sets_distinct(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                               uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms);
int gnnpe_refine_pages_open_distinct(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                     uint64_t limit, uint64_t page_rows, gnnpe_match_cursor **cursor);

/* ---- ABI version 12: induced matching ---------------------------------------------------------------------------------
 * R and D count MONOMORPHISMS: query edges land on data edges and nothing is asked of query non-edges.  Induced
 * (vertex-induced) matching -- "subgraph isomorphism" in VF2's sense, the notion of motif and graphlet counting -- also
 * sends every two non-adjacent query vertices to two non-adjacent data vertices.
 *
 * I(C, limit) = min(limit, number of maps counted by R(C, .) that also send every pair of distinct, non-adjacent query
 *   vertices to non-adjacent data vertices).  ID(C, limit) is the same with D in the place of R: the ordering pairs of
 *   gnnpe_host_query_symmetry also hold.
 *   - The degree test (query degree <= data degree) stays.
 *   - Automorphisms keep non-edges: for C closed under them ID counts one map per distinct induced occurrence, and
 *     ID(C, 2^64 - 1) * |Aut(Q)| = I(C, 2^64 - 1).  For arbitrary C both are the constrained counts, nothing more.
 *   - A query with no non-adjacent pair (1 or 2 vertices, K_n) has I = R and ID = D, and the device forms run the kernels
 *     of the functions above.
 *
 * The three functions below take a mode word: 0 is R, GNNPE_MATCH_DISTINCT is D, GNNPE_MATCH_INDUCED is I, both bits are
 * ID; any other bit returns GNNPE_ERR_ARG.  Arguments, requirements, refusals, row layout and cursor lifetime are those of
 * gnnpe_host_refine_sets, gnnpe_refine_sets and gnnpe_refine_pages_open, which are their mode-0 cases as the _distinct
 * functions are their GNNPE_MATCH_DISTINCT cases; the rows are the maps the mode counts.  On the device the non-edge test
 * runs inside the search, after the back-edge test and by the same binary search in the shorter of the two rows: an image
 * adjacent to an earlier image it must not be adjacent to is never descended into.  next, device_ptr, info and close
 * serve every kind of cursor. */
#define GNNPE_MATCH_DISTINCT 1u
#define GNNPE_MATCH_INDUCED 2u
int gnnpe_host_refine_sets_mode(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit, uint32_t mode,
                                uint64_t *answers);
int gnnpe_refine_sets_mode(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                           uint32_t mode, uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms);
int gnnpe_refine_pages_open_mode(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                 uint64_t limit, uint64_t page_rows, uint32_t mode, gnnpe_match_cursor **cursor);

/* ---- ABI version 13: per-vertex match counts ---------------------------------------------------------------------------
 * What a motif or graphlet counter asks of the matches is rarely the rows: it is how many matches every data vertex takes
 * part in, and in which role -- graphlet degree vectors, local triangle and clique counts, per-vertex motif features.  The
 * search visits every match anyway; the two functions below build that table inside it and write no rows.
 *
 * For a mode word m (0, GNNPE_MATCH_DISTINCT, GNNPE_MATCH_INDUCED, or both) let M_m(C) be the set of maps that
 * gnnpe_refine_sets_mode counts with limit 2^64 - 1.
 *
 *   V_m(C)[u][v] = |{ f in M_m(C) : f(u) = v }|     u < nq, v < n, uint64, row-major nq x n
 *
 * u is the query vertex id as in the query file (nq is the file's vertex count).  Every row of the table sums to |M_m(C)|.
 * v can be the image of u in some match iff V[u][v] > 0: the rows' supports are the exact candidate sets.
 *
 * Reading the table.  For C closed under Aut(Q) (exact-mode filter output, label/degree bitmaps, all-ones bitmaps), with
 * O(u) the orbit of u under the FULL automorphism group:
 *   - modes 0 and INDUCED: V[u][v] * |O(u)| / |Aut(Q)| is the number of distinct occurrences in which v plays a role of
 *     u's orbit (a triangle: V[u][v] / 2 triangles at v; a wedge: V[centre][v] / 2 wedges centred at v, V[end][v] wedges
 *     ending at v).
 *   - the DISTINCT modes: the same number is the sum of V[u'][v] over u' in O(u).  A single column of a symmetric query
 *     splits by the ordering pairs (the smallest image of a triangle always sits at vertex 0) and means nothing on its own.
 *   - for arbitrary C the table holds the constrained counts, nothing more.
 *
 * limit is a GUARD, not a cut: the table is exact only if the whole search ran.
 *   - *answers = min(|M|, limit), as for every other call.
 *   - *complete = 1 iff |M| < limit; limit = 2^64 - 1 always completes.
 *   - with *complete = 0 the table's contents are unspecified (and the device form copies nothing to host_counts).
 *   - with limit 0 the call launches nothing and returns *complete = 0.
 *   - if some C(u) is empty, or there are no start candidates, the table is all zeros and *complete = 1.
 *
 * gnnpe_host_refine_sets_vertex_counts: the host form, the backtracking of gnnpe_host_refine_sets_mode adding 1 to the nq
 *   cells of every find.  counts is nq x n uint64 of the caller's.  No limit on the query's size.  Unknown mode bits and a
 *   disconnected query return GNNPE_ERR_ARG.
 * gnnpe_refine_sets_vertex_counts: the device form (csrc/gnnpe_refine_vcount.hip).  Requirements and refusals are exactly
 *   those of gnnpe_refine_sets_mode: the whole simple graph on the device, a connected query graph of 1..32 vertices, no
 *   multigraph state, unknown mode bits GNNPE_ERR_ARG.
 *   - The search is gnnpe_refine_sets_mode's.  Every wave tallies its finds per depth and adds a tally to the table when it
 *     leaves the image it belongs to: one 64-bit atomic add per find (the last position) and one per visited image with at
 *     least one find below it, not nq per find.
 *   - host_counts (nq x n uint64) may be NULL: then nothing but the 16-byte counter block comes back to the host.
 *   - *dev_counts (dev_counts may be NULL) is the table on the device: a context-owned, grow-only buffer of nq * n * 8
 *     bytes, valid until the next call of this function on the context or until the context's rows are loaded or changed.
 *     An allocation the device refuses returns its error and leaves the context usable.
 *   - *device_ms (may be NULL) covers the zeroing of the table and the kernel. */
int gnnpe_host_refine_sets_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                         const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                                         uint32_t mode, uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_refine_sets_vertex_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                    uint64_t limit, uint32_t mode, uint64_t *answers, int *complete, uint64_t *host_counts,
                                    void **dev_counts, double *device_ms);

/* ---- ABI version 14: per-edge match counts -----------------------------------------------------------------------------
 * The other half of what motif and graphlet consumers ask for is per EDGE: the triangle support of every edge (the input of a
 * k-truss decomposition), edge-orbit graphlet degree vectors, per-edge motif features.  None of it follows from V_m(C): two
 * vertices can each sit in many matches without sharing one.  The functions below build the table inside the search.
 *
 * Query edges.  The edges of the loaded simple query graph are written (a_k, b_k) with a_k < b_k and sorted lexicographically,
 * k = 0 .. nqe - 1.  gnnpe_host_query_edges hands that list out (edges: cap x 2 uint32; conventions as
 * gnnpe_host_query_symmetry: *n_edges is always set, and a cap below it returns GNNPE_ERR_ARG).
 *
 * Data entries.  j is an index into the CSR the caller handed over: offsets / nbrs of the host form, the arrays of
 * gnnpe_load_csr for the device form -- the context keeps them entry for entry (row x starts at offsets[x], nbrs is copied as
 * it is).  Entry j in row x with nbrs[j] = y is the directed entry x -> y.  The graph is undirected: y -> x is an entry too.
 *
 *   E_m(C)[k][j] = |{ f in M_m(C) : f(a_k) = x and f(b_k) = y }|   for j = (x -> y), uint64, row-major nqe x offsets[n]
 *
 * with M_m(C) as in the ABI 13 text.  Every row sums to |M_m(C)|.  Summing row k over the entries of data row x gives
 * V[a_k][x]; summing row k over the entries with nbrs[j] = y gives V[b_k][y].
 *
 * Reading the table.
 *   - the undirected support of {x, y} under query edge k is E[k][x->y] + E[k][y->x].
 *   - triangle, mode 0: every E[k][x->y] is the number of triangles on {x, y} -- the truss support.
 *   - wedge 0 - 1 - 2, mode 0: E[0][x->y] = deg(y) - 1 and E[1][x->y] = deg(x) - 1.
 *   - for C closed under Aut(Q), in the DISTINCT modes a single row of a symmetric query splits by the ordering pairs, and
 *     so does a single direction of it (the smaller image of a triangle's edge 0 always sits at vertex 0).  A row and a
 *     direction mean nothing on their own there: what means something is the sum over the rows of the edge's orbit under
 *     Aut(Q), and over both directions -- the number of distinct occurrences in which {x, y} plays a role of that orbit.
 *   - for arbitrary C the table holds the constrained counts, nothing more.
 *
 * limit and *complete are exactly those of gnnpe_refine_sets_vertex_counts: limit is a guard, *answers = min(|M|, limit),
 * *complete = 1 iff |M| < limit; with *complete = 0 the table is unspecified and nothing is copied to the host; with limit 0
 * nothing is launched; an empty set gives a zero table and *complete = 1.
 * A single-vertex query has nqe = 0: the call succeeds with an empty table (counts / host_counts are not touched and may be
 * NULL, *dev_counts = NULL, nothing is allocated) and the usual *answers and *complete.
 *
 * gnnpe_host_refine_sets_edge_counts: the host form, the backtracking of gnnpe_host_refine_sets_mode adding 1 to the nqe cells
 *   of every find; the entry is found by binary search in the data row.  No limit on the query's size.  Unknown mode bits and a
 *   disconnected query return GNNPE_ERR_ARG.
 * gnnpe_refine_sets_edge_counts: the device form (csrc/gnnpe_refine_ecount.hip).  Requirements and refusals are exactly those
 *   of gnnpe_refine_sets_mode.
 *   - Every wave tallies its finds per depth, remembers the entry it stands on per depth, and adds a tally to the entries of a
 *     position's query edges when it leaves the image: deg_Q(last position) atomic adds per find, and for every visited image
 *     with a find below it one per query edge to its earlier positions.
 *   - host_counts (nqe x offsets[n] uint64) may be NULL.
 *   - *dev_counts (dev_counts may be NULL) is the table on the device: a context-owned, grow-only buffer of its own, valid
 *     until the next call of THIS function on the context or until the context's rows are loaded or changed; a
 *     gnnpe_refine_sets_vertex_counts call in between does not disturb it.  An allocation the device refuses returns its
 *     error and leaves the context usable.
 *   - *device_ms (may be NULL) covers the zeroing of the table and the kernel. */
int gnnpe_host_query_edges(const char *query_graph_path, uint32_t *edges, uint32_t cap, uint32_t *n_edges);
int gnnpe_host_refine_sets_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                       const char *query_graph_path, const uint32_t *candidate_bitmap, uint64_t limit,
                                       uint32_t mode, uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_refine_sets_edge_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                  uint64_t limit, uint32_t mode, uint64_t *answers, int *complete, uint64_t *host_counts,
                                  void **dev_counts, double *device_ms);

/* ---- ABI version 15: the matches through a given set of data edges, each once ----------------------------------------------
 * "Which matches use one of these data edges?" is the primitive of incremental (continuous) subgraph matching:
 *   - edges were added to G: load the new graph (gnnpe_csr_apply_edges of include/gnnpe_hip.h changes the resident one in place)
 *     and ask for the matches through the added edges -- exactly the new matches;
 *   - edges are about to be removed: ask on the current graph for the matches through them -- exactly the ones that vanish.
 * Re-running the query pays for |M| where it needs the difference; pinning endpoints through the bitmap takes 2 nqe calls per
 * edge and reports a match through several of the edges several times; E_m(C) has the counts per edge, which do not add up to a
 * count for a SET of edges, and no rows.
 *
 * M_m(C) is as in the ABI 13 text, the query edges (a_k, b_k), k = 0 .. nqe - 1, as gnnpe_host_query_edges numbers them.
 * F is a set of undirected data edges, handed over as delta_edges: n_delta x 2 uint32 pairs (x, y), either orientation; repeats
 * and both orientations of one edge are tolerated and mean the edge once.
 *
 *   Delta_m(C, F, limit) = min(limit, |{ f in M_m(C) : {f(a_k), f(b_k)} in F for at least one k }|)
 *
 * Every such map is counted and listed ONCE, however many of its query edges land in F.
 *   - modes 0 and DISTINCT, G' = G plus F with F disjoint from E(G), the same C: |M(G')| = |M(G)| + Delta(G', F).  The degree
 *     test does not disturb this: a match that avoids F already has deg_Q(u) distinct neighbours of f(u) in G.
 *   - the INDUCED modes: Delta is still exactly "the matches on the loaded graph that touch F", but adding an edge can also
 *     DESTROY induced matches, and those are not Delta of the new graph.  They are N of the old graph: ABI 18, below.
 *   - F = E(G) and nq >= 2: Delta = |M|.
 *   - F = {{x, y}}: Delta = the sum over k of E[k][x->y] + E[k][y->x].
 *   - a single-vertex query has no edge: Delta = 0.  n_delta == 0: Delta = 0.  Nothing is launched in either case.
 *
 * Refusals, all GNNPE_ERR_ARG with *answers = 0:
 *   - x == y, or an id >= n: checked on the host before anything is launched.
 *   - a pair that is not an edge of the graph.  The device form finds it on the device and reports it with the counter block, in
 *     the call's single wait; the context stays usable afterwards.  (Where nothing is launched -- limit 0, an empty set, a
 *     single-vertex query -- the device form does not look the pairs up.)
 *   - everything else exactly as gnnpe_refine_sets_mode: the whole simple graph on the device, a connected query of 1..32
 *     vertices, no multigraph state, no unknown mode bits.
 *
 * gnnpe_host_refine_sets_delta: the host form.  The backtracking of gnnpe_host_refine_sets_mode, unchanged, with one test at
 *   every find (is a query edge's image in F: a binary search among the sorted keys (min << 32) | max).  It walks all of M, not
 *   only Delta: it is the yardstick and shares nothing with the device form's search.
 * gnnpe_refine_sets_delta: the device form (csrc/gnnpe_refine_delta.hip): one launch per query edge k over one item per directed
 *   entry of F, in a matching order that starts at (a_k, b_k); a map is kept in the launch of its lowest-numbered query edge
 *   in F only.  Its cost follows Delta and nqe, not |M|.
 *   - matches, matches_cap and the row layout are as gnnpe_refine_sets_mode: the first min(*answers, matches_cap) rows are
 *     pairwise different maps of the set above.  Which maps come out when limit or the cap cuts, and their order, are
 *     unspecified.
 *   - *device_ms (may be NULL) covers the kernels, not the uploads.
 *   - the buffers are context-owned and grow-only; an allocation the device refuses returns its error and leaves the context
 *     usable.
 *   - the rows come page by page through gnnpe_refine_pages_open_delta (the last section). */
int gnnpe_host_refine_sets_delta(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                 const char *query_graph_path, const uint32_t *candidate_bitmap,
                                 const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                 uint64_t *answers);
int gnnpe_refine_sets_delta(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                            const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                            uint64_t *answers, uint32_t *matches, uint64_t matches_cap, double *device_ms);

/* ---- ABI version 17: count tables of the matches through a set of data edges ----------------------------------------------
 * The consumers of the ABI 13 and 14 tables -- graphlet degree vectors, local triangle and clique counts, the truss support of
 * every edge -- do not want the rows of gnnpe_refine_sets_delta after a batch of edge changes.  They want their table brought up
 * to date.  Re-running the whole count pays for |M|; tallying the delta rows on the host moves Delta * nq * 4 bytes and cannot be
 * done at all where Delta is 10^9.  The functions below build the TABLES of the matches through F inside the edge-anchored search,
 * and can add them to, or subtract them from, a table the caller keeps on the device:
 *     T -= tables of Delta(G, D);  gnnpe_csr_apply_edges(ctx, I, D);  T += tables of Delta(G', I).
 * Nothing per match leaves the device.
 *
 * M_m(C), the query edges (a_k, b_k), the entry index j, F and its hand-over as delta_edges are as in the ABI 13, 14 and 15 texts.
 * Let Dset_m(C, F) = { f in M_m(C) : {f(a_k), f(b_k)} in F for at least one k }.
 *
 *   VD_m(C, F)[u][v] = |{ f in Dset : f(u) = v }|                      nq  x n           uint64, row-major
 *   ED_m(C, F)[k][j] = |{ f in Dset : f(a_k) = x and f(b_k) = y }|     nqe x offsets[n]  uint64, j = (x -> y)
 *
 *   - every row of either table sums to |Dset| = Delta_m(C, F, 2^64 - 1).
 *   - summing ED row k over the entries of data row x gives VD[a_k][x].
 *   - F = E(G) and nq >= 2: VD = V_m(C) and ED = E_m(C).
 *   - INSERTION IDENTITY, modes 0 and DISTINCT.  G' = G + F with F disjoint from E(G), the same C: as sets of maps
 *     M(G') = M(G) + Dset(G', F), disjoint.  Hence V(G') = V(G) + VD(G', F), and E(G') = E(G) + ED(G', F) compared by the key
 *     (x, y) of an entry -- the entry indices of G and G' differ (gnnpe_csr_apply_edges_map of include/gnnpe_hip.h hands out the
 *     map between them and gnnpe_csr_carry_entries moves a device table through it); an entry of F has E(G) = 0.
 *   - DELETION IDENTITY, the same modes.  V(G - D) = V(G) - VD(G, D), and the same for E by keys.
 *   - the INDUCED modes: the tables are "the matches on the loaded graph that touch F", nothing more (the caveat of ABI 15; ABI 18
 *     has the count of the other half and ABI 19 its tables, and with both an induced table is maintained exactly).
 *   - a single-vertex query has Delta = 0: the V table is all zeros, the E table is empty as in ABI 14.
 *   - n_delta == 0: the tables are all zeros.
 *
 * limit is a GUARD exactly as in ABI 13 and 14, with Delta in the place of |M|: *answers = min(Delta, limit); *complete = 1 iff
 * Delta < limit; with *complete = 0 the table is unspecified and nothing is copied to the host; limit == 0 launches nothing and
 * gives *complete = 0; an empty C(u), no F or a single-vertex query launches nothing and gives a zero table and *complete = 1.
 *
 * gnnpe_host_refine_sets_delta_vertex_counts, gnnpe_host_refine_sets_delta_edge_counts: the host forms, the yardstick.  The unchanged
 *   backtracking of gnnpe_host_refine_sets_mode over all of M; at every find the F test of gnnpe_host_refine_sets_delta, then the
 *   cell increments of gnnpe_host_refine_sets_vertex_counts / _edge_counts.  They share nothing with the device search.  Refusals
 *   are those of gnnpe_host_refine_sets_delta.  counts is the caller's (nq x n, nqe x offsets[n]; NULL is accepted for an empty
 *   edge table).
 * gnnpe_refine_sets_delta_vertex_counts, gnnpe_refine_sets_delta_edge_counts: the device forms (csrc/gnnpe_refine_delta_counts.hip):
 *   the launches, items and charging rule of gnnpe_refine_sets_delta with the tallies and flushes of the ABI 13 / 14 kernels.
 *   Requirements and refusals are exactly those of gnnpe_refine_sets_delta: a loop or an id >= n is refused on the host, a pair
 *   that is no edge is found on the device and reported after the call's single wait, the context stays usable, and *answers is
 *   0 on every refusal.
 *   - dev_accum == NULL: sign must be 1 (else GNNPE_ERR_ARG).  The table lives in a context-owned, grow-only buffer of its own --
 *     one for VD, another for ED, neither of them the buffers of ABI 13 and 14, whose device views are not disturbed -- and is
 *     zeroed once per call, before the first launch.  It is valid until the next call of the same function on the context or
 *     until the context's rows are loaded or changed (gnnpe_csr_apply_edges changes them).  host_counts and *dev_counts are as
 *     in ABI 13 and 14.
 *   - dev_accum != NULL: caller-owned device memory of the table's size on the context's device (gnnpe_dev_alloc, a torch
 *     tensor).  sign is +1 or -1; host_counts must be NULL (else GNNPE_ERR_ARG); *dev_counts = dev_accum.  Nothing is zeroed:
 *     every cell ends at old + sign * c mod 2^64, c the cell of the table above.  All work is on the context's stream.
 *       . A refused call leaves the caller's table untouched, byte for byte: the pairs are looked up before the first search
 *         launch starts, and a search wave that finds the error flag set leaves before its first item.
 *       . With *complete = 0 the caller's table is unspecified: pass limit = 2^64 - 1 when accumulating.
 *       . Where nothing is launched the table is untouched.
 *   - *device_ms (may be NULL) covers the zeroing of a context-owned table and the kernels, not the uploads. */
int gnnpe_host_refine_sets_delta_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                               const char *query_graph_path, const uint32_t *candidate_bitmap,
                                               const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                               uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_host_refine_sets_delta_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                             const char *query_graph_path, const uint32_t *candidate_bitmap,
                                             const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                             uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_refine_sets_delta_vertex_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                          const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                          uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                          void *dev_accum, int sign, double *device_ms);
int gnnpe_refine_sets_delta_edge_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                        const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint32_t mode,
                                        uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                        void *dev_accum, int sign, double *device_ms);

/* ---- ABI version 18: the induced matches an edge change destroys or creates ------------------------------------------------------
 * Under the INDUCED modes an edge change works both ways: a new edge creates the matches through it (Delta of ABI 15, asked after
 * the insertion) and DESTROYS every match that had a non-adjacent query pair on its two ends; a removed edge destroys the matches
 * through it and CREATES those.  The functions below are the mirror image of ABI 15: the matches that put a non-adjacent query pair
 * on one of a given set of data vertex pairs -- asked before an insertion the matches it destroys, asked after a deletion the ones
 * it created.  With them a caller keeps an induced count (a motif or graphlet count) current without re-running it.
 *
 * Terms as in the ABI 12 - 15 texts, M_m(C) as in ABI 13.  The non-adjacent pairs of the loaded simple query graph are written
 * (a_k, b_k) with a_k < b_k and sorted lexicographically, k = 0 .. nqn - 1.  gnnpe_host_query_nonedges hands that list out (pairs:
 * cap x 2 uint32; conventions exactly as gnnpe_host_query_edges: *n_pairs is always set, and a cap below it returns GNNPE_ERR_ARG).
 * F is a set of unordered data vertex pairs that are NOT edges of the loaded graph, handed over as pairs: n_pairs x 2 uint32
 * (x, y), either orientation; repeats and both orientations of one pair are tolerated and mean the pair once.
 *
 *   N_m(C, F, limit) = min(limit, |{ f in M_m(C) : {f(a_k), f(b_k)} in F for at least one k }|)     m contains GNNPE_MATCH_INDUCED
 *
 * Every such map is counted and listed ONCE, however many of its non-adjacent pairs land in F.  Write Nset_m(C, F) for the set of
 * these maps and Dset_m(C, F) for the set of ABI 17.  The identities below hold for the INDUCED modes with the same C on both
 * graphs (a label bitmap, for instance; a degree bitmap differs between the two):
 *   - INSERTION.  G' = G + F with F disjoint from E(G).  As sets of maps M(G') = (M(G) - Nset(G, F)) + Dset(G', F), the union
 *     disjoint and Nset(G, F) inside M(G): |M(G')| = |M(G)| - N(G, F) + Delta(G', F).
 *   - DELETION.  G' = G - D with D inside E(G).  M(G') = (M(G) - Dset(G, D)) + Nset(G', D): |M(G')| = |M(G)| - Delta(G, D) + N(G', D).
 *   - MIXED BATCH, exact in two steps: first delete D (Delta on the graph before, gnnpe_csr_apply_edges, N on the graph after), then
 *     insert I (N on the graph before, gnnpe_csr_apply_edges, Delta on the graph after).  One step with both lists is not exact: a
 *     map can lose one pair to D and gain another from I.
 *   - F = all non-edges of G and a query with a non-adjacent pair: N = |M_m(C)|.
 *   - a query without a non-adjacent pair (1 or 2 vertices, K_n), or n_pairs == 0: N = 0, and nothing is launched.
 *   (The degree test does not disturb the identities for the reason given in ABI 15, and the ordering pairs do not depend on the
 *   graph.)
 *
 * Refusals, all GNNPE_ERR_ARG with *answers = 0:
 *   - a mode without GNNPE_MATCH_INDUCED, or with unknown bits.
 *   - x == y, or an id >= n: checked on the host before anything is launched.
 *   - a pair that IS an edge of the graph.  The device form finds it on the device and reports it with the counter block, in the
 *     call's single wait; the context stays usable afterwards.  (Where nothing is launched the device form does not look the pairs
 *     up.)
 *   - everything else exactly as gnnpe_refine_sets_mode.
 *
 * gnnpe_host_refine_sets_delta_nonedges: the host form, the yardstick.  The unchanged backtracking of gnnpe_host_refine_sets_mode
 *   over all of M with one test at every find (is the image of some non-adjacent query pair among the sorted keys of F); F's pairs
 *   are checked to be non-edges up front.  It shares nothing with the device search.
 * gnnpe_refine_sets_delta_nonedges: the device form (csrc/gnnpe_refine_delta_nonedges.hip): one launch per non-adjacent query pair k
 *   over one item per directed pair of F, in a matching order that starts at (a_k, b_k) and walks from the third position on; a map
 *   is kept in the launch of its lowest-numbered non-adjacent pair in F only.  Its cost follows N and nqn,
 *   not |M|.  matches, matches_cap, the row layout, *device_ms and the ownership of the buffers are exactly those of
 *   gnnpe_refine_sets_delta; the rows come page by page through gnnpe_refine_pages_open_delta_nonedges (the last section), and the
 *   count tables of Nset are ABI 19, below. */
int gnnpe_host_query_nonedges(const char *query_graph_path, uint32_t *pairs, uint32_t cap, uint32_t *n_pairs);
int gnnpe_host_refine_sets_delta_nonedges(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                          const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *pairs,
                                          uint64_t n_pairs, uint64_t limit, uint32_t mode, uint64_t *answers);
int gnnpe_refine_sets_delta_nonedges(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                     const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode, uint64_t *answers,
                                     uint32_t *matches, uint64_t matches_cap, double *device_ms);

/* ---- ABI version 19: count tables of the induced matches on a set of non-edges -----------------------------------------------------
 * The consumers of the count tables -- graphlet degree vectors, local motif counts, edge-orbit counts -- are the INDUCED consumers,
 * and under the induced modes the tables of ABI 17 are one half of what an edge change does to a table (its caveat).  The functions
 * below build the other half, the TABLES of Nset_m(C, F) of ABI 18, with the accumulate and sign conventions of ABI 17, so that
 *     insertion of F:  T -= tables of Nset(G, F);  gnnpe_csr_apply_edges(ctx, F, NULL);  T += tables of Dset(G', F)
 *     deletion  of D:  T -= tables of Dset(G, D);  gnnpe_csr_apply_edges(ctx, NULL, D);  T += tables of Nset(G', D)
 * keeps an induced vertex table exact on the device, and nothing per match leaves the device.  For an edge table the same holds by
 * the key (x, y) of an entry, as in ABI 17; carrying the entries of G to those of G' is the caller's call of
 * gnnpe_csr_carry_entries after gnnpe_csr_apply_edges_map in place of gnnpe_csr_apply_edges (include/gnnpe_hip.h, ABI 20, with the
 * loop written out): on the device as well.
 *
 * All terms are those of the ABI 12 - 18 texts.  Nset_m(C, F) is the set ABI 18 counts (limit 2^64 - 1); m must contain
 * GNNPE_MATCH_INDUCED; F is a set of data vertex pairs that are NOT edges of the loaded graph, handed over as in ABI 18.  The query
 * EDGES (a_k, b_k), k < nqe, are numbered as gnnpe_host_query_edges numbers them -- the rows of the edge table are the query's edges,
 * not its non-adjacent pairs -- and the entry index j is as in ABI 14.
 *
 *   VN_m(C, F)[u][v] = |{ f in Nset : f(u) = v }|                      nq  x n           uint64, row-major
 *   EN_m(C, F)[k][j] = |{ f in Nset : f(a_k) = x and f(b_k) = y }|     nqe x offsets[n]  uint64, j = (x -> y)
 *
 *   - every row of either table sums to |Nset| = N_m(C, F, 2^64 - 1) of ABI 18.
 *   - summing EN row k over the entries of data row x gives VN[a_k][x].
 *   - F = all non-edges of G and a query with a non-adjacent pair: VN = V_m(C) and EN = E_m(C) of ABI 13 / 14 in the same mode.
 *   - INSERTION, the induced modes, the same C on both graphs, G' = G + F with F disjoint from E(G):
 *     V(G') = V(G) - VN(G, F) + VD(G', F), and the same for E compared by the key (x, y) of an entry; an entry of F has E(G) = 0 and
 *     EN(G, F) = 0.
 *   - DELETION, G' = G - D: V(G') = V(G) - VD(G, D) + VN(G', D), and the same for E by keys.
 *   - MIXED BATCH: exact in two steps, delete then insert, as the ABI 18 text has it for the count.
 *   - a query without a non-adjacent pair (1 or 2 vertices, K_n), or n_pairs == 0: the V table is all zeros, the E table is all zeros
 *     (empty for a single-vertex query, as in ABI 14), nothing is launched and *complete = 1.
 *
 * limit, *answers and *complete are exactly those of ABI 17 with N in the place of Delta: *answers = min(N, limit); *complete = 1
 * iff N < limit; with *complete = 0 the table is unspecified and nothing is copied to the host; limit == 0 launches nothing and gives
 * *complete = 0.  host_counts, dev_counts, dev_accum and sign are exactly those of ABI 17 as well: sign must be 1 without dev_accum,
 * host_counts must be NULL with it, every cell of a caller's table ends at old + sign * c mod 2^64, a refused call leaves a caller's
 * table byte for byte as it was, and where nothing is launched it is untouched.
 *
 * Refusals are those of gnnpe_refine_sets_delta_nonedges, all GNNPE_ERR_ARG with *answers = 0: a mode without GNNPE_MATCH_INDUCED or
 * with unknown bits; a loop or an id >= n, refused on the host; a pair that IS an edge, found on the device and reported after the
 * call's single wait, after which the context stays usable (the host forms find it up front).  The sign and dev_accum refusals of
 * ABI 17 apply as well.
 *
 * gnnpe_host_refine_sets_delta_nonedges_vertex_counts, gnnpe_host_refine_sets_delta_nonedges_edge_counts: the host forms, the
 *   yardstick.  The unchanged backtracking of gnnpe_host_refine_sets_mode over all of M; at every find the one key test of
 *   gnnpe_host_refine_sets_delta_nonedges, then the cell increments of gnnpe_host_refine_sets_vertex_counts / _edge_counts.  They
 *   share nothing with the device search.  counts is the caller's (nq x n, nqe x offsets[n]; NULL is accepted for an empty edge table).
 * gnnpe_refine_sets_delta_nonedges_vertex_counts, gnnpe_refine_sets_delta_nonedges_edge_counts: the device forms
 *   (csrc/gnnpe_refine_delta_nonedges_counts.hip): the launches, items and charging rule of gnnpe_refine_sets_delta_nonedges with the
 *   tallies and flushes of the ABI 17 kernels.  Without dev_accum the table lives in a context-owned, grow-only buffer of its own --
 *   one for VN, another for EN, neither of them a buffer of ABI 13, 14 or 17, whose device views keep their documented lifetimes --
 *   zeroed once per call before the first launch, and valid until the next call of the same function on the context or until the
 *   context's rows are loaded or changed.  *device_ms is as in ABI 17.  A table has no rows to page; the rows of Nset come page by
 *   page through gnnpe_refine_pages_open_delta_nonedges (the last section). */
int gnnpe_host_refine_sets_delta_nonedges_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                        const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                        const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                        uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_host_refine_sets_delta_nonedges_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                      const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                      const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                      uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_refine_sets_delta_nonedges_vertex_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                   const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                   uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                   void *dev_accum, int sign, double *device_ms);
int gnnpe_refine_sets_delta_nonedges_edge_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                 const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint32_t mode,
                                                 uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                 void *dev_accum, int sign, double *device_ms);

/* ---- the matches through a set of data vertices, each once ---------------------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section and gnnpe_set_vertex_labels of include/gnnpe_hip.h only add symbols.)
 * ABI 15 - 19 are anchored at data EDGES.  "Which matches contain one of these data VERTICES?" is the question behind a vertex
 * removal, behind a relabel (gnnpe_set_vertex_labels: the matches a new label destroys are asked before it, the ones it creates
 * after it) and behind an ego query.  For a connected query of two or more vertices it can be emulated by gnnpe_refine_sets_delta
 * over every edge incident to the set -- 2 deg(s) single-entry items per vertex and one launch per query edge -- and for a
 * single-vertex query not at all.
 *
 * Terms as in the ABI 12 - 15 texts, M_m(C) as in ABI 13, Dset_m(C, F) as in ABI 17.  S is a set of data vertices, handed over as
 * vertices: n_vertices uint32 ids; repeats are tolerated and mean the vertex once.
 *
 *   Sset_m(C, S)          = { f in M_m(C) : f(u) in S for at least one query vertex u }
 *   DeltaV_m(C, S, limit) = min(limit, |Sset_m(C, S)|)
 *
 * Every such map is counted and listed ONCE, however many of its images lie in S.  All four modes are served.
 *   - S = V: DeltaV = |M_m(C)|.
 *   - S = {s}: DeltaV = the sum over u of V_m(C)[u][s] (ABI 13).
 *   - a connected query with nq >= 2: Sset_m(C, S) = Dset_m(C, E(S)), E(S) the edges of G with an endpoint in S (ABI 15 / 17): a
 *     query vertex has a query neighbour, so an image in S puts a query edge on an edge at S, and the converse is plain.
 *   - nq = 1: DeltaV = the number of s in S n C(0) that pass the label and degree test.  (The edge-anchored calls give 0 there.)
 *   - VERTEX REMOVAL.  G' = G minus E(S), nq >= 2, the same C, any mode: |M(G')| = |M(G)| - DeltaV(G, S).  The vertices of S are
 *     isolated in G' and a connected query asks for degree >= 1; a match that avoids S keeps every adjacency and non-adjacency,
 *     and the degrees it needs (its deg_Q(u) neighbours of f(u) are images outside S).
 *   - RELABEL.  G' = G with new labels on the vertices of S, and C and C' agree on every vertex outside S (a label bitmap of each
 *     graph does).  In any mode, as sets of maps M(G', C') = (M(G, C) - Sset(G, C, S)) + Sset(G', C', S), the union disjoint:
 *     |M(G', C')| = |M(G, C)| - DeltaV(G, C, S) + DeltaV(G', C', S).  A map that avoids S sees the same labels, sets, rows and
 *     degrees in both graphs.
 *   - n_vertices == 0, limit == 0 or an empty C(u): the answer is 0 and nothing is launched.
 *
 * Refusals, all GNNPE_ERR_ARG with *answers = 0 unless gnnpe_refine_sets_mode names another code:
 *   - an id >= n: checked on the host before anything is launched.
 *   - everything else exactly as gnnpe_refine_sets_mode: the whole simple graph on the device, a connected query of 1..32
 *     vertices, no multigraph state, no unknown mode bits.
 *   There is no refusal on the device: a vertex has nothing to look up.
 *
 * gnnpe_host_refine_sets_delta_vertices: the host form, the yardstick.  The backtracking of gnnpe_host_refine_sets_mode, unchanged,
 *   over all of M with one test at every find (is an image in S: a byte mask).  It shares nothing with the device form's search.
 * gnnpe_refine_sets_delta_vertices: the device form (csrc/gnnpe_refine_delta_vertices.hip): one launch per query vertex u over the
 *   first-level chunks of the start candidates S n C(u), in a matching order that starts at u; a map is kept in the launch of its
 *   lowest-numbered query vertex with an image in S only.  Its cost follows DeltaV and nq, not |M|.
 *   matches, matches_cap, the row layout, limit, *device_ms and the ownership of the buffers are exactly those of
 *   gnnpe_refine_sets_delta.  The rows come page by page through gnnpe_refine_pages_open_delta_vertices (the last section); the
 *   count tables of Sset are the next section; adding or removing vertices is gnnpe_csr_apply_vertices of include/gnnpe_hip.h
 *   (the removal loop: lost = DeltaV(G, C, R), apply, |M'| = |M| - lost); slab contexts and multigraph rows are out of scope. */
int gnnpe_host_refine_sets_delta_vertices(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                          const char *query_graph_path, const uint32_t *candidate_bitmap, const uint32_t *vertices,
                                          uint64_t n_vertices, uint64_t limit, uint32_t mode, uint64_t *answers);
int gnnpe_refine_sets_delta_vertices(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                     const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode, uint64_t *answers,
                                     uint32_t *matches, uint64_t matches_cap, double *device_ms);

/* ---- count tables of the matches through a set of data vertices -------------------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section only adds symbols.)
 * The consumers of the ABI 13 and 14 tables keep tables on the device, not rows.  With ABI 17, 19 and 20 such a table stays exact
 * across edge insertions and deletions; the functions below do the same for a relabel and for a vertex removal, what
 * gnnpe_refine_sets_delta_vertices does for the plain count:
 *     T -= tables of Sset(G, C, S);  gnnpe_set_vertex_labels(ctx, S, new labels);  T += tables of Sset(G', C', S)
 * and the same around a removal of E(S) through gnnpe_csr_apply_edges[_map].  Nothing per match leaves the device.
 *
 * Sset_m(C, S) and the hand-over of S are as in the section above, the query edges (a_k, b_k), k < nqe, those of
 * gnnpe_host_query_edges, the entry index j as in ABI 14.
 *
 *   VV_m(C, S)[u][v] = |{ f in Sset : f(u) = v }|                      nq  x n           uint64, row-major
 *   EV_m(C, S)[k][j] = |{ f in Sset : f(a_k) = x and f(b_k) = y }|     nqe x offsets[n]  uint64, j = (x -> y)
 *
 *   - every row of either table sums to |Sset| = DeltaV_m(C, S, 2^64 - 1); summing EV row k over the entries of data row x gives
 *     VV[a_k][x].
 *   - S = V: VV = V_m(C) and EV = E_m(C), the tables of ABI 13 / 14.
 *   - a connected query with nq >= 2: VV(C, S) = VD(C, E(S)) and EV(C, S) = ED(C, E(S)), the tables of ABI 17.
 *   - nq = 1: VV[0][s] = 1 for the s in S n C(0) that pass the label and degree test and 0 elsewhere; EV is empty as in ABI 14.
 *   - RELABEL, any mode, C and C' agreeing outside S: V(G', C') = V(G, C) - VV(G, C, S) + VV(G', C', S), and the same for E with the
 *     same entry indices, because a relabel moves no entry.
 *   - REMOVAL, G' = G - E(S), nq >= 2, the same C: V(G') = V(G) - VV(G, S); for E the same by the key (x, y) of an entry, or through
 *     gnnpe_csr_apply_edges_map and gnnpe_csr_carry_entries (include/gnnpe_hip.h).
 *
 * limit, *answers, *complete, host_counts, dev_counts, dev_accum and sign are exactly those of ABI 17 with DeltaV in the place of
 * Delta: *answers = min(DeltaV, limit); *complete = 1 iff DeltaV < limit; with *complete = 0 the table is unspecified and nothing is
 * copied to the host; limit == 0 launches nothing and gives *complete = 0; an empty C(u), an empty S or no vertex of S in any set
 * launches nothing: a context-owned table is all zeros, a caller's table is untouched, *complete = 1.  sign must be 1 without
 * dev_accum, host_counts must be NULL with dev_accum, and every cell of a caller's table ends at old + sign * c mod 2^64.
 *
 * gnnpe_host_refine_sets_delta_vertices_vertex_counts, gnnpe_host_refine_sets_delta_vertices_edge_counts: the host forms, the
 *   yardstick: the backtracking of gnnpe_host_refine_sets_delta_vertices with the cell increments of
 *   gnnpe_host_refine_sets_vertex_counts / _edge_counts at every find that counts.  counts is the caller's (NULL is accepted for an
 *   empty edge table).
 * gnnpe_refine_sets_delta_vertices_vertex_counts, gnnpe_refine_sets_delta_vertices_edge_counts: the device forms
 *   (csrc/gnnpe_refine_delta_vertices_counts.hip): the launches, items and charging rule of gnnpe_refine_sets_delta_vertices with the
 *   tallies and flushes of the ABI 13 / 14 kernels.  Refusals are those of gnnpe_refine_sets_delta_vertices plus the sign and
 *   dev_accum refusals of ABI 17.  An id >= n is refused on the host before anything is launched, and there is no refusal on the
 *   device: a refused call leaves a caller's table byte for byte as it was.  Without dev_accum the table lives in a context-owned,
 *   grow-only buffer of its own -- one for VV, another for EV, neither a buffer of ABI 13, 14, 17 or 19, whose device views keep
 *   their documented lifetimes -- zeroed once per call on the stream before the first launch, inside *device_ms, and valid until the
 *   next call of the same function on the context or until the context's rows are loaded or changed.  A single-vertex query has
 *   no edge table: the edge call gives *answers = DeltaV and *dev_counts = NULL.  A table has no rows to page; the rows of Sset
 *   come page by page through gnnpe_refine_pages_open_delta_vertices (the last section). */
int gnnpe_host_refine_sets_delta_vertices_vertex_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                        const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                        const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                        uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_host_refine_sets_delta_vertices_edge_counts(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                                      const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                      const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                      uint64_t *answers, int *complete, uint64_t *counts);
int gnnpe_refine_sets_delta_vertices_vertex_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                   const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                   uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                   void *dev_accum, int sign, double *device_ms);
int gnnpe_refine_sets_delta_vertices_edge_counts(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                                 const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint32_t mode,
                                                 uint64_t *answers, int *complete, uint64_t *host_counts, void **dev_counts,
                                                 void *dev_accum, int sign, double *device_ms);

/* ---- paged cursors over the delta matches: edges, non-edges and vertices ---------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section only adds symbols.)
 * A one-shot delta call (gnnpe_refine_sets_delta, _delta_nonedges, _delta_vertices) keeps min(answers, matches_cap) rows and the
 * rest are gone; a delta of 10^9 rows cannot be handed over at once.  The three functions below open the gnnpe_match_cursor of ABI 10
 * over the same sets, and gnnpe_refine_pages_next, _device_ptr, _info and _close serve these cursors as they serve ABI 10's: a
 * continuous-query subscriber, a join against the device page or a writer takes the delta page by page.
 *
 * WHAT COMES OUT.  The set of a cursor is Dset_m(C, F) (gnnpe_refine_pages_open_delta; ABI 17), Nset_m(C, F)
 * (gnnpe_refine_pages_open_delta_nonedges; ABI 18) or Sset_m(C, S) (gnnpe_refine_pages_open_delta_vertices; the vertices section),
 * with F, the pairs and S handed over as in the one-shot call of the same anchor.  Across the pages of a cursor every map of the set
 * comes out exactly once, whatever page_rows is: min(|set|, limit) rows in total, every page except the last exactly page_rows rows.
 * *done, the empty last page, the row layout (column = query vertex id), host_rows == NULL and *device_ms are exactly those of
 * ABI 10.  The order of the rows is unspecified, and so is which maps come out when `limit` cuts.
 *
 * CHARGING.  A map comes out once however many of its query edges, non-adjacent pairs or images land in F or S: the charging rules
 * of the one-shot kernels are used as they are (a map belongs to the launch of its lowest-numbered query edge or non-adjacent pair
 * in F, or of its lowest-numbered query vertex with an image in S).  No match is walked or tested twice because of a page end:
 * the ABI 10 guarantee, which here holds across the launches of the different anchors as well.
 *
 * MODES, REFUSALS.  Those of the one-shot call of the same anchor; every refusal sets *cursor = NULL.
 *   - page_rows == 0: refused, as in ABI 10.
 *   - the non-edge form: a mode without GNNPE_MATCH_INDUCED is refused.
 *   - a loop or an id >= n: GNNPE_ERR_ARG on the host before anything is launched.
 *   - a pair of F that is not an edge (edge form), or that is an edge (non-edge form): found on the device during open, inside the
 *     one wait open has anyway; GNNPE_ERR_ARG with the one-shot call's message, no cursor is handed out, the context stays usable.
 *   - NOTHING TO LAUNCH: where the one-shot call launches nothing -- limit 0, an empty C(u), an empty F or S, no vertex of S in any
 *     set, a single-vertex query under an edge anchor, a query without a non-adjacent pair -- open succeeds and hands out a cursor
 *     that is done before its first page.  The pairs are then not looked up, as the one-shot calls document.
 *
 * OWNERSHIP.  The cursor owns all its device memory: its copy of the bitmap; F as keys, pairs and entries, or S as a bitmap; the
 * candidate lists and item offsets of every launch; counters, suspend slots and one page.  It touches none of the context's buffers
 * of the one-shot calls.  Cursors of any kind, the one-shot delta calls, the count-table calls and the filters may therefore
 * interleave on one context between two pages.  The host arrays may be freed once open returns.
 *
 * LIFETIME.  As in ABI 10; gnnpe_csr_apply_edges[_map] and gnnpe_set_vertex_labels (include/gnnpe_hip.h) change the graph and so
 * invalidate an open delta cursor as well: next returns GNNPE_ERR_ARG and launches nothing, close still works.  For the caller's
 * update loop this means: the cursor over Dset(G, D) of a DELETION batch D is drained before the deletion is applied (it lists
 * matches of G), and the cursor over Dset(G', I) of an INSERTION batch I is opened after the insertion is applied (it lists matches
 * of G'); the same holds for Nset around the opposite change, and for Sset around a relabel or a removal.
 *
 * INFO.  info[5] keeps its five fields.  "First-level items not yet taken" counts the current launch and all later launches of the
 * cursor; "waves suspended" counts the suspend slots that hold a state.  After *done the third and fourth are 0.
 *
 * Device form (csrc/gnnpe_refine_delta_pages.hip): one launch per anchor as in the one-shot calls, under the suspend and resume of
 * ABI 10.  A page that runs from one anchor's launch into the next costs ONE host wait: the launches of the first unfinished anchor
 * and of all later ones are queued back to back, and a launch that finds the page full returns at once.
 * Paged forms of the count tables (no rows), slab contexts and multigraph rows are out of scope. */
int gnnpe_refine_pages_open_delta(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                  const uint32_t *delta_edges, uint64_t n_delta, uint64_t limit, uint64_t page_rows, uint32_t mode,
                                  gnnpe_match_cursor **cursor);
int gnnpe_refine_pages_open_delta_nonedges(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                           const uint32_t *pairs, uint64_t n_pairs, uint64_t limit, uint64_t page_rows, uint32_t mode,
                                           gnnpe_match_cursor **cursor);
int gnnpe_refine_pages_open_delta_vertices(gnnpe_ctx *ctx, const char *query_graph_path, const uint32_t *candidate_bitmap,
                                           const uint32_t *vertices, uint64_t n_vertices, uint64_t limit, uint64_t page_rows,
                                           uint32_t mode, gnnpe_match_cursor **cursor);

/* ---- the standing exact query: resident sets, one call per edge batch -------------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section and gnnpe_filter_support_bitmap_device of include/gnnpe_hip.h only add
 * symbols.)
 * The consumer of the update calls, the support tables and the delta searches: a query that stays open on a changing graph and is
 * told, batch by batch, which matches were created and which destroyed.  Composed by hand (the loops of include/gnnpe_hip.h), every
 * batch reads and plans the query file again for every refinement call, walks the nq x ceil(n/32) words of the candidate sets on the
 * host, uploads them for every delta call and downloads them after every gnnpe_filter_support_bitmap.  A gnnpe_standing handle is
 * opened once per (context, query, mode) and keeps on the device, for as long as it is open: the parsed query and its plans, the
 * support table S, the candidate bitmap C and the exact match count |M|.  Per batch nothing proportional to n crosses to the host
 * (what does: the batch itself, the plan of the support calls, 8 nq bytes of set sizes and the counter blocks).
 *
 * open: the exact plan of gnnpe_host_query_plan_exact at the context's e and the given l (2 or 3), S by gnnpe_filter_support_exact
 *   into a table the handle owns, C from S on the device, and |M| in `mode` (any combination of GNNPE_MATCH_DISTINCT and
 *   GNNPE_MATCH_INDUCED) by the search of gnnpe_refine_sets_mode on the resident sets, limit 2^64 - 1.  *count = |M|.  Requirements
 *   and refusals are those of gnnpe_filter_support_exact and gnnpe_refine_sets_mode: the whole simple graph on the device, the label
 *   table, a current gnnpe_vde, a connected query of 1..32 vertices; a slab context and the multigraph state are GNNPE_ERR_UNSUPPORTED.
 *   At most 16 handles are open on a context (the 17th open is GNNPE_ERR_ARG); they are registered on it as the output pools are,
 *   and gnnpe_destroy closes what is still open.
 * open_sets: no filter.  host_bitmap (nq x ceil(n/32) uint32) is uploaded once and is C from then on.  It must be sound for every
 *   graph the handle will see (a label bitmap is; a degree bitmap is not): the library does not maintain it.  set_bitmap replaces
 *   it and takes the count again (open_sets handles only).  No label table and no gnnpe_vde are needed.
 * rows_cap: the first rows_cap created and the first rows_cap destroyed rows of a batch (nq uint32 each, column = query vertex id)
 *   are kept on the device until the next batch; a cap below the true number truncates the rows, never the counts.
 *
 * gnnpe_standing_apply_edges(ctx, I, D): gnnpe_csr_apply_edges for the graph AND every handle open on the context.  With T the end
 *   vertices of the batch, for every handle
 *       S -= S_T(G);  destroyed = Delta(G, C, D);  apply;  gnnpe_vde;  S += S_T(G');  C' = bitmap(S);  created = Delta(G', C', I)
 *   and count += created - destroyed (Delta: gnnpe_refine_sets_delta; open_sets handles skip the S steps; gnnpe_vde runs where the
 *   context has a label table, so the context comes back with current embeddings).
 *   INDUCED handles also lose the matches that had a non-adjacent pair on an inserted edge and gain those on a deleted one (ABI 18):
 *       destroyed += N(G, C, I) before the apply, created += N(G', C', D) after it       (N: gnnpe_refine_sets_delta_nonedges).
 *   A MIXED batch (both lists non-empty) on a context with an induced handle is applied in two steps, D first and then I, for every
 *   handle: a match of G can run through an edge of D and sit on a pair of I, and one step would count it twice.  created and
 *   destroyed are summed over the two steps; a match that exists only on the graph in between is in both, so the count is exact and
 *   created - destroyed is the change, while the two row lists can hold such a transient match each.  Without an induced handle, or
 *   with one list empty, there is one apply and created / destroyed are exactly M(G') \ M(G) and M(G) \ M(G').
 *   Every search runs with limit 2^64 - 1: the counts are exact.  *device_ms (may be NULL): the sum over the calls inside.
 *   TRANSACTIONAL.  A pair of D that is not an edge, a pair of I that already is one, an edge in both lists, a loop, an id >= n
 *   (GNNPE_ERR_ARG, decided on the host or by one lookup kernel before anything changes), or a device allocation that
 *   gnnpe_csr_apply_edges is refused before its swap (its code): the graph and its generation, every handle's S and C byte for
 *   byte, its count, created, destroyed and kept rows are what they were; where S had lost S_T(G) it is added back on the unchanged
 *   graph.  (A failure of the device AFTER a swap -- the second step of a split batch, or a HIP error -- leaves the graph moved on
 *   and the handles stale.)  The empty batch succeeds, touches neither graph nor generation, and reports created = destroyed = 0 with
 *   no rows.  A context without a handle gets the plain apply (and gnnpe_vde).
 *
 * result: {count, created, destroyed, rows_created, rows_destroyed, graph generation}: the last two say how many rows are held.
 * rows: which = 0 created, 1 destroyed: the first min(cap, held) kept rows to host_rows, *n_rows = held.
 * set_sizes: |C(u)| for u < nq, as k_sets_sizes left them when C was last written.
 * set_members: the ascending ids of C(u) from k_sets_members: the first min(cap, |C(u)|) to host_ids, *n_ids = |C(u)|.
 * bitmap: C to the host (nq x ceil(n/32) uint32), for checks and for handing the sets to the other calls of this header.
 * table: *dev_table = S (nq x n uint64, the handle's; NULL for an open_sets handle), valid until the handle is refreshed or closed.
 *
 * STALENESS.  A handle remembers the graph generation and the label table it is exact for.  gnnpe_set_vertex_labels,
 *   gnnpe_csr_apply_vertices, gnnpe_load_csr (and the other loaders), gnnpe_set_label_table and a plain gnnpe_csr_apply_edges[_map]
 *   behind its back make it stale: every call on it except refresh and close returns GNNPE_ERR_ARG with a message naming
 *   gnnpe_standing_refresh, and gnnpe_standing_apply_edges (like gnnpe_standing_set_labels and gnnpe_standing_apply_vertices below) on
 *   the context refuses as well, before touching anything.
 * refresh: S, C and the count again from the graph as it is (it needs what open needs, a current gnnpe_vde included): the state of a
 *   fresh open, no rows.  An open_sets handle keeps its bitmap, and is refused if n changed.
 * close: frees everything; close(NULL) does nothing.
 *
 * Device code (csrc/gnnpe_standing.hip): k_sets_sizes and k_sets_members; the searches are the kernels of the one-shot calls, which
 * take the resident bitmap through an optional argument of their host scaffold.  DESIGN.md section 3.7, profiles/online_standing.txt.
 *
 * COUNT TABLES KEPT BY THE HANDLE (GNNPE_ABI_VERSION stays 20: symbols are added, and a handle that never calls keep_counts does,
 * byte for byte and launch for launch, what it did before).  The tables of ABI 13 and 14 on a changing graph, without the loop
 * `T -= ED(G, D); apply_map; T = carry(T); T += ED(G', I)` written by hand and without its per-call query file, host walk over C and
 * upload:
 *     V[u][v]: in how many matches of the handle's mode data vertex v is the image of query vertex u (nq x n uint64);
 *     E[k][j]: the same per adjacency entry j of the current graph and query edge k (query edges x entries uint64).
 * keep_counts(which, changes_cap): `which` is GNNPE_STANDING_VERTEX_COUNTS, GNNPE_STANDING_EDGE_COUNTS or both.  The tables are
 *   built now, on the graph as it is, by the searches of gnnpe_refine_sets_vertex_counts / _edge_counts on the resident sets, in the
 *   handle's mode, limit 2^64 - 1, into buffers the handle owns; per table it also reserves a scratch table D of the same size,
 *   zeroed once, for E one spare of the same size (the carry is out of place), and change arrays of changes_cap pairs.  It may be
 *   called again to add the other table or to change changes_cap (a table kept already stays as it is; a new cap empties the held
 *   change lists).  A stale handle is refused; an allocation the device refuses returns its code and leaves the handle as it was,
 *   without the table.
 * gnnpe_standing_apply_edges with such a handle: every step of the loop above also does, with D as dev_accum of the delta count
 *   kernels (ABI 17 and 19),
 *       D -= counts of Delta(G, C, D-list)  [induced: D -= counts of N(G, C, I)]      before the apply,
 *       T and D of E carried through the entry map (gnnpe_csr_carry_entries)           after it,
 *       D += counts of Delta(G', C', I)     [induced: D += counts of N(G', C', D-list)]
 *   the apply being gnnpe_csr_apply_edges_map if any handle on the context keeps E and the plain one otherwise.  After the last step
 *   ONE gnnpe_table_fold (include/gnnpe_hip.h) per kept table moves D into T and leaves the change list; a split induced mixed
 *   batch carries D through both applies and still folds once, so a batch has one change list, in the cells of the graph after it.
 *   The count kernels' answers are the searches' created / destroyed: with rows_cap == 0 the row searches are left out and no match
 *   is searched twice; with rows_cap > 0 both run (and must agree).  A refused batch leaves T and the last batch's change list byte
 *   for byte as they were and D all zeros (one memset); a failure behind a swap makes the handle stale, as before.  refresh (and
 *   set_bitmap) rebuild every kept table and empty the change lists.
 * counts(which: one bit): the table to host_counts (may be NULL), *dev_counts = T (valid until the next batch, refresh or close),
 *   *n_rows x *n_cols its shape.  A single-vertex query has an E of no rows (and *dev_counts = NULL) and a V no edge batch changes.
 * count_changes(which: one bit): the cells the last batch changed, ascending, with new - old as int64: the first
 *   min(cap, changes_cap, n) pairs to host_cells / host_deltas, *n_changes = n, the true number.  A V cell is u * n + v.  An E cell is
 *   k * entries + j with j an entry of the CURRENT graph: entries the batch deleted are gone and not listed, an inserted entry's
 *   delta is its new value, and a cell whose created and destroyed parts cancel is not listed.
 *   counts and count_changes on a handle that does not keep `which` are GNNPE_ERR_ARG.
 * WHY THE TABLES STAY EXACT WHILE C CHANGES.  With the filter, the steps of one batch search with different sets: C before the
 *   apply, C' after it.  Both are SOUND: they hold f(u) for every match f of their graph (in every mode: the filter keeps every
 *   embedding).  A search restricted to a sound set finds exactly the matches of the unrestricted search, so V_m(C) and E_m(C) are
 *   the tables V_m and E_m of the graph itself, whichever sound set was used.  The identities the loop rests on are statements
 *   about those: with M(G) the matches, M(G) \ M(G') is what Delta(G, ., D) (and N(G, ., I)) finds and M(G') \ M(G) what
 *   Delta(G', ., I) (and N(G', ., D)) finds (ABI 17 and 19), so T(G') = T(G) - table(M(G) \ M(G')) + table(M(G') \ M(G)) holds
 *   across the two different sound sets.  open_sets handles rely on the caller's promise above that the bitmap is sound for every
 *   graph the handle will see.
 *
 * LABEL AND VERTEX BATCHES THROUGH THE HANDLE (GNNPE_ABI_VERSION stays 20: symbols are added, and a process that never calls the two
 * entries below runs, launch for launch, what it ran before).  The other two updates of the resident graph, gnnpe_set_vertex_labels
 * and gnnpe_csr_apply_vertices, for the graph AND every handle open on the context, with created / destroyed rows and change lists
 * where gnnpe_standing_refresh has none.  What kept the hand-written loops of include/gnnpe_hip.h off this path is on the device now:
 * the touched sets (gnnpe_csr_closed_neighbourhood, gnnpe_csr_carry_vertex_set, gnnpe_filter_support_exact_delta_device) and S n C(u)
 * of the vertex-anchored searches (k_vset_member_of: nq x ceil(k / 64) ballot words come back for a list of k ids).  DeltaV below is
 * gnnpe_refine_sets_delta_vertices on the resident sets; a kept table takes the tables of the same search into D.
 *
 * gnnpe_standing_set_labels(ctx, vertices, labels, count): the pairs are read as gnnpe_set_vertex_labels reads them.  The current
 *   labels of the listed vertices come back in one gather of 4 count bytes; R* is the vertices whose label really changes, and with
 *   T = R* u N(R*), built once per call, every handle runs
 *       S -= S_T(G);  destroyed = DeltaV(G, C, R*);  gnnpe_set_vertex_labels(R*);  gnnpe_vde;  S += S_T(G');  C' = bitmap(S);
 *       created = DeltaV(G', C', R*);  one gnnpe_table_fold per kept table.
 *   WHY created AND destroyed ARE EXACT.  Let f be a match of G (in any mode: a match maps query vertices to data vertices of equal
 *   label).  If f uses no vertex of R*, every label, edge and non-edge it rests on is the same in G', so f is a match of G' too: it
 *   is in neither difference, and DeltaV(., ., R*) does not find it.  If f uses some r in R* as the image of u, then in G' the
 *   label of r differs from label(u) = label_G(r), so f is no match of G': f is in M(G) \ M(G').  So M(G) \ M(G') is exactly the
 *   matches of G through R*, which is what DeltaV(G, C, R*) finds for a sound C; by the same argument with G and G' exchanged
 *   M(G') \ M(G) is DeltaV(G', C', R*).  A listed vertex that keeps its label would break the second step: a match through it
 *   survives, and both searches would report it.  That is why the no-ops are dropped before anything else.
 *   No edge changes, so an induced handle needs no non-edge search, entries do not move and E needs no carry.  With rows_cap == 0
 *   and a kept table the count kernels' answers serve as created / destroyed, as in the edge path.  An empty R* (count == 0
 *   included) succeeds, touches neither graph nor generation, and reports created = destroyed = 0 with empty change lists.
 *   open_sets handles go along under the promise that their bitmap is sound for every graph the handle sees -- which a LABEL bitmap
 *   does not keep across a relabel: use gnnpe_standing_set_bitmap, or a bitmap that does not depend on the labels.
 *   TRANSACTIONAL as gnnpe_standing_apply_edges.  Decided before anything changes, leaving graph, generation and every handle byte
 *   for byte as they were (GNNPE_ERR_ARG): an id >= n, one vertex listed with two labels, a stale handle, and -- where a filter
 *   handle is open and the context has a label table -- a new label without a row in the table, which gnnpe_vde would refuse
 *   behind the change.  A failure before the relabel puts S back and zeroes D; a failure after it makes the handles stale.
 *
 * gnnpe_standing_apply_vertices(ctx, remove, n_remove, add_labels, n_add, &n_after): with R the removed vertices, A the added ones
 *   (the last n_add ids of G') and T = R u N_G(R), every handle runs
 *       S -= S_T(G);  destroyed = DeltaV(G, C, R);  gnnpe_csr_apply_vertices (with the entry map where a handle keeps E);
 *       S, and T and D of V, through gnnpe_csr_carry_vertices;  T and D of E through gnnpe_csr_carry_entries;  gnnpe_vde;
 *       T' = gnnpe_csr_carry_vertex_set(T, with_added);  S += S_T'(G');  C' = bitmap(S) at n';  created = DeltaV(G', C', A);  fold.
 *   A match of G is lost exactly when it uses a removed vertex; a match of G' is new exactly when it uses an added one, and an added
 *   vertex is isolated, so it completes a match of a single-vertex query only -- the general search covers that.
 *   The destroyed rows are in the ids of G; the created rows and both change lists are in the ids of G'.  The cells of removed
 *   vertices and entries are gone and not listed, the rule the E change list has for deleted entries.
 *   The out-of-place carries of S and V need a spare each; they and every table are given room for max(n, n') before the swap, and
 *   the spares are made at the first vertex batch, so a handle that only sees edge batches allocates nothing new.
 *   Refusals before anything changes: gnnpe_csr_apply_vertices' own (a null list, an id >= n, n' == 0, the id ranges), an added label
 *   without a row in the label table, a stale handle, and a gnnpe_standing_open_sets handle open on the context
 *   (GNNPE_ERR_UNSUPPORTED: its bitmap was made for the old n).  A refusal inside the apply before its swap puts S back and zeroes
 *   D.  The empty batch is a no-op.  *n_after = n'.
 *
 * PEELING THE GRAPH BY EDGE SUPPORT: the (Q, t)-truss and the truss level of every edge (GNNPE_ABI_VERSION stays 20: symbols are
 * added, and a process that never calls the two entries below runs, launch for launch, what it ran before).  The consumer the table
 * E was introduced for, written against the library without taking E off the device: gnnpe_csr_edges_below of include/gnnpe_hip.h
 * selects on the resident table, and only the selected pairs, 8 bytes per edge, cross to the host.
 * Definitions.  The handle keeps E with nqe rows.  The undirected edge {x, y} has the entry j = (x -> y) and its reverse r = (y -> x).
 *     SUPPORT  sup(x, y) = sum over k < nqe of (E[k][j] + E[k][r]), the uint64 sum mod 2^64 like every table sum here: the number of
 *              (match, query edge) incidences on the data edge.  For a triangle handle in DISTINCT mode it is the number of
 *              triangles on the edge, in mode 0 six times that.  The caller chooses the threshold in these units.
 *     (Q, t)-TRUSS of G: the largest subgraph on the same vertices in which every edge has sup >= t, matches counted inside the
 *              subgraph.
 *     LEVEL    of an edge: the largest t for which it belongs to the (Q, t)-truss.
 * WHY THE FIXPOINT IS UNIQUE.  For a handle that is not INDUCED a match of a subgraph H of G is a match of G: it rests on edges and
 *   labels only.  So deleting edges only destroys matches, whichever sound candidate sets the steps search with (the argument of
 *   "WHY THE TABLES STAY EXACT" above: the tables are those of the graph itself), and sup is monotone under deletion: sup_H <= sup_G
 *   on the edges of H.  If H1 and H2 have all supports >= t, so has their union, since each of its edges lies in an Hi and
 *   sup of the union >= sup_Hi: there is a largest such subgraph.  An edge with sup < t in some graph between G and the truss has
 *   sup < t in every smaller graph and is not in the truss, so every peeling order removes exactly the edges outside it and ends at
 *   the same graph.  INDUCED handles are refused (GNNPE_ERR_UNSUPPORTED): a deletion can create induced matches, support is not
 *   monotone and the fixpoint is not unique.
 * gnnpe_standing_peel(sq, min_support, max_rounds, host_removed, host_round, cap, out): each round
 *       gnnpe_csr_edges_below(E of sq, nqe, min_support) into a context-owned, grow-only pair buffer;
 *       nothing selected: stop, converged;
 *       the selected pairs cross to the host and are the delete_edges of ONE gnnpe_standing_apply_edges on the context.
 *   All edges below the threshold go at once, so the rounds are determined.  Going through gnnpe_standing_apply_edges means that every
 *   handle open on the context moves forward exactly as for a caller's batch (an induced handle of another query is fine there: the
 *   batch only deletes), and every kept table and every handle's S, C and count stay exact.  max_rounds == 0 means no limit;
 *   otherwise the loop ends after max_rounds rounds that deleted something.  out = {rounds that deleted something, edges removed,
 *   undirected edges left, converged}: converged is 1 only if a select found nothing, so a peel cut by max_rounds reports 0 and a
 *   second call goes on where it stopped.  host_removed (cap x 2 uint32) and host_round (cap uint32, may be NULL; rounds count from
 *   1) get the first cap removed edges in removal order.  The handle's result, rows and count_changes describe the last round, as for
 *   any batch; a peel that removes nothing (min_support == 0 for instance) touches neither graph nor generation nor those.
 *   Refused before anything changes: a stale handle (this one or another on the context), a handle that does not keep E
 *   (GNNPE_ERR_ARG, naming gnnpe_standing_keep_counts), a query without an edge (no E), an INDUCED handle (GNNPE_ERR_UNSUPPORTED).
 *   A failure inside round i leaves the graph and all handles in the state after round i - 1, because each round is one
 *   transactional batch; out and host_removed say how far the loop came.
 * gnnpe_standing_truss_levels(sq, restore, host_edges, host_levels, cap, out): t = min_kept of a select with threshold 0; peel with
 *   min_support = t + 1, everything removed gets level t; t = the new min_kept, which is larger; until no edge is left.  The jump
 *   makes the number of peels the number of distinct levels, not the largest support.  out = {edges, distinct levels, largest
 *   level, rounds in all}; the first cap edges come out in removal order, which is by level, with their levels.  Refusals: those of
 *   the peel.  restore != 0: one closing gnnpe_standing_apply_edges inserts every removed edge again; the graph is then the compact
 *   CSR of the original and count, sets and tables are those of before the call (the generation has moved on).  Its cost is one delta
 *   search over ALL edges, which the table of DESIGN.md section 3.7 prices at 1.3 to 4.8 full counts.  restore == 0 leaves the
 *   context with the empty graph on n vertices.  A failure on the way leaves the graph peeled as far as the loop came, nothing is
 *   restored, and out and host_edges say what was removed.  (A support of 2^64 - 1 has no threshold above it: GNNPE_ERR_RANGE.)
 * gnnpe_host_truss_levels: the host form and the library's own slow statement of the definition (host/online_capi.cpp): it peels
 *   the same way on a host CSR and counts E from scratch with gnnpe_host_refine_sets_edge_counts every round.  Modes as above.
 * Out of scope: a vertex form (a (Q, t)-core: removing vertices renumbers ids), a device-list apply (the list has to reach the host
 *   anyway to be reported), induced handles, slab contexts and multigraph rows, and a second-level split of hub items inside the
 *   delta searches: the peel inherits the known cost of a batch that deletes hub edges under large queries (DESIGN.md section 3.7,
 *   "Known and accepted").  csrc/gnnpe_standing.hip, profiles/online_standing_peel.txt.
 *
 * Not yet: a (Q, t)-core by vertex removal, a peel whose selected list stays on the device, vertex batches with an open_sets handle on the context, an automatic switch to gnnpe_standing_refresh where a batch
 * touches so much that recomputing is cheaper (profiles/online_standing_updates.txt has where that is), a fused carry-and-fold for E (T and D of E are carried as two gathers per apply), paged change lists (what is behind changes_cap is counted, not held), a device plan handle for
 * the support calls (their plan is uploaded per call), slab contexts, multigraph rows. */
#define GNNPE_STANDING_VERTEX_COUNTS 1u
#define GNNPE_STANDING_EDGE_COUNTS 2u
typedef struct gnnpe_standing gnnpe_standing;
int gnnpe_standing_open(gnnpe_ctx *ctx, const char *query_graph_path, uint32_t l, double epsilon, uint32_t mode, uint64_t rows_cap,
                        gnnpe_standing **sq, uint64_t *count, double *device_ms);
int gnnpe_standing_open_sets(gnnpe_ctx *ctx, const char *query_graph_path, uint32_t mode, uint64_t rows_cap,
                             const uint32_t *host_bitmap, gnnpe_standing **sq, uint64_t *count, double *device_ms);
int gnnpe_standing_set_bitmap(gnnpe_standing *sq, const uint32_t *host_bitmap);
int gnnpe_standing_apply_edges(gnnpe_ctx *ctx, const uint32_t *insert_edges, uint64_t n_insert, const uint32_t *delete_edges,
                               uint64_t n_delete, double *device_ms);
int gnnpe_standing_set_labels(gnnpe_ctx *ctx, const uint32_t *vertices, const uint32_t *labels, uint64_t count, double *device_ms);
int gnnpe_standing_apply_vertices(gnnpe_ctx *ctx, const uint32_t *remove, uint64_t n_remove, const uint32_t *add_labels, uint64_t n_add,
                                  uint32_t *n_after, double *device_ms);
int gnnpe_standing_result(gnnpe_standing *sq, uint64_t out[6]);
int gnnpe_standing_rows(gnnpe_standing *sq, int which, uint32_t *host_rows, uint64_t cap, uint64_t *n_rows);
int gnnpe_standing_set_sizes(gnnpe_standing *sq, uint64_t *sizes);
int gnnpe_standing_set_members(gnnpe_standing *sq, uint32_t u, uint32_t *host_ids, uint64_t cap, uint64_t *n_ids);
int gnnpe_standing_bitmap(gnnpe_standing *sq, uint32_t *host_bitmap);
int gnnpe_standing_table(gnnpe_standing *sq, void **dev_table);
int gnnpe_standing_keep_counts(gnnpe_standing *sq, uint32_t which, uint64_t changes_cap, double *device_ms);
int gnnpe_standing_counts(gnnpe_standing *sq, uint32_t which, uint64_t *host_counts, void **dev_counts, uint64_t *n_rows,
                          uint64_t *n_cols);
int gnnpe_standing_count_changes(gnnpe_standing *sq, uint32_t which, uint64_t *host_cells, int64_t *host_deltas, uint64_t cap,
                                 uint64_t *n_changes);
int gnnpe_standing_peel(gnnpe_standing *sq, uint64_t min_support, uint32_t max_rounds, uint32_t *host_removed, uint32_t *host_round,
                        uint64_t cap, uint64_t out[4], double *device_ms);
int gnnpe_standing_truss_levels(gnnpe_standing *sq, int restore, uint32_t *host_edges, uint64_t *host_levels, uint64_t cap,
                                uint64_t out[4], double *device_ms);
int gnnpe_host_truss_levels(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                            const char *query_graph_path, const uint32_t *candidate_bitmap, uint32_t mode, uint32_t *edges,
                            uint64_t *levels, uint64_t cap, uint64_t out[4]);
int gnnpe_standing_refresh(gnnpe_standing *sq, uint64_t *count, double *device_ms);
int gnnpe_standing_close(gnnpe_standing *sq);

#ifdef __cplusplus
}
#endif
#endif
