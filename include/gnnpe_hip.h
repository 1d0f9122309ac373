/*
 * gnnpe_hip.h -- C-ABI of the MI355X offline path-embedding engine (libgnnpe_hip.so).
 *
 * The reference (JamesWhiteSnow/GNN-PE) has no plugin / FFI seam: `custom.h` is a header of free
 * functions included by one translation unit.  This header is therefore the seam a
 * maintainer would add: every entry point names the reference function (file:line under
 * /root/reference/) whose work it takes over.  INTEGRATION.md shows the call sites in
 * GNN-PE/src/main.cpp.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, <0 on error; gnnpe_last_error() gives the message
 *     (thread local).  Unlike the reference, nothing calls exit() (functions.cpp:24-29).
 *   - "host" pointers are ordinary CPU memory owned by the caller; "dev" pointers are HIP device
 *     memory on the context's device (e.g. a torch tensor's data_ptr()).  The library owns every
 *     other device allocation behind the opaque context.
 *   - one context per GPU, driven from one host thread; work is enqueued on the context's stream
 *     (gnnpe_set_stream) and host-returning calls synchronise that stream.
 *   - ids are uint32 like the reference (`ui`, include/configuration/types.h:13-17); path counts and
 *     path ids are uint64 so inputs beyond the reference's 2^32 limit can be counted and streamed.
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails.
 */
#ifndef GNNPE_HIP_H
#define GNNPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNPE_ABI_VERSION 20

#define GNNPE_OK 0
#define GNNPE_ERR_ARG (-1)     /* bad argument / call order */
#define GNNPE_ERR_HIP (-2)     /* a HIP runtime call failed (message has the HIP error string) */
#define GNNPE_ERR_UNSUPPORTED (-3)
#define GNNPE_ERR_IO (-4)
#define GNNPE_ERR_RANGE (-5)   /* output does not fit the reference's 32-bit limits */

typedef struct gnnpe_ctx gnnpe_ctx;

int gnnpe_abi_version(void);
const char *gnnpe_last_error(void);

/* ---- context --------------------------------------------------------------------------------- */
/* Binds to HIP device `device_id`.  Returns NULL (and sets last_error) when no device is usable. */
gnnpe_ctx *gnnpe_create(int device_id);
void gnnpe_destroy(gnnpe_ctx *ctx);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the context's own. */
int gnnpe_set_stream(gnnpe_ctx *ctx, void *hip_stream);
int gnnpe_sync(gnnpe_ctx *ctx);

/* Device buffers for callers without a HIP runtime of their own (the C++ host CLI); Python callers
 * pass torch tensors instead.  gnnpe_copy_to_host synchronises the context's stream. */
int gnnpe_dev_alloc(gnnpe_ctx *ctx, uint64_t bytes, void **dev_ptr);
int gnnpe_dev_free(gnnpe_ctx *ctx, void *dev_ptr);
int gnnpe_copy_to_host(gnnpe_ctx *ctx, void *host_dst, const void *dev_src, uint64_t bytes);
int gnnpe_device_count(void);
/* The context's stream as a hipStream_t (for callers that enqueue their own work behind the engine's, e.g. the RCCL
 * send/recv of the C++ host's halo exchange), and an asynchronous device-to-device copy on it (either end may be memory
 * of another device of this process). */
int gnnpe_get_stream(gnnpe_ctx *ctx, void **hip_stream);
int gnnpe_copy_device(gnnpe_ctx *ctx, void *dev_dst, const void *dev_src, uint64_t bytes);
/* Page-locked host memory for buffers that receive gnnpe_copy_to_host / gnnpe_fill_paths output (PCIe-rate copies). */
int gnnpe_pinned_alloc(uint64_t bytes, void **host_ptr);
void gnnpe_pinned_free(void *host_ptr);

/* ---- inputs ---------------------------------------------------------------------------------- */
/* R0: the CSR that Static_Graph::loadGraphFromFile builds (graph.cpp:163-242; accessors
 * graph.h:154-176): offsets[n+1], neighbours sorted ascending per vertex, labels[n].  Host -> HBM. */
int gnnpe_load_csr(gnnpe_ctx *ctx, uint32_t n, const uint32_t *host_offsets, const uint32_t *host_nbrs,
                   const uint32_t *host_labels);

/* Vertex-partitioned variant (multi-GPU): this context holds the adjacency rows of
 * `rows[0..n_rows)` only (global vertex ids, any order; the rank's owned start vertices in
 * processing order), row k occupying row_nbrs[row_offsets[k] .. row_offsets[k+1]).  labels[n] is
 * replicated.  `nbr_capacity` reserves room (in neighbour entries) for halo rows appended later. */
int gnnpe_load_rows(gnnpe_ctx *ctx, uint32_t n, const uint32_t *host_labels, uint32_t n_rows,
                    const uint32_t *host_rows, const uint64_t *host_row_offsets, const uint32_t *host_row_nbrs,
                    uint64_t nbr_capacity);

/* Non-simple input: duplicate `e` lines.  Static_Graph::loadGraphFromFile stores what it reads (graph.cpp:211-218: no
 * de-duplication), so `degree` (graph.h:154-156) and the neighbour sum of gen_vde (custom.h:527-534) count the repeats, while
 * the hash set drops a path met again (custom.h:68-77).  The engine's enumeration takes simple rows, so such a graph is loaded
 * in two steps: gnnpe_load_csr / gnnpe_load_rows with every row WITHOUT its repeats (what the DFS + hash set amount to;
 * gnnpe_host_load_multigraph returns both forms), then this call with the same rows as the reference holds them (ascending,
 * repeats kept; row k of the loaded rows occupies row_nbrs[row_offsets[k] .. row_offsets[k+1])).  The library checks on the
 * device that the two forms belong together.  Afterwards gnnpe_vde sums over the rows given here, and with the whole graph
 * loaded the degree columns of the auxiliary index and the online filter are these rows' lengths (a slab-only context passes
 * them through gnnpe_set_degrees).  Reset by the next gnnpe_load_csr / gnnpe_load_rows.  GNN-PGE's groups and the refinement
 * refuse a context in this state.  Self entries are refused here as everywhere: for `e u u` the reference's loader writes one
 * slot twice and leaves the next one uninitialised (graph.cpp:211-218) -- it has no defined result to match. */
int gnnpe_set_multigraph_rows(gnnpe_ctx *ctx, uint32_t n_rows, const uint64_t *host_row_offsets, const uint32_t *host_row_nbrs);

/* R1: processing order and partition of every vertex, as main.cpp:77-85 reads them from
 * membership.txt (line i = "<sorted_nodes[i]> <membership[sorted_nodes[i]]>").  p = partition_num. */
int gnnpe_set_order(gnnpe_ctx *ctx, const uint32_t *host_sorted_nodes, const uint32_t *host_membership,
                    uint32_t p);

/* Slab of the processing order this context enumerates: start vertices sorted_nodes[begin..end).
 * Default (never called) = [0, n).  Multi-GPU: rank r owns one contiguous slab, so its paths are one
 * contiguous range of global path ids. */
int gnnpe_set_slab(gnnpe_ctx *ctx, uint32_t begin, uint32_t end);

/* R3: x_table[label][k] = gen_vde_x(label)[k] (custom.h:492-511), n_labels x e doubles.  The table
 * is host arithmetic (std::mt19937 re-seeded per label); host/label_table.cpp computes it. */
int gnnpe_set_label_table(gnnpe_ctx *ctx, uint32_t n_labels, uint32_t e, const double *host_x_table);

/* R3 itself: host arithmetic, exactly the reference's gen_vde_x (custom.h:492-511) for labels
 * 0..n_labels-1: std::mt19937(label), e draws of std::uniform_real_distribution<double>(0,1),
 * divided by their left-to-right sum.  out: n_labels x e doubles.  Needs no GPU. */
int gnnpe_host_label_table(uint32_t n_labels, uint32_t e, double *out);

/* R0 / R1 on the host, for callers that are not the C++ CLI (same code: host/graph_loader.cpp).
 * gnnpe_host_load_graph parses a `.graph` file like Static_Graph::loadGraphFromFile
 * (graph.cpp:163-242); the arrays are malloc'ed by the library, release them with gnnpe_host_free.
 * meta = {labels_count, max_degree, max_label_frequency} (printGraphMetaData, graph.cpp:244-247).
 * Returns 0, -1 (cannot open: the reference exits with -1) or -2 (malformed; gnnpe_last_error). */
int gnnpe_host_load_graph(const char *path, uint32_t *n, uint32_t *m, uint32_t **offsets, uint32_t **nbrs,
                          uint32_t **labels, uint32_t meta[3]);
/* The same loader without the refusal of duplicate `e` lines (gnnpe_host_load_graph answers -2 for them; both answer -2 for a
 * self-loop): offsets / nbrs are the rows as graph.cpp:211-233 leaves them; for a file with repeated lines simple_offsets /
 * simple_nbrs receive the de-duplicated rows (see gnnpe_set_multigraph_rows), else NULL. */
int gnnpe_host_load_multigraph(const char *path, uint32_t *n, uint32_t *m, uint32_t **offsets, uint32_t **nbrs,
                               uint32_t **labels, uint32_t meta[3], uint32_t **simple_offsets, uint32_t **simple_nbrs);
/* membership.txt (main.cpp:77-85): sorted_nodes[n], membership[n] caller-allocated; p = partition_num. */
int gnnpe_host_read_membership(const char *path, uint32_t n, uint32_t p, uint32_t *sorted_nodes, uint32_t *membership);
void gnnpe_host_free(void *ptr);

/* ---- ABI version 16: edge insertions and deletions applied to the resident graph -------------------------------------------
 * gnnpe_load_csr is the only other way to change the graph a context holds: the caller rebuilds the whole CSR and uploads all of
 * it for a handful of edges.  These calls apply a BATCH of undirected edge insertions I and deletions D to the whole graph the
 * context holds, on the device, from the few kilobytes that describe the batch.  It is the middle step of the loop that
 * gnnpe_refine_sets_delta (include/gnnpe_online.h, ABI 15) exists for: delta over D on G, apply, delta over I on G'.
 *
 * Edge lists.  insert_edges / delete_edges: k x 2 uint32 pairs (x, y), either orientation.  A repeat, or both orientations of one
 * edge, inside one list means the edge once (as gnnpe_refine_sets_delta takes F).  Either list may be NULL where its count is 0.
 *
 * Result.  G' = (E(G) minus D) plus I on the same n vertices with the same labels, as a COMPACT CSR: row x starts at the sum of
 * the new degrees below x, the rows lie back to back, each strictly ascending.  The layout is determined by G' alone, so the
 * entry indices j of gnnpe_refine_sets_edge_counts after the call index exactly the arrays the host form and gnnpe_csr_download
 * return.
 *
 * State after a successful device call: precisely what gnnpe_load_csr(ctx, n, offsets', nbrs', labels) leaves, offsets' / nbrs'
 * being the compact CSR of G'.  The graph generation moves on, so open match cursors (gnnpe_refine_pages_*) refuse to go on; the
 * reverse positions, the hub-row list and the neighbours' labels are rebuilt; order, slab, label-table results, counts and
 * everything else derived from the rows are reset as the loader resets them; the device tables of
 * gnnpe_refine_sets_vertex_counts / _edge_counts are no longer valid (their "rows loaded or changed").
 *
 * Refusals.  Each leaves the context exactly as it was -- the same graph, the same generation (open cursors go on working),
 * derived state kept: the new arrays are built in spare buffers and swapped in only on success.
 *   - GNNPE_ERR_ARG, on the host before anything is launched: x == y, or an id >= n.
 *   - GNNPE_ERR_ARG, found on the device and reported through one counter block in the call's single wait: an insertion that is
 *     already an edge of G, a deletion that is not, one edge in both lists (any orientations).  The message names one offending
 *     pair, the same one on every run.
 *   - GNNPE_ERR_UNSUPPORTED: no whole graph on the device (nothing loaded, or gnnpe_load_rows), or the multigraph state.
 *   - GNNPE_ERR_RANGE: entries' + n >= 2^32, the bound the 32-bit offsets and the refinement's items already live under.
 *   - an allocation the device refuses before the swap (the spare arrays, the batch's work area, a larger revpos / label array)
 *     returns its error and leaves the context usable and unchanged.  The rebuild after the swap is gnnpe_load_csr's own tail and
 *     fails as that does: if the device refuses the few words of the hub list or of the sort's temporary storage there, the context
 *     is left without a graph, as after a failed gnnpe_load_csr, and takes the next gnnpe_load_csr.
 * n_insert == n_delete == 0 succeeds, launches nothing and changes nothing: the generation stays, cursors stay valid.
 *
 * gnnpe_host_csr_apply_edges: the host form (host/graph_update.cpp): sort and de-duplicate the keys, merge row by row.  The same
 *   semantics and refusals (no context, so no UNSUPPORTED); nothing is written on a refusal.  out_offsets: n + 1 words; out_nbrs:
 *   out_cap words -- too few returns GNNPE_ERR_ARG with *n_entries_after set (entries + 2 n_insert always suffices).  It shares
 *   no code with the device form: it is its yardstick, and the host mirror of a caller (the host forms of the refinements take the
 *   CSR, and the edge-count tables are indexed by its entries).
 * gnnpe_csr_apply_edges: the device form (csrc/gnnpe_update.hip).  *n_entries_after (may be NULL) = offsets'[n]; on a refusal it
 *   holds the unchanged graph's entries.  *device_ms (may be NULL) covers everything between the upload of the keys and the end of
 *   the rebuild of the derived structure, not the uploads.  Transient memory: a second neighbour array (and second start / degree
 *   arrays), kept as the next call's spare (ping-pong, grow-only).
 * gnnpe_csr_download: the CSR the context holds, back on the host -- for a caller without a host mirror, the arrays the edge tables
 *   index.  Whole graph only (GNNPE_ERR_UNSUPPORTED otherwise).  host_offsets: n + 1 words; nbrs_cap too small returns
 *   GNNPE_ERR_ARG with *n_entries set. */
int gnnpe_host_csr_apply_edges(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs,
                               const uint32_t *insert_edges, uint64_t n_insert,
                               const uint32_t *delete_edges, uint64_t n_delete,
                               uint32_t *out_offsets, uint32_t *out_nbrs, uint64_t out_cap,
                               uint64_t *n_entries_after);
int gnnpe_csr_apply_edges(gnnpe_ctx *ctx, const uint32_t *insert_edges, uint64_t n_insert,
                          const uint32_t *delete_edges, uint64_t n_delete,
                          uint64_t *n_entries_after, double *device_ms);
int gnnpe_csr_download(gnnpe_ctx *ctx, uint32_t *host_offsets, uint32_t *host_nbrs,
                       uint64_t nbrs_cap, uint64_t *n_entries);

/* ---- ABI version 20: the entry map of a batch, and a caller's per-entry table carried through it -----------------------------
 * A per-edge table (gnnpe_refine_sets_edge_counts and its delta forms of include/gnnpe_online.h, a caller's truss numbers or edge
 * ids) is indexed by the adjacency entry j of the compact CSR, and gnnpe_csr_apply_edges moves every entry behind the first row it
 * touches.  These calls keep such a table on the device across a batch: the apply hands out where every entry of G' came from,
 * the carry moves the table.
 *
 * The map.  One uint32 per entry j' = (x -> y) of G': the index j of the entry (x -> y) in G if G has it, GNNPE_NO_ENTRY if it has
 * not (an inserted edge).  Both CSRs are sorted by (x, y), so the map is strictly increasing over the entries that are not
 * GNNPE_NO_ENTRY, and its image is exactly the entries of G that are not in D.
 *
 * gnnpe_host_csr_entry_map: the host form and the yardstick (host/graph_update.cpp): any two compact simple CSRs on the same n
 *   vertices, a two-pointer walk per row; map: new_offsets[n] words.  It shares no code with the device form.  A null argument
 *   returns GNNPE_ERR_ARG.
 * gnnpe_csr_apply_edges_map: everything gnnpe_csr_apply_edges does -- the same lists, result, state afterwards, refusals and
 *   transactional guarantee -- and the map, written by the merge kernel beside the neighbour words into a context-owned, grow-only
 *   device buffer that *dev_map names.  *n_entries_before / *n_entries_after (each may be NULL) are set on every return: on a
 *   refusal both hold the unchanged graph's entry count.  The map is valid until the next gnnpe_csr_apply_edges_map on the context,
 *   a plain gnnpe_csr_apply_edges (of any batch), or any other call that loads or changes the context's rows.  A REFUSED batch
 *   leaves the graph, the generation and the derived state as they were (the ABI 16 guarantee) and leaves the context WITHOUT a
 *   valid map, *dev_map = NULL: the map of an earlier batch is gone too.  The empty batch (n_insert == n_delete == 0) succeeds,
 *   leaves the graph and the generation alone as ABI 16 does, and produces the identity map, so a caller's loop needs no special
 *   case.  *device_ms covers what gnnpe_csr_apply_edges's covers, the map included.
 * gnnpe_csr_carry_entries: for r < n_rows and j' < entries_after, dst[r][j'] = src[r][map[j']], or 0 where the map says
 *   GNNPE_NO_ENTRY, through the context's valid map.  src is row-major n_rows x entries_before, dst row-major n_rows x
 *   entries_after, cells of elem_bytes = 8 (the count tables) or 4 (per-entry ids, truss numbers); both are the caller's device
 *   memory on the context's device, aligned to their cells.  The work runs on the context's stream; every cell of dst is written
 *   exactly once, src is not written.  GNNPE_ERR_ARG, with nothing launched: the context has no valid map (none was made, the last
 *   gnnpe_csr_apply_edges_map was refused, or the rows were loaded or changed since), elem_bytes is neither 4 nor 8, a pointer is
 *   null or misaligned while there is something to move, or the byte ranges of src and dst overlap.  n_rows == 0 or
 *   entries_after == 0 succeeds and launches nothing.  The entries of D simply do not appear in dst.
 *
 * The loop for an edge table T (E = gnnpe_refine_sets_delta_edge_counts, EN = gnnpe_refine_sets_delta_nonedges_edge_counts, both
 * with the caller's table as dev_accum; the EN terms in the induced modes only, where a mixed batch takes the two steps one after
 * the other as the ABI 18 text requires):
 *     T -= E(G, D);   gnnpe_csr_apply_edges_map(D);  T = carry(T);  T += EN(G', D)
 *     T -= EN(G, I);  gnnpe_csr_apply_edges_map(I);  T = carry(T);  T += E(G', I)
 * By the time of the carry the entries of D hold zero in T -- every match through an edge of D was subtracted by E(G, D) -- so
 * dropping them loses nothing; the entries of I start from the zero the carry writes. */
#define GNNPE_NO_ENTRY 0xFFFFFFFFu

int gnnpe_host_csr_entry_map(uint32_t n, const uint32_t *old_offsets, const uint32_t *old_nbrs,
                             const uint32_t *new_offsets, const uint32_t *new_nbrs, uint32_t *map);
int gnnpe_csr_apply_edges_map(gnnpe_ctx *ctx, const uint32_t *insert_edges, uint64_t n_insert,
                              const uint32_t *delete_edges, uint64_t n_delete,
                              uint64_t *n_entries_before, uint64_t *n_entries_after,
                              void **dev_map, double *device_ms);
int gnnpe_csr_carry_entries(gnnpe_ctx *ctx, uint32_t n_rows, uint32_t elem_bytes,
                            const void *dev_src, void *dev_dst, double *device_ms);

/* ---- folding a scratch table into a count table -----------------------------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section only adds a symbol.)
 * gnnpe_table_fold: dev_table and dev_delta are `cells` uint64 each on the context's device, 8-byte aligned, not overlapping.
 *   After the call table[i] = table[i] + delta[i] mod 2^64 for every i and delta is all zeros.  With n the number of nonzero
 *   delta[i], the first min(cap, n) pairs (i, (int64) delta[i]), in ascending i, sit in dev_change_cells (uint64) and
 *   dev_change_deltas (int64); nothing behind min(cap, n) is written; *n_changes = n whatever cap is.  The change arrays may be NULL
 *   iff cap == 0.  GNNPE_ERR_ARG before any launch: a null or misaligned pointer, ranges that overlap (any two of the four), a
 *   missing change array with cap > 0.  cells == 0 succeeds with *n_changes = 0.  The work runs on the context's stream with one
 *   host wait, for n_changes.
 *   The consumer is the standing exact query that keeps its count tables (gnnpe_standing_keep_counts of include/gnnpe_online.h):
 *   the delta count kernels of a batch add into a scratch table, the fold moves it into the table.  The zeroing happens inside the
 *   fold, so no batch pays a memset of the table's size; a refused batch is one memset of the scratch with the table untouched; and
 *   the list of changed cells comes out of the same pass.  Two passes over fixed tiles (csrc/gnnpe_table_fold.hip): a tile without a
 *   nonzero cell costs the second pass one word. */
int gnnpe_table_fold(gnnpe_ctx *ctx, void *dev_table, void *dev_delta, uint64_t cells, void *dev_change_cells, void *dev_change_deltas,
                     uint64_t cap, uint64_t *n_changes, double *device_ms);

/* ---- the edges whose support in a per-entry table lies below a threshold --------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section only adds symbols.)
 * dev_table is n_rows x entries uint64, row-major, over the adjacency entries of the whole simple graph resident now (the table E of
 * ABI 14, or what a standing query keeps).  The undirected edge {x, y} has the entry j = (x -> y) and its reverse entry r = (y -> x);
 *     sup(x, y) = sum over k < n_rows of (table[k][j] + table[k][r]),  a uint64 sum mod 2^64 like every table sum here.
 * gnnpe_csr_edges_below selects the edges with sup < threshold, each once, as (x, y) with x < y, in ascending order of the entry
 *   x -> y, which is ascending (x, y).  The first min(cap, *n_selected) pairs go to dev_pairs (cap x 2 uint32 on the context's
 *   device); nothing is written at or behind cap.  *n_selected is the true number of selected edges whatever cap is.  *min_kept is
 *   the smallest support among the edges NOT selected, 2^64 - 1 if there is none: the next threshold at which something happens,
 *   which lets a decomposition jump from level to level.  threshold == 0 selects nothing and still reports *min_kept.  The table
 *   is only read.  A graph without edges succeeds with 0 and 2^64 - 1.  The work runs on the context's stream with one host wait,
 *   for the two result words.  dev_pairs may be NULL iff cap == 0; device_ms may be NULL.
 *   GNNPE_ERR_ARG, with nothing launched and nothing written: a null argument, a table not aligned to 8 bytes (dev_pairs: to 4), dev_pairs
 *   overlapping the table, cap > 0 without dev_pairs, n_rows == 0, a slab context (anything but gnnpe_load_csr's whole graph) or
 *   the multigraph state.
 *   Device code (csrc/gnnpe_edges_below.hip): the two passes over fixed tiles of 2 048 entries of gnnpe_table_fold, no atomics.  One
 *   lane per entry; the lane of the direction x < y reads the 2 x n_rows cells, the cells at r as gathers of 8 bytes through the
 *   context's reverse positions.  A tile without a selected edge costs the second pass one word.
 * gnnpe_host_csr_edges_below: the host form and the yardstick (host/host_capi.cpp): a plain loop with a binary search for the reverse
 *   entry, on any compact simple CSR.  It shares no code with the device form.  GNNPE_ERR_ARG: a null argument, n_rows == 0, a
 *   neighbour >= n, an entry without its reverse.
 * The consumer is gnnpe_standing_peel of include/gnnpe_online.h.  Out of scope: slab contexts, multigraph rows, a vertex form. */
int gnnpe_host_csr_edges_below(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint64_t *table, uint32_t n_rows,
                               uint64_t threshold, uint32_t *pairs, uint64_t cap, uint64_t *n_selected, uint64_t *min_kept);
int gnnpe_csr_edges_below(gnnpe_ctx *ctx, const void *dev_table, uint32_t n_rows, uint64_t threshold, void *dev_pairs, uint64_t cap,
                          uint64_t *n_selected, uint64_t *min_kept, double *device_ms);

/* ---- vertex relabel on the resident graph -----------------------------------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section and gnnpe_refine_sets_delta_vertices of include/gnnpe_online.h only add
 * symbols.)
 * gnnpe_csr_apply_edges changes the edges and keeps the labels; these calls are the other half: new labels on a few vertices of the
 * whole graph the context holds, from the few bytes that name them, where gnnpe_load_csr uploads every row to change four bytes.
 * It is the middle step of the relabel loop that gnnpe_refine_sets_delta_vertices exists for:
 *     lost = DeltaV(G, C, S);  gnnpe_set_vertex_labels(ctx, S, labels');  gained = DeltaV(G', C', S);  |M'| = |M| - lost + gained.
 *
 * vertices / labels: count uint32 each, label(vertices[i]) becomes labels[i].  The same (vertex, label) pair repeated means it once.
 *
 * Result.  The same rows, with the new labels.  State after a successful call: precisely what gnnpe_load_csr(ctx, n, offsets, nbrs,
 * labels') leaves.  The CSR arrays, the reverse positions and the hub-row list are not touched or rebuilt and the entry indices are
 * unchanged; the neighbours' labels are patched through the reverse positions (one wave per changed vertex, lanes over its row:
 * the copy of v's label in the row of each neighbour u is one word, so two changed neighbours write different words).  The graph
 * generation moves on: open match cursors refuse to go on, and the device tables of ABI 13 / 14 and an entry map end by their own
 * "rows loaded or changed" wording.  Order and slab are reset and everything derived from the rows or the labels is invalidated as
 * the loader invalidates it; in particular the next gnnpe_vde checks the labels against the label table again.
 *
 * Refusals.  Each leaves the context exactly as it was, generation included; all are decided before the first launch.
 *   - GNNPE_ERR_ARG: a null pointer with count > 0; an id >= n; one vertex listed with two different labels.
 *   - GNNPE_ERR_UNSUPPORTED: no whole graph on the device (nothing loaded, or gnnpe_load_rows), or the multigraph state.
 * count == 0 succeeds, launches nothing and changes nothing: the generation stays, cursors stay valid.
 * *device_ms (may be NULL) covers the kernel, not the upload of the two lists.
 * Slab contexts and multigraph rows are out of scope (adding or removing vertices: the next section).
 *
 * gnnpe_labels_download: the labels the context holds, n words -- for a caller without a host mirror.  Whole graph only
 *   (GNNPE_ERR_UNSUPPORTED otherwise). */
int gnnpe_set_vertex_labels(gnnpe_ctx *ctx, const uint32_t *vertices, const uint32_t *labels, uint64_t count, double *device_ms);
int gnnpe_labels_download(gnnpe_ctx *ctx, uint32_t *host_labels);

/* ---- vertex removals and additions on the resident graph ------------------------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section only adds symbols.)
 * The one change the edge batches and the relabel cannot make is to the vertex set: a caller whose graph gains one vertex had to
 * rebuild the whole CSR and call gnnpe_load_csr, losing every per-vertex and per-edge table it keeps on the device.  These calls
 * apply a BATCH of vertex removals R and additions A to the whole graph the context holds, from the few words that describe it.
 *
 * The batch.  remove: n_remove ids of the current graph, a repeated id means the vertex once.  add_labels: the labels of the n_add
 * vertices to add, in order.  Either list may be NULL where its count is 0.
 *
 * Result.  G' has n' = n - |R| + |A| vertices.  A surviving vertex v gets the id v - |{r in R : r < v}|: survivors keep their
 * relative order.  Added vertex i gets the id n - |R| + i, the label add_labels[i] and an EMPTY row; its edges arrive through a
 * following gnnpe_csr_apply_edges, which may name the new ids.  Every edge with an end in R is gone, every other edge stands under
 * the new ids.  G' is the COMPACT CSR that G' alone determines: rows back to back, each strictly ascending; its entry indices are
 * those of gnnpe_csr_download and of the host form.
 *
 * Two maps describe the batch.
 *   - The vertex map: one uint32 per vertex v' of G': the old id of v', or GNNPE_NO_VERTEX for an added vertex.
 *   - The entry map: one uint32 per entry j' of G': the index of that entry in G.  No entry is new, so it never holds
 *     GNNPE_NO_ENTRY; it is strictly increasing, and its image is the entries of G with both ends outside R.
 *
 * gnnpe_host_csr_apply_vertices: the host form and the yardstick (host/graph_update.cpp): a table of new ids, the survivors' rows
 *   copied entry by entry.  It shares no code with the device form.  out_offsets: n' + 1 words; out_labels and vertex_map: n' words
 *   (n - |R| + n_add: the caller knows R); out_nbrs: out_cap words -- too few returns GNNPE_ERR_ARG with *n_after and
 *   *n_entries_after set (offsets[n] entries always suffice).  The same refusals as the device form (no context, so no UNSUPPORTED;
 *   a null output pointer is GNNPE_ERR_ARG); nothing is written on a refusal but the two counts.
 *
 * gnnpe_csr_apply_vertices: the device form (csrc/gnnpe_update_vertices.hip).
 *   State after success: precisely what gnnpe_load_csr(ctx, n', offsets', nbrs', labels') leaves.  The graph generation moves on,
 *   so open match cursors refuse to go on; the reverse positions, the hub-row list and the neighbours' labels are rebuilt by the
 *   loader's own tail; order, slab and everything derived from the rows are reset as the loader resets them; the device tables of
 *   gnnpe_refine_sets_vertex_counts / _edge_counts end by their "rows loaded or changed".
 *   *n_after, *n_entries_before, *n_entries_after (each may be NULL) are set on every return; on a refusal they hold the unchanged
 *   graph's counts.
 *   Maps.  The vertex map is always produced, into a context-owned grow-only buffer; dev_vertex_map may be NULL if the caller does
 *   not want the pointer.  The entry map is produced only where dev_entry_map is not NULL, into the slot of
 *   gnnpe_csr_apply_edges_map: gnnpe_csr_carry_entries then works after this call exactly as after that one.  With dev_entry_map ==
 *   NULL the context is left without a valid entry map, as a plain gnnpe_csr_apply_edges leaves it.  Both maps are valid until the
 *   next gnnpe_csr_apply_vertices (of any batch and any outcome) or any other call that loads or changes the context's rows; the
 *   entry map also ends at the next gnnpe_csr_apply_edges / _map.  On a refusal both pointers are NULL and the maps of an earlier
 *   batch are gone.
 *   The empty batch (n_remove == n_add == 0) succeeds, leaves graph and generation alone (cursors stay valid) and produces identity
 *   maps where maps were asked for, so a caller's loop needs no special case.
 *   Refusals.  Each leaves the context as it was -- the same graph, the same generation (open cursors go on), derived state kept:
 *   the new arrays are built in spare buffers and swapped in only on success.
 *     - GNNPE_ERR_ARG, on the host before anything is launched: a null list with a count > 0, an id >= n, n' == 0.
 *     - GNNPE_ERR_UNSUPPORTED: no whole graph on the device (nothing loaded, or gnnpe_load_rows), or the multigraph state.
 *     - GNNPE_ERR_RANGE: n' >= 2^32 - 1 (on the host before anything is launched), or entries' + n' >= 2^32 (entries' is known
 *       only after the compaction: decided in the call's single wait, with nothing but spare buffers written).
 *     - an allocation the device refuses before the swap returns its error and leaves the context usable and unchanged: whatever
 *       has to grow with n' (start, degree, label, presence and ownership arrays) is allocated aside and swapped in on success.
 *       The rebuild after the swap is gnnpe_load_csr's own tail and fails as that does (see gnnpe_csr_apply_edges).
 *   *device_ms (may be NULL) covers everything between the upload of the two lists and the end of the rebuild, not the uploads.
 *   Transient memory: as gnnpe_csr_apply_edges (the same spare arrays), a spare label array, one flag byte per entry of G.
 *
 * gnnpe_csr_carry_vertices: for r < n_rows and v' < n', dst[r][v'] = src[r][vertex_map[v']], or 0 where the map says
 *   GNNPE_NO_VERTEX, through the context's valid vertex map.  src is row-major n_rows x n, dst row-major n_rows x n', cells of
 *   elem_bytes = 8 (the count tables) or 4; both are the caller's device memory on the context's device, aligned to their cells.
 *   The work runs on the context's stream; every cell of dst is written exactly once, src is not written.  GNNPE_ERR_ARG, with
 *   nothing launched, as gnnpe_csr_carry_entries: the context has no valid vertex map (none was made, the last
 *   gnnpe_csr_apply_vertices was refused, or the rows were loaded or changed since -- a following gnnpe_csr_apply_edges included:
 *   carry the vertex tables before the edges of the new vertices are inserted), elem_bytes is neither 4 nor 8, a pointer is null or
 *   misaligned while there is something to move, or the byte ranges overlap.  n_rows == 0 succeeds and launches nothing.
 *   This is what keeps a gnnpe_refine_sets_vertex_counts table on the device across the batch.
 *
 * The loops, for candidate sets C, C' that agree on the survivors (the caller carries its bitmap columns through the vertex map;
 * DeltaV = gnnpe_refine_sets_delta_vertices, VV / EV its count tables with the caller's table as dev_accum and sign = -1 / +1):
 *   removal:  lost = DeltaV(G, C, R);  VV -= VV(G, C, R);  EV -= EV(G, C, R);  gnnpe_csr_apply_vertices(R);
 *             VV = carry_vertices(VV);  EV = carry_entries(EV);  |M'| = |M| - lost.
 *             By the time of the carry the columns of R and the entries at R hold zero, so dropping them loses nothing.
 *   growth:   gnnpe_csr_apply_vertices(A);  VV = carry_vertices(VV);  EV = carry_entries(EV);  gnnpe_csr_apply_edges_map(I);
 *             EV = carry_entries(EV);  gained = Delta(G', C', I) (gnnpe_refine_sets_delta), its tables added.  An added vertex
 *             without edges matches a single-vertex query only: DeltaV(G', C', A) counts those.
 * Slab contexts and multigraph rows are out of scope. */
#define GNNPE_NO_VERTEX 0xFFFFFFFFu

int gnnpe_host_csr_apply_vertices(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels,
                                  const uint32_t *remove, uint64_t n_remove, const uint32_t *add_labels, uint64_t n_add,
                                  uint32_t *out_offsets, uint32_t *out_nbrs, uint64_t out_cap, uint32_t *out_labels,
                                  uint32_t *vertex_map, uint32_t *n_after, uint64_t *n_entries_after);
int gnnpe_csr_apply_vertices(gnnpe_ctx *ctx, const uint32_t *remove, uint64_t n_remove,
                             const uint32_t *add_labels, uint64_t n_add,
                             uint32_t *n_after, uint64_t *n_entries_before, uint64_t *n_entries_after,
                             void **dev_vertex_map, void **dev_entry_map, double *device_ms);
int gnnpe_csr_carry_vertices(gnnpe_ctx *ctx, uint32_t n_rows, uint32_t elem_bytes,
                             const void *dev_src, void *dev_dst, double *device_ms);

/* ---- halo exchange helpers (device side of the RCCL all-to-all-v) ----------------- */
/* List the vertices whose adjacency rows this context needs but does not hold -- every vertex referenced by
 * a row it holds: after gnnpe_rows_drop_halo these are the neighbours of its slab's start vertices (all that
 * l=2 needs); called again after gnnpe_rows_append they are the rows two hops out (l=3) -- grouped by owning rank: owner r holds the slab
 * [slab_bounds[r], slab_bounds[r+1]) of the processing order.  dev_ids receives the ids (capacity
 * cap entries), host_counts[r] the number per owner.  Ids are ascending inside each group.  A vertex whose row is held
 * is never listed, so host_counts[own rank] = 0 and a second hop asks for nothing the first one brought.  At most 64
 * ranks; slab_bounds must run from 0 to n without a step down (empty slabs own nothing), else GNNPE_ERR_ARG before
 * anything is launched.  More than cap ids: GNNPE_ERR_ARG with the number needed in the message, nothing written. */
int gnnpe_halo_need(gnnpe_ctx *ctx, uint32_t n_ranks, const uint32_t *host_slab_bounds, void *dev_ids,
                    uint64_t cap, uint64_t *host_counts);
/* Degrees of requested rows (rows this context holds): dev_deg[k] = deg(dev_ids[k]). */
int gnnpe_rows_degree(gnnpe_ctx *ctx, uint64_t n_req, const void *dev_ids, void *dev_deg);
/* Pack the adjacency lists of the requested rows back to back into dev_out (sum of degrees entries). */
int gnnpe_rows_pack(gnnpe_ctx *ctx, uint64_t n_req, const void *dev_ids, void *dev_out, uint64_t cap);
/* Install received halo rows: ids, their degrees, and the packed adjacency (all device memory).  min_rank > 0 drops
 * the entries whose neighbour comes before processing position min_rank: a rank whose slab starts there never emits a
 * path that ends on one (kept iff rank[c] > rank[s]), so the LAST hop's halo rows can be truncated (l=2: the only hop;
 * l=3: pass 0 for the first hop).  Rows are validated (ids < n, ascending, no self-loop) and their reverse positions
 * and hub flags built here: the halo is graph structure and stays resident across steps.
 * Refusals (GNNPE_ERR_ARG); after every one of them the context holds exactly the rows it held before the call (this
 * covers the refusals only: after GNNPE_ERR_HIP the halo is unspecified -- gnnpe_rows_drop_halo, or load again):
 *   - dev_ids[k] >= n, or a vertex whose row the context already holds, owned or halo (with min_rank > 0 a second copy
 *     would truncate an owned row and paths would go missing): found on the device before anything is installed, the
 *     message names the position and the vertex.  An id given TWICE INSIDE ONE CALL is not looked for (that would take
 *     a second pass over the ids): the caller passes distinct ids, as gnnpe_halo_need lists them.
 *   - the degrees do not sum to n_nbrs; the neighbour buffer is full; min_rank > 0 before gnnpe_set_order; a context
 *     loaded by gnnpe_load_csr; more rows than vertices.
 *   - a row that is not a strictly ascending list of ids < n without the vertex itself: found when the rows are
 *     validated after the install, the message names the vertex, and ALL rows of the call are taken out again.  The
 *     caller may append corrected rows, or gnnpe_rows_drop_halo and repeat the exchange. */
int gnnpe_rows_append(gnnpe_ctx *ctx, uint64_t n_rows, const void *dev_ids, const void *dev_deg,
                      const void *dev_nbrs, uint64_t n_nbrs, uint32_t min_rank);

/* What the context holds: adjacency rows (own + halo), their neighbour entries (halo rows count as installed, i.e.
 * after truncation), rows longer than 64 entries.  Any output may be NULL. */
int gnnpe_rows_held(gnnpe_ctx *ctx, uint64_t *n_rows, uint64_t *n_entries, uint32_t *n_hub_rows);

/* Forget every appended halo row (back to the state right after gnnpe_load_rows), so the exchange
 * can be repeated. */
int gnnpe_rows_drop_halo(gnnpe_ctx *ctx);

/* ---- R4: vertex embedding (gen_vde, custom.h:513-544) ------------------------------------------ */
/* x = table[label], nx = sum of neighbours' x in ascending-neighbour order from 0.0 (bit-identical
 * to the reference's loop :527-534), vde = x + nx.  Computed for the rows this context holds
 * adjacency for (all vertices after gnnpe_load_csr; the slab rows after gnnpe_load_rows).  Any of
 * the host outputs (n x e doubles each, indexed by vertex id) may be NULL. */
int gnnpe_vde(gnnpe_ctx *ctx, double *host_x, double *host_nx, double *host_vde);
/* Device-resident vde table (n x e doubles, vertex-id indexed) for exchange between ranks. */
int gnnpe_vde_device_ptr(gnnpe_ctx *ctx, void **dev_vde, void **dev_x);
/* Gather / scatter slab rows of the vde table to/from a packed buffer of (end-begin) x e doubles in
 * processing order -- the all-gather payload (x needs no exchange: labels are replicated). */
int gnnpe_vde_pack_slab(gnnpe_ctx *ctx, uint32_t begin, uint32_t end, void *dev_buf);
int gnnpe_vde_unpack_slab(gnnpe_ctx *ctx, uint32_t begin, uint32_t end, const void *dev_buf);
/* The same for every rank's slab at once, from the all-gathered buffer [n_ranks][stride rows][e] (stride = the longest
 * slab; bounds[n_ranks + 1] host words, the slabs' first positions): one launch per step instead of n_ranks - 1.  The
 * rows of skip_rank (this rank's own: already in the table) are left alone; pass n_ranks to scatter all. */
int gnnpe_vde_unpack_all(gnnpe_ctx *ctx, uint32_t n_ranks, const uint32_t *bounds, uint32_t stride, uint32_t skip_rank,
                         const void *dev_buf);

/* ---- R2: path enumeration (dfs + VectorHash, custom.h:52-92; driver loop main.cpp:87-96) ------- */
/* Counts the paths of the context's slab with l edges (l+1 vertices).  l=2 is the reference's path (it
 * only works for l=2); l=3 is the same rule with the DFS depth fixed (4-vertex simple paths,
 * kept iff rank[last] > rank[first]; BASELINE config 5) and needs the adjacency rows two hops from the
 * slab on the device.  host_per_start[i] (slab length entries, may be NULL) = number of paths whose
 * start is sorted_nodes[slab_begin+i]; *host_total = their sum.  Leaves the scanned offsets on the
 * device for gnnpe_fill_paths*. */
int gnnpe_count_paths(gnnpe_ctx *ctx, uint32_t l, uint64_t *host_per_start, uint64_t *host_total);
/* The same count (l=2, the default rank-sorted enumeration) ENQUEUED only: no read-back, no host synchronisation; the
 * total stays in device memory.  For a step of a multi-GPU build (main.cpp:87-96 across devices) whose outputs were
 * sized by an earlier pass: count_enqueue -> gnnpe_count_total_device (the word a collective sends) ->
 * gnnpe_fill_paths_capped_device, with nothing on the host between the launches.  gnnpe_count_total fetches the
 * number whenever the host wants it (synchronises); every entry point that needs it on the host does so itself. */
int gnnpe_count_paths_enqueue(gnnpe_ctx *ctx, uint32_t l);
int gnnpe_count_total(gnnpe_ctx *ctx, uint64_t *host_total);
/* Copies the last count's total (one uint64) to caller-owned device memory on the context's stream. */
int gnnpe_count_total_device(gnnpe_ctx *ctx, void *dev_u64);

/* ---- R2 + R5: emit paths and their embeddings (gen_pde, custom.h:546-572) ----------------------- */
/* Emits the slab-local paths [begin, end) in the reference's order (start vertices in processing
 * order, neighbours ascending, reverse-dedup): vids (end-begin) x (l+1) uint32; pde = concat of
 * vde rows, pde_label = concat of x rows, (end-begin) x e(l+1) doubles each.  Any output may be
 * NULL.  The *_device form writes device memory and only enqueues work on the stream. */
int gnnpe_fill_paths(gnnpe_ctx *ctx, uint64_t begin, uint64_t end, uint32_t *host_vids, double *host_pde,
                     double *host_pde_label);
int gnnpe_fill_paths_device(gnnpe_ctx *ctx, uint64_t begin, uint64_t end, void *dev_vids, void *dev_pde,
                            void *dev_pde_label);
/* Emits rows [0, min(total, cap_rows)) into buffers of cap_rows rows without the host knowing the total (after
 * gnnpe_count_paths_enqueue): the kernel clips against the per-start output ranges, so nothing is written beyond
 * cap_rows.  ids and pde only (either may be NULL). */
int gnnpe_fill_paths_capped_device(gnnpe_ctx *ctx, uint64_t cap_rows, void *dev_vids, void *dev_pde);

/* ---- output pool: where the emitted rows live on the device -------------------------------------------------------
 * The reference keeps `all_paths` / `pde` in host vectors (main.cpp:87-96, custom.h:546-572); here they are device
 * buffers, and on MI355X the rate a kernel streams into a multi-GiB buffer differs by up to 25 % between allocations
 * (stable for the life of a buffer, not predictable from its address: scripts/vmm_probe*.hip).
 * A pool draws `candidates` independent allocations for rows_cap rows (ids: rows_cap x L uint32; pde: rows_cap x D
 * doubles, D = 0 for none), times the consumer in each -- the emit kernel itself when the context holds an l = L-1
 * count of at most rows_cap paths (call gnnpe_count_paths first), a streaming write otherwise -- keeps the fastest and
 * frees the others before it returns (transient memory: candidates x the output size, bounded by the free memory).
 * candidates = 1 takes what comes, unprobed.  The buffers stay valid until gnnpe_output_pool_destroy.
 * With an l = 2 count on the context the pool also runs gnnpe_emit_calibrate_device on the buffer it keeps (nine launches
 * of the emit kernels): pass candidates | GNNPE_POOL_NO_CALIBRATION where the buffer is filled once or twice (a CLI that
 * fills it once per chunk), so that the launches that choose a shape do not outnumber the ones that use it. */
#define GNNPE_POOL_NO_CALIBRATION 0x80000000u
typedef struct gnnpe_pool gnnpe_pool;
int gnnpe_output_pool_create(gnnpe_ctx *ctx, uint64_t rows_cap, uint32_t L, uint32_t D, uint32_t candidates, gnnpe_pool **pool);
int gnnpe_output_pool_acquire(gnnpe_pool *pool, void **dev_ids, void **dev_pde, uint64_t *rows_cap);
/* probe_ms[0 .. min(cap, candidates drawn)) = time of the probe in every candidate, *kept = the one in use,
 * *probed_with_emit_kernel = 1 if the probe was the emit kernel (0: streaming write, or a single unprobed candidate). */
int gnnpe_output_pool_report(gnnpe_pool *pool, uint32_t cap, float *probe_ms, uint32_t *n_candidates, uint32_t *kept,
                             int *probed_with_emit_kernel);
void gnnpe_output_pool_destroy(gnnpe_pool *pool);

/* Order-sensitive 64-bit checksum of n_rows emitted rows (n_rows x L uint32 on the device) whose first
 * row has global path id first_id; checksums of consecutive chunks ADD (mod 2^64).  For outputs too large
 * to keep (config 5: count + checksum only) and for comparing rank counts. */
int gnnpe_rows_checksum_device(gnnpe_ctx *ctx, uint64_t n_rows, uint32_t L, const void *dev_ids, uint64_t first_id,
                               uint64_t *host_sum);

/* Per path, the partition of its start vertex (membership[vids[0]]): what main.cpp:98-108 groups
 * partition_paths.txt by.  dev_part: (end-begin) uint32. */
int gnnpe_path_partitions_device(gnnpe_ctx *ctx, uint64_t begin, uint64_t end, void *dev_part);

/* ---- R7: text rendering of the offline outputs (writers, main.cpp:98-119) ------------------------ */
/* all_paths.txt body: each row "<v0> <v1> <v2> \n" -- every id followed by one space, then '\n'
 * (main.cpp:114-118).  dev_vids: n_rows x L uint32.  dev_text == NULL only sizes (*nbytes). */
int gnnpe_text_paths(gnnpe_ctx *ctx, uint64_t n_rows, uint32_t L, const void *dev_vids, void *dev_text, uint64_t cap,
                     uint64_t *nbytes);
/* partition_paths.txt body: one uint64 id per line (main.cpp:102-106). */
int gnnpe_text_ids(gnnpe_ctx *ctx, uint64_t n, const void *dev_ids, void *dev_text, uint64_t cap, uint64_t *nbytes);
/* Global ids (id_base + i, ascending) of the rows i < n whose partition dev_part[i] == pid: the list
 * main.cpp:98-108 writes for partition pid.  dev_ids: room for n uint64. */
int gnnpe_select_partition(gnnpe_ctx *ctx, uint64_t n, const void *dev_part, uint32_t pid, uint64_t id_base,
                           void *dev_ids, uint64_t *count);

/* ---- R6: index.dat (Partition ctor build loop custom.h:235-257 -> RTree::insert rtree.cpp:198-284) -- */
/* Bulk-loads the R-tree over `cnt` paths given as vertex tuples (cnt x L uint32, device memory, in the
 * partition's path order: leaf `son` = row index, custom.h:243) with point MBRs lo = hi = pde row
 * (custom.h:244-248), and assembles the complete file image in the reference's block format in device
 * memory owned by the context (valid until the next call).  hdr_out = {blocklength, node blocks, dim,
 * num_data, leaf nodes, internal nodes, root_is_data, root}.  Tree shape differs from the reference's
 * insertion-built tree (it is not reproducible even by the reference); every consumer
 * constraint of the online code holds (dense block ids, internal root, enclosing MBRs). */
int gnnpe_build_index_device(gnnpe_ctx *ctx, uint64_t cnt, uint32_t L, const void *dev_vids, void **dev_image,
                             uint64_t *nbytes, int32_t hdr_out[8]);
/* The image of partition `pid` straight from the enumeration state of the context (after gnnpe_vde + gnnpe_count_paths):
 * no tuple array.  For an l = 2 count the tree is built pair-major -- the (s, b) pairs (hub pairs: their 64-entry units)
 * are sorted by [label(s) | label(b) | z-order of vde[s], vde[b]] and the leaves read their points out of the pairs' row
 * blocks; for an l = 3 count triple-major (round 6, csrc/gnnpe_index_deep.hip.h) -- the (s, b, c) triples x 64-entry pieces of
 * c's row, each with the mask of its kept fourth vertices, sorted by [label(s) | label(b) | label(c) | z-order of their vde] --
 * otherwise (embedding widths without a specialised enumeration) the partition's tuples are collected and handed to
 * gnnpe_build_index_device.  Same file format, same
 * consumer constraints; the image stays valid until the next index call on the context. */
int gnnpe_build_index_partition_device(gnnpe_ctx *ctx, uint32_t pid, void **dev_image, uint64_t *nbytes, int32_t hdr_out[8]);
/* The same image together with the tree's auxiliary index (Partition::build_auxiliary_index, custom.h:268-364: per node
 * block key, degrees[L], label_mbr[2D]; layout as gnnpe_aux_index_device).  For the pair-major build (l = 2, whole graph
 * or gnnpe_set_degrees) the leaf kernel computes the leaves' rows while it assembles them and only the few upper levels
 * are a separate pass; otherwise the generic pass over the finished image runs.  Arrays are context-owned. */
int gnnpe_build_index_partition_aux_device(gnnpe_ctx *ctx, uint32_t pid, void **dev_image, uint64_t *nbytes, int32_t hdr_out[8],
                                           void **dev_key, void **dev_degrees, void **dev_label_mbr, uint32_t *n_nodes);
/* Whole job for partition `pid` of the context's slab: build (gnnpe_build_index_partition_device), write `path`
 * (<f>gnn-pe/partitions/partition-<pid>/index.dat).  The reference online run then skips its insert
 * loop (custom.h:222-235 only tests that the file exists). */
int gnnpe_build_index(gnnpe_ctx *ctx, uint32_t pid, const char *path);
/* index.dat of partitions 0..n_parts-1, all at once: every image is built on the device first, then the files are
 * written side by side (one writer thread per file: buffered writes to one file serialise, writes to different files do
 * not).  Same files as n_parts calls of gnnpe_build_index; aux_paths (or NULL): where to leave every partition's
 * auxiliary index (gnnpe_build_aux_index below). */
int gnnpe_build_index_files(gnnpe_ctx *ctx, uint32_t n_parts, const char *const *paths, const char *const *aux_paths);

/* Pieces for callers that assemble a partition's tuples themselves (multi-GPU host: the tuples of partition pid come
 * from every rank): rows of dev_rows (k x L uint32 selected by the global ids dev_sel[i] - sel_base) -> dev_out; and a
 * device buffer written to a file through pinned staging buffers (copy-back overlapped with the writes). */
int gnnpe_gather_rows_device(gnnpe_ctx *ctx, uint64_t k, uint32_t L, const void *dev_sel, uint64_t sel_base,
                             const void *dev_rows, void *dev_out);
int gnnpe_write_device_file(gnnpe_ctx *ctx, const void *dev_src, uint64_t nbytes, const char *path);

/* Same file format over explicit rectangles: cnt x 2*dim doubles (lo0, hi0, lo1, hi1, ...), son = row. */
int gnnpe_build_box_index_device(gnnpe_ctx *ctx, uint64_t cnt, uint32_t dim, const void *dev_boxes, void **dev_image,
                                 uint64_t *nbytes, int32_t hdr_out[8]);

/* ---- GNN-PGE offline (GNN-PGE/src/main.cpp:91-195) ------------------------- */
/* path_group / path_label_group of every vertex: per-dimension [min, max] over the embeddings
 * [vde[v], vde[u]] / [x[v], x[u]] of its 1-hop paths (v, u); n x 4e doubles each, laid out
 * (lo0, hi0, lo1, hi1, ...).  Needs gnnpe_vde.  Host outputs may be NULL. */
int gnnpe_pge_groups(gnnpe_ctx *ctx, double *host_path_group, double *host_path_label_group);
/* Device addresses of the two arrays gnnpe_pge_groups computed (n x 4e doubles each; vertex-id indexed): what a caller that
 * keeps working on the device reads instead of the host copies (GNN-PGE/src/main.cpp:141-176 fills the same values). */
int gnnpe_pge_device_ptr(gnnpe_ctx *ctx, void **dev_path_group, void **dev_path_label_group);
/* R-tree of one GNN-PGE partition (GNN-PGE/include/custom.h:141-195): entry i = path_group of
 * host_vertices[i] (the partition's vertices in membership.txt order), son = i; written to `path`
 * (<f>gnn-pge/partitions/partition-i/index.dat). */
int gnnpe_pge_build_index(gnnpe_ctx *ctx, uint64_t n_sel, const uint32_t *host_vertices, const char *path);

/* ---- GNN-PGE online: the filter (GNN-PGE/src/main.cpp:197-361, custom.h:292-480) --------------------------------- */
/* Query side (host, no GPU): gen_vde of the query graph, then per query vertex u the per-dimension [lo, hi] of the
 * embeddings [vde[u], vde[w]] (path_group) and [x[u], x[w]] (path_label_group) over its 1-hop paths (u, w)
 * (main.cpp:253-329): labels / degrees (n_query_vertices uint32) and pg / plg (n_query_vertices x 4e doubles, laid out
 * like gnnpe_pge_groups), malloc'ed (gnnpe_host_free).  A query vertex without an edge has no group in the reference
 * (its leaf test would read an empty vector): such a query is refused with GNNPE_ERR_UNSUPPORTED, the vertex named. */
int gnnpe_host_pge_query_groups(const char *query_graph_path, uint32_t e, uint32_t *n_query_vertices, uint32_t **labels,
                                uint32_t **degrees, double **path_group, double **path_label_group);
/* Installs path groups read back from <f>gnn-pge/data_vertices.bin (n x 4e doubles each, vertex-id indexed) instead of
 * computing them: the alternative to gnnpe_vde + gnnpe_pge_groups.  Call order: gnnpe_load_csr, gnnpe_set_label_table
 * (it fixes e), then this; a later load or gnnpe_pge_groups replaces the groups. */
int gnnpe_pge_set_groups(gnnpe_ctx *ctx, const double *host_path_group, const double *host_path_label_group);
/* Data side (device): Partition::query of every partition at once.  The R-tree walk only prunes; its result is the leaf
 * test (custom.h:327-374) applied to every data vertex, which is what this does: v is a candidate of query vertex u iff
 * deg(u) <= deg(v), label(u) == label(v), and for every k < 2e  plg_v[2k+1] >= plg_u[2k], plg_v[2k] <= plg_u[2k+1] and
 * pg_v[2k+1] >= pg_u[2k] -- exact fp64 comparisons, inclusive bounds, no epsilon.  Needs the whole graph (gnnpe_load_csr)
 * and the groups (gnnpe_pge_groups or gnnpe_pge_set_groups).  q_pg / q_plg: n_query_vertices x 4e doubles as
 * gnnpe_host_pge_query_groups returns them.  host_bitmap: n_query_vertices x ceil(n/32) uint32, the layout of
 * gnnpe_filter_candidates (gnnpe_refine takes it unchanged).  device_ms (may be NULL): time on the device. */
int gnnpe_pge_filter_candidates(gnnpe_ctx *ctx, uint32_t n_query_vertices, const uint32_t *q_labels, const uint32_t *q_degrees,
                                const double *q_path_group, const double *q_path_label_group, uint32_t *host_bitmap,
                                double *device_ms);

/* ---- the online filter ------------------------------------------------------------ */
/* Query side (host): what main.cpp:136-151 does to the query graph before it touches the index -- dfs_query
 * (custom.h:94-119), gen_vde, gen_query_pde (custom.h:574-631: paths sorted by degree weight, greedy vertex
 * cover).  Returns the plan's paths: vids / labels / degrees (n_paths x 3 uint32) and pde (n_paths x 3e doubles),
 * malloc'ed (gnnpe_host_free). */
int gnnpe_host_query_plan(const char *query_graph_path, uint32_t e, uint32_t *n_query_vertices, uint32_t *n_paths,
                          uint32_t **vids, uint32_t **labels, uint32_t **degrees, double **pde);
/* Data side (device): Partition::query (custom.h:366-489) for all partitions at once.  The R-tree traversal only
 * prunes; its result is its leaf test (custom.h:404-431) applied to every data path, which is what this does, fused
 * with the enumeration of the context's slab (gnnpe_set_order + gnnpe_vde first; no counts, no emitted paths; a
 * slab-only context also needs gnnpe_set_degrees and its halo rows).  host_bitmap:
 * n_query_vertices x ceil(n/32) uint32, bit v of row u = data vertex v is a candidate of query vertex u -- the
 * reference's candidate_set (main.cpp:165-171), ready for its refinement.  device_ms (may be NULL): time on the device. */
/* A context that holds only a slab's rows (gnnpe_load_rows) filters its own paths once it knows the degree of every
 * vertex (n uint32; the ranks' bitmaps are then OR-ed, dist.py).  Not needed after gnnpe_load_csr. */
int gnnpe_set_degrees(gnnpe_ctx *ctx, const uint32_t *host_degrees);
int gnnpe_filter_candidates(gnnpe_ctx *ctx, uint32_t n_paths, const uint32_t *q_vids, const uint32_t *q_labels,
                            const uint32_t *q_degrees, const double *q_pde, uint32_t n_query_vertices, double epsilon,
                            uint32_t *host_bitmap, double *device_ms);

/* ---- exact online queries (INTEGRATION.md "Exact mode") ---------------------------------------------------------------- */
/* The reference keeps every path in one orientation on both sides and compares position by position, so its candidate sets can
 * miss the image of a query vertex.  Exact mode tests every plan path in both orientations: for every embedding f, f(u) is in
 * the candidate set of u, and the refinement on these sets counts every embedding.  l = 3 (4-vertex plan paths) is exact only.
 * Query side (host): the exact plan, three parts concatenated in every output array --
 *   counts[0] paths of l + 1 vertices: l = 2 the reference's plan (gnnpe_host_query_plan); l = 3 every simple 4-vertex query
 *             path (dfs_query at depth 3), by degree weight descending (stable), taken while it covers a new vertex;
 *   counts[1] l = 3 only: 3-vertex paths of the reference's plan, in its order, for the vertices no 4-vertex path covers;
 *   counts[2] the query vertices still uncovered, one entry each (tested alone: label, degree, vde).
 * vids / labels / degrees: (l + 1) counts[0] + 3 counts[1] + counts[2] uint32; pde: e doubles per entry (the vde of the entry's
 * query vertex).  Each path is listed once; the filter adds the reverses.  malloc'ed (gnnpe_host_free). */
int gnnpe_host_query_plan_exact(const char *query_graph_path, uint32_t e, uint32_t l, uint32_t *n_query_vertices,
                                uint32_t counts[3], uint32_t **vids, uint32_t **labels, uint32_t **degrees, double **pde);
/* Data side (device): the plan of gnnpe_host_query_plan_exact, every path doubled with its reverse inside the library (at most
 * 512 paths per width after doubling, else GNNPE_ERR_UNSUPPORTED); the leaf test of gnnpe_filter_candidates over the
 * enumeration of the context's slab for each width, and label / degree / vde for the single vertices (the slab's own
 * vertices).  Same requirements as gnnpe_filter_candidates.  A slab-only context at l = 3 also needs the rows two hops out
 * (gnnpe_halo_need after the first gnnpe_rows_append) AND the vde of every vertex three hops out -- the fourth vertex of a
 * path; gnnpe_vde computes it for the rows the context holds only, so install the all-gathered table (gnnpe_vde_unpack_all, as
 * dist.py does) or hold those rows too.  Nothing checks this: a missing vde reads as zeros and drops candidates.
 * host_bitmap: the layout gnnpe_refine takes. */
int gnnpe_filter_candidates_exact(gnnpe_ctx *ctx, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                                  const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                                  uint32_t n_query_vertices, double epsilon, uint32_t *host_bitmap, double *device_ms);

/* ---- filter support tables: exact candidate sets kept current across updates ------------------------------------------------------
 * (Headed by name: GNNPE_ABI_VERSION stays 20, this section only adds symbols.)
 * The exact candidate set is a union over passing data paths and cannot be patched bit by bit: a deletion may remove the last path
 * that supported a bit.  The number of supporting paths can be patched, and the paths whose status an update changes lie within l
 * hops of the batch.  These calls keep that number -- the support table S of the exact filter -- and derive the bitmap from it, so
 * that a standing exact query pays neither gnnpe_set_order nor a whole-graph gnnpe_filter_candidates_exact per batch.
 *
 * Definitions.  The plan is what gnnpe_host_query_plan_exact returns: parts main (width W = l + 1), tri (width 3, l = 3 only) and
 * single, each path listed once.  S[u][v] is a uint64 cell of a table of n_query_vertices rows by n columns, row-major, in the
 * CALLER's device memory; it is the sum of
 *   - over the plan paths q of main and tri and the positions j with q.vids[j] == u: the number of DIRECTED simple data paths P of
 *     q's width that pass q position by position with P[j] == v.  "Pass" is the leaf test of gnnpe_filter_candidates: labels equal,
 *     query degree <= data degree, in no dimension q > d && |q - d| > epsilon;
 *   - over the single entries with vid u: 1 if v passes the same three tests alone.
 * Counting directed paths against the plan as listed equals counting every undirected path in one orientation against the plan
 * doubled with its reverses, which is what the filter kernels do: S[u][v] != 0 exactly where gnnpe_filter_candidates_exact sets bit
 * v of row u.  The table depends on no processing order: none of these calls needs gnnpe_set_order, and none uses a slab.
 * S_T, for a vertex set T, is the same sum over the paths that contain at least one vertex of T, each counted once, and over the
 * singles with v in T.  S_V = S.  (Each once: a path is charged to the smallest position j with P[j] in T; a work item (t, j) walks
 * the paths with P[j] = t, any vertex to the right of j, only vertices outside T to the left -- csrc/gnnpe_filter_support.hip.)
 *
 * gnnpe_filter_support_exact: dev_table = S(G), overwritten.
 * gnnpe_filter_support_exact_delta: dev_table += sign * S_T(G) with T = vertices (n_vertices ids < n; a repeated id means the vertex
 *   once).  sign is +1 or -1; the subtraction is the wrapping 64-bit add, as in the count tables of ABI 17.  n_vertices == 0 succeeds,
 *   launches nothing and leaves the table's bytes alone.
 * gnnpe_filter_support_bitmap: host_bitmap (n_query_vertices x ceil(n/32) uint32, the layout gnnpe_filter_candidates and every
 *   refinement call take) with bit v of row u set where S[u][v] != 0.
 * *device_ms (may be NULL): the time on the device, the plan's upload excluded.  Each call waits for the device once; nothing per
 * path leaves the device.
 *
 * Requirements: the whole graph on the device (gnnpe_load_csr state), a label table, and gnnpe_vde since the last change of the rows
 * or the labels.  Refusals, all on the host before any launch, each leaving the context and the table untouched:
 *   - the plan checks of gnnpe_filter_candidates_exact, the limit of 512 paths per width after doubling included
 *     (GNNPE_ERR_UNSUPPORTED);
 *   - GNNPE_ERR_ARG: a null or not 8-byte aligned dev_table, a sign other than +1 / -1, an id >= n, a null list with a count > 0;
 *   - GNNPE_ERR_UNSUPPORTED: a slab-only context (gnnpe_load_rows) or the multigraph state;
 *   - GNNPE_ERR_ARG naming gnnpe_vde where the embeddings are missing or stale: what catches a caller who forgot it after an update.
 *
 * The loops.  A, R and N as above; every update call resets gnnpe_vde, which the next support call asks for.
 *   Edges, batch B = I u D, T = the end vertices of B:
 *       S -= S_T(G);  gnnpe_csr_apply_edges(B);  gnnpe_vde;  S += S_T(G');  C' = bitmap(S)
 *     Degree and vde change only at the ends of B, and a path with a changed edge contains both of its ends: every path whose
 *     existence or test result changes contains a vertex of T.
 *   Relabel of R: the same with gnnpe_set_vertex_labels and T = R u N(R) -- the vde of a neighbour changes too.
 *   Vertex batch removing R and adding A:
 *       S -= S_T(G), T = R u N_G(R);  gnnpe_csr_apply_vertices;  gnnpe_csr_carry_vertices(n_rows = n_query_vertices, elem_bytes = 8);
 *       gnnpe_vde;  S += S_T'(G'), T' = the new ids of N_G(R) \ R together with the added vertices
 *     After the subtraction the columns of R hold zero, so dropping them in the carry loses nothing; an added vertex has an empty
 *     row and can still pass a single-vertex test.
 * Not here: slab contexts, multigraph rows, the reference-mode filter, a plan handle that would save the upload per call. */
int gnnpe_filter_support_exact(gnnpe_ctx *ctx, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                               const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                               uint32_t n_query_vertices, double epsilon, void *dev_table, double *device_ms);
int gnnpe_filter_support_exact_delta(gnnpe_ctx *ctx, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                                     const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                                     uint32_t n_query_vertices, double epsilon, const uint32_t *vertices, uint64_t n_vertices,
                                     int sign, void *dev_table, double *device_ms);
int gnnpe_filter_support_bitmap(gnnpe_ctx *ctx, uint32_t n_query_vertices, const void *dev_table, uint32_t *host_bitmap,
                                double *device_ms);
/* gnnpe_filter_support_bitmap_device (headed by name, GNNPE_ABI_VERSION stays 20): the kernel of gnnpe_filter_support_bitmap into
 * the CALLER's device buffer dev_bitmap (n_query_vertices x ceil(n/32) uint32, 4-byte aligned), on the context's stream.  Every word
 * of every row is written; the bits at positions >= n of a row's last word are zero.  Nothing comes to the host and the call waits
 * for nothing -- what follows on the context's stream sees the bitmap -- unless device_ms is given: the two events of a timed call
 * are waited for.  Requirements and refusals as gnnpe_filter_support_bitmap.  The consumer is the standing exact query of
 * include/gnnpe_online.h (gnnpe_standing_open), whose candidate sets never leave the device. */
int gnnpe_filter_support_bitmap_device(gnnpe_ctx *ctx, uint32_t n_query_vertices, const void *dev_table, void *dev_bitmap,
                                       double *device_ms);

/* ---- touched sets on the device (headed by name, GNNPE_ABI_VERSION stays 20: symbols are added) ----------------------------------
 * The relabel loop and the vertex-batch loop above need T = R u N_G(R) and T' = the new ids of T's survivors with the added
 * vertices.  A caller with a host copy of the rows builds them there; these three make and use them on the device, from the
 * resident rows and the resident vertex map, so that nothing proportional to n or m crosses to the host per batch
 * (csrc/gnnpe_touched.hip).  A set has two forms, both in the CALLER's device memory on the context's device: a bitmap of ceil(n/32)
 * uint32 (every word written, the bits at and above n zero) and its ascending ids.
 *
 * gnnpe_csr_closed_neighbourhood: T = R u N_G(R) for R = vertices (n_vertices ids < n; a repeated id means the vertex once) into
 *   dev_bits and dev_ids (room for ids_cap ids), *n_ids = |T|.  One wave per vertex of R marks its row with atomicOr into the zeroed
 *   bitmap; the ids come from the ordered compaction of the bitmap.  If ids_cap < |T| the call returns GNNPE_ERR_ARG with *n_ids set
 *   and the bitmap written; of the ids only the first ids_cap are.  n_vertices == 0 gives the empty set.  Refused before any launch:
 *   an id >= n, a null list with a count > 0, a null or misaligned pointer (GNNPE_ERR_ARG); a slab context or the multigraph state
 *   (GNNPE_ERR_UNSUPPORTED).  One host wait, for the count.
 * gnnpe_csr_carry_vertex_set: a set of G through the context's valid vertex map.  Bit v' of dev_bits_new (ceil(n'/32) words) is
 *   set where vertex_map[v'] is a vertex of dev_bits_old (ceil(n/32) words) and, with with_added != 0, where the map says
 *   GNNPE_NO_VERTEX.  One lane per vertex of G', the wave's answers one ballot stored as two words: no atomics.  ids_cap, *n_ids and
 *   the wait as above.  Without a valid vertex map it is refused as gnnpe_csr_carry_vertices is (a following gnnpe_csr_apply_edges
 *   ends the map); the two bitmaps must not overlap.
 * gnnpe_filter_support_exact_delta_device: gnnpe_filter_support_exact_delta with T taken from dev_bits and dev_ids (n_ids ascending
 *   ids, each < n, each once, the bitmap holding exactly them: the caller's promise, which the two calls above keep).  It makes that
 *   call's launches without the host sort, the upload and the scatter of the list -- the two share their body -- so for the same T
 *   the two leave byte-equal tables.  n_ids == 0 succeeds and launches nothing.  Requirements and refusals as the host-list call.
 * *device_ms (may be NULL): the time on the device between the uploads and the wait. */
int gnnpe_csr_closed_neighbourhood(gnnpe_ctx *ctx, const uint32_t *vertices, uint64_t n_vertices, void *dev_bits, void *dev_ids,
                                   uint64_t ids_cap, uint64_t *n_ids, double *device_ms);
int gnnpe_csr_carry_vertex_set(gnnpe_ctx *ctx, const void *dev_bits_old, int with_added, void *dev_bits_new, void *dev_ids,
                               uint64_t ids_cap, uint64_t *n_ids, double *device_ms);
int gnnpe_filter_support_exact_delta_device(gnnpe_ctx *ctx, uint32_t l, const uint32_t counts[3], const uint32_t *q_vids,
                                            const uint32_t *q_labels, const uint32_t *q_degrees, const double *q_pde,
                                            uint32_t n_query_vertices, double epsilon, const void *dev_bits, const void *dev_ids,
                                            uint64_t n_ids, int sign, void *dev_table, double *device_ms);

/* The refinement half of the reference's online step (custom.h:634-932) is outside SURVEY section 8's scope (frozen since round 1)
 * and ships in a library of its own since round 6: include/gnnpe_online.h, libgnnpe_online.so (gnnpe_refine, gnnpe_host_refine). */

/* ---- the online side's data load ------------------------------------------------------- */
/* `gnnpe_main --sidecars` leaves <f>gnn-pe/paths.bin (magic "GNNPEPTH", uint32 version = 1, uint32 L, uint64 P, then the
 * P x L uint32 rows of all_paths.txt) and <f>gnn-pe/vde.bin (uint32 n, e; x, nx, vde: n x e doubles each).  This returns
 * what gen_pde (custom.h:546-572) builds by re-parsing the text -- per path vids / labels / degrees (P x L uint32) and
 * pde / pde_label (P x L*e doubles; labels[] and degrees[] are the graph's, `vertices[vid].label/.degree`) -- as flat
 * malloc'ed arrays (gnnpe_host_free).  Host only, no GPU.  gnnpe_host_write_paths_header writes the 24-byte header to an
 * open FILE* (the writer side, used by the CLI). */
int gnnpe_host_load_path_sidecar(const char *paths_bin, const char *vde_bin, uint32_t n, const uint32_t *labels,
                                 const uint32_t *degrees, uint64_t *n_paths, uint32_t *L, uint32_t *e, uint32_t **vids,
                                 uint32_t **path_labels, uint32_t **path_degrees, double **pde, double **pde_label);
int gnnpe_host_write_paths_header(void *file, uint32_t L, uint64_t n_paths);

/* The partition's copy of the paths -- the loop of Partition::Partition (custom.h:205-216: `paths.push_back(
 * data_paths[path_id])` for every id of partition_paths.txt): the same arrays as gnnpe_host_load_path_sidecar, but
 * only the rows of one partition, in the order of its partition_paths.txt (`path_ids`, also returned), i.e. indexed by
 * what the leaf entries of that partition's index.dat carry in `son` (custom.h:243). */
int gnnpe_host_load_partition_sidecar(const char *paths_bin, const char *vde_bin, const char *partition_paths_txt, uint32_t n,
                                      const uint32_t *labels, const uint32_t *degrees, uint64_t *n_paths, uint32_t *L,
                                      uint32_t *e, uint32_t **path_ids, uint32_t **vids, uint32_t **path_labels,
                                      uint32_t **path_degrees, double **pde, double **pde_label);

/* The auxiliary index of a partition's R-tree -- Partition::build_auxiliary_index (custom.h:268-364), which the
 * reference recomputes on every start of `-m online` by walking the tree block by block: per node block id,
 * degrees[L] (largest degree per path position below the node), label_mbr[2D] (lo0, hi0, lo1, hi1, ... of pde_label
 * below the node) and key = 0 - hi_0 - ... - hi_{D-1} of the node's entry in its parent (0 for the root).
 * gnnpe_aux_index_device: bottom-up pass over ANY index.dat image in device memory (bulk-loaded here or written by the
 * reference's insert loop); dev_tuples = the partition's paths, [cnt x L] uint32 vertex ids in partition order (what
 * the leaf entries' `son` index).  Needs the graph, the label table and gnnpe_vde in the context.  Outputs are
 * context-owned device arrays (valid until the next call): key double[n_nodes], degrees uint32[n_nodes x L], label_mbr
 * double[n_nodes x 2D]. */
int gnnpe_aux_index_device(gnnpe_ctx *ctx, const void *dev_image, uint64_t nbytes, uint64_t cnt, uint32_t L,
                           const void *dev_tuples, void **dev_key, void **dev_degrees, void **dev_label_mbr,
                           uint32_t *n_nodes, uint32_t *dim);
/* Partition pid of the current count: its index image (the one gnnpe_build_index just built, or a fresh build), its
 * auxiliary index, written to `path` as aux_index.bin: magic "GNNPEAUX", uint32 version = 1, L, D, reserved, uint64
 * n_nodes, then key, degrees, label_mbr as above.  `gnnpe_main --index --sidecars` leaves one next to every index.dat. */
int gnnpe_build_aux_index(gnnpe_ctx *ctx, uint32_t pid, const char *path);
/* Host-side reader of aux_index.bin: malloc'ed arrays (gnnpe_host_free).  No GPU. */
int gnnpe_host_load_aux_index(const char *path, uint32_t *n_nodes, uint32_t *L, uint32_t *D, double **key, uint32_t **degrees,
                              double **label_mbr);

/* ---- introspection for bench / tests ------------------------------------------------------------ */
/* Name of the kernel instantiation that dominates the fill (for matching rocprofv3 rows). */
const char *gnnpe_fill_kernel_name(void);
/* Selects the enumeration implementation (call before gnnpe_count_paths).  Both produce identical outputs:
 *   4 one wave per start vertex over rank-sorted neighbour records; rows longer than 64 are streamed in id order by
 *     the same kernel (default)
 *   1 one wave per (start, middle) pair, direct stores, run-time embedding width: the generic form used for widths
 *     without a specialised instantiation (e not in {1,2,3,4,8}); selectable as the A/B baseline */
int gnnpe_set_fill_variant(gnnpe_ctx *ctx, int variant);
/* Shape of the emit launch of variant 4 (the reference's dfs + gen_pde, custom.h:66-92, 546-572); outputs are identical.
 * Times: BASELINE config 3 into an allocation of the fast / of the slow class, profiles/r05_emit_ab.txt, r06_emit_oneshot.txt.
 *   0    whichever gnnpe_emit_calibrate_device measured fastest into the fill's output buffer; shape 1 for a buffer nobody
 *        calibrated (default)
 *   1    one wave per start vertex, ONE-SHOT since round 6 -- workgroups in launch order, exit; 128 rows staged per flush
 *        (k_fill_ranked): 2.73-2.76 / 3.23-3.3 ms (rounds 4-5: a resident grid of five workgroups per CU, start vertices from
 *        ticket counters: 2.81-2.84 / 3.3-3.4)
 *   4    the same kernel as a resident grid of three workgroups per CU, start vertices in order from ticket counters:
 *        3.05-3.25 / 3.13-3.6 ms -- the faster one in one kind of slow allocation (at widths e > 2: natural occupancy)
 *   2    one wave per output tile of 64 rows, workgroups in launch order, one store burst per wave (k_fill_tiles): 3.2-3.3 /
 *        3.3-3.55 ms; graphs with rows longer than 64 still take the start-vertex kernel, which streams such rows
 *   3    persistent waves that take output tiles in order from ticket counters, three tiles in flight per wave
 *        (k_fill_tickets, e <= 2): 3.9 / 4.1 ms -- measured and never chosen.  Since ABI 6 the kernel lives in the diagnostic
 *        build only (make DIAG=1 diag); the shipped library accepts the value and answers with shape 2
 * The environment variable GNNPE_EMIT=starts|starts_low|tiles, read when the context is created, overrides the context's setting. */
int gnnpe_set_emit_shape(gnnpe_ctx *ctx, int shape);
/* Times the emit shapes 1, 4 and 2 into the caller's output buffers (rows [0, total) of the context's current l=2 count, which
 * must fit rows_cap, the buffers' capacity in rows; three launches each: the buffers are overwritten with the paths) and
 * remembers the fastest FOR THESE BUFFERS: with emit shape 0 later fills into them take it.  The rate a kernel reaches depends
 * on the allocation it writes to and on its shape.  ms_by_shape (5 floats, indexed by shape; may be null)
 * receives the times, 0 for a shape that was not run -- all 0 when only one shape applies (hub rows, fewer than 2^24 paths).
 * The entry is dropped when the buffer is freed through gnnpe_dev_free / gnnpe_output_pool_destroy.
 * gnnpe_output_pool_create calibrates the buffer it keeps unless told not to. */
int gnnpe_emit_calibrate_device(gnnpe_ctx *ctx, uint64_t rows_cap, void *dev_vids, void *dev_pde, float *ms_by_shape, int *shape_kept);
/* Bytes of the index.dat a partition of `points` paths of dimension D becomes (header block + one 4 KiB block per node of the
 * bulk-loaded tree; rtnode.cpp:27-28, blk_file.cpp:38-52), by the builder that writes it: 0 = the pair-major / triple-major build behind
 * gnnpe_build_index / gnnpe_build_index_partition_device (nodes of min(capacity - 1, 64) entries), 1 = the tuple-array build
 * gnnpe_build_index_device (min(capacity - 2, 64): what the multi-GPU path uses).  No GPU, no context: callers check the
 * reference's 2 GiB limit (blk_file.h:32-33) BEFORE anything is built or written.  0 for a dimension no node holds. */
uint64_t gnnpe_index_file_bytes(uint64_t points, uint32_t D, int builder);
/* Name of the emit kernel the context's last fill launched ("" before the first fill): the rocprofv3 row to match. */
const char *gnnpe_emit_kernel_name(gnnpe_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
