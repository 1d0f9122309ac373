// graph_update.h -- a batch of undirected edge insertions and deletions applied to a CSR on the host: the host form of
// gnnpe_csr_apply_edges (include/gnnpe_hip.h, ABI 16), the yardstick of the device form and the host mirror of a caller.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace gnnpe_host {

// The two directed keys (x << 32) | y of every pair, ascending, each once.  -1 and *err for x == y or an id >= n.
int update_edge_keys(uint32_t n, const uint32_t *edges, uint64_t n_edges, const char *what, std::vector<uint64_t> *keys, std::string *err);

// G' = (E(G) minus D) plus I as a compact CSR.  0, or -1 (refusal: *err names one offending pair) / -5 (entries' + n >= 2^32);
// nothing is written on a refusal.
int csr_apply_edges(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *insert_edges, uint64_t n_insert,
                    const uint32_t *delete_edges, uint64_t n_delete, std::vector<uint32_t> *out_offsets, std::vector<uint32_t> *out_nbrs,
                    std::string *err);

// map[j'] for every entry j' = (x -> y) of the new CSR: the index of the entry (x -> y) in the old one, 0xFFFFFFFF
// (GNNPE_NO_ENTRY) where the old row does not have y.  Both are compact simple CSRs on the same n vertices.
void csr_entry_map(uint32_t n, const uint32_t *old_offsets, const uint32_t *old_nbrs, const uint32_t *new_offsets, const uint32_t *new_nbrs,
                   uint32_t *map);

// The host form of gnnpe_csr_apply_vertices: the vertices of `remove` (ids < n, repeats tolerated) leave with their edges, the
// survivors keep their order under new ids, one vertex per word of add_labels is appended with an empty row.  vertex_map: the old
// id of every new vertex, 0xFFFFFFFF (GNNPE_NO_VERTEX) for an added one.  0, or -1 (an id >= n, no vertex left: *err says which) /
// -5 (n' >= 2^32 - 1 or entries' + n' >= 2^32); the outputs of a refused batch mean nothing.
int csr_apply_vertices(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels, const uint32_t *remove,
                       uint64_t n_remove, const uint32_t *add_labels, uint64_t n_add, std::vector<uint32_t> *out_offsets,
                       std::vector<uint32_t> *out_nbrs, std::vector<uint32_t> *out_labels, std::vector<uint32_t> *vertex_map, std::string *err);

}  // namespace gnnpe_host
