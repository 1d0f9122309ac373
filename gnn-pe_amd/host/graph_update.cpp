// graph_update.cpp -- gnnpe_host_csr_apply_edges: sort and de-duplicate the directed keys of the two lists, check them against
// the rows, merge row by row.  gnnpe_host_csr_entry_map: the entries of one CSR among those of another, a two-pointer walk per
// row.  gnnpe_host_csr_apply_vertices: a table of new ids, then the rows of the survivors copied entry by entry.  Plain C++; shares
// nothing with csrc/gnnpe_update.hip or csrc/gnnpe_update_vertices.hip.
#include "graph_update.h"

#include <algorithm>

namespace gnnpe_host {

int update_edge_keys(uint32_t n, const uint32_t *edges, uint64_t n_edges, const char *what, std::vector<uint64_t> *keys, std::string *err)
{
    keys->clear();
    keys->reserve(2 * n_edges);
    for (uint64_t i = 0; i < n_edges; i++) {
        const uint32_t x = edges[2 * i], y = edges[2 * i + 1];
        if (x == y || x >= n || y >= n) {
            *err = std::string(what) + " (" + std::to_string(x) + ", " + std::to_string(y) + ")" +
                   (x == y ? " is a loop" : " names a vertex the graph does not have (n = " + std::to_string(n) + ")");
            return -1;
        }
        keys->push_back(((uint64_t)x << 32) | y);
        keys->push_back(((uint64_t)y << 32) | x);
    }
    std::sort(keys->begin(), keys->end());
    keys->erase(std::unique(keys->begin(), keys->end()), keys->end());
    return 0;
}

static std::string pair_text(uint64_t key) { return "(" + std::to_string((uint32_t)(key >> 32)) + ", " + std::to_string((uint32_t)key) + ")"; }

int csr_apply_edges(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *insert_edges, uint64_t n_insert,
                    const uint32_t *delete_edges, uint64_t n_delete, std::vector<uint32_t> *out_offsets, std::vector<uint32_t> *out_nbrs,
                    std::string *err)
{
    std::vector<uint64_t> ins, del;
    if (update_edge_keys(n, insert_edges, n_insert, "insertion", &ins, err) != 0) return -1;
    if (update_edge_keys(n, delete_edges, n_delete, "deletion", &del, err) != 0) return -1;
    auto is_edge = [&](uint64_t key) {
        const uint32_t x = (uint32_t)(key >> 32), y = (uint32_t)key;
        return std::binary_search(nbrs + offsets[x], nbrs + offsets[x + 1], y);
    };
    for (uint64_t k : ins) {
        if (std::binary_search(del.begin(), del.end(), k)) {
            *err = "edge " + pair_text(k) + " is in both lists";
            return -1;
        }
        if (is_edge(k)) {
            *err = "insertion " + pair_text(k) + " is already an edge of the graph";
            return -1;
        }
    }
    for (uint64_t k : del)
        if (!is_edge(k)) {
            *err = "deletion " + pair_text(k) + " is not an edge of the graph";
            return -1;
        }
    const uint64_t after = (uint64_t)offsets[n] + ins.size() - del.size();
    if (after + n >= (1ull << 32)) {
        *err = std::to_string(after) + " entries + " + std::to_string(n) + " vertices exceed 32-bit addressing";
        return -5;
    }
    out_offsets->assign((size_t)n + 1, 0);
    out_nbrs->clear();
    out_nbrs->reserve(after);
    size_t pi = 0, pd = 0;
    for (uint32_t x = 0; x < n; x++) {
        (*out_offsets)[x] = (uint32_t)out_nbrs->size();
        uint32_t j = offsets[x];
        const uint32_t end = offsets[x + 1];
        // the old row and the row's insert keys, both ascending, merged; an old entry that is the next delete key is skipped
        for (;;) {
            const bool have_ins = pi < ins.size() && (uint32_t)(ins[pi] >> 32) == x;
            if (j < end && (!have_ins || nbrs[j] < (uint32_t)ins[pi])) {
                if (pd < del.size() && del[pd] == (((uint64_t)x << 32) | nbrs[j])) pd++;
                else out_nbrs->push_back(nbrs[j]);
                j++;
            } else if (have_ins) {
                out_nbrs->push_back((uint32_t)ins[pi++]);
            } else {
                break;
            }
        }
    }
    (*out_offsets)[n] = (uint32_t)out_nbrs->size();
    return 0;
}

void csr_entry_map(uint32_t n, const uint32_t *old_offsets, const uint32_t *old_nbrs, const uint32_t *new_offsets, const uint32_t *new_nbrs,
                   uint32_t *map)
{
    for (uint32_t x = 0; x < n; x++) {
        uint32_t j = old_offsets[x];
        const uint32_t end = old_offsets[x + 1];
        // both rows ascend: the old row's pointer only moves forward
        for (uint32_t k = new_offsets[x]; k < new_offsets[x + 1]; k++) {
            while (j < end && old_nbrs[j] < new_nbrs[k]) j++;
            map[k] = j < end && old_nbrs[j] == new_nbrs[k] ? j : 0xFFFFFFFFu;
        }
    }
}

int csr_apply_vertices(uint32_t n, const uint32_t *offsets, const uint32_t *nbrs, const uint32_t *labels, const uint32_t *remove,
                       uint64_t n_remove, const uint32_t *add_labels, uint64_t n_add, std::vector<uint32_t> *out_offsets,
                       std::vector<uint32_t> *out_nbrs, std::vector<uint32_t> *out_labels, std::vector<uint32_t> *vertex_map, std::string *err)
{
    // new id of every vertex, 0xFFFFFFFF for a removed one: a running count of the survivors
    std::vector<uint32_t> id((size_t)n, 0);
    for (uint64_t i = 0; i < n_remove; i++) {
        if (remove[i] >= n) {
            *err = "vertex " + std::to_string(remove[i]) + " is not a vertex of the graph (n = " + std::to_string(n) + ")";
            return -1;
        }
        id[remove[i]] = 0xFFFFFFFFu;
    }
    uint64_t kept = 0;
    for (uint32_t v = 0; v < n; v++)
        if (id[v] != 0xFFFFFFFFu) id[v] = (uint32_t)kept++;
    const uint64_t after = kept + n_add;
    if (after == 0) {
        *err = "the batch leaves no vertex";
        return -1;
    }
    if (after >= 0xFFFFFFFFull) {
        *err = std::to_string(after) + " vertices exceed 32-bit ids";
        return -5;
    }
    out_offsets->clear();
    out_nbrs->clear();
    out_labels->clear();
    vertex_map->clear();
    for (uint32_t v = 0; v < n; v++) {
        if (id[v] == 0xFFFFFFFFu) continue;
        out_offsets->push_back((uint32_t)out_nbrs->size());
        out_labels->push_back(labels[v]);
        vertex_map->push_back(v);
        for (uint32_t j = offsets[v]; j < offsets[v + 1]; j++)
            if (id[nbrs[j]] != 0xFFFFFFFFu) out_nbrs->push_back(id[nbrs[j]]);
    }
    for (uint64_t i = 0; i < n_add; i++) {
        out_offsets->push_back((uint32_t)out_nbrs->size());
        out_labels->push_back(add_labels[i]);
        vertex_map->push_back(0xFFFFFFFFu);
    }
    out_offsets->push_back((uint32_t)out_nbrs->size());
    if (out_nbrs->size() + after >= (1ull << 32)) {
        *err = std::to_string(out_nbrs->size()) + " entries + " + std::to_string(after) + " vertices exceed 32-bit addressing";
        return -5;
    }
    return 0;
}

}  // namespace gnnpe_host
