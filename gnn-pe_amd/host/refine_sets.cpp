// refine_sets.cpp -- see refine_sets.h
#include "refine_sets.h"

#include <algorithm>
#include <vector>

#include "refine.h"

namespace gnnpe_host {

namespace {

struct SetSearch {
    const StaticGraph &g, &q;
    const uint32_t *bitmap;
    uint64_t words;
    std::vector<uint32_t> order, pivot;       // matching order; an earlier neighbour of order[i] for i >= 1
    std::vector<std::vector<uint32_t>> back;  // the other earlier neighbours of order[i]
    std::vector<std::vector<uint32_t>> above, below;  // earlier query vertices whose image order[i]'s must be greater / smaller than
    std::vector<std::vector<uint32_t>> non;   // induced: the earlier query vertices order[i] is not adjacent to
    std::vector<uint32_t> image;              // query vertex -> data vertex
    std::vector<uint8_t> used;                // data vertex taken
    uint64_t count = 0, limit;
    uint64_t *vcounts = nullptr;              // vertex counts: nq x g.n cells, every find adds 1 to the cell of each of its images
    uint64_t *ecounts = nullptr;              // edge counts: qedges.size() x g.offsets[g.n] cells, every find adds 1 per query edge
    std::vector<std::pair<uint32_t, uint32_t>> qedges;  // query_edges(q), for ecounts
    std::vector<std::pair<uint32_t, uint32_t>> anchors;  // delta: the query pairs looked up in F -- query_edges(q), or query_nonedges(q)
    const std::vector<uint64_t> *delta = nullptr;       // delta: ascending keys (min << 32) | max; a find with no anchor on one is dropped
    const std::vector<uint8_t> *in_s = nullptr;         // vertices: a byte per data vertex, 1 = in S; a find with no image in S is dropped

    bool in_set(uint32_t u, uint32_t v) const { return (bitmap[(size_t)u * words + (v >> 5)] >> (v & 31)) & 1u; }
    bool fits(uint32_t u, uint32_t v) const
    {
        return in_set(u, v) && !used[v] && g.labels[v] == q.labels[u] && g.degree(v) >= q.degree(u);
    }
    bool edge(uint32_t a, uint32_t b) const
    {
        if (g.degree(b) < g.degree(a)) std::swap(a, b);  // the shorter row
        return std::binary_search(g.neighbors.begin() + g.offsets[a], g.neighbors.begin() + g.offsets[a + 1], b);
    }
    void extend(size_t depth)
    {
        if (depth == order.size()) {
            if (delta) {
                bool touches = false;
                for (size_t k = 0; k < anchors.size() && !touches; k++)
                    touches = std::binary_search(delta->begin(), delta->end(), delta_key(image[anchors[k].first], image[anchors[k].second]));
                if (!touches) return;
            }
            if (in_s) {
                bool touches = false;
                for (uint32_t u = 0; u < q.n && !touches; u++) touches = (*in_s)[image[u]] != 0;
                if (!touches) return;
            }
            count++;
            if (vcounts)
                for (uint32_t u = 0; u < q.n; u++) vcounts[(size_t)u * g.n + image[u]]++;
            for (size_t k = 0; ecounts && k < qedges.size(); k++) {
                // the entry f(a_k) -> f(b_k): its index in the CSR, by binary search in the row of f(a_k)
                const uint32_t x = image[qedges[k].first], y = image[qedges[k].second];
                const auto row = g.neighbors.begin() + g.offsets[x], end = g.neighbors.begin() + g.offsets[x + 1];
                const auto it = std::lower_bound(row, end, y);
                if (it != end && *it == y) ecounts[k * (size_t)g.offsets[g.n] + (size_t)(it - g.neighbors.begin())]++;
            }
            return;
        }
        const uint32_t u = order[depth], p = image[pivot[depth]];
        for (uint32_t i = g.offsets[p]; i < g.offsets[p + 1] && count < limit; i++) {
            const uint32_t v = g.neighbors[i];
            if (!fits(u, v)) continue;
            bool ok = true;
            for (uint32_t w : above[depth]) ok &= v > image[w];
            for (uint32_t w : below[depth]) ok &= v < image[w];
            if (!ok) continue;
            for (uint32_t w : back[depth])
                if (!edge(v, image[w])) {
                    ok = false;
                    break;
                }
            if (!ok) continue;
            for (uint32_t w : non[depth])
                if (edge(v, image[w])) {
                    ok = false;
                    break;
                }
            if (!ok) continue;
            image[u] = v;
            used[v] = 1;
            extend(depth + 1);
            used[v] = 0;
        }
    }
};

}  // namespace

// The walk of refine_sets_run: a table (of job.table's kind, zeroed) is filled at the finds; a find that touches no edge of
// `delta` (F as ascending keys) is dropped, and so is one with no image in `in_s` (S as a byte mask)
static int refine_sets_walk(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words, uint64_t limit,
                            const SetsJob &job, uint64_t *table, const std::vector<uint64_t> *delta, const std::vector<uint8_t> *in_s,
                            uint64_t *answers, std::string *err)
{
    const uint32_t nq = query.n;
    const auto *pairs = job.pairs;
    uint64_t *vcounts = job.table == SetsJob::kVertexTable ? table : nullptr, *ecounts = job.table == SetsJob::kEdgeTable ? table : nullptr;
    if (!answers || !bitmap || words != ((uint64_t)data.n + 31) / 32) {
        if (err) *err = "refine_sets_count: one bitmap row of ceil(n / 32) words per query vertex expected";
        return -2;
    }
    *answers = 0;
    if (nq == 0) return 0;
    MatchOrder mo;
    if (build_match_order(query, set_sizes(bitmap, words, nq), &mo, err) != 0) return -2;  // (a disconnected query is refused whatever the limit)
    if (limit == 0) return 0;
    SetSearch s{data, query, bitmap, words, mo.order, mo.pivot, {}, std::vector<std::vector<uint32_t>>(nq),
                std::vector<std::vector<uint32_t>>(nq), std::vector<std::vector<uint32_t>>(nq), std::vector<uint32_t>(nq, 0),
                std::vector<uint8_t>(data.n, 0), 0, limit, vcounts, ecounts,
                ecounts ? query_edges(query) : std::vector<std::pair<uint32_t, uint32_t>>(),
                !delta ? std::vector<std::pair<uint32_t, uint32_t>>() : job.nonedges ? query_nonedges(query) : query_edges(query), delta, in_s};
    for (uint32_t i = 0; i < nq; i++) s.back.emplace_back(mo.back.begin() + mo.back_off[i], mo.back.begin() + mo.back_off[i + 1]);
    // every earlier query vertex but the pivot and the back neighbours is a non-neighbour: tested after the back edges
    for (uint32_t i = 1; job.induced && i < nq; i++)
        for (uint32_t j = 0; j < i; j++) {
            const uint32_t w = mo.order[j];
            if (w != mo.pivot[i] && std::find(s.back[i].begin(), s.back[i].end(), w) == s.back[i].end()) s.non[i].push_back(w);
        }
    if (pairs) {
        // f(a) < f(b) is tested where the later of the two in the order gets its image
        std::vector<uint32_t> pos_of(nq, 0);
        for (uint32_t i = 0; i < nq; i++) pos_of[mo.order[i]] = i;
        for (const auto &ab : *pairs) {
            if (ab.first >= nq || ab.second >= nq || ab.first == ab.second) {
                if (err) *err = "refine_sets_count: an ordering pair names a vertex the query does not have";
                return -2;
            }
            if (pos_of[ab.first] < pos_of[ab.second]) s.above[pos_of[ab.second]].push_back(ab.first);
            else s.below[pos_of[ab.first]].push_back(ab.second);
        }
    }
    const uint32_t start = mo.order[0];
    for (uint32_t v : set_members(bitmap, words, start, data.n)) {
        if (s.count >= limit) break;
        if (!s.fits(start, v)) continue;
        s.image[start] = v;
        s.used[v] = 1;
        s.extend(1);
        s.used[v] = 0;
    }
    *answers = std::min(s.count, limit);
    return 0;
}

std::vector<std::pair<uint32_t, uint32_t>> query_edges(const StaticGraph &query)
{
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (uint32_t a = 0; a < query.n; a++)
        for (uint32_t i = query.offsets[a]; i < query.offsets[a + 1]; i++) {
            const uint32_t b = query.neighbors[i];
            if (a < b && (out.empty() || out.back() != std::make_pair(a, b))) out.emplace_back(a, b);  // (a repeated `e` line: once)
        }
    return out;
}

std::vector<std::pair<uint32_t, uint32_t>> query_nonedges(const StaticGraph &query)
{
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (uint32_t a = 0; a < query.n; a++)
        for (uint32_t b = a + 1; b < query.n; b++)
            if (!std::binary_search(query.neighbors.begin() + query.offsets[a], query.neighbors.begin() + query.offsets[a + 1], b))
                out.emplace_back(a, b);
    return out;
}

size_t sets_table_cells(const StaticGraph &data, const StaticGraph &query, SetsJob::Table table)
{
    if (table == SetsJob::kVertexTable) return (size_t)query.n * data.n;
    if (table == SetsJob::kEdgeTable) return query_edges(query).size() * (size_t)(data.n ? data.offsets[data.n] : 0);
    return 0;
}

int delta_edge_keys(uint32_t n, const uint32_t *delta_edges, uint64_t n_delta, std::vector<uint64_t> *keys, std::string *err)
{
    keys->clear();
    if (n_delta && !delta_edges) {
        if (err) *err = "delta edges: null argument";
        return -2;
    }
    for (uint64_t i = 0; i < n_delta; i++) {
        const uint32_t x = delta_edges[2 * i], y = delta_edges[2 * i + 1];
        if (x == y || x >= n || y >= n) {
            if (err) *err = "delta edge " + std::to_string(i) + " (" + std::to_string(x) + ", " + std::to_string(y) + "): " +
                            (x == y ? "a loop" : "a vertex id the graph does not have");
            return -2;
        }
        keys->push_back(delta_key(x, y));
    }
    std::sort(keys->begin(), keys->end());
    keys->erase(std::unique(keys->begin(), keys->end()), keys->end());
    return 0;
}

int delta_vertex_ids(uint32_t n, const uint32_t *vertices, uint64_t n_vertices, std::vector<uint32_t> *ids, std::string *err)
{
    ids->clear();
    if (n_vertices && !vertices) {
        if (err) *err = "vertices: null argument";
        return -2;
    }
    for (uint64_t i = 0; i < n_vertices; i++)
        if (vertices[i] >= n) {
            if (err) *err = "vertex " + std::to_string(i) + " (" + std::to_string(vertices[i]) + "): a vertex id the graph does not have";
            return -2;
        }
    ids->assign(vertices, vertices + n_vertices);
    std::sort(ids->begin(), ids->end());
    ids->erase(std::unique(ids->begin(), ids->end()), ids->end());
    return 0;
}

// F as ascending keys, each a checked edge of the graph -- or, with `nonedges`, each checked NOT to be one: what a job through F
// refuses
static int delta_keys_checked(const StaticGraph &data, const uint32_t *delta_edges, uint64_t n_delta, bool nonedges,
                              std::vector<uint64_t> *keys, std::string *err)
{
    if (delta_edge_keys(data.n, delta_edges, n_delta, keys, err) != 0) return -2;
    for (uint64_t key : *keys) {
        const uint32_t x = (uint32_t)(key >> 32), y = (uint32_t)key;
        if (std::binary_search(data.neighbors.begin() + data.offsets[x], data.neighbors.begin() + data.offsets[x + 1], y) == nonedges) {
            if (err) *err = (nonedges ? "pair (" : "delta edge (") + std::to_string(x) + ", " + std::to_string(y) +
                            (nonedges ? ") is an edge of the graph" : ") is not an edge of the graph");
            return -2;
        }
    }
    return 0;
}

int refine_sets_run(const StaticGraph &data, const StaticGraph &query, const uint32_t *bitmap, uint64_t words, uint64_t limit,
                    const SetsJob &job, uint64_t *answers, bool *complete, uint64_t *counts, std::string *err)
{
    const size_t cells = sets_table_cells(data, query, job.table);
    if (answers) *answers = 0;
    if (job.table != SetsJob::kNoTable && (!complete || (!counts && cells))) {
        // (the texts name the three forms this entry had once: callers show them)
        if (err) *err = job.through ? "refine_sets_delta counts: null argument"
                        : job.table == SetsJob::kVertexTable ? "refine_sets_vertex_counts: null argument"
                                                             : "refine_sets_edge_counts: null argument";
        return -2;
    }
    if (complete) *complete = false;
    std::vector<uint64_t> keys;
    if (job.nonedges && (!job.through || !job.induced)) {
        if (err) *err = "the maps through a set of non-edges: an induced job";
        return -2;
    }
    if (job.through && delta_keys_checked(data, job.delta_edges, job.n_delta, job.nonedges, &keys, err) != 0) return -2;
    std::vector<uint32_t> ids;
    std::vector<uint8_t> in_s;
    if (job.through_vertices) {
        if (job.through) {
            if (err) *err = "a job through a set of edges or through a set of vertices, not both";
            return -2;
        }
        if (delta_vertex_ids(data.n, job.vertices, job.n_vertices, &ids, err) != 0) return -2;
        in_s.assign(data.n, 0);
        for (uint32_t v : ids) in_s[v] = 1;
    }
    if (cells) std::fill(counts, counts + cells, 0ull);
    // (an empty F or S drops every find: limit 0, and the walk still refuses what it refuses)
    const bool nothing = (job.through && keys.empty()) || (job.through_vertices && ids.empty());
    const int rc = refine_sets_walk(data, query, bitmap, words, nothing ? 0 : limit, job, cells ? counts : nullptr,
                                    job.through ? &keys : nullptr, job.through_vertices ? &in_s : nullptr, answers, err);
    // the walk stops at `limit` finds: below it, it walked everything (limit 0 walks nothing, and 0 < 0 is false; no F: 0 < limit)
    if (rc == 0 && complete) *complete = *answers < limit;
    return rc;
}

}  // namespace gnnpe_host
