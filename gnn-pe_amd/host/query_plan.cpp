// query_plan.cpp -- see query_plan.h
#include "query_plan.h"

#include <algorithm>
#include <set>

#include "../../include/gnnpe_hip.h"

namespace gnnpe_host {

namespace {

struct PlanPath {
    uint32_t v[3];
    uint32_t weight;
};

// dfs_query (custom.h:94-119) for paths of `len` vertices (the reference's: 3)
void dfs(const StaticGraph &q, std::vector<uint32_t> &path, std::set<std::vector<uint32_t>> &seen,
         std::vector<std::vector<uint32_t>> &out, size_t len = 3)
{
    if (path.size() == len) {
        if (seen.count(path)) return;
        std::vector<uint32_t> rev(path.rbegin(), path.rend());
        if (seen.count(rev)) return;
        out.push_back(path);
        seen.insert(path);
        return;
    }
    const uint32_t node = path.back();
    for (uint32_t i = q.offsets[node]; i < q.offsets[node + 1]; i++) {
        const uint32_t nb = q.neighbors[i];
        if (std::find(path.begin(), path.end(), nb) != path.end()) continue;
        path.push_back(nb);
        dfs(q, path, seen, out, len);
        path.pop_back();
    }
}

}  // namespace

int query_vde(const StaticGraph &q, uint32_t e, std::vector<double> *x_out, std::vector<double> *vde_out, std::string *err)
{
    // gen_vde (custom.h:513-544): x from the label, nx summed over ascending neighbours from 0.0, vde = x + nx
    const uint32_t n = q.n, n_labels = std::max<uint32_t>(q.labels_count, 1);
    std::vector<double> table((size_t)n_labels * e);
    std::vector<double> &x = *x_out, &vde = *vde_out;
    x.assign((size_t)n * e, 0.0);
    vde.assign((size_t)n * e, 0.0);
    if (gnnpe_host_label_table(n_labels, e, table.data()) != 0) {
        if (err) *err = "label table failed";
        return -2;
    }
    for (uint32_t v = 0; v < n; v++)
        for (uint32_t k = 0; k < e; k++) x[(size_t)v * e + k] = table[(size_t)q.labels[v] * e + k];
    for (uint32_t v = 0; v < n; v++)
        for (uint32_t k = 0; k < e; k++) {
            double nx = 0.0;
            for (uint32_t i = q.offsets[v]; i < q.offsets[v + 1]; i++) nx += x[(size_t)q.neighbors[i] * e + k];
            vde[(size_t)v * e + k] = x[(size_t)v * e + k] + nx;
        }
    return 0;
}

int build_pge_query_groups(const StaticGraph &q, uint32_t e, PgeQueryGroups *out, std::string *err)
{
    if (!out || e == 0) {
        if (err) *err = "build_pge_query_groups: null output / e = 0";
        return -2;
    }
    const uint32_t n = q.n, D = 2 * e, W = 2 * D;
    for (uint32_t u = 0; u < n; u++)
        if (q.degree(u) == 0) {  // its group stays empty in the reference (main.cpp:278-281), and its leaf test reads past it
            if (err) *err = "query vertex " + std::to_string(u) + " has no edge: GNN-PGE defines no path group for it";
            return -3;
        }
    std::vector<double> x, vde;
    if (query_vde(q, e, &x, &vde, err) != 0) return -2;
    out->n_vertices = n;
    out->e = e;
    out->labels.assign(q.labels.begin(), q.labels.begin() + n);
    out->degrees.resize(n);
    out->pg.assign((size_t)n * W, 0.0);
    out->plg.assign((size_t)n * W, 0.0);
    std::vector<double> pe(D), le(D);
    for (uint32_t u = 0; u < n; u++) {
        out->degrees[u] = q.degree(u);
        double *g = &out->pg[(size_t)u * W], *lg = &out->plg[(size_t)u * W];
        // main.cpp:253-329: the 1-hop paths (u, w), w in adjacency order; the first path's embedding seeds [lo, hi], the others
        // replace a bound they pass -- the reference's own compare-and-replace, in its order
        for (uint32_t i = q.offsets[u]; i < q.offsets[u + 1]; i++) {
            const uint32_t w = q.neighbors[i];
            for (uint32_t k = 0; k < e; k++) {
                pe[k] = vde[(size_t)u * e + k];
                pe[e + k] = vde[(size_t)w * e + k];
                le[k] = x[(size_t)u * e + k];
                le[e + k] = x[(size_t)w * e + k];
            }
            const bool first = i == q.offsets[u];
            for (uint32_t j = 0; j < D; j++) {
                if (first || g[2 * j] > pe[j]) g[2 * j] = pe[j];
                if (first || g[2 * j + 1] < pe[j]) g[2 * j + 1] = pe[j];
                if (first || lg[2 * j] > le[j]) lg[2 * j] = le[j];
                if (first || lg[2 * j + 1] < le[j]) lg[2 * j + 1] = le[j];
            }
        }
    }
    return 0;
}

int build_query_plan(const StaticGraph &q, uint32_t e, QueryPlan *out, std::string *err)
{
    if (!out || e == 0) {
        if (err) *err = "build_query_plan: null output / e = 0";
        return -2;
    }
    const uint32_t n = q.n, L = 3;
    out->n_vertices = n;
    out->L = L;
    out->e = e;
    out->vids.clear();
    out->labels.clear();
    out->degrees.clear();
    out->pde.clear();
    out->pde_label.clear();

    // main.cpp:139-146
    std::vector<std::vector<uint32_t>> all_paths;
    std::set<std::vector<uint32_t>> seen;
    for (uint32_t node = 0; node < n; node++) {
        std::vector<uint32_t> path = {node};
        dfs(q, path, seen, all_paths);
    }

    std::vector<double> x, vde;
    if (query_vde(q, e, &x, &vde, err) != 0) return -2;

    // gen_query_pde (custom.h:574-631): weight = sum of degrees; std::sort by weight, descending -- the same
    // library algorithm and comparator as the reference, so ties fall the same way
    std::vector<PlanPath> paths(all_paths.size());
    for (size_t i = 0; i < all_paths.size(); i++) {
        paths[i].weight = 0;
        for (uint32_t j = 0; j < L; j++) {
            paths[i].v[j] = all_paths[i][j];
            paths[i].weight += q.degree(all_paths[i][j]);
        }
    }
    std::sort(paths.begin(), paths.end(), [](const PlanPath &a, const PlanPath &b) { return a.weight > b.weight; });
    std::set<uint32_t> covered;
    for (const PlanPath &p : paths) {
        uint32_t hit = 0;
        for (uint32_t j = 0; j < L; j++) hit += covered.count(p.v[j]) ? 1u : 0u;
        if (hit != L) {
            for (uint32_t j = 0; j < L; j++) {
                covered.insert(p.v[j]);
                out->vids.push_back(p.v[j]);
                out->labels.push_back(q.labels[p.v[j]]);
                out->degrees.push_back(q.degree(p.v[j]));
                for (uint32_t k = 0; k < e; k++) {
                    out->pde.push_back(vde[(size_t)p.v[j] * e + k]);
                    out->pde_label.push_back(x[(size_t)p.v[j] * e + k]);
                }
            }
        }
        if (covered.size() == n) break;
    }
    return 0;
}

namespace {

// one path (or, at width 1, one vertex) onto a plan: vids, labels, degrees, and the vde / x of every position
void append_path(const StaticGraph &q, uint32_t e, const uint32_t *v, uint32_t width, const std::vector<double> &x,
                 const std::vector<double> &vde, QueryPlan *out)
{
    for (uint32_t j = 0; j < width; j++) {
        out->vids.push_back(v[j]);
        out->labels.push_back(q.labels[v[j]]);
        out->degrees.push_back(q.degree(v[j]));
        for (uint32_t k = 0; k < e; k++) {
            out->pde.push_back(vde[(size_t)v[j] * e + k]);
            out->pde_label.push_back(x[(size_t)v[j] * e + k]);
        }
    }
}

void reset_plan(QueryPlan *p, uint32_t n, uint32_t L, uint32_t e)
{
    *p = QueryPlan();
    p->n_vertices = n;
    p->L = L;
    p->e = e;
}

}  // namespace

int build_query_plan_exact(const StaticGraph &q, uint32_t e, uint32_t l, ExactPlan *out, std::string *err)
{
    if (!out || e == 0 || (l != 2 && l != 3)) {
        if (err) *err = "build_query_plan_exact: null output / e = 0 / l not 2 or 3";
        return -2;
    }
    const uint32_t n = q.n;
    QueryPlan ref;  // the reference's plan: the main plan at l = 2, the pool of (b) at l = 3
    if (build_query_plan(q, e, &ref, err) != 0) return -2;
    std::vector<double> x, vde;
    if (query_vde(q, e, &x, &vde, err) != 0) return -2;
    reset_plan(&out->main, n, l + 1, e);
    reset_plan(&out->tri, n, 3, e);
    reset_plan(&out->single, n, 1, e);
    std::set<uint32_t> covered;
    // the gen_query_pde rule (custom.h:606-626): a path is taken while it still covers a new vertex, until all are covered
    auto take = [&](const uint32_t *v, uint32_t width, QueryPlan *dst) {
        if (covered.size() == n) return;
        uint32_t hit = 0;
        for (uint32_t j = 0; j < width; j++) hit += covered.count(v[j]) ? 1u : 0u;
        if (hit == width) return;
        for (uint32_t j = 0; j < width; j++) covered.insert(v[j]);
        append_path(q, e, v, width, x, vde, dst);
    };
    if (l == 2) {
        out->main = ref;
        for (uint32_t v : ref.vids) covered.insert(v);
    } else {
        // (a) every simple 4-vertex path by the dfs_query rule (a path whose reverse was kept is dropped), sorted by weight =
        // the sum of its degrees, descending.  The reference has no 4-vertex plan, hence no tie order to follow: std::stable_sort
        // keeps ties in DFS order, so the plan does not depend on the standard library's sort
        std::vector<std::vector<uint32_t>> all4;
        std::set<std::vector<uint32_t>> seen;
        for (uint32_t node = 0; node < n; node++) {
            std::vector<uint32_t> path = {node};
            dfs(q, path, seen, all4, 4);
        }
        std::vector<uint32_t> weight(all4.size(), 0);
        std::vector<size_t> order(all4.size());
        for (size_t i = 0; i < all4.size(); i++) {
            order[i] = i;
            for (uint32_t v : all4[i]) weight[i] += q.degree(v);
        }
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight[a] > weight[b]; });
        for (size_t i : order) take(all4[i].data(), 4, &out->main);
        // (b) what no 4-vertex path covers, from the reference's 3-vertex plan in its order
        for (uint32_t i = 0; i < ref.n_paths(); i++) take(&ref.vids[(size_t)i * 3], 3, &out->tri);
    }
    // (c) a query vertex on no plan path (no 3- or 4-vertex path through it, e.g. a single-edge query) is tested alone
    for (uint32_t u = 0; u < n; u++)
        if (!covered.count(u)) append_path(q, e, &u, 1, x, vde, &out->single);
    return 0;
}

}  // namespace gnnpe_host
