// main_pge.cpp -- `gnnpge_main`: drop-in for the GROUPED variant's `main` (GNN-PGE/src/main.cpp:38-361), the first "next"
// row of SURVEY 8(f).
//
// Same flags and defaults as the reference.
// -m offline reads <f>gnn-pge/membership.txt, writes
//   <f>gnn-pge/data_vertices.bin                         (main.cpp:179-194)
//   <f>gnn-pge/partitions/partition-i/index.dat          (Partition ctor, custom.h:141-195; the reference
//                                                          builds these at the end of its offline run too)
// Embeddings, path groups and the R-tree images come from the GPU through include/gnnpe_hip.h.
// The `key` double of every record is uninitialised memory in the reference for data vertices
// (SURVEY 8(f)); it is written as 0 here and never read by the reference's online code for them.
//
// -m online -q <query.graph> answers the query (main.cpp:197-361): reads membership.txt and data_vertices.bin back
// (checked against the graph and -e before any GPU call), computes the query vertices' path groups on the host
// (main.cpp:253-329), runs the leaf test of Partition::query over every data vertex on the GPU (k_pge_filter: the
// R-tree walk only prunes) and the refinement on the device (gnnpe_refine in libgnnpe_online.so), and prints the
// reference's answer line.  Unlike the reference it writes nothing: a missing partitions/partition-i/index.dat is not
// built as a side effect, and no index.dat is read.  -m filter stops after the filter and writes
// <f>gnn-pge/candidates.bin (the format of gnnpe_main's <f>gnn-pe/candidates.bin).
#include <string>
#include <vector>

#include "../../include/gnnpe_online.h"  // for the type of gnnpe_refine only: the library is dlopen()ed (cli_common.h, ONLINE)
#include "cli_common.h"
#include "graph_loader.h"

using namespace cli;

namespace {

// <f>gnn-pge/data_vertices.bin (main.cpp:179-194, read back at main.cpp:197-233): uint32 n, then per vertex uint32 vid,
// label, degree, double key, x[e], nx[e], vde[e], path_group[4e], path_label_group[4e].  A file written for another graph
// or another -e is refused here, before any GPU call: the reference would read past its records or mix them up.
void read_data_vertices(const std::string &path, const gnnpe_host::StaticGraph &g, uint32_t e, std::vector<double> *pg,
                        std::vector<double> *plg)
{
    const std::string again = "; run `gnnpge_main -m offline` with the same -d and -e first";
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die("cannot open " + path + again);
    const size_t rec = 20 + 88 * (size_t)e, W = 4 * (size_t)e;
    const uint64_t want = 4 + (uint64_t)g.n * rec;
    std::vector<char> buf;
    if (fseek(f, 0, SEEK_END) != 0) die("cannot read " + path);
    const long got = ftell(f);
    if (got < 0 || (uint64_t)got != want) {
        fclose(f);
        die(path + " holds " + std::to_string(got) + " bytes, " + std::to_string(want) + " expected for the " + std::to_string(g.n) +
            " vertices of the data graph at -e " + std::to_string(e) + ": it was written for another graph or another -e" + again);
    }
    rewind(f);
    buf.resize(want);
    if (fread(buf.data(), 1, want, f) != want) die("cannot read " + path);
    fclose(f);
    uint32_t count = 0;
    memcpy(&count, buf.data(), 4);
    if (count != g.n)
        die(path + " holds " + std::to_string(count) + " vertices, the data graph " + std::to_string(g.n) + again);
    pg->resize((size_t)g.n * W);
    plg->resize((size_t)g.n * W);
    for (uint32_t v = 0; v < g.n; v++) {
        const char *p = buf.data() + 4 + (size_t)v * rec;
        uint32_t vid, label, degree;
        memcpy(&vid, p, 4);
        memcpy(&label, p + 4, 4);
        memcpy(&degree, p + 8, 4);
        if (vid != v || label != g.labels[v] || degree != g.degree(v))
            die(path + ": record " + std::to_string(v) + " (vid " + std::to_string(vid) + ", label " + std::to_string(label) + ", degree " +
                std::to_string(degree) + ") does not match the data graph (label " + std::to_string(g.labels[v]) + ", degree " +
                std::to_string(g.degree(v)) + "): it was written for another graph" + again);
        p += 20 + 24 * (size_t)e;  // key, x, nx, vde
        memcpy(&(*pg)[(size_t)v * W], p, 8 * W);
        memcpy(&(*plg)[(size_t)v * W], p + 8 * W, 8 * W);
    }
}

// -m online / -m filter (main.cpp:197-361): see the file comment
int run_online(const Options &o)
{
    const auto t0 = Clock::now();
    uint64_t limit = 0xFFFFFFFFull;  // MAX_LIMIT = UINT_MAX (main.cpp:60-67)
    if (o.answers != "MAX") {
        uint32_t lim;
        if (!parse_u32(o.answers, &lim)) die("-n must be MAX or an integer");
        limit = lim;
    }
    gnnpe_host::StaticGraph g;
    std::string err;
    int rc = g.load(o.data_graph, &err, true);  // GNN-PGE: simple graphs only
    if (rc == -1) {  // graph.cpp:166-169
        printf("%s\n", err.c_str());
        exit(-1);
    }
    if (rc != 0) die(o.data_graph + ": " + err);
    std::vector<uint32_t> sorted_nodes, membership;  // read and checked as the reference reads it (main.cpp:76-89); any order gives the same sets
    if (gnnpe_host::read_membership(o.dataset_path + "gnn-pge/membership.txt", g.n, o.partition_num, &sorted_nodes, &membership,
                                    &err) != 0)
        die(err);
    const uint32_t e = o.vde_dim;
    std::vector<double> pg, plg;
    read_data_vertices(o.dataset_path + "gnn-pge/data_vertices.bin", g, e, &pg, &plg);

    const auto tq = Clock::now();  // the query plan (main.cpp:248-331): gen_vde and the groups of the query vertices
    uint32_t n_qv = 0, *ql = nullptr, *qd = nullptr;
    double *qpg = nullptr, *qplg = nullptr;
    rc = gnnpe_host_pge_query_groups(o.query_graph.c_str(), e, &n_qv, &ql, &qd, &qpg, &qplg);
    if (rc == -1) {
        printf("%s\n", gnnpe_last_error());
        exit(-1);
    }
    if (rc != 0) die(o.query_graph + ": " + gnnpe_last_error());
    const double plan_ms = secs(tq, Clock::now()) * 1e3;

    if (gnnpe_device_count() <= 0) die("no HIP device: this tool has no CPU fallback");
    gnnpe_ctx *ctx = gnnpe_create(0);
    if (!ctx) die(std::string("gnnpe_create: ") + gnnpe_last_error());
    const uint32_t nl = std::max<uint32_t>(g.labels_count, 1);
    std::vector<double> table((size_t)nl * e);
    check(gnnpe_host_label_table(nl, e, table.data()), "label table");
    check(gnnpe_load_csr(ctx, g.n, g.offsets.data(), g.neighbors.data(), g.labels.data()), "load_csr");
    check(gnnpe_set_label_table(ctx, nl, e, table.data()), "set_label_table");
    check(gnnpe_pge_set_groups(ctx, pg.data(), plg.data()), "pge_set_groups");
    const uint64_t words = ((uint64_t)g.n + 31) / 32;
    std::vector<uint32_t> bitmap((size_t)n_qv * words);
    double ms = 0.0;
    check(gnnpe_pge_filter_candidates(ctx, n_qv, ql, qd, qpg, qplg, bitmap.data(), &ms), "pge_filter");
    gnnpe_host_free(ql);
    gnnpe_host_free(qd);
    gnnpe_host_free(qpg);
    gnnpe_host_free(qplg);
    if (o.mode == "online") {  // main.cpp:352-358: refinement on the united candidate sets, then the answer line
        uint64_t answers = 0;
        double refine_ms = 0.0;
        // the refinement lives in libgnnpe_online.so beside this binary (include/gnnpe_online.h), as for gnnpe_main -m online
        void *online = open_online(o.tool);
        check(ONLINE(gnnpe_refine)(ctx, o.query_graph.c_str(), bitmap.data(), limit, &answers, &refine_ms), "refine");
        gnnpe_destroy(ctx);
        printf("Answer Num: %llu Query Time (ms): %g\n", (unsigned long long)answers, plan_ms + ms + refine_ms);
        if (o.timing)
            fprintf(stderr, "{\"vertices\": %u, \"query_vertices\": %u, \"filter_device_ms\": %.3f, \"refine_ms\": %.3f, "
                            "\"end_to_end_s\": %.3f}\n",
                    g.n, n_qv, ms, refine_ms, secs(t0, Clock::now()));
        return 0;
    }
    gnnpe_destroy(ctx);
    // uint32 n_query_vertices; per query vertex uint32 count + ascending data vertex ids (what oracle-side refinement reads)
    const std::string out = o.dataset_path + "gnn-pge/candidates.bin";
    FILE *f = fopen(out.c_str(), "wb");
    if (!f) die("cannot write " + out);
    bool ok = fwrite(&n_qv, 4, 1, f) == 1;
    std::vector<uint32_t> ids;
    for (uint32_t u = 0; u < n_qv; u++) {
        ids.clear();
        for (uint64_t w = 0; w < words; w++)
            for (uint32_t bits = bitmap[(size_t)u * words + w]; bits; bits &= bits - 1)
                ids.push_back((uint32_t)(w * 32 + __builtin_ctz(bits)));
        const uint32_t c = (uint32_t)ids.size();
        ok = ok && fwrite(&c, 4, 1, f) == 1 && (!c || fwrite(ids.data(), 4, c, f) == c);
    }
    if (fclose(f) != 0 || !ok) die("write failed on " + out);
    if (o.timing)
        fprintf(stderr, "{\"vertices\": %u, \"query_vertices\": %u, \"filter_device_ms\": %.3f, \"end_to_end_s\": %.3f}\n", g.n,
                n_qv, ms, secs(t0, Clock::now()));
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    Options o = parse_args(argc, argv, "gnnpge_main");
    const auto t0 = Clock::now();
    // GNN-PGE/include/custom.h:47-49: path_length = 1 + 1 (vertices per path), pde_dim = vde_dim * path_length
    if (o.path_length != 2) die("-l " + std::to_string(o.path_length) + ": only the reference default (2) is supported");
    if (o.partition_num == 0) die("-p must be >= 1");
    if (!o.apply_edges_file.empty()) die("--apply-edges is an option of gnnpe_main's exact -m online / -m filter");
    if (!o.set_labels_file.empty()) die("--set-labels is an option of gnnpe_main's exact -m online / -m filter");
    if (!o.apply_vertices_file.empty()) die("--apply-vertices is an option of gnnpe_main's exact -m online / -m filter");
    if (o.incremental) die("--incremental is an option of gnnpe_main's exact -m online / -m filter");
    if (!o.delta_vertices_file.empty()) die("--delta-vertices is an option of gnnpe_main's --refine sets");
    if (o.delta_pages_given) die("--delta-pages is an option of gnnpe_main's --refine sets");
    if (o.mode == "online" || o.mode == "filter") return run_online(o);
    if (o.mode != "offline") return 0;

    gnnpe_host::StaticGraph g;
    std::string err;
    int rc = g.load(o.data_graph, &err, true);  // GNN-PGE: simple graphs only
    if (rc == -1) {  // graph.cpp:166-169
        printf("%s\n", err.c_str());
        exit(-1);
    }
    if (rc != 0) die(o.data_graph + ": " + err);
    std::vector<uint32_t> sorted_nodes, membership;
    if (gnnpe_host::read_membership(o.dataset_path + "gnn-pge/membership.txt", g.n, o.partition_num, &sorted_nodes, &membership,
                                    &err) != 0)
        die(err);
    const std::string partitions_path = o.dataset_path + "gnn-pge/partitions/";
    for (uint32_t i = 0; i < o.partition_num; i++)
        if (!is_dir(partitions_path + "partition-" + std::to_string(i)))
            die("missing directory " + partitions_path + "partition-" + std::to_string(i) + "/ (the prep step creates it)");
    // partition_vertices[membership[node]] in membership.txt order (main.cpp:86-89)
    std::vector<std::vector<uint32_t>> part(o.partition_num);
    for (uint32_t node : sorted_nodes) part[membership[node]].push_back(node);

    if (gnnpe_device_count() <= 0) die("no HIP device: this tool has no CPU fallback");
    gnnpe_ctx *ctx = gnnpe_create(0);
    if (!ctx) die(std::string("gnnpe_create: ") + gnnpe_last_error());
    const uint32_t e = o.vde_dim, nl = std::max<uint32_t>(g.labels_count, 1);
    std::vector<double> table((size_t)nl * e);
    check(gnnpe_host_label_table(nl, e, table.data()), "label table");
    check(gnnpe_load_csr(ctx, g.n, g.offsets.data(), g.neighbors.data(), g.labels.data()), "load_csr");
    check(gnnpe_set_label_table(ctx, nl, e, table.data()), "set_label_table");
    const size_t ne = (size_t)g.n * e;
    std::vector<double> x(ne), nx(ne), vde(ne), pg(ne * 4), plg(ne * 4);
    check(gnnpe_vde(ctx, x.data(), nx.data(), vde.data()), "vde");            // main.cpp:93
    check(gnnpe_pge_groups(ctx, pg.data(), plg.data()), "pge_groups");        // main.cpp:97-177
    const auto t1 = Clock::now();

    {  // main.cpp:179-194
        const std::string path = o.dataset_path + "gnn-pge/data_vertices.bin";
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) die("cannot open " + path + " for writing");
        const uint32_t D2 = 4 * e;
        std::vector<char> rec(12 + 8 + 8 * (3 * (size_t)e + 2 * D2));
        fwrite(&g.n, 4, 1, f);
        for (uint32_t v = 0; v < g.n; v++) {
            char *p = rec.data();
            const uint32_t deg = g.degree(v);
            const double key = 0.0;
            memcpy(p, &v, 4);
            memcpy(p + 4, &g.labels[v], 4);
            memcpy(p + 8, &deg, 4);
            memcpy(p + 12, &key, 8);
            p += 20;
            memcpy(p, &x[(size_t)v * e], 8 * e);
            memcpy(p + 8 * e, &nx[(size_t)v * e], 8 * e);
            memcpy(p + 16 * e, &vde[(size_t)v * e], 8 * e);
            p += 24 * e;
            memcpy(p, &pg[(size_t)v * D2], 8 * D2);
            memcpy(p + 8 * D2, &plg[(size_t)v * D2], 8 * D2);
            if (fwrite(rec.data(), 1, rec.size(), f) != rec.size()) die("write error on " + path);
        }
        if (fclose(f) != 0) die("write error on " + path);
    }
    const auto t2 = Clock::now();
    for (uint32_t i = 0; i < o.partition_num; i++)
        check(gnnpe_pge_build_index(ctx, part[i].size(), part[i].data(),
                                    (partitions_path + "partition-" + std::to_string(i) + "/index.dat").c_str()),
              "pge_build_index");
    const auto t3 = Clock::now();
    gnnpe_destroy(ctx);
    if (o.timing)
        fprintf(stderr, "{\"vertices\": %u, \"load_embed_group_s\": %.3f, \"write_bin_s\": %.3f, \"index_s\": %.3f, \"end_to_end_s\": %.3f}\n",
                g.n, secs(t0, t1), secs(t1, t2), secs(t2, t3), secs(t0, t3));
    return 0;
}
