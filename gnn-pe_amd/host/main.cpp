// main.cpp -- `gnnpe_main`: drop-in for the reference's `main -m offline` (GNN-PE/src/main.cpp:38-120).
//
// Same flags, same defaults, same input files and the same output files:
//   <f>gnn-pe/membership.txt                       (read;  main.cpp:77-85)
//   <f>gnn-pe/partitions/partition-i/partition_paths.txt   (written; main.cpp:98-108)
//   <f>/gnn-pe/all_paths.txt                       (written; main.cpp:110-119)
// The enumeration, embeddings and text rendering run on MI355X GPUs through the C-ABI in
// include/gnnpe_hip.h; this file is host orchestration and file I/O only.  `-m online` stays the
// reference's own binary for anyone who wants it: it consumes the files written here unchanged.  This tool's own
// `-m online -q <query.graph>` answers the query without any of those files: filter on the GPU, refinement on the
// device too (run_filter); `-m filter` stops after the filter and writes the candidate sets.
//
// Deliberate differences from the reference (all fail-loud instead of silent):
//   - missing membership.txt / partition directories are errors (the reference reads zeros /
//     writes nothing: main.cpp:80,101,110 never check their streams);
//   - `-l 3` writes 4-vertex paths (the rule of custom.h:66-92 with the DFS depth fixed; BASELINE config 5),
//     where the reference enumerates 3-vertex paths whatever -l says and prints a garbage 4th column
//     (SURVEY D4); its online binary cannot read those files.  `-m online|filter -l 3` queries with 4-vertex paths, in exact
//     mode (the reference has no l = 3 semantics to follow).  Other -l values are refused;
//   - path counts beyond 2^32-1 are refused unless --allow-large (the reference's `ui` overflows).
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gnnpe_hip.h"
#include "../../include/gnnpe_online.h"  // for the types of its functions only: the library is dlopen()ed (cli_common.h, ONLINE)
#include "cli_common.h"
#include "graph_loader.h"
#include "slab_offline.h"

using gnnpe_host::StaticGraph;

namespace {

using namespace cli;

// Grow-only host buffer in pinned memory: device-to-host copies into it run at PCIe speed instead of through the
// driver's pageable staging, and nothing is zero-filled on resize.
struct HostBuf {
    char *p = nullptr;
    size_t cap = 0, len = 0;
    ~HostBuf()
    {
        if (p) gnnpe_pinned_free(p);
    }
    void resize(size_t n)
    {
        if (n > cap) {
            if (p) gnnpe_pinned_free(p);
            p = nullptr;
            cap = std::max(n + n / 8, (size_t)1 << 20);
            void *q = nullptr;
            if (gnnpe_pinned_alloc(cap, &q) != 0) die(std::string("pinned host buffer: ") + gnnpe_last_error());
            p = (char *)q;
        }
        len = n;
    }
    char *data() { return p; }
    void assign(const std::string &s)
    {
        resize(s.size());
        memcpy(p, s.data(), s.size());
    }
};

// Background writer: the GPU renders chunk k+1 while chunk k goes to the file.
class FileSink {
public:
    explicit FileSink(const std::string &path) : path_(path)
    {
        f_ = fopen(path.c_str(), "wb");
        if (!f_) die("cannot open " + path + " for writing");
        setvbuf(f_, nullptr, _IOFBF, 8 << 20);
        th_ = std::thread([this] { run(); });
    }
    HostBuf *acquire()
    {  // a free buffer (two in flight)
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return pending_ < 2; });
        return &bufs_[next_++ & 1];
    }
    void submit(HostBuf *b, size_t n)
    {
        std::unique_lock<std::mutex> lk(mu_);
        queue_.push_back({b, n});
        pending_++;
        cv_.notify_all();
    }
    void write_now(const std::string &s) { submit_copy(s); }
    uint64_t close()
    {
        {
            std::unique_lock<std::mutex> lk(mu_);
            done_ = true;
            cv_.notify_all();
        }
        th_.join();
        if (fclose(f_) != 0 || failed_) die("write error on " + path_);
        return bytes_;
    }

private:
    void submit_copy(const std::string &s)
    {
        HostBuf *b = acquire();
        b->assign(s);
        submit(b, s.size());
    }
    void run()
    {
        for (;;) {
            std::pair<HostBuf *, size_t> item;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return !queue_.empty() || done_; });
                if (queue_.empty()) return;
                item = queue_.front();
                queue_.erase(queue_.begin());
            }
            if (item.second && fwrite(item.first->data(), 1, item.second, f_) != item.second) failed_ = true;
            bytes_ += item.second;
            {
                std::unique_lock<std::mutex> lk(mu_);
                pending_--;
                cv_.notify_all();
            }
        }
    }
    std::string path_;
    FILE *f_ = nullptr;
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<std::pair<HostBuf *, size_t>> queue_;
    HostBuf bufs_[2];
    int pending_ = 0, next_ = 0;
    bool done_ = false, failed_ = false;
    uint64_t bytes_ = 0;
};

struct Device {
    gnnpe_ctx *ctx = nullptr;
    uint32_t slab_begin = 0, slab_end = 0;
    uint64_t total = 0, base = 0;
};

// the file of --vertex-counts / --delta-vertex-counts: a line `v c_0 .. c_{nq-1}` for every data vertex with a count
void write_vertex_table(const std::string &path, const StaticGraph &g, uint32_t n_qv, const std::vector<uint64_t> &table)
{
    FILE *vf = fopen(path.c_str(), "w");
    if (!vf) die("cannot write " + path);
    for (uint32_t v = 0; v < g.n; v++) {
        bool any = false;
        for (uint32_t u = 0; u < n_qv && !any; u++) any = table[(size_t)u * g.n + v] != 0;
        if (!any) continue;
        fprintf(vf, "%u", v);
        for (uint32_t u = 0; u < n_qv; u++) fprintf(vf, " %llu", (unsigned long long)table[(size_t)u * g.n + v]);
        fputc('\n', vf);
    }
    if (fclose(vf) != 0) die("write failed on " + path);
}

// the file of --edge-counts / --delta-edge-counts: the query edges in a `#` line, then a line `x y c_0 .. c_{nqe-1}` for every
// adjacency entry with a count
void write_edge_table(const std::string &path, const StaticGraph &g, uint32_t nqe, const std::vector<uint32_t> &qe,
                      const std::vector<uint64_t> &table)
{
    const size_t entries = g.offsets[g.n];
    FILE *ef = fopen(path.c_str(), "w");
    if (!ef) die("cannot write " + path);
    fputc('#', ef);
    for (uint32_t k = 0; k < nqe; k++) fprintf(ef, " %u-%u", qe[2 * k], qe[2 * k + 1]);
    fputc('\n', ef);
    // the rows ascend, so the entries in CSR order are ascending by (x, y)
    for (uint32_t x = 0; x < g.n; x++)
        for (size_t j = g.offsets[x]; j < g.offsets[x + 1]; j++) {
            bool any = false;
            for (uint32_t k = 0; k < nqe && !any; k++) any = table[(size_t)k * entries + j] != 0;
            if (!any) continue;
            fprintf(ef, "%u %u", x, g.neighbors[j]);
            for (uint32_t k = 0; k < nqe; k++) fprintf(ef, " %llu", (unsigned long long)table[(size_t)k * entries + j]);
            fputc('\n', ef);
        }
    if (fclose(ef) != 0) die("write failed on " + path);
}

// F of --delta-edges and of --delta-nonedges: one `x y` per line
std::vector<uint32_t> read_delta_edges(const std::string &path)
{
    std::vector<uint32_t> pairs;
    FILE *df = fopen(path.c_str(), "r");
    if (!df) die("cannot read " + path);
    for (unsigned long long x, y;;) {
        const int got = fscanf(df, "%llu %llu", &x, &y);
        if (got == EOF) break;
        if (got != 2 || x > 0xFFFFFFFFull || y > 0xFFFFFFFFull) die(path + ": one `x y` per line expected");
        pairs.push_back((uint32_t)x);
        pairs.push_back((uint32_t)y);
    }
    fclose(df);
    return pairs;
}

// S of --delta-vertices: one vertex id per line
std::vector<uint32_t> read_vertex_list(const std::string &path)
{
    std::vector<uint32_t> ids;
    FILE *vf = fopen(path.c_str(), "r");
    if (!vf) die("cannot read " + path);
    for (unsigned long long v;;) {
        const int got = fscanf(vf, "%llu", &v);
        if (got == EOF) break;
        if (got != 1 || v > 0xFFFFFFFFull) die(path + ": one vertex id per line expected");
        ids.push_back((uint32_t)v);
    }
    fclose(vf);
    return ids;
}

// the file of --set-labels: one `v label` per line
void read_label_list(const std::string &path, std::vector<uint32_t> *vs, std::vector<uint32_t> *ls)
{
    FILE *lf = fopen(path.c_str(), "r");
    if (!lf) die("cannot read " + path);
    unsigned long long v = 0, lab = 0;
    for (int got; (got = fscanf(lf, "%llu %llu", &v, &lab)) != EOF;) {
        if (got != 2 || v > 0xFFFFFFFFull || lab > 0xFFFFFFFFull) die(path + ": one `v label` per line expected");
        vs->push_back((uint32_t)v);
        ls->push_back((uint32_t)lab);
    }
    fclose(lf);
}

// the file of --apply-vertices: one `- v` (remove the vertex) or `+ label` (add a vertex with that label) per line
void read_vertex_batch(const std::string &path, std::vector<uint32_t> *remove, std::vector<uint32_t> *add_labels)
{
    FILE *vf = fopen(path.c_str(), "r");
    if (!vf) die("cannot read " + path);
    char sign = 0;
    unsigned long long x = 0;
    for (int got; (got = fscanf(vf, " %c %llu", &sign, &x)) != EOF;) {
        if (got != 2 || (sign != '+' && sign != '-') || x > 0xFFFFFFFFull) die(path + ": one `- v` or `+ label` per line expected");
        (sign == '+' ? add_labels : remove)->push_back((uint32_t)x);
    }
    fclose(vf);
}

// the file of --matches: one match per line, the images of the query vertices in their order
struct MatchFile {
    const std::string &path;
    uint32_t n_qv;
    FILE *f;
    MatchFile(const std::string &path_, uint32_t n_qv_) : path(path_), n_qv(n_qv_), f(fopen(path_.c_str(), "w"))
    {
        if (!f) die("cannot write " + path);
    }
    void write(const std::vector<uint32_t> &rows, uint64_t n_rows)
    {
        for (uint64_t k = 0; k < n_rows; k++)
            for (uint32_t u = 0; u < n_qv; u++) fprintf(f, "%u%c", rows[(size_t)k * n_qv + u], u + 1 == n_qv ? '\n' : ' ');
    }
    void close()
    {
        if (fclose(f) != 0) die("write failed on " + path);
    }
};

// -m online, main.cpp:173-181: the refinement on the candidate sets.  On the device, through libgnnpe_online.so: gnnpe_refine,
// or with --refine sets, where the sets are complete, one of the set-restricted forms, all in the mode of --distinct (every
// matching subgraph once) and --induced (induced matches only, so that the answer is I or ID):
//   --all-matches            every match up to -n into --matches, page by page through the match cursor (gnnpe_refine_pages_*)
//   --vertex-counts FILE     gnnpe_refine_sets_vertex_counts: per data vertex the matches it takes part in, by query vertex
//   --edge-counts FILE       gnnpe_refine_sets_edge_counts: the same per adjacency entry and query edge
//   --delta-edges FILE       gnnpe_refine_sets_delta: the matches through the listed data edges, each once; with
//                            --delta-vertex-counts / --delta-edge-counts FILE gnnpe_refine_sets_delta_vertex_counts / _edge_counts,
//                            the count tables of those matches
//   --delta-nonedges FILE    gnnpe_refine_sets_delta_nonedges: the induced matches that put a non-adjacent query pair on one of
//                            the listed non-edges, each once; with --delta-vertex-counts / --delta-edge-counts FILE
//                            gnnpe_refine_sets_delta_nonedges_vertex_counts / _edge_counts, the count tables of those matches
//   --delta-vertices FILE    gnnpe_refine_sets_delta_vertices: the matches with an image among the listed data vertices, each once;
//                            with --delta-vertex-counts / --delta-edge-counts FILE gnnpe_refine_sets_delta_vertices_vertex_counts /
//                            _edge_counts, the count tables of those matches
//   --delta-pages ROWS       with one of the three --delta-* anchors: every match of the delta up to -n into --matches, ROWS per page
//                            through a delta cursor (gnnpe_refine_pages_open_delta, _open_delta_nonedges, _open_delta_vertices)
//   none of these            gnnpe_refine_sets_mode
// The four one-shot counts also write --matches, at most min(-n, 2^20) of them.  For a table -n is a guard: it is exact only below it.
struct Refinement {
    void *online = nullptr;  // the library's handle
    uint64_t answers = 0, n_written = 0, n_pages = 0;
    double refine_ms = 0.0;
};

Refinement refine_online(const Options &o, gnnpe_ctx *ctx, const StaticGraph &g, const std::vector<uint32_t> &bitmap, uint32_t n_qv,
                         uint64_t limit)
{
    Refinement r;
    void *online = r.online = open_online(o.tool);
    const char *query = o.query_graph.c_str();
    if (o.refine != "sets") {
        check(ONLINE(gnnpe_refine)(ctx, query, bitmap.data(), limit, &r.answers, &r.refine_ms), "refine");
        return r;
    }
    const uint32_t match_mode = (o.distinct ? GNNPE_MATCH_DISTINCT : 0u) | (o.induced ? GNNPE_MATCH_INDUCED : 0u);
    const bool nonedges = !o.delta_nonedges_file.empty(), through = !o.delta_edges_file.empty() || nonedges;
    const bool vertices = !o.delta_vertices_file.empty();
    const struct {
        const char *flag, *what;
        const std::string &path;
        bool edge_table;
    } tables[] = {{"--vertex-counts", "refine_sets_vertex_counts", o.vertex_counts_file, false},
                  {"--edge-counts", "refine_sets_edge_counts", o.edge_counts_file, true},
                  {"--delta-vertex-counts",
                   vertices   ? "refine_sets_delta_vertices_vertex_counts"
                   : nonedges ? "refine_sets_delta_nonedges_vertex_counts"
                              : "refine_sets_delta_vertex_counts",
                   o.delta_vertex_counts_file, false},
                  {"--delta-edge-counts",
                   vertices   ? "refine_sets_delta_vertices_edge_counts"
                   : nonedges ? "refine_sets_delta_nonedges_edge_counts"
                              : "refine_sets_delta_edge_counts",
                   o.delta_edge_counts_file, true}};
    for (const auto &t : tables) {
        if (t.path.empty()) continue;
        uint32_t nqe = 0;
        std::vector<uint32_t> qe((size_t)n_qv * n_qv + 2);
        if (t.edge_table) check(ONLINE(gnnpe_host_query_edges)(query, qe.data(), (uint32_t)(qe.size() / 2), &nqe), "host_query_edges");
        const std::vector<uint32_t> edges =
            through ? read_delta_edges(nonedges ? o.delta_nonedges_file : o.delta_edges_file) : std::vector<uint32_t>();
        std::vector<uint64_t> table(t.edge_table ? (size_t)nqe * g.offsets[g.n] : (size_t)n_qv * g.n);
        int complete = 0;
        if (vertices) {
            const std::vector<uint32_t> ids = read_vertex_list(o.delta_vertices_file);
            check((t.edge_table ? ONLINE(gnnpe_refine_sets_delta_vertices_edge_counts) : ONLINE(gnnpe_refine_sets_delta_vertices_vertex_counts))(
                      ctx, query, bitmap.data(), ids.data(), ids.size(), limit, match_mode, &r.answers, &complete, table.data(), nullptr,
                      nullptr, 1, &r.refine_ms), t.what);
        } else if (nonedges)
            check((t.edge_table ? ONLINE(gnnpe_refine_sets_delta_nonedges_edge_counts) : ONLINE(gnnpe_refine_sets_delta_nonedges_vertex_counts))(
                      ctx, query, bitmap.data(), edges.data(), edges.size() / 2, limit, match_mode, &r.answers, &complete, table.data(),
                      nullptr, nullptr, 1, &r.refine_ms), t.what);
        else if (through)
            check((t.edge_table ? ONLINE(gnnpe_refine_sets_delta_edge_counts) : ONLINE(gnnpe_refine_sets_delta_vertex_counts))(
                      ctx, query, bitmap.data(), edges.data(), edges.size() / 2, limit, match_mode, &r.answers, &complete, table.data(),
                      nullptr, nullptr, 1, &r.refine_ms), t.what);
        else
            check((t.edge_table ? ONLINE(gnnpe_refine_sets_edge_counts) : ONLINE(gnnpe_refine_sets_vertex_counts))(
                      ctx, query, bitmap.data(), limit, match_mode, &r.answers, &complete, table.data(), nullptr, &r.refine_ms), t.what);
        if (!complete)
            die(std::string(t.flag) + ": the matches reached -n " + std::to_string(limit) + ", so the table is not complete and " + t.path +
                " was not written; raise -n");
        if (t.edge_table) write_edge_table(t.path, g, nqe, qe, table);
        else write_vertex_table(t.path, g, n_qv, table);
        return r;
    }
    if (o.all_matches) {  // one page on the host at a time
        const uint64_t page = std::min<uint64_t>(o.match_page, std::max<uint64_t>(limit, 1));
        gnnpe_match_cursor *cur = nullptr;
        check(ONLINE(gnnpe_refine_pages_open_mode)(ctx, query, bitmap.data(), limit, page, match_mode, &cur), "refine_pages_open");
        const auto pages_next = ONLINE(gnnpe_refine_pages_next);
        MatchFile mf(o.matches_file, n_qv);
        std::vector<uint32_t> rows((size_t)page * n_qv);
        for (int done = 0; !done;) {
            uint64_t got = 0;
            double page_ms = 0.0;
            check(pages_next(cur, rows.data(), &got, &done, &page_ms), "refine_pages_next");
            mf.write(rows, got);
            r.answers += got;
            r.refine_ms += page_ms;
            r.n_pages++;
        }
        ONLINE(gnnpe_refine_pages_close)(cur);
        mf.close();
        r.n_written = r.answers;
        return r;
    }
    if (o.delta_pages_given) {  // the delta through a cursor, one page on the host at a time
        const uint64_t page = std::min<uint64_t>(o.delta_pages, std::max<uint64_t>(limit, 1));
        gnnpe_match_cursor *cur = nullptr;
        if (vertices) {
            const std::vector<uint32_t> ids = read_vertex_list(o.delta_vertices_file);
            check(ONLINE(gnnpe_refine_pages_open_delta_vertices)(ctx, query, bitmap.data(), ids.data(), ids.size(), limit, page, match_mode, &cur),
                  "refine_pages_open_delta_vertices");
        } else {
            const std::vector<uint32_t> pairs = read_delta_edges(nonedges ? o.delta_nonedges_file : o.delta_edges_file);
            check((nonedges ? ONLINE(gnnpe_refine_pages_open_delta_nonedges) : ONLINE(gnnpe_refine_pages_open_delta))(
                      ctx, query, bitmap.data(), pairs.data(), pairs.size() / 2, limit, page, match_mode, &cur),
                  nonedges ? "refine_pages_open_delta_nonedges" : "refine_pages_open_delta");
        }
        const auto pages_next = ONLINE(gnnpe_refine_pages_next);
        MatchFile mf(o.matches_file, n_qv);
        std::vector<uint32_t> rows((size_t)page * n_qv);
        for (int done = 0; !done;) {
            uint64_t got = 0;
            double page_ms = 0.0;
            check(pages_next(cur, rows.data(), &got, &done, &page_ms), "refine_pages_next");
            mf.write(rows, got);
            r.answers += got;
            r.refine_ms += page_ms;
            r.n_pages++;
        }
        ONLINE(gnnpe_refine_pages_close)(cur);
        mf.close();
        r.n_written = r.answers;
        return r;
    }
    const uint64_t cap = o.matches_file.empty() ? 0 : std::min<uint64_t>(limit, 1ull << 20);
    std::vector<uint32_t> rows((size_t)cap * n_qv);
    if (!o.delta_edges_file.empty()) {
        const std::vector<uint32_t> edges = read_delta_edges(o.delta_edges_file);
        check(ONLINE(gnnpe_refine_sets_delta)(ctx, query, bitmap.data(), edges.data(), edges.size() / 2, limit, match_mode, &r.answers,
                                              cap ? rows.data() : nullptr, cap, &r.refine_ms), "refine_sets_delta");
    } else if (nonedges) {
        const std::vector<uint32_t> pairs = read_delta_edges(o.delta_nonedges_file);
        check(ONLINE(gnnpe_refine_sets_delta_nonedges)(ctx, query, bitmap.data(), pairs.data(), pairs.size() / 2, limit, match_mode, &r.answers,
                                                       cap ? rows.data() : nullptr, cap, &r.refine_ms), "refine_sets_delta_nonedges");
    } else if (!o.delta_vertices_file.empty()) {
        const std::vector<uint32_t> ids = read_vertex_list(o.delta_vertices_file);
        check(ONLINE(gnnpe_refine_sets_delta_vertices)(ctx, query, bitmap.data(), ids.data(), ids.size(), limit, match_mode, &r.answers,
                                                       cap ? rows.data() : nullptr, cap, &r.refine_ms), "refine_sets_delta_vertices");
    } else {
        check(ONLINE(gnnpe_refine_sets_mode)(ctx, query, bitmap.data(), limit, match_mode, &r.answers, cap ? rows.data() : nullptr, cap,
                                             &r.refine_ms), "refine_sets");
    }
    if (!o.matches_file.empty()) {
        MatchFile mf(o.matches_file, n_qv);
        mf.write(rows, r.n_written = std::min(r.answers, cap));
        mf.close();
    }
    return r;
}

// a file of --apply-edges: one `+ x y` (insert) or `- x y` (delete) per line
static void read_edge_batch(const std::string &path, std::vector<uint32_t> *ins, std::vector<uint32_t> *del)
{
    FILE *af = fopen(path.c_str(), "r");
    if (!af) die("cannot read " + path);
    char sign = 0;
    unsigned long long x = 0, y = 0;
    for (int got; (got = fscanf(af, " %c %llu %llu", &sign, &x, &y)) != EOF;) {
        if (got != 3 || (sign != '+' && sign != '-') || x > 0xFFFFFFFFull || y > 0xFFFFFFFFull)
            die(path + ": one `+ x y` or `- x y` per line expected");
        std::vector<uint32_t> &to = sign == '+' ? *ins : *del;
        to.push_back((uint32_t)x);
        to.push_back((uint32_t)y);
    }
    fclose(af);
}

// -m online --exact [-l 3] --standing with one or more of --apply-edges FILE, --set-labels FILE, --apply-vertices FILE, each
// repeatable: a standing exact query (gnnpe_standing_open, with --distinct / --induced in its mode) opened on the graph as loaded
// and carried through the batches in command-line order, one gnnpe_standing_apply_edges, gnnpe_standing_set_labels or
// gnnpe_standing_apply_vertices each.  Prints `standing: count created destroyed device_ms` for the open (created = destroyed = 0)
// and after every batch.  No order and no membership.txt are read: the support calls need none.
int run_standing(const Options &o)
{
    StaticGraph g;
    std::string err;
    int rc = g.load(o.data_graph, &err, o.strict);
    if (rc == -1) {
        printf("%s\n", err.c_str());
        exit(-1);
    }
    if (rc != 0) die(o.data_graph + ": " + err);
    if (!g.simple) die(o.data_graph + " repeats an edge (duplicate `e` lines): --standing needs a simple graph");
    // per batch two lists: insertions and deletions (pairs), vertices and labels, or removed vertices and added labels
    std::vector<std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> batches(o.standing_batches.size());
    for (size_t i = 0; i < batches.size(); i++) {  // before a GPU is touched
        const char kind = o.standing_batches[i].first;
        if (kind == 'p' || kind == 't') continue;  // --peel T, --truss-levels FILE: no batch file to read
        (kind == 'e' ? read_edge_batch : kind == 'l' ? read_label_list : read_vertex_batch)(o.standing_batches[i].second, &batches[i].first, &batches[i].second);
    }
    if (gnnpe_device_count() <= 0) die("no HIP device: this tool has no CPU fallback");
    gnnpe_ctx *ctx = gnnpe_create(0);
    if (!ctx) die(std::string("gnnpe_create: ") + gnnpe_last_error());
    check(load_graph_into(ctx, g), "load_csr");
    const uint32_t n_labels = std::max<uint32_t>(g.labels_count, 1);
    std::vector<double> table((size_t)n_labels * o.vde_dim);
    check(gnnpe_host_label_table(n_labels, o.vde_dim, table.data()), "label table");
    check(gnnpe_set_label_table(ctx, n_labels, o.vde_dim, table.data()), "set_label_table");
    check(gnnpe_vde(ctx, nullptr, nullptr, nullptr), "vde");
    void *online = open_online(o.tool);
    const uint32_t mode = (o.distinct ? GNNPE_MATCH_DISTINCT : 0u) | (o.induced ? GNNPE_MATCH_INDUCED : 0u);
    gnnpe_standing *sq = nullptr;
    uint64_t count = 0;
    double ms = 0.0;
    check(ONLINE(gnnpe_standing_open)(ctx, o.query_graph.c_str(), o.path_length, 1e-6, mode, 0, &sq, &count, &ms), "standing_open");
    printf("standing: %llu 0 0 %.3f\n", (unsigned long long)count, ms);
    // --standing-vertex-counts / --standing-edge-counts: the handle keeps the tables; only the number of changed cells is asked for
    const uint32_t keep = (o.standing_vertex_counts_file.empty() ? 0u : GNNPE_STANDING_VERTEX_COUNTS) |
                          (o.standing_edge_counts_file.empty() ? 0u : GNNPE_STANDING_EDGE_COUNTS);
    // --peel / --truss-levels select on the kept E; the `changes:` lines and the table files stay those of the two flags above
    if (keep || o.standing_peels)
        check(ONLINE(gnnpe_standing_keep_counts)(sq, keep | (o.standing_peels ? GNNPE_STANDING_EDGE_COUNTS : 0u), 0, nullptr), "standing_keep_counts");
    const auto apply = ONLINE(gnnpe_standing_apply_edges);
    const auto relabel = ONLINE(gnnpe_standing_set_labels);
    const auto apply_vertices = ONLINE(gnnpe_standing_apply_vertices);
    const auto result = ONLINE(gnnpe_standing_result);
    const auto changes = ONLINE(gnnpe_standing_count_changes);
    for (size_t i = 0; i < batches.size(); i++) {
        const std::vector<uint32_t> &a = batches[i].first, &b = batches[i].second;
        const char kind = o.standing_batches[i].first;
        const std::string &file = o.standing_batches[i].second;
        if (kind == 'p' || kind == 't') {  // a peel by edge support, or the truss level of every edge (the graph is restored)
            uint64_t held_rows = 0, entries = 0, res[4], out[6];
            uint32_t hubs = 0;
            check(gnnpe_rows_held(ctx, &held_rows, &entries, &hubs), "rows_held");
            const uint64_t cap = entries / 2;
            std::vector<uint32_t> pairs(2 * cap + 2), rounds(cap + 1);
            std::vector<uint64_t> levels(cap + 1);
            std::string out_file = kind == 't' ? file : "";
            for (const auto &po : o.standing_peel_outs)
                if (po.first == i) out_file = po.second;
            if (kind == 'p')
                check(ONLINE(gnnpe_standing_peel)(sq, strtoull(file.c_str(), nullptr, 10), 0, pairs.data(), rounds.data(), cap, res, &ms), ("--peel " + file).c_str());
            else
                check(ONLINE(gnnpe_standing_truss_levels)(sq, 1, pairs.data(), levels.data(), cap, res, &ms), ("--truss-levels " + file).c_str());
            check(result(sq, out), "standing_result");
            if (kind == 'p')
                printf("peel: %llu %llu %llu %llu %llu %.3f\n", (unsigned long long)res[0], (unsigned long long)res[1], (unsigned long long)res[2],
                       (unsigned long long)res[3], (unsigned long long)out[0], ms);
            else
                printf("truss: %llu %llu %llu %llu %.3f\n", (unsigned long long)res[0], (unsigned long long)res[1], (unsigned long long)res[2],
                       (unsigned long long)res[3], ms);
            if (!out_file.empty()) {
                FILE *f = fopen(out_file.c_str(), "w");
                if (!f) die("cannot write " + out_file);
                const uint64_t k = kind == 'p' ? res[1] : res[0];
                for (uint64_t e = 0; e < k; e++)
                    fprintf(f, "%u %u %llu\n", pairs[2 * e], pairs[2 * e + 1], kind == 'p' ? (unsigned long long)rounds[e] : (unsigned long long)levels[e]);
                fclose(f);
            }
            continue;
        }
        if (kind == 'e') check(apply(ctx, a.data(), a.size() / 2, b.data(), b.size() / 2, &ms), ("--apply-edges " + file).c_str());
        else if (kind == 'l') check(relabel(ctx, a.data(), b.data(), a.size(), &ms), ("--set-labels " + file).c_str());
        else check(apply_vertices(ctx, a.data(), a.size(), b.data(), b.size(), &g.n, &ms), ("--apply-vertices " + file).c_str());
        uint64_t out[6];
        check(result(sq, out), "standing_result");
        printf("standing: %llu %llu %llu %.3f\n", (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], ms);
        if (keep) {
            uint64_t total = 0;
            for (uint32_t which : {GNNPE_STANDING_VERTEX_COUNTS, GNNPE_STANDING_EDGE_COUNTS}) {
                uint64_t n_changes = 0;
                if (keep & which) check(changes(sq, which, nullptr, nullptr, 0, &n_changes), "standing_count_changes");
                total += n_changes;
            }
            printf("changes: %llu\n", (unsigned long long)total);
        }
    }
    if (keep) {  // the tables after the last batch, on the graph as it is now (g.n: as the last vertex batch left it)
        uint64_t entries = 0;
        g.offsets.assign((size_t)g.n + 1, 0);
        (void)gnnpe_csr_download(ctx, g.offsets.data(), nullptr, 0, &entries);  // no room: refused with the entry count set
        g.neighbors.assign(entries, 0);
        check(gnnpe_csr_download(ctx, g.offsets.data(), g.neighbors.data(), entries, &entries), "csr_download");
        const auto counts = ONLINE(gnnpe_standing_counts);
        uint64_t rows = 0, cols = 0;
        if (keep & GNNPE_STANDING_VERTEX_COUNTS) {
            check(counts(sq, GNNPE_STANDING_VERTEX_COUNTS, nullptr, nullptr, &rows, &cols), "standing_counts");
            std::vector<uint64_t> table(rows * cols);
            check(counts(sq, GNNPE_STANDING_VERTEX_COUNTS, table.data(), nullptr, nullptr, nullptr), "standing_counts");
            write_vertex_table(o.standing_vertex_counts_file, g, (uint32_t)rows, table);
        }
        if (keep & GNNPE_STANDING_EDGE_COUNTS) {
            check(counts(sq, GNNPE_STANDING_EDGE_COUNTS, nullptr, nullptr, &rows, &cols), "standing_counts");
            if (cols != entries) die("--standing-edge-counts: the table has " + std::to_string(cols) + " columns, the graph " + std::to_string(entries) + " entries");
            std::vector<uint64_t> table(rows * cols);
            check(counts(sq, GNNPE_STANDING_EDGE_COUNTS, table.data(), nullptr, nullptr, nullptr), "standing_counts");
            uint32_t nqe = 0;
            std::vector<uint32_t> qe(2 * (size_t)rows + 2);
            check(ONLINE(gnnpe_host_query_edges)(o.query_graph.c_str(), qe.data(), (uint32_t)(qe.size() / 2), &nqe), "host_query_edges");
            write_edge_table(o.standing_edge_counts_file, g, nqe, qe, table);
        }
    }
    check(ONLINE(gnnpe_standing_close)(sq), "standing_close");
    gnnpe_destroy(ctx);
    return 0;
}

// Exact mode (--exact at -l 2, always at -l 3): the plan of gnnpe_host_query_plan_exact, every path tested in
// both orientations, so that the refinement counts every embedding.  Same answer line and candidates.bin; --timing adds the plan
// sizes by path width and the candidate count of every query vertex.
//
// -m online / -m filter: the reference's `-m online` (main.cpp:121-185) without its files.  Filter on the GPU -- query plan on the host
// (dfs_query / gen_query_pde), then the leaf test of Partition::query over every enumerated data path.  No
// all_paths.txt, no index.dat: only the data graph and membership.txt (any order gives the same candidate sets).
// Writes <f>gnn-pe/candidates.bin: uint32 n_query_vertices; per query vertex uint32 count + ascending data vertex
// ids -- the reference's candidate_set, ready for its refinement (main.cpp:176-179).  -m online goes on with the
// refinement on the device (refine_online) and prints the reference's answer line instead of writing the file, with --distinct
// a second line `Automorphisms: K`.
int run_standing(const Options &o);

int run_filter(const Options &o)
{
    if (o.standing) return run_standing(o);
    const auto t0 = Clock::now();
    const bool exact = o.exact || o.path_length == 3;  // (main() admits -l 2 and -l 3 only)
    StaticGraph g;
    std::string err;
    int rc = g.load(o.data_graph, &err, o.strict);
    if (rc == -1) {
        printf("%s\n", err.c_str());
        exit(-1);
    }
    if (rc != 0) die(o.data_graph + ": " + err);
    if (exact && o.mode == "online" && !g.simple)  // the refinement counts embeddings in simple graphs only (gnnpe_refine)
        die(o.data_graph + " repeats an edge (duplicate `e` lines): exact -m online (--exact, -l 3) needs a simple graph");
    // with --apply-vertices, --apply-edges or --set-labels the metadata block and the plan size are printed once the batches are
    // applied and the labels are set: they describe the graph the answer is for
    const bool updating = !o.apply_vertices_file.empty() || !o.apply_edges_file.empty() || !o.set_labels_file.empty();
    if (!updating) fputs(g.metadata_text().c_str(), stdout);
    std::vector<uint32_t> sorted_nodes, membership;
    if (gnnpe_host::read_membership(o.dataset_path + "gnn-pe/membership.txt", g.n, o.partition_num, &sorted_nodes,
                                    &membership, &err) != 0)
        die(err);
    uint32_t n_qv = 0, n_qp = 0, *qv = nullptr, *ql = nullptr, *qd = nullptr, counts[3] = {0, 0, 0};
    double *qp = nullptr;
    if (exact) {
        rc = gnnpe_host_query_plan_exact(o.query_graph.c_str(), o.vde_dim, o.path_length, &n_qv, counts, &qv, &ql, &qd, &qp);
        n_qp = counts[0];
    } else {
        rc = gnnpe_host_query_plan(o.query_graph.c_str(), o.vde_dim, &n_qv, &n_qp, &qv, &ql, &qd, &qp);
    }
    if (rc == -1) {
        printf("%s\n", gnnpe_last_error());
        exit(-1);
    }
    if (rc != 0) die(o.query_graph + ": " + gnnpe_last_error());
    if (!updating) printf("%u\n", n_qp);  // gen_query_pde prints the plan size (custom.h:629)
    if (gnnpe_device_count() <= 0) die("no HIP device: this tool has no CPU fallback");
    gnnpe_ctx *ctx = gnnpe_create(0);
    if (!ctx) die(std::string("gnnpe_create: ") + gnnpe_last_error());
    check(load_graph_into(ctx, g), "load_csr");
    // the host copy follows the device (g.n is set by the caller): the count tables below are indexed by the entries of the CSR the
    // context holds
    auto follow_rows = [&](uint64_t entries) {
        g.offsets.assign((size_t)g.n + 1, 0);
        g.neighbors.assign(entries, 0);
        check(gnnpe_csr_download(ctx, g.offsets.data(), g.neighbors.data(), entries, &entries), "csr_download");
        g.m = (uint32_t)(entries / 2);
        g.max_degree = 0;
        for (uint32_t v = 0; v < g.n; v++) g.max_degree = std::max(g.max_degree, g.offsets[v + 1] - g.offsets[v]);
    };
    // ... with the label figures of the metadata block (graph.cpp:223)
    auto follow_labels = [&]() {
        g.labels.assign(g.n, 0);
        check(gnnpe_labels_download(ctx, g.labels.data()), "labels_download");
        std::map<uint32_t, uint32_t> freq;
        uint32_t max_label = 0;
        for (uint32_t x = 0; x < g.n; x++) {
            freq[g.labels[x]]++;
            max_label = std::max(max_label, g.labels[x]);
        }
        g.labels_count = std::max<uint32_t>((uint32_t)freq.size(), g.n ? max_label + 1 : 0);
        g.max_label_frequency = 0;
        for (const auto &kv : freq) g.max_label_frequency = std::max(g.max_label_frequency, kv.second);
    };
    // --incremental: the support table S of the exact filter on the graph as loaded, then around every batch S -= S_T(G), the batch,
    // gnnpe_vde, S += S_T'(G') (the loops of include/gnnpe_hip.h); the bitmap below is derived from S.  The label table is set
    // once, with a row for every label a batch can bring: a row depends on its label alone, so the embeddings are those of the
    // table the plain run sets after the batches
    void *support = nullptr;
    double support_ms = 0.0;
    auto support_delta = [&](const std::vector<uint32_t> &T, int sign) {
        double ms1 = 0.0;
        check(gnnpe_filter_support_exact_delta(ctx, o.path_length, counts, qv, ql, qd, qp, n_qv, 1e-6, T.data(), T.size(), sign, support, &ms1),
              "filter_support_exact_delta");
        support_ms += ms1;
    };
    auto with_neighbours = [&](const std::vector<uint32_t> &R) {  // R u N(R) in the host copy of the graph
        std::vector<uint32_t> T(R);
        for (uint32_t v : R)
            if (v < g.n) T.insert(T.end(), g.neighbors.begin() + g.offsets[v], g.neighbors.begin() + g.offsets[v + 1]);
        return T;
    };
    if (o.incremental) {
        uint32_t n_labels = std::max<uint32_t>(g.labels_count, 1);
        if (!o.apply_vertices_file.empty()) {
            std::vector<uint32_t> rem, add;
            read_vertex_batch(o.apply_vertices_file, &rem, &add);
            for (uint32_t lab : add) n_labels = std::max(n_labels, lab + 1);
        }
        if (!o.set_labels_file.empty()) {
            std::vector<uint32_t> vs, ls;
            read_label_list(o.set_labels_file, &vs, &ls);
            for (uint32_t lab : ls) n_labels = std::max(n_labels, lab + 1);
        }
        std::vector<double> table((size_t)n_labels * o.vde_dim);
        check(gnnpe_host_label_table(n_labels, o.vde_dim, table.data()), "label table");
        check(gnnpe_set_label_table(ctx, n_labels, o.vde_dim, table.data()), "set_label_table");
        check(gnnpe_vde(ctx, nullptr, nullptr, nullptr), "vde");
        check(gnnpe_dev_alloc(ctx, (uint64_t)n_qv * g.n * 8, &support), "support table");
        check(gnnpe_filter_support_exact(ctx, o.path_length, counts, qv, ql, qd, qp, n_qv, 1e-6, support, nullptr), "filter_support_exact");
    }
    if (!o.apply_vertices_file.empty()) {  // first: an edge file may name the new ids
        std::vector<uint32_t> rem, add;
        read_vertex_batch(o.apply_vertices_file, &rem, &add);
        uint32_t n2 = 0;
        uint64_t entries = 0;
        void *dev_vmap = nullptr;
        std::vector<uint32_t> touched;  // R u N_G(R), ids of G
        if (o.incremental) {
            for (uint32_t v : rem)
                if (v >= g.n) die("--apply-vertices: vertex " + std::to_string(v) + " is not a vertex of the graph");
            touched = with_neighbours(rem);
            support_delta(touched, -1);
        }
        check(gnnpe_csr_apply_vertices(ctx, rem.data(), rem.size(), add.data(), add.size(), &n2, nullptr, &entries, &dev_vmap, nullptr, nullptr),
              "--apply-vertices");
        std::vector<uint32_t> vmap(n2);
        check(gnnpe_copy_to_host(ctx, vmap.data(), dev_vmap, (uint64_t)n2 * 4), "vertex map");
        if (o.incremental) {  // the table through the vertex map (the columns of R hold zero by now), then the paths of G' through T'
            void *carried = nullptr;
            check(gnnpe_dev_alloc(ctx, (uint64_t)n_qv * n2 * 8, &carried), "support table");
            check(gnnpe_csr_carry_vertices(ctx, n_qv, 8, support, carried, nullptr), "carry_vertices");
            check(gnnpe_dev_free(ctx, support), "support table");
            support = carried;
            check(gnnpe_vde(ctx, nullptr, nullptr, nullptr), "vde");
            std::vector<uint32_t> new_of(g.n, GNNPE_NO_VERTEX), after;
            for (uint32_t v = 0; v < n2; v++) {
                if (vmap[v] != GNNPE_NO_VERTEX) new_of[vmap[v]] = v;
                else after.push_back(v);
            }
            for (uint32_t v : touched)
                if (new_of[v] != GNNPE_NO_VERTEX) after.push_back(new_of[v]);
            support_delta(after, +1);
        }
        // order and membership through the vertex map: the survivors in their old order, the added vertices behind them in partition 0
        // (exact mode's candidate sets do not depend on the order)
        std::vector<uint32_t> new_id(g.n, GNNPE_NO_VERTEX), order, member(n2, 0);
        for (uint32_t v = 0; v < n2; v++)
            if (vmap[v] != GNNPE_NO_VERTEX) {
                new_id[vmap[v]] = v;
                member[v] = membership[vmap[v]];
            }
        for (uint32_t v : sorted_nodes)
            if (new_id[v] != GNNPE_NO_VERTEX) order.push_back(new_id[v]);
        for (uint32_t v = 0; v < n2; v++)
            if (vmap[v] == GNNPE_NO_VERTEX) order.push_back(v);
        sorted_nodes.swap(order);
        membership.swap(member);
        g.n = n2;
        follow_rows(entries);
        follow_labels();
    }
    if (!o.apply_edges_file.empty()) {  // the whole query runs on the updated graph
        std::vector<uint32_t> ins, del;
        read_edge_batch(o.apply_edges_file, &ins, &del);
        uint64_t entries = 0;
        std::vector<uint32_t> ends(ins);  // T: the end vertices of the batch
        ends.insert(ends.end(), del.begin(), del.end());
        if (o.incremental) {
            for (uint32_t v : ends)
                if (v >= g.n) die("--apply-edges: vertex " + std::to_string(v) + " is not a vertex of the graph");
            support_delta(ends, -1);
        }
        check(gnnpe_csr_apply_edges(ctx, ins.data(), ins.size() / 2, del.data(), del.size() / 2, &entries, nullptr), "--apply-edges");
        if (o.incremental) {
            check(gnnpe_vde(ctx, nullptr, nullptr, nullptr), "vde");
            support_delta(ends, +1);
        }
        follow_rows(entries);
    }
    if (!o.set_labels_file.empty()) {  // ... and on the relabelled one
        std::vector<uint32_t> vs, ls;
        read_label_list(o.set_labels_file, &vs, &ls);
        std::vector<uint32_t> touched;  // T = R u N(R): the embedding of a neighbour changes too
        if (o.incremental) {
            for (uint32_t v : vs)
                if (v >= g.n) die("--set-labels: vertex " + std::to_string(v) + " is not a vertex of the graph");
            touched = with_neighbours(vs);
            support_delta(touched, -1);
        }
        check(gnnpe_set_vertex_labels(ctx, vs.data(), ls.data(), vs.size(), nullptr), "--set-labels");
        if (o.incremental) {
            check(gnnpe_vde(ctx, nullptr, nullptr, nullptr), "vde");
            support_delta(touched, +1);
        }
        follow_labels();
    }
    if (updating) {
        fputs(g.metadata_text().c_str(), stdout);
        printf("%u\n", n_qp);
    }
    const uint32_t n_labels = std::max<uint32_t>(g.labels_count, 1);
    std::vector<double> table((size_t)n_labels * o.vde_dim);
    check(gnnpe_host_label_table(n_labels, o.vde_dim, table.data()), "label table");
    check(gnnpe_set_order(ctx, sorted_nodes.data(), membership.data(), o.partition_num), "set_order");
    check(gnnpe_set_label_table(ctx, n_labels, o.vde_dim, table.data()), "set_label_table");
    check(gnnpe_vde(ctx, nullptr, nullptr, nullptr), "vde");
    uint64_t P = 0;
    check(gnnpe_count_paths(ctx, o.path_length, nullptr, &P), "count_paths");
    const uint64_t words = ((uint64_t)g.n + 31) / 32;
    std::vector<uint32_t> bitmap((size_t)n_qv * words);
    double ms = 0.0;
    if (o.incremental) {  // the sets of the updated graph from the table carried to it; ms: the delta calls and this one
        check(gnnpe_filter_support_bitmap(ctx, n_qv, support, bitmap.data(), &ms), "filter_support_bitmap");
        ms += support_ms;
        check(gnnpe_dev_free(ctx, support), "support table");
    } else if (exact)
        check(gnnpe_filter_candidates_exact(ctx, o.path_length, counts, qv, ql, qd, qp, n_qv, 1e-6, bitmap.data(), &ms), "filter");
    else
        check(gnnpe_filter_candidates(ctx, n_qp, qv, ql, qd, qp, n_qv, 1e-6 /* custom.h:43 */, bitmap.data(), &ms), "filter");
    // --timing in exact mode: plan sizes by path width, candidates per query vertex (the reference mode's line is unchanged)
    std::string exact_json;
    if (exact && o.timing) {
        const uint32_t W = o.path_length + 1;
        exact_json = "\"exact\": true, \"l\": " + std::to_string(o.path_length) + ", \"plan_paths_by_width\": {\"" +
                     std::to_string(W) + "\": " + std::to_string(counts[0]);
        if (W != 3) exact_json += ", \"3\": " + std::to_string(counts[1]);
        exact_json += ", \"1\": " + std::to_string(counts[2]) + "}, \"candidates\": [";
        for (uint32_t u = 0; u < n_qv; u++) {
            uint64_t k = 0;
            for (uint64_t w = 0; w < words; w++) k += __builtin_popcount(bitmap[(size_t)u * words + w]);
            exact_json += (u ? ", " : "") + std::to_string(k);
        }
        exact_json += "], ";
    }
    if (o.mode == "online") {  // main.cpp:173-181: refinement on the candidate sets, then the answer line
        uint64_t limit = 0xFFFFFFFFull;  // MAX_LIMIT = UINT_MAX (main.cpp:62-69)
        if (o.answers != "MAX") {
            uint32_t lim;
            if (!parse_u32(o.answers, &lim)) die("-n must be MAX or an integer");
            limit = lim;
        }
        const Refinement r = refine_online(o, ctx, g, bitmap, n_qv, limit);
        const bool sets = o.refine == "sets";
        gnnpe_destroy(ctx);
        printf("Answer Number: %llu Query Time (ms): %g\n", (unsigned long long)r.answers, ms + r.refine_ms);
        if (o.distinct) {
            // the answer is the number of distinct subgraphs; times the automorphisms it is the number of embeddings
            void *online = r.online;
            uint64_t aut = 0;
            std::vector<uint32_t> pairs((size_t)n_qv * n_qv);
            uint32_t n_pairs = 0;
            check(ONLINE(gnnpe_host_query_symmetry)(o.query_graph.c_str(), &aut, pairs.data(), (uint32_t)(pairs.size() / 2), &n_pairs),
                  "query_symmetry");
            printf("Automorphisms: %llu\n", (unsigned long long)aut);
        }
        if (o.induced) exact_json += "\"induced\": true, ";
        if (o.timing && sets && (o.all_matches || o.delta_pages_given))
            fprintf(stderr, "{%s\"refine\": \"sets\", \"matches_written\": %llu, \"match_pages\": %llu, \"paths\": %llu, "
                            "\"query_paths\": %u, \"filter_device_ms\": %.3f, \"refine_ms\": %.3f, \"end_to_end_s\": %.3f}\n",
                    exact_json.c_str(), (unsigned long long)r.n_written, (unsigned long long)r.n_pages, (unsigned long long)P, n_qp, ms,
                    r.refine_ms, secs(t0, Clock::now()));
        else if (o.timing && sets)
            fprintf(stderr, "{%s\"refine\": \"sets\", \"matches_written\": %llu, \"paths\": %llu, \"query_paths\": %u, "
                            "\"filter_device_ms\": %.3f, \"refine_ms\": %.3f, \"end_to_end_s\": %.3f}\n",
                    exact_json.c_str(), (unsigned long long)r.n_written, (unsigned long long)P, n_qp, ms, r.refine_ms,
                    secs(t0, Clock::now()));
        else if (o.timing)
            fprintf(stderr, "{%s\"paths\": %llu, \"query_paths\": %u, \"filter_device_ms\": %.3f, \"refine_ms\": %.3f, "
                            "\"end_to_end_s\": %.3f}\n",
                    exact_json.c_str(), (unsigned long long)P, n_qp, ms, r.refine_ms, secs(t0, Clock::now()));
        gnnpe_host_free(qv);
        gnnpe_host_free(ql);
        gnnpe_host_free(qd);
        gnnpe_host_free(qp);
        return 0;
    }
    gnnpe_destroy(ctx);
    const std::string out = o.dataset_path + "gnn-pe/candidates.bin";
    FILE *f = fopen(out.c_str(), "wb");
    if (!f) die("cannot write " + out);
    fwrite(&n_qv, 4, 1, f);
    for (uint32_t u = 0; u < n_qv; u++) {
        std::vector<uint32_t> ids;
        for (uint64_t w = 0; w < words; w++)
            for (uint32_t bits = bitmap[(size_t)u * words + w]; bits; bits &= bits - 1)
                ids.push_back((uint32_t)(w * 32 + __builtin_ctz(bits)));
        const uint32_t c = (uint32_t)ids.size();
        fwrite(&c, 4, 1, f);
        if (c) fwrite(ids.data(), 4, c, f);
    }
    if (fclose(f) != 0) die("write failed on " + out);
    gnnpe_host_free(qv);
    gnnpe_host_free(ql);
    gnnpe_host_free(qd);
    gnnpe_host_free(qp);
    if (o.timing)
        fprintf(stderr, "{%s\"paths\": %llu, \"query_paths\": %u, \"filter_device_ms\": %.3f, \"end_to_end_s\": %.3f}\n",
                exact_json.c_str(), (unsigned long long)P, n_qp, ms, secs(t0, Clock::now()));
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    const double before_main_s = secs_since_process_start();
    Options o = parse_args(argc, argv);
    const auto t_start = Clock::now();

    // main.cpp:58-59: path_length += 1; pde_dim = vde_dim * path_length
    if (o.path_length != 2 && o.path_length != 3)
        die("-l " + std::to_string(o.path_length) + ": only -l 2 and -l 3 are supported (the reference always enumerates "
            "3-vertex paths and mis-prints them for any other -l)");
    if (o.path_length == 3 && o.mode != "online" && o.mode != "filter")
        fprintf(stderr, "note: -l 3 writes 4-vertex paths; the reference's online binary only reads -l 2 files (SURVEY D4)\n");
    const uint32_t L = o.path_length + 1;
    if (o.answers != "MAX") {  // main.cpp:62-69 (MAX_LIMIT is an online-only knob)
        uint32_t lim;
        if (!parse_u32(o.answers, &lim)) die("-n must be MAX or an integer");
    }
    if (o.partition_num == 0) die("-p must be >= 1");
    // --refine sets counts inside EVERY candidate set, so it needs complete sets (INTEGRATION.md "Exact mode")
    if (!o.matches_file.empty() && o.refine != "sets") die("--matches needs --refine sets");
    if (o.all_matches && o.matches_file.empty()) die("--all-matches needs --matches FILE");
    if (o.match_page_given && !o.all_matches) die("--match-page needs --all-matches");
    if (o.distinct && o.refine != "sets") die("--distinct needs --refine sets");
    if (o.induced && o.refine != "sets") die("--induced needs --refine sets");
    if (!o.vertex_counts_file.empty() && o.refine != "sets") die("--vertex-counts needs --refine sets");
    if (!o.vertex_counts_file.empty() && !o.matches_file.empty()) die("--vertex-counts and --matches exclude each other");
    if (!o.edge_counts_file.empty() && o.refine != "sets") die("--edge-counts needs --refine sets");
    if (!o.edge_counts_file.empty() && !o.matches_file.empty()) die("--edge-counts and --matches exclude each other");
    if (!o.edge_counts_file.empty() && !o.vertex_counts_file.empty()) die("--edge-counts and --vertex-counts exclude each other");
    if (!o.delta_edges_file.empty() && o.refine != "sets") die("--delta-edges needs --refine sets");
    if (!o.delta_edges_file.empty() && (o.all_matches || !o.vertex_counts_file.empty() || !o.edge_counts_file.empty()))
        die("--delta-edges excludes --all-matches, --vertex-counts and --edge-counts");
    if (!o.delta_nonedges_file.empty()) {
        if (o.refine != "sets") die("--delta-nonedges needs --refine sets");
        if (!o.induced) die("--delta-nonedges needs --induced");
        if (!o.delta_edges_file.empty()) die("--delta-nonedges and --delta-edges exclude each other");
        if (o.all_matches || !o.vertex_counts_file.empty() || !o.edge_counts_file.empty())
            die("--delta-nonedges excludes --all-matches, --vertex-counts and --edge-counts");
    }
    if (!o.delta_vertices_file.empty()) {
        if (o.refine != "sets") die("--delta-vertices needs --refine sets");
        if (!o.delta_edges_file.empty() || !o.delta_nonedges_file.empty())
            die("--delta-vertices excludes --delta-edges and --delta-nonedges");
        if (o.all_matches || !o.vertex_counts_file.empty() || !o.edge_counts_file.empty())
            die("--delta-vertices excludes --all-matches, --vertex-counts and --edge-counts");
        (void)read_vertex_list(o.delta_vertices_file);  // a malformed file is refused before a GPU is touched
    }
    if (o.delta_pages_given) {
        if (o.delta_edges_file.empty() && o.delta_nonedges_file.empty() && o.delta_vertices_file.empty())
            die("--delta-pages needs --delta-edges FILE or --delta-nonedges FILE or --delta-vertices FILE");
        if (o.matches_file.empty()) die("--delta-pages needs --matches FILE");
        if (!o.delta_vertex_counts_file.empty() || !o.delta_edge_counts_file.empty())
            die("--delta-pages excludes --delta-vertex-counts and --delta-edge-counts");
    }
    for (const char *flag : {"--delta-vertex-counts", "--delta-edge-counts"}) {
        const bool edge_table = std::string(flag) == "--delta-edge-counts";
        if ((edge_table ? o.delta_edge_counts_file : o.delta_vertex_counts_file).empty()) continue;
        if (o.refine != "sets") die(std::string(flag) + " needs --refine sets");
        if (o.delta_edges_file.empty() && o.delta_nonedges_file.empty() && o.delta_vertices_file.empty())
            die(std::string(flag) + " needs --delta-edges FILE or --delta-nonedges FILE or --delta-vertices FILE");
        if (edge_table && !o.delta_vertex_counts_file.empty()) die("--delta-vertex-counts and --delta-edge-counts exclude each other");
        if (!o.matches_file.empty()) die(std::string(flag) + " and --matches exclude each other");
    }
    if (o.refine == "sets" && o.mode != "online") die("--refine sets applies to -m online only");
    // exact -m online / -m filter read nothing that was derived from the old graph (only the data graph and membership.txt)
    if (!o.apply_edges_file.empty() && !((o.mode == "online" || o.mode == "filter") && (o.exact || o.path_length == 3)))
        die("--apply-edges applies to exact -m online / -m filter only (--exact or -l 3): every other mode reads files that were "
            "made from the graph as it was");
    if (!o.set_labels_file.empty() && !((o.mode == "online" || o.mode == "filter") && (o.exact || o.path_length == 3)))
        die("--set-labels applies to exact -m online / -m filter only (--exact or -l 3): every other mode reads files that were "
            "made from the graph as it was");
    if (!o.apply_vertices_file.empty() && !((o.mode == "online" || o.mode == "filter") && (o.exact || o.path_length == 3)))
        die("--apply-vertices applies to exact -m online / -m filter only (--exact or -l 3): every other mode reads files that were "
            "made from the graph as it was");
    if (o.standing) {
        if (!(o.mode == "online" && (o.exact || o.path_length == 3)) || o.standing_batches.empty())
            die("--standing applies to exact -m online (--exact or -l 3) with one or more --apply-edges, --set-labels, --apply-vertices FILE, "
                "--peel T or --truss-levels FILE");
        if (o.incremental) die("--standing keeps its own support table: --incremental does not go with it");
    } else if (!o.standing_vertex_counts_file.empty() || !o.standing_edge_counts_file.empty())
        die("--standing-vertex-counts and --standing-edge-counts need --standing");
    else if (o.standing_peels)
        die("--peel and --truss-levels need --standing");
    if (o.incremental && o.apply_vertices_file.empty() && o.apply_edges_file.empty() && o.set_labels_file.empty())
        die("--incremental applies with --apply-vertices, --apply-edges or --set-labels: it carries the exact filter's support table "
            "across their batches");
    if (!o.apply_vertices_file.empty() && !o.standing) {  // a malformed file is refused before a GPU is touched (--standing reads every batch there)
        std::vector<uint32_t> rem, add;
        read_vertex_batch(o.apply_vertices_file, &rem, &add);
    }
    if (!o.set_labels_file.empty() && !o.standing) {  // a malformed file is refused before a GPU is touched
        std::vector<uint32_t> vs, ls;
        read_label_list(o.set_labels_file, &vs, &ls);
    }
    if (o.refine == "sets" && !(o.exact || o.path_length == 3))
        die("--refine sets needs complete candidate sets: add --exact or use -l 3 (the reference-mode filter's sets miss "
            "embeddings, and only the start vertex's set may restrict the search there)");
    if (o.mode == "online" || o.mode == "filter") return run_filter(o);
    if (o.exact) die("--exact applies to -m online and -m filter only");
    if (o.mode != "offline") return 0;  // the reference does nothing for other modes
    if (o.write_index && gnnpe_index_file_bytes(1, L * o.vde_dim, 0) == 0)  // before the graph is read or a GPU is touched
        die("--index: an entry of " + std::to_string(L * o.vde_dim) + " dimensions (" + std::to_string(16ull * L * o.vde_dim + 4) +
            " bytes) gives a node capacity below 3 in a 4096-byte block (rtnode.cpp:27-28); use a smaller -e");

    // HIP start-up (0.1-0.2 s: runtime initialisation, context, code objects) runs beside the graph load.  An error
    // exit in between (die() -> exit()) must not tear the process down under that thread: it is joined first.
    static int early_ndev = -1;
    static gnnpe_ctx *early_ctx = nullptr;
    static std::thread *warm = nullptr;
    const bool slab_path = o.gpus > 1 || o.transport_explicit;
    if (!slab_path) {
        warm = new std::thread([] {
            early_ndev = gnnpe_device_count();
            if (early_ndev > 0) early_ctx = gnnpe_create(0);
        });
        atexit([] {
            if (warm && warm->joinable()) warm->join();
        });
    }

    StaticGraph g;
    std::string err;
    int rc = g.load(o.data_graph, &err, o.strict);
    if (rc == -1) {  // graph.cpp:166-169
        printf("%s\n", err.c_str());
        exit(-1);
    }
    if (rc != 0) die(o.data_graph + ": " + err);
    fputs(g.metadata_text().c_str(), stdout);  // printGraphMetaData, main.cpp:73
    const auto t_loaded = Clock::now();

    std::vector<uint32_t> sorted_nodes, membership;
    if (gnnpe_host::read_membership(o.dataset_path + "gnn-pe/membership.txt", g.n, o.partition_num, &sorted_nodes,
                                    &membership, &err) != 0)
        die(err);
    const std::string partitions_path = o.dataset_path + "gnn-pe/partitions/";
    for (uint32_t i = 0; i < o.partition_num; i++)
        if (!is_dir(partitions_path + "partition-" + std::to_string(i)))
            die("missing directory " + partitions_path + "partition-" + std::to_string(i) + "/ (the prep step creates it)");

    // ---- device setup ----
    if (warm) {
        warm->join();
        delete warm;
        warm = nullptr;
    }
    const int ndev = early_ndev >= 0 ? early_ndev : gnnpe_device_count();
    if (ndev <= 0) die("no HIP device: this tool has no CPU fallback");
    if (o.gpus < 1 || (o.gpus > ndev && !o.same_device)) die("--gpus " + std::to_string(o.gpus) + " but " + std::to_string(ndev) + " device(s) present");
    std::vector<double> table((size_t)std::max<uint32_t>(g.labels_count, 1) * o.vde_dim);
    check(gnnpe_host_label_table(std::max<uint32_t>(g.labels_count, 1), o.vde_dim, table.data()), "label table");
    if (slab_path) {
        // the north-star split: one thread + one GPU per slab of the order, each with its own rows only, halo by
        // all-to-all-v, concurrent emit and pwrite (host/slab_offline.cpp); `--gpus 1 --transport rccl` runs the same
        // code as a 1-rank communicator
        if (o.sidecars) die("--sidecars is a single-GPU option");
        return slab::run_offline_slabs(o, g, sorted_nodes, membership, table, t_start, t_loaded);
    }
    // --index: the partitions' index.dat files are the work of a SECOND context on the same device, on a thread of its own, beside
    // the text files: the two share nothing but the host arrays, the 22 GB of index blocks cross PCIe while the text is rendered
    // and written, and the files of both kinds go to the file system side by side (one file takes ~10 GB/s on these boxes whatever
    // the number of writers, scripts/fs_write_probe.cpp; sixteen files take 30-40).  The thread builds its context and its count,
    // then waits for the main thread's size check before it writes anything.
    struct IndexJob {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        int go = 0;  // 0: wait, 1: write the files, -1: give up
        double seconds = 0.0;
        std::string error;
    };
    static IndexJob *index_job = nullptr;
    std::vector<std::string> ips, aps;
    for (uint32_t pid = 0; pid < o.partition_num; pid++) {
        ips.push_back(partitions_path + "partition-" + std::to_string(pid) + "/index.dat");
        aps.push_back(partitions_path + "partition-" + std::to_string(pid) + "/aux_index.bin");
    }
    if (o.write_index) {
        index_job = new IndexJob();
        index_job->th = std::thread([&, job = index_job] {
            const auto i0 = Clock::now();
            auto fail = [&](const char *what) { job->error = std::string(what) + ": " + gnnpe_last_error(); };
            // test hook (tests/test_gpu_cli.py): GNNPE_FAULT_RANK=index:create fails this thread as an out-of-memory would
            const char *fault = getenv("GNNPE_FAULT_RANK");
            if (fault && !strcmp(fault, "index:create")) {
                job->error = "gnnpe_create (index): injected fault";
                return;
            }
            gnnpe_ctx *ctx = gnnpe_create(0);
            if (!ctx) return fail("gnnpe_create (index)");
            uint64_t P2 = 0;
            if (load_graph_into(ctx, g) != 0 ||
                gnnpe_set_order(ctx, sorted_nodes.data(), membership.data(), o.partition_num) != 0 ||
                gnnpe_set_label_table(ctx, std::max<uint32_t>(g.labels_count, 1), o.vde_dim, table.data()) != 0 ||
                gnnpe_vde(ctx, nullptr, nullptr, nullptr) != 0 || gnnpe_count_paths(ctx, o.path_length, nullptr, &P2) != 0) {
                fail("index context");
                gnnpe_destroy(ctx);
                return;
            }
            {
                std::unique_lock<std::mutex> lk(job->mu);
                job->cv.wait(lk, [&] { return job->go != 0; });
                if (job->go < 0) {
                    gnnpe_destroy(ctx);
                    return;
                }
            }
            std::vector<const char *> ipp, app;
            for (uint32_t pid = 0; pid < o.partition_num; pid++) {
                ipp.push_back(ips[pid].c_str());
                app.push_back(aps[pid].c_str());
            }
            // every partition's image first, then the files side by side; with --sidecars also the trees' auxiliary index
            // (custom.h:268-364), which the online side otherwise rebuilds on every start
            if (gnnpe_build_index_files(ctx, o.partition_num, ipp.data(), o.sidecars ? app.data() : nullptr) != 0) fail("build_index_files");
            gnnpe_destroy(ctx);
            job->seconds = secs(i0, Clock::now());
        });
        atexit([] {  // an error exit on the main thread: the index thread is told to give up and joined first
            if (index_job && index_job->th.joinable()) {
                {
                    std::unique_lock<std::mutex> lk(index_job->mu);
                    if (index_job->go == 0) index_job->go = -1;
                }
                index_job->cv.notify_all();
                index_job->th.join();
            }
        });
    }
    std::vector<Device> devs(1);
    devs[0].ctx = early_ctx ? early_ctx : gnnpe_create(0);  // (again on this thread if the early one failed: for its message)
    if (!devs[0].ctx) die(std::string("gnnpe_create: ") + gnnpe_last_error());
    check(load_graph_into(devs[0].ctx, g), "load_csr");
    check(gnnpe_set_order(devs[0].ctx, sorted_nodes.data(), membership.data(), o.partition_num), "set_order");
    check(gnnpe_set_label_table(devs[0].ctx, std::max<uint32_t>(g.labels_count, 1), o.vde_dim, table.data()), "set_label_table");
    const auto t_setup = Clock::now();

    // ---- R4 + R2 count on device 0 over the whole order: per-start counts size everything ----
    std::vector<double> hx, hnx, hvde;
    if (o.sidecars) {
        hx.resize((size_t)g.n * o.vde_dim);
        hnx.resize(hx.size());
        hvde.resize(hx.size());
    }
    for (int d = 0; d < o.gpus; d++)
        check(gnnpe_vde(devs[d].ctx, d == 0 && o.sidecars ? hx.data() : nullptr, d == 0 && o.sidecars ? hnx.data() : nullptr,
                        d == 0 && o.sidecars ? hvde.data() : nullptr), "vde");
    std::vector<uint64_t> per_start(g.n);
    uint64_t P = 0;
    check(gnnpe_count_paths(devs[0].ctx, o.path_length, per_start.data(), &P), "count_paths");
    if (P > 0xFFFFFFFFull && !o.allow_large)
        die(std::to_string(P) + " paths exceed the reference's 32-bit path ids (use --allow-large to write anyway)");
    // slabs with equal path counts
    {
        uint64_t acc = 0;
        uint32_t i = 0;
        for (int d = 0; d < o.gpus; d++) {
            devs[d].slab_begin = i;
            devs[d].base = acc;
            const uint64_t target = P * (uint64_t)(d + 1) / (uint64_t)o.gpus;
            while (i < g.n && (acc < target || d == o.gpus - 1)) acc += per_start[i++];
            devs[d].slab_end = i;
            devs[d].total = acc - devs[d].base;
        }
    }
    std::vector<uint64_t> part_count(o.partition_num, 0);  // main.cpp:102: header of partition_paths.txt
    for (uint32_t i = 0; i < g.n; i++) part_count[membership[sorted_nodes[i]]] += per_start[i];
    if (o.write_index) {  // before anything is written
        const std::string big = index_size_problem(part_count, P, (o.path_length + 1) * o.vde_dim,
                                                   // the pair-major (l = 2) and triple-major (l = 3) builds exist at the widths with a specialised
                                                   // enumeration; else the tuple-array build
                                                   (o.vde_dim <= 4 || o.vde_dim == 8) ? 0 : 1);
        if (!big.empty() && !o.allow_large) die(big + " (use --allow-large to write the files anyway)");
        if (!big.empty()) fprintf(stderr, "%s: warning: %s\n", o.tool, big.c_str());
        {
            std::unique_lock<std::mutex> lk(index_job->mu);
            index_job->go = 1;  // the size check has passed: the index thread may write
        }
        index_job->cv.notify_all();
    }
    for (int d = 0; d < o.gpus; d++) {
        if (o.gpus > 1) {
            check(gnnpe_set_slab(devs[d].ctx, devs[d].slab_begin, devs[d].slab_end), "set_slab");
            uint64_t t = 0;
            check(gnnpe_count_paths(devs[d].ctx, o.path_length, nullptr, &t), "count_paths(slab)");
            if (t != devs[d].total) die("slab count mismatch");
        }
    }
    const auto t_counted = Clock::now();

    // ---- emit + render + write, chunk by chunk, slab by slab (rank order = file order) ----
    FileSink all_paths(o.dataset_path + "/gnn-pe/all_paths.txt");  // main.cpp:110 (sic: extra slash)
    all_paths.write_now(std::to_string(P) + "\n");
    std::vector<FileSink *> part_files;
    for (uint32_t i = 0; i < o.partition_num; i++) {
        part_files.push_back(new FileSink(partitions_path + "partition-" + std::to_string(i) + "/partition_paths.txt"));
        part_files[i]->write_now(std::to_string(part_count[i]) + "\n");
    }
    // --sidecars: the rows again as uint32 tuples (paths.bin), so that an online start can skip the text re-parse of
    // gen_pde (custom.h:546-572); read back by gnnpe_host_load_path_sidecar
    FILE *paths_bin = nullptr;
    std::vector<uint32_t> ids_host;
    if (o.sidecars) {
        paths_bin = fopen((o.dataset_path + "gnn-pe/paths.bin").c_str(), "wb");
        if (!paths_bin) die("cannot write paths.bin");
        setvbuf(paths_bin, nullptr, _IOFBF, 8 << 20);
        check(gnnpe_host_write_paths_header(paths_bin, L, P), "paths.bin");
    }
    double t_gpu = 0.0;
    for (int d = 0; d < o.gpus; d++) {
        gnnpe_ctx *ctx = devs[d].ctx;
        const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(o.chunk_paths, devs[d].total));
        void *d_ids = nullptr, *d_part = nullptr, *d_sel = nullptr, *d_text = nullptr;
        const uint64_t text_cap = chunk * (11ull * L + 1) + 64;
        // the emitted rows live in the library's output pool: one allocation (no candidate draw since round 4); when one
        // chunk holds every path the pool times both emit shapes into it and later fills take the faster one
        gnnpe_pool *pool = nullptr;
        check(gnnpe_output_pool_create(ctx, chunk, L, 0, 1u | GNNPE_POOL_NO_CALIBRATION, &pool), "output pool");
        check(gnnpe_output_pool_acquire(pool, &d_ids, nullptr, nullptr), "output pool");
        check(gnnpe_dev_alloc(ctx, chunk * 4, &d_part), "alloc part");
        check(gnnpe_dev_alloc(ctx, chunk * 8, &d_sel), "alloc sel");
        check(gnnpe_dev_alloc(ctx, text_cap, &d_text), "alloc text");
        for (uint64_t b = 0; b < devs[d].total; b += chunk) {
            const uint64_t e = std::min(devs[d].total, b + chunk), cnt = e - b;
            const auto g0 = Clock::now();
            check(gnnpe_fill_paths_device(ctx, b, e, d_ids, nullptr, nullptr), "fill_paths");
            check(gnnpe_path_partitions_device(ctx, b, e, d_part), "path_partitions");
            uint64_t nb = 0;
            check(gnnpe_text_paths(ctx, cnt, L, d_ids, d_text, text_cap, &nb), "text_paths");
            HostBuf *buf = all_paths.acquire();
            buf->resize(nb);
            check(gnnpe_copy_to_host(ctx, buf->data(), d_text, nb), "copy text");
            t_gpu += secs(g0, Clock::now());
            all_paths.submit(buf, nb);
            if (paths_bin) {
                ids_host.resize(cnt * L);
                check(gnnpe_copy_to_host(ctx, ids_host.data(), d_ids, cnt * L * 4), "copy ids");
                if (fwrite(ids_host.data(), 4, cnt * L, paths_bin) != cnt * L) die("write error on paths.bin");
            }
            for (uint32_t pid = 0; pid < o.partition_num; pid++) {
                const auto g1 = Clock::now();
                uint64_t k = 0, pb = 0;
                check(gnnpe_select_partition(ctx, cnt, d_part, pid, devs[d].base + b, d_sel, &k), "select_partition");
                check(gnnpe_text_ids(ctx, k, d_sel, d_text, text_cap, &pb), "text_ids");
                HostBuf *pbuf = part_files[pid]->acquire();
                pbuf->resize(pb);
                check(gnnpe_copy_to_host(ctx, pbuf->data(), d_text, pb), "copy ids text");
                t_gpu += secs(g1, Clock::now());
                part_files[pid]->submit(pbuf, pb);
            }
        }
        gnnpe_output_pool_destroy(pool);
        gnnpe_dev_free(ctx, d_part);
        gnnpe_dev_free(ctx, d_sel);
        gnnpe_dev_free(ctx, d_text);
    }
    uint64_t bytes_all = all_paths.close(), bytes_part = 0;
    for (auto *f : part_files) {
        bytes_part += f->close();
        delete f;
    }
    const auto t_written = Clock::now();

    if (paths_bin && fclose(paths_bin) != 0) die("write error on paths.bin");
    if (o.sidecars) {  // ignored by the reference; carrier for the embedding parity check and the online data load
        FILE *f = fopen((o.dataset_path + "gnn-pe/vde.bin").c_str(), "wb");
        if (!f) die("cannot write vde.bin");
        uint32_t hdr[2] = {g.n, o.vde_dim};
        fwrite(hdr, 4, 2, f);
        fwrite(hx.data(), 8, hx.size(), f);
        fwrite(hnx.data(), 8, hnx.size(), f);
        fwrite(hvde.data(), 8, hvde.size(), f);
        fclose(f);
    }
    double t_index = 0.0, t_index_wait = 0.0;
    if (o.write_index) {  // optional accelerator: the reference online run reuses an existing index.dat (custom.h:222-235)
        const auto i0 = Clock::now();
        index_job->th.join();
        t_index_wait = secs(i0, Clock::now());
        t_index = index_job->seconds;
        if (!index_job->error.empty()) {
            // the second context is an overlap, not a requirement: two copies of the graph and its count state plus
            // the main thread's chunk buffers may not fit where one did.  The text is written and its buffers are freed: build
            // the files on the main context, one after the other, as round 4 did.
            fprintf(stderr, "%s: note: index context failed (%s); building index.dat on the main context instead\n", o.tool,
                    index_job->error.c_str());
            std::vector<const char *> ipp, app;
            for (uint32_t pid = 0; pid < o.partition_num; pid++) {
                ipp.push_back(ips[pid].c_str());
                app.push_back(aps[pid].c_str());
            }
            check(gnnpe_build_index_files(devs[0].ctx, o.partition_num, ipp.data(), o.sidecars ? app.data() : nullptr),
                  "build_index_files (main context)");
            t_index = secs(i0, Clock::now());
        }
        for (auto &ip : ips) warn_if_index_too_large_for_reference(ip);
    }
    for (auto &d : devs) gnnpe_destroy(d.ctx);

    if (o.timing) {
        fprintf(stderr,
                "{\"paths\": %llu, \"gpus\": %d, \"load_s\": %.3f, \"setup_s\": %.3f, \"vde_count_s\": %.3f, "
                "\"emit_render_copy_s\": %.3f, \"write_total_s\": %.3f, \"text_gb_per_s\": %.2f, \"end_to_end_s\": %.3f, "
                "\"all_paths_bytes\": %llu, \"partition_bytes\": %llu, \"index_build_s\": %.3f, \"index_wait_after_text_s\": %.3f, "
                "\"before_main_s\": %.2f}\n",
                (unsigned long long)P, o.gpus, secs(t_start, t_loaded), secs(t_loaded, t_setup), secs(t_setup, t_counted),
                t_gpu, secs(t_counted, t_written), (bytes_all + bytes_part) / 1e9 / std::max(1e-9, secs(t_counted, t_written)),
                secs(t_start, Clock::now()), (unsigned long long)bytes_all,
                (unsigned long long)bytes_part, t_index, t_index_wait, before_main_s);
    }
    // (What a caller's wall-clock holds beyond end_to_end_s: 0.02 s before main() -- `before_main_s` -- and 0.10-0.15 s after it at
    // config 3, the kernel unmapping the process; leaving through _exit() instead of the runtime's unwinding measured the same.)
    return 0;
}
