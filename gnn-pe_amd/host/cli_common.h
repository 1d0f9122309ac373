// cli_common.h -- flag parsing and small helpers shared by gnnpe_main (GNN-PE/src/main.cpp mirror) and
// gnnpge_main (GNN-PGE/src/main.cpp mirror).  Both reference programs take the same eight CLI11 flags.
#pragma once

#include <dlfcn.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gnnpe_hip.h"
#include "graph_loader.h"

using Clock = std::chrono::steady_clock;

namespace cli {

struct Options {
    const char *tool = "gnnpe_main";
    // the reference's flags and defaults (main.cpp:40-56, custom.h:45-50)
    std::string dataset_path = "../Test/";
    std::string data_graph = "../Test/data_graph.graph";
    std::string query_graph = "../Test/query_graph.graph";
    std::string mode = "offline";
    std::string answers = "MAX";
    uint32_t partition_num = 5, path_length = 2, vde_dim = 2;
    // extensions
    int gpus = 1;
    uint64_t chunk_paths = 8ull << 20;  // 8M paths per pass: small enough to pipeline render, copy-back and file writes
    bool allow_large = false, timing = false, sidecars = false, write_index = false;
    bool exact = false;   // -m online / filter at -l 2: the orientation-complete filter (always on at -l 3; refused in other
                          // modes; INTEGRATION.md "Exact mode")
    // -m online with complete sets (--exact, -l 3): "start" = the frozen refinement (gnnpe_refine), "sets" = the set-restricted
    // one (gnnpe_refine_sets); --matches FILE (needs sets) writes the embeddings, one per line
    std::string refine = "start", matches_file;
    // --all-matches (needs --matches): every embedding up to -n, page by page through the match cursor (gnnpe_refine_pages_*);
    // --match-page ROWS (needs --all-matches): rows per page
    bool all_matches = false, match_page_given = false;
    uint64_t match_page = 1ull << 20;
    bool distinct = false;  // --distinct (needs --refine sets): every matching subgraph once (gnnpe_refine_sets_distinct)
    // --vertex-counts FILE (needs --refine sets, not with --matches): per data vertex, in how many matches it is the image of each
    // query vertex (gnnpe_refine_sets_vertex_counts); -n is a guard there -- a search that reaches it writes no file
    std::string vertex_counts_file;
    // --edge-counts FILE (needs --refine sets, not with --matches or --vertex-counts): per adjacency entry, in how many matches it
    // carries each query edge (gnnpe_refine_sets_edge_counts); -n is a guard as for --vertex-counts
    std::string edge_counts_file;
    // --delta-edges FILE (needs --refine sets; with --matches but not --all-matches, not with the count tables): one data edge
    // `x y` per line; the answer is the matches through at least one of them, each once (gnnpe_refine_sets_delta)
    std::string delta_edges_file;
    // --delta-nonedges FILE (needs --refine sets and --induced; with --matches but not --all-matches, not with --delta-edges,
    // --vertex-counts or --edge-counts): one data vertex pair `x y` per line, none of them an edge; the answer is the induced matches
    // that put a non-adjacent query pair on at least one of them, each once (gnnpe_refine_sets_delta_nonedges)
    std::string delta_nonedges_file;
    // --delta-vertex-counts FILE, --delta-edge-counts FILE (need --refine sets and --delta-edges, --delta-nonedges or --delta-vertices; not with each
    // other, --matches or the count tables): the table of --vertex-counts / --edge-counts over the matches through the delta edges
    // only (gnnpe_refine_sets_delta_vertex_counts / _edge_counts), or with --delta-nonedges over the induced matches on those pairs
    // only (gnnpe_refine_sets_delta_nonedges_vertex_counts / _edge_counts), or with --delta-vertices over the matches with an image
    // among those vertices only (gnnpe_refine_sets_delta_vertices_vertex_counts / _edge_counts); -n is a guard as for --vertex-counts
    std::string delta_vertex_counts_file, delta_edge_counts_file;
    // --apply-edges FILE (exact -m online / -m filter only): lines `+ x y` / `- x y`, a batch of edge insertions and deletions
    // applied to the loaded data graph on the device before anything is computed from it (gnnpe_csr_apply_edges)
    std::string apply_edges_file;
    std::vector<std::string> apply_edges_files;  // every --apply-edges in the order given
    // the batches of --standing in command-line order: {'e' --apply-edges, 'l' --set-labels, 'v' --apply-vertices, FILE}
    // ... and {'p' --peel, T} / {'t' --truss-levels, FILE}: a peel of the graph by edge support (gnnpe_standing_peel) and the truss
    // level of every edge (gnnpe_standing_truss_levels, with restore), in the same order
    std::vector<std::pair<char, std::string>> standing_batches;
    std::vector<std::pair<size_t, std::string>> standing_peel_outs;  // --peel-out FILE: {index of the --peel before it, FILE}
    bool standing_peels = false;                                     // a --peel or --truss-levels was given
    bool standing = false;  // --standing: a standing exact query carried through the batches (gnnpe_standing_* of include/gnnpe_online.h)
    // --standing-vertex-counts FILE, --standing-edge-counts FILE (need --standing): the handle keeps the table (gnnpe_standing_keep_counts),
    // every batch prints `changes: <n>`, and the table after the last batch is written in the format of --vertex-counts / --edge-counts
    std::string standing_vertex_counts_file, standing_edge_counts_file;
    // --delta-vertices FILE (needs --refine sets; with --distinct, --induced and --matches, not with --delta-edges, --delta-nonedges,
    // --all-matches, --vertex-counts or --edge-counts): one data vertex id per line; the answer is the matches with at least one image
    // among them, each once (gnnpe_refine_sets_delta_vertices); --delta-vertex-counts / --delta-edge-counts write their tables
    std::string delta_vertices_file;
    // --delta-pages ROWS (needs --matches and one of --delta-edges, --delta-nonedges, --delta-vertices; not with --delta-vertex-counts
    // or --delta-edge-counts): every match of the delta up to -n into --matches, ROWS per page through a delta cursor
    // (gnnpe_refine_pages_open_delta, _open_delta_nonedges, _open_delta_vertices)
    bool delta_pages_given = false;
    uint64_t delta_pages = 0;
    // --set-labels FILE (exact -m online / -m filter only): lines `v label`, new labels for those data vertices, set on the device
    // after --apply-edges and before anything is computed from the graph (gnnpe_set_vertex_labels)
    std::string set_labels_file;
    // --apply-vertices FILE (exact -m online / -m filter only): lines `- v` / `+ label`, a batch of vertex removals and additions
    // applied to the loaded data graph on the device before --apply-edges and --set-labels (gnnpe_csr_apply_vertices)
    std::string apply_vertices_file;
    // --incremental (with --apply-vertices / --apply-edges / --set-labels): the exact candidate sets come from the filter's support table
    // carried across the batches (gnnpe_filter_support_exact, _delta, _bitmap) and not from a filter pass over the updated graph
    bool incremental = false;
    bool induced = false;   // --induced (needs --refine sets): induced matching, query non-edges on data non-edges (GNNPE_MATCH_INDUCED)
    bool strict = false;  // refuse a graph file with a duplicate `e` line (the reference loads it as it is: graph.cpp:211-218)
    bool same_device = false;  // testing aid: all --gpus contexts on device 0 (halo by device copies: RCCL needs distinct GPUs)
    std::string transport = "rccl";  // --gpus N > 1: "rccl" (ncclSend/ncclRecv over xGMI) or "copy" (device-to-device copies)
    // --transport given explicitly: take the slab path (host/slab_offline.cpp) even with --gpus 1 -- a 1-rank communicator
    // whose exchanges go through librccl (self ncclSend/ncclRecv), i.e. the N > 1 code on a single-GPU box
    bool transport_explicit = false;
};

static const char *g_tool = "gnnpe_main";

inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// seconds since the kernel started this process (exec, dynamic loading, the libraries' static constructors -- what a caller's
// wall-clock holds in front of main()); 10 ms resolution (/proc/self/stat field 22 against CLOCK_BOOTTIME); < 0 when unknown
inline double secs_since_process_start()
{
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[2048];
    const size_t nr = fread(buf, 1, sizeof(buf) - 1, f);
    fclose(f);
    buf[nr] = 0;
    const char *p = strrchr(buf, ')');  // (the command name may hold blanks)
    if (!p) return -1.0;
    unsigned long long start = 0;
    int field = 2;
    for (p++; *p && field < 22;) {
        while (*p == ' ') p++;
        field++;
        if (field == 22) {
            start = strtoull(p, nullptr, 10);
            break;
        }
        while (*p && *p != ' ') p++;
    }
    struct timespec ts;
    if (!start || clock_gettime(CLOCK_BOOTTIME, &ts) != 0) return -1.0;
    return (double)ts.tv_sec + ts.tv_nsec * 1e-9 - (double)start / (double)sysconf(_SC_CLK_TCK);
}

[[noreturn]] inline void die(const std::string &msg, int code = 1)
{
    fprintf(stderr, "%s: %s\n", g_tool, msg.c_str());
    exit(code);
}

inline void check(int rc, const char *what)
{
    if (rc != 0) die(std::string(what) + ": " + gnnpe_last_error());
}

inline bool parse_u32(const std::string &s, uint32_t *v)
{
    if (s.empty()) return false;
    char *end = nullptr;
    unsigned long long x = strtoull(s.c_str(), &end, 10);
    if (*end || x > 0xFFFFFFFFull) return false;
    *v = (uint32_t)x;
    return true;
}

// CLI11-style parsing of `-x v`, `-xv`, `--long v`, `--long=v`
inline Options parse_args(int argc, char **argv, const char *tool = "gnnpe_main")
{
    Options o;
    o.tool = tool;
    g_tool = tool;
    struct Opt { char s; const char *l; } opts[] = {{'f', "file"}, {'d', "data"}, {'q', "query"}, {'m', "mode"},
                                                     {'p', "partition"}, {'l', "length"}, {'e', "embedding"}, {'n', "answers"}};
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], val;
        char key = 0;
        if (a == "-h" || a == "--help") {
            printf("%s -f <dataset dir/> -d <data.graph> -m offline -p <partitions> [-l 2] [-e 2]\n"
                   "           [--gpus N] [--transport rccl|copy] [--chunk PATHS] [--index] [--sidecars] [--timing] [--allow-large]\n"
                   "       %s -f <dataset dir/> -d <data.graph> -q <query.graph> -m online|filter [-l 2|3] [--exact] [--timing]\n"
                   "           [--refine start|sets [--distinct] [--induced]] [--matches FILE [--all-matches [--match-page ROWS]]]\n"
                   "           [--vertex-counts FILE | --edge-counts FILE | (--delta-edges FILE | --delta-nonedges FILE | --delta-vertices FILE)\n"
                   "           [--delta-vertex-counts FILE | --delta-edge-counts FILE | --delta-pages ROWS]] [--apply-edges FILE]\n"
                   "           [--set-labels FILE] [--apply-vertices FILE] [--incremental]\n"
                   "       --matches FILE writes at most 2^20 embeddings (needs --refine sets); with --all-matches every embedding up to -n,\n"
                   "       in pages of ROWS embeddings (default 1048576); --distinct counts and writes every matching subgraph once;\n"
                   "       --induced counts and writes induced matches only: non-adjacent query vertices on non-adjacent data vertices;\n"
                   "       --vertex-counts FILE (needs --refine sets, not with --matches; combines with --distinct and --induced) writes one\n"
                   "       line `v c_0 ... c_{nq-1}` per data vertex in a match, ascending: c_u = the matches that send query vertex u to v.\n"
                   "       -n is a guard there: if the matches reach it, no file is written and the exit status is non-zero;\n"
                   "       --edge-counts FILE (needs --refine sets, not with --matches or --vertex-counts; combines with --distinct and\n"
                   "       --induced) writes a first line `# a_0-b_0 a_1-b_1 ...`, the query edges with a_k < b_k, and one line\n"
                   "       `x y c_0 ... c_{nqe-1}` per directed adjacency entry x -> y in a match, ascending by (x, y): c_k = the matches that\n"
                   "       send a_k to x and b_k to y.  -n is a guard as for --vertex-counts;\n"
                   "       --delta-edges FILE (needs --refine sets; combines with --distinct, --induced and --matches, not with\n"
                   "       --all-matches or the count tables): FILE has one data edge `x y` per line; the answer is the number of matches\n"
                   "       that put a query edge on at least one of them, each match once, and --matches writes those;\n"
                   "       --delta-vertex-counts FILE, --delta-edge-counts FILE (need --refine sets and --delta-edges or --delta-nonedges\n"
                   "       or --delta-vertices;\n"
                   "       combine with --distinct, --induced and --apply-edges, not with each other, --matches, --vertex-counts or\n"
                   "       --edge-counts) write the file of --vertex-counts / --edge-counts over the matches through the delta edges only,\n"
                   "       or with --delta-nonedges over the induced matches on the listed non-edges only, or with --delta-vertices over\n"
                   "       the matches with an image among the listed vertices only.  -n is a guard as for --vertex-counts;\n"
                   "       --delta-nonedges FILE (needs --refine sets and --induced; combines with --distinct, --matches,\n"
                   "       --delta-vertex-counts and --delta-edge-counts, not with --delta-edges, --all-matches, --vertex-counts or\n"
                   "       --edge-counts): FILE has one pair of data vertices `x y` per line, none of them an edge; the answer is the number\n"
                   "       of induced matches that put a non-adjacent query pair on at least one of them, each match once -- the matches\n"
                   "       that inserting these edges destroys -- and --matches writes those;\n"
                   "       --apply-edges FILE (exact mode only: --exact or -l 3): FILE has one line `+ x y` (insert the edge) or `- x y`\n"
                   "       (delete it) per edge; the batch is applied to the data graph on the device and the query runs on the result:\n"
                   "       the metadata block and the rows of --edge-counts / --vertex-counts and of their --delta forms\n"
                   "       are the updated graph's;\n"
                   "       --delta-vertices FILE (needs --refine sets; combines with --distinct, --induced, --matches, --delta-vertex-counts\n"
                   "       and --delta-edge-counts, not with --delta-edges, --delta-nonedges, --all-matches, --vertex-counts or\n"
                   "       --edge-counts): FILE has one data vertex id per line; the\n"
                   "       answer is the number of matches with at least one image among them, each match once, and --matches writes those;\n"
                   "       --set-labels FILE (exact mode only: --exact or -l 3): FILE has one line `v label` per vertex; the labels are set\n"
                   "       on the device after --apply-edges and the query runs on the result: the metadata block is the relabelled graph's;\n"
                   "       under --standing it may be repeated and is a batch of its own (gnnpe_standing_set_labels)\n"
                   "       --apply-vertices FILE (exact mode only: --exact or -l 3): FILE has one line `- v` (remove vertex v with its edges;\n"
                   "       the survivors keep their order under new ids) or `+ label` (append a vertex with that label and no edges) per\n"
                   "       change; applied on the device first, so that --apply-edges, --set-labels and --delta-vertices name the new ids;\n"
                   "       under --standing it may be repeated and is a batch of its own (gnnpe_standing_apply_vertices): there the\n"
                   "       --apply-edges, --set-labels and --apply-vertices batches are applied in command-line order, one `standing:`\n"
                   "       line each, and a batch names the ids the batches before it left\n"
                   "       --incremental (with --apply-edges, --set-labels or --apply-vertices): the candidate sets come from the exact\n"
                   "       filter's support table, built on the graph as loaded and patched around every batch, not from a filter pass over\n"
                   "       the updated graph; same sets, same answer\n"
                   "       --standing-vertex-counts FILE, --standing-edge-counts FILE (need --standing; either or both): the standing query\n"
                   "       keeps the table across the batches (--apply-edges, --set-labels, --apply-vertices), prints `changes: <n>` per batch (the cells the batch changed,\n"
                   "       over the kept tables) and writes the table after the last batch as --vertex-counts / --edge-counts do\n"
                   "       --peel T [--peel-out FILE], --truss-levels FILE (need --standing, not --induced; repeatable, applied in\n"
                   "       command-line order with the batch files): the standing query keeps its per-edge table and the graph is peeled\n"
                   "       by edge support on the device.  --peel T deletes, round by round, every edge whose support is below T and\n"
                   "       prints `peel: <rounds> <edges removed> <edges left> <converged> <count> <device ms>`; FILE gets one `x y round`\n"
                   "       line per removed edge.  --truss-levels writes `x y level` for every edge, restores the graph and prints\n"
                   "       `truss: <edges> <levels> <largest level> <rounds> <device ms>`\n",
                   tool, tool);
            exit(0);
        }
        if (a == "--gpus" || a == "--chunk") {
            if (i + 1 >= argc) die(a + " needs a value");
            uint64_t v = strtoull(argv[++i], nullptr, 10);
            if (a == "--gpus") o.gpus = (int)v; else o.chunk_paths = v;
            continue;
        }
        if (a == "--transport") {
            if (i + 1 >= argc) die(a + " needs a value");
            o.transport = argv[++i];
            if (o.transport != "rccl" && o.transport != "copy") die("--transport must be rccl or copy");
            o.transport_explicit = true;
            continue;
        }
        if (a == "--refine" || a == "--matches" || a == "--vertex-counts" || a == "--edge-counts" || a == "--delta-edges" ||
            a == "--delta-nonedges" ||
            a == "--apply-edges" || a == "--delta-vertex-counts" || a == "--delta-edge-counts" || a == "--delta-vertices" ||
            a == "--set-labels" || a == "--apply-vertices" || a == "--standing-vertex-counts" || a == "--standing-edge-counts" ||
            a == "--peel" || a == "--peel-out" || a == "--truss-levels") {
            if (i + 1 >= argc) die(a + " needs a value");
            if (a == "--peel") {
                char *end = nullptr;
                (void)strtoull(argv[++i], &end, 10);
                if (*end || end == argv[i] || argv[i][0] == '-') die("--peel must be an unsigned integer (the smallest support an edge keeps)");
                o.standing_batches.emplace_back('p', argv[i]);
                o.standing_peels = true;
                continue;
            }
            if (a == "--peel-out") {
                if (o.standing_batches.empty() || o.standing_batches.back().first != 'p') die("--peel-out FILE follows the --peel T it belongs to");
                o.standing_peel_outs.emplace_back(o.standing_batches.size() - 1, argv[++i]);
                continue;
            }
            if (a == "--truss-levels") { o.standing_batches.emplace_back('t', argv[++i]); o.standing_peels = true; continue; }
            if (a == "--standing-vertex-counts") { o.standing_vertex_counts_file = argv[++i]; continue; }
            if (a == "--standing-edge-counts") { o.standing_edge_counts_file = argv[++i]; continue; }
            if (a == "--matches") { o.matches_file = argv[++i]; continue; }
            if (a == "--vertex-counts") { o.vertex_counts_file = argv[++i]; continue; }
            if (a == "--edge-counts") { o.edge_counts_file = argv[++i]; continue; }
            if (a == "--delta-edges") { o.delta_edges_file = argv[++i]; continue; }
            if (a == "--delta-nonedges") { o.delta_nonedges_file = argv[++i]; continue; }
            if (a == "--delta-vertex-counts") { o.delta_vertex_counts_file = argv[++i]; continue; }
            if (a == "--delta-edge-counts") { o.delta_edge_counts_file = argv[++i]; continue; }
            if (a == "--apply-edges") { o.apply_edges_file = argv[++i]; o.apply_edges_files.push_back(o.apply_edges_file); o.standing_batches.emplace_back('e', o.apply_edges_file); continue; }
            if (a == "--delta-vertices") { o.delta_vertices_file = argv[++i]; continue; }
            if (a == "--set-labels") { o.set_labels_file = argv[++i]; o.standing_batches.emplace_back('l', o.set_labels_file); continue; }
            if (a == "--apply-vertices") { o.apply_vertices_file = argv[++i]; o.standing_batches.emplace_back('v', o.apply_vertices_file); continue; }
            o.refine = argv[++i];
            if (o.refine != "start" && o.refine != "sets") die("--refine must be start or sets");
            continue;
        }
        if (a == "--match-page") {
            if (i + 1 >= argc) die(a + " needs a value");
            char *end = nullptr;
            o.match_page = strtoull(argv[++i], &end, 10);
            if (*end || end == argv[i] || o.match_page == 0) die("--match-page must be an integer of at least 1");
            o.match_page_given = true;
            continue;
        }
        if (a == "--delta-pages") {
            if (i + 1 >= argc) die(a + " needs a value");
            char *end = nullptr;
            o.delta_pages = strtoull(argv[++i], &end, 10);
            if (*end || end == argv[i] || o.delta_pages == 0) die("--delta-pages must be an integer of at least 1");
            o.delta_pages_given = true;
            continue;
        }
        if (a == "--all-matches") { o.all_matches = true; continue; }
        if (a == "--distinct") { o.distinct = true; continue; }
        if (a == "--induced") { o.induced = true; continue; }
        if (a == "--allow-large") { o.allow_large = true; continue; }
        if (a == "--timing") { o.timing = true; continue; }
        if (a == "--sidecars") { o.sidecars = true; continue; }
        if (a == "--index") { o.write_index = true; continue; }
        if (a == "--same-device") { o.same_device = true; continue; }
        if (a == "--strict") { o.strict = true; continue; }
        if (a == "--exact") { o.exact = true; continue; }
        if (a == "--incremental") { o.incremental = true; continue; }
        if (a == "--standing") { o.standing = true; continue; }
        if (a.rfind("--", 0) == 0) {
            std::string name = a.substr(2);
            size_t eq = name.find('=');
            bool has_val = eq != std::string::npos;
            if (has_val) { val = name.substr(eq + 1); name = name.substr(0, eq); }
            for (auto &op : opts) if (name == op.l) key = op.s;
            if (!key) die("unknown option " + a);
            if (!has_val) { if (i + 1 >= argc) die(a + " needs a value"); val = argv[++i]; }
        } else if (a.size() >= 2 && a[0] == '-') {
            for (auto &op : opts) if (a[1] == op.s) key = op.s;
            if (!key) die("unknown option " + a);
            if (a.size() > 2) val = a.substr(2);
            else { if (i + 1 >= argc) die(a + " needs a value"); val = argv[++i]; }
        } else {
            die("unexpected argument " + a);
        }
        bool ok = true;
        switch (key) {
        case 'f': o.dataset_path = val; break;
        case 'd': o.data_graph = val; break;
        case 'q': o.query_graph = val; break;
        case 'm': o.mode = val; break;
        case 'n': o.answers = val; break;
        case 'p': ok = parse_u32(val, &o.partition_num); break;
        case 'l': ok = parse_u32(val, &o.path_length); break;
        case 'e': ok = parse_u32(val, &o.vde_dim); break;
        }
        if (!ok) die("bad value for -" + std::string(1, key) + ": " + val);
    }
    return o;
}

// The reference's block file seeks with 32-bit offsets (`fseek(fp, (bnum - act_block) * blocklength, SEEK_CUR)`,
// include/blockfile/blk_file.h:33): an index.dat of 2 GiB or more -- its own insert-built ones included -- breaks its
// online run.  The file is still written (other consumers may read it); the user is told to use more partitions.
inline void warn_if_index_too_large_for_reference(const std::string &path)
{
    struct stat st;
    if (stat(path.c_str(), &st) == 0 && (uint64_t)st.st_size >= (1ull << 31))
        fprintf(stderr, "%s: warning: %s is %.2f GiB; the reference's online binary cannot seek in index files of 2 GiB or more "
                        "(blk_file.h:33) -- use a larger -p\n", g_tool, path.c_str(), st.st_size / 1073741824.0);
}

// directory of the running binary, with the trailing slash ("" when /proc/self/exe cannot be read): where libgnnpe_online.so lives
inline std::string exe_dir()
{
    char buf[4096];
    const ssize_t k = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    if (k <= 0) return "";
    buf[k] = 0;
    std::string s(buf);
    const size_t cut = s.rfind('/');
    return cut == std::string::npos ? "" : s.substr(0, cut + 1);
}

// -m online: libgnnpe_online.so (include/gnnpe_online.h), which lives beside the binary and is never linked against
inline void *open_online(const char *tool)
{
    void *online = dlopen((exe_dir() + "libgnnpe_online.so").c_str(), RTLD_NOW | RTLD_GLOBAL);
    if (!online) online = dlopen("libgnnpe_online.so", RTLD_NOW | RTLD_GLOBAL);
    if (!online) die(std::string("-m online needs libgnnpe_online.so beside ") + tool + ": " + dlerror());
    return online;
}

// A function of that library, typed from its declaration in the header: ONLINE(gnnpe_refine)(ctx, ...) where `online` is the
// handle.  A call that does not match the declaration does not compile (dlsym itself checks nothing).
template <class F>
F online_sym(void *lib, const char *name)
{
    F fn = (F)dlsym(lib, name);
    if (!fn) die(std::string("libgnnpe_online.so does not export ") + name);
    return fn;
}
#define ONLINE(fn) cli::online_sym<decltype(&fn)>(online, #fn)

// Size of the index.dat a partition of `points` paths becomes, so that the 2 GiB limit above is checked BEFORE anything is
// written: the library's own figure for the builder that will write the file (gnnpe_index_file_bytes: 0 = the pair-major build
// of the single-GPU path, 1 = the tuple-array build of --gpus N; their nodes hold different numbers of entries).
inline uint64_t index_file_bytes(uint64_t points, uint32_t D, int builder) { return gnnpe_index_file_bytes(points, D, builder); }
// --index: the message for a partition whose index.dat would reach 2 GiB (empty when every file stays below), naming the
// smallest -p that keeps partitions of equal size below it.  The caller refuses unless --allow-large.
inline std::string index_size_problem(const std::vector<uint64_t> &part_count, uint64_t P, uint32_t D, int builder)
{
    uint64_t worst = 0;
    uint32_t worst_pid = 0;
    if (index_file_bytes(1, D, builder) == 0)  // no node holds three entries of this width (rtnode.cpp:27-28): nothing to size
        die("--index: an entry of " + std::to_string(D) + " dimensions (" + std::to_string(16ull * D + 4) +
            " bytes) gives a node capacity below 3 in a 4096-byte block; use a smaller -e");
    for (uint32_t i = 0; i < part_count.size(); i++) {
        const uint64_t b = index_file_bytes(part_count[i], D, builder);
        if (b > worst) worst = b, worst_pid = i;
    }
    if (worst < (1ull << 31)) return "";
    uint32_t p_min = (uint32_t)part_count.size();
    while (index_file_bytes((P + p_min - 1) / p_min, D, builder) >= (1ull << 31)) p_min++;
    return "partition " + std::to_string(worst_pid) + " holds " + std::to_string(part_count[worst_pid]) + " paths: its index.dat would be " +
           std::to_string(worst >> 20) + " MiB, and the reference's online binary cannot seek in index files of 2 GiB or more "
           "(blk_file.h:33); partitions of equal size stay below that from -p " + std::to_string(p_min);
}

// R0 onto a context: the rows the enumeration runs on and, for a file that is not a simple graph, the rows as the reference's
// loader holds them (graph_loader.h) for gen_vde and the degree columns
inline int load_graph_into(gnnpe_ctx *ctx, const gnnpe_host::StaticGraph &g)
{
    int rc = gnnpe_load_csr(ctx, g.n, g.enum_offsets().data(), g.enum_neighbors().data(), g.labels.data());
    if (rc != 0 || g.simple) return rc;
    std::vector<uint64_t> off(g.offsets.begin(), g.offsets.end());
    return gnnpe_set_multigraph_rows(ctx, g.n, off.data(), g.neighbors.data());
}

inline bool is_dir(const std::string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

}  // namespace cli
