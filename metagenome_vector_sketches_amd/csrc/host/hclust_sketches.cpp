// hclust_sketches -- the agglomerative tree of the samples of a sketch DB under average linkage (UPGMA) or complete linkage, on
// the MI355X, in the Jaccard distance 1 - k every other analysis here uses, k the clamped Jaccard estimate above --floor.  Where
// linkage_sketches (single linkage) chains, these do not; they keep the m x m table of integer sums on the device, 8 m^2 bytes,
// and return records that do not depend on any blocking (mvs_hclust, include/mvs_hip.h "Average and complete linkage").
//
//   hclust_sketches --db <folder>/ --output <merges.tsv> [--method average|complete] [--floor <t>] [--min_norm <x>]
//                   [--cut <u>]... [--clusters <K>]... [--newick <tree.nwk>] [--report <r.txt>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).  With
// --min_norm x a sample whose norm in vector_norms.txt is below x is left out.  At most 131072 samples take part.
// <merges.tsv>, tab-separated, doubles as %.17g, one line per merge in (height, round, slot) order -- SciPy's linkage matrix
// with the names beside it; a leaf's id is its index among the samples that take part, the t-th line's id is m + t:
//   #id  left  right  height  size  round  rep_left  rep_right         (rep: the NAME of the cluster's first sample in DB order)
// --cut u: the clusters after every merge with height <= u; --clusters K: the first m - K merges, K clusters.  Each of them, in
//   the order given, writes <merges.tsv>.cut<k>.tsv, k = 1, 2, ...: name <TAB> label for every sample of the DB, labels 0-based
//   in order of each cluster's first sample, -1 for a sample --min_norm left out.  silhouette_sketches --labels reads these.
// --newick: the rooted tree, a leaf at height 0, every branch as long as the parent's height minus the child's; names quoted
//   where Newick asks for it.
// --report: key <TAB> value -- samples taking part and left out, method, floor, rounds, the table's bytes, kernel times, row
//   scans and the bytes they read, compactions, the largest height, one line per cut file.  Every file is written under
//   <file>.part and renamed when complete.
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

#include <cstring>

using namespace mvs_host;

namespace {

constexpr const char* kProg = "hclust_sketches";

struct Cut {
    bool by_count;
    double level;
    long count;
};

struct Options {
    std::string db_folder, output, newick, report;
    std::vector<Cut> cuts;
    int method = MVS_HCLUST_AVERAGE, device = -1;
    double min_norm = 0.0, floor = 0.0;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --output <file> [--method average|complete] [--floor <float in [0,1)>] [--min_norm <float>] [--cut <height>]..."
                 " [--clusters <int >= 1>]... [--newick <file>] [--report <file>] [--device <int>] [--help]"
              << std::endl;
}

inline std::string fmt17(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// a Newick label: as it is, or in single quotes (a quote doubled) where it holds a character an unquoted label may not --
// blanks, brackets, quotes, ':', ';', ',' -- or an underscore, which an unquoted label would turn into a blank
std::string newick_name(const std::string& name) {
    bool plain = !name.empty();
    for (const char ch : name)
        if (ch <= ' ' || ch == 0x7f || std::strchr("()[]':;,_", ch)) plain = false;
    if (plain) return name;
    std::string q = "'";
    for (const char ch : name) {
        q += ch;
        if (ch == '\'') q += ch;
    }
    return q + "'";
}

// the tree of Z (m leaves) as Newick, without recursion: a chain of 10^5 merges is as deep
std::string newick_text(int64_t m, const std::vector<double>& Z, const std::vector<std::string>& leaf_names) {
    if (m == 1) return newick_name(leaf_names[0]) + ";\n";
    auto height_of = [&](int64_t id) { return id < m ? 0.0 : Z[(size_t)(4 * (id - m) + 2)]; };
    struct Frame {
        int64_t id, parent;
        int next;                                                // children written so far
    };
    std::string text;
    std::vector<Frame> stack{{2 * m - 2, -1, 0}};
    while (!stack.empty()) {
        Frame& f = stack.back();
        if (f.id >= m && f.next < 2) {
            text += f.next == 0 ? '(' : ',';
            const int64_t child = (int64_t)Z[(size_t)(4 * (f.id - m) + f.next)];
            ++f.next;
            const int64_t id = f.id;
            stack.push_back({child, id, 0});                     // (f is stale from here)
            continue;
        }
        if (f.id >= m) text += ')';
        else text += newick_name(leaf_names[(size_t)f.id]);
        if (f.parent >= 0) text += ':' + fmt17(height_of(f.parent) - height_of(f.id));
        stack.pop_back();
    }
    return text + ";\n";
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet loaded, kept;
};

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall0 = std::chrono::steady_clock::now();
    Options o;
    // --cut and --clusters fill one list, in the order given: the cut files are numbered by it
    auto take_cut = [&o](const std::string& v) {
        double u = 0.0;
        return parse_number(v, &u) && !std::isnan(u) ? (o.cuts.push_back({false, u, 0}), true) : false;
    };
    auto take_clusters = [&o](const std::string& v) {
        long k = 0;
        return parse_integer(v, &k) && k >= 1 && k <= MVS_HCLUST_MAX_TOTAL ? (o.cuts.push_back({true, 0.0, k}), true) : false;
    };
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--newick", &o.newick),
        path_flag("--report", &o.report),
        word_flag("--method", &o.method, {{"average", MVS_HCLUST_AVERAGE}, {"complete", MVS_HCLUST_COMPLETE}}, "--method takes average or complete"),
        hook_flag("--cut", take_cut, "--cut takes a height, a number"),
        hook_flag("--clusters", take_clusters, "--clusters takes a number of clusters, 1 .. " + std::to_string(MVS_HCLUST_MAX_TOTAL)),
        number_flag("--min_norm", &o.min_norm, not_nan, "--min_norm takes a number"),
        number_flag("--floor", &o.floor, in_half_open_unit, "--floor takes a number in [0, 1)"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    const bool have_min_norm = was_given(flags, "--min_norm");
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const int64_t n = sdb.n;

    // who takes part
    std::vector<double> norms;
    if (have_min_norm) norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
    std::vector<int32_t> order;
    for (int64_t i = 0; i < n; ++i)
        if (!have_min_norm || (i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm)) order.push_back((int32_t)i);
    const int64_t m = (int64_t)order.size();
    if (m < 1 || m > MVS_HCLUST_MAX_TOTAL) {
        std::cerr << kProg << ": " << m << " samples take part; a tree takes 1 .. " << MVS_HCLUST_MAX_TOTAL
                  << (have_min_norm ? " (see --min_norm)" : "") << std::endl;
        return 1;
    }
    for (const Cut& c : o.cuts)
        if (c.by_count && c.count > m) {
            std::cerr << kProg << ": --clusters " << c.count << " among the " << m << " samples that take part" << std::endl;
            return 1;
        }
    std::vector<double> norms_sq((size_t)m);
    for (int64_t r = 0; r < m; ++r) norms_sq[(size_t)r] = sdb.info.norms_sq[(size_t)order[(size_t)r]];

    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.loaded)) return rc;
    const mvs_sketch_set* set = g.loaded;
    if (m < n) {                                                 // (else the loaded set is the set of those that take part)
        if (mvs_sketch_set_gather(g.ctx, g.loaded, order.data(), MVS_MEM_HOST, m, &g.kept) != MVS_OK)
            return gpu_fail(kProg, "gathering the samples that take part");
        set = g.kept;
        g.loaded.reset();
    }
    std::vector<mvs_hmerge> merges((size_t)std::max<int64_t>(1, m - 1));
    int64_t rounds = 0;
    if (mvs_hclust(g.ctx, set, norms_sq.data(), MVS_MEM_HOST, o.floor, 0, m, o.method, merges.data(), &rounds) != MVS_OK)
        return gpu_fail(kProg, "building the tree");
    double dots_ms = 0.0, fill_ms = 0.0, nearest_ms = 0.0, merge_ms = 0.0, compact_ms = 0.0;
    int64_t row_scans = 0, bytes_scanned = 0, compactions = 0;
    mvs_ctx_hclust_stats(g.ctx, &dots_ms, &fill_ms, &nearest_ms, &merge_ms, &compact_ms, nullptr, &row_scans, &bytes_scanned, &compactions);

    // the sorted tree; the first sample of every cluster id
    std::vector<double> Z((size_t)(4 * std::max<int64_t>(1, m - 1)));
    if (mvs_hclust_order(m, merges.data(), Z.data()) != MVS_OK) return gpu_fail(kProg, "ordering the merges");
    auto name_of = [&](int64_t r) -> const std::string& { return sdb.info.names[(size_t)order[(size_t)r]]; };
    std::vector<int64_t> first((size_t)(2 * m - 1));
    for (int64_t i = 0; i < m; ++i) first[(size_t)i] = i;
    std::vector<int32_t> round_of((size_t)std::max<int64_t>(1, m - 1));
    {
        std::vector<int64_t> by((size_t)(m - 1));                // the sorted order once more, for the rounds
        for (int64_t t = 0; t < m - 1; ++t) by[(size_t)t] = t;
        std::sort(by.begin(), by.end(), [&](int64_t x, int64_t y) {
            const mvs_hmerge &p = merges[(size_t)x], &q = merges[(size_t)y];
            return p.height != q.height ? p.height < q.height : p.round != q.round ? p.round < q.round : p.a < q.a;
        });
        for (int64_t t = 0; t < m - 1; ++t) round_of[(size_t)t] = merges[(size_t)by[(size_t)t]].round;
    }
    std::string text = "#id\tleft\tright\theight\tsize\tround\trep_left\trep_right\n";
    double top = 0.0;
    for (int64_t t = 0; t < m - 1; ++t) {
        const int64_t l = (int64_t)Z[(size_t)(4 * t)], r = (int64_t)Z[(size_t)(4 * t + 1)];
        first[(size_t)(m + t)] = std::min(first[(size_t)l], first[(size_t)r]);
        top = std::max(top, Z[(size_t)(4 * t + 2)]);
        text += std::to_string(m + t) + '\t' + std::to_string(l) + '\t' + std::to_string(r) + '\t' + fmt17(Z[(size_t)(4 * t + 2)]) + '\t' +
                std::to_string((int64_t)Z[(size_t)(4 * t + 3)]) + '\t' + std::to_string(round_of[(size_t)t]) + '\t' + name_of(first[(size_t)l]) + '\t' +
                name_of(first[(size_t)r]) + '\n';
    }

    std::string cut_report;
    std::vector<int32_t> labels((size_t)m), all((size_t)n);
    for (size_t k = 0; k < o.cuts.size(); ++k) {
        const Cut& c = o.cuts[k];
        const int rc = c.by_count ? mvs_hclust_cut_count(m, merges.data(), c.count, labels.data()) : mvs_hclust_cut(m, merges.data(), c.level, labels.data());
        if (rc != MVS_OK) return gpu_fail(kProg, "cutting the tree");
        std::fill(all.begin(), all.end(), -1);
        int32_t groups = 0;
        for (int64_t r = 0; r < m; ++r) {
            all[(size_t)order[(size_t)r]] = labels[(size_t)r];
            groups = std::max(groups, labels[(size_t)r] + 1);
        }
        std::string cut;
        for (int64_t i = 0; i < n; ++i) cut += sdb.info.names[(size_t)i] + '\t' + std::to_string(all[(size_t)i]) + '\n';
        const std::string file = o.output + ".cut" + std::to_string(k + 1) + ".tsv";
        if (const int wrc = write_then_rename(kProg, file, cut)) return wrc;
        cut_report += "cut" + std::to_string(k + 1) + '\t' + (c.by_count ? "clusters\t" + std::to_string(c.count) : "height\t" + fmt17(c.level)) + '\t' +
                      std::to_string(groups) + '\n';
    }
    if (!o.newick.empty()) {
        std::vector<std::string> leaf_names((size_t)m);
        for (int64_t r = 0; r < m; ++r) leaf_names[(size_t)r] = name_of(r);
        if (const int rc = write_then_rename(kProg, o.newick, newick_text(m, Z, leaf_names))) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    const char* method = o.method == MVS_HCLUST_AVERAGE ? "average" : "complete";
    if (!o.report.empty()) {
        const int64_t ld = (m + 1) & ~(int64_t)1;
        const std::string rep = "samples\t" + std::to_string(n) + "\nfitted\t" + std::to_string(m) + "\nexcluded_min_norm\t" + std::to_string(n - m) +
                                "\nmethod\t" + method + "\ndimension\t" + std::to_string(sdb.dimension) + "\nfloor\t" + fmt9(o.floor) + "\nrounds\t" +
                                std::to_string(rounds) + "\ntable_bytes\t" + std::to_string(8 * m * ld) + "\ndots_ms\t" + fmt9(dots_ms) + "\nfill_ms\t" +
                                fmt9(fill_ms) + "\nnearest_ms\t" + fmt9(nearest_ms) + "\nmerge_ms\t" + fmt9(merge_ms) + "\ncompact_ms\t" +
                                fmt9(compact_ms) + "\nrow_scans\t" + std::to_string(row_scans) + "\nbytes_scanned\t" + std::to_string(bytes_scanned) +
                                "\ncompactions\t" + std::to_string(compactions) + "\nlargest_height\t" + fmt17(top) + '\n' + cut_report + "wall_ms\t" +
                                fmt9(wall_ms) + '\n';
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Tree of " << m << " samples (" << method << " linkage): " << rounds << " rounds, largest height " << fmt9(top) << " (dots "
              << fmt9(dots_ms) << " ms, nearest " << fmt9(nearest_ms) << " ms, merge " << fmt9(merge_ms) << " ms)" << std::endl;
    return 0;
}
