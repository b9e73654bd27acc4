// levels_sketches -- what every Jaccard level would keep of a sketch DB, in one pass on the MI355X: the "choose your threshold"
// step in front of cluster_sketches, linkage_sketches, dereplicate_sketches, verify_pairs and search.py -j.  For each of up to
// 64 levels: the linked pairs, the samples with and without a neighbour, and the mean, median and largest number of
// neighbours per sample (mvs_pairwise_levels, include/mvs_hip.h: the link rule of the clustering evaluated per level, so the
// degrees equal what cluster_sketches reports at that level).  The reference leaves this to a histogram at the end of
// src/interpret_pairwise_comp.py, one run per level.
//
//   levels_sketches --db <folder>/ --output <levels.tsv> [--levels t0,t1,...] [--per_sample <degrees.tsv>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).
// --levels: 1 to 64 strictly ascending numbers in (0,1), separated by commas; default
//   0.01,0.02,0.03,0.05,0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9,0.95,0.99
// <levels.tsv>, tab-separated, a header line and one line per level:
//   level  pairs  linked_samples  isolated_samples  mean_degree  median_degree  max_degree
// level as %.9g; pairs = (sum of the degrees) / 2 -- the rule is symmetric, an odd sum is a fatal internal error (exit 2);
// linked_samples = samples with a degree > 0, isolated_samples the others; mean_degree = sum / samples as %.9g; median_degree
// the median of the samples' degrees (the mean of the two middle ones for an even count) as %.9g; max_degree the largest.
// --per_sample: one line per sample in DB order, its name followed by its degree at every level; the header line is
// "sample" followed by the levels.  Both files are written under <file>.part and renamed when complete.
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "levels_sketches";
constexpr const char* kDefaultLevels = "0.01,0.02,0.03,0.05,0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9,0.95,0.99";

struct Options {
    std::string db_folder, output, per_sample;
    std::vector<double> levels;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --output <file> [--levels <t0,t1,...: 1 to 64 ascending floats in (0,1)>] [--per_sample <file>]"
                 " [--device <int>] [--help]"
              << std::endl;
}

// "t0,t1,..." -> 1 .. MVS_MAX_LEVELS strictly ascending numbers in (0,1)
bool parse_levels(const std::string& v, std::vector<double>& out) {
    out.clear();
    size_t at = 0;
    while (true) {
        const size_t comma = v.find(',', at);
        const std::string tok = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        double t = 0.0;
        if (!parse_number(tok, &t) || !(t > 0.0) || !(t < 1.0)) return false;
        if (!out.empty() && !(out.back() < t)) return false;
        if (out.size() == (size_t)MVS_MAX_LEVELS) return false;
        out.push_back(t);
        if (comma == std::string::npos) return true;
        at = comma + 1;
    }
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
};

std::string fmt(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.9g", v);
    return buf;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--per_sample", &o.per_sample),
        hook_flag("--levels", [&o](const std::string& v) { return parse_levels(v, o.levels); },
                  "--levels takes 1 to 64 strictly ascending numbers in the open range (0,1), separated by commas"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    if (o.levels.empty()) parse_levels(kDefaultLevels, o.levels);
    const int m = (int)o.levels.size();
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;

    std::vector<int32_t> deg((size_t)n * m, 0);
    std::vector<int64_t> totals((size_t)m, 0);
    double dots_ms = 0.0, count_ms = 0.0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        mvs_ctx_set_timing(g.ctx, 1);
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (mvs_pairwise_levels(g.ctx, g.set, db.norms_sq.data(), MVS_MEM_HOST, o.levels.data(), m, 0, n, 0, n, deg.data(), MVS_MEM_HOST,
                                totals.data()) != MVS_OK)
            return gpu_fail(kProg, "counting");
        mvs_ctx_levels_stats(g.ctx, &dots_ms, &count_ms, nullptr, nullptr);
    }

    std::string text = "level\tpairs\tlinked_samples\tisolated_samples\tmean_degree\tmedian_degree\tmax_degree\n";
    std::vector<int32_t> column((size_t)n);
    for (int l = 0; l < m; ++l) {
        int64_t sum = 0, linked = 0;
        for (int64_t i = 0; i < n; ++i) {
            const int32_t v = deg[(size_t)i * m + l];
            column[(size_t)i] = v;
            sum += v;
            linked += v > 0;
        }
        if (sum != totals[(size_t)l] || (sum & 1)) {
            std::cerr << kProg << ": internal error: level " << fmt(o.levels[(size_t)l]) << " has a degree sum of " << sum << " and a total of "
                      << totals[(size_t)l] << " (the rule is symmetric: equal and even)" << std::endl;
            return 2;
        }
        std::sort(column.begin(), column.end());
        double median = 0.0;
        if (n > 0) median = (n & 1) ? (double)column[(size_t)(n / 2)] : ((double)column[(size_t)(n / 2 - 1)] + (double)column[(size_t)(n / 2)]) / 2.0;
        text += fmt(o.levels[(size_t)l]) + '\t' + std::to_string(sum / 2) + '\t' + std::to_string(linked) + '\t' + std::to_string(n - linked) +
                '\t' + fmt(n > 0 ? (double)sum / (double)n : 0.0) + '\t' + fmt(median) + '\t' + std::to_string(n > 0 ? column.back() : 0) + '\n';
    }
    if (!o.per_sample.empty()) {
        std::string per = "sample";
        for (int l = 0; l < m; ++l) per += '\t' + fmt(o.levels[(size_t)l]);
        per += '\n';
        for (int64_t i = 0; i < n; ++i) {
            per += db.names[(size_t)i];
            for (int l = 0; l < m; ++l) per += '\t' + std::to_string(deg[(size_t)i * m + l]);
            per += '\n';
        }
        if (const int rc = write_then_rename(kProg, o.per_sample, per)) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    std::cout << "Counted the neighbours of " << n << " samples at " << m << " levels (dots " << fmt(dots_ms) << " ms, counts " << fmt(count_ms)
              << " ms)" << std::endl;
    return 0;
}
