// communities_sketches -- modularity communities (Louvain with a connected split) of the samples of a sketch DB, computed on
// the MI355X.  The reference has no such tool.  The graph is the comparison's kept cells above a floor with the weight
// a = rint(k * 2^20) of include/mvs_hip.h "Communities"; everything is an integer, so the files are the same whatever the
// blocking.  No cell leaves the device (mvs_communities).
//
//   communities_sketches --db <folder>/ --output <communities.tsv> [--floor <t>] [--resolution <g>] [--min_norm <x>]
//                        [--max_rounds <r>] [--levels <file>] [--clusters <file>] [--report <file>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt, vectors.bin).
// --floor t       Jaccard estimates at or below t are no edges (0 < t < 1, default 0.05)
// --resolution g  2^-12 <= g <= 16, default 1: larger values give smaller communities
// --min_norm x    a sample whose norm in vector_norms.txt is below x is left out: it links to nothing and its community is -1
// --max_rounds r  rounds of local moving per level at most (default 100)
// Output, tab-separated, under <file>.part until complete; doubles as %.17g:
//   --output    #sample  community  size  degree  strength          one line per sample in DB order; communities numbered in the
//               order of their first sample; strength = the sum of the sample's edge weights (as Jaccard estimates).
//               silhouette_sketches --labels reads column 2 unchanged.
//   --clusters  #community  size  representative  internal_weight  total_strength      representative: the member of largest norm
//               (ties: the first); internal_weight = the weights inside, each edge once; total_strength = the members' strengths
//   --levels    #sample  level_0  level_1 ...      the membership after every level (before the connected split)
//   --report    key<TAB>value lines: samples, excluded_min_norm, edges, total_weight, communities, split (communities the connected
//               split added), modularity, then level / communities / rounds / modularity per level, then the kernel times
// One line on stdout.  Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

#include <cmath>

using namespace mvs_host;

namespace {

constexpr const char* kProg = "communities_sketches";

struct Options {
    std::string db_folder, output, levels, clusters, report;
    double floor = 0.05, resolution = 1.0, min_norm = 0.0;
    long max_rounds = 100;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --output <file> [--floor <float in (0,1)>] [--resolution <float in [2^-12,16]>] [--min_norm <float>]"
              << " [--max_rounds <int>] [--levels <file>] [--clusters <file>] [--report <file>] [--device <int>] [--help]" << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
};

std::string fmt17(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// hi * 2^64 + lo in two's complement, as a long double
long double wide(uint64_t hi, uint64_t lo) {
    const bool neg = hi >> 63;
    if (neg) {
        lo = ~lo + 1;
        hi = ~hi + (lo == 0 ? 1 : 0);
    }
    const long double v = std::ldexp((long double)hi, 64) + (long double)lo;
    return neg ? -v : v;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--levels", &o.levels),
        path_flag("--clusters", &o.clusters),
        path_flag("--report", &o.report),
        number_flag("--floor", &o.floor, in_open_unit, "--floor takes a number in the open range (0, 1)"),
        number_flag("--resolution", &o.resolution, [](double g) { return g >= 1.0 / 4096.0 && g <= 16.0; },
                    "--resolution takes a number in [2^-12, 16]"),
        number_flag("--min_norm", &o.min_norm, not_nan, "--min_norm takes a number"),
        integer_flag("--max_rounds", &o.max_rounds, 1, 1L << 30, "--max_rounds takes an integer, 1 or more"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    const bool have_min_norm = was_given(flags, "--min_norm");
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;
    // a sample below --min_norm gets a NaN norm: it links to nothing (the comparison's rule) and no cell of it has a weight
    std::vector<double> norms_sq = db.norms_sq;
    std::vector<char> out_of_it((size_t)n, 0);
    int64_t excluded = 0;
    if (have_min_norm) {
        const std::vector<double> norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
        for (int64_t i = 0; i < n; ++i)
            if (!(i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm)) {
                out_of_it[(size_t)i] = 1;
                norms_sq[(size_t)i] = std::nan("");
                ++excluded;
            }
        if (excluded == n && n > 0) {
            std::cerr << kProg << ": 0 samples take part (see --min_norm)" << std::endl;
            return 1;
        }
    }

    const int cap = MVS_COMMUNITY_MAX_LEVELS;
    std::vector<int32_t> labels((size_t)n), degree((size_t)n), level_labels;
    std::vector<uint64_t> strength((size_t)n), internal((size_t)n), total((size_t)n), qhi((size_t)cap), qlo((size_t)cap);
    std::vector<int64_t> lcomm((size_t)cap), lrounds((size_t)cap);
    mvs_community_result res{};
    double ms[5] = {0, 0, 0, 0, 0};
    int64_t row_blocks = 0;
    if (n > 0) {
        level_labels.resize((size_t)cap * (size_t)n);
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        if (!o.report.empty()) mvs_ctx_set_timing(g.ctx, 1);
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (mvs_communities(g.ctx, g.set, norms_sq.data(), MVS_MEM_HOST, o.floor, o.resolution, o.max_rounds, labels.data(), level_labels.data(),
                            cap, degree.data(), strength.data(), internal.data(), total.data(), MVS_MEM_HOST, lcomm.data(), lrounds.data(),
                            qhi.data(), qlo.data(), &res) != MVS_OK)
            return gpu_fail(kProg, "finding the communities");
        mvs_ctx_community_stats(g.ctx, &ms[0], &ms[1], &ms[2], &ms[3], &ms[4], nullptr, nullptr, nullptr, &row_blocks, nullptr, nullptr, nullptr);
    }
    // the communities of the samples that take part, numbered in the order of their first sample
    std::vector<int32_t> new_id((size_t)res.communities, -1);
    std::vector<int64_t> sizes, rep;
    std::vector<uint64_t> c_internal, c_total;
    for (int64_t i = 0; i < n; ++i) {
        if (out_of_it[(size_t)i]) {
            labels[(size_t)i] = -1;
            continue;
        }
        const int32_t old = labels[(size_t)i];
        if (new_id[(size_t)old] < 0) {
            new_id[(size_t)old] = (int32_t)sizes.size();
            sizes.push_back(0);
            rep.push_back(i);
            c_internal.push_back(internal[(size_t)old]);
            c_total.push_back(total[(size_t)old]);
        }
        const int32_t c = new_id[(size_t)old];
        labels[(size_t)i] = c;
        ++sizes[(size_t)c];
        if (db.norms_sq[(size_t)i] > db.norms_sq[(size_t)rep[(size_t)c]]) rep[(size_t)c] = i;
    }
    const double unit = 1.0 / 1048576.0;
    const long double rw2 = 4096.0L * (long double)res.total_weight * (long double)res.total_weight;
    auto modularity = [&](uint64_t hi, uint64_t lo) { return res.total_weight ? (double)(wide(hi, lo) / rw2) : 0.0; };

    std::ostringstream text;
    text << "#sample\tcommunity\tsize\tdegree\tstrength\n";
    for (int64_t i = 0; i < n; ++i) {
        const int32_t c = labels[(size_t)i];
        text << db.names[(size_t)i] << '\t' << c << '\t' << (c < 0 ? 0 : sizes[(size_t)c]) << '\t' << degree[(size_t)i] << '\t'
             << fmt17((double)strength[(size_t)i] * unit) << '\n';
    }
    if (const int rc = write_then_rename(kProg, o.output, text.str())) return rc;
    if (!o.clusters.empty()) {
        std::ostringstream ct;
        ct << "#community\tsize\trepresentative\tinternal_weight\ttotal_strength\n";
        for (size_t c = 0; c < sizes.size(); ++c)
            ct << c << '\t' << sizes[c] << '\t' << db.names[(size_t)rep[c]] << '\t' << fmt17((double)(c_internal[c] / 2) * unit) << '\t'
               << fmt17((double)c_total[c] * unit) << '\n';
        if (const int rc = write_then_rename(kProg, o.clusters, ct.str())) return rc;
    }
    if (!o.levels.empty()) {
        std::ostringstream lt;
        lt << "#sample";
        for (int64_t l = 0; l < res.levels; ++l) lt << "\tlevel_" << l;
        lt << '\n';
        for (int64_t i = 0; i < n; ++i) {
            lt << db.names[(size_t)i];
            for (int64_t l = 0; l < res.levels; ++l) lt << '\t' << level_labels[(size_t)l * (size_t)n + (size_t)i];
            lt << '\n';
        }
        if (const int rc = write_then_rename(kProg, o.levels, lt.str())) return rc;
    }
    const double q = modularity(res.qnum_hi, res.qnum_lo);
    if (!o.report.empty()) {
        std::ostringstream rt;
        rt << "samples\t" << n << "\nexcluded_min_norm\t" << excluded << "\nfloor\t" << fmt17(o.floor) << "\nresolution\t" << fmt17(o.resolution)
           << "\nedges\t" << res.edges << "\ntotal_weight\t" << res.total_weight << "\ncommunities\t" << sizes.size() << "\nsplit\t"
           << (res.communities - res.composed) << "\nmodularity\t" << fmt17(q) << "\nlevels\t" << res.levels << "\n";
        for (int64_t l = 0; l < res.levels; ++l)
            rt << "level\t" << l << "\tcommunities\t" << lcomm[(size_t)l] << "\trounds\t" << lrounds[(size_t)l] << "\tmodularity\t"
               << fmt17(modularity(qhi[(size_t)l], qlo[(size_t)l])) << "\n";
        rt << "row_blocks\t" << row_blocks << "\ncompare_ms\t" << fmt17(ms[0]) << "\nbuild_ms\t" << fmt17(ms[1]) << "\nmove_ms\t" << fmt17(ms[2])
           << "\naggregate_ms\t" << fmt17(ms[3]) << "\n";
        if (const int rc = write_then_rename(kProg, o.report, rt.str())) return rc;
    }
    std::cout << "Communities of " << (n - excluded) << " samples at Jaccard > " << o.floor << ", resolution " << o.resolution << ": "
              << res.edges << " edges, " << sizes.size() << " communities, modularity " << fmt9(q) << ", " << res.levels << " levels" << std::endl;
    return 0;
}
