// hdbscan_sketches -- HDBSCAN* clusters of the samples of a sketch DB, computed on the MI355X: no Jaccard level to choose.
// cluster_sketches and linkage_sketches are single linkage at a level the user must know, and a path of overlapping samples
// becomes one cluster.  Here a pair weighs min(J, core_a, core_b), core the Jaccard estimate of a sample's K-th nearest
// neighbour, the single-linkage tree of that weight is condensed, and clusters are picked by their stability over all levels
// (include/mvs_hip.h "HDBSCAN*").  The reference has no such tool.  Top-k cells and kept cells never leave the device
// (mvs_hdbscan); the selection is integer arithmetic on the host.
//
//   hdbscan_sketches --db <folder>/ --output <file> [--min_samples <K>] [--min_cluster_size <s>] [--floor <t>] [--no_root_clusters]
//                    [--clusters <file>] [--links <file>] [--report <file>] [--device <i>] [--help]
//
// Reads the DB the way cluster_sketches does.  --min_samples 1..256 (default 5; at most samples - 1), --min_cluster_size >= 2
// (default 5), --floor in (0,1) (default 0.05): pairs at or below it are not compared, and a component at the floor is the
// largest cluster there can be; --no_root_clusters never reports such a component when it splits into clusters.  Every output is
// tab-separated, written under <file>.part and renamed when complete, doubles as %.17g, levels as integers (Jaccard x 2^30):
//   --output    #sample  cluster  strength  core_jaccard  lambda_out          one line per sample in DB order; cluster -1 = noise
//   --clusters  #cluster  parent  size  selected  label  representative  birth  death  stability     every condensed cluster
//   --links     #sample_a  sample_b  weight  jaccard  merged_size            the tree, best first; weight = the mutual reachability
//   --report    key <TAB> value: counts, noise, rounds and times
// One line on stdout:  Clustered <n> samples: <C> clusters, <N> noise, <L> links
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "hdbscan_sketches";

struct Options {
    std::string db_folder, output, clusters, links, report;
    long min_samples = 5, min_cluster_size = 5;
    double floor = 0.05;
    int device = -1;
    bool no_roots = false;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --output <file> [--min_samples <int in 1..256>] [--min_cluster_size <int >= 2>] [--floor <float in (0,1)>]"
                 " [--no_root_clusters] [--clusters <file>] [--links <file>] [--report <file>] [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
};

std::string g17(double v) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--clusters", &o.clusters),
        path_flag("--links", &o.links),
        path_flag("--report", &o.report),
        switch_flag("--no_root_clusters", &o.no_roots),
        integer_flag("--min_samples", &o.min_samples, 1, 256, "--min_samples takes an integer from 1 to 256"),
        integer_flag("--min_cluster_size", &o.min_cluster_size, 2, 2147483647L, "--min_cluster_size takes an integer of at least 2"),
        number_flag("--floor", &o.floor, in_open_unit, "--floor takes a number in the open range (0,1)"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;
    if (n > 0 && o.min_samples > n - 1) {
        std::cerr << kProg << ": --min_samples " << o.min_samples << ": a sample of a DB of " << n << " has only " << n - 1 << " neighbours" << std::endl;
        return 1;
    }

    const size_t words = (size_t)std::max<int64_t>(n, 1);
    std::vector<double> core(words), strength(words);
    std::vector<mvs_link> links(words);
    std::vector<int32_t> labels(words);
    std::vector<int64_t> lambda(words);
    std::vector<mvs_hdbscan_cluster> clusters(words);
    int64_t n_links = 0, n_clusters = 0, ranges = 0, rounds = 0, edges = 0;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        if (!o.report.empty()) mvs_ctx_set_timing(g.ctx, 1);
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (mvs_hdbscan(g.ctx, g.set, db.norms_sq.data(), MVS_MEM_HOST, (int)o.min_samples, o.floor, o.min_cluster_size,
                        o.no_roots ? MVS_HDBSCAN_NO_ROOTS : 0, core.data(), links.data(), &n_links, labels.data(), strength.data(), lambda.data(),
                        clusters.data(), (int64_t)clusters.size(), &n_clusters) != MVS_OK)
            return gpu_fail(kProg, "clustering");
        mvs_ctx_hdbscan_stats(g.ctx, &ms[0], &ms[1], &ms[2], &ms[3], &ms[4], &ms[5], &ranges, &rounds, nullptr, &edges);
    }

    int64_t noise = 0, selected = 0;
    std::ostringstream text;
    text << "#sample\tcluster\tstrength\tcore_jaccard\tlambda_out\n";
    for (int64_t i = 0; i < n; ++i) {
        noise += labels[(size_t)i] < 0;
        text << db.names[(size_t)i] << '\t' << labels[(size_t)i] << '\t' << g17(strength[(size_t)i]) << '\t' << g17(core[(size_t)i]) << '\t'
             << lambda[(size_t)i] << '\n';
    }
    std::ostringstream ctext;
    ctext << "#cluster\tparent\tsize\tselected\tlabel\trepresentative\tbirth\tdeath\tstability\n";
    for (int64_t i = 0; i < n_clusters; ++i) {
        const mvs_hdbscan_cluster& c = clusters[(size_t)i];
        ctext << i << '\t' << c.parent << '\t' << c.size << '\t' << c.selected << '\t' << (c.selected ? selected : -1) << '\t'
              << db.names[(size_t)c.representative] << '\t' << c.birth << '\t' << c.death << '\t' << c.stability << '\n';
        selected += c.selected;
    }
    // the size of the merged cluster after each link: a union-find over the links in order
    std::vector<int64_t> parent((size_t)n), size((size_t)n, 1);
    for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = i;
    auto find = [&](int64_t x) {
        while (parent[(size_t)x] != x) {
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    };
    std::ostringstream ltext;
    ltext << "#sample_a\tsample_b\tweight\tjaccard\tmerged_size\n";
    for (int64_t i = 0; i < n_links; ++i) {
        const mvs_link& l = links[(size_t)i];
        int64_t ra = find(l.a);
        const int64_t rb = find(l.b);
        if (ra != rb) {
            parent[(size_t)rb] = ra;
            size[(size_t)ra] += size[(size_t)rb];
        }
        const double inter = (double)l.dot / (double)sdb.dimension;                                        // :661
        const double jac = inter / (db.norms_sq[(size_t)l.a] + db.norms_sq[(size_t)l.b] - inter);           // :662
        ltext << db.names[(size_t)l.a] << '\t' << db.names[(size_t)l.b] << '\t' << g17(l.jaccard) << '\t' << g17(jac) << '\t' << size[(size_t)ra]
              << '\n';
    }
    std::ostringstream rtext;
    rtext << "samples\t" << n << "\nmin_samples\t" << o.min_samples << "\nmin_cluster_size\t" << o.min_cluster_size << "\nfloor\t" << g17(o.floor)
          << "\nroot_clusters\t" << (o.no_roots ? 0 : 1) << "\nclusters\t" << selected << "\ncondensed_clusters\t" << n_clusters << "\nnoise\t" << noise
          << "\nlinks\t" << n_links << "\nedges\t" << edges << "\nrounds\t" << rounds << "\ncore_ranges\t" << ranges << "\ncore_dots_ms\t" << fmt9(ms[0])
          << "\ncore_select_ms\t" << fmt9(ms[1]) << "\ncore_kth_ms\t" << fmt9(ms[2]) << "\ncompare_ms\t" << fmt9(ms[3]) << "\nforest_ms\t" << fmt9(ms[4])
          << "\nhost_ms\t" << fmt9(ms[5]) << "\n";
    if (!o.clusters.empty())
        if (const int rc = write_then_rename(kProg, o.clusters, ctext.str())) return rc;
    if (!o.links.empty())
        if (const int rc = write_then_rename(kProg, o.links, ltext.str())) return rc;
    if (!o.report.empty())
        if (const int rc = write_then_rename(kProg, o.report, rtext.str())) return rc;
    if (const int rc = write_then_rename(kProg, o.output, text.str())) return rc;
    std::cout << "Clustered " << n << " samples: " << selected << " clusters, " << noise << " noise, " << n_links << " links" << std::endl;
    return 0;
}
