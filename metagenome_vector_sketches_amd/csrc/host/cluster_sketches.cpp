// cluster_sketches -- single-linkage clusters of the samples of a sketch DB at a Jaccard level, computed on the MI355X.
// The reference has no such tool: there the thresholded matrix is written (src/pairwise_comp_optimized.cpp:645-817), read
// back and grouped by the user.  Here the comparison's kept cells never leave the device (mvs_pairwise_cluster); the answer
// is one line per sample.
//
//   cluster_sketches --db <folder>/ --min_jaccard <t> --output <file> [--min_size <m>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does: dimension.txt, dtype.txt (int32 unless it says int16), vector_norms.txt
// (names and norms, :893-901), vectors.bin.  Two samples are linked iff their Jaccard estimate (:661-662) exceeds t (0 < t < 1);
// a cluster is a connected component.  The output is tab-separated, written under <file>.part and renamed when complete:
//   #sample  cluster  representative  size  degree
// one line per sample in DB order -- its name, its cluster's id (clusters are numbered by ascending first member), the NAME
// of the cluster's representative (the member with the largest norm; ties: the first), the cluster's size and the number of
// samples the sample itself is linked to -- restricted to clusters of at least --min_size members (default 1: everything;
// ids are not renumbered).  One line on stdout:
//   Clustered <n> samples at Jaccard > <t>: <C> clusters, <S> singletons, largest <L>
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "cluster_sketches";

struct Options {
    std::string db_folder, output;
    double min_jaccard = 0.0;
    long min_size = 1;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0 << " --db <folder> --min_jaccard <float in (0,1)> --output <file> [--min_size <int>] [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
    Owned<mvs_cluster, mvs_cluster_destroy> cluster;
};

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        number_flag("--min_jaccard", &o.min_jaccard, in_open_unit, "--min_jaccard takes a number in the open range (0,1)", kRefuse),
        integer_flag("--min_size", &o.min_size, 1, LONG_MAX, "--min_size takes an integer >= 1"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;

    std::vector<int32_t> labels((size_t)n), degree((size_t)n), reps((size_t)n), sizes((size_t)n);
    int64_t n_clusters = 0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (mvs_cluster_create(g.ctx, n, &g.cluster) != MVS_OK) return gpu_fail(kProg, "allocating the forest");
        if (mvs_pairwise_cluster(g.ctx, g.set, db.norms_sq.data(), MVS_MEM_HOST, o.min_jaccard, g.cluster) != MVS_OK)
            return gpu_fail(kProg, "comparing");
        if (mvs_cluster_finish(g.cluster, db.norms_sq.data(), MVS_MEM_HOST, labels.data(), degree.data(), reps.data(), sizes.data(),
                               MVS_MEM_HOST, &n_clusters) != MVS_OK)
            return gpu_fail(kProg, "numbering the clusters");
    }
    int64_t singletons = 0, largest = 0;
    for (int64_t c = 0; c < n_clusters; ++c) {
        singletons += sizes[(size_t)c] == 1;
        largest = std::max<int64_t>(largest, sizes[(size_t)c]);
    }
    std::ostringstream text;
    text << "#sample\tcluster\trepresentative\tsize\tdegree\n";
    for (int64_t i = 0; i < n; ++i) {
        const int32_t c = labels[(size_t)i];
        if (sizes[(size_t)c] < o.min_size) continue;
        text << db.names[(size_t)i] << '\t' << c << '\t' << db.names[(size_t)reps[(size_t)c]] << '\t' << sizes[(size_t)c] << '\t'
             << degree[(size_t)i] << '\n';
    }
    if (const int rc = write_then_rename(kProg, o.output, text.str())) return rc;
    std::cout << "Clustered " << n << " samples at Jaccard > " << o.min_jaccard << ": " << n_clusters << " clusters, " << singletons
              << " singletons, largest " << largest << std::endl;
    return 0;
}
