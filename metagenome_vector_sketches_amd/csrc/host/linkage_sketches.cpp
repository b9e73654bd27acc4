// linkage_sketches -- the single-linkage tree of the samples of a sketch DB, computed on the MI355X: the maximum spanning
// forest of the graph "Jaccard estimate > t".  One comparison at the lowest level of interest answers every higher level:
// the links above a level u >= t connect exactly the clusters cluster_sketches would report at u.  The reference has no
// such tool.  The comparison's kept cells never leave the device (mvs_pairwise_linkage); the answer is one line per link.
//
//   linkage_sketches --db <folder>/ --min_jaccard <t> --output <file> [--cut <level>]... [--device <i>] [--help]
//
// Reads the DB the way cluster_sketches does (dimension.txt, dtype.txt, vector_norms.txt, vectors.bin).  The output is
// tab-separated, written under <file>.part and renamed when complete, one line per link, best first:
//   #rank  sample_a  sample_b  jaccard  dot  size
// rank from 0, the samples' NAMES (a before b in DB order), the link's Jaccard estimate (:661-662, %.17g), the dot, and the
// size of the merged cluster after this link.  Each --cut <u> (t <= u < 1) adds <file>.cut<k>.tsv, k = 0, 1, ... in
// command-line order:
//   #sample  cluster  representative  size
// one line per sample in DB order, by cluster_sketches' definitions at level u (no degree column: the tree does not know the
// graph's degrees), built on the device from the links above u (mvs_linkage_cells -> mvs_cluster_*).  One line on stdout:
//   Linked <n> samples at Jaccard > <t>: <L> links, <C> components, weakest link <J>        (<J> = "none" without a link)
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "linkage_sketches";

struct Options {
    std::string db_folder, output;
    double min_jaccard = 0.0;
    std::vector<double> cuts;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0 << " --db <folder> --min_jaccard <float in (0,1)> --output <file> [--cut <float in [min_jaccard,1)>]... [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
    DeviceMem d_cells;
    Owned<mvs_linkage, mvs_linkage_destroy> linkage;
    Owned<mvs_cluster, mvs_cluster_destroy> cluster;
};

std::string g17(double v) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    const char* cut_refusal = "--cut takes a number in [min_jaccard,1)";
    auto take_cut = [&o](const std::string& v) {
        double u = 0.0;
        return parse_number(v, &u) && in_open_unit(u) ? (o.cuts.push_back(u), true) : false;
    };
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        number_flag("--min_jaccard", &o.min_jaccard, in_open_unit, "--min_jaccard takes a number in the open range (0,1)", kRefuse),
        hook_flag("--cut", take_cut, cut_refusal),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags);
    for (double u : o.cuts)
        if (u < o.min_jaccard) args.refuse(cut_refusal);                 // a level below the one the tree is built at
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;

    std::vector<mvs_link> links((size_t)std::max<int64_t>(n, 1));
    int64_t n_links = 0;
    std::vector<std::string> cut_texts;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (mvs_linkage_create(g.ctx, n, sdb.dimension, db.norms_sq.data(), MVS_MEM_HOST, &g.linkage) != MVS_OK)
            return gpu_fail(kProg, "allocating the forest");
        if (mvs_pairwise_linkage(g.ctx, g.set, db.norms_sq.data(), MVS_MEM_HOST, o.min_jaccard, g.linkage) != MVS_OK)
            return gpu_fail(kProg, "comparing");
        if (mvs_linkage_finish(g.linkage, links.data(), (int64_t)links.size(), MVS_MEM_HOST, &n_links) != MVS_OK)
            return gpu_fail(kProg, "sorting the links");
        if (!o.cuts.empty() && g.d_cells.alloc(g.ctx, (size_t)n * sizeof(mvs_cell)) != MVS_OK)
            return gpu_fail(kProg, "allocating the cell buffer");
        std::vector<int32_t> labels((size_t)n), reps((size_t)n), sizes((size_t)n);
        for (double u : o.cuts) {
            int64_t m = 0, n_clusters = 0;
            if (mvs_linkage_cells(g.linkage, u, (mvs_cell*)g.d_cells.p, n, &m) != MVS_OK) return gpu_fail(kProg, "listing the links above a cut");
            if (mvs_cluster_create(g.ctx, n, &g.cluster) != MVS_OK) return gpu_fail(kProg, "allocating a cut's clusters");
            if (mvs_cluster_add_cells(g.cluster, (const mvs_cell*)g.d_cells.p, m) != MVS_OK) return gpu_fail(kProg, "clustering a cut");
            if (mvs_cluster_finish(g.cluster, db.norms_sq.data(), MVS_MEM_HOST, labels.data(), nullptr, reps.data(), sizes.data(),
                                   MVS_MEM_HOST, &n_clusters) != MVS_OK)
                return gpu_fail(kProg, "numbering a cut's clusters");
            g.cluster.reset();
            std::ostringstream text;
            text << "#sample\tcluster\trepresentative\tsize\n";
            for (int64_t i = 0; i < n; ++i) {
                const int32_t c = labels[(size_t)i];
                text << db.names[(size_t)i] << '\t' << c << '\t' << db.names[(size_t)reps[(size_t)c]] << '\t' << sizes[(size_t)c] << '\n';
            }
            cut_texts.push_back(text.str());
        }
    } else {
        cut_texts.assign(o.cuts.size(), "#sample\tcluster\trepresentative\tsize\n");
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
    std::ostringstream text;
    text << "#rank\tsample_a\tsample_b\tjaccard\tdot\tsize\n";
    for (int64_t i = 0; i < n_links; ++i) {
        const mvs_link& l = links[(size_t)i];
        int64_t ra = find(l.a);
        const int64_t rb = find(l.b);
        if (ra != rb) {
            parent[(size_t)rb] = ra;
            size[(size_t)ra] += size[(size_t)rb];
        }
        text << i << '\t' << db.names[(size_t)l.a] << '\t' << db.names[(size_t)l.b] << '\t' << g17(l.jaccard) << '\t' << l.dot << '\t'
             << size[(size_t)ra] << '\n';
    }
    for (size_t k = 0; k < cut_texts.size(); ++k) {
        if (const int rc = write_then_rename(kProg, o.output + ".cut" + std::to_string(k) + ".tsv", cut_texts[k])) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, text.str())) return rc;
    std::cout << "Linked " << n << " samples at Jaccard > " << o.min_jaccard << ": " << n_links << " links, " << n - n_links
              << " components, weakest link " << (n_links ? g17(links[(size_t)n_links - 1].jaccard) : std::string("none")) << std::endl;
    return 0;
}
