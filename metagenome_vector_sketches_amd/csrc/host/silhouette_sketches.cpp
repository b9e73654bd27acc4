// silhouette_sketches -- how good is a labelling of the samples of a sketch DB?  Per sample the silhouette, the nearest other
// group and the squared distance to the own group's centroid; per group the medoid, the mean silhouette, the mean distance
// inside the group and the dispersion -- on the MI355X, in the Jaccard distance 1 - k every other analysis here uses, k the
// clamped Jaccard estimate above --floor.  Neither the n x n matrix nor the sample x group table is stored, and the number of
// groups is not bounded (mvs_silhouette, include/mvs_hip.h "Labelling quality").
//
//   silhouette_sketches --db <folder>/ --labels <file> --output <samples.tsv> [--column <c>] [--noise <text>] [--clusters <file>]
//                       [--floor <t>] [--min_norm <x>] [--report <r.txt>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).
// --labels: tab-separated, one line per sample, the name in field 1 and the label in field --column (1-based, default 2): the
//   files cluster_sketches, hdbscan_sketches and dereplicate_sketches write, unchanged, or a plain name<TAB>label file.  Lines
//   that begin with '#' and empty lines are skipped; a line with fewer fields or a name given twice is an error.  A label
//   equal to --noise (default -1) means unlabelled, and so does a sample the file does not name: such samples have a nearest
//   group and belong to none.  With --min_norm x a sample whose norm in vector_norms.txt is below x is left out altogether.
//   Group ids are given in order of first appearance walking the DB's samples.  At least 2 groups.
// --floor t (default 0, in [0, 1)): estimates that do not exceed t count as 0.
// <samples.tsv>, tab-separated, doubles as %.17g, NaN as nan, one line per sample that takes part, in DB order:
//   #sample  label  silhouette  a  b  nearest  centroid_d2            (label: the --noise text for an unlabelled sample)
// --clusters, one line per group in id order:
//   #label  size  medoid  mean_silhouette  mean_within  dispersion    (medoid: a sample's NAME)
// --report: key <TAB> value -- the mean silhouette, the negative silhouettes, groups, the unlabelled, unnamed and left-out
//   samples, the file's names the DB does not have, floor, kernel and wall times.  Every file is written under <file>.part and
//   renamed when complete.
// Exit codes: 1 bad arguments, DB or labels file, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

#include <unordered_map>
#include <unordered_set>

using namespace mvs_host;

namespace {

constexpr const char* kProg = "silhouette_sketches";

struct Options {
    std::string db_folder, labels, output, clusters, report, noise = "-1";
    long column = 2;
    int device = -1;
    double min_norm = 0.0, floor = 0.0;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --labels <file: name<TAB>...<TAB>label per line> --output <file> [--column <int >= 1>] [--noise <text>]"
                 " [--clusters <file>] [--floor <float in [0,1)>] [--min_norm <float>] [--report <file>] [--device <int>] [--help]"
              << std::endl;
}

inline std::string fmt17(double v) {
    if (std::isnan(v)) return "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// name -> label text of the --labels file; 0, or 1 after a message
int read_labels(const std::string& file, long column, std::unordered_map<std::string, std::string>& label_of) {
    std::ifstream in(file);
    if (!in) {
        std::cerr << kProg << ": cannot read " << file << std::endl;
        return 1;
    }
    std::string line;
    for (int64_t no = 1; std::getline(in, line); ++no) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        std::string name, label;
        size_t at = 0;
        bool found = column == 1;
        for (long f = 1; at <= line.size(); ++f) {
            size_t tab = line.find('\t', at);
            if (tab == std::string::npos) tab = line.size();
            if (f == 1) name = line.substr(at, tab - at);
            if (f == column) {
                label = line.substr(at, tab - at);
                found = true;
                break;
            }
            at = tab + 1;
        }
        if (!found || name.empty() || label.empty()) {
            std::cerr << kProg << ": " << file << " line " << no << ": expected a name and a label in field " << column << std::endl;
            return 1;
        }
        if (!label_of.emplace(name, label).second) {
            std::cerr << kProg << ": " << file << " line " << no << ": " << name << " appears twice" << std::endl;
            return 1;
        }
    }
    return 0;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet loaded, kept;
};

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall0 = std::chrono::steady_clock::now();
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--labels", &o.labels, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--clusters", &o.clusters),
        path_flag("--report", &o.report),
        path_flag("--noise", &o.noise),
        integer_flag("--column", &o.column, 1, 1000000, "--column takes a field number, 1 or more"),
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
    std::unordered_map<std::string, std::string> label_of;
    if (const int rc = read_labels(o.labels, o.column, label_of)) return rc;

    // who takes part, and the group ids in order of first appearance
    std::vector<double> norms;
    if (have_min_norm) norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
    std::vector<int32_t> order, labels;
    std::vector<std::string> group_names;
    std::unordered_map<std::string, int32_t> id_of;
    std::unordered_set<std::string> seen;                       // the file's names the DB has
    int64_t unnamed = 0, noise = 0, below_norm = 0;
    for (int64_t i = 0; i < n; ++i) {
        const auto it = label_of.find(sdb.info.names[(size_t)i]);
        if (it != label_of.end()) seen.insert(it->first);
        if (have_min_norm && !(i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm)) {
            ++below_norm;
            continue;
        }
        int32_t id = -1;
        if (it == label_of.end()) {
            ++unnamed;
        } else if (it->second == o.noise) {
            ++noise;
        } else {
            const auto ins = id_of.emplace(it->second, (int32_t)group_names.size());
            if (ins.second) group_names.push_back(it->second);
            id = ins.first->second;
        }
        order.push_back((int32_t)i);
        labels.push_back(id);
    }
    const int64_t unknown_names = (int64_t)(label_of.size() - seen.size());
    const int64_t m = (int64_t)order.size(), G = (int64_t)group_names.size();
    if (G < 2) {
        std::cerr << kProg << ": " << G << " groups among the " << m << " samples that take part (a silhouette needs at least two"
                  << (have_min_norm ? "; lower --min_norm" : "") << ")" << std::endl;
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
    mvs_silhouette_result res{};
    std::vector<int64_t> sizes((size_t)G), medoids((size_t)G);
    std::vector<int32_t> nearest((size_t)m);
    std::vector<double> sil((size_t)m), a((size_t)m), b((size_t)m), c2((size_t)m), g_mean((size_t)G), g_within((size_t)G), g_disp((size_t)G);
    if (mvs_silhouette(g.ctx, set, norms_sq.data(), MVS_MEM_HOST, o.floor, 0, m, labels.data(), (int)G, &res, sizes.data(), nearest.data(), sil.data(),
                       a.data(), b.data(), c2.data(), g_mean.data(), g_within.data(), g_disp.data(), medoids.data()) != MVS_OK)
        return gpu_fail(kProg, "computing the sums");
    double dots_ms = 0.0, reduce_ms = 0.0, gather_ms = 0.0;
    int64_t row_blocks = 0, block_rows = 0;
    mvs_ctx_label_stats(g.ctx, &dots_ms, &reduce_ms, &gather_ms, &row_blocks, &block_rows);

    auto name_of = [&](int64_t r) -> const std::string& { return sdb.info.names[(size_t)order[(size_t)r]]; };
    std::string text = "#sample\tlabel\tsilhouette\ta\tb\tnearest\tcentroid_d2\n";
    for (int64_t r = 0; r < m; ++r) {
        const int32_t id = labels[(size_t)r], h = nearest[(size_t)r];
        text += name_of(r) + '\t' + (id >= 0 ? group_names[(size_t)id] : o.noise) + '\t' + fmt17(sil[(size_t)r]) + '\t' + fmt17(a[(size_t)r]) + '\t' +
                fmt17(b[(size_t)r]) + '\t' + (h >= 0 ? group_names[(size_t)h] : o.noise) + '\t' + fmt17(c2[(size_t)r]) + '\n';
    }
    if (!o.clusters.empty()) {
        std::string cl = "#label\tsize\tmedoid\tmean_silhouette\tmean_within\tdispersion\n";
        for (int64_t k = 0; k < G; ++k)
            cl += group_names[(size_t)k] + '\t' + std::to_string(sizes[(size_t)k]) + '\t' + name_of(medoids[(size_t)k]) + '\t' + fmt17(g_mean[(size_t)k]) +
                  '\t' + fmt17(g_within[(size_t)k]) + '\t' + fmt17(g_disp[(size_t)k]) + '\n';
        if (const int rc = write_then_rename(kProg, o.clusters, cl)) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (!o.report.empty()) {
        const std::string rep = "samples\t" + std::to_string(n) + "\ntaking_part\t" + std::to_string(m) + "\nlabelled\t" + std::to_string(res.labelled) +
                                "\ngroups\t" + std::to_string(G) + "\nmean_silhouette\t" + fmt17(res.mean) + "\nnegative_silhouettes\t" +
                                std::to_string(res.negative) + "\nunlabelled_noise\t" + std::to_string(noise) + "\nunlabelled_unnamed\t" +
                                std::to_string(unnamed) + "\nexcluded_min_norm\t" + std::to_string(below_norm) + "\nunknown_names\t" +
                                std::to_string(unknown_names) + "\ndimension\t" + std::to_string(sdb.dimension) + "\nfloor\t" + fmt9(o.floor) +
                                "\ndots_ms\t" + fmt9(dots_ms) + "\nreduce_ms\t" + fmt9(reduce_ms) + "\ngather_ms\t" + fmt9(gather_ms) + "\nrow_blocks\t" +
                                std::to_string(row_blocks) + "\nblock_rows\t" + std::to_string(block_rows) + "\nwall_ms\t" + fmt9(wall_ms) + '\n';
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Silhouette of " << G << " groups on " << res.labelled << " labelled of " << m << " samples: mean " << fmt9(res.mean) << ", "
              << res.negative << " negative (dots " << fmt9(dots_ms) << " ms, reduce " << fmt9(reduce_ms) << " ms)" << std::endl;
    return 0;
}
