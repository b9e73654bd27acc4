// pca_sketches -- PCA ordination of a sketch DB on the MI355X: where every sample lies on the main axes of variation of the DB,
// and where the samples of a second DB lie in that space.  The reference does this in src/clusters.py with scikit-learn on a
// dense float copy of vectors.bin (a PCA of the samples whose norm is at least 10, then the projection of big_vectors.bin);
// here the Gram matrix over the samples is exact (mvs_sketch_moments) and nothing leaves the limb planes (mvs_pca_fit,
// mvs_pca_transform, include/mvs_hip.h "ordination").
//
//   pca_sketches --db <folder>/ --components <c> --output <scores.tsv> [--min_norm <x>] [--axes <axes.tsv>]
//                [--project <folder2>/ --project_output <scores2.tsv>] [--tol <e>] [--max_iters <k>] [--report <r.txt>]
//                [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).
// --components: 1 .. min(64, dimension).  --min_norm x: the fit uses the samples whose norm in vector_norms.txt is at least x
//   (clusters.py uses 10); default: every sample.  At least two samples must remain.
// <scores.tsv>, tab-separated, one line per sample of the DB in DB order, those left out of the fit included:
//   name  fitted(1/0)  pc1 ... pcc          scores as %.9g
// --axes: one line per dimension k: k  mean  pc1 ... pcc (the k-th entry of the mean and of every axis), %.9g.
// --project / --project_output (both or neither): the scores of another DB of the same dimension on the same axes, in the format
//   of <scores.tsv> with fitted = 0.
// --tol (default 1e-10, in [0, 1)), --max_iters (default 300, >= 1): the solver's stopping rule; a fit that did not converge
//   warns on stderr and still writes.  --report: samples fitted, iterations, converged, total variance, per component the
//   variance, its ratio and its residual, the kernel and wall times.
// Every file is written under <file>.part and renamed when complete.
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "pca_sketches";

struct Options {
    std::string db_folder, output, axes, project, project_output, report, bad_flag;
    int components = 0, max_iters = 300, device = -1;
    double min_norm = 0.0, tol = 1e-10;
    bool show_help = false, have_db = false, have_out = false, have_c = false, have_min_norm = false, unknown = false;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --components <int: 1 to 64> --output <file> [--min_norm <float>] [--axes <file>]"
                 " [--project <folder> --project_output <file>] [--tol <float in [0,1)>] [--max_iters <int >= 1>] [--report <file>]"
                 " [--device <int>] [--help]"
              << std::endl;
}

// bad_flag: the first flag whose value is missing, unparsable or out of range (reported before anything is touched)
void parse(int argc, char* argv[], Options& o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_value = i + 1 < argc;
        auto bad = [&](const char* flag) {
            if (o.bad_flag.empty()) o.bad_flag = flag;
        };
        std::string* text = a == "--db" ? &o.db_folder : a == "--output" ? &o.output : a == "--axes" ? &o.axes : a == "--project" ? &o.project
                          : a == "--project_output" ? &o.project_output : a == "--report" ? &o.report : nullptr;
        if (a == "--help") {
            o.show_help = true;
        } else if (text) {
            if (!has_value) {
                o.unknown = true;
                continue;
            }
            *text = argv[++i];
            if (a == "--db") o.have_db = true;
            if (a == "--output") o.have_out = true;
        } else if (a == "--components") {
            long v = 0;
            if (!parse_integer(has_value ? argv[++i] : "", &v) || v < 1 || v > 64) bad("--components");
            else o.components = (int)v, o.have_c = true;
        } else if (a == "--max_iters") {
            long v = 0;
            if (!parse_integer(has_value ? argv[++i] : "", &v) || v < 1 || v > 1000000) bad("--max_iters");
            else o.max_iters = (int)v;
        } else if (a == "--min_norm") {
            if (!parse_number(has_value ? argv[++i] : "", &o.min_norm) || std::isnan(o.min_norm)) bad("--min_norm");
            else o.have_min_norm = true;
        } else if (a == "--tol") {
            if (!parse_number(has_value ? argv[++i] : "", &o.tol) || !(o.tol >= 0.0) || !(o.tol < 1.0)) bad("--tol");
        } else if (a == "--device") {
            if (!parse_device(has_value ? argv[++i] : "", &o.device)) bad("--device");
        } else {
            o.unknown = true;
        }
    }
}

struct Gpu {
    mvs_ctx* ctx = nullptr;
    mvs_sketch_set* set = nullptr;
    mvs_sketch_set* fit = nullptr;
    mvs_sketch_set* other = nullptr;
    mvs_pca* pca = nullptr;
    ~Gpu() {
        if (pca) mvs_pca_destroy(pca);
        if (other) mvs_sketch_set_destroy(other);
        if (fit) mvs_sketch_set_destroy(fit);
        if (set) mvs_sketch_set_destroy(set);
        if (ctx) mvs_ctx_destroy(ctx);
    }
};

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall0 = std::chrono::steady_clock::now();
    Options o;
    parse(argc, argv, o);
    if (o.show_help) {
        print_usage(argv[0]);
        return 0;
    }
    if (!o.bad_flag.empty()) {
        if (o.bad_flag == "--components") std::cerr << kProg << ": --components takes an integer from 1 to 64" << std::endl;
        else if (o.bad_flag == "--max_iters") std::cerr << kProg << ": --max_iters takes an integer of at least 1" << std::endl;
        else if (o.bad_flag == "--min_norm") std::cerr << kProg << ": --min_norm takes a number" << std::endl;
        else if (o.bad_flag == "--tol") std::cerr << kProg << ": --tol takes a number in [0, 1)" << std::endl;
        else std::cerr << kProg << ": --device takes a device index" << std::endl;
        return 1;
    }
    if (o.unknown || !o.have_db || !o.have_out || !o.have_c || o.project.empty() != o.project_output.empty()) {
        print_usage(argv[0]);
        return 1;
    }
    SketchDb sdb, pdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const int64_t n = sdb.n;
    const int d = sdb.dimension, c = o.components;
    if (c > d) {
        std::cerr << kProg << ": --components " << c << " exceeds the DB's dimension " << d << std::endl;
        return 1;
    }
    if (!o.project.empty()) {
        if (const int rc = open_sketch_db(o.project, pdb)) return rc;
        if (pdb.dimension != d) {
            std::cerr << kProg << ": " << o.project << " has dimension " << pdb.dimension << ", " << o.db_folder << " has " << d << std::endl;
            return 1;
        }
    }
    std::vector<char> fitted((size_t)n, 1);
    std::vector<int32_t> rows;
    if (o.have_min_norm) {
        const std::vector<double> norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
        for (int64_t i = 0; i < n; ++i) {
            fitted[(size_t)i] = i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm;
            if (fitted[(size_t)i]) rows.push_back((int32_t)i);
        }
    }
    const int64_t n_fit = o.have_min_norm ? (int64_t)rows.size() : n;
    if (n_fit < 2) {
        std::cerr << kProg << ": " << n_fit << " samples to fit (a PCA needs at least two" << (o.have_min_norm ? "; lower --min_norm" : "") << ")"
                  << std::endl;
        return 1;
    }

    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
    const mvs_sketch_set* fit_set = g.set;
    if (o.have_min_norm && n_fit < n) {
        if (mvs_sketch_set_gather(g.ctx, g.set, rows.data(), MVS_MEM_HOST, n_fit, &g.fit) != MVS_OK) return gpu_fail(kProg, "gathering the fitted samples");
        fit_set = g.fit;
    }
    if (mvs_pca_fit(g.ctx, fit_set, 0, n_fit, c, o.tol, o.max_iters, &g.pca) != MVS_OK) return gpu_fail(kProg, "fitting");
    double gram_ms = 0.0, eigen_ms = 0.0, scores_ms = 0.0, total_variance = 0.0;
    int64_t slabs = 0;
    int iterations = 0, converged = 0;
    mvs_ctx_pca_stats(g.ctx, &gram_ms, &eigen_ms, nullptr, &slabs, nullptr);
    mvs_pca_info(g.pca, nullptr, nullptr, nullptr, &iterations, &converged, &total_variance);
    std::vector<double> mean((size_t)d), axes((size_t)c * d), variances((size_t)c), residuals((size_t)c);
    mvs_pca_get(g.pca, mean.data(), axes.data(), variances.data(), residuals.data());
    if (!converged)
        std::cerr << kProg << ": warning: the fit did not converge to --tol " << fmt9(o.tol) << " in " << iterations << " iterations" << std::endl;

    std::vector<double> scores((size_t)n * c);
    if (mvs_pca_transform(g.ctx, g.pca, g.set, 0, n, scores.data(), MVS_MEM_HOST) != MVS_OK) return gpu_fail(kProg, "computing the scores");
    mvs_ctx_pca_stats(g.ctx, nullptr, nullptr, &scores_ms, nullptr, nullptr);
    if (!o.project.empty()) {
        if (const int rc = load_sketch_db(kProg, g.ctx, pdb, &g.other)) return rc;
        std::vector<double> other((size_t)pdb.n * c);
        if (mvs_pca_transform(g.ctx, g.pca, g.other, 0, pdb.n, other.data(), MVS_MEM_HOST) != MVS_OK)
            return gpu_fail(kProg, "computing the projected scores");
        double ms = 0.0;
        mvs_ctx_pca_stats(g.ctx, nullptr, nullptr, &ms, nullptr, nullptr);
        scores_ms += ms;
        if (const int rc = write_then_rename(kProg, o.project_output, scores_text(pdb.info.names, nullptr, other, c))) return rc;
    }
    if (!o.axes.empty()) {
        std::string text;
        for (int k = 0; k < d; ++k) {
            text += std::to_string(k) + '\t' + fmt9(mean[(size_t)k]);
            for (int j = 0; j < c; ++j) text += '\t' + fmt9(axes[(size_t)j * d + k]);
            text += '\n';
        }
        if (const int rc = write_then_rename(kProg, o.axes, text)) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, scores_text(sdb.info.names, &fitted, scores, c))) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (!o.report.empty()) {
        std::string text = "samples\t" + std::to_string(n) + "\nfitted\t" + std::to_string(n_fit) + "\ndimension\t" + std::to_string(d) +
                           "\ncomponents\t" + std::to_string(c) + "\niterations\t" + std::to_string(iterations) + "\nconverged\t" +
                           std::to_string(converged) + "\ntotal_variance\t" + fmt9(total_variance) + "\ncomponent\tvariance\tratio\tresidual\n";
        for (int j = 0; j < c; ++j)
            text += std::to_string(j + 1) + '\t' + fmt9(variances[(size_t)j]) + '\t' + fmt9(variances[(size_t)j] / total_variance) + '\t' +
                    fmt9(residuals[(size_t)j]) + '\n';
        text += "gram_ms\t" + fmt9(gram_ms) + "\neigen_ms\t" + fmt9(eigen_ms) + "\nscores_ms\t" + fmt9(scores_ms) + "\nslabs\t" + std::to_string(slabs) +
                "\nwall_ms\t" + fmt9(wall_ms) + '\n';
        if (const int rc = write_then_rename(kProg, o.report, text)) return rc;
    }
    std::cout << "Fitted " << c << " components on " << n_fit << " of " << n << " samples in " << iterations << " iterations (gram " << fmt9(gram_ms)
              << " ms, eigen " << fmt9(eigen_ms) << " ms, scores " << fmt9(scores_ms) << " ms)" << std::endl;
    return 0;
}
