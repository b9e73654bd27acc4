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
    std::string db_folder, output, axes, project, project_output, report;
    int components = 0, max_iters = 300, device = -1;
    double min_norm = 0.0, tol = 1e-10;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --components <int: 1 to 64> --output <file> [--min_norm <float>] [--axes <file>]"
                 " [--project <folder> --project_output <file>] [--tol <float in [0,1)>] [--max_iters <int >= 1>] [--report <file>]"
                 " [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set, fit, other;
    Owned<mvs_pca, mvs_pca_destroy> pca;
};

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall0 = std::chrono::steady_clock::now();
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--axes", &o.axes),
        path_flag("--project", &o.project),
        path_flag("--project_output", &o.project_output),
        path_flag("--report", &o.report),
        integer_flag("--components", &o.components, 1, 64, "--components takes an integer from 1 to 64", kUsage),
        integer_flag("--max_iters", &o.max_iters, 1, 1000000, "--max_iters takes an integer of at least 1"),
        number_flag("--min_norm", &o.min_norm, not_nan, "--min_norm takes a number"),
        number_flag("--tol", &o.tol, in_half_open_unit, "--tol takes a number in [0, 1)"),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags);
    if (o.project.empty() != o.project_output.empty()) args.usage = true;    // both or neither
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    const bool have_min_norm = was_given(flags, "--min_norm");
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
    if (have_min_norm) {
        const std::vector<double> norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
        for (int64_t i = 0; i < n; ++i) {
            fitted[(size_t)i] = i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm;
            if (fitted[(size_t)i]) rows.push_back((int32_t)i);
        }
    }
    const int64_t n_fit = have_min_norm ? (int64_t)rows.size() : n;
    if (n_fit < 2) {
        std::cerr << kProg << ": " << n_fit << " samples to fit (a PCA needs at least two" << (have_min_norm ? "; lower --min_norm" : "") << ")"
                  << std::endl;
        return 1;
    }

    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
    const mvs_sketch_set* fit_set = g.set;
    if (have_min_norm && n_fit < n) {
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
