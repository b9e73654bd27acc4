// pcoa_sketches -- principal coordinates of a sketch DB on the MI355X in the geometry every other analysis here uses: the
// Jaccard estimate of two samples.  Classical PCoA of the distance sqrt(1 - k), k the clamped estimate above --floor; the
// n x n matrix is never stored (mvs_pcoa_fit, mvs_pcoa_transform, include/mvs_hip.h "principal coordinates").
//
//   pcoa_sketches --db <folder>/ --components <c> --output <coords.tsv> [--min_norm <x>] [--floor <t>]
//                 [--project <folder2>/ --project_output <coords2.tsv>] [--tol <e>] [--max_iters <k>] [--report <r.txt>]
//                 [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).
// --components: 1 .. min(64, fitted samples - 1).  --min_norm x: the fit uses the samples whose norm in vector_norms.txt is at
//   least x; default: every sample.  At least two samples must remain.  --floor t (default 0, in [0, 1)): estimates that do
//   not exceed t count as 0.
// <coords.tsv>, tab-separated, one line per sample of the DB in DB order, those left out of the fit included:
//   name  fitted(1/0)  pc1 ... pcc          %.9g; a fitted sample's coordinates, Gower's out-of-sample scores for the others
// --project / --project_output (both or neither): the out-of-sample scores of another DB of the same dimension, in the format
//   of <coords.tsv> with fitted = 0.  Everything lives in ONE sketch set: the fitted samples first, then those left out, then
//   the other DB's, under a limb code that suits both DBs.
// --tol (default 1e-10, in [0, 1)), --max_iters (default 300, >= 1): the solver's stopping rule; a fit that did not converge
//   warns on stderr and still writes.  --report: samples fitted, iterations, converged, trace, grand mean, the negative Ritz
//   values of the solver's block, per component the eigenvalue, its ratio and its residual, the kernel and wall times.
// Every file is written under <file>.part and renamed when complete.
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "pcoa_sketches";

struct Options {
    std::string db_folder, output, project, project_output, report;
    int components = 0, max_iters = 300, device = -1;
    double min_norm = 0.0, floor = 0.0, tol = 1e-10;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --components <int: 1 to 64> --output <file> [--min_norm <float>] [--floor <float in [0,1)>]"
                 " [--project <folder> --project_output <file>] [--tol <float in [0,1)>] [--max_iters <int >= 1>] [--report <file>]"
                 " [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet loaded, ordered;
    Owned<mvs_pcoa, mvs_pcoa_destroy> pcoa;
};

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall0 = std::chrono::steady_clock::now();
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--project", &o.project),
        path_flag("--project_output", &o.project_output),
        path_flag("--report", &o.report),
        integer_flag("--components", &o.components, 1, 64, "--components takes an integer from 1 to 64", kUsage),
        integer_flag("--max_iters", &o.max_iters, 1, 1000000, "--max_iters takes an integer of at least 1"),
        number_flag("--min_norm", &o.min_norm, not_nan, "--min_norm takes a number"),
        number_flag("--floor", &o.floor, in_half_open_unit, "--floor takes a number in [0, 1)"),
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
    if (!o.project.empty()) {
        if (const int rc = open_sketch_db(o.project, pdb)) return rc;
        if (pdb.dimension != d) {
            std::cerr << kProg << ": " << o.project << " has dimension " << pdb.dimension << ", " << o.db_folder << " has " << d << std::endl;
            return 1;
        }
    }
    const int64_t n_other = o.project.empty() ? 0 : pdb.n, n_all = n + n_other;
    // the order of the one set: the fitted samples, those left out, the other DB's
    std::vector<char> fitted((size_t)n, 1);
    if (have_min_norm) {
        const std::vector<double> norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
        for (int64_t i = 0; i < n; ++i) fitted[(size_t)i] = i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm;
    }
    std::vector<int32_t> order;
    std::vector<int64_t> place((size_t)n);                       // where sample i of the DB sits in the set
    for (int pass = 1; pass >= 0; --pass)
        for (int64_t i = 0; i < n; ++i)
            if (fitted[(size_t)i] == pass) {
                place[(size_t)i] = (int64_t)order.size();
                order.push_back((int32_t)i);
            }
    int64_t n_fit = 0;
    for (int64_t i = 0; i < n; ++i) n_fit += fitted[(size_t)i];
    if (n_fit < 2) {
        std::cerr << kProg << ": " << n_fit << " samples to fit (principal coordinates need at least two" << (have_min_norm ? "; lower --min_norm" : "")
                  << ")" << std::endl;
        return 1;
    }
    if (c > n_fit - 1) {
        std::cerr << kProg << ": --components " << c << " exceeds the fitted samples less one, " << n_fit - 1 << std::endl;
        return 1;
    }
    if (n_all > INT32_MAX) {
        std::cerr << kProg << ": " << n_all << " samples exceed the set's row index" << std::endl;
        return 1;
    }
    for (int64_t j = 0; j < n_other; ++j) order.push_back((int32_t)(n + j));
    std::vector<double> norms_sq((size_t)n_all);
    for (int64_t r = 0; r < n_all; ++r) {
        const int64_t src = order[(size_t)r];
        norms_sq[(size_t)r] = src < n ? sdb.info.norms_sq[(size_t)src] : pdb.info.norms_sq[(size_t)(src - n)];
    }

    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    std::vector<const SketchDb*> dbs{&sdb};
    if (n_other) dbs.push_back(&pdb);
    if (const int rc = load_sketch_dbs(kProg, g.ctx, dbs, &g.loaded)) return rc;
    const mvs_sketch_set* set = g.loaded;
    if (n_fit < n) {                                             // (else the loaded order is the set's order already)
        if (mvs_sketch_set_gather(g.ctx, g.loaded, order.data(), MVS_MEM_HOST, n_all, &g.ordered) != MVS_OK)
            return gpu_fail(kProg, "ordering the samples");
        set = g.ordered;
        g.loaded.reset();
    }
    if (mvs_pcoa_fit(g.ctx, set, norms_sq.data(), MVS_MEM_HOST, 0, n_fit, c, o.floor, o.tol, o.max_iters, &g.pcoa) != MVS_OK)
        return gpu_fail(kProg, "fitting");
    double dots_ms = 0.0, apply_ms = 0.0, eigen_ms = 0.0, grand = 0.0, trace = 0.0;
    int64_t passes = 0, row_blocks = 0, block_rows = 0;
    int iterations = 0, converged = 0, negative = 0;
    mvs_ctx_pcoa_stats(g.ctx, &dots_ms, &apply_ms, &eigen_ms, &passes, &row_blocks, &block_rows);
    mvs_pcoa_info(g.pcoa, nullptr, nullptr, nullptr, nullptr, &iterations, &converged, &negative, nullptr, &grand, &trace);
    std::vector<double> lambda((size_t)c), coords((size_t)n_fit * c), residuals((size_t)c);
    mvs_pcoa_get(g.pcoa, lambda.data(), nullptr, coords.data(), nullptr, residuals.data());
    if (!converged)
        std::cerr << kProg << ": warning: the fit did not converge to --tol " << fmt9(o.tol) << " in " << iterations << " iterations" << std::endl;

    // the samples behind the fitted ones: Gower's scores
    double transform_dots_ms = 0.0, transform_apply_ms = 0.0;
    std::vector<double> rest((size_t)(n_all - n_fit) * c);
    if (n_all > n_fit) {
        if (mvs_pcoa_transform(g.ctx, g.pcoa, set, norms_sq.data(), MVS_MEM_HOST, n_fit, n_all, rest.data(), MVS_MEM_HOST) != MVS_OK)
            return gpu_fail(kProg, "computing the out-of-sample scores");
        mvs_ctx_pcoa_stats(g.ctx, &transform_dots_ms, &transform_apply_ms, nullptr, nullptr, nullptr, nullptr);
    }
    std::vector<double> scores((size_t)n * c);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t at = place[(size_t)i];
        const double* src = at < n_fit ? coords.data() + (size_t)at * c : rest.data() + (size_t)(at - n_fit) * c;
        std::copy(src, src + c, scores.begin() + (size_t)i * c);
    }
    if (n_other) {
        const std::vector<double> other(rest.begin() + (size_t)(n - n_fit) * c, rest.end());
        if (const int rc = write_then_rename(kProg, o.project_output, scores_text(pdb.info.names, nullptr, other, c))) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, scores_text(sdb.info.names, &fitted, scores, c))) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (!o.report.empty()) {
        std::string text = "samples\t" + std::to_string(n) + "\nfitted\t" + std::to_string(n_fit) + "\nprojected\t" + std::to_string(n_other) +
                           "\ndimension\t" + std::to_string(d) + "\ncomponents\t" + std::to_string(c) + "\nfloor\t" + fmt9(o.floor) + "\niterations\t" +
                           std::to_string(iterations) + "\nconverged\t" + std::to_string(converged) + "\ntrace\t" + fmt9(trace) + "\ngrand_mean\t" +
                           fmt9(grand) + "\nnegative_ritz\t" + std::to_string(negative) + "\ncomponent\teigenvalue\tratio\tresidual\n";
        for (int j = 0; j < c; ++j)
            text += std::to_string(j + 1) + '\t' + fmt9(lambda[(size_t)j]) + '\t' + fmt9(lambda[(size_t)j] / trace) + '\t' + fmt9(residuals[(size_t)j]) + '\n';
        text += "dots_ms\t" + fmt9(dots_ms) + "\napply_ms\t" + fmt9(apply_ms) + "\neigen_ms\t" + fmt9(eigen_ms) + "\npasses\t" + std::to_string(passes) +
                "\nrow_blocks\t" + std::to_string(row_blocks) + "\nblock_rows\t" + std::to_string(block_rows) + "\ntransform_dots_ms\t" +
                fmt9(transform_dots_ms) + "\ntransform_apply_ms\t" + fmt9(transform_apply_ms) + "\nwall_ms\t" + fmt9(wall_ms) + '\n';
        if (const int rc = write_then_rename(kProg, o.report, text)) return rc;
    }
    std::cout << "Fitted " << c << " coordinates on " << n_fit << " of " << n << " samples in " << iterations << " iterations (dots " << fmt9(dots_ms)
              << " ms, apply " << fmt9(apply_ms) << " ms, solver " << fmt9(eigen_ms) << " ms)" << std::endl;
    return 0;
}
