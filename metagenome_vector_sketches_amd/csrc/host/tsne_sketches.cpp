// tsne_sketches -- the t-SNE map of a sketch DB's Jaccard kNN graph on the MI355X: exact top-k neighbours, perplexity
// calibration, exact all-pairs gradient (mvs_tsne, include/mvs_hip.h "t-SNE").  No Barnes-Hut, no n x n matrix; the coordinates
// are reproducible bit for bit.
//
//   tsne_sketches --db <folder>/ --output <coords.tsv> [--perplexity <p>] [--neighbours <K>] [--iterations <k>]
//                 [--exaggeration <e>] [--exaggeration_iters <k>] [--learning_rate <x>] [--init pcoa|random] [--seed <s>]
//                 [--min_norm <x>] [--report <r.txt>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).
// --perplexity (default 30, 1 .. K), --neighbours (default ceil(3 x perplexity), 1 .. 256), --iterations (default 750),
//   --exaggeration (default 12) for the first --exaggeration_iters (default 250) iterations, --learning_rate (default
//   max(n / 48, 50)), --init (default pcoa: the two leading principal coordinates, scaled to 1e-4; random: uniform in +-1e-4 from
//   --seed, default 0).  --min_norm x: the map uses the samples whose norm in vector_norms.txt is at least x; default: all.
// <coords.tsv>, tab-separated, one line per sample of the DB in DB order -- the format of pca_sketches and pcoa_sketches:
//   name  fitted(1/0)  pc1  pc2            %.17g (a double read back is the double computed); a sample left out: 0 nan nan
// --report: samples, fitted, neighbours, the graph's stored entries, rows calibrated at beta = 0, the learning rate, the KL
//   divergence, the kernel times by stage and the wall time.
// Every file is written under <file>.part and renamed when complete.
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "tsne_sketches";

struct Options {
    std::string db_folder, output, report;
    double perplexity = 30.0, exaggeration = 12.0, learning_rate = 0.0, min_norm = 0.0;
    long neighbours = 0, iterations = 750, exaggeration_iters = 250, init = MVS_TSNE_INIT_PCOA;
    unsigned long long seed = 0;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --output <file> [--perplexity <float: 1 to 256>] [--neighbours <int: 1 to 256>] [--iterations <int >= 0>]"
                 " [--exaggeration <float > 0>] [--exaggeration_iters <int >= 0>] [--learning_rate <float > 0>] [--init pcoa|random]"
                 " [--seed <int >= 0>] [--min_norm <float>] [--report <file>] [--device <int>] [--help]"
              << std::endl;
}

std::string fmt17(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
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
        path_flag("--output", &o.output, kUsage),
        path_flag("--report", &o.report),
        integer_flag("--iterations", &o.iterations, 0, 1000000, "--iterations takes an integer from 0 to 1000000"),
        integer_flag("--exaggeration_iters", &o.exaggeration_iters, 0, 1000000, "--exaggeration_iters takes an integer from 0 to 1000000"),
        integer_flag("--neighbours", &o.neighbours, 1, 256, "--neighbours takes an integer from 1 to 256"),
        integer_flag("--seed", &o.seed, 0, LONG_MAX, "--seed takes a non-negative integer"),
        number_flag("--perplexity", &o.perplexity, [](double p) { return p >= 1.0 && p <= 256.0; }, "--perplexity takes a number from 1 to 256"),
        number_flag("--exaggeration", &o.exaggeration, positive_finite, "--exaggeration takes a positive number"),
        number_flag("--learning_rate", &o.learning_rate, positive_finite, "--learning_rate takes a positive number"),
        number_flag("--min_norm", &o.min_norm, not_nan, "--min_norm takes a number"),
        word_flag("--init", &o.init, {{"pcoa", MVS_TSNE_INIT_PCOA}, {"random", MVS_TSNE_INIT_RANDOM}}, "--init takes pcoa or random"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    const bool have_min_norm = was_given(flags, "--min_norm");
    const long K = o.neighbours > 0 ? o.neighbours : (long)std::ceil(3.0 * o.perplexity);
    if (K > 256) {
        std::cerr << kProg << ": --perplexity " << fmt9(o.perplexity) << " asks for " << K << " neighbours, top-k holds 256 (give --neighbours)" << std::endl;
        return 1;
    }
    if (o.perplexity > (double)K) {
        std::cerr << kProg << ": --perplexity " << fmt9(o.perplexity) << " exceeds --neighbours " << K << std::endl;
        return 1;
    }
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const int64_t n = sdb.n;
    std::vector<char> fitted((size_t)n, 1);
    if (have_min_norm) {
        const std::vector<double> norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
        for (int64_t i = 0; i < n; ++i) fitted[(size_t)i] = i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm;
    }
    std::vector<int32_t> order;
    for (int64_t i = 0; i < n; ++i)
        if (fitted[(size_t)i]) order.push_back((int32_t)i);
    const int64_t n_fit = (int64_t)order.size();
    const int64_t need = o.init == MVS_TSNE_INIT_PCOA ? 3 : 1;
    if (n_fit < need) {
        std::cerr << kProg << ": " << n_fit << " samples to map (--init " << (o.init == MVS_TSNE_INIT_PCOA ? "pcoa" : "random") << " needs at least " << need
                  << (have_min_norm ? "; lower --min_norm" : "") << ")" << std::endl;
        return 1;
    }
    if (n_fit > (1LL << 21)) {
        std::cerr << kProg << ": " << n_fit << " samples exceed the 2^21 an exact map holds" << std::endl;
        return 1;
    }
    std::vector<double> norms_sq((size_t)n_fit);
    for (int64_t r = 0; r < n_fit; ++r) norms_sq[(size_t)r] = sdb.info.norms_sq[(size_t)order[(size_t)r]];

    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.loaded)) return rc;
    const mvs_sketch_set* set = g.loaded;
    if (n_fit < n) {
        if (mvs_sketch_set_gather(g.ctx, g.loaded, order.data(), MVS_MEM_HOST, n_fit, &g.kept) != MVS_OK) return gpu_fail(kProg, "selecting the samples");
        set = g.kept;
        g.loaded.reset();
    }
    mvs_tsne_params p;
    p.perplexity = o.perplexity;
    p.exaggeration = o.exaggeration;
    p.learning_rate = o.learning_rate;
    p.neighbours = o.neighbours;
    p.iterations = o.iterations;
    p.exaggeration_iters = o.exaggeration_iters;
    p.init = o.init;
    p.seed = o.seed;
    mvs_tsne_result res;
    std::vector<double> Y((size_t)n_fit * 2);
    if (mvs_tsne(g.ctx, set, norms_sq.data(), MVS_MEM_HOST, &p, Y.data(), nullptr, nullptr, &res, nullptr) != MVS_OK) return gpu_fail(kProg, "mapping");
    double topk_ms = 0.0, calibrate_ms = 0.0, graph_ms = 0.0, repulse_ms = 0.0, attract_ms = 0.0, update_ms = 0.0;
    int64_t iterations = 0, entries = 0, units = 0, row_blocks = 0;
    mvs_ctx_tsne_stats(g.ctx, &topk_ms, &calibrate_ms, &graph_ms, &repulse_ms, &attract_ms, &update_ms, &iterations, &entries, &units, &row_blocks);

    std::string text;
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        text += sdb.info.names[(size_t)i];
        if (fitted[(size_t)i]) {
            text += "\t1\t" + fmt17(Y[(size_t)at * 2]) + '\t' + fmt17(Y[(size_t)at * 2 + 1]) + '\n';
            ++at;
        } else {
            text += "\t0\tnan\tnan\n";
        }
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (!o.report.empty()) {
        const std::string report =
            "samples\t" + std::to_string(n) + "\nfitted\t" + std::to_string(n_fit) + "\ndimension\t" + std::to_string(sdb.dimension) + "\nperplexity\t" +
            fmt9(o.perplexity) + "\nneighbours\t" + std::to_string(res.neighbours) + "\nentries\t" + std::to_string(res.entries) + "\nbeta_zero_rows\t" +
            std::to_string(res.beta_zero_rows) + "\niterations\t" + std::to_string(res.iterations) + "\nlearning_rate\t" + fmt17(res.learning_rate) +
            "\nkl\t" + fmt9(res.kl) + "\ntopk_ms\t" + fmt9(topk_ms) + "\ncalibrate_ms\t" + fmt9(calibrate_ms) + "\ngraph_ms\t" + fmt9(graph_ms) +
            "\nrepulse_ms\t" + fmt9(repulse_ms) + "\nattract_ms\t" + fmt9(attract_ms) + "\nupdate_ms\t" + fmt9(update_ms) + "\nunits\t" +
            std::to_string(units) + "\nrow_blocks\t" + std::to_string(row_blocks) + "\nwall_ms\t" + fmt9(wall_ms) + '\n';
        if (const int rc = write_then_rename(kProg, o.report, report)) return rc;
    }
    std::cout << "Mapped " << n_fit << " of " << n << " samples: " << res.neighbours << " neighbours, " << res.entries << " entries, " << res.iterations
              << " iterations, KL " << fmt9(res.kl) << " (repulsion " << fmt9(repulse_ms) << " ms, attraction " << fmt9(attract_ms) << " ms)" << std::endl;
    return 0;
}
