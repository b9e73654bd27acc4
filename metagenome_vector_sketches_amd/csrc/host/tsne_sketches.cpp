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
    std::string db_folder, output, report, bad_flag;
    double perplexity = 30.0, exaggeration = 12.0, learning_rate = 0.0, min_norm = 0.0;
    long neighbours = 0, iterations = 750, exaggeration_iters = 250, init = MVS_TSNE_INIT_PCOA;
    unsigned long long seed = 0;
    int device = -1;
    bool show_help = false, have_db = false, have_out = false, have_min_norm = false, unknown = false;
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

// bad_flag: the first flag whose value is missing, unparsable or out of range (reported before anything is touched)
void parse(int argc, char* argv[], Options& o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_value = i + 1 < argc;
        auto bad = [&](const char* flag) {
            if (o.bad_flag.empty()) o.bad_flag = flag;
        };
        std::string* text = a == "--db" ? &o.db_folder : a == "--output" ? &o.output : a == "--report" ? &o.report : nullptr;
        long* count = a == "--iterations" ? &o.iterations : a == "--exaggeration_iters" ? &o.exaggeration_iters : nullptr;
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
        } else if (count) {
            long v = 0;
            if (!parse_integer(has_value ? argv[++i] : "", &v) || v < 0 || v > 1000000) bad(a == "--iterations" ? "--iterations" : "--exaggeration_iters");
            else *count = v;
        } else if (a == "--neighbours") {
            long v = 0;
            if (!parse_integer(has_value ? argv[++i] : "", &v) || v < 1 || v > 256) bad("--neighbours");
            else o.neighbours = v;
        } else if (a == "--seed") {
            long v = 0;
            if (!parse_integer(has_value ? argv[++i] : "", &v) || v < 0) bad("--seed");
            else o.seed = (unsigned long long)v;
        } else if (a == "--perplexity") {
            if (!parse_number(has_value ? argv[++i] : "", &o.perplexity) || !(o.perplexity >= 1.0) || !(o.perplexity <= 256.0)) bad("--perplexity");
        } else if (a == "--exaggeration") {
            if (!parse_number(has_value ? argv[++i] : "", &o.exaggeration) || !(o.exaggeration > 0.0) || std::isinf(o.exaggeration)) bad("--exaggeration");
        } else if (a == "--learning_rate") {
            if (!parse_number(has_value ? argv[++i] : "", &o.learning_rate) || !(o.learning_rate > 0.0) || std::isinf(o.learning_rate))
                bad("--learning_rate");
        } else if (a == "--min_norm") {
            if (!parse_number(has_value ? argv[++i] : "", &o.min_norm) || std::isnan(o.min_norm)) bad("--min_norm");
            else o.have_min_norm = true;
        } else if (a == "--init") {
            const std::string v = has_value ? argv[++i] : "";
            if (v == "pcoa") o.init = MVS_TSNE_INIT_PCOA;
            else if (v == "random") o.init = MVS_TSNE_INIT_RANDOM;
            else bad("--init");
        } else if (a == "--device") {
            if (!parse_device(has_value ? argv[++i] : "", &o.device)) bad("--device");
        } else {
            o.unknown = true;
        }
    }
}

struct Gpu {
    mvs_ctx* ctx = nullptr;
    mvs_sketch_set* loaded = nullptr;
    mvs_sketch_set* kept = nullptr;
    ~Gpu() {
        if (kept) mvs_sketch_set_destroy(kept);
        if (loaded) mvs_sketch_set_destroy(loaded);
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
        if (o.bad_flag == "--perplexity") std::cerr << kProg << ": --perplexity takes a number from 1 to 256" << std::endl;
        else if (o.bad_flag == "--neighbours") std::cerr << kProg << ": --neighbours takes an integer from 1 to 256" << std::endl;
        else if (o.bad_flag == "--iterations" || o.bad_flag == "--exaggeration_iters")
            std::cerr << kProg << ": " << o.bad_flag << " takes an integer from 0 to 1000000" << std::endl;
        else if (o.bad_flag == "--exaggeration" || o.bad_flag == "--learning_rate")
            std::cerr << kProg << ": " << o.bad_flag << " takes a positive number" << std::endl;
        else if (o.bad_flag == "--seed") std::cerr << kProg << ": --seed takes a non-negative integer" << std::endl;
        else if (o.bad_flag == "--min_norm") std::cerr << kProg << ": --min_norm takes a number" << std::endl;
        else if (o.bad_flag == "--init") std::cerr << kProg << ": --init takes pcoa or random" << std::endl;
        else std::cerr << kProg << ": --device takes a device index" << std::endl;
        return 1;
    }
    if (o.unknown || !o.have_db || !o.have_out) {
        print_usage(argv[0]);
        return 1;
    }
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
    if (o.have_min_norm) {
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
                  << (o.have_min_norm ? "; lower --min_norm" : "") << ")" << std::endl;
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
        mvs_sketch_set_destroy(g.loaded);
        g.loaded = nullptr;
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
