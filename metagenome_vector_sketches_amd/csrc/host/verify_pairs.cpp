// verify_pairs -- the pairs of a sketch DB whose Jaccard ESTIMATE exceeds a level, each with its EXACT Jaccard and containments
// computed from the hash lists the DB was sketched from, on the MI355X: filter on sketches, verify on sets.  The reference has
// no such tool: it measures its estimator offline on simulated vectors (src/compute_error_of_random_projections.py); here the
// kept cells of the comparison stay on the device and go straight into mvs_intersect_cells.
//
//   verify_pairs --db <folder>/ --hashes <file> --min_jaccard <t> --output <pairs.tsv> [--exact_min <u>] [--report <file>]
//                [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin) and the
// hash file the way `project_everything sketch` does (its <file>.csr cache when valid, else the text).  The hash file's sample
// names must be the DB's names in the DB's order.  Pairs are kept by the rule of mvs_search_block: Jaccard estimate
// (:661-662) > t, 0 < t < 1.  The output is tab-separated, written under <pairs.tsv>.part and renamed when complete, one line
// per kept pair with row < col in ascending (row, col):
//   row_name  col_name  est_jaccard  exact_jaccard  inter  size_row  size_col  contain_row  contain_col
// est_jaccard is the unclamped fp64 estimate (inter_est = dot / d; inter_est / (n2r + n2c - inter_est)); exact_jaccard =
// inter / (size_row + size_col - inter), contain_row = inter / size_row, contain_col = inter / size_col, all fp64 in that
// order, 0/0 printed as nan; floats as %.9g.  --exact_min u (0 <= u < 1) drops the lines whose exact Jaccard is <= u: the
// verified edge list.  --report writes counts (pairs kept by the estimate, pairs with exact J > t, pairs with exact J <= t),
// the RMSE and the largest absolute error of the estimate over the kept pairs, and kernel and wall times.
// Exit codes: 1 bad arguments, DB or hash file, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "verify_pairs";

struct Options {
    std::string db_folder, hash_file, output, report;
    double min_jaccard = 0.0, exact_min = -1.0;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --hashes <file> --min_jaccard <float in (0,1)> --output <file> [--exact_min <float in [0,1)>]"
                 " [--report <file>] [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
    OwnedHashSet hs;
    DeviceMem d_inter, d_cells, d_norms;
};

struct Pair {
    int32_t row, col, dot, inter;
};

std::string fmt(double v) {
    if (v != v) return "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%.9g", v);
    return buf;
}

double ratio(double num, double den) { return den == 0.0 ? std::nan("") : num / den; }

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall_begin = std::chrono::steady_clock::now();
    Options o;
    std::vector<Flag> flags = {                                   // absent: --min_jaccard speaks before --hashes
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--report", &o.report),
        number_flag("--min_jaccard", &o.min_jaccard, in_open_unit, "--min_jaccard takes a number in the open range (0,1)", kRefuse),
        text_flag("--hashes", &o.hash_file, "--hashes takes the hash file the DB was sketched from", kRefuse),
        number_flag("--exact_min", &o.exact_min, in_half_open_unit, "--exact_min takes a number in the range [0,1)"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;
    const int dimension = sdb.dimension;

    HashSets sets;
    if (const int rc = load_db_hashes(kProg, o.hash_file, sdb, sets)) return rc;

    std::vector<Pair> pairs;
    std::vector<int32_t> sizes((size_t)n);
    double compare_ms = 0.0, intersect_ms = 0.0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        mvs_ctx_set_timing(g.ctx, 1);
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (mvs_hash_set_create(g.ctx, sets.hashes.data(), MVS_MEM_HOST, sets.offsets.data(), n, &g.hs) != MVS_OK)
            return gpu_fail(kProg, "uploading the hash lists");
        if (mvs_hash_set_sizes(g.hs, sizes.data(), MVS_MEM_HOST) != MVS_OK) return gpu_fail(kProg, "reading the set sizes");
        if (g.d_norms.alloc(g.ctx, (size_t)n * 8) != MVS_OK ||
            mvs_device_copy(g.ctx, g.d_norms.p, MVS_MEM_DEVICE, db.norms_sq.data(), MVS_MEM_HOST, (size_t)n * 8) != MVS_OK)
            return gpu_fail(kProg, "uploading the norms");
        std::vector<mvs_cell> cells;
        std::vector<int32_t> inter;
        auto compare = [&](int64_t rb, int64_t re, mvs_cell* d_cells, int64_t capacity, int64_t* count) {
            const int rc = mvs_search_block(g.ctx, g.set, (const double*)g.d_norms.p, o.min_jaccard, rb, re, 0, n, d_cells, capacity, count);
            float ms = 0.f;
            if (mvs_ctx_kernel_ms(g.ctx, 1, &ms) == MVS_OK) compare_ms += ms;
            return rc;
        };
        auto verify = [&](const mvs_cell* d_cells, void* d_inter, int64_t count) {
            if (mvs_intersect_cells(g.ctx, g.hs, nullptr, d_cells, MVS_MEM_DEVICE, count, (int32_t*)d_inter, MVS_MEM_DEVICE) != MVS_OK)
                return gpu_fail(kProg, "intersecting");
            double kms = 0.0;
            mvs_ctx_intersect_stats(g.ctx, &kms, nullptr, nullptr, nullptr);
            intersect_ms += kms;
            cells.resize((size_t)count);
            inter.resize((size_t)count);
            if (mvs_device_copy(g.ctx, cells.data(), MVS_MEM_HOST, d_cells, MVS_MEM_DEVICE, (size_t)count * sizeof(mvs_cell)) != MVS_OK ||
                mvs_device_copy(g.ctx, inter.data(), MVS_MEM_HOST, d_inter, MVS_MEM_DEVICE, (size_t)count * 4) != MVS_OK)
                return gpu_fail(kProg, "downloading");
            for (int64_t i = 0; i < count; ++i)                        // sorted by (row, col) inside a block, blocks ascend
                if (cells[(size_t)i].row < cells[(size_t)i].col)
                    pairs.push_back({cells[(size_t)i].row, cells[(size_t)i].col, cells[(size_t)i].dot, inter[(size_t)i]});
            return 0;
        };
        if (const int rc = for_kept_cell_blocks(kProg, g.ctx, n, 4, g.d_cells, g.d_inter, compare, verify)) return rc;
    }

    std::string text;
    int64_t above = 0, below = 0, written = 0;
    double err_sq = 0.0, err_max = 0.0;
    int64_t err_n = 0;
    for (const Pair& p : pairs) {
        const double n2r = db.norms_sq[(size_t)p.row], n2c = db.norms_sq[(size_t)p.col];
        const double inter_est = (double)p.dot / (double)dimension;
        const double est = inter_est / (n2r + n2c - inter_est);
        const double sa = (double)sizes[(size_t)p.row], sb = (double)sizes[(size_t)p.col], in = (double)p.inter;
        const double exact = ratio(in, sa + sb - in);
        if (exact > o.min_jaccard) ++above;
        else ++below;
        if (exact == exact && est == est) {
            const double e = std::fabs(est - exact);
            err_sq += e * e;
            err_max = std::max(err_max, e);
            ++err_n;
        }
        if (o.exact_min >= 0.0 && exact <= o.exact_min) continue;
        text += db.names[(size_t)p.row] + '\t' + db.names[(size_t)p.col] + '\t' + fmt(est) + '\t' + fmt(exact) + '\t' + std::to_string(p.inter) +
                '\t' + std::to_string(sizes[(size_t)p.row]) + '\t' + std::to_string(sizes[(size_t)p.col]) + '\t' + fmt(ratio(in, sa)) + '\t' +
                fmt(ratio(in, sb)) + '\n';
        ++written;
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall_begin).count();
    if (!o.report.empty()) {
        std::string rep;
        rep += "samples\t" + std::to_string(n) + "\n";
        rep += "min_jaccard\t" + fmt(o.min_jaccard) + "\n";
        rep += "pairs_kept_by_estimate\t" + std::to_string((int64_t)pairs.size()) + "\n";
        rep += "pairs_exact_above\t" + std::to_string(above) + "\n";
        rep += "false_positives\t" + std::to_string(below) + "\n";
        rep += "pairs_written\t" + std::to_string(written) + "\n";
        rep += "estimate_rmse\t" + fmt(err_n ? std::sqrt(err_sq / (double)err_n) : 0.0) + "\n";
        rep += "estimate_max_abs_error\t" + fmt(err_max) + "\n";
        rep += "compare_kernel_ms\t" + fmt(compare_ms) + "\n";
        rep += "intersect_kernel_ms\t" + fmt(intersect_ms) + "\n";
        rep += "wall_s\t" + fmt(wall_s) + "\n";
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Verified " << pairs.size() << " pairs of " << n << " samples kept at Jaccard > " << o.min_jaccard << ": " << above
              << " above exactly, " << below << " at or below; " << written << " written" << std::endl;
    return 0;
}
