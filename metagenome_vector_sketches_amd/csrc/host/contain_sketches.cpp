// contain_sketches -- the pairs of a sketch DB in which one sample is (estimated to be) CONTAINED in the other, on the MI355X:
// "which samples contain this one".  Every other tool keeps a pair by its Jaccard estimate, which the size ratio of the two
// samples bounds; this one keeps it by the containment rule of mvs_pairwise_contain (include/mvs_hip.h) and can verify the kept
// pairs on the hash lists the DB was sketched from (mvs_intersect_cells).  The reference has no such tool.
//
//   contain_sketches --db <folder>/ --min_containment <c> --output <pairs.tsv> [--mode row|max] [--slack <z>]
//                    [--hashes <file> [--exact_min <u>]] [--report <file>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).  A cell
// (row, col), row != col, is kept when the containment estimate (dot / d) / n2[row] exceeds c (0 < c < 1) by more than z
// standard errors (z = --slack, default 0; negative z widens the list: candidates for --hashes).  The output is tab-separated,
// written under <pairs.tsv>.part and renamed when complete, one line per kept cell in ascending (row, col):
//   contained  container  est_containment  z_score  est_jaccard  dot
// est_containment = inter / n2[row], inter = dot / d; z_score = (inter - c * n2[row]) * sqrt(d) / sqrt(n2[row] * n2[col]);
// est_jaccard = inter / (n2[row] + n2[col] - inter); fp64 in that order, floats as %.9g.  --mode max keeps a pair that passes in
// either direction and writes ONE line per unordered pair: the contained sample is the one with the smaller norm (equal norms:
// the smaller index), the line's figures are those of that direction.
// --hashes FILE (the hash file the DB was sketched from, read as verify_pairs reads it): each block's cells go to
// mvs_intersect_cells while they are on the device and the line gains
//   inter  size_contained  size_container  exact_containment
// (exact_containment = inter / size_contained, 0 / 0 printed as nan); only lines with exact_containment > --exact_min are
// written (default: c).  --report writes counts (cells kept, pairs, pairs above the exact cut, pairs written), the RMSE of the
// containment estimate against the exact value, and kernel and wall times.
// Exit codes: 1 bad arguments, DB or hash file, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "contain_sketches";

struct Options {
    std::string db_folder, hash_file, output, report;
    double min_containment = 0.0, slack = 0.0, exact_min = -1.0;
    int device = -1, mode = MVS_CONTAIN_ROW;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --min_containment <float in (0,1)> --output <file> [--mode row|max] [--slack <float>]"
                 " [--hashes <file> [--exact_min <float in [0,1)>]] [--report <file>] [--device <int>] [--help]"
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
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--report", &o.report),
        text_flag("--hashes", &o.hash_file, "--hashes takes the hash file the DB was sketched from"),
        number_flag("--min_containment", &o.min_containment, in_open_unit, "--min_containment takes a number in the open range (0,1)", kRefuse),
        number_flag("--slack", &o.slack, [](double z) { return std::isfinite(z); }, "--slack takes a finite number"),
        word_flag("--mode", &o.mode, {{"row", MVS_CONTAIN_ROW}, {"max", MVS_CONTAIN_MAX}}, "--mode takes row or max"),
        number_flag("--exact_min", &o.exact_min, in_half_open_unit, "--exact_min takes a number in the range [0,1)"),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags);
    const bool have_hashes = was_given(flags, "--hashes");
    if (o.exact_min >= 0.0 && !have_hashes) args.refuse("--exact_min needs --hashes");
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;
    const double dd = (double)sdb.dimension;
    const double c = o.min_containment;
    const double exact_min = o.exact_min >= 0.0 ? o.exact_min : c;

    HashSets sets;
    if (have_hashes)
        if (const int rc = load_db_hashes(kProg, o.hash_file, sdb, sets)) return rc;

    std::vector<Pair> pairs;
    std::vector<int32_t> sizes((size_t)n);
    double dots_ms = 0.0, select_ms = 0.0, intersect_ms = 0.0;
    int64_t cells_kept = 0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        mvs_ctx_set_timing(g.ctx, 1);
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        if (have_hashes) {
            if (mvs_hash_set_create(g.ctx, sets.hashes.data(), MVS_MEM_HOST, sets.offsets.data(), n, &g.hs) != MVS_OK)
                return gpu_fail(kProg, "uploading the hash lists");
            if (mvs_hash_set_sizes(g.hs, sizes.data(), MVS_MEM_HOST) != MVS_OK) return gpu_fail(kProg, "reading the set sizes");
        }
        if (g.d_norms.alloc(g.ctx, (size_t)n * 8) != MVS_OK ||
            mvs_device_copy(g.ctx, g.d_norms.p, MVS_MEM_DEVICE, db.norms_sq.data(), MVS_MEM_HOST, (size_t)n * 8) != MVS_OK)
            return gpu_fail(kProg, "uploading the norms");
        std::vector<mvs_cell> cells;
        std::vector<int32_t> inter;
        auto compare = [&](int64_t rb, int64_t re, mvs_cell* d_cells, int64_t capacity, int64_t* count) {
            const int rc = mvs_pairwise_contain(g.ctx, g.set, (const double*)g.d_norms.p, MVS_MEM_DEVICE, c, o.slack, o.mode, rb, re, 0, n, d_cells,
                                                MVS_MEM_DEVICE, capacity, count);
            double dms = 0.0, sms = 0.0;
            if (mvs_ctx_contain_stats(g.ctx, &dms, &sms, nullptr, nullptr) == MVS_OK) {
                dots_ms += dms;
                select_ms += sms;
            }
            return rc;
        };
        auto keep = [&](const mvs_cell* d_cells, void* d_inter, int64_t count) {
            cells_kept += count;
            cells.resize((size_t)count);
            inter.assign((size_t)count, 0);
            if (have_hashes) {
                if (mvs_intersect_cells(g.ctx, g.hs, nullptr, d_cells, MVS_MEM_DEVICE, count, (int32_t*)d_inter, MVS_MEM_DEVICE) != MVS_OK)
                    return gpu_fail(kProg, "intersecting");
                double kms = 0.0;
                mvs_ctx_intersect_stats(g.ctx, &kms, nullptr, nullptr, nullptr);
                intersect_ms += kms;
                if (mvs_device_copy(g.ctx, inter.data(), MVS_MEM_HOST, d_inter, MVS_MEM_DEVICE, (size_t)count * 4) != MVS_OK)
                    return gpu_fail(kProg, "downloading");
            }
            if (mvs_device_copy(g.ctx, cells.data(), MVS_MEM_HOST, d_cells, MVS_MEM_DEVICE, (size_t)count * sizeof(mvs_cell)) != MVS_OK)
                return gpu_fail(kProg, "downloading");
            for (int64_t i = 0; i < count; ++i) {                       // sorted by (row, col) inside a block, blocks ascend
                const mvs_cell& x = cells[(size_t)i];
                if (o.mode == MVS_CONTAIN_MAX) {                        // one line per unordered pair: from the smaller norm's side
                    const double a = db.norms_sq[(size_t)x.row], b = db.norms_sq[(size_t)x.col];
                    if (!(a < b || (a == b && x.row < x.col))) continue;
                }
                pairs.push_back({x.row, x.col, x.dot, inter[(size_t)i]});
            }
            return 0;
        };
        if (const int rc = for_kept_cell_blocks(kProg, g.ctx, n, 4, g.d_cells, g.d_inter, compare, keep)) return rc;
    }

    std::string text;
    int64_t above = 0, written = 0, err_n = 0;
    double err_sq = 0.0;
    for (const Pair& p : pairs) {
        const double n2r = db.norms_sq[(size_t)p.row], n2c = db.norms_sq[(size_t)p.col];
        const double inter_est = (double)p.dot / dd;
        const double est = inter_est / n2r;
        const double t = c * n2r;
        const double e = inter_est - t;
        const double z = e * std::sqrt(dd) / std::sqrt(n2r * n2c);
        const double jac = inter_est / (n2r + n2c - inter_est);
        std::string line = db.names[(size_t)p.row] + '\t' + db.names[(size_t)p.col] + '\t' + fmt(est) + '\t' + fmt(z) + '\t' + fmt(jac) +
                           '\t' + std::to_string(p.dot);
        if (have_hashes) {
            const double sa = (double)sizes[(size_t)p.row], in = (double)p.inter;
            const double exact = ratio(in, sa);
            if (exact == exact && est == est && std::isfinite(est)) {
                const double d = est - exact;
                err_sq += d * d;
                ++err_n;
            }
            if (!(exact > exact_min)) continue;
            ++above;
            line += '\t' + std::to_string(p.inter) + '\t' + std::to_string(sizes[(size_t)p.row]) + '\t' +
                    std::to_string(sizes[(size_t)p.col]) + '\t' + fmt(exact);
        }
        text += line + '\n';
        ++written;
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall_begin).count();
    const char* mode_name = o.mode == MVS_CONTAIN_MAX ? "max" : "row";
    if (!o.report.empty()) {
        std::string rep;
        rep += "samples\t" + std::to_string(n) + "\n";
        rep += "min_containment\t" + fmt(c) + "\n";
        rep += "slack\t" + fmt(o.slack) + "\n";
        rep += std::string("mode\t") + mode_name + "\n";
        rep += "cells_kept\t" + std::to_string(cells_kept) + "\n";
        rep += "pairs\t" + std::to_string((int64_t)pairs.size()) + "\n";
        if (have_hashes) {
            rep += "exact_min\t" + fmt(exact_min) + "\n";
            rep += "pairs_exact_above\t" + std::to_string(above) + "\n";
            rep += "estimate_rmse\t" + fmt(err_n ? std::sqrt(err_sq / (double)err_n) : 0.0) + "\n";
        }
        rep += "pairs_written\t" + std::to_string(written) + "\n";
        rep += "dots_kernel_ms\t" + fmt(dots_ms) + "\n";
        rep += "select_kernel_ms\t" + fmt(select_ms) + "\n";
        if (have_hashes) rep += "intersect_kernel_ms\t" + fmt(intersect_ms) + "\n";
        rep += "wall_s\t" + fmt(wall_s) + "\n";
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Kept " << cells_kept << " cells of " << n << " samples at containment > " << c << " (mode " << mode_name << ", slack "
              << o.slack << "): " << pairs.size() << " pairs";
    if (have_hashes) std::cout << ", " << above << " with exact containment > " << exact_min;
    std::cout << "; " << written << " written" << std::endl;
    return 0;
}
