// permanova_sketches -- do labelled groups of samples of a sketch DB differ?  PERMANOVA (Anderson 2001) on the MI355X in the
// geometry every other analysis here uses: the distance sqrt(1 - k), k the clamped Jaccard estimate above --floor.  The n x n
// matrix is never stored and the relabellings are summed in the same pass as the observed labelling (mvs_permanova,
// include/mvs_hip.h "PERMANOVA").
//
//   permanova_sketches --db <folder>/ --groups <file> --output <result.tsv> [--permutations <p>] [--seed <s>] [--floor <t>]
//                      [--min_norm <x>] [--perm_output <perms.tsv>] [--report <r.txt>] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does (dimension.txt, dtype.txt, vector_norms.txt :893-901, vectors.bin).
// --groups: one line per sample, name<TAB>group (empty lines are skipped; a line without a tab or a name given twice is an
//   error).  A sample takes part if the file names it and, with --min_norm x, its norm in vector_norms.txt is at least x.
//   The others are left out and counted in the report, as are the file's names the DB does not have.  Group ids are given in
//   order of first appearance walking the DB's taking-part samples.  At most 255 groups; at least 2; fewer groups than samples.
// --permutations (default 999, 0 .. 16382), --seed (default 0): the relabellings (mvs_permutation_labels).  --floor t (default
//   0, in [0, 1)): estimates that do not exceed t count as 0.
// <result.tsv>, tab-separated, doubles as %.17g:
//   samples groups permutations ss_total ss_within ss_between df_between df_within pseudo_F R2 p_value      (header)
//   one line of values
//   group size mean_within_d2                                                                                (header)
//   one line per group, in id order, the group's name first
// --perm_output: the pseudo-F of every relabelling, one %.17g per line.  --report: the counts above, seed, floor, kernel and
//   wall times.  Every file is written under <file>.part and renamed when complete.
// Exit codes: 1 bad arguments, DB or groups file, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

#include <unordered_map>
#include <unordered_set>

using namespace mvs_host;

namespace {

constexpr const char* kProg = "permanova_sketches";

struct Options {
    std::string db_folder, groups, output, perm_output, report;
    long permutations = 999;
    unsigned long long seed = 0;
    int device = -1;
    double min_norm = 0.0, floor = 0.0;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --db <folder> --groups <file: name<TAB>group per line> --output <file> [--permutations <int: 0 to 16382>] [--seed <int>]"
                 " [--floor <float in [0,1)>] [--min_norm <float>] [--perm_output <file>] [--report <file>] [--device <int>] [--help]"
              << std::endl;
}

inline std::string fmt17(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// --seed: the whole string is a decimal integer below 2^64 without a sign
bool parse_seed(const std::string& v, unsigned long long* out) {
    char* end = nullptr;
    errno = 0;
    *out = strtoull(v.c_str(), &end, 10);
    return !(v.empty() || v[0] == '-' || end == v.c_str() || *end || errno);
}

// name -> group of the --groups file; 0, or 1 after a message
int read_groups(const std::string& file, std::unordered_map<std::string, std::string>& group_of) {
    std::ifstream in(file);
    if (!in) {
        std::cerr << kProg << ": cannot read " << file << std::endl;
        return 1;
    }
    std::string line;
    for (int64_t no = 1; std::getline(in, line); ++no) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 == line.size()) {
            std::cerr << kProg << ": " << file << " line " << no << ": expected name<TAB>group" << std::endl;
            return 1;
        }
        if (!group_of.emplace(line.substr(0, tab), line.substr(tab + 1)).second) {
            std::cerr << kProg << ": " << file << " line " << no << ": " << line.substr(0, tab) << " appears twice" << std::endl;
            return 1;
        }
    }
    return 0;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet loaded, labelled;
};

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall0 = std::chrono::steady_clock::now();
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--groups", &o.groups, kUsage),
        path_flag("--output", &o.output, kUsage),
        path_flag("--perm_output", &o.perm_output),
        path_flag("--report", &o.report),
        integer_flag("--permutations", &o.permutations, 0, MVS_MAX_GROUP_SLOTS - 2,
                     "--permutations takes an integer from 0 to " + std::to_string(MVS_MAX_GROUP_SLOTS - 2)),
        hook_flag("--seed", [&o](const std::string& v) { return parse_seed(v, &o.seed); }, "--seed takes a non-negative integer below 2^64"),
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
    std::unordered_map<std::string, std::string> group_of;
    if (const int rc = read_groups(o.groups, group_of)) return rc;

    // who takes part, and the group ids in order of first appearance
    std::vector<double> norms;
    if (have_min_norm) norms = read_plain_norms(o.db_folder + "vector_norms.txt", n);
    std::vector<int32_t> order;
    std::vector<uint8_t> labels;
    std::vector<std::string> group_names;
    std::unordered_map<std::string, int> id_of;
    std::unordered_set<std::string> seen;                       // the file's names the DB has
    int64_t unlabelled = 0, below_norm = 0;
    for (int64_t i = 0; i < n; ++i) {
        const auto it = group_of.find(sdb.info.names[(size_t)i]);
        if (it == group_of.end()) {
            ++unlabelled;
            continue;
        }
        seen.insert(it->first);
        if (have_min_norm && !(i < (int64_t)norms.size() && norms[(size_t)i] >= o.min_norm)) {
            ++below_norm;
            continue;
        }
        const auto ins = id_of.emplace(it->second, (int)group_names.size());
        if (ins.second) {
            if (group_names.size() == 255) {
                std::cerr << kProg << ": more than 255 groups" << std::endl;
                return 1;
            }
            group_names.push_back(it->second);
        }
        order.push_back((int32_t)i);
        labels.push_back((uint8_t)ins.first->second);
    }
    const int64_t unknown_names = (int64_t)(group_of.size() - seen.size());
    const int64_t m = (int64_t)order.size(), G = (int64_t)group_names.size();
    if (G < 2) {
        std::cerr << kProg << ": " << G << " groups among the " << m << " samples that take part (PERMANOVA needs at least two"
                  << (have_min_norm ? "; lower --min_norm" : "") << ")" << std::endl;
        return 1;
    }
    if (G >= m) {
        std::cerr << kProg << ": " << G << " groups of " << m << " samples (PERMANOVA needs fewer groups than samples)" << std::endl;
        return 1;
    }
    std::vector<double> norms_sq((size_t)m);
    for (int64_t r = 0; r < m; ++r) norms_sq[(size_t)r] = sdb.info.norms_sq[(size_t)order[(size_t)r]];

    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.loaded)) return rc;
    const mvs_sketch_set* set = g.loaded;
    if (m < n) {                                                 // (else the loaded set is the labelled set already)
        if (mvs_sketch_set_gather(g.ctx, g.loaded, order.data(), MVS_MEM_HOST, m, &g.labelled) != MVS_OK)
            return gpu_fail(kProg, "gathering the labelled samples");
        set = g.labelled;
        g.loaded.reset();
    }
    mvs_permanova_result res{};
    std::vector<int64_t> sizes((size_t)G);
    std::vector<double> mean_d2((size_t)G), perm_f((size_t)o.permutations);
    if (mvs_permanova(g.ctx, set, norms_sq.data(), MVS_MEM_HOST, o.floor, 0, m, labels.data(), (int)G, o.permutations, o.seed, &res, sizes.data(),
                      mean_d2.data(), perm_f.data()) != MVS_OK)
        return gpu_fail(kProg, "computing the sums");
    double dots_ms = 0.0, quantise_ms = 0.0, sums_ms = 0.0;
    int64_t row_blocks = 0, block_rows = 0, slots = 0;
    mvs_ctx_groups_stats(g.ctx, &dots_ms, &quantise_ms, &sums_ms, &row_blocks, &block_rows, &slots);

    std::string text = "samples\tgroups\tpermutations\tss_total\tss_within\tss_between\tdf_between\tdf_within\tpseudo_F\tR2\tp_value\n";
    text += std::to_string(res.samples) + '\t' + std::to_string(res.groups) + '\t' + std::to_string(res.permutations) + '\t' + fmt17(res.ss_total) + '\t' +
            fmt17(res.ss_within) + '\t' + fmt17(res.ss_between) + '\t' + std::to_string(res.df_between) + '\t' + std::to_string(res.df_within) + '\t' +
            fmt17(res.f) + '\t' + fmt17(res.r2) + '\t' + fmt17(res.p_value) + '\n';
    text += "group\tsize\tmean_within_d2\n";
    for (int64_t k = 0; k < G; ++k) text += group_names[(size_t)k] + '\t' + std::to_string(sizes[(size_t)k]) + '\t' + fmt17(mean_d2[(size_t)k]) + '\n';
    if (!o.perm_output.empty()) {
        std::string perms;
        for (const double f : perm_f) perms += fmt17(f) + '\n';
        if (const int rc = write_then_rename(kProg, o.perm_output, perms)) return rc;
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (!o.report.empty()) {
        const std::string rep = "samples\t" + std::to_string(n) + "\nlabelled\t" + std::to_string(m) + "\nexcluded_unlabelled\t" + std::to_string(unlabelled) +
                                "\nexcluded_min_norm\t" + std::to_string(below_norm) + "\nunknown_names\t" + std::to_string(unknown_names) + "\ndimension\t" +
                                std::to_string(sdb.dimension) + "\ngroups\t" + std::to_string(G) + "\npermutations\t" + std::to_string(o.permutations) +
                                "\nseed\t" + std::to_string(o.seed) + "\nfloor\t" + fmt9(o.floor) + "\nslots\t" + std::to_string(slots) + "\ndots_ms\t" +
                                fmt9(dots_ms) + "\nquantise_ms\t" + fmt9(quantise_ms) + "\nsums_ms\t" + fmt9(sums_ms) + "\nrow_blocks\t" +
                                std::to_string(row_blocks) + "\nblock_rows\t" + std::to_string(block_rows) + "\nwall_ms\t" + fmt9(wall_ms) + '\n';
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "PERMANOVA of " << G << " groups on " << m << " of " << n << " samples: pseudo-F " << fmt9(res.f) << ", R2 " << fmt9(res.r2) << ", p "
              << fmt9(res.p_value) << " from " << o.permutations << " permutations (dots " << fmt9(dots_ms) << " ms, quantise " << fmt9(quantise_ms)
              << " ms, sums " << fmt9(sums_ms) << " ms)" << std::endl;
    return 0;
}
