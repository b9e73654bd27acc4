// abundance_pairs -- the abundance-weighted measures of pairs of samples, computed from their hash lists and k-mer abundances on
// the MI355X (mvs_abund_overlap_cells, include/mvs_hip.h "abundance-weighted overlaps"): Bray-Curtis, weighted Jaccard (Ruzicka),
// the cosine of the abundance vectors with its angular similarity, abundance-weighted containment.  The reference carries no
// abundances and has no such tool.
//
//   abundance_pairs --hashes <file> --output <pairs.tsv> [--abundances <file>] (--db <folder>/ --min_jaccard <t> | --all_pairs)
//                   [--report <file>] [--device <i>] [--help]
//
// --hashes / --abundances are what `sketch_reads --output / --abundances` wrote: "name: h1 h2 ..." and "name: a1 a2 ...", token i
// of line s of the one belonging to token i of line s of the other (lines without ':' are skipped in both).  With --abundances
// both texts are parsed token by token, in order -- the <file>.csr cache holds every sample sorted and without duplicates, which
// is not the order the abundances are aligned with --, and the set is built by mvs_hash_set_create_counted with the abundances as
// weights: unsorted lists with duplicates are legal and their weights add.  Refused with exit 1 before a device is touched:
// different names or a different order of the samples, a different number of tokens on some line, a hash that is no 64-bit
// decimal number, an abundance outside 1 .. 4294967295.  Without --abundances the hash file is read the way verify_pairs reads
// it (its <file>.csr cache when valid, else the text), the set is plain and every abundance is 1.
// Which pairs: with --db and --min_jaccard t (0 < t < 1) the cells that mvs_search_block keeps on the sketch DB -- the hash
// file's sample names must be the DB's in the DB's order; cells and records stay on the device until the block's download --;
// with --all_pairs every row < col, in blocks of at most 2^20 cells, and no DB is read.  Exactly one of the two.
// The output is tab-separated, written under <pairs.tsv>.part and renamed when complete, one line per pair with row < col in
// ascending (row, col):
//   row_name col_name inter size_row size_col jaccard sum_row sum_col shared_row shared_col
//   w_contain_row w_contain_col bray_curtis ruzicka cosine angular
// inter, sizes, sums (S of a sample) and shared_* (w_row, w_col) are integers; jaccard = inter / (size_row + size_col - inter) in
// fp64 and the six measures of mvs_abund_similarity are written as %.17g, nan for 0/0.  --report writes samples, pairs, the sum
// of inter, the kernel times of the comparison and of the overlaps, and the wall time.
// Exit codes: 1 bad arguments, DB, hash or abundance file, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "abundance_pairs";
constexpr int64_t kBlockCells = 1LL << 20;

struct Options {
    std::string db_folder, hash_file, abund_file, output, report;
    double min_jaccard = 0.0;
    bool all_pairs = false;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --hashes <file> --output <file> [--abundances <file>] (--db <folder> --min_jaccard <float in (0,1)> | --all_pairs)"
                 " [--report <file>] [--device <int>] [--help]\n"
              << "        --hashes / --abundances: 'name: h1 h2 ...' and 'name: a1 a2 ...' as sketch_reads writes them, token for token;\n"
              << "        without --abundances every abundance is 1\n"
              << "        --db with --min_jaccard: the pairs the sketch comparison keeps; --all_pairs: every pair, no DB"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
    OwnedHashSet hs;
    DeviceMem d_out, d_cells, d_norms;
};

struct Pair {
    int32_t row, col;
    mvs_abund_overlap o;
};

// the named lines of a "name: t1 t2 ..." text: names and, per line, where its tokens begin and end
struct TokenText {
    std::string bytes;
    std::vector<std::string> names;
    std::vector<std::pair<size_t, size_t>> body;
};

bool read_token_text(const std::string& path, TokenText& t) {
    if (!read_whole_file(path, t.bytes)) return false;
    const std::string& s = t.bytes;
    for (size_t b = 0; b < s.size();) {
        size_t e = s.find('\n', b);
        if (e == std::string::npos) e = s.size();
        const size_t colon = s.find(':', b);
        if (colon < e) {
            t.names.push_back(s.substr(b, colon - b));
            t.body.push_back({colon + 1, e});
        }
        b = e + 1;
    }
    return true;
}

// the next token of [at, end): false at the end of the line; *value is the token as a decimal number, *ok = it is one below 2^64
bool next_token(const std::string& s, size_t& at, size_t end, uint64_t* value, bool* ok) {
    while (at < end && (s[at] == ' ' || s[at] == '\t' || s[at] == '\r')) ++at;
    if (at >= end) return false;
    uint64_t v = 0;
    *ok = true;
    size_t digits = 0;
    for (; at < end && s[at] != ' ' && s[at] != '\t' && s[at] != '\r'; ++at, ++digits) {
        const unsigned d = (unsigned)(s[at] - '0');
        if (d > 9 || v > (UINT64_MAX - d) / 10) *ok = false;
        else v = v * 10 + d;
    }
    *value = v;
    return true;
}

// first index at which the two lists of names differ (the shorter list's length if one is a prefix), or -1
int64_t first_difference(const std::vector<std::string>& a, const std::vector<std::string>& b) {
    size_t at = 0;
    while (at < a.size() && at < b.size() && a[at] == b[at]) ++at;
    return at == a.size() && at == b.size() ? -1 : (int64_t)at;
}

std::string fmt(double v) {
    if (v != v) return "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

}  // namespace

int main(int argc, char* argv[]) {
    const auto wall_begin = std::chrono::steady_clock::now();
    Options o;
    std::vector<Flag> flags = {
        path_flag("--output", &o.output, kUsage),
        path_flag("--db", &o.db_folder),
        path_flag("--abundances", &o.abund_file),
        path_flag("--report", &o.report),
        text_flag("--hashes", &o.hash_file, "--hashes takes the hash file of the samples", kRefuse),
        number_flag("--min_jaccard", &o.min_jaccard, in_open_unit, "--min_jaccard takes a number in the open range (0,1)"),
        switch_flag("--all_pairs", &o.all_pairs),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags);
    const bool with_db = was_given(flags, "--db"), with_level = was_given(flags, "--min_jaccard");
    if (o.all_pairs && (with_db || with_level)) args.refuse("--all_pairs and --db with --min_jaccard exclude each other: give exactly one of the two");
    else if (!o.all_pairs && !with_db && !with_level) args.refuse("which pairs? give --db with --min_jaccard, or --all_pairs");
    else if (!o.all_pairs && !with_db) args.refuse("--min_jaccard needs the sketch DB: --db takes its folder");
    else if (!o.all_pairs && !with_level) args.refuse("--min_jaccard takes a number in the open range (0,1)");
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;

    SketchDb sdb;
    if (!o.all_pairs)
        if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;

    // the samples: names, and either plain lists (HashSets) or values with weights in the order of the text
    HashSets sets;
    std::vector<std::string> names;
    std::vector<uint64_t> values;
    std::vector<uint32_t> weights;
    std::vector<int64_t> offsets;
    const bool counted = !o.abund_file.empty();
    if (!counted) {
        if (const int rc = load_hash_sets(kProg, o.hash_file, true, sets)) return rc;
        names = sets.names;
    } else {
        TokenText ht, at;
        for (const auto& file : {std::make_pair(&o.hash_file, &ht), std::make_pair(&o.abund_file, &at)})
            if (!read_token_text(*file.first, *file.second)) {
                std::cerr << "Error opening " << *file.first << " for reading." << std::endl;
                return 1;
            }
        if (const int64_t d = first_difference(ht.names, at.names); d >= 0) {
            std::cerr << kProg << ": the samples of " << o.abund_file << " (" << at.names.size() << ") are not those of " << o.hash_file << " ("
                      << ht.names.size() << ") in the same order: first difference at sample " << d << std::endl;
            return 1;
        }
        offsets.push_back(0);
        for (size_t s = 0; s < ht.names.size(); ++s) {
            size_t hp = ht.body[s].first, ap = at.body[s].first;
            uint64_t h = 0, a = 0;
            bool h_ok = true, a_ok = true;
            for (;;) {
                const bool more_h = next_token(ht.bytes, hp, ht.body[s].second, &h, &h_ok);
                const bool more_a = next_token(at.bytes, ap, at.body[s].second, &a, &a_ok);
                if (more_h != more_a) {
                    std::cerr << kProg << ": sample " << s << " (" << ht.names[s] << ") has " << (more_h ? "more" : "fewer") << " hashes in "
                              << o.hash_file << " than abundances in " << o.abund_file << " (after " << (int64_t)values.size() - offsets.back()
                              << " tokens)" << std::endl;
                    return 1;
                }
                if (!more_h) break;
                if (!h_ok) {
                    std::cerr << kProg << ": sample " << s << " (" << ht.names[s] << ") of " << o.hash_file << ": token "
                              << (int64_t)values.size() - offsets.back() << " is no decimal number below 2^64" << std::endl;
                    return 1;
                }
                if (!a_ok || a < 1 || a > 4294967295ULL) {
                    std::cerr << kProg << ": sample " << s << " (" << ht.names[s] << ") of " << o.abund_file << ": token "
                              << (int64_t)values.size() - offsets.back() << " is no abundance from 1 to 4294967295" << std::endl;
                    return 1;
                }
                values.push_back(h);
                weights.push_back((uint32_t)a);
            }
            if ((int64_t)values.size() - offsets.back() >= (1LL << 31)) {
                std::cerr << kProg << ": sample " << s << " (" << ht.names[s] << ") holds 2^31 values or more" << std::endl;
                return 1;
            }
            offsets.push_back((int64_t)values.size());
        }
        names = std::move(ht.names);
    }
    if (!o.all_pairs) {
        const std::vector<std::string>& db_names = sdb.info.names;
        if (const int64_t d = first_difference(names, db_names); d >= 0) {
            std::cerr << kProg << ": the samples of " << o.hash_file << " (" << names.size() << ") are not those of " << sdb.folder
                      << "vector_norms.txt (" << sdb.n << ") in the same order: first difference at sample " << d << std::endl;
            return 1;
        }
    }
    const int64_t n = (int64_t)names.size();
    if (n >= (1LL << 31) - 256) {
        std::cerr << kProg << ": too many samples for 32-bit sample indices" << std::endl;
        return 1;
    }

    std::vector<Pair> pairs;
    std::vector<int32_t> sizes((size_t)n);
    std::vector<uint64_t> sum((size_t)n), sq_lo((size_t)n), sq_hi((size_t)n);
    double compare_ms = 0.0, overlap_ms = 0.0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        mvs_ctx_set_timing(g.ctx, 1);
        const int made = counted ? mvs_hash_set_create_counted(g.ctx, values.data(), MVS_MEM_HOST, weights.data(), MVS_MEM_HOST, offsets.data(), n,
                                                               1, 0, nullptr, &g.hs)
                                 : mvs_hash_set_create(g.ctx, sets.hashes.data(), MVS_MEM_HOST, sets.offsets.data(), n, &g.hs);
        if (made != MVS_OK) return gpu_fail(kProg, "uploading the hash lists");
        if (mvs_hash_set_sizes(g.hs, sizes.data(), MVS_MEM_HOST) != MVS_OK) return gpu_fail(kProg, "reading the set sizes");
        if (mvs_hash_set_abundance_totals(g.hs, sum.data(), sq_lo.data(), sq_hi.data(), MVS_MEM_HOST) != MVS_OK)
            return gpu_fail(kProg, "summing the abundances");
        std::vector<mvs_cell> cells;
        std::vector<mvs_abund_overlap> recs;
        auto add_kernel_time = [&] {
            double kms = 0.0;
            mvs_ctx_intersect_stats(g.ctx, &kms, nullptr, nullptr, nullptr);
            overlap_ms += kms;
        };
        if (o.all_pairs) {
            // every row < col in (row, col) order, a block of cells at a time
            auto flush = [&]() -> int {
                if (cells.empty()) return 0;
                recs.resize(cells.size());
                if (mvs_abund_overlap_cells(g.ctx, g.hs, nullptr, cells.data(), MVS_MEM_HOST, (int64_t)cells.size(), recs.data(), MVS_MEM_HOST) !=
                    MVS_OK)
                    return gpu_fail(kProg, "computing the overlaps");
                add_kernel_time();
                for (size_t i = 0; i < cells.size(); ++i) pairs.push_back({cells[i].row, cells[i].col, recs[i]});
                cells.clear();
                return 0;
            };
            for (int64_t r = 0; r < n; ++r)
                for (int64_t c = r + 1; c < n; ++c) {
                    cells.push_back(mvs_cell{(int32_t)r, (int32_t)c, 0, 0});
                    if ((int64_t)cells.size() == kBlockCells)
                        if (const int rc = flush()) return rc;
                }
            if (const int rc = flush()) return rc;
        } else {
            if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
            if (g.d_norms.alloc(g.ctx, (size_t)n * 8) != MVS_OK ||
                mvs_device_copy(g.ctx, g.d_norms.p, MVS_MEM_DEVICE, sdb.info.norms_sq.data(), MVS_MEM_HOST, (size_t)n * 8) != MVS_OK)
                return gpu_fail(kProg, "uploading the norms");
            auto compare = [&](int64_t rb, int64_t re, mvs_cell* d_cells, int64_t capacity, int64_t* count) {
                const int rc = mvs_search_block(g.ctx, g.set, (const double*)g.d_norms.p, o.min_jaccard, rb, re, 0, n, d_cells, capacity, count);
                float ms = 0.f;
                if (mvs_ctx_kernel_ms(g.ctx, 1, &ms) == MVS_OK) compare_ms += ms;
                return rc;
            };
            auto weigh = [&](const mvs_cell* d_cells, void* d_out, int64_t count) {
                if (mvs_abund_overlap_cells(g.ctx, g.hs, nullptr, d_cells, MVS_MEM_DEVICE, count, (mvs_abund_overlap*)d_out, MVS_MEM_DEVICE) != MVS_OK)
                    return gpu_fail(kProg, "computing the overlaps");
                add_kernel_time();
                cells.resize((size_t)count);
                recs.resize((size_t)count);
                if (mvs_device_copy(g.ctx, cells.data(), MVS_MEM_HOST, d_cells, MVS_MEM_DEVICE, (size_t)count * sizeof(mvs_cell)) != MVS_OK ||
                    mvs_device_copy(g.ctx, recs.data(), MVS_MEM_HOST, d_out, MVS_MEM_DEVICE, (size_t)count * sizeof(mvs_abund_overlap)) != MVS_OK)
                    return gpu_fail(kProg, "downloading");
                for (int64_t i = 0; i < count; ++i)                    // sorted by (row, col) inside a block, blocks ascend
                    if (cells[(size_t)i].row < cells[(size_t)i].col) pairs.push_back({cells[(size_t)i].row, cells[(size_t)i].col, recs[(size_t)i]});
                return 0;
            };
            if (const int rc = for_kept_cell_blocks(kProg, g.ctx, n, sizeof(mvs_abund_overlap), g.d_cells, g.d_out, compare, weigh)) return rc;
        }
    }

    std::string text;
    int64_t inter_sum = 0;
    for (const Pair& p : pairs) {
        const size_t r = (size_t)p.row, c = (size_t)p.col;
        double m[6];
        if (mvs_abund_similarity(&p.o, sum[r], sq_lo[r], sq_hi[r], sizes[r], sum[c], sq_lo[c], sq_hi[c], sizes[c], m) != MVS_OK) {
            std::cerr << kProg << ": pair (" << names[r] << ", " << names[c] << "): " << mvs_last_error() << std::endl;
            return 2;
        }
        const double in = (double)p.o.inter, den = (double)sizes[r] + (double)sizes[c] - in;
        inter_sum += p.o.inter;
        text += names[r] + '\t' + names[c] + '\t' + std::to_string(p.o.inter) + '\t' + std::to_string(sizes[r]) + '\t' + std::to_string(sizes[c]) +
                '\t' + fmt(den == 0.0 ? std::nan("") : in / den) + '\t' + std::to_string(sum[r]) + '\t' + std::to_string(sum[c]) + '\t' +
                std::to_string(p.o.w_row) + '\t' + std::to_string(p.o.w_col);
        for (const double v : m) text += '\t' + fmt(v);
        text += '\n';
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall_begin).count();
    if (!o.report.empty()) {
        std::string rep;
        rep += "samples\t" + std::to_string(n) + "\n";
        rep += "pairs\t" + std::to_string((int64_t)pairs.size()) + "\n";
        rep += "inter_sum\t" + std::to_string(inter_sum) + "\n";
        rep += "compare_kernel_ms\t" + fmt(compare_ms) + "\n";
        rep += "overlap_kernel_ms\t" + fmt(overlap_ms) + "\n";
        rep += "wall_s\t" + fmt(wall_s) + "\n";
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Weighed " << pairs.size() << " pairs of " << n << " samples"
              << (counted ? " by their abundances" : " (no abundances: 1 per value)") << std::endl;
    return 0;
}
