// gather_sketches -- which samples of a hash file make up each query, and how much of the query each explains that the ones
// before it did not: the greedy minimum-set-cover walk (the rule of sourmash `gather`) on the exact hash lists, on the MI355X
// (mvs_gather, include/mvs_hip.h "gather").  The reference has no such tool: its search (src/jaccard.py) ranks pairs, and ten
// strains that all contain the same third of a query are reported ten times there.
//
//   gather_sketches --hashes <file> --query <file> --output <gather.tsv> [--min_hashes <k>] [--max_matches <r>]
//                   [--report <file>] [--device <i>] [--help]
//
// --hashes is read the way `project_everything sketch` and verify_pairs read a hash file (its <file>.csr cache when valid, else
// the text); --query holds one "name: hashes" record per line, the format of the search.  All queries go into one hash set, one
// mvs_gather per query against every sample of --hashes.  The walk stops at the first sample that would add fewer than
// --min_hashes hashes (default 50: sourmash's 50 kbp threshold at scaled = 1000) or after --max_matches records (default: no
// bound).  The output is tab-separated with a header line, written under <gather.tsv>.part and renamed when complete, one line
// per match in the order the walk found them (a query without matches writes no line):
//   query  rank  match  intersect  unique  f_orig_query  f_match  f_unique_to_query  remaining
// rank counts from 0; intersect = |Q n H|, unique = the hashes this match added, remaining = the query's hashes still
// unexplained after it; f_orig_query = intersect / |Q|, f_match = intersect / |H|, f_unique_to_query = unique / |Q|, fp64 as
// %.9g.  --report writes one line per query: its size, matches, the hashes explained and their fraction, the survivors of the
// first phase, the rounds, and the kernel times of the three phases.
// Exit codes: 1 bad arguments or files, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "gather_sketches";

struct Options {
    std::string hash_file, query_file, output, report;
    long min_hashes = 50, max_matches = -1;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --hashes <file> --query <file> --output <file> [--min_hashes <int >= 1>] [--max_matches <int >= 0>]"
                 " [--report <file>] [--device <int>] [--help]\n"
              << "        --min_hashes: a match must add at least this many of the query's hashes; default 50"
                 " (sourmash gather's 50 kbp threshold at scaled = 1000)"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedHashSet hs_db, hs_q;
};

std::string ratio9(double num, double den) { return den == 0.0 ? "nan" : fmt9(num / den); }

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {                                   // absent: --hashes speaks before --query
        path_flag("--output", &o.output, kUsage),
        path_flag("--report", &o.report),
        text_flag("--hashes", &o.hash_file, "--hashes takes the hash file of the samples to gather from", kRefuse),
        text_flag("--query", &o.query_file, "--query takes a file of 'name: hashes' lines", kRefuse),
        integer_flag("--min_hashes", &o.min_hashes, 1, 0x7fffffffL, "--min_hashes takes an integer >= 1"),
        integer_flag("--max_matches", &o.max_matches, 0, 0x7fffffffL, "--max_matches takes an integer >= 0"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    HashSets db, queries;
    if (const int rc = load_hash_sets(kProg, o.hash_file, true, db)) return rc;
    if (const int rc = load_hash_sets(kProg, o.query_file, false, queries)) return rc;
    const int64_t n = (int64_t)db.names.size(), nq = (int64_t)queries.names.size();

    std::string text = "query\trank\tmatch\tintersect\tunique\tf_orig_query\tf_match\tf_unique_to_query\tremaining\n";
    std::string rep = "query\tsize\tmatches\texplained\tf_explained\tsurvivors\trounds\toverlap_ms\tmark_ms\trounds_ms\n";
    int64_t written = 0;
    if (nq > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        mvs_ctx_set_timing(g.ctx, 1);
        if (mvs_hash_set_create(g.ctx, db.hashes.data(), MVS_MEM_HOST, db.offsets.data(), n, &g.hs_db) != MVS_OK ||
            mvs_hash_set_create(g.ctx, queries.hashes.data(), MVS_MEM_HOST, queries.offsets.data(), nq, &g.hs_q) != MVS_OK)
            return gpu_fail(kProg, "uploading the hash lists");
        std::vector<int32_t> sizes((size_t)n);
        if (mvs_hash_set_sizes(g.hs_db, sizes.data(), MVS_MEM_HOST) != MVS_OK) return gpu_fail(kProg, "reading the set sizes");
        const int64_t room = o.max_matches < 0 ? n : std::min<int64_t>(o.max_matches, n);
        std::vector<mvs_gather_match> matches((size_t)std::max<int64_t>(room, 1));
        for (int64_t q = 0; q < nq; ++q) {
            int64_t count = 0;
            int32_t q_size = 0;
            if (mvs_gather(g.ctx, g.hs_q, q, g.hs_db, nullptr, MVS_MEM_HOST, 0, (int32_t)o.min_hashes, room, matches.data(), MVS_MEM_HOST,
                           &count, &q_size) != MVS_OK)
                return gpu_fail(kProg, "gathering");
            int64_t explained = 0;
            for (int64_t r = 0; r < count; ++r) {
                const mvs_gather_match& m = matches[(size_t)r];
                explained += m.unique;
                text += queries.names[(size_t)q] + '\t' + std::to_string(r) + '\t' + db.names[(size_t)m.sample] + '\t' +
                        std::to_string(m.intersect) + '\t' + std::to_string(m.unique) + '\t' + ratio9(m.intersect, q_size) + '\t' +
                        ratio9(m.intersect, sizes[(size_t)m.sample]) + '\t' + ratio9(m.unique, q_size) + '\t' +
                        std::to_string(m.remaining) + '\n';
            }
            written += count;
            int64_t survivors = 0, rounds = 0;
            double overlap_ms = 0.0, mark_ms = 0.0, rounds_ms = 0.0;
            mvs_ctx_gather_stats(g.ctx, &survivors, &rounds, nullptr, nullptr, &overlap_ms, &mark_ms, &rounds_ms);
            rep += queries.names[(size_t)q] + '\t' + std::to_string(q_size) + '\t' + std::to_string(count) + '\t' +
                   std::to_string(explained) + '\t' + ratio9((double)explained, q_size) + '\t' + std::to_string(survivors) + '\t' +
                   std::to_string(rounds) + '\t' + fmt9(overlap_ms) + '\t' + fmt9(mark_ms) + '\t' + fmt9(rounds_ms) + '\n';
        }
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    if (!o.report.empty())
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    std::cout << "Gathered " << nq << " queries from " << n << " samples at min_hashes " << o.min_hashes << ": " << written
              << " matches written" << std::endl;
    return 0;
}
