// sketch_reads -- read sets (FASTA / FASTQ, plain or gzip, of any size) -> the hash file every other tool here starts from,
// with k-mer abundances and a minimum count, hashed and counted on the MI355X (mvs_kmer_sketcher_*, include/mvs_hip.h
// "abundances").  The reference has no such step.
//
//   sketch_reads --output <hashes.txt> [--abundances <file>] [--min_abundance <int >= 1>] [--max_abundance <int >= 0>] [--ksize <k>]
//                [--scaled <s>] [--seed <n>] [--list <file>] [--window_bytes <n>] [--histogram <file>] [--report <file>]
//                [--device <i>] [--help] FILE...
//
// One sample per FILE, named by the file name up to its first '.' (the rule of sketch_sequences).  --list names a file with one
// sample per line, "name<TAB>path[<TAB>path...]": a sample made of several files (read pairs, lanes).  Sample names must differ
// and must not contain ':': both are checked before the device is touched.  The files stream through SeqStream (mvs_reads.hpp):
// one mvs_kmer_sketcher_add per window of --window_bytes text, every record a piece, so host memory is bounded by the window and
// the longest record, not by the file.  A value is written iff its abundance in the sample is >= --min_abundance (default 1) and,
// with --max_abundance > 0, <= that.
// --output and its .csr cache are in the format of sketch_sequences ("name: h1 h2 ...", ascending; "name:" for an empty
// sample), written under <file>.part and renamed; with --min_abundance 1 the two tools write byte-identical files for the same
// inputs.  --abundances: "name: a1 a2 ...", token i of line s belonging to token i of line s of the output.  --histogram:
// "name<TAB>abundance<TAB>distinct_values" for the non-zero bins, counted before the filter; 255 means 255 or more.  --report:
// per sample bases, records, valid k-mers, values kept, distinct values, values that passed; then the stage times.
// Exit codes: 1 bad arguments or files, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"
#include "mvs_reads.hpp"

#include <unordered_set>

using namespace mvs_host;

namespace {

constexpr const char* kProg = "sketch_reads";

struct Options {
    std::string output, abundances, histogram, report, list;
    std::vector<std::string> files;
    long ksize = 31, scaled = 1000, seed = 42, window_bytes = 268435456L, min_abundance = 1, max_abundance = 0;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --output <file> [--abundances <file>] [--min_abundance <int >= 1>] [--max_abundance <int >= 0>]"
                 " [--ksize <int 1..32>] [--scaled <int >= 1>] [--seed <int 0..4294967295>] [--list <file>]"
                 " [--window_bytes <int >= 1>] [--histogram <file>] [--report <file>] [--device <int>] [--help] FILE...\n"
              << "        FILE: FASTA or FASTQ, plain or gzip (by content), of any size; one sample per file\n"
              << "        --list: one sample per line, name<TAB>path[<TAB>path...] (pairs, lanes)\n"
              << "        --min_abundance: default 1; --max_abundance: default 0 = no cap; a value is kept iff its count in the sample"
                 " passes both\n"
              << "        --ksize: default 31; --scaled: default 1000 (a hash is kept iff it is <= 2^64 / scaled); --seed: default 42\n"
              << "        --window_bytes: text read per library call; default 268435456\n"
              << "        --output: 'name: h1 h2 ...' per sample, values ascending; --abundances: 'name: a1 a2 ...' aligned with it\n"
              << "        --histogram: name<TAB>abundance<TAB>distinct values, before the filter; 255 = 255 or more"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedHashSet hs;
    Owned<mvs_kmer_sketcher, mvs_kmer_sketcher_destroy> sk;
};

struct Sample {
    std::string name;
    std::vector<std::string> files;
    int64_t records = 0, bases = 0;
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--output", &o.output, kUsage),
        path_flag("--abundances", &o.abundances),
        path_flag("--histogram", &o.histogram),
        path_flag("--report", &o.report),
        text_flag("--list", &o.list, "--list takes a file of samples, one per line: name<TAB>path[<TAB>path...]"),
        integer_flag("--min_abundance", &o.min_abundance, 1, 4294967295L, "--min_abundance takes an integer from 1 to 4294967295"),
        integer_flag("--max_abundance", &o.max_abundance, 0, 4294967295L, "--max_abundance takes an integer from 0 to 4294967295"),
        integer_flag("--ksize", &o.ksize, 1, 32, "--ksize takes an integer from 1 to 32"),
        integer_flag("--scaled", &o.scaled, 1, LONG_MAX, "--scaled takes an integer >= 1"),
        integer_flag("--seed", &o.seed, 0, 4294967295L, "--seed takes an integer from 0 to 4294967295"),
        integer_flag("--window_bytes", &o.window_bytes, 1, LONG_MAX, "--window_bytes takes an integer >= 1"),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags, &o.files);
    if (o.max_abundance > 0 && o.max_abundance < o.min_abundance) args.refuse("--max_abundance is below --min_abundance");
    if (o.files.empty() && o.list.empty()) args.usage = true;     // nothing to sketch
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;

    std::vector<Sample> samples;
    for (const std::string& f : o.files) {
        const std::string file_name = fs::path(f).filename().string();
        samples.push_back({file_name.substr(0, file_name.find('.')), {f}, 0});
    }
    if (!o.list.empty()) {
        std::ifstream in(o.list);
        if (!in) {
            std::cerr << "Error opening " << o.list << " for reading." << std::endl;
            return 1;
        }
        std::string line;
        size_t line_no = 0;
        while (std::getline(in, line)) {
            ++line_no;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty()) continue;
            Sample s;
            size_t at = line.find('\t');
            s.name = line.substr(0, at);
            while (at != std::string::npos) {
                const size_t next = line.find('\t', at + 1);
                const std::string path = line.substr(at + 1, next == std::string::npos ? std::string::npos : next - at - 1);
                if (!path.empty()) s.files.push_back(path);
                at = next;
            }
            if (s.files.empty()) {
                std::cerr << kProg << ": " << o.list << ": line " << line_no << ": the sample '" << s.name << "' has no path (name<TAB>path[<TAB>path...])"
                          << std::endl;
                return 1;
            }
            samples.push_back(std::move(s));
        }
    }
    std::unordered_set<std::string> seen;
    for (const Sample& s : samples) {
        if (s.name.find_first_of(":\n") != std::string::npos) {
            std::cerr << kProg << ": the sample name '" << s.name << "' (" << s.files[0] << ") contains ':'" << std::endl;
            return 1;
        }
        if (!seen.insert(s.name).second) {
            std::cerr << kProg << ": duplicate sample name '" << s.name << "' (" << s.files[0] << ")" << std::endl;
            return 1;
        }
    }
    const int64_t n = (int64_t)samples.size();

    uint64_t max_hash = 0;
    if (mvs_kmer_max_hash(o.scaled, &max_hash) != MVS_OK) return gpu_fail(kProg, "max_hash");
    Gpu g;
    if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
    mvs_ctx_set_timing(g.ctx, 1);
    if (mvs_kmer_sketcher_create(g.ctx, n, (int)o.ksize, (uint32_t)o.seed, max_hash, &g.sk) != MVS_OK) return gpu_fail(kProg, "creating the sketcher");

    // ---- stream: one add per window, every record a piece ----
    double parse_s = 0.0, add_s = 0.0;
    int64_t windows = 0, text_lines = 0;
    {
        std::string bases, err;
        std::vector<SeqRecord> recs;
        std::vector<int64_t> offsets;
        std::vector<int32_t> owner;
        for (int64_t s = 0; s < n; ++s)
            for (const std::string& f : samples[(size_t)s].files) {
                SeqStream in;
                auto t0 = std::chrono::steady_clock::now();
                bool ok = in.open(f, (size_t)o.window_bytes, err);
                while (ok && !in.done()) {
                    ok = in.next(bases, recs, err);
                    parse_s += seconds_since(t0);
                    if (!ok || recs.empty()) break;
                    // the pieces: every record with the '\n' behind it -- a break, which ends every k-mer as a piece's end does
                    offsets.clear();
                    owner.assign(recs.size(), (int32_t)s);
                    for (const SeqRecord& r : recs) {
                        offsets.push_back((int64_t)r.begin);
                        samples[(size_t)s].bases += (int64_t)(r.end - r.begin);
                    }
                    offsets.push_back((int64_t)bases.size());
                    samples[(size_t)s].records += (int64_t)recs.size();
                    t0 = std::chrono::steady_clock::now();
                    if (mvs_kmer_sketcher_add(g.sk, (const uint8_t*)bases.data(), MVS_MEM_HOST, offsets.data(), owner.data(), (int64_t)recs.size()) !=
                        MVS_OK)
                        return gpu_fail(kProg, "sketching");
                    add_s += seconds_since(t0);
                    ++windows;
                    t0 = std::chrono::steady_clock::now();
                }
                if (!ok) {
                    std::cerr << (err.compare(0, 14, "Error opening ") == 0 ? err : std::string(kProg) + ": " + err) << std::endl;
                    return 1;
                }
                text_lines += (int64_t)in.lines();
            }
    }
    double hash_ms = 0.0;
    int64_t second_trips = 0;

    // ---- finish: count, filter ----
    const auto t_finish = std::chrono::steady_clock::now();
    std::vector<int64_t> hist(o.histogram.empty() ? 0 : (size_t)std::max<int64_t>(n, 1) * 256);
    if (mvs_kmer_sketcher_finish(g.sk, (uint32_t)o.min_abundance, (uint32_t)o.max_abundance, o.histogram.empty() ? nullptr : hist.data(), &g.hs) !=
        MVS_OK)
        return gpu_fail(kProg, "counting");
    const double finish_s = seconds_since(t_finish);
    double sort_ms = 0.0, count_ms = 0.0;
    mvs_ctx_abund_stats(g.ctx, &sort_ms, &count_ms, nullptr, nullptr, nullptr, nullptr, nullptr);
    int64_t growths = 0;
    mvs_kmer_sketcher_info(g.sk, &hash_ms, nullptr, nullptr, nullptr, &second_trips, &growths);
    std::vector<int64_t> st_kmers((size_t)n), st_kept((size_t)n), st_distinct((size_t)n), st_passed((size_t)n), off((size_t)n + 1);
    int64_t total = 0;
    if (mvs_kmer_sketcher_stats(g.sk, nullptr, st_kmers.data(), st_kept.data(), st_distinct.data(), st_passed.data()) != MVS_OK ||
        mvs_hash_set_info(g.hs, nullptr, &total, nullptr) != MVS_OK)
        return gpu_fail(kProg, "reading the statistics");
    std::vector<uint64_t> flat((size_t)std::max<int64_t>(total, 1));
    std::vector<uint32_t> abund((size_t)std::max<int64_t>(total, 1));
    if (mvs_hash_set_export(g.hs, flat.data(), MVS_MEM_HOST, off.data()) != MVS_OK ||
        mvs_hash_set_abundances(g.hs, abund.data(), MVS_MEM_HOST) != MVS_OK)
        return gpu_fail(kProg, "reading the hashes");

    // ---- write: the text, its parsed form, the side files ----
    const auto t_write = std::chrono::steady_clock::now();
    std::string text, atext;
    for (int64_t s = 0; s < n; ++s) {
        text += samples[(size_t)s].name + ":";
        atext += samples[(size_t)s].name + ":";
        for (int64_t i = off[(size_t)s]; i < off[(size_t)s + 1]; ++i) {
            text += ' ';
            text += std::to_string(flat[(size_t)i]);
            if (!o.abundances.empty()) {
                atext += ' ';
                atext += std::to_string(abund[(size_t)i]);
            }
        }
        text += '\n';
        atext += '\n';
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    if (!getenv("MVS_NO_CSR_CACHE")) {
        HashSets sets;
        if (sets.hashes.reset((size_t)total)) {
            sets.offsets.assign(off.begin(), off.end());
            for (const Sample& s : samples) sets.names.push_back(s.name);
            if (total > 0) memcpy(sets.hashes.data(), flat.data(), (size_t)total * 8);
            (void)write_csr_cache(o.output, sets);
        }
    }
    if (!o.abundances.empty())
        if (const int rc = write_then_rename(kProg, o.abundances, atext)) return rc;
    if (!o.histogram.empty()) {
        std::string h;
        for (int64_t s = 0; s < n; ++s)
            for (int b = 1; b < 256; ++b)
                if (hist[(size_t)s * 256 + (size_t)b])
                    h += samples[(size_t)s].name + '\t' + std::to_string(b) + '\t' + std::to_string(hist[(size_t)s * 256 + (size_t)b]) + '\n';
        if (const int rc = write_then_rename(kProg, o.histogram, h)) return rc;
    }
    const double write_s = seconds_since(t_write);
    int64_t all_bases = 0;
    for (const Sample& s : samples) all_bases += s.bases;
    if (!o.report.empty()) {
        std::string rep = "sample\tbases\trecords\tkmers\tkept\tdistinct\tpassed\n";
        for (int64_t s = 0; s < n; ++s)
            rep += samples[(size_t)s].name + '\t' + std::to_string(samples[(size_t)s].bases) + '\t' + std::to_string(samples[(size_t)s].records) + '\t' +
                   std::to_string(st_kmers[(size_t)s]) + '\t' + std::to_string(st_kept[(size_t)s]) + '\t' + std::to_string(st_distinct[(size_t)s]) +
                   '\t' + std::to_string(st_passed[(size_t)s]) + '\n';
        rep += "# ksize " + std::to_string(o.ksize) + " scaled " + std::to_string(o.scaled) + " seed " + std::to_string(o.seed) + " max_hash " +
               std::to_string(max_hash) + " min_abundance " + std::to_string(o.min_abundance) + " max_abundance " + std::to_string(o.max_abundance) + "\n";
        rep += "# windows " + std::to_string(windows) + " window_bytes " + std::to_string(o.window_bytes) + " lines " + std::to_string(text_lines) +
               " second_trips " + std::to_string(second_trips) + " growths " + std::to_string(growths) + "\n";
        rep += "# parse_s " + fmt9(parse_s) + " add_s " + fmt9(add_s) + " hash_ms " + fmt9(hash_ms) + " finish_s " + fmt9(finish_s) + " sort_ms " +
               fmt9(sort_ms) + " count_ms " + fmt9(count_ms) + " write_s " + fmt9(write_s) + "\n";
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Sketched " << n << " samples (" << all_bases << " bases in " << windows << " windows) at ksize " << o.ksize << ", scaled " << o.scaled
              << ", min abundance " << o.min_abundance << ": " << total << " hashes written" << std::endl;
    return 0;
}
