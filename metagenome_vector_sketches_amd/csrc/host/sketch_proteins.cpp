// sketch_proteins -- protein FASTA files (.faa), or with --translate DNA FASTA / FASTQ files read in all six frames, plain or
// gzip -> the hash file every other tool here starts from, hashed on the MI355X (mvs_hash_set_from_residues, include/mvs_hip.h
// "protein sketches").  DNA k-mers see nothing below roughly 80 % identity; these sketches are what relations between families
// show in.  The reference has no such step.
//
//   sketch_proteins --output <hashes.txt> [--alphabet protein|dayhoff|hp] [--translate] [--ksize <k>] [--scaled <s>] [--seed <n>]
//                   [--singleton] [--list <file>] [--batch_bytes <n>] [--report <file>] [--device <i>] [--help] FILE...
//
// Samples, their names, --singleton, --list, --batch_bytes, the output text with its .csr cache and the exit codes are
// sketch_sequences' (mvs_sketch_tool.hpp): every downstream tool reads the output unchanged.  --ksize counts residues; its
// default follows the alphabet (10 / 16 / 42).  The sequence reader judges lines by their place, never by their content, so
// it reads .faa as it is.  --report writes one line per sample (bytes, records, hashed k-mers, values kept, distinct values),
// the alphabet and the input kind, and the stage times.
#include "mvs_host.hpp"
#include "mvs_tool.hpp"
#include "mvs_fasta.hpp"
#include "mvs_sketch_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "sketch_proteins";
constexpr const char* kAlphabets[3] = {"protein", "dayhoff", "hp"};      // indexed by MVS_AA_*
constexpr long kDefaultKsize[3] = {10, 16, 42};

struct Options {
    std::string output, report, list;
    std::vector<std::string> files;
    long ksize = 0, scaled = 200, seed = 42, batch_bytes = 1L << 30;
    int device = -1, alphabet = MVS_AA_PROTEIN;
    bool singleton = false, translate = false;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --output <file> [--alphabet protein|dayhoff|hp] [--translate] [--ksize <int 1..64>] [--scaled <int >= 1>]"
                 " [--seed <int 0..4294967295>] [--singleton] [--list <file>] [--batch_bytes <int >= 1>] [--report <file>] [--device <int>]"
                 " [--help] FILE...\n"
              << "        FILE: protein FASTA, or with --translate DNA FASTA or FASTQ read in all six frames; plain or gzip (by content);"
                 " one sample per file, or per record with --singleton\n"
              << "        --alphabet: default protein; --ksize: residues, default 10 / 16 / 42 for protein / dayhoff / hp\n"
              << "        --scaled: default 200 (a hash is kept iff it is <= 2^64 / scaled); --seed: default 42\n"
              << "        --batch_bytes: bytes per library call; default 1073741824\n"
              << "        --output: 'name: h1 h2 ...' per sample, values ascending (MurmurHash3_x64_128 of the k-mer's residues in the"
                 " alphabet)"
              << std::endl;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--output", &o.output, kUsage),
        path_flag("--report", &o.report),
        switch_flag("--singleton", &o.singleton),
        switch_flag("--translate", &o.translate),
        text_flag("--list", &o.list, "--list takes a file of input paths, one per line"),
        hook_flag("--alphabet",
                  [&o](const std::string& v) {
                      for (int a = 0; a < 3; ++a)
                          if (v == kAlphabets[a]) return o.alphabet = a, true;
                      return false;
                  },
                  "--alphabet takes protein, dayhoff or hp"),
        integer_flag("--ksize", &o.ksize, 1, 64, "--ksize takes an integer from 1 to 64"),
        integer_flag("--scaled", &o.scaled, 1, LONG_MAX, "--scaled takes an integer >= 1"),
        integer_flag("--seed", &o.seed, 0, 4294967295L, "--seed takes an integer from 0 to 4294967295"),
        integer_flag("--batch_bytes", &o.batch_bytes, 1, LONG_MAX, "--batch_bytes takes an integer >= 1"),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags, &o.files);
    if (o.files.empty() && o.list.empty()) args.usage = true;     // nothing to sketch
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    if (o.ksize == 0) o.ksize = kDefaultKsize[o.alphabet];
    if (const int rc = append_list_file(o.list, o.files)) return rc;

    // ---- parse: every file into one buffer; a sample is a run of records ----
    SketchTimes tm;
    SketchInput in;
    const auto t_parse = std::chrono::steady_clock::now();
    if (const int rc = read_sketch_input(kProg, o.files, o.singleton, in)) return rc;
    tm.parse_s = seconds_since(t_parse);
    const int64_t n = (int64_t)in.samples.size();

    // ---- sketch: batches of whole samples ----
    uint64_t max_hash = 0;
    if (mvs_kmer_max_hash(o.scaled, &max_hash) != MVS_OK) return gpu_fail(kProg, "max_hash");
    const int kind = o.translate ? MVS_SEQ_TRANSLATE : MVS_SEQ_PROTEIN;
    if (const int rc = sketch_in_batches(
            kProg, in, o.batch_bytes, o.device,
            [&](mvs_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int64_t m, mvs_hash_set** hs) {
                return mvs_hash_set_from_residues(ctx, bytes, MVS_MEM_HOST, offsets, m, kind, o.alphabet, (int)o.ksize, (uint32_t)o.seed,
                                                  max_hash, hs);
            },
            [](mvs_ctx* ctx, double* ms, int64_t* trips) { return mvs_ctx_aa_stats(ctx, ms, nullptr, nullptr, nullptr, nullptr, trips); },
            mvs_ctx_aa_sample_stats, tm))
        return rc;

    // ---- write: the text, then its parsed form ----
    const auto t_write = std::chrono::steady_clock::now();
    size_t total = 0;
    if (const int rc = write_sketches(kProg, o.output, in.samples, &total)) return rc;
    tm.write_s = seconds_since(t_write);
    if (!o.report.empty()) {
        std::string rep = sketch_report_rows(in.samples, "bytes");
        rep += std::string("# alphabet ") + kAlphabets[o.alphabet] + " input " + (o.translate ? "translate" : "protein") + " ksize " +
               std::to_string(o.ksize) + " scaled " + std::to_string(o.scaled) + " seed " + std::to_string(o.seed) + " max_hash " +
               std::to_string(max_hash) + "\n";
        rep += sketch_report_times(tm);
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Sketched " << n << " samples (" << in.bytes.size() << " bytes) in alphabet " << kAlphabets[o.alphabet]
              << (o.translate ? ", translated in six frames" : "") << ", at ksize " << o.ksize << ", scaled " << o.scaled << ": " << total
              << " hashes written" << std::endl;
    return 0;
}
