// sketch_sequences -- FASTA / FASTQ files (plain or gzip) -> the hash file every other tool here starts from, hashed on the
// MI355X (mvs_hash_set_from_sequences, include/mvs_hip.h "sketches from sequences").  The reference has no such step: its hash
// lists come from sourmash signatures computed elsewhere (`project_everything convert` unpacks them).
//
//   sketch_sequences --output <hashes.txt> [--ksize <k>] [--scaled <s>] [--seed <n>] [--singleton] [--list <file>]
//                    [--batch_bytes <n>] [--report <file>] [--device <i>] [--help] FILE...
//
// One sample per input file, named by the file name up to its first '.' (the rule of `convert`); with --singleton one sample per
// record, named by the record (its header up to the first white space).  --list names a file with one more input path per line.
// The records of a sample are joined with one '\n', so no k-mer spans two records.  Samples are handed to the library in batches
// of up to --batch_bytes bases (a larger sample is a batch of its own).  The output is "name: h1 h2 ..." with the values
// ascending, one line per sample in input order, written under <hashes.txt>.part and renamed when complete; its parsed form goes
// to <hashes.txt>.csr, which `project_everything sketch`, verify_pairs and gather_sketches map instead of parsing the text.  A
// sample without a value is written as "name:", which every reader takes as an empty sample.  Sample names must differ and must
// not contain ':' (the text format ends the name there): both are checked before the device is touched.
// --report writes one line per sample (bases, records, valid k-mers, values kept, distinct values) and the stage times.
// Exit codes: 1 bad arguments or files, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"
#include "mvs_tool.hpp"
#include "mvs_fasta.hpp"
#include "mvs_sketch_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "sketch_sequences";

struct Options {
    std::string output, report, list;
    std::vector<std::string> files;
    long ksize = 31, scaled = 1000, seed = 42, batch_bytes = 1L << 30;
    int device = -1;
    bool singleton = false;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0
              << " --output <file> [--ksize <int 1..32>] [--scaled <int >= 1>] [--seed <int 0..4294967295>] [--singleton]"
                 " [--list <file>] [--batch_bytes <int >= 1>] [--report <file>] [--device <int>] [--help] FILE...\n"
              << "        FILE: FASTA or FASTQ, plain or gzip (by content); one sample per file, or per record with --singleton\n"
              << "        --ksize: default 31; --scaled: default 1000 (a hash is kept iff it is <= 2^64 / scaled); --seed: default 42\n"
              << "        --batch_bytes: bases per library call; default 1073741824\n"
              << "        --output: 'name: h1 h2 ...' per sample, values ascending (MurmurHash3_x64_128 of the canonical k-mer,"
                 " sourmash's DNA rule)"
              << std::endl;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--output", &o.output, kUsage),
        path_flag("--report", &o.report),
        switch_flag("--singleton", &o.singleton),
        text_flag("--list", &o.list, "--list takes a file of input paths, one per line"),
        integer_flag("--ksize", &o.ksize, 1, 32, "--ksize takes an integer from 1 to 32"),
        integer_flag("--scaled", &o.scaled, 1, LONG_MAX, "--scaled takes an integer >= 1"),
        integer_flag("--seed", &o.seed, 0, 4294967295L, "--seed takes an integer from 0 to 4294967295"),
        integer_flag("--batch_bytes", &o.batch_bytes, 1, LONG_MAX, "--batch_bytes takes an integer >= 1"),
        device_flag(&o.device),
    };
    Args args = parse_flags(argc, argv, flags, &o.files);
    if (o.files.empty() && o.list.empty()) args.usage = true;     // nothing to sketch
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
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
    if (const int rc = sketch_in_batches(
            kProg, in, o.batch_bytes, o.device,
            [&](mvs_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int64_t m, mvs_hash_set** hs) {
                return mvs_hash_set_from_sequences(ctx, bytes, MVS_MEM_HOST, offsets, m, (int)o.ksize, (uint32_t)o.seed, max_hash, hs);
            },
            [](mvs_ctx* ctx, double* ms, int64_t* trips) { return mvs_ctx_kmer_stats(ctx, ms, nullptr, nullptr, nullptr, nullptr, trips); },
            mvs_ctx_kmer_sample_stats, tm))
        return rc;

    // ---- write: the text, then its parsed form ----
    const auto t_write = std::chrono::steady_clock::now();
    size_t total = 0;
    if (const int rc = write_sketches(kProg, o.output, in.samples, &total)) return rc;
    tm.write_s = seconds_since(t_write);
    if (!o.report.empty()) {
        std::string rep = sketch_report_rows(in.samples, "bases");
        rep += "# ksize " + std::to_string(o.ksize) + " scaled " + std::to_string(o.scaled) + " seed " + std::to_string(o.seed) +
               " max_hash " + std::to_string(max_hash) + "\n";
        rep += sketch_report_times(tm);
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Sketched " << n << " samples (" << in.bytes.size() << " bytes) at ksize " << o.ksize << ", scaled " << o.scaled << ": " << total
              << " hashes written" << std::endl;
    return 0;
}
