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

#include <unordered_set>

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

struct Gpu {
    OwnedCtx ctx;
    OwnedHashSet hs;
};

struct Sample {
    std::string name;
    int64_t bases = 0, records = 0, kmers = 0, kept = 0;
    std::vector<uint64_t> hashes;
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
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
    if (!o.list.empty()) {
        std::ifstream in(o.list);
        if (!in) {
            std::cerr << "Error opening " << o.list << " for reading." << std::endl;
            return 1;
        }
        std::string line;
        while (std::getline(in, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (!line.empty()) o.files.push_back(line);
        }
    }
    std::unordered_set<std::string> seen;
    auto name_ok = [&](const std::string& name, const std::string& from) {
        if (name.find_first_of(":\n") != std::string::npos) {
            std::cerr << kProg << ": the sample name '" << name << "' (" << from << ") contains ':'" << std::endl;
            return false;
        }
        if (!seen.insert(name).second) {
            std::cerr << kProg << ": duplicate sample name '" << name << "' (" << from << ")" << std::endl;
            return false;
        }
        return true;
    };
    if (!o.singleton)
        for (const std::string& f : o.files) {
            const std::string file_name = fs::path(f).filename().string();
            if (!name_ok(file_name.substr(0, file_name.find('.')), f)) return 1;
        }

    // ---- parse: every file into one buffer; a sample is a run of records ----
    const auto t_parse = std::chrono::steady_clock::now();
    std::string bases;
    std::vector<Sample> samples;
    std::vector<int64_t> begin;          // where each sample starts in `bases`; its bytes end where the next one starts
    for (const std::string& f : o.files) {
        std::vector<SeqRecord> recs;
        std::string err;
        if (!bases.empty()) bases.push_back('\n');
        const size_t file_begin = bases.size();
        if (!read_sequences(f, bases, recs, err)) {
            std::cerr << (err.compare(0, 14, "Error opening ") == 0 ? err : std::string(kProg) + ": " + err) << std::endl;
            return 1;
        }
        if (o.singleton) {
            for (const SeqRecord& r : recs) {
                if (!name_ok(r.name, f)) return 1;
                Sample s;
                s.name = r.name;
                s.bases = (int64_t)(r.end - r.begin);
                s.records = 1;
                samples.push_back(std::move(s));
                begin.push_back((int64_t)r.begin);
            }
        } else {
            const std::string file_name = fs::path(f).filename().string();
            Sample s;
            s.name = file_name.substr(0, file_name.find('.'));
            for (const SeqRecord& r : recs) s.bases += (int64_t)(r.end - r.begin);
            s.records = (int64_t)recs.size();
            samples.push_back(std::move(s));
            begin.push_back((int64_t)file_begin);
        }
    }
    begin.push_back((int64_t)bases.size());
    const double parse_s = seconds_since(t_parse);
    const int64_t n = (int64_t)samples.size();

    // ---- sketch: batches of whole samples ----
    uint64_t max_hash = 0;
    if (mvs_kmer_max_hash(o.scaled, &max_hash) != MVS_OK) return gpu_fail(kProg, "max_hash");
    double sketch_s = 0.0, kernel_ms = 0.0, export_s = 0.0;
    int64_t batches = 0, second_trips = 0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        mvs_ctx_set_timing(g.ctx, 1);
        for (int64_t s0 = 0; s0 < n;) {
            int64_t s1 = s0 + 1;
            while (s1 < n && begin[(size_t)s1 + 1] - begin[(size_t)s0] <= o.batch_bytes) ++s1;
            const int64_t m = s1 - s0;
            const auto t_sketch = std::chrono::steady_clock::now();
            if (mvs_hash_set_from_sequences(g.ctx, (const uint8_t*)bases.data(), MVS_MEM_HOST, begin.data() + s0, m, (int)o.ksize,
                                            (uint32_t)o.seed, max_hash, &g.hs) != MVS_OK)
                return gpu_fail(kProg, "sketching");
            sketch_s += seconds_since(t_sketch);
            double ms = 0.0;
            int64_t trips = 0;
            std::vector<int64_t> kmers((size_t)m), kept((size_t)m), off((size_t)m + 1);
            mvs_ctx_kmer_stats(g.ctx, &ms, nullptr, nullptr, nullptr, nullptr, &trips);
            kernel_ms += ms;
            second_trips += trips;
            const auto t_export = std::chrono::steady_clock::now();
            int64_t total = 0;
            if (mvs_ctx_kmer_sample_stats(g.ctx, m, kmers.data(), kept.data()) != MVS_OK ||
                mvs_hash_set_info(g.hs, nullptr, &total, nullptr) != MVS_OK)
                return gpu_fail(kProg, "reading the statistics");
            std::vector<uint64_t> flat((size_t)std::max<int64_t>(total, 1));
            if (mvs_hash_set_export(g.hs, flat.data(), MVS_MEM_HOST, off.data()) != MVS_OK) return gpu_fail(kProg, "reading the hashes");
            for (int64_t s = 0; s < m; ++s) {
                Sample& sm = samples[(size_t)(s0 + s)];
                sm.kmers = kmers[(size_t)s];
                sm.kept = kept[(size_t)s];
                sm.hashes.assign(flat.begin() + off[(size_t)s], flat.begin() + off[(size_t)s + 1]);
            }
            g.hs.reset();
            export_s += seconds_since(t_export);
            ++batches;
            s0 = s1;
        }
    }

    // ---- write: the text, then its parsed form ----
    const auto t_write = std::chrono::steady_clock::now();
    std::string text;
    size_t total = 0;
    for (const Sample& s : samples) {
        text += s.name + ":";
        for (uint64_t h : s.hashes) {
            text += ' ';
            text += std::to_string(h);
        }
        text += '\n';
        total += s.hashes.size();
    }
    if (const int rc = write_then_rename(kProg, o.output, text)) return rc;
    if (!getenv("MVS_NO_CSR_CACHE")) {
        HashSets sets;
        if (sets.hashes.reset(total)) {
            sets.offsets.assign(1, 0);
            for (const Sample& s : samples) {
                sets.names.push_back(s.name);
                if (!s.hashes.empty()) memcpy(sets.hashes.data() + sets.offsets.back(), s.hashes.data(), s.hashes.size() * 8);
                sets.offsets.push_back(sets.offsets.back() + (int64_t)s.hashes.size());
            }
            (void)write_csr_cache(o.output, sets);
        }
    }
    const double write_s = seconds_since(t_write);
    if (!o.report.empty()) {
        std::string rep = "sample\tbases\trecords\tkmers\tkept\tdistinct\n";
        for (const Sample& s : samples)
            rep += s.name + '\t' + std::to_string(s.bases) + '\t' + std::to_string(s.records) + '\t' + std::to_string(s.kmers) + '\t' +
                   std::to_string(s.kept) + '\t' + std::to_string(s.hashes.size()) + '\n';
        rep += "# ksize " + std::to_string(o.ksize) + " scaled " + std::to_string(o.scaled) + " seed " + std::to_string(o.seed) +
               " max_hash " + std::to_string(max_hash) + "\n";
        rep += "# batches " + std::to_string(batches) + " second_trips " + std::to_string(second_trips) + "\n";
        rep += "# parse_s " + fmt9(parse_s) + " sketch_s " + fmt9(sketch_s) + " kernel_ms " + fmt9(kernel_ms) + " export_s " + fmt9(export_s) +
               " write_s " + fmt9(write_s) + "\n";
        if (const int rc = write_then_rename(kProg, o.report, rep)) return rc;
    }
    std::cout << "Sketched " << n << " samples (" << bases.size() << " bytes) at ksize " << o.ksize << ", scaled " << o.scaled << ": " << total
              << " hashes written" << std::endl;
    return 0;
}
