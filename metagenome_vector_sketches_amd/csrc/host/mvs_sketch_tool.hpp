// mvs_sketch_tool.hpp -- what sketch_sequences and sketch_proteins share around their library call: the input list, the sample
// names and their checks, the files parsed into one buffer of samples, the batches of whole samples handed to the library, the
// hash text with its .csr cache, and the per-sample lines of the report.  Included after mvs_host.hpp, mvs_tool.hpp and
// mvs_fasta.hpp.
#pragma once

#include <unordered_set>

namespace mvs_host {

struct SketchSample {
    std::string name;
    int64_t bases = 0, records = 0, kmers = 0, kept = 0;
    std::vector<uint64_t> hashes;
};

// what the batches cost and did
struct SketchTimes {
    double parse_s = 0.0, sketch_s = 0.0, kernel_ms = 0.0, export_s = 0.0, write_s = 0.0;
    int64_t batches = 0, second_trips = 0;
};

inline double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the input files parsed into `bytes`: one sample per file, or per record with `singleton`
struct SketchInput {
    std::string bytes;
    std::vector<SketchSample> samples;
    std::vector<int64_t> begin;          // where each sample starts in `bytes`; its bytes end where the next one starts
};

// --list: one more input path per line.  -> 0, or the exit code
inline int append_list_file(const std::string& list, std::vector<std::string>& files) {
    if (list.empty()) return 0;
    std::ifstream in(list);
    if (!in) {
        std::cerr << "Error opening " << list << " for reading." << std::endl;
        return 1;
    }
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty()) files.push_back(line);
    }
    return 0;
}

// Names must differ and must not contain ':' (the text format ends the name there).  Without `singleton` the names are the file
// names up to their first '.', checked before a file is opened; with it the records' names, checked as they are read.
inline int read_sketch_input(const char* prog, const std::vector<std::string>& files, bool singleton, SketchInput& in) {
    std::unordered_set<std::string> seen;
    auto name_ok = [&](const std::string& name, const std::string& from) {
        if (name.find_first_of(":\n") != std::string::npos) {
            std::cerr << prog << ": the sample name '" << name << "' (" << from << ") contains ':'" << std::endl;
            return false;
        }
        if (!seen.insert(name).second) {
            std::cerr << prog << ": duplicate sample name '" << name << "' (" << from << ")" << std::endl;
            return false;
        }
        return true;
    };
    auto sample_name = [](const std::string& f) {
        const std::string file_name = fs::path(f).filename().string();
        return file_name.substr(0, file_name.find('.'));
    };
    if (!singleton)
        for (const std::string& f : files)
            if (!name_ok(sample_name(f), f)) return 1;
    for (const std::string& f : files) {
        std::vector<SeqRecord> recs;
        std::string err;
        if (!in.bytes.empty()) in.bytes.push_back('\n');
        const size_t file_begin = in.bytes.size();
        if (!read_sequences(f, in.bytes, recs, err)) {
            std::cerr << (err.compare(0, 14, "Error opening ") == 0 ? err : std::string(prog) + ": " + err) << std::endl;
            return 1;
        }
        if (singleton) {
            for (const SeqRecord& r : recs) {
                if (!name_ok(r.name, f)) return 1;
                SketchSample s;
                s.name = r.name;
                s.bases = (int64_t)(r.end - r.begin);
                s.records = 1;
                in.samples.push_back(std::move(s));
                in.begin.push_back((int64_t)r.begin);
            }
        } else {
            SketchSample s;
            s.name = sample_name(f);
            for (const SeqRecord& r : recs) s.bases += (int64_t)(r.end - r.begin);
            s.records = (int64_t)recs.size();
            in.samples.push_back(std::move(s));
            in.begin.push_back((int64_t)file_begin);
        }
    }
    in.begin.push_back((int64_t)in.bytes.size());
    return 0;
}

// Batches of whole samples of up to batch_bytes bytes (a larger sample is a batch of its own).  sketch(ctx, bytes, offsets, m,
// &set) is the library call; stats(ctx, &kernel_ms, &second_trips) and sample_stats(ctx, m, kmers, kept) read what it left.
template <class Sketch, class Stats, class SampleStats>
int sketch_in_batches(const char* prog, SketchInput& in, long batch_bytes, int device, Sketch sketch, Stats stats, SampleStats sample_stats,
                      SketchTimes& tm) {
    const int64_t n = (int64_t)in.samples.size();
    if (n == 0) return 0;
    OwnedCtx ctx;
    OwnedHashSet hs;
    if (mvs_ctx_create(choose_device(device), &ctx) != MVS_OK) return gpu_fail(prog, "creating context");
    mvs_ctx_set_timing(ctx, 1);
    for (int64_t s0 = 0; s0 < n;) {
        int64_t s1 = s0 + 1;
        while (s1 < n && in.begin[(size_t)s1 + 1] - in.begin[(size_t)s0] <= batch_bytes) ++s1;
        const int64_t m = s1 - s0;
        const auto t_sketch = std::chrono::steady_clock::now();
        if (sketch((mvs_ctx*)ctx, (const uint8_t*)in.bytes.data(), in.begin.data() + s0, m, &hs) != MVS_OK) return gpu_fail(prog, "sketching");
        tm.sketch_s += seconds_since(t_sketch);
        double ms = 0.0;
        int64_t trips = 0;
        std::vector<int64_t> kmers((size_t)m), kept((size_t)m), off((size_t)m + 1);
        stats((mvs_ctx*)ctx, &ms, &trips);
        tm.kernel_ms += ms;
        tm.second_trips += trips;
        const auto t_export = std::chrono::steady_clock::now();
        int64_t total = 0;
        if (sample_stats((mvs_ctx*)ctx, m, kmers.data(), kept.data()) != MVS_OK || mvs_hash_set_info(hs, nullptr, &total, nullptr) != MVS_OK)
            return gpu_fail(prog, "reading the statistics");
        std::vector<uint64_t> flat((size_t)std::max<int64_t>(total, 1));
        if (mvs_hash_set_export(hs, flat.data(), MVS_MEM_HOST, off.data()) != MVS_OK) return gpu_fail(prog, "reading the hashes");
        for (int64_t s = 0; s < m; ++s) {
            SketchSample& sm = in.samples[(size_t)(s0 + s)];
            sm.kmers = kmers[(size_t)s];
            sm.kept = kept[(size_t)s];
            sm.hashes.assign(flat.begin() + off[(size_t)s], flat.begin() + off[(size_t)s + 1]);
        }
        hs.reset();
        tm.export_s += seconds_since(t_export);
        ++tm.batches;
        s0 = s1;
    }
    return 0;
}

// "name: h1 h2 ..." per sample under <output>.part, renamed when complete, then its parsed form as <output>.csr.  -> 0 or the
// exit code; *total: values written
inline int write_sketches(const char* prog, const std::string& output, const std::vector<SketchSample>& samples, size_t* total) {
    std::string text;
    *total = 0;
    for (const SketchSample& s : samples) {
        text += s.name + ":";
        for (uint64_t h : s.hashes) {
            text += ' ';
            text += std::to_string(h);
        }
        text += '\n';
        *total += s.hashes.size();
    }
    if (const int rc = write_then_rename(prog, output, text)) return rc;
    if (!getenv("MVS_NO_CSR_CACHE")) {
        HashSets sets;
        if (sets.hashes.reset(*total)) {
            sets.offsets.assign(1, 0);
            for (const SketchSample& s : samples) {
                sets.names.push_back(s.name);
                if (!s.hashes.empty()) memcpy(sets.hashes.data() + sets.offsets.back(), s.hashes.data(), s.hashes.size() * 8);
                sets.offsets.push_back(sets.offsets.back() + (int64_t)s.hashes.size());
            }
            (void)write_csr_cache(output, sets);
        }
    }
    return 0;
}

// the report's table: `unit` names what a sample's bytes are ("bases", "bytes")
inline std::string sketch_report_rows(const std::vector<SketchSample>& samples, const char* unit) {
    std::string rep = std::string("sample\t") + unit + "\trecords\tkmers\tkept\tdistinct\n";
    for (const SketchSample& s : samples)
        rep += s.name + '\t' + std::to_string(s.bases) + '\t' + std::to_string(s.records) + '\t' + std::to_string(s.kmers) + '\t' +
               std::to_string(s.kept) + '\t' + std::to_string(s.hashes.size()) + '\n';
    return rep;
}
inline std::string sketch_report_times(const SketchTimes& tm) {
    return "# batches " + std::to_string(tm.batches) + " second_trips " + std::to_string(tm.second_trips) + "\n# parse_s " + fmt9(tm.parse_s) +
           " sketch_s " + fmt9(tm.sketch_s) + " kernel_ms " + fmt9(tm.kernel_ms) + " export_s " + fmt9(tm.export_s) + " write_s " +
           fmt9(tm.write_s) + "\n";
}

}  // namespace mvs_host
