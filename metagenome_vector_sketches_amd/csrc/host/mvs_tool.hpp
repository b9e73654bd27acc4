// mvs_tool.hpp -- what the tools over a sketch DB share (cluster_sketches, linkage_sketches, dereplicate_sketches, verify_pairs,
// pca_sketches, pcoa_sketches, gather_sketches, permanova_sketches, hdbscan_sketches, silhouette_sketches, hclust_sketches, communities_sketches, tsne_sketches, pairwise_comp_optimized for the loader, and sketch_sequences for the flag values and the output file): opening the DB folder, loading vectors.bin into a sketch set, reporting a
// device error, writing an output file under <file>.part, the hash file a DB was sketched from, and the parsing of flag values.  Header-only; include it after
// mvs_host.hpp.  Each tool keeps its own parse() chain, usage text, Gpu holder and output format.
#ifndef MVS_TOOL_HPP
#define MVS_TOOL_HPP

#include "mvs_host.hpp"

namespace mvs_host {

// ---- flag values ----
// the whole non-empty string is a number / a decimal integer; range checks are the caller's (they differ per flag)
inline bool parse_number(const std::string& v, double* out) {
    char* end = nullptr;
    *out = strtod(v.c_str(), &end);
    return !v.empty() && end != v.c_str() && !*end;
}
inline bool parse_integer(const std::string& v, long* out) {
    char* end = nullptr;
    *out = strtol(v.c_str(), &end, 10);
    return !v.empty() && end != v.c_str() && !*end;
}
// --device <i>: a device index
inline bool parse_device(const std::string& v, int* out) {
    long m = 0;
    if (!parse_integer(v, &m) || m < 0 || m > 1023) return false;
    *out = (int)m;
    return true;
}
// the device a tool works on: --device when it was given (>= 0), else MVS_DEVICE, else 0
inline int choose_device(int device_flag) { return device_flag >= 0 ? device_flag : pick_device(); }

// ---- errors and output ----
inline int gpu_fail(const char* prog, const char* what) {
    std::cerr << prog << ": " << what << ": " << mvs_last_error() << std::endl;
    return 2;
}

// `text` under <path>.part, then renamed
inline int write_then_rename(const char* prog, const std::string& path, const std::string& text) {
    const std::string part = path + ".part";
    {
        std::ofstream out(part, std::ios::binary | std::ios::trunc);
        out << text;
        out.flush();
        if (!out) {
            std::cerr << prog << ": cannot write " << part << std::endl;
            ::unlink(part.c_str());
            return 1;
        }
    }
    if (::rename(part.c_str(), path.c_str()) != 0) {
        std::cerr << prog << ": cannot rename " << part << " to " << path << std::endl;
        ::unlink(part.c_str());
        return 1;
    }
    return 0;
}

// ---- the DB folder ----
struct SketchDb {
    std::string folder, matrix_file;
    int dimension = 0, elem_bytes = 4;
    int64_t n = 0;          // vectors in vectors.bin
    DbInfo info;            // names and norms of those n
};

// Reads the DB the way pairwise_comp_optimized does: dimension.txt, dtype.txt (int32 unless it says int16), vector_norms.txt
// (names and norms), the size of vectors.bin.  0, or 1 after the reference's message on stderr.
inline int open_sketch_db(const std::string& folder, SketchDb& db) {
    db.folder = folder;
    const std::string norms_file = folder + "vector_norms.txt";                   // raw concatenation, as :853-891
    if (!fs::exists(norms_file)) {                                                // :855-858
        std::cerr << "Error: Required file 'vector_norms.txt' not found in output folder: " << folder << std::endl;
        return 1;
    }
    std::string dtype = "int32";
    {
        std::ifstream dtype_in(folder + "dtype.txt");                             // :859-865
        if (dtype_in) std::getline(dtype_in, dtype);
    }
    db.dimension = 0;
    {
        std::ifstream dim_in(folder + "dimension.txt");                           // :866-873
        if (dim_in) dim_in >> db.dimension;
    }
    if (db.dimension <= 0) {
        std::cerr << "Error: could not read a positive dimension from " << folder << "dimension.txt" << std::endl;
        return 1;
    }
    db.elem_bytes = dtype == "int16" ? 2 : 4;
    db.matrix_file = folder + "vectors.bin";                                      // :891
    read_norms(norms_file, db.info);                                              // :893-901
    int64_t file_size = 0;
    {
        std::ifstream file(db.matrix_file, std::ios::ate | std::ios::binary);     // :911-914
        file_size = file ? (int64_t)file.tellg() : 0;
    }
    db.n = file_size / ((int64_t)db.dimension * db.elem_bytes);
    if ((int64_t)db.info.norms_sq.size() < db.n) {
        std::cerr << "Error: vector_norms.txt has " << db.info.norms_sq.size() << " entries for " << db.n << " vectors" << std::endl;
        return 1;
    }
    db.info.norms_sq.resize((size_t)db.n);
    db.info.names.resize((size_t)db.n);
    return 0;
}

// vectors.bin of every DB of `dbs` (same dimension), one behind the other, goes through the device in row chunks straight from
// the page cache (the files are mapped, the library copies from the mappings) and is re-coded into the limb planes of *set (an
// earlier set there is destroyed), with a limb code that suits them all.  Reads matrix_file, elem_bytes, n and dimension of
// each.  0, 1 (a file) or 2 (the device), after a message on stderr.
inline int load_sketch_dbs(const char* prog, mvs_ctx* ctx, const std::vector<const SketchDb*>& dbs, mvs_sketch_set** set) {
    struct Mapping {
        const char* base = nullptr;
        size_t bytes = 0;
    };
    std::vector<Mapping> maps(dbs.size());
    auto unmap_all = [&] {
        for (const Mapping& m : maps)
            if (m.bytes) ::munmap((void*)m.base, m.bytes);
    };
    int64_t n = 0;
    for (size_t k = 0; k < dbs.size(); ++k) {
        const SketchDb& db = *dbs[k];
        const int fd = ::open(db.matrix_file.c_str(), O_RDONLY);
        if (fd < 0) {
            std::cerr << "Error opening file: " << db.matrix_file << std::endl;    // :35-38
            unmap_all();
            return 1;
        }
        const size_t bytes = (size_t)(db.n * (int64_t)db.dimension * db.elem_bytes);
        if (bytes) {
            void* m = ::mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) {
                ::close(fd);
                std::cerr << "Error reading file: " << db.matrix_file << std::endl;
                unmap_all();
                return 1;
            }
            ::madvise(m, bytes, MADV_SEQUENTIAL);
            maps[k].base = (const char*)m;
            maps[k].bytes = bytes;
        }
        ::close(fd);
        n += db.n;
    }
    // One pass in the common case: the planes are allocated for two limbs (|v| <= 32639, i.e. samples of up to tens
    // of millions of hashes) and every chunk reports its largest |v| with the same upload; only if a chunk needs
    // more limbs than the set has does the load start over with the limb count the data seen so far asks for.
    int rc = 0;
    for (int limbs = 2, attempt = 0; attempt < 4 && !rc; ++attempt) {
        if (*set) {
            mvs_sketch_set_destroy(*set);
            *set = nullptr;
        }
        if (mvs_sketch_set_alloc(ctx, n, dbs[0]->dimension, limbs, set) != MVS_OK) {
            rc = gpu_fail(prog, "allocating sketch set");
            break;
        }
        int64_t max_abs = 0, first = 0;
        for (size_t k = 0; k < dbs.size(); ++k) {
            const SketchDb& db = *dbs[k];
            const int64_t row_bytes = (int64_t)db.dimension * db.elem_bytes;
            const int64_t chunk_rows = std::max<int64_t>(1, (1LL << 30) / row_bytes);
            for (int64_t r0 = 0; r0 < db.n && !rc && mvs_limbs_for_max_abs(max_abs) <= limbs; r0 += chunk_rows) {
                int64_t m = 0;
                if (mvs_sketch_set_fill_stats(*set, maps[k].base + r0 * row_bytes, db.elem_bytes, MVS_MEM_HOST, first + r0,
                                              std::min(chunk_rows, db.n - r0), &m) != MVS_OK)
                    rc = gpu_fail(prog, "re-coding vectors.bin");
                max_abs = std::max(max_abs, m);
            }
            first += db.n;
        }
        if (mvs_limbs_for_max_abs(max_abs) <= limbs) break;
        limbs = mvs_limbs_for_max_abs(max_abs);
    }
    unmap_all();
    return rc;
}
inline int load_sketch_db(const char* prog, mvs_ctx* ctx, const SketchDb& db, mvs_sketch_set** set) {
    return load_sketch_dbs(prog, ctx, {&db}, set);
}

// ---- what the ordination tools share (pca_sketches, pcoa_sketches; permanova_sketches for the norms and its report) ----
inline std::string fmt9(double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.9g", v);
    return buf;
}

// the norms of vector_norms.txt as read_norms takes them (the text after the first space), not squared
inline std::vector<double> read_plain_norms(const std::string& file, int64_t n) {
    std::vector<double> norms;
    std::ifstream in(file);
    std::string line;
    while ((int64_t)norms.size() < n && std::getline(in, line)) {
        const size_t pos = line.find(' ');
        if (pos == std::string::npos) continue;
        norms.push_back(std::stod(line.substr(pos + 1)));
    }
    return norms;
}

// name  fitted(1/0)  c values as %.9g, one line per sample; fitted == nullptr: 0 throughout
inline std::string scores_text(const std::vector<std::string>& names, const std::vector<char>* fitted, const std::vector<double>& scores, int c) {
    std::string text;
    for (size_t i = 0; i < names.size(); ++i) {
        text += names[i];
        text += fitted && (*fitted)[i] ? "\t1" : "\t0";
        for (int j = 0; j < c; ++j) text += '\t' + fmt9(scores[i * (size_t)c + j]);
        text += '\n';
    }
    return text;
}

// ---- the hash file a DB was sketched from ----
// The hash lists of the DB's samples: the parsed form `project_everything sketch` left next to the text (<file>.csr) when it
// is valid, else the text.  The file's sample names must be the DB's names in the DB's order.  0, or 1 after a message on
// stderr; no device is needed.
inline int load_db_hashes(const char* prog, const std::string& hash_file, const SketchDb& db, HashSets& sets) {
    bool parsed = load_csr_cache(hash_file, sets);
    if (!parsed) {
        try {
            parsed = read_hash_file(hash_file, true, sets);
        } catch (const std::exception& e) {
            std::cerr << prog << ": reading " << hash_file << ": " << e.what() << std::endl;
            return 1;
        }
    }
    if (!parsed) {
        std::cerr << "Error opening " << hash_file << " for reading." << std::endl;
        return 1;
    }
    const std::vector<std::string>& names = db.info.names;
    if ((int64_t)sets.names.size() != db.n || !std::equal(sets.names.begin(), sets.names.end(), names.begin())) {
        size_t at = 0;
        while (at < sets.names.size() && at < (size_t)db.n && sets.names[at] == names[at]) ++at;
        std::cerr << prog << ": the samples of " << hash_file << " (" << sets.names.size() << ") are not those of " << db.folder
                  << "vector_norms.txt (" << db.n << ") in the same order: first difference at sample " << at << std::endl;
        return 1;
    }
    return 0;
}

}  // namespace mvs_host

#endif
