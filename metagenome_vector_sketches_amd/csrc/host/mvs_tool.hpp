// mvs_tool.hpp -- what the tools over a sketch DB share: the fourteen *_sketches tools, verify_pairs, sketch_sequences (the
// command line, the device holders and the output file) and pairwise_comp_optimized (the loader).  It holds
//   - the command line: one Flag per flag, parse_flags() over the table, Args for what it found and for the exit;
//   - the holders of what a tool keeps on the device (Owned, DeviceMem);
//   - reporting a device error and writing an output file under <file>.part;
//   - opening the DB folder and loading vectors.bin into a sketch set;
//   - the row-block loop of the tools that answer kept cells on the device (for_kept_cell_blocks);
//   - what the ordination tools share;
//   - the hash file a DB was sketched from.
// Header-only; include it after mvs_host.hpp.  Each tool keeps its own flag table, usage text and output format.
#ifndef MVS_TOOL_HPP
#define MVS_TOOL_HPP

#include "mvs_host.hpp"

#include <climits>
#include <functional>
#include <utility>

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

// ---- the command line ----
// A tool describes its flags once, as a table of Flag, and parse_flags() walks argv over it.  The rules, the same for every tool:
// "--help" in a flag's place asks for the usage text and wins over everything.  A flag that takes a value takes the next argument
// whatever it looks like; at the end of argv a checked flag judges the empty string and a path flag counts as an unknown argument.
// A value that `take` refuses leaves the flag's text as the refusal, and the first refusal in argv order stands; a flag given
// twice keeps its last good value.  After argv the absent flags speak in table order: kRefuse as if their value had been
// refused, kUsage by asking for the usage text.  A refusal (exit 1, one line on stderr) goes before the usage text (exit 1, on
// stdout), which is what an unknown argument, a path flag without a value or an absent kUsage flag lead to.
enum Absent { kOptional, kRefuse, kUsage };

struct Flag {
    enum Kind { kPath, kChecked, kSwitch };
    const char* name;
    Kind kind;
    std::function<bool(const std::string&)> take;    // stores a good value and says yes; a kSwitch gets ""
    std::string refusal;                              // "<name> takes ...", printed after "<prog>: "
    Absent absent = kOptional;
    bool given = false;                               // parse_flags: it took a value
};

// a path or a text that is not judged: --db, --output, --report, ...
inline Flag path_flag(const char* name, std::string* out, Absent absent = kOptional) {
    return {name, Flag::kPath, [out](const std::string& v) { return *out = v, true; }, "", absent};
}
// a text that must not be empty: --hashes, --list, --query
inline Flag text_flag(const char* name, std::string* out, std::string refusal, Absent absent = kOptional) {
    return {name, Flag::kChecked, [out](const std::string& v) { return v.empty() ? false : (*out = v, true); }, std::move(refusal), absent};
}
// a number that `ok` accepts
inline Flag number_flag(const char* name, double* out, bool (*ok)(double), std::string refusal, Absent absent = kOptional) {
    auto take = [out, ok](const std::string& v) {
        double x = 0.0;
        return parse_number(v, &x) && ok(x) ? (*out = x, true) : false;
    };
    return {name, Flag::kChecked, take, std::move(refusal), absent};
}
inline bool in_open_unit(double x) { return x > 0.0 && x < 1.0; }       // (0,1)
inline bool in_half_open_unit(double x) { return x >= 0.0 && x < 1.0; }  // [0,1)
inline bool not_nan(double x) { return !std::isnan(x); }
inline bool positive_finite(double x) { return x > 0.0 && !std::isinf(x); }
// a decimal integer in lo .. hi
template <class T>
Flag integer_flag(const char* name, T* out, long lo, long hi, std::string refusal, Absent absent = kOptional) {
    auto take = [out, lo, hi](const std::string& v) {
        long x = 0;
        return parse_integer(v, &x) && x >= lo && x <= hi ? (*out = (T)x, true) : false;
    };
    return {name, Flag::kChecked, take, std::move(refusal), absent};
}
// one word of a list, each with the value it stands for
template <class T>
Flag word_flag(const char* name, T* out, std::vector<std::pair<std::string, T>> words, std::string refusal) {
    auto take = [out, words](const std::string& v) {
        for (const auto& w : words)
            if (v == w.first) return *out = w.second, true;
        return false;
    };
    return {name, Flag::kChecked, take, std::move(refusal), kOptional};
}
inline Flag device_flag(int* out) {
    return {"--device", Flag::kChecked, [out](const std::string& v) { return parse_device(v, out); }, "--device takes a device index", kOptional};
}
// a flag without a value
inline Flag switch_flag(const char* name, bool* out) {
    return {name, Flag::kSwitch, [out](const std::string&) { return *out = true; }, "", kOptional};
}
// a value nobody else has: `take` judges and stores it
inline Flag hook_flag(const char* name, std::function<bool(const std::string&)> take, std::string refusal) {
    return {name, Flag::kChecked, std::move(take), std::move(refusal), kOptional};
}
inline bool was_given(const std::vector<Flag>& flags, const std::string& name) {
    for (const Flag& f : flags)
        if (name == f.name) return f.given;
    return false;
}

// What parse_flags() found.  A tool's own rules across flags go between the parse and exit_code(): refuse() keeps the first
// refusal, so a rule never speaks over a flag that was refused before it, and `usage = true` asks for the usage text.
struct Args {
    bool help = false, usage = false;
    std::string refusal;
    void refuse(const std::string& text) {
        if (refusal.empty()) refusal = text;
    }
    // what main returns before it touches anything, or -1: go on
    int exit_code(const char* prog, void (*print_usage)(const char*), const char* argv0) const {
        if (help) return print_usage(argv0), 0;
        if (!refusal.empty()) return std::cerr << prog << ": " << refusal << std::endl, 1;
        if (usage) return print_usage(argv0), 1;
        return -1;
    }
};

// files != nullptr: an argument that is no flag and does not begin with "--" is an input file (sketch_sequences)
inline Args parse_flags(int argc, char* argv[], std::vector<Flag>& flags, std::vector<std::string>* files = nullptr) {
    Args args;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_value = i + 1 < argc;
        Flag* flag = nullptr;
        for (Flag& f : flags)
            if (a == f.name) flag = &f;
        if (a == "--help") args.help = true;
        else if (!flag && files && a.compare(0, 2, "--") != 0) files->push_back(a);
        else if (!flag || (flag->kind == Flag::kPath && !has_value)) args.usage = true;
        else if (flag->take(flag->kind != Flag::kSwitch && has_value ? argv[++i] : "")) flag->given = true;
        else args.refuse(flag->refusal);
    }
    for (const Flag& f : flags) {
        if (!f.given && f.absent == kRefuse) args.refuse(f.refusal);
        if (!f.given && f.absent == kUsage) args.usage = true;
    }
    return args;
}

// ---- what a tool holds on the device ----
// One object of the C ABI, destroyed with its holder.  A tool lists its holders as plain members of a struct and writes no
// destructor.  THE ORDER OF THE MEMBERS MATTERS: members are destroyed in reverse order of declaration, and whatever was made on
// a context -- device memory above all -- must go before the context does.  So the context is declared first, the sets next,
// device memory after them, and what is built from those last.
template <class T, int (*Destroy)(T*)>
struct Owned {
    T* p = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (p) Destroy(p);
        p = nullptr;
    }
    operator T*() const { return p; }
    T** operator&() { return &p; }                    // where mvs_*_create and load_sketch_dbs put (and replace) the object
};
using OwnedCtx = Owned<mvs_ctx, mvs_ctx_destroy>;
using OwnedSketchSet = Owned<mvs_sketch_set, mvs_sketch_set_destroy>;
using OwnedHashSet = Owned<mvs_hash_set, mvs_hash_set_destroy>;

// memory of mvs_device_alloc (not cleared), which is freed on the context it came from: declare it after that context
struct DeviceMem {
    mvs_ctx* ctx = nullptr;
    void* p = nullptr;
    DeviceMem() = default;
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    ~DeviceMem() { free(); }
    int alloc(mvs_ctx* on, size_t bytes) {
        free();
        ctx = on;
        return mvs_device_alloc(ctx, bytes, 0, &p);
    }
    void free() {
        if (p) mvs_device_free(ctx, p);
        p = nullptr;
    }
};

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

// ---- kept cells answered on the device (verify_pairs, abundance_pairs --db, contain_sketches) ----
// The rows [0, n) in blocks: compare(rb, re, d_cells, capacity, &count) leaves a block's kept cells in device memory and
// returns the library's code; a block that keeps more than the buffers hold (MVS_E_CAPACITY: count is what it needs) is done
// again with larger ones.  consume(d_cells, d_results, count) then answers the cells into `results`, result_bytes per cell, and
// takes both home; it returns the tool's exit code, 0 to go on.  A tool's time accounting goes into its compare, which runs
// once per attempt.  The two buffers are the tool's (declared after its context, as every DeviceMem).  0, or the exit code
// after a message on stderr.
template <class Compare, class Consume>
int for_kept_cell_blocks(const char* prog, mvs_ctx* ctx, int64_t n, size_t result_bytes, DeviceMem& cells, DeviceMem& results,
                         Compare&& compare, Consume&& consume) {
    const int64_t block_rows = std::max<int64_t>(256, std::min<int64_t>(n, (1LL << 28) / std::max<int64_t>(n, 1) / 256 * 256));
    int64_t capacity = 1 << 20;
    for (int64_t rb = 0; rb < n;) {
        const int64_t re = std::min(n, rb + block_rows);
        if (!cells.p && (cells.alloc(ctx, (size_t)capacity * sizeof(mvs_cell)) != MVS_OK || results.alloc(ctx, (size_t)capacity * result_bytes) != MVS_OK))
            return gpu_fail(prog, "allocating the cell buffers");
        int64_t count = 0;
        const int rc = compare(rb, re, (mvs_cell*)cells.p, capacity, &count);
        if (rc == MVS_E_CAPACITY) {
            cells.free();
            results.free();
            capacity = count + count / 8 + 1024;
            continue;
        }
        if (rc != MVS_OK) return gpu_fail(prog, "comparing");
        if (count > 0)
            if (const int exit_code = consume((const mvs_cell*)cells.p, results.p, count)) return exit_code;
        rb = re;
    }
    return 0;
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
    if (const int rc = load_hash_sets(prog, hash_file, true, sets)) return rc;
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
