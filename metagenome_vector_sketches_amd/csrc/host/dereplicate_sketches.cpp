// dereplicate_sketches -- greedy dereplication of the samples of a sketch DB at a Jaccard level, computed on the MI355X: a set
// of representatives such that every sample is within the level of its representative and no two representatives are within
// the level of each other (the rule of dRep, galah, CD-HIT, linclust).  The reference has no such tool.  The comparison's kept
// cells never leave the device (mvs_dereplicate); the answer is one line per sample.
//
//   dereplicate_sketches --db <folder>/ --min_jaccard <t> --output <file> [--order norm|index] [--device <i>] [--help]
//
// Reads the DB the way pairwise_comp_optimized does: dimension.txt, dtype.txt (int32 unless it says int16), vector_norms.txt
// (names and norms, :893-901), vectors.bin.  Two samples are linked iff their Jaccard estimate (:661-662) exceeds t (0 < t < 1).
// Samples are walked in priority order -- --order norm (default): the largest norm, i.e. the largest estimated hash set, first,
// equal norms in DB order; --order index: DB order -- and a sample becomes a representative iff no representative before it is
// linked to it; otherwise it joins the earliest representative linked to it.  The output is tab-separated, written under
// <file>.part and renamed when complete:
//   #sample  representative  jaccard  size
// one line per sample in DB order -- its name, the NAME of its representative (itself for a representative), the Jaccard estimate
// to the representative (inter = dot / d; J = inter / (n2_a + n2_b - inter), %.9g; 1 for a representative) and the size of the
// representative's group.  One line on stdout:
//   Dereplicated <n> samples at Jaccard > <t>: <R> representatives, <S> singletons, largest <L>
// Exit codes: 1 bad arguments or DB, 2 device errors.  One GPU (--device, else MVS_DEVICE, else 0).
#include "mvs_host.hpp"

namespace fs = std::filesystem;
using namespace mvs_host;

namespace {

struct Options {
    std::string db_folder, output, bad_flag;
    double min_jaccard = 0.0;
    bool by_index = false;
    int device = -1;
    bool show_help = false, have_db = false, have_t = false, have_out = false, unknown = false;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0 << " --db <folder> --min_jaccard <float in (0,1)> --output <file> [--order norm|index] [--device <int>] [--help]"
              << std::endl;
}

// bad_flag: the first flag whose value is missing, unparsable or out of range (reported before anything is touched)
void parse(int argc, char* argv[], Options& o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_value = i + 1 < argc;
        auto bad = [&](const char* flag) {
            if (o.bad_flag.empty()) o.bad_flag = flag;
        };
        char* end = nullptr;
        if (a == "--help") {
            o.show_help = true;
        } else if (a == "--db" || a == "--output") {
            if (!has_value) {
                o.unknown = true;
                continue;
            }
            (a == "--db" ? o.db_folder : o.output) = argv[++i];
            (a == "--db" ? o.have_db : o.have_out) = true;
        } else if (a == "--min_jaccard") {
            o.have_t = true;
            const std::string v = has_value ? argv[++i] : "";
            const double t = strtod(v.c_str(), &end);
            if (v.empty() || end == v.c_str() || *end || !(t > 0.0) || !(t < 1.0)) bad("--min_jaccard");
            else o.min_jaccard = t;
        } else if (a == "--order") {
            const std::string v = has_value ? argv[++i] : "";
            if (v != "norm" && v != "index") bad("--order");
            else o.by_index = v == "index";
        } else if (a == "--device") {
            const std::string v = has_value ? argv[++i] : "";
            const long m = strtol(v.c_str(), &end, 10);
            if (v.empty() || end == v.c_str() || *end || m < 0 || m > 1023) bad("--device");
            else o.device = (int)m;
        } else {
            o.unknown = true;
        }
    }
}

struct Gpu {
    mvs_ctx* ctx = nullptr;
    mvs_sketch_set* set = nullptr;
    ~Gpu() {
        if (set) mvs_sketch_set_destroy(set);
        if (ctx) mvs_ctx_destroy(ctx);
    }
};

int gpu_fail(const char* what) {
    std::cerr << "dereplicate_sketches: " << what << ": " << mvs_last_error() << std::endl;
    return 2;
}

// vectors.bin -> limb planes, in row chunks straight from the mapping; two limbs unless a chunk's largest |v| asks for more
int load_db(Gpu& g, const std::string& matrix_file, int elem_bytes, int64_t n, int d) {
    const int64_t row_bytes = (int64_t)d * elem_bytes;
    const int64_t chunk_rows = std::max<int64_t>(1, (1LL << 30) / row_bytes);
    const int fd = ::open(matrix_file.c_str(), O_RDONLY);
    if (fd < 0) {
        std::cerr << "Error opening file: " << matrix_file << std::endl;       // :35-38
        return 1;
    }
    const size_t bytes = (size_t)(n * row_bytes);
    const char* base = nullptr;
    if (bytes) {
        void* m = ::mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            ::close(fd);
            std::cerr << "Error reading file: " << matrix_file << std::endl;
            return 1;
        }
        ::madvise(m, bytes, MADV_SEQUENTIAL);
        base = (const char*)m;
    }
    ::close(fd);
    int rc = 0;
    for (int limbs = 2, attempt = 0; attempt < 4 && !rc; ++attempt) {
        if (g.set) {
            mvs_sketch_set_destroy(g.set);
            g.set = nullptr;
        }
        if (mvs_sketch_set_alloc(g.ctx, n, d, limbs, &g.set) != MVS_OK) {
            rc = gpu_fail("allocating sketch set");
            break;
        }
        int64_t max_abs = 0;
        for (int64_t r0 = 0; r0 < n && !rc && mvs_limbs_for_max_abs(max_abs) <= limbs; r0 += chunk_rows) {
            int64_t m = 0;
            if (mvs_sketch_set_fill_stats(g.set, base + r0 * row_bytes, elem_bytes, MVS_MEM_HOST, r0, std::min(chunk_rows, n - r0), &m) != MVS_OK)
                rc = gpu_fail("re-coding vectors.bin");
            max_abs = std::max(max_abs, m);
        }
        if (mvs_limbs_for_max_abs(max_abs) <= limbs) break;
        limbs = mvs_limbs_for_max_abs(max_abs);
    }
    if (bytes) ::munmap((void*)base, bytes);
    return rc;
}

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    parse(argc, argv, o);
    if (o.show_help) {
        print_usage(argv[0]);
        return 0;
    }
    if (!o.have_t && o.bad_flag.empty()) o.bad_flag = "--min_jaccard";
    if (!o.bad_flag.empty()) {
        if (o.bad_flag == "--min_jaccard") std::cerr << "dereplicate_sketches: --min_jaccard takes a number in the open range (0,1)" << std::endl;
        else if (o.bad_flag == "--order") std::cerr << "dereplicate_sketches: --order takes norm or index" << std::endl;
        else std::cerr << "dereplicate_sketches: --device takes a device index" << std::endl;
        return 1;
    }
    if (o.unknown || !o.have_db || !o.have_out) {
        print_usage(argv[0]);
        return 1;
    }
    const std::string db_folder = o.db_folder;
    const std::string norms_file = db_folder + "vector_norms.txt";                // raw concatenation, as :853-891
    if (!fs::exists(norms_file)) {                                                // :855-858
        std::cerr << "Error: Required file 'vector_norms.txt' not found in output folder: " << db_folder << std::endl;
        return 1;
    }
    std::string dtype = "int32";
    {
        std::ifstream dtype_in(db_folder + "dtype.txt");                          // :859-865
        if (dtype_in) std::getline(dtype_in, dtype);
    }
    int dimension = 0;
    {
        std::ifstream dim_in(db_folder + "dimension.txt");                        // :866-873
        if (dim_in) dim_in >> dimension;
    }
    if (dimension <= 0) {
        std::cerr << "Error: could not read a positive dimension from " << db_folder << "dimension.txt" << std::endl;
        return 1;
    }
    const int elem_bytes = dtype == "int16" ? 2 : 4;
    const std::string matrix_file = db_folder + "vectors.bin";                    // :891
    DbInfo db;
    read_norms(norms_file, db);                                                   // :893-901
    int64_t file_size = 0;
    {
        std::ifstream file(matrix_file, std::ios::ate | std::ios::binary);        // :911-914
        file_size = file ? (int64_t)file.tellg() : 0;
    }
    const int64_t n = file_size / ((int64_t)dimension * elem_bytes);
    if ((int64_t)db.norms_sq.size() < n) {
        std::cerr << "Error: vector_norms.txt has " << db.norms_sq.size() << " entries for " << n << " vectors" << std::endl;
        return 1;
    }
    db.norms_sq.resize((size_t)n);
    db.names.resize((size_t)n);

    std::vector<int32_t> rep_of((size_t)n), link_dot((size_t)n), link_q((size_t)n), sizes((size_t)n);
    int64_t n_reps = 0;
    if (n > 0) {
        Gpu g;
        const int device = o.device >= 0 ? o.device : pick_device();
        if (mvs_ctx_create(device, &g.ctx) != MVS_OK) return gpu_fail("creating context");
        const int rc = load_db(g, matrix_file, elem_bytes, n, dimension);
        if (rc) return rc;
        std::vector<int32_t> index_order;
        if (o.by_index) {
            index_order.resize((size_t)n);
            for (int64_t i = 0; i < n; ++i) index_order[(size_t)i] = (int32_t)i;
        }
        if (mvs_dereplicate(g.ctx, g.set, db.norms_sq.data(), MVS_MEM_HOST, o.min_jaccard, o.by_index ? index_order.data() : nullptr,
                            rep_of.data(), link_dot.data(), link_q.data(), sizes.data(), MVS_MEM_HOST, &n_reps) != MVS_OK)
            return gpu_fail("dereplicating");
    }
    int64_t singletons = 0, largest = 0;
    for (int64_t i = 0; i < n; ++i) {
        singletons += sizes[(size_t)i] == 1;
        largest = std::max<int64_t>(largest, sizes[(size_t)i]);
    }
    const std::string part = o.output + ".part";
    {
        std::ofstream out(part, std::ios::binary | std::ios::trunc);
        out << "#sample\trepresentative\tjaccard\tsize\n";
        char buf[64];
        for (int64_t i = 0; i < n; ++i) {
            const int32_t r = rep_of[(size_t)i];
            double j = 1.0;
            if (r != (int32_t)i) {                                                // the estimate before its clamp, as --top_k scores it
                const double inter = (double)link_dot[(size_t)i] / (double)dimension;
                j = inter / (db.norms_sq[(size_t)i] + db.norms_sq[(size_t)r] - inter);
            }
            snprintf(buf, sizeof(buf), "%.9g", j);
            out << db.names[(size_t)i] << '\t' << db.names[(size_t)r] << '\t' << buf << '\t' << sizes[(size_t)r] << '\n';
        }
        out.flush();
        if (!out) {
            std::cerr << "dereplicate_sketches: cannot write " << part << std::endl;
            ::unlink(part.c_str());
            return 1;
        }
    }
    if (::rename(part.c_str(), o.output.c_str()) != 0) {
        std::cerr << "dereplicate_sketches: cannot rename " << part << " to " << o.output << std::endl;
        ::unlink(part.c_str());
        return 1;
    }
    std::cout << "Dereplicated " << n << " samples at Jaccard > " << o.min_jaccard << ": " << n_reps << " representatives, " << singletons
              << " singletons, largest " << largest << std::endl;
    return 0;
}
