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
#include "mvs_tool.hpp"

using namespace mvs_host;

namespace {

constexpr const char* kProg = "dereplicate_sketches";

struct Options {
    std::string db_folder, output;
    double min_jaccard = 0.0;
    bool by_index = false;
    int device = -1;
};

void print_usage(const char* argv0) {
    std::cout << "Usage:\n"
              << "        " << argv0 << " --db <folder> --min_jaccard <float in (0,1)> --output <file> [--order norm|index] [--device <int>] [--help]"
              << std::endl;
}

struct Gpu {
    OwnedCtx ctx;
    OwnedSketchSet set;
};

}  // namespace

int main(int argc, char* argv[]) {
    Options o;
    std::vector<Flag> flags = {
        path_flag("--db", &o.db_folder, kUsage),
        path_flag("--output", &o.output, kUsage),
        number_flag("--min_jaccard", &o.min_jaccard, in_open_unit, "--min_jaccard takes a number in the open range (0,1)", kRefuse),
        word_flag("--order", &o.by_index, {{"norm", false}, {"index", true}}, "--order takes norm or index"),
        device_flag(&o.device),
    };
    const Args args = parse_flags(argc, argv, flags);
    if (const int rc = args.exit_code(kProg, print_usage, argv[0]); rc >= 0) return rc;
    SketchDb sdb;
    if (const int rc = open_sketch_db(o.db_folder, sdb)) return rc;
    const DbInfo& db = sdb.info;
    const int64_t n = sdb.n;
    const int dimension = sdb.dimension;

    std::vector<int32_t> rep_of((size_t)n), link_dot((size_t)n), link_q((size_t)n), sizes((size_t)n);
    int64_t n_reps = 0;
    if (n > 0) {
        Gpu g;
        if (mvs_ctx_create(choose_device(o.device), &g.ctx) != MVS_OK) return gpu_fail(kProg, "creating context");
        if (const int rc = load_sketch_db(kProg, g.ctx, sdb, &g.set)) return rc;
        std::vector<int32_t> index_order;
        if (o.by_index) {
            index_order.resize((size_t)n);
            for (int64_t i = 0; i < n; ++i) index_order[(size_t)i] = (int32_t)i;
        }
        if (mvs_dereplicate(g.ctx, g.set, db.norms_sq.data(), MVS_MEM_HOST, o.min_jaccard, o.by_index ? index_order.data() : nullptr,
                            rep_of.data(), link_dot.data(), link_q.data(), sizes.data(), MVS_MEM_HOST, &n_reps) != MVS_OK)
            return gpu_fail(kProg, "dereplicating");
    }
    int64_t singletons = 0, largest = 0;
    for (int64_t i = 0; i < n; ++i) {
        singletons += sizes[(size_t)i] == 1;
        largest = std::max<int64_t>(largest, sizes[(size_t)i]);
    }
    std::ostringstream text;
    text << "#sample\trepresentative\tjaccard\tsize\n";
    char buf[64];
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = rep_of[(size_t)i];
        double j = 1.0;
        if (r != (int32_t)i) {                                                    // the estimate before its clamp, as --top_k scores it
            const double inter = (double)link_dot[(size_t)i] / (double)dimension;
            j = inter / (db.norms_sq[(size_t)i] + db.norms_sq[(size_t)r] - inter);
        }
        snprintf(buf, sizeof(buf), "%.9g", j);
        text << db.names[(size_t)i] << '\t' << db.names[(size_t)r] << '\t' << buf << '\t' << sizes[(size_t)r] << '\n';
    }
    if (const int rc = write_then_rename(kProg, o.output, text.str())) return rc;
    std::cout << "Dereplicated " << n << " samples at Jaccard > " << o.min_jaccard << ": " << n_reps << " representatives, " << singletons
              << " singletons, largest " << largest << std::endl;
    return 0;
}
