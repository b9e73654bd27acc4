// mvs_host.hpp -- host-side pieces shared by the drop-in executables: the reference's text/binary
// formats on both sides of the hot path.  Everything numeric is done by libmvs_hip.so (include/mvs_hip.h).
//   mvs_hash_text.hpp  hash text -> CSR: the parsers, read_hash_file, the .csr cache, load_hash_sets
//   mvs_shard.hpp      matrix shard folders: the row encoder, both writers, the reader, the legacy int16 format
//   here               the DB folder's text (format_g*, norm_*, DbInfo, read_norms) and pick_device
//
// Citations are relative to the reference root.
#ifndef MVS_HOST_HPP
#define MVS_HOST_HPP

#include "mvs_hash_text.hpp"
#include "mvs_shard.hpp"

namespace mvs_host {

// ---------------------------------------------------------------------------------------------------
// DB folder (src/project_everything.cpp:306-361 writes it, src/pairwise_comp_optimized.cpp:852-914 reads it)
// ---------------------------------------------------------------------------------------------------
// `os << double` with default precision / flags == "%g"
inline std::string format_g(double v) {
    char b[64];
    snprintf(b, sizeof b, "%g", v);
    return b;
}
// `os << float` likewise (src/standalone_projection.cpp:40)
inline std::string format_g_float(float v) { return format_g((double)v); }

// norm of one sketch: the reference takes the float32 path (cast / sqrt(float d), Eigen norm) whose
// last digit is not reproducible; this build defines it as sqrt(double(sumsq) / d).
inline double norm_from_sumsq(int64_t sumsq, int d) { return std::sqrt((double)sumsq / (double)d); }
// the float32 evaluation of src/project_everything.cpp:328-329, summed in index order
inline float norm_float32_path(const int32_t* v, int d) {
    const float root = std::sqrt((float)d);
    float acc = 0.0f;
    for (int k = 0; k < d; ++k) {
        const float f = (float)v[k] / root;
        acc += f * f;
    }
    return std::sqrt(acc);
}

struct DbInfo {
    std::string dtype = "int32";
    int dimension = 0;
    int64_t total_vectors = 0;
    std::vector<std::string> names;
    std::vector<double> norms_sq;   // stod(text)^2, src/pairwise_comp_optimized.cpp:893-901
};

inline bool read_norms(const std::string& norms_file, DbInfo& db) {
    std::ifstream in(norms_file);
    if (!in) return false;
    std::string line;
    while (std::getline(in, line)) {
        const size_t pos = line.find(' ');
        if (pos == std::string::npos) continue;
        const double norm = std::stod(line.substr(pos + 1));
        db.names.push_back(line.substr(0, pos));
        db.norms_sq.push_back(norm * norm);
    }
    return true;
}

inline int pick_device() {
    const char* e = getenv("MVS_DEVICE");
    return e ? atoi(e) : 0;
}

}  // namespace mvs_host

#endif
