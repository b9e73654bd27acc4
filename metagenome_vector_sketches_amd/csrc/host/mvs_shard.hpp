// mvs_shard.hpp -- matrix shard folders: the row encoder, the two writers of the active format (write_shard from a cell
// list, ShardWriter piece by piece), its reader, and the legacy int16 format with the zstd binding.  No device is needed.
//
// Citations are relative to the reference root.
#ifndef MVS_SHARD_HPP
#define MVS_SHARD_HPP

#include <cmath>
#include <condition_variable>
#include <deque>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <utility>

#include <dlfcn.h>

#include "../../../include/mvs_hip.h"
#include "mvs_codec.hpp"
#include "mvs_hash_text.hpp"       // pwrite_all, run_threads, and the headers both need

namespace mvs_host {

// ---------------------------------------------------------------------------------------------------
// matrix shard folder, active format (writer src/pairwise_comp_optimized.cpp:645-817)
// ---------------------------------------------------------------------------------------------------
struct ShardStats {
    uint64_t jac_space = 0, ngh_space = 0, rows = 0;
};

// A contiguous run of rows, encoded by one thread: the rows' records back to back, and per row its id, where its record
// starts in `bytes` and its first column -- the directory entries, rebased to the file by append_parts()
struct ShardPart {
    std::string bytes;
    std::vector<uint32_t> row, first_col;
    std::vector<uint64_t> pos;
    uint64_t jac_space = 0, ngh_space = 0;
};

// The two row sources of encode_rows(): row r has the id id(r) and the cells [begin(r), end(r)) -- at least one --, cell i
// the column col(i) and the value q(i).
// write_shard's: runs of an array of mvs_cell, row r being cells[row_first[r] .. row_first[r + 1])
struct CellRunRows {
    const mvs_cell* cells;
    const size_t* row_first;
    uint32_t id(size_t r) const { return (uint32_t)cells[row_first[r]].row; }
    size_t begin(size_t r) const { return row_first[r]; }
    size_t end(size_t r) const { return row_first[r + 1]; }
    int32_t col(size_t i) const { return cells[i].col; }
    uint16_t q(size_t i) const { return (uint16_t)cells[i].q; }
};
// ShardWriter::add's: the rows live[r] of a CSR piece, whose values are 8 bit (q) or 16 bit (q16)
struct CsrPieceRows {
    const mvs_row_block* b;
    const int64_t* live;
    uint32_t id(size_t r) const { return (uint32_t)(b->row_begin + live[r]); }
    size_t begin(size_t r) const { return (size_t)b->row_ptr[live[r]]; }
    size_t end(size_t r) const { return (size_t)b->row_ptr[live[r] + 1]; }
    int32_t col(size_t i) const { return b->col[i]; }
    uint16_t q(size_t i) const { return b->q ? (uint16_t)b->q[i] : b->q16[i]; }
};

// The row encoder: rows [r0, r1) of `rows` into `part`, each as compact_vector(q) followed, when it has more than one
// cell, by rice_sequence(column deltas) (src/pairwise_comp_optimized.cpp:718-736)
template <class Rows>
inline void encode_rows(ShardPart& part, size_t r0, size_t r1, const Rows& rows) {
    std::ostringstream os(std::ios::binary);
    std::vector<uint16_t> jac;
    std::vector<uint64_t> delta;
    for (size_t r = r0; r < r1; ++r) {
        const size_t i = rows.begin(r), n = rows.end(r) - i;
        part.row.push_back(rows.id(r));
        part.pos.push_back((uint64_t)os.tellp());
        part.first_col.push_back((uint32_t)rows.col(i));
        jac.resize(n);
        delta.resize(n - 1);
        for (size_t k = 0; k < n; ++k) {
            jac[k] = rows.q(i + k);
            if (k > 0) {
                if (rows.col(i + k) <= rows.col(i + k - 1)) throw std::runtime_error("columns not ascending");
                delta[k - 1] = (uint64_t)(rows.col(i + k) - rows.col(i + k - 1));
            }
        }
        mvs_codec::compact_vector cv_jc;
        cv_jc.build(jac.begin(), jac.size());
        cv_jc.save(os);
        part.jac_space += cv_jc.num_bytes();
        if (jac.size() > 1) {                     // :732 a single-entry row has no delta sequence
            mvs_codec::rice_sequence rs_delta;
            rs_delta.encode(delta.begin(), delta.size());
            rs_delta.save(os);
            part.ngh_space += rs_delta.num_bytes();
        }
    }
    part.bytes = os.str();
}

// Part t = rows [cut[t], cut[t + 1]), every part on a thread of its own.  What an encoder throws reaches the caller as a
// runtime_error that starts with `who` (the lowest-numbered failing part's).
template <class Rows>
inline std::vector<ShardPart> encode_parts(const char* who, const std::vector<size_t>& cut, const Rows& rows) {
    std::vector<ShardPart> parts(cut.size() - 1);
    try {
        run_threads((unsigned)parts.size(), [&](unsigned t) { encode_rows(parts[t], cut[t], cut[t + 1], rows); });
    } catch (const std::exception& e) {
        throw std::runtime_error(std::string(who) + ": " + e.what());
    } catch (...) {
        throw std::runtime_error(std::string(who) + ": unknown error in an encoder thread");
    }
    return parts;
}

// The parts in order, the first starting at file_pos: their directory entries are rebased from the part to the file and
// appended to the three vectors, their space counts added to `st`, and put(at, bytes) gets each part's bytes.  Returns the
// file position behind the last part.
template <class Put>
inline uint64_t append_parts(std::vector<ShardPart>& parts, uint64_t file_pos, std::vector<uint32_t>& row_vec,
                             std::vector<uint64_t>& curr_pos, std::vector<uint32_t>& start_neighbor, ShardStats& st, Put&& put) {
    for (ShardPart& part : parts) {
        row_vec.insert(row_vec.end(), part.row.begin(), part.row.end());
        start_neighbor.insert(start_neighbor.end(), part.first_col.begin(), part.first_col.end());
        for (const uint64_t p : part.pos) curr_pos.push_back(file_pos + p);
        st.jac_space += part.jac_space;
        st.ngh_space += part.ngh_space;
        const uint64_t at = file_pos;
        file_pos += part.bytes.size();
        put(at, std::move(part.bytes));
    }
    return file_pos;
}

// row_index.bin -- row ids, then byte-offset deltas between consecutive rows (:769-783) -- and neighbor_start.bin, the
// rows' first columns.  Returns the bytes of the latter's sequence, and whether both files were written.
inline std::pair<uint64_t, bool> write_shard_directory(const std::string& index_path, const std::string& start_path,
                                                       const std::vector<uint32_t>& row_vec, const std::vector<uint64_t>& curr_pos,
                                                       const std::vector<uint32_t>& start_neighbor) {
    std::ofstream index_out(index_path, std::ios::binary);
    mvs_codec::compact_vector cv_rows;
    cv_rows.build(row_vec.begin(), row_vec.size());
    cv_rows.save(index_out);
    std::vector<uint64_t> pos_delta(curr_pos.empty() ? 0 : curr_pos.size() - 1);
    for (size_t k = 1; k < curr_pos.size(); ++k) pos_delta[k - 1] = curr_pos[k] - curr_pos[k - 1];
    mvs_codec::compact_vector cv_cps;
    cv_cps.build(pos_delta.begin(), pos_delta.size());
    cv_cps.save(index_out);
    index_out.close();
    std::ofstream ngh_out(start_path, std::ios::binary);
    mvs_codec::rice_sequence rs_start;
    rs_start.encode(start_neighbor.begin(), start_neighbor.size());
    rs_start.save(ngh_out);
    ngh_out.close();
    return {rs_start.num_bytes(), index_out && ngh_out};
}

// cells must be grouped by row with ascending columns inside a row (mvs_pairwise_rows order).
// threads: 0 = all host threads (rows are encoded independently).
// Rows are written in ascending order (the reference iterates a std::unordered_map, i.e. in an
// unspecified order; its reader builds a map and accepts any order).
inline ShardStats write_shard(const std::string& folder, const mvs_cell* cells, size_t n_cells,
                              unsigned threads = 0) {
    if (!fs::exists(folder)) fs::create_directories(folder);
    std::ofstream bin_out(folder + "matrix.bin", std::ios::binary);
    // row table (first cell of every row), then the rows are encoded by workers, each a contiguous run of
    // rows into its own buffer; the buffers are written out in order, so the file is the one a single
    // thread would write
    std::vector<size_t> row_first;
    for (size_t i = 0; i < n_cells; ++i)
        if (i == 0 || cells[i].row != cells[i - 1].row) row_first.push_back(i);
    const size_t n_rows = row_first.size();
    row_first.push_back(n_cells);
    if (threads == 0) threads = std::max(1u, std::thread::hardware_concurrency());
    threads = (unsigned)std::min<size_t>(threads, std::max<size_t>(1, n_rows / 4096));
    threads = std::max(1u, threads);
    std::vector<size_t> cut(threads + 1);
    for (unsigned t = 0; t <= threads; ++t) cut[t] = n_rows * t / threads;
    std::vector<ShardPart> parts = encode_parts("write_shard", cut, CellRunRows{cells, row_first.data()});
    ShardStats st;
    std::vector<uint32_t> row_vec, start_neighbor;
    std::vector<uint64_t> curr_pos_vec;
    append_parts(parts, 0, row_vec, curr_pos_vec, start_neighbor, st,
                 [&](uint64_t, std::string&& bytes) { bin_out.write(bytes.data(), (std::streamsize)bytes.size()); });
    bin_out.close();
    st.rows = row_vec.size();
    const auto [start_bytes, written] = write_shard_directory(folder + "row_index.bin", folder + "neighbor_start.bin", row_vec, curr_pos_vec, start_neighbor);
    if (!written) throw std::runtime_error("write_shard: writing the index files of " + folder + " failed");
    st.ngh_space += start_bytes;
    return st;
}

// The same shard written piece by piece: add() takes CSR pieces of consecutive whole rows in ascending row order
// (mvs_row_block, what mvs_pairwise_stream delivers) and appends their rows to matrix.bin at once; only the per-row
// directory (row id, byte offset, first column) stays in memory until finish() writes row_index.bin and
// neighbor_start.bin.  The files are byte for byte what write_shard() writes for the same cells.
class ShardWriter {
public:
    // The three files are written under ".part" names and renamed in finish(): a comparison that fails half way (out of
    // memory, a device error, an aborted callback) leaves a shard that was there before untouched, as the reference does --
    // it only opens its output once all results exist (src/pairwise_comp_optimized.cpp:645-817 runs after the tile loop).
    explicit ShardWriter(const std::string& folder, unsigned threads = 0) : folder_(folder), threads_(threads) {
        if (!fs::exists(folder_)) fs::create_directories(folder_);
        bin_fd_ = ::open((folder_ + "matrix.bin.part").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (bin_fd_ < 0) throw std::runtime_error("ShardWriter: cannot create " + folder_ + "matrix.bin.part");
        if (threads_ == 0) threads_ = std::max(1u, std::thread::hardware_concurrency());
        // matrix.bin is written by a few threads of its own (pwrite at the position every run of bytes is known to have):
        // the encoded rows of a piece go to the file while the next piece is being encoded or downloaded, and one thread
        // copying into the page cache would be what bounds a dense shard (1.4 GB at ~3 GB/s)
        try {
            spawn_file_threads();
        } catch (...) {                    // a thread that could not start: the ones that did must not outlive the object
            stop_file_threads();
            ::close(bin_fd_);
            ::unlink((folder_ + "matrix.bin.part").c_str());
            throw;
        }
    }
    ShardWriter(const ShardWriter&) = delete;
    ShardWriter& operator=(const ShardWriter&) = delete;
    ~ShardWriter() {
        stop_file_threads();
        if (bin_fd_ >= 0) ::close(bin_fd_);
        if (!finished_)                    // finish() did not complete: nothing half-written stays behind
            for (const char* f : {"matrix.bin.part", "row_index.bin.part", "neighbor_start.bin.part"}) ::unlink((folder_ + f).c_str());
    }

private:
    void spawn_file_threads() {
        for (int t = 0; t < 4; ++t)
            file_threads_.emplace_back([this] {
                for (;;) {
                    Job job;
                    {
                        std::unique_lock<std::mutex> lk(mu_);
                        cv_.wait(lk, [this] { return closing_ || !pending_.empty(); });
                        if (pending_.empty()) return;
                        job = std::move(pending_.front());
                        pending_.pop_front();
                    }
                    cv_.notify_all();
                    if (!pwrite_all(bin_fd_, job.bytes.data(), job.bytes.size(), job.pos)) {
                        std::lock_guard<std::mutex> lk(mu_);
                        write_failed_ = true;
                    }
                }
            });
    }

public:
    void add(const mvs_row_block& b) {
        const int64_t rows = b.row_end - b.row_begin;
        if (rows < 0 || b.row_begin < next_row_) throw std::runtime_error("ShardWriter: pieces must come in ascending row order");
        next_row_ = b.row_end;
        cells_ += (uint64_t)b.n_cells;
        std::vector<int64_t> live;                                  // rows of the piece that hold cells
        for (int64_t r = 0; r < rows; ++r)
            if (b.row_ptr[r + 1] > b.row_ptr[r]) live.push_back(r);
        const size_t n_rows = live.size();
        if (n_rows == 0) return;
        // encoder threads by the piece's CELLS (a dense piece is a few hundred rows of ten thousand cells each), every
        // thread a contiguous run of rows holding about the same number of cells
        unsigned threads = (unsigned)std::min<size_t>(threads_, std::max<size_t>(1, (size_t)b.n_cells / 32768));
        threads = (unsigned)std::min<size_t>(std::max(1u, threads), n_rows);
        std::vector<size_t> cut(threads + 1, n_rows);
        cut[0] = 0;
        for (unsigned t = 1; t < threads; ++t) {
            const int64_t target = b.n_cells / threads * t;
            size_t lo = cut[t - 1], hi = n_rows;
            while (lo < hi) {                                       // first live row whose first cell is at or past the target
                const size_t mid = (lo + hi) / 2;
                if (b.row_ptr[live[mid]] < target) lo = mid + 1;
                else hi = mid;
            }
            cut[t] = lo;
        }
        std::vector<ShardPart> parts = encode_parts("ShardWriter", cut, CsrPieceRows{&b, live.data()});
        pos_ = append_parts(parts, pos_, row_vec_, curr_pos_vec_, start_neighbor_, stats_,
                            [this](uint64_t at, std::string&& bytes) { enqueue(at, std::move(bytes)); });
    }

    // The same for a piece whose rows the device has already encoded (mvs_pairwise_stream_encoded): the records go to the
    // file as they are, the directory entries are rebased to the file position.
    void add_encoded(const mvs_encoded_rows& b) {
        if (b.row_begin < next_row_) throw std::runtime_error("ShardWriter: pieces must come in ascending row order");
        next_row_ = b.row_end;
        cells_ += (uint64_t)b.n_cells;
        if (b.n_rows == 0) return;
        uint64_t jac = 0;
        for (int64_t r = 0; r < b.n_rows; ++r) {
            row_vec_.push_back(b.rows[r]);
            start_neighbor_.push_back(b.first_col[r]);
            curr_pos_vec_.push_back(pos_ + b.offset[r]);
            jac += b.jac_bytes[r];
        }
        stats_.jac_space += jac;
        stats_.ngh_space += (uint64_t)b.n_bytes - jac;
        // the pinned buffer is only valid during the call: the piece is copied once, in a few runs so that the file threads
        // share it
        const uint64_t at = pos_;
        pos_ += (uint64_t)b.n_bytes;
        const size_t run = 8u << 20;
        for (size_t o = 0; o < (size_t)b.n_bytes; o += run)
            enqueue(at + o, std::string(reinterpret_cast<const char*>(b.bytes) + o, std::min(run, (size_t)b.n_bytes - o)));
    }

    uint64_t cells() const { return cells_; }

    ShardStats finish() {
        stop_file_threads();
        if (bin_fd_ >= 0) ::close(bin_fd_);
        bin_fd_ = -1;
        if (write_failed_) throw std::runtime_error("ShardWriter: writing " + folder_ + "matrix.bin failed");
        stats_.rows = row_vec_.size();
        const auto [start_bytes, written] =
            write_shard_directory(folder_ + "row_index.bin.part", folder_ + "neighbor_start.bin.part", row_vec_, curr_pos_vec_, start_neighbor_);
        if (!written) throw std::runtime_error("ShardWriter: writing the index files of " + folder_ + " failed");
        stats_.ngh_space += start_bytes;
        for (const char* f : {"matrix.bin", "row_index.bin", "neighbor_start.bin"})
            if (::rename((folder_ + f + ".part").c_str(), (folder_ + f).c_str()) != 0)
                throw std::runtime_error("ShardWriter: cannot rename " + folder_ + f + ".part");
        finished_ = true;
        return stats_;
    }

private:
    struct Job {
        uint64_t pos = 0;
        std::string bytes;
    };
    void enqueue(uint64_t pos, std::string&& bytes) {
        if (bytes.empty()) return;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [this] { return pending_.size() < 64; });
            pending_.push_back(Job{pos, std::move(bytes)});
        }
        cv_.notify_all();
    }
    void stop_file_threads() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            closing_ = true;
        }
        cv_.notify_all();
        for (auto& th : file_threads_)
            if (th.joinable()) th.join();
    }
    std::string folder_;
    unsigned threads_;
    int bin_fd_ = -1;
    std::vector<std::thread> file_threads_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Job> pending_;
    bool closing_ = false, write_failed_ = false, finished_ = false;
    uint64_t pos_ = 0, cells_ = 0;
    int64_t next_row_ = 0;
    std::vector<uint32_t> row_vec_, start_neighbor_;
    std::vector<uint64_t> curr_pos_vec_;
    ShardStats stats_;
};

// decode a shard folder back into (row, col, q) triples in file order -- what the reader's
// load_neighbors_for_rows_jaccard_wo_sort (src/read_pc_mat_cmp.cpp:597-671) reconstructs
inline bool read_shard(const std::string& folder, std::vector<mvs_cell>& out) {
    std::ifstream index_in(folder + "row_index.bin", std::ios::binary);
    std::ifstream bin_in(folder + "matrix.bin", std::ios::binary);
    std::ifstream ngh_in(folder + "neighbor_start.bin", std::ios::binary);
    if (!index_in || !bin_in || !ngh_in) return false;
    mvs_codec::compact_vector cv_rows, cv_cps;
    cv_rows.load(index_in);
    cv_cps.load(index_in);
    mvs_codec::rice_sequence rs_start;
    rs_start.load(ngh_in);
    uint64_t addr = 0;
    for (uint64_t r = 0; r < cv_rows.size(); ++r) {
        if (r > 0) addr += cv_cps.access(r - 1);
        bin_in.seekg((std::streamoff)addr);
        mvs_codec::compact_vector jac;
        jac.load(bin_in);
        std::vector<uint64_t> delta;
        if (jac.size() > 1) {
            mvs_codec::rice_sequence rs;
            rs.load(bin_in);
            rs.decode(delta);
        }
        uint64_t col = rs_start.access(r);
        for (uint64_t k = 0; k < jac.size(); ++k) {
            if (k > 0) col += delta[k - 1];
            mvs_cell c;
            c.row = (int32_t)cv_rows.access(r);
            c.col = (int32_t)col;
            c.dot = 0;
            c.q = (int32_t)jac.access(k);
            out.push_back(c);
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------
// legacy int16 shard format (writer src/pairwise_comp_optimized_16bits.cpp:251-323; the reference has no reader
// for it).  matrix.bin: per row elias_fano(cols, universe = last col + 1) then compact_vector(round(dot / d));
// row_index.bin: compact_vector(rows) + compact_vector(byte offset of each row in matrix.bin); both files are
// then compressed with zstd and the originals removed (:317-322, `system("zstd -f ...")`).  zstd is bound at run
// time (libzstd.so.1); where it is missing the uncompressed files stay, which is also what the reference's
// `zstd -f x && rm -f x` leaves behind when the command fails.
// ---------------------------------------------------------------------------------------------------
struct Zstd {
    size_t (*bound)(size_t) = nullptr;
    size_t (*compress)(void*, size_t, const void*, size_t, int) = nullptr;
    size_t (*decompress)(void*, size_t, const void*, size_t) = nullptr;
    unsigned long long (*content_size)(const void*, size_t) = nullptr;
    unsigned (*is_error)(size_t) = nullptr;
    bool ok = false;
    Zstd() {
        void* h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libzstd.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        bound = reinterpret_cast<decltype(bound)>(dlsym(h, "ZSTD_compressBound"));
        compress = reinterpret_cast<decltype(compress)>(dlsym(h, "ZSTD_compress"));
        decompress = reinterpret_cast<decltype(decompress)>(dlsym(h, "ZSTD_decompress"));
        content_size = reinterpret_cast<decltype(content_size)>(dlsym(h, "ZSTD_getFrameContentSize"));
        is_error = reinterpret_cast<decltype(is_error)>(dlsym(h, "ZSTD_isError"));
        ok = bound && compress && decompress && content_size && is_error;
    }
    static const Zstd& get() {
        static Zstd z;
        return z;
    }
};

inline bool read_whole_file(const std::string& path, std::string& bytes) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    bytes.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    return true;
}

// `zstd -f path && rm -f path` (level 3, the tool's default)
inline bool zstd_file_and_remove(const std::string& path) {
    const Zstd& z = Zstd::get();
    std::string raw;
    if (!z.ok || !read_whole_file(path, raw)) return false;
    std::string out(z.bound(raw.size()), '\0');
    const size_t n = z.compress(&out[0], out.size(), raw.data(), raw.size(), 3);
    if (z.is_error(n)) return false;
    std::ofstream os(path + ".zst", std::ios::binary);
    os.write(out.data(), (std::streamsize)n);
    os.close();
    if (!os) return false;
    fs::remove(path);
    return true;
}

// contents of path, or of path.zst when only that exists
inline bool read_maybe_zstd(const std::string& path, std::string& bytes) {
    if (read_whole_file(path, bytes)) return true;
    std::string packed;
    const Zstd& z = Zstd::get();
    if (!z.ok || !read_whole_file(path + ".zst", packed)) return false;
    const unsigned long long n = z.content_size(packed.data(), packed.size());
    if (n > (1ULL << 40)) return false;                       // unknown / error sentinel values are huge
    bytes.assign((size_t)n, '\0');
    const size_t got = z.decompress(&bytes[0], bytes.size(), packed.data(), packed.size());
    return !z.is_error(got) && got == n;
}

// cells grouped by row with ascending columns (mvs_pairwise_rows order); returns the number of rows written
inline uint64_t write_shard_legacy16(const std::string& folder, const mvs_cell* cells, size_t n_cells, int dimension) {
    if (!fs::exists(folder)) fs::create_directories(folder);
    const std::string bin_filename = folder + "matrix.bin", index_filename = folder + "row_index.bin";
    std::ofstream bin_out(bin_filename, std::ios::binary);
    std::ofstream index_out(index_filename, std::ios::binary);
    std::vector<int32_t> row_vec;
    std::vector<int64_t> curr_pos_vec;
    int64_t current_pos = 0;
    for (size_t i = 0; i < n_cells;) {
        size_t j = i;
        while (j < n_cells && cells[j].row == cells[i].row) ++j;
        std::vector<int32_t> cols(j - i);
        std::vector<int64_t> vals(j - i);
        for (size_t k = i; k < j; ++k) {
            cols[k - i] = cells[k].col;
            vals[k - i] = (int64_t)std::round((double)cells[k].dot / (double)dimension);        // :274-279
        }
        row_vec.push_back(cells[i].row);
        curr_pos_vec.push_back(current_pos);
        mvs_codec::elias_fano ef;
        ef.encode(cols.begin(), cols.size(), (uint64_t)cols.back() + 1);                      // :294-296
        ef.save(bin_out);
        current_pos += (int64_t)ef.num_bytes();
        mvs_codec::compact_vector cv;
        cv.build(vals.begin(), vals.size());                                                   // :299-302
        cv.save(bin_out);
        current_pos += (int64_t)cv.num_bytes();
        i = j;
    }
    bin_out.close();
    mvs_codec::compact_vector cv_rows, cv_pos;
    cv_rows.build(row_vec.begin(), row_vec.size());
    cv_rows.save(index_out);
    cv_pos.build(curr_pos_vec.begin(), curr_pos_vec.size());
    cv_pos.save(index_out);
    index_out.close();
    if (!zstd_file_and_remove(bin_filename) || !zstd_file_and_remove(index_filename))
        std::cerr << "zstd not available: " << bin_filename << " / " << index_filename << " left uncompressed" << std::endl;
    return row_vec.size();
}

// decode the legacy int16 shard back into (row, col, value = round(dot / d)) triples (value in mvs_cell::dot, q = 0)
inline bool read_shard_legacy16(const std::string& folder, std::vector<mvs_cell>& out) {
    std::string bin, index;
    if (!read_maybe_zstd(folder + "matrix.bin", bin) || !read_maybe_zstd(folder + "row_index.bin", index)) return false;
    std::istringstream index_in(index, std::ios::binary), bin_in(bin, std::ios::binary);
    mvs_codec::compact_vector cv_rows, cv_pos;
    cv_rows.load(index_in);
    cv_pos.load(index_in);
    for (uint64_t r = 0; r < cv_rows.size(); ++r) {
        bin_in.seekg((std::streamoff)cv_pos.access(r));
        mvs_codec::elias_fano ef;
        ef.load(bin_in);
        mvs_codec::compact_vector cv;
        cv.load(bin_in);
        if (ef.size() != cv.size()) throw std::runtime_error("legacy shard: row lengths disagree");
        std::vector<uint64_t> cols;
        ef.decode(cols);
        for (uint64_t k = 0; k < cols.size(); ++k) {
            mvs_cell c;
            c.row = (int32_t)cv_rows.access(r);
            c.col = (int32_t)cols[k];
            c.dot = (int32_t)cv.access(k);
            c.q = 0;
            out.push_back(c);
        }
    }
    return true;
}

}  // namespace mvs_host

#endif
