// mvs_hash_text.hpp -- hash text files ("name: h1 h2 ...") into CSR sets: the token parsers, read_hash_file() and its
// steps, the binary .csr cache beside the text, and load_hash_sets(), the tools' one way to either.  No device is needed.
// pwrite_all() and run_threads() are here too; mvs_shard.hpp uses them as well.
//
// Citations are relative to the reference root.
#ifndef MVS_HASH_TEXT_HPP
#define MVS_HASH_TEXT_HPP

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <filesystem>
#include <iostream>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <cerrno>
#include <csignal>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace mvs_host {

namespace fs = std::filesystem;

// n bytes from p to the file at offset off, in calls of at most 1 GiB; false at the first call that writes nothing
inline bool pwrite_all(int fd, const char* p, size_t n, uint64_t off) {
    while (n) {
        const ssize_t w = ::pwrite(fd, p, std::min<size_t>(n, (size_t)1 << 30), (off_t)off);
        if (w <= 0) return false;
        p += w;
        n -= (size_t)w;
        off += (uint64_t)w;
    }
    return true;
}

// body(t) for t = 0 .. n-1 on n threads (n == 1: on the caller's).  All of them are joined before this returns, and what a
// body throws (the codec's runtime_error, bad_alloc) is thrown to the caller instead of ending the process in
// std::terminate: the exception of the lowest t that failed.
template <class Body>
inline void run_threads(unsigned n, Body&& body) {
    n = std::max(1u, n);
    std::vector<std::exception_ptr> errors(n);
    auto guarded = [&](unsigned t) {
        try {
            body(t);
        } catch (...) {
            errors[t] = std::current_exception();
        }
    };
    if (n == 1) {
        guarded(0);
    } else {
        std::vector<std::thread> pool;
        try {
            for (unsigned t = 0; t < n; ++t) pool.emplace_back(guarded, t);
        } catch (...) {                                       // a thread that could not start: the ones that did are joined
            for (auto& th : pool) th.join();
            throw;
        }
        for (auto& th : pool) th.join();
    }
    for (const std::exception_ptr& e : errors)
        if (e) std::rethrow_exception(e);
}

// ---------------------------------------------------------------------------------------------------
// hash text -> CSR
// ---------------------------------------------------------------------------------------------------
// Flat uint64 storage that is filled by the parser's workers (a std::vector would value-initialise
// gigabytes on one thread first).
struct HashBuffer {
    uint64_t* p = nullptr;
    size_t n = 0;
    void* map_base = nullptr;        // non-NULL: p points into a read-only file mapping of map_len bytes (the CSR cache)
    size_t map_len = 0;
    HashBuffer() = default;
    HashBuffer(const HashBuffer&) = delete;
    HashBuffer& operator=(const HashBuffer&) = delete;
    ~HashBuffer() { release(); }
    void release() {
        if (map_base) ::munmap(map_base, map_len);
        else free(p);
        p = nullptr;
        map_base = nullptr;
        n = map_len = 0;
    }
    bool reset(size_t count) {
        release();
        p = (uint64_t*)malloc(std::max<size_t>(8, count * sizeof(uint64_t)));
        n = p ? count : 0;
        return p != nullptr;
    }
    void adopt_mapping(void* base, size_t len, const uint64_t* first, size_t count) {
        release();
        map_base = base;
        map_len = len;
        p = const_cast<uint64_t*>(first);
        n = count;
    }
    const uint64_t* data() const { return p; }
    uint64_t* data() { return p; }
    size_t size() const { return n; }
    uint64_t operator[](size_t i) const { return p[i]; }
};

struct HashSets {
    std::vector<std::string> names;
    HashBuffer hashes;               // concatenated, unique within a sample (sorted)
    std::vector<int64_t> offsets;    // names.size() + 1
};

// ---------------------------------------------------------------------------------------------------
// Binary CSR cache of a hash text file: "<hash_file>.csr" next to it.  Parsing the text is what bounds
// `project_everything sketch` end to end (src/project_everything.cpp:264-281 parses serially; here all host threads
// parse, and it still is 10-100x the device time), so the parsed form -- names, offsets, unique sorted u64 values,
// exactly what read_hash_file() returns -- is kept and mapped on the next run (read_hash_file() writes it while it parses
// when asked to; write_csr_cache() writes one from sets in memory).  The cache is valid only for the
// text file it was made from (size and modification time are recorded); anything else falls back to the text.
//   header (64 B): magic "MVSCSR01", u64 text size, i64 text mtime (ns), u64 samples, u64 values, u64 name bytes
//   i64 offsets[samples + 1], u64 name_ends[samples], names, padding to 8, u64 values[]
// ---------------------------------------------------------------------------------------------------
struct CsrHeader {
    char magic[8];
    uint64_t text_size;
    int64_t text_mtime_ns;
    uint64_t samples, values, name_bytes;
    uint64_t reserved[2];
};
static_assert(sizeof(CsrHeader) == 64, "header layout");

inline std::string csr_cache_path(const std::string& hash_file) { return hash_file + ".csr"; }
// the file a cache is written to before it is renamed into place: one per writing process (two runs on the same hash file
// must not write into each other's file)
inline std::string csr_cache_part_path(const std::string& hash_file) {
    return csr_cache_path(hash_file) + ".part." + std::to_string((long)::getpid());
}

// ".part.<pid>" files next to `hash_file` whose writer no longer exists (a killed run leaves up to the size of the cache
// behind): removed before a new cache is written.  A pid that cannot be probed (another user's process) is left alone.
inline void remove_stale_cache_parts(const std::string& hash_file) {
    namespace fs = std::filesystem;
    std::error_code ec;
    const fs::path cache(csr_cache_path(hash_file));
    const fs::path dir = cache.parent_path().empty() ? fs::path(".") : cache.parent_path();
    const std::string prefix = cache.filename().string() + ".part.";
    for (fs::directory_iterator it(dir, ec), end; !ec && it != end; it.increment(ec)) {
        const std::string name = it->path().filename().string();
        if (name.size() <= prefix.size() || name.compare(0, prefix.size(), prefix) != 0) continue;
        const std::string tail = name.substr(prefix.size());
        if (tail.find_first_not_of("0123456789") != std::string::npos || tail.size() > 10) continue;
        const long pid = std::strtol(tail.c_str(), nullptr, 10);
        if (pid <= 0 || pid == (long)::getpid()) continue;
        if (::kill((pid_t)pid, 0) != 0 && errno == ESRCH) ::unlink(it->path().c_str());
    }
}

inline bool text_identity(const std::string& path, uint64_t& size, int64_t& mtime_ns) {
    struct stat st;
    if (::stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
    size = (uint64_t)st.st_size;
    mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000LL + st.st_mtim.tv_nsec;
    return true;
}

// Sort + unique of one sample's hashes when the text did not have them in strictly increasing order (the reference's
// `convert` writes an unordered_set's iteration order, src/project_everything.cpp:222-228).  The projection needs the
// set, not an order; sorted unique values are what the .csr cache is defined to hold, so the order is kept -- with an LSD
// radix sort on 11-bit digits over the bits that are actually set (FracMinHash values are < 2^64 / scaled: 5 passes),
// ~10 ns per value where std::sort takes 60 (that sort was 70 % of the first `sketch` run's parse stage).
// Returns the number of unique values, which are left sorted at v[0 .. return).
inline size_t sort_unique_u64(uint64_t* v, size_t n) {
    if (n < 256) {
        std::sort(v, v + n);
        return (size_t)(std::unique(v, v + n) - v);
    }
    uint64_t any = 0;
    for (size_t i = 0; i < n; ++i) any |= v[i];
    int bits = 0;
    while (bits < 64 && (any >> bits) != 0) ++bits;
    static thread_local std::vector<uint64_t> tmp;
    static thread_local std::vector<uint32_t> hist;
    tmp.resize(n);
    // LSD passes over the 11-bit digits at the given shifts (ascending); v holds the result
    auto radix = [&](const int* shifts, int passes) {
        hist.assign((size_t)passes * 2048, 0);
        for (size_t i = 0; i < n; ++i)
            for (int ps = 0; ps < passes; ++ps) ++hist[(size_t)ps * 2048 + ((v[i] >> shifts[ps]) & 2047)];
        uint64_t* src = v;
        uint64_t* dst = tmp.data();
        for (int ps = 0; ps < passes; ++ps) {
            uint32_t* h = hist.data() + (size_t)ps * 2048;
            uint32_t run = 0;
            bool one_bucket = false;
            for (int b = 0; b < 2048; ++b) {
                const uint32_t c = h[b];
                one_bucket = one_bucket || c == n;
                h[b] = run;
                run += c;
            }
            if (one_bucket) continue;                          // every value has the same digit here: nothing moves
            const int sh = shifts[ps];
            for (size_t i = 0; i < n; ++i) dst[h[(src[i] >> sh) & 2047]++] = src[i];
            std::swap(src, dst);
        }
        if (src != v) memcpy(v, src, n * sizeof(uint64_t));
    };
    bool sorted = false;
    if (bits > 22 && n < ((size_t)1 << 21)) {
        // Hash values are spread evenly: the top 22 bits alone put fewer than 2^21 of them in order but for a few
        // neighbours, which one insertion sweep settles -- two passes instead of five or six.  A sweep that has to move
        // more than a few places per value (values that crowd together) is given up for the full sort.
        const int top[2] = {bits - 22, bits - 11};
        radix(top, 2);
        size_t moved = 0;
        const size_t budget = 4 * n;
        size_t i = 1;
        for (; i < n && moved <= budget; ++i) {
            const uint64_t x = v[i];
            size_t j = i;
            while (j > 0 && v[j - 1] > x) {
                v[j] = v[j - 1];
                --j;
            }
            v[j] = x;
            moved += i - j;
        }
        sorted = i == n && moved <= budget;
    }
    if (!sorted) {
        int all[6];
        const int passes = std::max(1, (bits + 10) / 11);
        for (int ps = 0; ps < passes; ++ps) all[ps] = 11 * ps;
        radix(all, passes);
    }
    return (size_t)(std::unique(v, v + n) - v);
}

// An upper bound of the number of values parse_u64_raw() extracts from [p, end): every extracted value consumes one whole
// run of decimal digits (an optional sign in front of it), so there are at most as many values as digit runs -- "12-3" is
// two values to `iss >> hash` (12, then -3 modulo 2^64), "1+2+3" three.  Exact for well-formed lines without duplicates.
inline size_t count_token_starts_scalar(const char* p, const char* end) {
    size_t count = 0;
    bool prev_digit = false;
    for (; p < end; ++p) {
        const bool digit = (unsigned)(*p - '0') <= 9u;
        count += (size_t)(digit && !prev_digit);
        prev_digit = digit;
    }
    return count;
}

// Parse whitespace separated unsigned 64-bit integers the way `while (iss >> hash)` does
// (src/project_everything.cpp:275-279, src/standalone_projection.cpp:32-35): stop at the first token
// that is not a number in range.  Values are stored at dst in text order (the caller provides room for
// count_token_starts() of them); `increasing` is cleared when they are not strictly increasing.
inline size_t parse_u64_raw_scalar(const char* p, const char* end, uint64_t* dst, bool& increasing) {
    size_t n = 0;
    uint64_t prev = 0;
    auto push = [&](uint64_t v) {
        increasing = increasing && (n == 0 || v > prev);
        prev = v;
        dst[n++] = v;
    };
    while (true) {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\v' || *p == '\f')) ++p;
        if (p >= end) break;
        // one optional sign; num_get<unsigned long> accepts '-' and negates modulo 2^64 ("-1" reads 2^64 - 1)
        const bool negate = *p == '-';
        if (*p == '+' || *p == '-') ++p;
        if (p >= end || *p < '0' || *p > '9') break;
        // up to 19 digits cannot overflow (10^19 < 2^64): only a 20th digit needs the check
        uint64_t v = 0;
        bool overflow = false;
        const char* q = p;
        const char* lim = end - p > 19 ? p + 19 : end;
        while (q < lim && (unsigned)(*q - '0') <= 9u) v = v * 10 + (uint64_t)(*q++ - '0');
        while (q < end && (unsigned)(*q - '0') <= 9u) {
            const uint64_t dgt = (uint64_t)(*q - '0');
            if (v > (UINT64_MAX - dgt) / 10) overflow = true;
            v = v * 10 + dgt;
            ++q;
        }
        p = q;
        if (overflow) break;                                   // failbit in the reference
        if (negate) v = 0 - v;
        // the extraction stops at the first character that is not a digit and the NEXT one starts right there: "12abc"
        // gives 12 and then fails at 'a', "12-3" gives 12 and then -3 (modulo 2^64), "1+2" gives 1 and 2
        // (tests/golden/ref_parser.json: the reference binaries on such lines)
        push(v);
    }
    return n;
}

#if defined(__x86_64__)
#define MVS_HOST_AVX2 __attribute__((target("avx2,bmi,popcnt")))
MVS_HOST_AVX2 inline size_t count_token_starts_avx2(const char* p, const char* end) {
    size_t count = 0;
    uint32_t carry = 0;                                       // was the byte in front a digit?
    const __m256i below0 = _mm256_set1_epi8('0' - 1), above9 = _mm256_set1_epi8('9' + 1);
    for (; end - p >= 32; p += 32) {
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(p));
        const uint32_t w = (uint32_t)_mm256_movemask_epi8(_mm256_and_si256(_mm256_cmpgt_epi8(c, below0), _mm256_cmpgt_epi8(above9, c)));
        count += (size_t)__builtin_popcount(w & ~((w << 1) | carry));
        carry = w >> 31;
    }
    bool prev_digit = carry != 0;
    for (; p < end; ++p) {
        const bool digit = (unsigned)(*p - '0') <= 9u;
        count += (size_t)(digit && !prev_digit);
        prev_digit = digit;
    }
    return count;
}

// the value of the (up to 16) digits that end at pos: three multiply-adds
MVS_HOST_AVX2 inline uint64_t last_digits16_avx2(const char* pos, size_t len) {
    alignas(16) static const uint8_t keep_tail[32] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                                      255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255};
    __m128i c = _mm_sub_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(pos - 16)), _mm_set1_epi8('0'));
    c = _mm_and_si128(c, _mm_loadu_si128(reinterpret_cast<const __m128i*>(keep_tail + len)));
    const __m128i t1 = _mm_maddubs_epi16(c, _mm_set1_epi16(0x010a));          // bytes (10, 1): pairs of digits -> 0..99
    const __m128i t2 = _mm_madd_epi16(t1, _mm_set1_epi32(0x00010064));        // words (100, 1): -> 0..9999
    const __m128i t3 = _mm_packus_epi32(t2, t2);
    const __m128i t4 = _mm_madd_epi16(t3, _mm_set1_epi32(0x00012710));        // words (10000, 1): -> 0..99999999
    const uint64_t both = (uint64_t)_mm_cvtsi128_si64(t4);
    return (both & 0xffffffffu) * 100000000ull + (both >> 32);
}

// digits [tok, pos) -> value; false: more than 20 digits or a value >= 2^64
MVS_HOST_AVX2 inline bool digits_to_u64_avx2(const char* tok, const char* pos, uint64_t& v) {
    const size_t len = (size_t)(pos - tok);
    if (len <= 16) {
        v = last_digits16_avx2(pos, len);
        return true;
    }
    if (len > 20) return false;
    uint64_t hi = 0;
    for (const char* q = tok; q < pos - 16; ++q) hi = hi * 10 + (uint64_t)(*q - '0');
    const uint64_t lo = last_digits16_avx2(pos, 16);
    if (hi > 1844 || (hi == 1844 && lo > 6744073709551615ull)) return false;
    v = hi * 10000000000000000ull + lo;
    return true;
}

// The common line -- decimal digits and blanks, nothing else, tokens of at most 20 digits in range -- without a
// branch per character: 64 bytes give one bit mask of the non-digits, every set bit ends a token, and a token's last 16
// digits are converted with three multiply-adds (the wider ones, up to four leading digits, by hand).  Returns false
// when the line holds anything else (a sign, a tab, a letter, 21 digits, a value >= 2^64): the caller then parses the
// whole line with parse_u64_raw_scalar(), which defines the behaviour.  The loads reach up to 63 bytes past `end` and 16
// bytes in front of a token: the caller guarantees map_begin + 16 <= p and end + 64 <= map_end.
MVS_HOST_AVX2 inline bool parse_u64_line_avx2(const char* p, const char* end, uint64_t* dst, size_t& n_out, bool& increasing) {
    const __m256i below0 = _mm256_set1_epi8('0' - 1), above9 = _mm256_set1_epi8('9' + 1), blank = _mm256_set1_epi8(' ');
    size_t n = 0;
    uint64_t prev = 0, v = 0;
    bool inc = true;
    const char* tok = p;
    for (const char* b = p; b < end; b += 64) {
        const __m256i c0 = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(b));
        const __m256i c1 = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(b + 32));
        const uint64_t d0 = (uint32_t)_mm256_movemask_epi8(_mm256_and_si256(_mm256_cmpgt_epi8(c0, below0), _mm256_cmpgt_epi8(above9, c0)));
        const uint64_t d1 = (uint32_t)_mm256_movemask_epi8(_mm256_and_si256(_mm256_cmpgt_epi8(c1, below0), _mm256_cmpgt_epi8(above9, c1)));
        const uint64_t s0 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(c0, blank));
        const uint64_t s1 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(c1, blank));
        const size_t len = (size_t)(end - b);
        const uint64_t valid = len >= 64 ? ~0ull : ((1ull << len) - 1);
        uint64_t nd = ~(d0 | (d1 << 32)) & valid;
        if (nd != ((s0 | (s1 << 32)) & valid)) return false;
        if (len < 64) nd |= 1ull << len;                       // the end of the line ends the last token
        while (nd) {
            const char* pos = b + __builtin_ctzll(nd);
            nd &= nd - 1;
            if (pos > tok) {
                if (!digits_to_u64_avx2(tok, pos, v)) return false;
                inc = inc && (n == 0 || v > prev);
                prev = v;
                dst[n++] = v;
            }
            tok = pos + 1;
        }
    }
    if (tok < end) {                                           // a line whose length is a multiple of 64
        if (!digits_to_u64_avx2(tok, end, v)) return false;
        inc = inc && (n == 0 || v > prev);
        dst[n++] = v;
    }
    n_out = n;
    increasing = increasing && inc;
    return true;
}

inline bool host_has_avx2() {
    static const bool yes = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi") && __builtin_cpu_supports("popcnt") &&
                            !getenv("MVS_HOST_NO_SIMD");
    return yes;
}
#else
inline bool host_has_avx2() { return false; }
#endif

inline size_t count_token_starts(const char* p, const char* end) {
#if defined(__x86_64__)
    if (host_has_avx2()) return count_token_starts_avx2(p, end);
#endif
    return count_token_starts_scalar(p, end);
}

// [p, end) -> dst (room for count_token_starts(p, end) values), in text order.  map_begin / map_end: the readable range
// around the line (the vectorised path reads 16 bytes in front of a token and up to 63 bytes past the line).
inline size_t parse_u64_raw(const char* p, const char* end, const char* map_begin, const char* map_end, uint64_t* dst, bool& increasing) {
#if defined(__x86_64__)
    if (host_has_avx2() && p - map_begin >= 16 && map_end - end >= 64) {
        const char* e = end;
        while (e > p && (e[-1] == '\r' || e[-1] == ' ')) --e;             // "\r\n" files; trailing blanks
        size_t n = 0;
        bool inc = increasing;
        if (parse_u64_line_avx2(p, e, dst, n, inc)) {
            increasing = inc;
            return n;
        }
    }
#endif
    return parse_u64_raw_scalar(p, end, dst, increasing);
}

// The sorted unique values of a line, APPENDED to `out` (a line whose values are strictly increasing -- what this
// repository's `convert` writes -- is unique and sorted as it stands and skips the sort).
inline void parse_u64_tokens(const char* p, const char* end, std::vector<uint64_t>& out) {
    const size_t first = out.size();
    out.resize(first + count_token_starts(p, end));
    bool increasing = true;
    size_t n = parse_u64_raw(p, end, p, end, out.data() + first, increasing);     // no slack around a bare string: scalar
    if (!increasing) n = sort_unique_u64(out.data() + first, n);
    out.resize(first + n);
}

inline bool write_csr_cache(const std::string& hash_file, const HashSets& sets, unsigned threads = 0);

// ---- read_hash_file()'s steps ----
// A text file mapped read-only, not copied: hash lists run to gigabytes of text.  An empty file maps to nothing.
class MappedText {
public:
    MappedText() = default;
    MappedText(const MappedText&) = delete;
    MappedText& operator=(const MappedText&) = delete;
    ~MappedText() {
        if (begin_ && size_) ::munmap((void*)begin_, size_);
    }
    // false: not there, not a regular file, or not mappable
    bool open(const std::string& path) {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        bool ok = ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
        if (ok && st.st_size) {
            void* m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            ok = m != MAP_FAILED;
            if (ok) {
                ::madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
                begin_ = (const char*)m;
                size_ = (size_t)st.st_size;
            }
        }
        ::close(fd);
        return ok;
    }
    const char* begin() const { return begin_; }
    size_t size() const { return size_; }
    // the mapping is readable up to the end of its last page (zero filled past the end of the file): parse_u64_raw's slack
    const char* map_end() const {
        const size_t page = (size_t)std::max<long>(4096, sysconf(_SC_PAGESIZE));
        return begin_ ? begin_ + (size_ + page - 1) / page * page : nullptr;
    }

private:
    const char* begin_ = nullptr;
    size_t size_ = 0;
};

// One record of the text: the line [b, e) without its '\n', the values after position `colon`
struct Rec { size_t b, e, colon; };

// The line table.  Each worker scans one slice of the file for '\n' (a slice per 4 MiB, at most `threads`).  std::getline
// yields a final record without '\n' if there is text after the last newline and no extra record for a trailing newline.
// with_names: lines without ':' are skipped (src/project_everything.cpp:267-270); otherwise the values start with the line.
inline std::vector<Rec> line_records(const MappedText& text, bool with_names, unsigned threads) {
    const char* const buf = text.begin();
    const size_t size = text.size();
    const unsigned tl = (unsigned)std::min<size_t>(threads, std::max<size_t>(1, size >> 22));
    std::vector<std::vector<size_t>> nl(tl);
    run_threads(tl, [&](unsigned t) {
        size_t pos = size * t / tl;
        const size_t end = size * (t + 1) / tl;
        while (pos < end) {
            const char* q = (const char*)memchr(buf + pos, '\n', end - pos);
            if (!q) break;
            nl[t].push_back((size_t)(q - buf));
            pos = (size_t)(q - buf) + 1;
        }
    });
    std::vector<Rec> recs;
    size_t pos = 0;
    auto add_line = [&](size_t b, size_t e) {
        if (with_names) {
            const char* c = (const char*)memchr(buf + b, ':', e - b);      // no ':' -> skipped (:267-270)
            if (c) recs.push_back({b, e, (size_t)(c - buf)});
        } else {
            recs.push_back({b, e, b - 1});
        }
    };
    for (unsigned t = 0; t < tl; ++t)
        for (size_t e : nl[t]) {
            add_line(pos, e);
            pos = e + 1;
        }
    if (pos < size) add_line(pos, size);
    return recs;
}

// body(i) for every line i < n, on `threads` threads that draw runs of lines from one counter
template <class Body>
inline void for_lines(size_t n, unsigned threads, Body&& body) {
    std::atomic<size_t> next_line{0};
    const size_t grain = std::max<size_t>(1, n / ((size_t)threads * 32));
    run_threads(threads, [&](unsigned) {
        for (size_t i0 = next_line.fetch_add(grain); i0 < n; i0 = next_line.fetch_add(grain))
            for (size_t i = i0; i < std::min(n, i0 + grain); ++i) body(i);
    });
}

// The head of a cache file for `sets`: header, offsets, name ends, names, padding to 8.  `id` gives the text's identity
// (text_size, text_mtime_ns); the magic and the counts are filled in here.
inline std::string csr_head(const CsrHeader& id, const HashSets& sets) {
    CsrHeader h = id;
    memcpy(h.magic, "MVSCSR01", 8);
    h.samples = sets.names.size();
    h.values = sets.hashes.size();
    std::vector<uint64_t> ends(sets.names.size());
    uint64_t at = 0;
    for (size_t i = 0; i < sets.names.size(); ++i) ends[i] = at += sets.names[i].size();
    h.name_bytes = at;
    std::string head;
    head.reserve(sizeof h + sets.offsets.size() * 8 + ends.size() * 8 + (size_t)at + 8);
    head.append(reinterpret_cast<const char*>(&h), sizeof h);
    head.append(reinterpret_cast<const char*>(sets.offsets.data()), sets.offsets.size() * 8);
    head.append(reinterpret_cast<const char*>(ends.data()), ends.size() * 8);
    for (const std::string& nm : sets.names) head.append(nm);
    if (at % 8) head.append(8 - at % 8, '\0');
    return head;
}

// The cache written WHILE read_hash_file() parses.  A line's values have their final place in the flat array -- and in the
// file -- before the line is parsed (room[], the prefix sums of the first pass's counts), so three writer threads copy
// finished runs of lines into "<text>.csr.part.<pid>" behind the parsers; finish() adds the head and renames the file.
// What holds it together:
//   * a line's value count is published with release (publish) and read by the writers with acquire: whoever sees the
//     count sees the values;
//   * a writer never copies past the first line whose count differs from its room -- from there on every offset would
//     move -- and sets `bad` instead;
//   * nobody reads the flat array while it is compacted: stop_for_compaction() joins the writers first;
//   * a joinable thread is never destroyed: every way out joins the writers, the destructor included;
//   * the job lives on the heap (a shared_ptr) because the finishing thread may outlive read_hash_file(); it reads the
//     caller's `out`, which therefore has to outlive that thread;
//   * every way out without a complete file unlinks the .part;
//   * when a line fell short (or a write failed) the file is written from the finished sets by write_csr_cache().
class CsrCacheJob : public std::enable_shared_from_this<CsrCacheJob> {
public:
    ~CsrCacheJob() { abandon(); }

    // room: n + 1 prefix sums (copied: they are the final offsets when no line falls short); flat: where line i's values
    // go, at room[i].  false: no cache this time (the text's identity, the .part or a thread was not to be had), and
    // nothing is left behind.
    bool start(const std::string& text, const std::vector<int64_t>& room, uint64_t name_bytes, const uint64_t* flat) {
        text_ = text;
        part_ = csr_cache_part_path(text);
        remove_stale_cache_parts(text);
        if (!text_identity(text, id_.text_size, id_.text_mtime_ns)) return false;
        fd_ = ::open(part_.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd_ < 0) return false;
        n_ = room.size() - 1;
        head_bytes_ = sizeof(CsrHeader) + (n_ + 1) * 8 + n_ * 8 + (size_t)((name_bytes + 7) / 8 * 8);
        flat_ = flat;
        room_ = room;
        got_.reset(new std::atomic<int64_t>[n_ ? n_ : 1]);
        for (size_t i = 0; i < n_; ++i) got_[i].store(-1, std::memory_order_relaxed);
        try {
            for (int t = 0; t < 3; ++t) helpers_.emplace_back(&CsrCacheJob::write_finished_lines, this);
        } catch (const std::exception&) {
            abandon();                                         // no thread to be had: the parse goes on without the cache
            return false;
        }
        return true;
    }

    // line i is parsed: k values stand at flat[room[i]]
    void publish(size_t i, size_t k) { got_[i].store((int64_t)k, std::memory_order_release); }

    // the parse failed, or the job never got going: give up quietly
    void abandon() {
        stop_ = true;
        join_helpers();
        if (fd_ < 0) return;
        ::close(fd_);
        fd_ = -1;
        ::unlink(part_.c_str());
    }

    // a line gave fewer values than its room: the writers have stopped at the first such line at the latest and touch
    // nothing from there on; wait until they are gone
    void stop_for_compaction() {
        bad_ = true;
        join_helpers();
    }

    // The finisher: waits for the writers, then either completes the file (head + rename) or, if a line fell short or a
    // write failed, writes the cache from the finished sets.  It reads *sets until it is joined.
    std::thread finish(const HashSets* sets) {
        std::shared_ptr<CsrCacheJob> self = shared_from_this();
        return std::thread([self, sets]() { self->complete(*sets); });
    }

private:
    void join_helpers() {
        for (auto& th : helpers_) th.join();
        helpers_.clear();
    }

    // the writers' loop: claim the next run of finished lines (up to 32 MiB), copy it into the file at its final place
    void write_finished_lines() {
        while (!stop_ && !bad_) {
            size_t i0, i1;
            {
                std::unique_lock<std::mutex> lock(claim_);
                i0 = next_;
                if (i0 >= n_) return;
                int64_t g;
                while ((g = got_[i0].load(std::memory_order_acquire)) < 0) {
                    if (stop_ || bad_) return;
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                }
                i1 = i0;
                while (i1 < n_ && (g = got_[i1].load(std::memory_order_acquire)) >= 0 && (room_[i1] - room_[i0]) * 8 < (32 << 20)) {
                    if (g != room_[i1 + 1] - room_[i1]) {              // a short line: every later offset moves
                        bad_ = true;
                        return;
                    }
                    ++i1;
                }
                next_ = i1;
            }
            if (!pwrite_all(fd_, reinterpret_cast<const char*>(flat_ + room_[i0]), (size_t)(room_[i1] - room_[i0]) * 8,
                            head_bytes_ + (uint64_t)room_[i0] * 8)) {
                bad_ = true;
                return;
            }
        }
    }

    void complete(const HashSets& sets) {
        join_helpers();
        bool ok = !bad_ && !stop_;
        if (ok) {
            const std::string head = csr_head(id_, sets);
            ok = head.size() == head_bytes_ && pwrite_all(fd_, head.data(), head.size(), 0);
        }
        ok = (::close(fd_) == 0) && ok;
        fd_ = -1;
        if (ok && ::rename(part_.c_str(), csr_cache_path(text_).c_str()) == 0) return;
        ::unlink(part_.c_str());
        if (bad_ && !stop_) (void)write_csr_cache(text_, sets, 0);
    }

    std::string text_, part_;
    CsrHeader id_{};                                           // the text's size and modification time
    int fd_ = -1;
    size_t head_bytes_ = 0, n_ = 0, next_ = 0;                 // next_: the first line no writer has claimed (under claim_)
    const uint64_t* flat_ = nullptr;
    std::vector<int64_t> room_;
    std::unique_ptr<std::atomic<int64_t>[]> got_;              // -1 until line i is parsed, then its value count
    std::mutex claim_;
    std::atomic<bool> stop_{false}, bad_{false};               // stop: give up quietly; bad: a short line or a write error
    std::vector<std::thread> helpers_;
};

// One record per line.  with_names: "name: h1 h2 ..." (lines without ':' are skipped,
// src/project_everything.cpp:267-270); otherwise every line is a hash list
// (src/standalone_projection.cpp:28-35).
// cache_for: when not empty, the binary cache "<cache_for>.csr" (above) is written WHILE the text is parsed, by a
// CsrCacheJob (4 GB for 10k samples of 50k hashes, at the ~5 GB/s the kernel takes them: started after the parse, beside
// the projection, that copy was what a first `sketch` run waited for at its end).  cache_writer: the thread that
// completes the cache (it may outlive this call and reads `out`: join it before `out` goes away); without one the call
// returns when the cache is complete.
// (Parsing straight into a MAP_SHARED mapping of the cache file -- no copy at all -- took 8 s instead of 0.5 s on the GPU
// box's file system: a write fault per 4 KiB page of a file mapping, 16 threads deep.)
inline bool read_hash_file(const std::string& path, bool with_names, HashSets& out, unsigned threads = 0,
                           const std::string& cache_for = std::string(), std::thread* cache_writer = nullptr) {
    MappedText text;
    if (!text.open(path)) return false;
    const char* const buf = text.begin();
    const char* const map_end = text.map_end();
    if (threads == 0) threads = std::max(1u, std::thread::hardware_concurrency());
    const bool lap_on = getenv("MVS_STAGE_TIMING") != nullptr;
    auto lap_t = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        const auto t = std::chrono::steady_clock::now();
        if (lap_on) std::cerr << "[stage]   read_hash_file: " << what << " " << std::chrono::duration<double>(t - lap_t).count() << " s" << std::endl;
        lap_t = t;
    };

    const std::vector<Rec> recs = line_records(text, with_names, threads);
    lap("line table");

    // pass 1: an upper bound of every line's value count (exact for well-formed lines without duplicates) fixes where the
    // line's values go in the flat array, so that pass 2 can parse them in place (no buffer per sample, no copy into the
    // flat array afterwards)
    const size_t n = recs.size();
    threads = (unsigned)std::min<size_t>(threads, std::max<size_t>(1, n));
    std::vector<int64_t> room(n + 1, 0);
    for_lines(n, threads, [&](size_t i) { room[i + 1] = (int64_t)count_token_starts(buf + recs[i].colon + 1, buf + recs[i].e); });
    for (size_t i = 0; i < n; ++i) room[i + 1] += room[i];
    const size_t total_room = (size_t)room[n];
    lap("count");

    const size_t map_len = std::max<size_t>(total_room * 8, 8);
    void* base = ::mmap(nullptr, map_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base == MAP_FAILED) return false;
    ::madvise(base, map_len, MADV_HUGEPAGE);
    uint64_t* const flat = reinterpret_cast<uint64_t*>(base);

    uint64_t name_bytes = 0;
    if (with_names)
        for (size_t i = 0; i < n; ++i) name_bytes += recs[i].colon - recs[i].b;
    std::shared_ptr<CsrCacheJob> job;
    if (!cache_for.empty() && with_names && total_room) {
        job = std::make_shared<CsrCacheJob>();
        if (!job->start(cache_for, room, name_bytes, flat)) job.reset();
    }

    // pass 2: parse every line in place; sort + unique where the text was not strictly increasing
    std::vector<int64_t> offsets(n + 1, 0);
    try {
        for_lines(n, threads, [&](size_t i) {
            bool increasing = true;
            uint64_t* dst = flat + room[i];
            size_t k = parse_u64_raw(buf + recs[i].colon + 1, buf + recs[i].e, buf, map_end, dst, increasing);
            if (!increasing) k = sort_unique_u64(dst, k);
            offsets[i + 1] = (int64_t)k;
            if (job) job->publish(i, k);
        });
    } catch (...) {
        if (job) job->abandon();
        ::munmap(base, map_len);
        throw;
    }
    lap("tokens -> values");

    // lines that gave fewer values than their room (a bad token, duplicates): close the gaps
    for (size_t i = 0; i < n; ++i) offsets[i + 1] += offsets[i];
    const size_t total = (size_t)offsets[n];
    if (total != total_room) {
        if (job) job->stop_for_compaction();
        for (size_t i = 0; i < n; ++i) {
            const int64_t g = offsets[i + 1] - offsets[i];
            if (offsets[i] != room[i] && g) memmove(flat + offsets[i], flat + room[i], (size_t)g * 8);
        }
    }
    out.offsets = std::move(offsets);
    out.names.assign(n, std::string());
    if (with_names)
        for (size_t i = 0; i < n; ++i) out.names[i].assign(buf + recs[i].b, recs[i].colon - recs[i].b);
    out.hashes.adopt_mapping(base, map_len, flat, total);
    lap("offsets, names");

    if (job) {
        std::thread finisher = job->finish(&out);
        if (cache_writer) *cache_writer = std::move(finisher);
        else finisher.join();
    }
    return true;
}

// best effort: a cache that cannot be written is simply not there next time.  The values (gigabytes: 4 GB for 10k samples
// of 50k hashes) are written by several threads at their offsets -- the copy into the page cache is what takes the time
// and one thread moves ~2-5 GB/s; callers that have better things to do run this on a thread of its own.
inline bool write_csr_cache(const std::string& hash_file, const HashSets& sets, unsigned threads) {
    CsrHeader id{};
    if (!text_identity(hash_file, id.text_size, id.text_mtime_ns)) return false;
    const std::string path = csr_cache_path(hash_file), tmp = csr_cache_part_path(hash_file);
    remove_stale_cache_parts(hash_file);
    const std::string head = csr_head(id, sets);
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return false;
    std::atomic<bool> ok{pwrite_all(fd, head.data(), head.size(), 0)};
    const size_t value_bytes = sets.hashes.size() * 8;
    if (ok && value_bytes) {
        if (threads == 0) threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        const size_t chunk = (size_t)64 << 20;
        const size_t n_chunks = (value_bytes + chunk - 1) / chunk;
        threads = (unsigned)std::min<size_t>(threads, n_chunks);
        std::atomic<size_t> next{0};
        const char* base = reinterpret_cast<const char*>(sets.hashes.data());
        run_threads(threads, [&](unsigned) {
            for (size_t i = next++; i < n_chunks && ok; i = next++) {
                const size_t o = i * chunk, n = std::min(chunk, value_bytes - o);
                if (!pwrite_all(fd, base + o, n, head.size() + o)) ok = false;
            }
        });
    }
    const bool closed = ::close(fd) == 0;
    if (!ok || !closed || rename(tmp.c_str(), path.c_str()) != 0) {
        ::unlink(tmp.c_str());
        return false;
    }
    return true;
}

// true: `out` holds the cached sets (values mapped, not copied).  false: no cache, stale cache, or damaged file.
inline bool load_csr_cache(const std::string& hash_file, HashSets& out) {
    uint64_t text_size = 0;
    int64_t text_mtime = 0;
    if (!text_identity(hash_file, text_size, text_mtime)) return false;
    const std::string path = csr_cache_path(hash_file);
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (::fstat(fd, &st) != 0 || (size_t)st.st_size < sizeof(CsrHeader)) {
        ::close(fd);
        return false;
    }
    const size_t len = (size_t)st.st_size;
    void* m = ::mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) return false;
    const char* base = (const char*)m;
    CsrHeader h;
    memcpy(&h, base, sizeof h);
    const size_t names_pad = (size_t)((h.name_bytes + 7) / 8 * 8);
    const bool sane = memcmp(h.magic, "MVSCSR01", 8) == 0 && h.text_size == text_size && h.text_mtime_ns == text_mtime &&
                      h.samples < (1ULL << 40) && h.values < (1ULL << 48) && h.name_bytes < (1ULL << 40) &&
                      len == sizeof h + (h.samples + 1) * 8 + h.samples * 8 + names_pad + h.values * 8;
    if (!sane) {
        ::munmap(m, len);
        return false;
    }
    const int64_t* offs = (const int64_t*)(base + sizeof h);
    const uint64_t* ends = (const uint64_t*)(offs + h.samples + 1);
    const char* names = (const char*)(ends + h.samples);
    const uint64_t* values = (const uint64_t*)(names + names_pad);
    bool ok = offs[0] == 0 && (uint64_t)offs[h.samples] == h.values && (h.samples == 0 || ends[h.samples - 1] == h.name_bytes);
    for (uint64_t i = 0; ok && i < h.samples; ++i)
        ok = offs[i + 1] >= offs[i] && (i == 0 || ends[i] >= ends[i - 1]);
    if (!ok) {
        ::munmap(m, len);
        return false;
    }
    out.offsets.assign(offs, offs + h.samples + 1);
    out.names.resize((size_t)h.samples);
    for (uint64_t i = 0; i < h.samples; ++i) {
        const uint64_t b = i ? ends[i - 1] : 0;
        out.names[(size_t)i].assign(names + b, (size_t)(ends[i] - b));
    }
    ::madvise(m, len, MADV_SEQUENTIAL);
    out.hashes.adopt_mapping(m, len, values, (size_t)h.values);
    return true;
}

// A hash file for a tool: its .csr cache when `use_cache` and the cache is valid, else the text.  0, or 1 after a message
// on stderr.
inline int load_hash_sets(const char* prog, const std::string& file, bool use_cache, HashSets& sets) {
    bool parsed = use_cache && load_csr_cache(file, sets);
    if (!parsed) {
        try {
            parsed = read_hash_file(file, true, sets);
        } catch (const std::exception& e) {
            std::cerr << prog << ": reading " << file << ": " << e.what() << std::endl;
            return 1;
        }
    }
    if (!parsed) {
        std::cerr << "Error opening " << file << " for reading." << std::endl;
        return 1;
    }
    return 0;
}

}  // namespace mvs_host

#endif
