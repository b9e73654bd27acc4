// mvs_reads_selftest -- the streaming sequence reader (mvs_reads.hpp) against the whole-file parser (mvs_fasta.hpp) on crafted
// files, plain and gzip, at windows of 1, 2, 7, 64 and 4096 bytes: for every window the steps' bases joined with '\n' and their
// records must be exactly what read_sequences yields for the file, and a malformed file must fail with the same message.  The
// cases are those of mvs_fasta_selftest: wrapped sequences and qualities, quality lines that start with '@' or '>' or consist of
// ACGT, "\r\n", empty lines, no final newline, an empty file, every malformed input.  No device library.  Exits 0 when
// everything holds.
#include "mvs_reads.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include <unistd.h>

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::cerr << "FAILED line " << __LINE__ << ": " #cond << std::endl;         \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

using mvs_host::SeqRecord;

struct Parsed {
    bool ok = false;
    std::string bases, err;
    std::vector<std::string> names, seqs;
    size_t steps = 0, largest_step = 0;
};

Parsed whole(const std::string& path) {
    Parsed r;
    std::vector<SeqRecord> recs;
    r.ok = mvs_host::read_sequences(path, r.bases, recs, r.err);
    for (const SeqRecord& x : recs) {
        r.names.push_back(x.name);
        r.seqs.push_back(r.bases.substr(x.begin, x.end - x.begin));
    }
    return r;
}

Parsed streamed(const std::string& path, size_t window) {
    Parsed r;
    mvs_host::SeqStream st;
    if (!st.open(path, window, r.err)) return r;
    std::string bases;
    std::vector<SeqRecord> recs;
    bool first = true;
    while (!st.done()) {
        if (!st.next(bases, recs, r.err)) return r;
        ++r.steps;
        r.largest_step = std::max(r.largest_step, bases.size());
        if (recs.empty()) {
            CHECK(bases.empty() && st.done());
            continue;
        }
        if (!first) r.bases.push_back('\n');
        first = false;
        r.bases += bases;
        for (const SeqRecord& x : recs) {
            CHECK(x.begin <= x.end && x.end <= bases.size());
            r.names.push_back(x.name);
            r.seqs.push_back(bases.substr(x.begin, x.end - x.begin));
        }
    }
    r.ok = true;
    return r;
}

std::string gzip(const std::string& text) {
    z_stream z{};
    if (deflateInit2(&z, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return std::string();
    std::string out(deflateBound(&z, (uLong)text.size()) + 64, '\0');
    z.next_in = (Bytef*)text.data();
    z.avail_in = (uInt)text.size();
    z.next_out = (Bytef*)out.data();
    z.avail_out = (uInt)out.size();
    const int rc = deflate(&z, Z_FINISH);
    out.resize(rc == Z_STREAM_END ? z.total_out : 0);
    deflateEnd(&z);
    return out;
}

void write_file(const std::string& path, const std::string& bytes) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f << bytes;
}

const size_t kWindows[] = {1, 2, 7, 64, 4096};

// the file at `path` reads the same through every window as in one piece; -> that result
Parsed same_as_whole(const std::string& path) {
    const Parsed want = whole(path);
    for (size_t w : kWindows) {
        const Parsed got = streamed(path, w);
        const bool good = got.ok == want.ok && (want.ok ? got.bases == want.bases && got.names == want.names && got.seqs == want.seqs
                                                         : got.err == want.err);
        if (!good) {
            std::cerr << "  " << path << " at window " << w << ": ok " << got.ok << " / " << want.ok << ", err '" << got.err << "' / '"
                      << want.err << "', " << got.names.size() << " / " << want.names.size() << " records" << std::endl;
            ++g_failed;
        }
    }
    return want;
}

}  // namespace

int main() {
    char dir_template[] = "/tmp/mvs_reads_selftest_XXXXXX";
    const char* dir = mkdtemp(dir_template);
    if (!dir) {
        std::cerr << "no temporary directory" << std::endl;
        return 1;
    }
    const std::string d = dir;
    std::vector<std::string> files;
    auto both = [&](const std::string& name, const std::string& text, bool good, const char* needle = nullptr) {
        for (int z = 0; z < 2; ++z) {
            const std::string path = d + "/" + name + (z ? ".gz" : ".txt");
            write_file(path, z ? gzip(text) : text);
            files.push_back(path);
            const Parsed r = same_as_whole(path);
            CHECK(r.ok == good);
            if (needle) CHECK(r.err.find(path + ": line ") == 0 && r.err.find(needle) != std::string::npos);
        }
    };
    // ---- good inputs ----
    both("fasta", ">a first sample\nACGT\nacgt\n>b\tx\nNNAC\n\n>c\n>d\nT", true);
    both("fasta_crlf", "\r\n>a x\r\nAC\r\nGT\r\n>\r\nTT\r\n", true);
    both("empty", "", true);
    both("blank", "\n\n", true);
    both("header_only", ">only", true);
    both("fastq_quals", "@r1 lane 1\nACGTAC\n+\nACGTAC\n@r2\nGGTT\n+r2\n@CGT\n@r3\nAAAA\n+\n>AAA\n@r4\nCC\n+\n+T\n", true);
    both("fastq_wrapped", "@a\r\nACG\r\nTAC\r\n+\r\nIII\r\nII\r\nI\r\n\r\n@e\r\n\r\n+\r\n\r\n@b\r\nTT\r\n+\r\n@@", true);
    {
        std::string text;
        for (int i = 0; i < 300; ++i) text += "@read" + std::to_string(i) + " x\nACGTACGTNN" + std::string((size_t)(i % 37), 'G') + "\n+\n" +
                                              std::string((size_t)(10 + i % 37), i % 2 ? '@' : 'A') + "\n";
        both("fastq_many", text, true);
        // a record far larger than every window but the last
        both("fasta_long", ">long\n" + std::string(3000, 'A') + "\n" + std::string(500, 'C') + "\n>short\nGT\n", true);
        // what one step yields is bounded by the window and the longest record, not by the file
        const Parsed s = streamed(d + "/fastq_many.txt", 64);
        CHECK(s.ok && s.steps > 100 && s.largest_step < 64 + 2 * 50);
    }
    // ---- malformed: the same message as the whole-file parser ----
    both("m1", "ACGT\n>a\nAC\n", false, "before the first header");
    both("m2", "\n\n  >a\nAC\n", false, "before the first header");
    both("m3", "@a\nACGT\n", false, "cut short");
    both("m4", "@a\nACGT\n+\n", false, "cut short");
    both("m5", "@a\nACGT\n+\nIII", false, "cut short");
    both("m6", "@a\nACGT\n+\nIIII\n@b\nAC\n+\nI\n", false, "cut short");
    both("m7", "@a\nACGT\n+\nIIIII\n", false, "longer than the sequence");
    both("m8", "@a\nACGT\n+\nIII\nII\n", false, "longer than the sequence");
    both("m9", "@a\nACGT\n+\nIIII\nACGT\n", false, "starts with '@'");
    both("m10", "@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", false, "longer than the sequence");
    // binary rubbish must not crash and must end the same way
    {
        std::string junk;
        unsigned x = 12345;
        for (int i = 0; i < 20000; ++i) {
            x = x * 1664525u + 1013904223u;
            junk.push_back((char)(x >> 24));
        }
        int k = 0;
        for (const char* head : {"", ">", "@", "@a\n", ">a\n"}) {
            const std::string path = d + "/junk" + std::to_string(k++) + ".txt";
            write_file(path, std::string(head) + junk);
            files.push_back(path);
            (void)same_as_whole(path);
        }
    }
    // a damaged gzip stream and a missing file
    {
        std::string text;
        for (int i = 0; i < 3000; ++i) text += ">rec" + std::to_string(i) + " x\nACGTACGTNN\nacgt\n";
        const std::string gz = gzip(text);
        write_file(d + "/cut.gz", gz.substr(0, gz.size() / 2));
        files.push_back(d + "/cut.gz");
        const Parsed want = whole(d + "/cut.gz");
        for (size_t w : {(size_t)64, (size_t)4096}) {
            const Parsed got = streamed(d + "/cut.gz", w);
            CHECK(!want.ok && !got.ok && got.err.find(d + "/cut.gz") == 0);
        }
        const Parsed missing = streamed(d + "/nothing", 64);
        CHECK(!missing.ok && missing.err == "Error opening " + d + "/nothing for reading.");
    }
    for (const std::string& f : files) ::unlink(f.c_str());
    ::rmdir(dir);
    if (g_failed) {
        std::cerr << g_failed << " checks failed" << std::endl;
        return 1;
    }
    std::cout << "mvs_reads_selftest: all checks passed" << std::endl;
    return 0;
}
