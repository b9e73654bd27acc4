// mvs_fasta_selftest -- crafted good and bad inputs through the sequence parser (mvs_fasta.hpp): FASTA and FASTQ, wrapped lines,
// "\r\n", quality strings made of the letters ACGT or starting with '@', empty records, gzip files, and every kind of malformed
// input, which must fail with a message that names the file and the line.  No device library.  Exits 0 when everything holds.
#include "mvs_fasta.hpp"

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
    std::vector<SeqRecord> recs;
};

Parsed parse(const std::string& text) {
    Parsed r;
    r.ok = mvs_host::parse_sequences(text.data(), text.size(), "input.fa", r.bases, r.recs, r.err);
    return r;
}

std::string names(const Parsed& r) {
    std::string s;
    for (const SeqRecord& x : r.recs) s += x.name + "[" + r.bases.substr(x.begin, x.end - x.begin) + "]";
    return s;
}

bool fails_at(const std::string& text, size_t line, const char* needle) {
    Parsed r;
    r.bases = "kept";
    r.recs.resize(1);
    r.ok = mvs_host::parse_sequences(text.data(), text.size(), "input.fa", r.bases, r.recs, r.err);
    const std::string where = "input.fa: line " + std::to_string(line) + ": ";
    const bool good = !r.ok && r.err.compare(0, where.size(), where) == 0 && r.err.find(needle) != std::string::npos &&
                      r.bases == "kept" && r.recs.size() == 1;
    if (!good) std::cerr << "  got ok = " << r.ok << ", err = '" << r.err << "'" << std::endl;
    return good;
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

}  // namespace

int main() {
    // ---- FASTA ----
    {
        const Parsed r = parse(">a first sample\nACGT\nacgt\n>b\tx\nNNAC\n\n>c\n>d\nT");
        CHECK(r.ok && r.recs.size() == 4);
        CHECK(r.bases == "ACGTacgt\nNNAC\n\nT");
        CHECK(names(r) == "a[ACGTacgt]b[NNAC]c[]d[T]");
    }
    {
        const Parsed r = parse("\r\n>a x\r\nAC\r\nGT\r\n>\r\nTT\r\n");
        CHECK(r.ok && r.bases == "ACGT\nTT" && names(r) == "a[ACGT][TT]");
    }
    {
        const Parsed r = parse("");
        CHECK(r.ok && r.recs.empty() && r.bases.empty());
        const Parsed s = parse("\n\n");
        CHECK(s.ok && s.recs.empty());
        const Parsed t = parse(">only");
        CHECK(t.ok && t.recs.size() == 1 && t.recs[0].name == "only" && t.bases.empty());
    }
    // appended behind what the buffer holds, without a break in front of the first record
    {
        Parsed r;
        r.bases = "XY";
        r.ok = mvs_host::parse_sequences(">a\nAC\n>b\nGT\n", 12, "f", r.bases, r.recs, r.err);
        CHECK(r.ok && r.bases == "XYAC\nGT" && r.recs[0].begin == 2 && r.recs[1].begin == 5 && r.recs[1].end == 7);
    }
    // ---- FASTQ ----
    {
        // quality strings of the letters ACGT, one starting with '@', one with '>', one with '+'
        const Parsed r = parse("@r1 lane 1\nACGTAC\n+\nACGTAC\n@r2\nGGTT\n+r2\n@CGT\n@r3\nAAAA\n+\n>AAA\n@r4\nCC\n+\n+T\n");
        CHECK(r.ok && r.bases == "ACGTAC\nGGTT\nAAAA\nCC");
        CHECK(names(r) == "r1[ACGTAC]r2[GGTT]r3[AAAA]r4[CC]");
    }
    {
        // wrapped sequence and quality, "\r\n", an empty record, no newline at the end
        const Parsed r = parse("@a\r\nACG\r\nTAC\r\n+\r\nIII\r\nII\r\nI\r\n\r\n@e\r\n\r\n+\r\n\r\n@b\r\nTT\r\n+\r\n@@");
        CHECK(r.ok && names(r) == "a[ACGTAC]e[]b[TT]" && r.bases == "ACGTAC\n\nTT");
    }
    // ---- malformed ----
    CHECK(fails_at("ACGT\n>a\nAC\n", 1, "before the first header"));
    CHECK(fails_at("\n\n  >a\nAC\n", 3, "before the first header"));
    CHECK(fails_at("@a\nACGT\n", 2, "cut short"));
    CHECK(fails_at("@a\nACGT\n+\n", 3, "cut short"));
    CHECK(fails_at("@a\nACGT\n+\nIII", 4, "cut short"));
    CHECK(fails_at("@a\nACGT\n+\nIIII\n@b\nAC\n+\nI\n", 8, "cut short"));
    CHECK(fails_at("@a\nACGT\n+\nIIIII\n", 4, "longer than the sequence"));
    CHECK(fails_at("@a\nACGT\n+\nIII\nII\n", 5, "longer than the sequence"));
    CHECK(fails_at("@a\nACGT\n+\nIIII\nACGT\n", 5, "starts with '@'"));
    CHECK(fails_at("@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", 5, "longer than the sequence"));   // "@b" counts as quality
    // binary rubbish must not crash
    {
        std::string junk;
        unsigned x = 12345;
        for (int i = 0; i < 100000; ++i) {
            x = x * 1664525u + 1013904223u;
            junk.push_back((char)(x >> 24));
        }
        for (const char* head : {"", ">", "@", "@a\n", ">a\n"}) {
            const Parsed r = parse(std::string(head) + junk);
            CHECK(r.ok || r.err.compare(0, 15, "input.fa: line ") == 0);
            for (const SeqRecord& s : r.recs) CHECK(s.begin <= s.end && s.end <= r.bases.size());
        }
    }
    // ---- files: plain, gzip, damaged gzip, missing ----
    {
        char dir_template[] = "/tmp/mvs_fasta_selftest_XXXXXX";
        const char* dir = mkdtemp(dir_template);
        CHECK(dir != nullptr);
        if (dir) {
            const std::string d = dir;
            std::string text;
            for (int i = 0; i < 3000; ++i) text += ">rec" + std::to_string(i) + " x\nACGTACGTNN\nacgt\n";
            const std::string gz = gzip(text);
            CHECK(gz.size() > 20 && gz.size() < text.size());
            write_file(d + "/a.fa", text);
            write_file(d + "/a.anything", gz);            // by content, not by name
            write_file(d + "/cut.gz", gz.substr(0, gz.size() / 2));
            write_file(d + "/bad.fq", "@a\nACGT\n+\nII\n");
            Parsed plain, zipped, cut, bad, missing;
            plain.ok = mvs_host::read_sequences(d + "/a.fa", plain.bases, plain.recs, plain.err);
            zipped.ok = mvs_host::read_sequences(d + "/a.anything", zipped.bases, zipped.recs, zipped.err);
            CHECK(plain.ok && zipped.ok && plain.recs.size() == 3000 && plain.bases == zipped.bases && names(plain) == names(zipped));
            CHECK(plain.recs[2999].name == "rec2999" && plain.bases.size() == 3000 * 14 + 2999);
            cut.ok = mvs_host::read_sequences(d + "/cut.gz", cut.bases, cut.recs, cut.err);
            CHECK(!cut.ok && cut.err.find(d + "/cut.gz") == 0 && cut.bases.empty() && cut.recs.empty());
            bad.ok = mvs_host::read_sequences(d + "/bad.fq", bad.bases, bad.recs, bad.err);
            CHECK(!bad.ok && bad.err == d + "/bad.fq: line 4: the FASTQ record of line 1 is cut short: its quality string holds 2 of 4 characters");
            missing.ok = mvs_host::read_sequences(d + "/nothing", missing.bases, missing.recs, missing.err);
            CHECK(!missing.ok && missing.err == "Error opening " + d + "/nothing for reading.");
            for (const char* f : {"/a.fa", "/a.anything", "/cut.gz", "/bad.fq"}) ::unlink((d + f).c_str());
            ::rmdir(dir);
        }
    }
    if (g_failed) {
        std::cerr << g_failed << " checks failed" << std::endl;
        return 1;
    }
    std::cout << "mvs_fasta_selftest: all checks passed" << std::endl;
    return 0;
}
