// mvs_fasta.hpp -- FASTA / FASTQ, plain or gzip, into the byte buffer mvs_hash_set_from_sequences takes.  Pure host (zlib, as
// mvs_ingest.hpp); the format is chosen by content, not by file name: gzip by its magic (zlib's gzread passes anything else
// through), FASTA or FASTQ by the first character of the first line that is not empty ('>' or '@').
//
// Only sequence lines reach the buffer: no header, no '+' line, no quality line (a quality string may consist of the letters
// ACGT and may start with '@' or '>': it is recognised by its place and its length, never by its content), no line end ("\r\n"
// is accepted).  Records are joined with ONE '\n' -- a break for the sketching rule, so no k-mer spans two records -- and
// reported with their names (the header up to the first white space) and byte ranges.  Sequences and quality strings may be
// wrapped over several lines in both formats; empty lines between records are skipped.
//
// Malformed input fails with "<file>: line <n>: <what>" in `err`, never with a crash: data before the first header, a FASTQ
// record cut short (no '+' line, or the file ends inside the quality string), a quality string whose length differs from the
// sequence's, a gzip stream that is damaged or cut short.  On failure `bases` and `records` are what they were before the call.
#ifndef MVS_FASTA_HPP
#define MVS_FASTA_HPP

#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace mvs_host {

struct SeqRecord {
    std::string name;
    size_t begin = 0, end = 0;   // its bases are bytes [begin, end) of the buffer
};

// the records of the text [p, p + n) appended to bases / records; `label` names the input in messages
inline bool parse_sequences(const char* p, size_t n, const std::string& label, std::string& bases, std::vector<SeqRecord>& records,
                            std::string& err) {
    const size_t bases_before = bases.size(), records_before = records.size();
    size_t line_no = 0;
    auto fail = [&](size_t line, const std::string& what) {
        err = label + ": line " + std::to_string(line) + ": " + what;
        bases.resize(bases_before);
        records.resize(records_before);
        return false;
    };
    auto open_record = [&](const char* b, const char* e) {   // [b, e): the header behind its first character
        const char* w = b;
        while (w < e && *w != ' ' && *w != '\t' && *w != '\v' && *w != '\f') ++w;
        if (records.size() > records_before) bases.push_back('\n');
        SeqRecord r;
        r.name.assign(b, w);
        r.begin = r.end = bases.size();
        records.push_back(std::move(r));
    };
    enum { kStart, kFastaSeq, kFastqHeader, kFastqSeq, kFastqQual } state = kStart;
    size_t seq_len = 0, qual_len = 0, record_line = 0;
    size_t pos = 0;
    while (pos < n) {
        const char* b = p + pos;
        const char* nl = (const char*)memchr(b, '\n', n - pos);
        const char* e = nl ? nl : p + n;
        pos = (size_t)(e - p) + 1;
        ++line_no;
        if (e > b && e[-1] == '\r') --e;
        const size_t len = (size_t)(e - b);
        switch (state) {
            case kStart:
                if (len == 0) break;
                if (*b == '>') {
                    open_record(b + 1, e);
                    state = kFastaSeq;
                } else if (*b == '@') {
                    open_record(b + 1, e);
                    record_line = line_no;
                    seq_len = 0;
                    state = kFastqSeq;
                } else {
                    return fail(line_no, "data before the first header (a FASTA record starts with '>', a FASTQ record with '@')");
                }
                break;
            case kFastaSeq:
                if (len == 0) break;
                if (*b == '>') {
                    open_record(b + 1, e);
                } else {
                    bases.append(b, len);
                    records.back().end = bases.size();
                }
                break;
            case kFastqHeader:
                if (len == 0) break;
                if (*b != '@') return fail(line_no, "a FASTQ record starts with '@'");
                open_record(b + 1, e);
                record_line = line_no;
                seq_len = 0;
                state = kFastqSeq;
                break;
            case kFastqSeq:
                if (len > 0 && *b == '+') {
                    qual_len = 0;
                    state = seq_len == 0 ? kFastqHeader : kFastqQual;
                } else {
                    bases.append(b, len);
                    records.back().end = bases.size();
                    seq_len += len;
                }
                break;
            case kFastqQual:
                qual_len += len;
                if (qual_len > seq_len)
                    return fail(line_no, "the quality string is longer than the sequence (" + std::to_string(qual_len) + " and " +
                                             std::to_string(seq_len) + ") in the record of line " + std::to_string(record_line));
                if (qual_len == seq_len) state = kFastqHeader;
                break;
        }
    }
    if (state == kFastqSeq)
        return fail(line_no, "the FASTQ record of line " + std::to_string(record_line) + " is cut short: no '+' line");
    if (state == kFastqQual)
        return fail(line_no, "the FASTQ record of line " + std::to_string(record_line) + " is cut short: its quality string holds " +
                                 std::to_string(qual_len) + " of " + std::to_string(seq_len) + " characters");
    return true;
}

// the whole file, gunzipped if it is gzip
inline bool slurp_maybe_gzip(const std::string& path, std::string& data, std::string& err) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) {
        err = "Error opening " + path + " for reading.";
        return false;
    }
    gzbuffer(f, 1u << 20);
    data.clear();
    std::vector<char> buf(1u << 22);
    for (;;) {
        const int got = gzread(f, buf.data(), (unsigned)buf.size());
        if (got < 0) {
            int code = 0;
            const char* msg = gzerror(f, &code);
            err = path + ": " + (msg && *msg ? msg : "read error");
            gzclose(f);
            return false;
        }
        if (got == 0) break;
        data.append(buf.data(), (size_t)got);
    }
    int code = 0;
    const char* msg = gzerror(f, &code);
    if (code != Z_OK && code != Z_STREAM_END) {
        err = path + ": " + (msg && *msg ? msg : "read error");
        gzclose(f);
        return false;
    }
    if (gzclose(f) != Z_OK) {       // Z_BUF_ERROR: the gzip stream ends before its trailer
        err = path + ": the gzip stream is cut short";
        return false;
    }
    return true;
}

// the records of one file appended to bases / records
inline bool read_sequences(const std::string& path, std::string& bases, std::vector<SeqRecord>& records, std::string& err) {
    std::string data;
    if (!slurp_maybe_gzip(path, data, err)) return false;
    return parse_sequences(data.data(), data.size(), path, bases, records, err);
}

}  // namespace mvs_host

#endif
