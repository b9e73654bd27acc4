// mvs_reads.hpp -- FASTA / FASTQ, plain or gzip, read through a text window of a given size: what sketch_reads feeds to
// mvs_kmer_sketcher_add window by window, so that host memory is bounded by the window and not by the file.  Pure host (zlib).
//
// SeqStream is read_sequences (mvs_fasta.hpp) cut into steps: the same rules line by line (format by content, wrapped sequences
// and qualities, a quality string recognised by its place and length, "\r\n", empty lines, a last line without '\n') and the same
// "<file>: line <n>: <what>" messages.  A step reads about `window` bytes of text (gzread in chunks) and yields the bases of the
// records that END in it, joined with ONE '\n'; the record that the window cuts is carried into the next step, and a record
// larger than the window makes the step read on until the record ends: the window grows, nothing is ever yielded in parts.
// For every window size the steps' bases, joined with '\n', and their records are exactly what read_sequences yields for the
// file.  A malformed file fails in the step that meets the damage; the steps before it have yielded their records.
#ifndef MVS_READS_HPP
#define MVS_READS_HPP

#include "mvs_fasta.hpp"

#include <algorithm>

namespace mvs_host {

class SeqStream {
public:
    SeqStream() = default;
    SeqStream(const SeqStream&) = delete;
    SeqStream& operator=(const SeqStream&) = delete;
    ~SeqStream() {
        if (f_) gzclose(f_);
    }

    bool open(const std::string& path, size_t window, std::string& err) {
        path_ = path;
        window_ = std::max<size_t>(window, 1);
        f_ = gzopen(path.c_str(), "rb");
        if (!f_) {
            err = "Error opening " + path + " for reading.";
            return false;
        }
        gzbuffer(f_, 1u << 20);
        return true;
    }

    // true once every record has been yielded
    bool done() const { return eof_; }
    // lines read so far
    size_t lines() const { return line_no_; }

    // One step: bases / records are REPLACED by the records that end in this window (possibly none at the file's end).
    // false: `err` says why; the stream is then useless.
    bool next(std::string& bases, std::vector<SeqRecord>& records, std::string& err) {
        bases.clear();
        records.clear();
        out_bases_ = &bases;
        out_records_ = &records;
        size_t taken = 0;
        chunk_.resize(std::min<size_t>(window_, 1u << 22));
        while (!eof_ && (taken < window_ || records.empty())) {
            const size_t want = taken < window_ ? std::min(chunk_.size(), window_ - taken) : chunk_.size();
            const int got = gzread(f_, chunk_.data(), (unsigned)want);
            if (got < 0) return gz_fail(err);
            if (got == 0) {
                int code = 0;
                (void)gzerror(f_, &code);
                if (code != Z_OK && code != Z_STREAM_END) return gz_fail(err);
                const int rc = gzclose(f_);
                f_ = nullptr;
                if (rc != Z_OK) {       // Z_BUF_ERROR: the gzip stream ends before its trailer
                    err = path_ + ": the gzip stream is cut short";
                    return false;
                }
                eof_ = true;
                if (!pending_.empty()) {                                   // a last line without '\n'
                    if (!line(pending_.data(), pending_.data() + pending_.size(), err)) return false;
                    pending_.clear();
                }
                if (state_ == kFastqSeq)
                    return fail(err, "the FASTQ record of line " + std::to_string(record_line_) + " is cut short: no '+' line");
                if (state_ == kFastqQual)
                    return fail(err, "the FASTQ record of line " + std::to_string(record_line_) + " is cut short: its quality string holds " +
                                         std::to_string(qual_len_) + " of " + std::to_string(seq_len_) + " characters");
                if (open_) complete();
                break;
            }
            taken += (size_t)got;
            // whole lines: those of the carried text + this chunk
            const char* p = chunk_.data();
            const char* end = p + got;
            while (p < end) {
                const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
                if (!nl) {
                    pending_.append(p, end);
                    break;
                }
                if (pending_.empty()) {
                    if (!line(p, nl, err)) return false;
                } else {
                    pending_.append(p, nl);
                    if (!line(pending_.data(), pending_.data() + pending_.size(), err)) return false;
                    pending_.clear();
                }
                p = nl + 1;
            }
        }
        return true;
    }

private:
    enum State { kStart, kFastaSeq, kFastqHeader, kFastqSeq, kFastqQual };

    bool fail(std::string& err, const std::string& what) {
        err = path_ + ": line " + std::to_string(line_no_) + ": " + what;
        return false;
    }
    bool gz_fail(std::string& err) {
        int code = 0;
        const char* msg = gzerror(f_, &code);
        err = path_ + ": " + (msg && *msg ? msg : "read error");
        return false;
    }
    void open_record(const char* b, const char* e) {   // [b, e): the header behind its first character
        if (open_) complete();
        const char* w = b;
        while (w < e && *w != ' ' && *w != '\t' && *w != '\v' && *w != '\f') ++w;
        cur_name_.assign(b, w);
        cur_.clear();
        open_ = true;
    }
    // the open record has ended: it joins this step's output
    void complete() {
        if (!out_records_->empty()) out_bases_->push_back('\n');
        SeqRecord r;
        r.name = cur_name_;
        r.begin = out_bases_->size();
        out_bases_->append(cur_);
        r.end = out_bases_->size();
        out_records_->push_back(std::move(r));
        cur_.clear();
        open_ = false;
    }
    // one line [b, e) without its '\n': the switch of parse_sequences
    bool line(const char* b, const char* e, std::string& err) {
        ++line_no_;
        if (e > b && e[-1] == '\r') --e;
        const size_t len = (size_t)(e - b);
        switch (state_) {
            case kStart:
                if (len == 0) break;
                if (*b == '>') {
                    open_record(b + 1, e);
                    state_ = kFastaSeq;
                } else if (*b == '@') {
                    open_record(b + 1, e);
                    record_line_ = line_no_;
                    seq_len_ = 0;
                    state_ = kFastqSeq;
                } else {
                    return fail(err, "data before the first header (a FASTA record starts with '>', a FASTQ record with '@')");
                }
                break;
            case kFastaSeq:
                if (len == 0) break;
                if (*b == '>') open_record(b + 1, e);
                else cur_.append(b, len);
                break;
            case kFastqHeader:
                if (len == 0) break;
                if (*b != '@') return fail(err, "a FASTQ record starts with '@'");
                open_record(b + 1, e);
                record_line_ = line_no_;
                seq_len_ = 0;
                state_ = kFastqSeq;
                break;
            case kFastqSeq:
                if (len > 0 && *b == '+') {
                    qual_len_ = 0;
                    if (seq_len_ == 0) {
                        complete();
                        state_ = kFastqHeader;
                    } else {
                        state_ = kFastqQual;
                    }
                } else {
                    cur_.append(b, len);
                    seq_len_ += len;
                }
                break;
            case kFastqQual:
                qual_len_ += len;
                if (qual_len_ > seq_len_)
                    return fail(err, "the quality string is longer than the sequence (" + std::to_string(qual_len_) + " and " +
                                         std::to_string(seq_len_) + ") in the record of line " + std::to_string(record_line_));
                if (qual_len_ == seq_len_) {
                    complete();
                    state_ = kFastqHeader;
                }
                break;
        }
        return true;
    }

    std::string path_;
    size_t window_ = 1;
    gzFile f_ = nullptr;
    bool eof_ = false;
    std::vector<char> chunk_;
    std::string pending_;          // the text behind the last '\n' read
    State state_ = kStart;
    size_t line_no_ = 0, seq_len_ = 0, qual_len_ = 0, record_line_ = 0;
    bool open_ = false;            // a record has begun and not ended
    std::string cur_name_, cur_;   // ... its name and its bases so far
    std::string* out_bases_ = nullptr;
    std::vector<SeqRecord>* out_records_ = nullptr;
};

}  // namespace mvs_host

#endif
