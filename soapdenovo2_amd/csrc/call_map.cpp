// call_map.cpp -- the `map` sub-command (call_align, standardPregraph/map.c:94-147): reads -> contigs, on the GPU.
//
//   map -s lib.cfg -g prefix [-f] [-p n_cpu] [-k kmer_R2C] [-h contig_total_length]
//
// Reads <prefix>.contig, .ContigIndex and .preGraphBasic; writes <prefix>.readOnContig.gz, .readInGap.gz, .peGrads and, with -f,
// .shortreadInGap.gz and .PEreadOnContig.gz -- for the same -p, the reference's files (the .gz ones after decompression).  With the
// long-read pass: <prefix>.longReadInGap and, with -f, .RlongReadInGap, byte for byte.
//
// Layout of the stage:
//   1. the contigs of K + 2 bases or more are read (readseq1by1 semantics) and packed; the device builds the k-mer index (map_kernels.hip)
//   2. the reads are read one by one exactly as read1seqInLib does with pairs = 1 (readseq1by1.c:1037-1244; NOT pregraph's AIORead
//      chunking) and cut into the reference's batches: maxReadNum = 100000000 / (maxReadLen - K + 1), rounded down to even
//      (prlRead2Ctg.c:814-815).  parse1read sees the global ALIGNLEN as it stands when the batch is processed (:905-926), so every
//      batch carries the value after its last read
//   3. a batch is packed (pg_pack_read's layout) and mapped by the read kernel, a lane a read
//   4. recordAlldgn (:627-725) runs on the host in read order; the text and binary records are deflated by host threads, one gzip
//      member per few megabytes (the same rule as .edge.gz)
//   5. with SOAPDENOVO2_AMD_MAP_LONG=1 the long-read pass (prlLongRead2Ctg, prlRead2Ctg.c:1080-1298) runs between 1. and 2.: the
//      libraries with asm_flags=4 are read one read at a time (pairs = 0: f= and q= files too), mapped a lane a read, or a wavefront
//      a read with SOAPDENOVO2_AMD_MAP_LONG_KERNEL=wave (lane is the default until the two are measured), and the
//      footprinted ones written to <prefix>.longReadInGap and, with -f, <prefix>.RlongReadInGap (plain files)
// Not here: without that switch a config with a long-read library (asm_flags=4) is refused before anything is written; one GPU (the
// first of SOAPDENOVO2_AMD_DEVICES).  SOAPDENOVO2_AMD_MAP_HOST=1 runs the host twin of the index and the read kernels instead (the CPU
// tests).
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <zlib.h>

#include <algorithm>
#include <deque>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "env.hpp"
#include "host_reads.hpp"
#include "map_index.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

double now_s() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

inline char base2int(char c) { return (char)((c & 0x06) >> 1); }          // inc/def.h:39

// ---- input: fgets()/feof() on a plain or gzip file, with stdio's end-of-file rule (the flag is raised by a read that finds nothing) ----
class LineIn {
public:
    explicit LineIn(const std::string& path) : buf_(1 << 20) {
        const bool gz = path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0;    // openFile4read, readseq1by1.c:676-714
        if (gz) gz_ = gzopen(path.c_str(), "rb");
        else fp_ = fopen(path.c_str(), "rb");
        if (!gz_ && !fp_) { fprintf(stderr, "Cannot open %s. Now exit to system...\n", path.c_str()); exit(-1); }
        if (gz_) gzbuffer(gz_, 1 << 20);
    }
    ~LineIn() { close(); }
    void close() {
        if (gz_) gzclose(gz_);
        if (fp_) fclose(fp_);
        gz_ = nullptr; fp_ = nullptr; eof_ = true;
    }
    bool eof() const { return eof_; }
    // fgets(s, n): at most n - 1 characters, up to and including a newline; -1 = nothing read (NULL)
    int gets(char* s, int n) {
        int k = 0;
        while (k < n - 1) {
            if (pos_ == end_ && !fill()) break;
            const size_t want = std::min(end_ - pos_, (size_t)(n - 1 - k));
            const char* p = buf_.data() + pos_;
            const char* nl = (const char*)memchr(p, '\n', want);
            const size_t take = nl ? (size_t)(nl - p) + 1 : want;
            memcpy(s + k, p, take);
            k += (int)take;
            pos_ += take;
            if (nl) break;
        }
        if (k == 0) return -1;
        s[k] = 0;
        return k;
    }

private:
    bool fill() {
        if (eof_) return false;
        const long n = gz_ ? (long)gzread(gz_, buf_.data(), (unsigned)buf_.size()) : (long)fread(buf_.data(), 1, buf_.size(), fp_);
        if (n <= 0) { eof_ = true; return false; }
        pos_ = 0;
        end_ = (size_t)n;
        return true;
    }
    gzFile gz_ = nullptr;
    FILE* fp_ = nullptr;
    std::vector<char> buf_;
    size_t pos_ = 0, end_ = 0;
    bool eof_ = false;
};

// the bases of one line as readseq1by1 / read1seqfq take them (readseq1by1.c:98-124): the line's strlen (newline included) counts
// against what is left of max_len; letters are folded and go through base2int, '.' is an A, anything else is dropped
inline void take_line(const char* str, int strL, int max_len, char* seq, int& n) {
    if (strL + n > max_len) strL = max_len - n;
    for (int i = 0; i < strL; i++) {
        const char c = str[i];
        if (c >= 'a' && c <= 'z') seq[n++] = base2int((char)(c - 'a' + 'A'));
        else if (c >= 'A' && c <= 'Z') seq[n++] = base2int(c);
        else if (c == '.') seq[n++] = base2int('A');
    }
}

// readseq1by1 (readseq1by1.c:50-136); num_seq < 0: the call that only finds the first header
void readseq1by1(LineIn& in, char* seq, std::string& name, int& len, int num_seq, int max_len, int line_len, std::vector<char>& str) {
    str.resize((size_t)line_len + 1);
    int n = 0, k;
    while ((k = in.gets(str.data(), line_len)) >= 0) {
        if (str[0] == '#') continue;
        if (str[0] == '>') {
            len = n;
            char tmp[4096];
            tmp[0] = 0;
            sscanf(str.data() + 1, "%4095s", tmp);
            name = tmp;
            return;
        }
        take_line(str.data(), (int)strlen(str.data()), max_len, seq, n);
    }
    len = num_seq >= 0 ? n : 0;
}

// read1seqfq (readseq1by1.c:362-447)
void read1seqfq(LineIn& in, char* seq, int& len, int max_len, int line_len, std::vector<char>& str) {
    str.resize((size_t)line_len + 1);
    bool flag = false;
    while (in.gets(str.data(), line_len) >= 0)
        if (str[0] == '@') { flag = true; break; }
    if (!flag) { len = 0; return; }
    int n = 0;
    while (in.gets(str.data(), line_len) >= 0) {
        if (str[0] == '+') {
            in.gets(str.data(), line_len);                          // the quality line
            len = n;
            return;
        }
        take_line(str.data(), (int)strlen(str.data()), max_len, seq, n);
    }
    len = n;
}

// ---- b=: one record at a time (read1seqbam, readseq1by1.c:449-592).  host_reads.cpp's BAM reader decodes records the same way but pushes
// whole files at pregraph's sink (with its take-back delay line); map pulls records one by one and takes pairs back itself
// (prlRead2Ctg.c:875-888), so it has this small pull reader over the same format.
class BamIn {
public:
    explicit BamIn(const std::string& path) {
        gz_ = gzopen(path.c_str(), "rb");
        if (!gz_) { fprintf(stderr, "Cannot open %s. Now exit to system...\n", path.c_str()); exit(-1); }
        gzbuffer(gz_, 1 << 20);
        char magic[4];
        int32_t l_text = 0, n_ref = 0;
        bool ok = need(magic, 4) && !memcmp(magic, "BAM\1", 4) && need(&l_text, 4) && l_text >= 0 && skip((size_t)l_text) && need(&n_ref, 4) && n_ref >= 0;
        for (int32_t r = 0; ok && r < n_ref; r++) {
            int32_t l_name = 0, l_ref = 0;
            ok = need(&l_name, 4) && l_name >= 0 && skip((size_t)l_name) && need(&l_ref, 4);
        }
        if (!ok) { fprintf(stderr, "Cannot read the header.\n"); exit(-1); }
    }
    ~BamIn() { close(); }
    void close() { if (gz_) gzclose(gz_); gz_ = nullptr; }
    // one record: false = end of file (samread < 0).  flag and the SEQ column's bases (cut to max_len characters) are returned
    bool next(uint16_t& flag, char* seq, int& n, int max_len) {
        n = 0;
        if (!gz_) return false;
        int32_t block = 0;
        if (!need(&block, 4) || block < 32) return false;
        rec_.resize((size_t)block);
        if (!need(rec_.data(), (size_t)block)) return false;
        const uint32_t l_read_name = rec_[8];
        uint16_t n_cigar;
        int32_t l_seq;
        memcpy(&n_cigar, rec_.data() + 12, 2); memcpy(&flag, rec_.data() + 14, 2); memcpy(&l_seq, rec_.data() + 16, 4);
        const size_t seq_at = 32 + (size_t)l_read_name + 4 * (size_t)n_cigar;
        if (l_seq < 0 || seq_at + ((size_t)l_seq + 1) / 2 > (size_t)block) return false;
        static const char nt16[] = "=ACMGRSVTWYHKDBN";
        const int look = std::min((int)l_seq, std::max(max_len, 0));
        for (int j = 0; j < look; j++) {
            const char ch = nt16[(rec_[seq_at + (size_t)(j >> 1)] >> ((~j & 1) << 2)) & 0xf];
            if (ch >= 'A' && ch <= 'Z') seq[n++] = base2int(ch);
        }
        return true;
    }

private:
    bool need(void* dst, size_t n) { return gzread(gz_, dst, (unsigned)n) == (int)n; }
    bool skip(size_t n) { char tmp[4096]; while (n) { const size_t k = std::min(n, sizeof tmp); if (!need(tmp, k)) return false; n -= k; } return true; }
    gzFile gz_ = nullptr;
    std::vector<uint8_t> rec_;
};

void reverse2k(char* s, int n) {                                    // readseq1by1.c:788-802
    std::reverse(s, s + n);
    for (int i = 0; i < n; i++) s[i] ^= 2;
}

struct PeInfo { int insertS; long long PE_bound; int rank, pair_num_cut; };

// read1seqInLib (readseq1by1.c:1037-1244) over the libs of parse_lib_config (sorted by avg_ins as scan_libInfo leaves them, lib.c:505):
// with pairs = 1, asm_ctg = 0 for the short reads, with pairs = 0, asm_ctg = 4 for the long-read pass (long_pass).  max_len_all =
// maxReadLen4all; line_buf_len = the maxReadLen that decides whether gStr is there (prlRead2Ctg.c:826-829, :1133-1136)
class LibReader {
public:
    LibReader(const LibConfig& cfg, int max_len_all, int line_buf_len, bool long_pass = false)
        : cfg_(cfg), all_(max_len_all), long_(long_pass), st_(cfg.libs.size()) {
        max_len_ = all_;
        line_len_ = 5000 < line_buf_len ? -1 : 5000;                // with gStr: lines of maxReadLen + 1
    }
    long long n_solexa = 0, readNumBack = 0;
    std::vector<PeInfo> pes;
    int max_len() const { return max_len_; }

    // false = no more reads; type = -1: the pair is taken back (BAM)
    bool next(char* seq, int& len, int& libNo, int& type) {
        size_t i = (size_t)libNo;
        const size_t prevLib = i;
        const size_t nl = cfg_.libs.size();
        Lib& S = st_[i];
        const bool at_end = (S.type != 4 && !S.fp1) || (S.type == 4 && !S.fp3) || (S.type == 4 && readstate_ < 0) ||
                            (S.type == 1 && S.fp1->eof() && S.fp2->eof()) || (S.type == 2 && (S.fp1->eof() || S.fp2->eof())) ||
                            (S.type != 1 && S.type != 2 && S.type != 4 && S.fp1->eof());
        if (at_end) {
            if (S.type == 4) {
                if (S.fp3 && readstate_ < 0) S.fp3->close();
                readstate_ = 0;
            } else if (S.fp1 && S.fp1->eof()) {
                S.fp1->close();
                if (S.fp2) S.fp2->close();
            } else if (S.fp2 && S.fp2->eof()) {
                S.fp2->close();
                if (S.fp1) S.fp1->close();
            }
            i = next_valid(i);
            libNo = (int)i;
            if (i < nl && cfg_.libs[i].rd_len_cutoff > 0) max_len_ = std::min(cfg_.libs[i].rd_len_cutoff, all_);
            else max_len_ = all_;
            if (!long_ && i != prevLib && readNumBack < n_solexa) { // insert size bookkeeping (:1092-1103), pairs only
                const LibInfo& P = cfg_.libs[prevLib];
                pes.push_back(PeInfo{P.avg_ins, n_solexa, P.rank, P.pair_num_cut});
                readNumBack = n_solexa;
            }
            if (i >= nl) return false;
            open(i);
            Lib& T = st_[i];
            std::string nm;
            if (T.type == 1) {
                readseq1by1(*T.fp1, seq, nm, len, -1, max_len_, ll(), str_);
                readseq1by1(*T.fp2, seq, nm, len, -1, max_len_, ll(), str_);
            } else if (T.type == 3 || T.type == 5) readseq1by1(*T.fp1, seq, nm, len, -1, max_len_, ll(), str_);
        }
        Lib& T = st_[i];
        const int rev = cfg_.libs[i].reverse;
        std::string nm;
        if (T.type == 1 || T.type == 2) {
            LineIn& f = T.paired == 1 ? *T.fp1 : *T.fp2;
            if (T.type == 1) readseq1by1(f, seq, nm, len, 1, max_len_, ll(), str_);
            else read1seqfq(f, seq, len, max_len_, ll(), str_);
            if (rev) reverse2k(seq, len);
            if (T.paired == 1) {
                T.paired = 2;
                if (len > 0 || !T.fp1->eof()) { n_solexa++; return true; }
                return next(seq, len, libNo, type);
            }
            T.paired = 1;
            n_solexa++;
            return true;
        }
        if (T.type == 6) read1seqfq(*T.fp1, seq, len, max_len_, ll(), str_);
        else if (T.type == 4) read_bam(T, seq, len, type, cfg_.libs[i].asm_flag);
        else readseq1by1(*T.fp1, seq, nm, len, 1, max_len_, ll(), str_);
        if (rev) reverse2k(seq, len);
        if ((T.type != 4 && (len > 0 || !T.fp1->eof())) || (T.type == 4 && (len > 0 || readstate_ >= 0))) { n_solexa++; return true; }
        return next(seq, len, libNo, type);
    }

private:
    struct Lib {
        int type = 1, index = 0, paired = 0;
        std::unique_ptr<LineIn> fp1, fp2;
        std::unique_ptr<BamIn> fp3;
    };
    int ll() const { return line_len_ > 0 ? line_len_ : max_len_ + 1; }
    size_t files_of(const LibInfo& L, int type) const {
        switch (type) {
        case 1: return L.f1.size(); case 2: return L.q1.size(); case 3: return L.p.size(); case 4: return L.b.size();
        case 5: return L.f.size(); case 6: return L.q.size();
        }
        return 0;
    }
    // nextValidIndex (readseq1by1.c:595-674).  pair = 1, asm_ctg = 0: libs with asm_flags 2 or 3; f1/f2, q1/q2, p, b (no f=, q=).
    // pair = 0, asm_ctg = 4: libs with asm_flags 4; f= and q= files after those
    size_t next_valid(size_t i) {
        const int last = long_ ? 6 : 4;
        while (i < cfg_.libs.size()) {
            const LibInfo& L = cfg_.libs[i];
            if (long_ ? L.asm_flag != 4 : (L.asm_flag != 2 && L.asm_flag != 3)) { i++; continue; }
            Lib& S = st_[i];
            if (S.type <= last && (size_t)S.index < files_of(L, S.type)) return i;
            if (S.type < last) { S.type++; S.index = 0; }
            else i++;
        }
        return i;
    }
    static std::string trim(std::string s) { while (!s.empty() && s.back() == ' ') s.pop_back(); return s; }
    void open(size_t i) {                                           // openFileInLib (readseq1by1.c:736-786)
        const LibInfo& L = cfg_.libs[i];
        Lib& S = st_[i];
        auto say = [](const std::string& f) { fprintf(stderr, "Import reads from file:\n %s\n", f.c_str()); };
        if (S.type == 1 || S.type == 2) {
            const std::string a = trim(S.type == 1 ? L.f1[S.index] : L.q1[S.index]), b = trim(S.type == 1 ? L.f2[S.index] : L.q2[S.index]);
            say(a); say(b);
            S.fp1.reset(new LineIn(a));
            S.fp2.reset(new LineIn(b));
            S.paired = 1;
        } else if (S.type == 3 || S.type == 5 || S.type == 6) {
            const std::string a = trim(S.type == 3 ? L.p[S.index] : S.type == 5 ? L.f[S.index] : L.q[S.index]);
            say(a);
            S.fp1.reset(new LineIn(a));
            S.paired = 0;
        } else if (S.type == 4) {
            const std::string a = trim(L.b[S.index]);
            say(a);
            S.fp3.reset(new BamIn(a));
            S.paired = 0;
        }
        S.index++;
    }
    // read1seqbam's pairing state machine (readseq1by1.c:470-575); map reads only asm_flags 2 / 3 libs, so no record is skipped
    void read_bam(Lib& T, char* seq, int& len, int& type, int) {
        type = 0;
        uint16_t flag = 0;
        int n = 0;
        readstate_ = T.fp3->next(flag, seq, n, max_len_) ? 0 : -1;
        if (readstate_ >= 0) {
            if (flag & 0x0200) {
                switch (bam_state_) { case -3: bam_state_ = -2; break; case -2: bam_state_ = 0; break; case -1: bam_state_ = 2; break; default: bam_state_ = -3; }
            } else {
                switch (bam_state_) { case -3: bam_state_ = -1; break; case -2: bam_state_ = 1; break; case -1: bam_state_ = 3; break; default: bam_state_ = -3; }
            }
            if (bam_state_ == 3) bam_state_ = -3;
            else if (bam_state_ == 0 || bam_state_ == 1 || bam_state_ == 2) { bam_state_ = -3; type = -1; }
        } else bam_state_ = -3;
        len = n;
    }
    const LibConfig& cfg_;
    int all_, max_len_, line_len_;
    bool long_;
    std::vector<Lib> st_;
    std::vector<char> str_;
    int readstate_ = 0, bam_state_ = -3;
};

// ---- output: gzip members deflated by worker threads, written in order ----
class GzOut {
public:
    GzOut(const std::string& path, int workers) : workers_(std::max(1, workers)) {
        fp_ = fopen(path.c_str(), "wb");
        if (!fp_) { fprintf(stderr, "Cannot open %s. Now exit to system...\n", path.c_str()); exit(-1); }
    }
    ~GzOut() { close(); }
    std::string buf;
    void maybe_flush() { if (buf.size() >= (4u << 20)) submit(); }
    void close() {
        if (!fp_) return;
        if (!buf.empty()) submit();
        while (!q_.empty()) drain_one();
        fclose(fp_);
        fp_ = nullptr;
    }
    double t_deflate = 0;

private:
    static std::string member(std::string text) {
        z_stream z;
        memset(&z, 0, sizeof z);
        std::string out;
        if (deflateInit2(&z, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return out;
        out.resize(deflateBound(&z, (uLong)text.size()) + 64);
        z.next_in = (Bytef*)text.data();
        z.avail_in = (uInt)text.size();
        z.next_out = (Bytef*)&out[0];
        z.avail_out = (uInt)out.size();
        deflate(&z, Z_FINISH);
        out.resize(z.total_out);
        deflateEnd(&z);
        return out;
    }
    void submit() {
        if ((int)q_.size() >= workers_) drain_one();
        q_.push_back(std::async(std::launch::async, member, std::move(buf)));
        buf = std::string();
    }
    void drain_one() {
        const double t0 = now_s();
        const std::string m = q_.front().get();
        t_deflate += now_s() - t0;
        q_.pop_front();
        fwrite(m.data(), 1, m.size(), fp_);
    }
    FILE* fp_ = nullptr;
    int workers_;
    std::deque<std::future<std::string>> q_;
};

template <typename T> void put_bin(std::string& s, const T& v) { s.append((const char*)&v, sizeof v); }
void put_i64(std::string& s, long long v) { char t[24]; s.append(t, (size_t)snprintf(t, sizeof t, "%lld", v)); }

struct Options {
    std::string cfg, prefix;
    int K = 0, p = 8, small_k = 0;
    bool fill = false;
};

// ---- the batch: reads as read, their packed images, the kernel's answers and recordAlldgn (prlRead2Ctg.c:627-725) ----
struct Batch {
    std::vector<char> seq;                 // read r at r * row
    std::vector<int32_t> len, ins;
    size_t row = 0, n = 0;
};

struct Recorder {
    const Options& o;
    int K;
    GzOut& on_ctg;
    GzOut& in_gap;
    GzOut* short_gap;                      // -f
    GzOut* pe_on_ctg;                      // -f
    std::vector<char> rc1;                 // rcSeq[1] of prlRead2Ctg.c: calloc'ed, maxReadLen bytes
    long long readCounter = 0, mapCounter = 0, readsInGap = 0;
    std::vector<uint32_t> ctg;
    std::vector<int32_t> pos;
    std::vector<uint8_t> orien, fp;

    // the 2-bit image of read t, packed into rcSeq[1] with masked writes (writeChar2tightString, seq.c:81-107): the bits past the read
    // are what the buffer held before
    void tight(const Batch& b, size_t t) {
        const char* s = b.seq.data() + t * b.row;
        const int L = b.len[t];
        for (int i = 0; i < L; i++) {
            char& byte = rc1[(size_t)(i / 4)];
            const int sh = 6 - 2 * (i % 4);
            byte = (char)((byte & ~(3 << sh)) | ((s[i] & 3) << sh));
        }
    }
    void output1read(const Batch& b, size_t t, char orient, int dh) {          // output1read_gz (:427-451)
        const int L = b.len[t];
        readsInGap++;
        tight(b, t);
        std::string& s = in_gap.buf;
        put_bin(s, L); put_bin(s, (int32_t)ctg[t]); put_bin(s, pos[t]);
        s.append(rc1.data(), (size_t)(L / 4 + 1));
        in_gap.maybe_flush();
        if (o.fill && b.ins[t] < 2000 && L > 0) {
            std::string& x = short_gap->buf;
            char h[128];
            x.append(h, (size_t)snprintf(h, sizeof h, ">%d\t%d\t%d\t%c\t%d\t%d\n", L, (int)ctg[t], pos[t], orient, b.ins[t], dh));
            const char* q = b.seq.data() + t * b.row;
            for (int i = 0; i < L; i++) x.push_back("ACTG"[q[i] & 3]);
            x.push_back('\n');
            short_gap->maybe_flush();
        }
    }
    void pe_on_contig(const Batch& b, size_t t) {                             // getPEreadOnContig (:487-523)
        if (!(b.ins[t] < 2000 && b.ins[t] == b.ins[t - 1])) return;
        std::string& s = pe_on_ctg->buf;
        for (size_t r : {t - 1, t}) {
            put_bin(s, b.len[r]); put_bin(s, (int32_t)ctg[r]); put_bin(s, pos[r]); put_bin(s, (char)orien[r]); put_bin(s, b.ins[r]);
            tight(b, r);
            s.append(rc1.data(), (size_t)(b.len[r] / 4 + 1));
        }
        pe_on_ctg->maybe_flush();
    }
    void read_in_gap(const Batch& b, size_t t, int ins, bool read_one) {      // getReadIngap (:548-591)
        const size_t r1 = read_one ? t : t - 1, r2 = read_one ? t + 1 : t;
        const size_t mate = read_one ? r2 : r1, me = read_one ? r1 : r2;
        const char orient = orien[mate] == '+' ? '-' : '+';
        ctg[me] = ctg[mate];
        pos[me] = pos[mate] + ins - b.len[me];
        output1read(b, me, orient, read_one ? 1 : 2);
    }
    void record(const Batch& b, const std::vector<MapOut>& out, int p) {
        const size_t n = b.n;
        ctg.resize(n); pos.resize(n); fp.resize(n);
        if (orien.size() < n) orien.resize(n, 0);
        // orienArray is only written for a read that maps (:336-360): an unmapped read's entry keeps whatever the same place of an earlier
        // batch left (0 from calloc at first), and recordAlldgn does read it for the mate of a footprinted read (:711-720)
        for (size_t t = 0; t < n; t++) {
            ctg[t] = out[t].ctg; pos[t] = out[t].pos; fp[t] = out[t].footprint;
            if (out[t].ctg) orien[t] = out[t].orien;
        }
        // what the chop stage left in rcSeq[1]: thread 0 (reads t % p == 0 of K + 1 bases or more) reverse-complements each of its reads
        // into it (chopKmer4read, :153-231 -- the buffer is rcSeq[threadID] with threadID = 1 for thread 0)
        for (size_t t = 0; t < n; t += (size_t)p) {
            const int L = b.len[t];
            if (L < K + 1) continue;
            const char* s = b.seq.data() + t * b.row;
            for (int i = 0; i < L; i++) rc1[(size_t)i] = (char)(s[L - 1 - i] ^ 2);
        }
        std::string& oc = on_ctg.buf;
        char line[96];
        for (size_t t = 0; t < n; t++) {
            readCounter++;
            bool rd1gap = false, rd2gap = false;
            const int32_t id = (int32_t)ctg[t];
            if (t % 2 == 1) {                                      // (ctgIdArray is unsigned: `< 1` is `== 0`)
                if (ctg[t] < 1u && ctg[t - 1] > 0u) { read_in_gap(b, t, b.ins[t], false); rd2gap = true; }
                else if (ctg[t] > 0u && ctg[t - 1] < 1u) { read_in_gap(b, t - 1, b.ins[t - 1], true); rd1gap = true; }
                else if (ctg[t] > 0u && ctg[t - 1] > 0u && o.fill) pe_on_contig(b, t);
            }
            if (id < 1) continue;
            mapCounter++;
            oc.append(line, (size_t)snprintf(line, sizeof line, "%lld\t%u\t%d\t%c\n", readCounter, ctg[t], pos[t], (char)orien[t]));
            if (t % 2 == 0) continue;
            // a footprinted read that is mapped leaves its image in readInGap too.  locate1read (:389-425) is never reached: footprint is
            // only set for a read whose contig was chosen, and a chosen contig has an id of 1 or more (ids are getID of a name > 0 or an
            // ordinal from 1, and getTwinCtg of an id >= 1 stays >= 1 for ContigIndex's pairs), so `ctgIdArray[t] < 1` never holds there
            if (fp[t - 1] && !rd1gap) output1read(b, t - 1, orien[t] == '+' ? '-' : '+', 1);
            if (fp[t] && !rd2gap) output1read(b, t, orien[t - 1] == '+' ? '-' : '+', 2);
        }
        on_ctg.maybe_flush();
    }
};

int getMinOverlap(const std::string& prefix, int& maxReadLen) {                 // map.c:47-77
    FILE* fp = fopen((prefix + ".preGraphBasic").c_str(), "r");
    int overlaplen = 23;
    if (!fp) return overlaplen;
    char line[1024], ch;
    int num_kmer, minr, maxn;
    while (fgets(line, sizeof line, fp)) {
        if (line[0] == 'V') sscanf(line + 6, "%d %c %d", &num_kmer, &ch, &overlaplen);
        else if (line[0] == 'M') sscanf(line, "MaxReadLen %d MinReadLen %d MaxNameLen %d", &maxReadLen, &minr, &maxn);
    }
    fclose(fp);
    return overlaplen;
}

// <prefix>.contig as prlContig2nodes reads it (prlHashCtg.c:345-440): readseqpar's maximum length (readseq1by1.c:225-277: strlen - 1 of
// every fgets piece of 4949 characters) caps every contig (readseq1by1 with maxReadLen = maxCtgLen); contigs shorter than K + 2 are
// left out; a contig's id is the number its name starts with, else its ordinal
void read_contigs(const std::string& prefix, int K, MapContigs& c, long long& num_seq) {
    const std::string name = prefix + ".contig";
    int maxCtgLen = 10;
    {
        FILE* fp = fopen(name.c_str(), "r");
        if (!fp) { fprintf(stderr, "Cannot open %s. Now exit to system...\n", name.c_str()); exit(-1); }
        char str[5000];
        int n = 0, minCtg = 1000;
        long long k = -1;
        while (fgets(str, 4950, fp)) {
            if (str[0] == '>') {
                if (k >= 0) { maxCtgLen = std::max(maxCtgLen, n); minCtg = std::min(minCtg, n); }
                n = 0;
                k++;
            } else n += (int)strlen(str) - 1;
        }
        maxCtgLen = std::max(maxCtgLen, n);
        num_seq = k + 1;
        fclose(fp);
    }
    LineIn in(name);
    std::vector<char> seq((size_t)maxCtgLen + 8), str;
    std::string next_name;
    int len = 0;
    readseq1by1(in, seq.data(), next_name, len, -1, maxCtgLen, 5000, str);
    auto getID = [](const std::string& s) { return !s.empty() && s[0] >= '0' && s[0] <= '9' ? atoi(s.c_str()) : 0; };
    long long i = 0;
    c.off.assign(1, 0);
    while (!in.eof()) {
        const int contigId = getID(next_name);
        readseq1by1(in, seq.data(), next_name, len, 1, maxCtgLen, 5000, str);
        ++i;
        if (len < K + 1 || len < K + 2) continue;
        c.id.push_back(contigId > 0 ? (uint32_t)contigId : (uint32_t)i);
        c.len.push_back(len);
        const size_t w0 = c.words.size(), nw = ((size_t)len + 31) / 32;
        c.words.resize(w0 + nw, 0);
        for (int j = 0; j < len; j++) c.words[w0 + (size_t)(j >> 5)] |= (uint64_t)(seq[(size_t)j] & 3) << (62 - 2 * (j & 31));
        c.off.push_back(c.words.size());
        c.n_kmers += (uint64_t)(len - K + 1);
    }
    c.words.resize(c.words.size() + 8, 0);                          // read_kmer reads NW + 1 words from a k-mer's first word on
}

// basicContigInfo (prlRead2Ctg.c:727-770)
void contig_info(const std::string& prefix, std::vector<int32_t>& len, std::vector<int8_t>& bal) {
    const std::string name = prefix + ".ContigIndex";
    FILE* fp = fopen(name.c_str(), "r");
    if (!fp) { fprintf(stderr, "Cannot open %s. Now exit to system...\n", name.c_str()); exit(-1); }
    char line[1024];
    int num_all = 0, num_long = 0, index, length, bal_ed;
    if (fgets(line, sizeof line, fp)) sscanf(line + 8, "%d %d", &num_all, &num_long);
    fprintf(stderr, "%d edge(s) in the graph.\n", num_all);
    len.assign((size_t)std::max(num_all, 0) + 2, 0);
    bal.assign(len.size(), 1);
    if (!fgets(line, sizeof line, fp)) line[0] = 0;
    num_long = 0;
    auto put = [&](int at, int l, int b) {
        if ((size_t)at >= len.size()) { len.resize((size_t)at + 1, 0); bal.resize((size_t)at + 1, 1); }
        len[(size_t)at] = l;
        bal[(size_t)at] = (int8_t)b;
    };
    while (fgets(line, sizeof line, fp)) {
        if (sscanf(line, "%d %d %d", &index, &length, &bal_ed) < 3) continue;
        put(++num_long, length, bal_ed + 1);
        if (index != num_long) fprintf(stderr, "BasicContigInfo: %d vs %d.\n", index, num_long);
        if (bal_ed == 0) continue;
        put(++num_long, length, -bal_ed + 1);
    }
    fclose(fp);
}

// prlLongRead2Ctg (prlRead2Ctg.c:1080-1298) with recordLongRead and output1read (:456-492, :612-625): the libraries with asm_flags=4,
// a read at a time, a batch through the engine, the footprinted reads into <prefix>.longReadInGap (and .RlongReadInGap with -f).
// Returns longReadLen (0: no such library, nothing done, no file), -1 on an engine error.
int long_pass(const LibConfig& cfg, const Options& o, int K, MapEngine& eng, bool wave, int max_rd_len) {
    int long_len = 0;                                               // getMaxLongReadLen (lib.c:43-68)
    bool has = false;
    for (const LibInfo& L : cfg.libs)
        if (L.asm_flag == 4) { has = true; long_len = std::max(long_len, L.rd_len_cutoff); }
    if (!has) return 0;
    if (long_len <= 0) long_len = max_rd_len;
    const int max_len_all = std::max(max_rd_len, long_len);         // maxReadLen4all
    fprintf(stderr, "In file: %s, long read len %d, max name len %d.\n", o.cfg.c_str(), long_len, 256);
    long long maxReadNum = 100000000LL / (long_len - K + 1 > 0 ? long_len - K + 1 : 1);
    maxReadNum = maxReadNum % 2 == 0 ? maxReadNum : maxReadNum - 1;
    // (this repository's own guard: the reference divides by longReadLen - K + 1 as it is and goes on)
    if (long_len < K || maxReadNum < 2) { fprintf(stderr, "Long read length %d is too small for K = %d.\n", long_len, K); return -1; }
    FILE* fp1 = fopen((o.prefix + ".longReadInGap").c_str(), "wb");
    FILE* fp2 = o.fill ? fopen((o.prefix + ".RlongReadInGap").c_str(), "w") : nullptr;
    if (!fp1 || (o.fill && !fp2)) { fprintf(stderr, "Cannot open %s.longReadInGap. Now exit to system...\n", o.prefix.c_str()); exit(-1); }
    LibReader rd(cfg, max_len_all, long_len, true);
    Batch b;
    b.row = (size_t)max_len_all + 8;
    const size_t cap = (size_t)std::min<long long>(maxReadNum, 1 << 12);
    b.seq.resize(cap * b.row);
    b.len.resize(cap);
    std::vector<char> rc1((size_t)max_len_all + 8, 0);              // rcSeq[1]: zeroed once, then what the chop and the writes leave
    std::vector<uint64_t> words, off, koff;
    std::vector<MapOut> res;
    std::string out1, out2;
    long long readCounter = 0, readsInGap = 0;
    double t_read = 0, t_pack = 0, t_map = 0, t_rec = 0;
    const double k0 = eng.t_kernel, c0 = eng.t_copy;
    int align_len = 0, libNo = 0, prevLibNo = -1, type = 0;
    auto flush = [&]() -> int {
        const double a = now_s();
        words.clear(); off.resize(b.n); koff.resize(b.n + 1);
        koff[0] = 0;
        for (size_t t = 0; t < b.n; t++) {
            const int L = b.len[t];
            off[t] = words.size();
            const size_t w0 = words.size();
            words.resize(w0 + ((size_t)L + 31) / 32, 0);
            const char* s = b.seq.data() + t * b.row;
            for (int j = 0; j < L; j++) words[w0 + (size_t)(j >> 5)] |= (uint64_t)(s[j] & 3) << (62 - 2 * (j & 31));
            koff[t + 1] = koff[t] + (L >= K + 1 ? (uint64_t)(L - K + 1) : 0);
        }
        words.resize(words.size() + 8, 0);
        res.resize(b.n);
        const double c = now_s();
        const int e = eng.map(MapBatch{words.data(), words.size(), off.data(), b.len.data(), koff.data(), b.n}, align_len, res.data(), nullptr, wave);
        if (e) { fprintf(stderr, "map: %s\n", pg_last_error()); return e; }
        const double d = now_s();
        // chop thread 0's reverse complements (reads t % p == 0 of K + 1 bases or more), then recordLongRead in read order
        for (size_t t = 0; t < b.n; t += (size_t)o.p) {
            const int L = b.len[t];
            if (L < K + 1) continue;
            const char* s = b.seq.data() + t * b.row;
            for (int i = 0; i < L; i++) rc1[(size_t)i] = (char)(s[L - 1 - i] ^ 2);
        }
        for (size_t t = 0; t < b.n; t++) {
            readCounter++;
            if (!res[t].footprint) continue;
            readsInGap++;
            const char* s = b.seq.data() + t * b.row;
            const int L = b.len[t];
            for (int i = 0; i < L; i++) {                           // writeChar2tightString (seq.c:81-107)
                char& byte = rc1[(size_t)(i / 4)];
                const int sh = 6 - 2 * (i % 4);
                byte = (char)((byte & ~(3 << sh)) | ((s[i] & 3) << sh));
            }
            put_bin(out1, L); put_bin(out1, (int32_t)res[t].ctg); put_bin(out1, res[t].pos);
            out1.append(rc1.data(), (size_t)(L / 4 + 1));
            if (o.fill && L > 0) {                                  // insSizeArray[t] = 18 < 2000 always
                char h[128];
                out2.append(h, (size_t)snprintf(h, sizeof h, ">%d\t%d\t%d\t%c\t%d\t%d\n", L, (int)res[t].ctg, res[t].pos, (char)res[t].orien, 18, 0));
                for (int i = 0; i < L; i++) out2.push_back("ACTG"[s[i] & 3]);
                out2.push_back('\n');
            }
        }
        fwrite(out1.data(), 1, out1.size(), fp1);
        if (fp2) fwrite(out2.data(), 1, out2.size(), fp2);
        out1.clear(); out2.clear();
        t_pack += c - a; t_map += d - c; t_rec += now_s() - d;
        b.n = 0;
        return 0;
    };
    double r0 = now_s();
    for (;;) {
        if (b.n == b.len.size()) {
            const size_t nc = std::min<size_t>((size_t)maxReadNum, b.len.size() * 2);
            b.seq.resize(nc * b.row); b.len.resize(nc);
        }
        int L = 0;
        if (!rd.next(b.seq.data() + b.n * b.row, L, libNo, type)) break;
        if (type == -1) {                                           // a bad BAM pair goes back (:1184-1196)
            if (b.n) b.n--;
            rd.n_solexa -= 2;
            continue;
        }
        b.len[b.n] = L;
        if (libNo != prevLibNo) {                                   // :1198-1204
            prevLibNo = libNo;
            align_len = std::max(cfg.libs[(size_t)libNo].map_len, 35);
            fprintf(stderr, "Map_len %d.\n", align_len);
        }
        b.n++;
        if ((long long)b.n == maxReadNum) {
            t_read += now_s() - r0;
            if (flush()) { fclose(fp1); if (fp2) fclose(fp2); return -1; }
            r0 = now_s();
        }
    }
    t_read += now_s() - r0;
    if (b.n) {
        if (flush()) { fclose(fp1); if (fp2) fclose(fp2); return -1; }
        fprintf(stderr, "Output %lld out of %lld (%.1f)%% reads in gaps.\n", readsInGap, readCounter, (float)readsInGap / readCounter * 100);
    }
    fclose(fp1);
    if (fp2) fclose(fp2);
    fprintf(stderr, "%d reads deleted.\n", 0);
    if (env_user("PG_HOST_VERBOSE"))
        fprintf(stderr, "[map long] %s kernel: %lld reads, parse %.3fs, pack %.3fs, map %.3fs (kernel %.6fs, copies %.3fs), record %.3fs; "
                        "reads done in passes %llu, distinct ids %llu\n",
                wave ? "wave" : "lane", readCounter, t_read, t_pack, t_map, eng.t_kernel - k0, eng.t_copy - c0, t_rec,
                (unsigned long long)eng.n_passes, (unsigned long long)eng.n_ids);
    return long_len;
}

int run_map(int argc, char** argv, bool mer127) {
    const double t_start = now_s();
    fprintf(stderr, "\n********************\nMap\n********************\n\n");
    Options o;
    bool in = false, out = false;
    optind = 1;
    fprintf(stderr, "Parameters: map ");
    auto usage = [&]() {
        fprintf(stderr, "\nmap -s configFile -g inputGraph [-f] [-p n_cpu -k kmer_R2C] [-h contig_total_length]\n");
        fprintf(stderr, "  -s <string>        configFile: the config file of solexa reads\n");
        fprintf(stderr, "  -g <string>        inputGraph: prefix of input graph file names\n");
        fprintf(stderr, "  -h (optional)      total length of contigs for init hash table. [1024]\n");
        fprintf(stderr, "  -f (optional)      output gap related reads in map step for using SRkgf to fill gap, [NO]\n");
        fprintf(stderr, "  -p <int>           n_cpu: number of cpu for use, [8]\n");
        fprintf(stderr, "  -k <int>           kmer_R2C(min 13, max %d): kmer size used for mapping read to contig, [K]\n", mer127 ? 127 : 63);
    };
    int copt;
    while ((copt = getopt(argc, argv, "s:g:K:p:k:h:f")) != EOF) {
        switch (copt) {
        case 's': fprintf(stderr, "-s %s ", optarg); in = true; o.cfg = optarg; break;
        case 'g': fprintf(stderr, "-g %s ", optarg); out = true; o.prefix = optarg; break;
        case 'K': fprintf(stderr, "-K %s ", optarg); o.K = atoi(optarg); break;
        case 'p': fprintf(stderr, "-p %s ", optarg); o.p = atoi(optarg); break;
        case 'k': fprintf(stderr, "-k %s ", optarg); o.small_k = atoi(optarg); break;
        case 'h': fprintf(stderr, "-h %s ", optarg); break;                   // a sizing hint of the reference's k-mer sets only
        case 'f': o.fill = true; fprintf(stderr, "-f "); break;
        default:
            if (!in || !out) { usage(); return 1; }
        }
    }
    fprintf(stderr, "\n\n");
    if (!in || !out) { usage(); return 1; }
    if (o.p < 1) { fprintf(stderr, "-p must be 1 or more.\n"); return 1; }
    int mrl_graph = 0;
    int K = getMinOverlap(o.prefix, mrl_graph);                                 // -K is overwritten here, as in map.c:102
    const int kmax = mer127 ? 128 : 64;
    if (o.small_k > 12 && o.small_k < kmax && o.small_k % 2 == 1) K = o.small_k;
    if (K < 1 || K > (mer127 ? 127 : 63)) { fprintf(stderr, "Kmer size %d is not supported by this build.\n", K); return 1; }
    fprintf(stderr, "Kmer size: %d.\n", K);

    const LibConfig cfg = parse_lib_config(o.cfg.c_str());
    const bool long_on = env_on(env_user("SOAPDENOVO2_AMD_MAP_LONG"));
    bool long_wave = false;
    if (const char* e = long_on ? env_user("SOAPDENOVO2_AMD_MAP_LONG_KERNEL") : nullptr) {
        long_wave = !strcmp(e, "wave");
        if (!long_wave && strcmp(e, "lane")) { fprintf(stderr, "SOAPDENOVO2_AMD_MAP_LONG_KERNEL is lane or wave, not %s.\n", e); return 1; }
    }
    if (!long_on)
        for (const LibInfo& L : cfg.libs)
            if (L.asm_flag == 4) {
                fprintf(stderr, "Long-read libraries (asm_flags=4) are not supported by this map stage; run the reference binary for this "
                                "config.  Nothing was written.  SOAPDENOVO2_AMD_MAP_LONG=1 turns the long-read pass on.\n");
                return 2;
            }
    fprintf(stderr, "Contig length cutoff: %d.\n", K + 2);

    // 1. the index
    const double t0 = now_s();
    MapContigs contigs;
    long long num_seq = 0;
    read_contigs(o.prefix, K, contigs, num_seq);
    std::vector<int32_t> clen;
    std::vector<int8_t> cbal;
    fprintf(stderr, "\n%lld contig(s) read, %zu of %d bases or more.\n", num_seq, contigs.len.size(), K + 2);
    const int nw = mer127 ? 4 : 2;
    std::unique_ptr<MapEngine> eng;
    if (env_on(env_user("SOAPDENOVO2_AMD_MAP_HOST"))) eng = map_engine_host(K, nw);
    else {
        int device = 0;
        if (const char* e = env_user("SOAPDENOVO2_AMD_DEVICE")) device = atoi(e);
        if (const char* e = env_user("SOAPDENOVO2_AMD_DEVICES")) if (*e) device = atoi(e);      // the first of the list
        eng = map_engine_device(device, K, nw);
        if (!eng) { fprintf(stderr, "map: %s\n", pg_last_error()); return 1; }
    }
    const double t1 = now_s();
    const int max_all = cfg.max_rd_len ? cfg.max_rd_len : 100;                  // prlRead2Ctg.c:796-799: maxReadLen
    fprintf(stderr, "In file: %s, max seq len %d, max name len %d\n", o.cfg.c_str(), max_all, 256);
    contig_info(o.prefix, clen, cbal);
    int rc = eng->build(contigs, clen.data(), cbal.data(), (uint32_t)clen.size());
    if (rc) { fprintf(stderr, "map: %s\n", pg_last_error()); return 1; }
    { MapContigs none; std::swap(contigs, none); }
    const double t2 = now_s();
    fprintf(stderr, "Time spent on graph construction: %ds.\n\n", (int)(t2 - t0));

    // 5. the long reads (map.c:129-133).  What they leave for the short pass is maxReadLen4all (prlRead2Ctg.c:803-806), which .peGrads'
    // header prints.  The short reads themselves stay cut at max_rd_len: the reference would cut them at maxReadLen4all, into buffers of
    // max_rd_len bytes, so a longer short read is past what it defines (and rows of maxReadLen4all bytes for every short read of a
    // batch would be gigabytes for nothing)
    int max_len_all = max_all;
    if (long_on) {
        const int long_len = long_pass(cfg, o, K, *eng, long_wave, max_all);
        if (long_len < 0) return 1;
        max_len_all = std::max(max_all, long_len);
        fprintf(stderr, "Time spent on aligning long reads: %ds.\n\n", (int)(now_s() - t2));
    }
    const double t2b = now_s();

    // 2. - 4. the reads
    long long maxReadNum = 100000000LL / (max_all - K + 1);
    maxReadNum = maxReadNum % 2 == 0 ? maxReadNum : maxReadNum - 1;
    if (maxReadNum < 2) { fprintf(stderr, "max_rd_len %d is too small for K = %d.\n", max_all, K); return 1; }
    const int workers = 4;
    GzOut on_ctg(o.prefix + ".readOnContig.gz", workers), in_gap(o.prefix + ".readInGap.gz", workers);
    std::unique_ptr<GzOut> short_gap, pe_on;
    if (o.fill) {
        short_gap.reset(new GzOut(o.prefix + ".shortreadInGap.gz", workers));
        pe_on.reset(new GzOut(o.prefix + ".PEreadOnContig.gz", workers));
    }
    Recorder rec{o, K, on_ctg, in_gap, short_gap.get(), pe_on.get(), std::vector<char>((size_t)max_all + 8, 0)};
    on_ctg.buf += "read\tcontig\tpos\n";
    LibReader rd(cfg, max_all, max_all);
    Batch b;
    b.row = (size_t)max_all + 8;
    const size_t cap = (size_t)std::min<long long>(maxReadNum, 1 << 22);
    b.seq.resize(cap * b.row);
    b.len.resize(cap);
    b.ins.resize(cap);
    std::vector<uint64_t> words, off, koff;
    std::vector<MapOut> res;
    double t_read = 0, t_pack = 0, t_map = 0, t_rec = 0;
    int align_len = 0, insSize = 0, libNo = 0, prevLibNo = -1, type = 0;
    auto flush = [&]() -> int {
        const double a = now_s();
        words.clear(); off.resize(b.n); koff.resize(b.n + 1);
        koff[0] = 0;
        for (size_t t = 0; t < b.n; t++) {
            const int L = b.len[t];
            off[t] = words.size();
            const size_t w0 = words.size();
            words.resize(w0 + ((size_t)L + 31) / 32, 0);
            const char* s = b.seq.data() + t * b.row;
            for (int j = 0; j < L; j++) words[w0 + (size_t)(j >> 5)] |= (uint64_t)(s[j] & 3) << (62 - 2 * (j & 31));
            koff[t + 1] = koff[t] + (L >= K + 1 ? (uint64_t)(L - K + 1) : 0);
        }
        words.resize(words.size() + 8, 0);
        res.resize(b.n);
        const double c = now_s();
        const int e = eng->map(MapBatch{words.data(), words.size(), off.data(), b.len.data(), koff.data(), b.n}, align_len, res.data());
        if (e) { fprintf(stderr, "map: %s\n", pg_last_error()); return e; }
        const double d = now_s();
        rec.record(b, res, o.p);
        t_pack += c - a; t_map += d - c; t_rec += now_s() - d;
        b.n = 0;
        return 0;
    };
    double r0 = now_s();
    for (;;) {
        if (b.n == b.len.size()) {                                  // the buffers grow up to maxReadNum
            const size_t nc = std::min<size_t>((size_t)maxReadNum, b.len.size() * 2);
            b.seq.resize(nc * b.row); b.len.resize(nc); b.ins.resize(nc);
        }
        int L = 0;
        if (!rd.next(b.seq.data() + b.n * b.row, L, libNo, type)) break;
        if (type == -1) {                                           // a bad pair goes back (:875-888)
            if (b.n) b.n--;
            rd.n_solexa -= 2;
            continue;
        }
        b.len[b.n] = L;
        if (libNo != prevLibNo) {                                   // :890-904
            prevLibNo = libNo;
            insSize = cfg.libs[(size_t)libNo].avg_ins;
            align_len = cfg.libs[(size_t)libNo].map_len;
            align_len = insSize > 1000 ? std::max(align_len, 35) : std::max(align_len, 32);
            fprintf(stderr, "Current insert size is %d, map_len is %d.\n", insSize, align_len);
        }
        b.ins[b.n] = insSize;
        if (insSize > 1000) align_len = std::max(align_len, L / 2 + 1);
        b.n++;
        if ((long long)b.n == maxReadNum) {
            t_read += now_s() - r0;
            if ((rc = flush())) return 1;
            r0 = now_s();
        }
    }
    t_read += now_s() - r0;
    const bool tail = b.n > 0;
    if (tail && (rc = flush())) return 1;
    const double t3 = now_s();
    if (tail) {
        fprintf(stderr, "\nTotal reads         %lld\n", rec.readCounter);
        fprintf(stderr, "Reads in gaps       %lld\n", rec.readsInGap);
        fprintf(stderr, "Ratio               %.1f%%\n", (float)rec.readsInGap / rec.readCounter * 100);
    }
    fprintf(stderr, "Reads on contigs    %lld\n", rec.mapCounter);
    fprintf(stderr, "Ratio               %.1f%%\n", (float)rec.mapCounter / rec.readCounter * 100);
    on_ctg.close();
    {
        FILE* fo2 = fopen((o.prefix + ".peGrads").c_str(), "w");
        if (!fo2) { fprintf(stderr, "Cannot open %s.peGrads. Now exit to system...\n", o.prefix.c_str()); exit(-1); }
        fprintf(fo2, "grads&num: %d\t%lld\t%d\n", (int)rd.pes.size(), rd.n_solexa, max_len_all);
        if (!rd.pes.empty()) fprintf(stderr, "%d pe insert size, the largest boundary is %lld.\n\n", (int)rd.pes.size(), rd.pes.back().PE_bound);
        else fprintf(stderr, "No paired reads found.\n");
        for (const PeInfo& p : rd.pes) fprintf(fo2, "%d\t%lld\t%d\t%d\n", p.insertS, p.PE_bound, p.rank, p.pair_num_cut);
        fclose(fo2);
    }
    in_gap.close();
    if (o.fill) { short_gap->close(); pe_on->close(); }
    const double t4 = now_s();
    fprintf(stderr, "Time spent on aligning reads: %ds.\n\n", (int)(t3 - t2b));
    if (env_user("PG_HOST_VERBOSE"))
        fprintf(stderr, "[map] contigs %.3fs, index %.3fs (device %.3fs), reads: parse %.3fs, pack %.3fs, map %.3fs (kernel %.3fs, copies %.3fs), "
                        "record %.3fs, files %.3fs (deflate waits %.3fs); whole stage %.3fs\n",
                t1 - t0, t2 - t1, eng->t_index, t_read, t_pack, t_map, eng->t_kernel, eng->t_copy, t_rec, t4 - t3,
                on_ctg.t_deflate + in_gap.t_deflate, t4 - t_start);
    fprintf(stderr, "Overall time spent on alignment: %dm.\n\n", (int)(t4 - t_start) / 60);
    return 0;
}

}  // namespace
}  // namespace pg

// map.c:94 call_align -- the 63-mer build
extern "C" int call_align(int argc, char** argv) { return pg::run_map(argc, argv, false); }
// map.c:94 call_align -- the 127-mer build
extern "C" int call_align_127mer(int argc, char** argv) { return pg::run_map(argc, argv, true); }
