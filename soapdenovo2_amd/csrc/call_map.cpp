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
// Both passes are one loop (run_pass: batches, the BAM take-back, pack_batch, the engine, the timers); a pass brings what it does when
// the library changes (on_read) and its recorder (Recorder, LongRecorder; both write through RcSeq1, the model of rcSeq[1]).  The 2-bit
// packer and the BAM record reader are host_reads.cpp's.
//   6. the index lives on the first GPU of SOAPDENOVO2_AMD_DEVICES unless it is cut over all the ranks of that list by key (map_owner,
//      map_index.hpp; ShardedDeviceMapEngine, map_kernels.hip): with SOAPDENOVO2_AMD_MAP_SHARD=1 and two ranks or more listed, or when
//      the plan (pg_host_map_plan, map_plan.cpp) says that the table does not fit the first GPU and more ranks are listed.  The plan is
//      asked once the contigs are counted and before anything is allocated or written; an index that fits nowhere ends the command there
// Not here: without that switch a config with a long-read library (asm_flags=4) is refused before anything is written.
// SOAPDENOVO2_AMD_MAP_HOST=1 runs the host twin of the index and the read kernels instead (the CPU tests), cut the same way.
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <deque>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "device_list.hpp"
#include "env.hpp"
#include "host_reads.hpp"
#include "map_index.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

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
        else if (T.type == 4) read_bam(T, seq, len, type);
        else readseq1by1(*T.fp1, seq, nm, len, 1, max_len_, ll(), str_);
        if (rev) reverse2k(seq, len);
        if ((T.type != 4 && (len > 0 || !T.fp1->eof())) || (T.type == 4 && (len > 0 || readstate_ >= 0))) { n_solexa++; return true; }
        return next(seq, len, libNo, type);
    }

private:
    struct Lib {
        int type = 1, index = 0, paired = 0;
        std::unique_ptr<LineIn> fp1, fp2;
        std::unique_ptr<BamReader> fp3;
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
            S.fp3.reset(new BamReader(a));
            S.paired = 0;
        }
        S.index++;
    }
    // b=: one record (host_reads.hpp's BamReader) through read1seqbam's pairing step; type = -1: the pair is taken back.  map reads only
    // asm_flags 2 / 3 libs and the long pass asm_flags 4, so no record is skipped
    void read_bam(Lib& T, char* seq, int& len, int& type) {
        type = 0;
        uint16_t flag = 0;
        readstate_ = T.fp3->next(flag, (uint8_t*)seq, len, max_len_) ? 0 : -1;
        if (readstate_ < 0) { bam_state_ = -3; return; }
        const BamPair pair = bam_pair_step(bam_state_, (flag & 0x0200) != 0);
        bam_state_ = pair.state;
        if (pair.take_back) type = -1;
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
    std::vector<char> seq;                 // read r at r * row; a row has 8 bytes past the longest read (pack_codes)
    std::vector<int32_t> len, ins;
    size_t row = 0, n = 0;
    const char* read(size_t t) const { return seq.data() + t * row; }
    void grow(size_t cap) { seq.resize(cap * row); len.resize(cap); ins.resize(cap); }
};

// the batch as the engines take it (MapBatch): pg_pack_read's layout, koff[r] = k-mers of the reads before r
void pack_batch(const Batch& b, int K, std::vector<uint64_t>& words, std::vector<uint64_t>& off, std::vector<uint64_t>& koff) {
    words.clear(); off.resize(b.n); koff.resize(b.n + 1);
    koff[0] = 0;
    for (size_t t = 0; t < b.n; t++) {
        const int L = b.len[t];
        off[t] = words.size();
        words.resize(off[t] + ((size_t)L + 31) / 32);
        pack_codes((const uint8_t*)b.read(t), L, words.data() + off[t]);
        koff[t + 1] = koff[t] + (L >= K + 1 ? (uint64_t)(L - K + 1) : 0);
    }
    words.resize(words.size() + 8, 0);                              // read_kmer reads NW + 1 words from a k-mer's first word on
}

// rcSeq[1] of prlRead2Ctg.c: calloc'ed once, maxReadLen bytes, then what the chop stage and the writers leave in it
struct RcSeq1 {
    std::vector<char> buf;
    explicit RcSeq1(int max_len) : buf((size_t)max_len + 8, 0) {}
    // the chop stage: thread 0 (reads t % p == 0 of K + 1 bases or more) reverse-complements each of its reads into it (chopKmer4read,
    // :153-231 -- the buffer is rcSeq[threadID] with threadID = 1 for thread 0)
    void chop(const Batch& b, int K, int p) {
        for (size_t t = 0; t < b.n; t += (size_t)p) {
            const int L = b.len[t];
            if (L < K + 1) continue;
            const char* s = b.read(t);
            for (int i = 0; i < L; i++) buf[(size_t)i] = (char)(s[L - 1 - i] ^ 2);
        }
    }
    // the 2-bit image of read t, packed into it with masked writes (writeChar2tightString, seq.c:81-107): L / 4 + 1 bytes, the bits past
    // the read are what the buffer held before
    const char* tight(const Batch& b, size_t t) {
        const char* s = b.read(t);
        const int L = b.len[t];
        for (int i = 0; i < L; i++) {
            char& byte = buf[(size_t)(i / 4)];
            const int sh = 6 - 2 * (i % 4);
            byte = (char)((byte & ~(3 << sh)) | ((s[i] & 3) << sh));
        }
        return buf.data();
    }
};

// the text record of .shortreadInGap and .RlongReadInGap (output1read_gz / output1read, :427-492)
void put_text_read(std::string& x, const Batch& b, size_t t, int ctg, int pos, char orient, int dh) {
    const int L = b.len[t];
    char h[128];
    x.append(h, (size_t)snprintf(h, sizeof h, ">%d\t%d\t%d\t%c\t%d\t%d\n", L, ctg, pos, orient, b.ins[t], dh));
    const char* q = b.read(t);
    for (int i = 0; i < L; i++) x.push_back("ACTG"[q[i] & 3]);
    x.push_back('\n');
}

struct Recorder {
    const Options& o;
    int K;
    GzOut& on_ctg;
    GzOut& in_gap;
    GzOut* short_gap;                      // -f
    GzOut* pe_on_ctg;                      // -f
    RcSeq1 rc1;
    long long readCounter = 0, mapCounter = 0, readsInGap = 0;
    std::vector<uint32_t> ctg;
    std::vector<int32_t> pos;
    std::vector<uint8_t> orien, fp;

    void output1read(const Batch& b, size_t t, char orient, int dh) {          // output1read_gz (:427-451)
        const int L = b.len[t];
        readsInGap++;
        std::string& s = in_gap.buf;
        put_bin(s, L); put_bin(s, (int32_t)ctg[t]); put_bin(s, pos[t]);
        s.append(rc1.tight(b, t), (size_t)(L / 4 + 1));
        in_gap.maybe_flush();
        if (o.fill && b.ins[t] < 2000 && L > 0) {
            put_text_read(short_gap->buf, b, t, (int)ctg[t], pos[t], orient, dh);
            short_gap->maybe_flush();
        }
    }
    void pe_on_contig(const Batch& b, size_t t) {                             // getPEreadOnContig (:487-523)
        if (!(b.ins[t] < 2000 && b.ins[t] == b.ins[t - 1])) return;
        std::string& s = pe_on_ctg->buf;
        for (size_t r : {t - 1, t}) {
            put_bin(s, b.len[r]); put_bin(s, (int32_t)ctg[r]); put_bin(s, pos[r]); put_bin(s, (char)orien[r]); put_bin(s, b.ins[r]);
            s.append(rc1.tight(b, r), (size_t)(b.len[r] / 4 + 1));
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
        rc1.chop(b, K, p);
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
        c.words.resize(w0 + nw);
        pack_codes((const uint8_t*)seq.data(), len, c.words.data() + w0);
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

// recordLongRead and output1read (prlRead2Ctg.c:456-492, :612-625): the footprinted reads into <prefix>.longReadInGap and, with -f,
// .RlongReadInGap (plain files, written a batch at a time)
struct LongRecorder {
    const Options& o;
    int K;
    RcSeq1 rc1;
    FILE* fp1;
    FILE* fp2;                             // -f
    long long readCounter = 0, readsInGap = 0;
    std::string out1, out2;
    LongRecorder(const Options& opt, int k, int max_len) : o(opt), K(k), rc1(max_len) {
        fp1 = fopen((o.prefix + ".longReadInGap").c_str(), "wb");
        fp2 = o.fill ? fopen((o.prefix + ".RlongReadInGap").c_str(), "w") : nullptr;
        if (!fp1 || (o.fill && !fp2)) { fprintf(stderr, "Cannot open %s.longReadInGap. Now exit to system...\n", o.prefix.c_str()); exit(-1); }
    }
    ~LongRecorder() { close(); }
    void close() {
        if (fp1) fclose(fp1);
        if (fp2) fclose(fp2);
        fp1 = fp2 = nullptr;
    }
    void record(const Batch& b, const std::vector<MapOut>& res, int p) {
        rc1.chop(b, K, p);
        for (size_t t = 0; t < b.n; t++) {
            readCounter++;
            if (!res[t].footprint) continue;
            readsInGap++;
            const int L = b.len[t];
            put_bin(out1, L); put_bin(out1, (int32_t)res[t].ctg); put_bin(out1, res[t].pos);
            out1.append(rc1.tight(b, t), (size_t)(L / 4 + 1));
            if (o.fill && L > 0) put_text_read(out2, b, t, (int)res[t].ctg, res[t].pos, (char)res[t].orien, 0);      // insSizeArray[t] = 18 < 2000 always
        }
        fwrite(out1.data(), 1, out1.size(), fp1);
        if (fp2) fwrite(out2.data(), 1, out2.size(), fp2);
        out1.clear(); out2.clear();
    }
};

// ---- one pass over the libraries: the loop of prlRead2Ctg (:865-945) and prlLongRead2Ctg (:1182-1250) ----
struct PassTimes {
    double parse = 0, pack = 0, map = 0, record = 0;
    bool tail = false;                     // the reads ended inside a batch (the reference's summaries are printed behind that batch only)
};

// Reads come from rd one by one into batches of maxReadNum (the buffers grow up to that from first_cap); a batch is packed, mapped with
// the ALIGNLEN that stands after its last read, and handed to record(batch, answers).  on_read(lib, first, L, align_len) is the pass's
// own part: called for every read that is kept (L bases, of library lib; first = the library has changed), it sets ALIGNLEN and returns
// the read's insert size.  Returns 0, or -1 after an engine error (reported).
template <typename OnRead, typename Record>
int run_pass(const LibConfig& cfg, LibReader& rd, int max_len, size_t first_cap, long long maxReadNum, int K, MapEngine& eng, bool wave,
             OnRead on_read, Record record, PassTimes& tm) {
    Batch b;
    b.row = (size_t)max_len + 8;
    b.grow(std::min((size_t)maxReadNum, first_cap));
    std::vector<uint64_t> words, off, koff;
    std::vector<MapOut> res;
    int align_len = 0, libNo = 0, prevLibNo = -1, type = 0;
    auto flush = [&]() -> int {
        const double a = now_s();
        pack_batch(b, K, words, off, koff);
        res.resize(b.n);
        const double c = now_s();
        const int e = eng.map(MapBatch{words.data(), words.size(), off.data(), b.len.data(), koff.data(), b.n}, align_len, res.data(), nullptr, wave);
        if (e) { fprintf(stderr, "map: %s\n", pg_last_error()); return -1; }
        const double d = now_s();
        record(b, res);
        tm.pack += c - a; tm.map += d - c; tm.record += now_s() - d;
        b.n = 0;
        return 0;
    };
    double r0 = now_s();
    for (;;) {
        if (b.n == b.len.size()) b.grow(std::min((size_t)maxReadNum, b.len.size() * 2));
        int L = 0;
        if (!rd.next(b.seq.data() + b.n * b.row, L, libNo, type)) break;
        if (type == -1) {                                           // a bad BAM pair goes back (:875-888, :1184-1196)
            if (b.n) b.n--;
            rd.n_solexa -= 2;
            continue;
        }
        b.len[b.n] = L;
        b.ins[b.n] = on_read(cfg.libs[(size_t)libNo], libNo != prevLibNo, L, align_len);
        prevLibNo = libNo;
        b.n++;
        if ((long long)b.n == maxReadNum) {
            tm.parse += now_s() - r0;
            if (flush()) return -1;
            r0 = now_s();
        }
    }
    tm.parse += now_s() - r0;
    tm.tail = b.n > 0;
    return tm.tail ? flush() : 0;
}

// prlLongRead2Ctg (prlRead2Ctg.c:1080-1298): the libraries with asm_flags=4, a read at a time (run_pass), the footprinted reads to LongRecorder.
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
    LongRecorder rec(o, K, max_len_all);
    LibReader rd(cfg, max_len_all, long_len, true);
    const double k0 = eng.t_kernel, c0 = eng.t_copy;
    auto on_read = [](const LibInfo& lib, bool first, int, int& align_len) {              // :1198-1206
        if (first) {
            align_len = std::max(lib.map_len, 35);
            fprintf(stderr, "Map_len %d.\n", align_len);
        }
        return 18;
    };
    PassTimes tm;
    const int e = run_pass(cfg, rd, max_len_all, 1 << 12, maxReadNum, K, eng, wave, on_read,
                           [&](const Batch& b, const std::vector<MapOut>& res) { rec.record(b, res, o.p); }, tm);
    rec.close();
    if (e) return -1;
    if (tm.tail)
        fprintf(stderr, "Output %lld out of %lld (%.1f)%% reads in gaps.\n", rec.readsInGap, rec.readCounter, (float)rec.readsInGap / rec.readCounter * 100);
    fprintf(stderr, "%d reads deleted.\n", 0);
    if (env_user("PG_HOST_VERBOSE"))
        fprintf(stderr, "[map long] %s kernel: %lld reads, parse %.3fs, pack %.3fs, map %.3fs (kernel %.6fs, copies %.3fs), record %.3fs; "
                        "reads done in passes %llu, distinct ids %llu\n",
                wave ? "wave" : "lane", rec.readCounter, tm.parse, tm.pack, tm.map, eng.t_kernel - k0, eng.t_copy - c0, tm.record,
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
    // 6. where the index goes: one table on the first device, or cut over the listed ranks
    const bool host = env_on(env_user("SOAPDENOVO2_AMD_MAP_HOST"));
    const std::vector<int> devices = parse_device_list(env_user("SOAPDENOVO2_AMD_DEVICES"));
    int device = 0;
    if (const char* e = env_user("SOAPDENOVO2_AMD_DEVICE")) device = atoi(e);
    if (!devices.empty()) device = devices[0];
    const int n_listed = (int)devices.size();
    bool sharded = env_on(env_user("SOAPDENOVO2_AMD_MAP_SHARD")) && n_listed >= 2;
    // the test hook SOAPDENOVO2_AMD_MAP_BUDGET_MB: the most a rank's table may take, so that the does-not-fit paths run at test sizes
    // (where the batch buffers outweigh any index); with it the host twin is planned too, against no device
    const char* hook = env_test("SOAPDENOVO2_AMD_MAP_BUDGET_MB");
    if (!host || hook) {
        uint64_t device_bytes = ~0ull >> 2, plan[12];
        if (!host && map_device_free_bytes(device, &device_bytes) != PG_OK) { fprintf(stderr, "map: %s\n", pg_last_error()); return 1; }
        const uint64_t table_cap = hook ? (uint64_t)atoll(hook) << 20 : ~0ull;
        auto fits = [&](int n) {                                      // a batch holds at most 1e8 k-mers (prlRead2Ctg.c:814)
            pg_host_map_plan(contigs.n_kmers, mer127 ? 1 : 0, n, 100000000ull, device_bytes, plan);
            return plan[9] != 0 && plan[0] <= table_cap;
        };
        if (!sharded && !fits(1) && n_listed >= 2) sharded = true;
        if (sharded && n_listed > DEVICE_LIST_MAX_RANKS) {           // (a longer list is no matter to a run on the first device)
            fprintf(stderr, "map: SOAPDENOVO2_AMD_DEVICES names %d ranks, the most an index is cut over is %d.\n", n_listed, DEVICE_LIST_MAX_RANKS);
            return 1;
        }
        const int n_ranks = sharded ? n_listed : 1;
        if (!fits(n_ranks)) {
            const uint64_t table = plan[0], peak = plan[7], budget = plan[8], whole = plan[10];
            int fewest = (int)plan[11];                               // the plan's own answer; under the hook's cap, the same search with it
            if (hook) {
                fewest = 0;
                for (int n = 1; n <= DEVICE_LIST_MAX_RANKS && !fewest; n++) if (fits(n)) fewest = n;
            }
            fprintf(stderr, "map: the contig index does not fit: %llu k-mers are %llu bytes as one table; over %d rank(s) a rank's table is %llu bytes "
                            "(%llu with its buffers) and the budget of a device is %llu bytes",
                    (unsigned long long)contigs.n_kmers, (unsigned long long)whole, n_ranks, (unsigned long long)table, (unsigned long long)peak,
                    (unsigned long long)budget);
            if (hook) fprintf(stderr, "; SOAPDENOVO2_AMD_MAP_BUDGET_MB caps a rank's table at %llu bytes", (unsigned long long)table_cap);
            if (fewest) fprintf(stderr, ".  %d ranks would hold it: list them in SOAPDENOVO2_AMD_DEVICES.  Nothing was written.\n", fewest);
            else fprintf(stderr, ".  No number of ranks up to %d holds it.  Nothing was written.\n", DEVICE_LIST_MAX_RANKS);
            return 1;
        }
    }
    std::unique_ptr<MapEngine> eng;
    if (host) eng = sharded ? map_engine_host_sharded(n_listed, K, nw) : map_engine_host(K, nw);
    else eng = sharded ? map_engine_device_sharded(devices.data(), n_listed, K, nw) : map_engine_device(device, K, nw);
    if (!eng) { fprintf(stderr, "map: %s\n", pg_last_error()); return 1; }
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
    Recorder rec{o, K, on_ctg, in_gap, short_gap.get(), pe_on.get(), RcSeq1(max_all)};
    on_ctg.buf += "read\tcontig\tpos\n";
    LibReader rd(cfg, max_all, max_all);
    int insSize = 0;
    auto on_read = [&insSize](const LibInfo& lib, bool first, int L, int& align_len) {   // :890-904
        if (first) {
            insSize = lib.avg_ins;
            align_len = insSize > 1000 ? std::max(lib.map_len, 35) : std::max(lib.map_len, 32);
            fprintf(stderr, "Current insert size is %d, map_len is %d.\n", insSize, align_len);
        }
        if (insSize > 1000) align_len = std::max(align_len, L / 2 + 1);
        return insSize;
    };
    PassTimes tm;
    if (run_pass(cfg, rd, max_all, (size_t)1 << 22, maxReadNum, K, *eng, false, on_read,
                 [&](const Batch& b, const std::vector<MapOut>& res) { rec.record(b, res, o.p); }, tm)) return 1;
    const double t3 = now_s();
    if (tm.tail) {
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
                t1 - t0, t2 - t1, eng->t_index, tm.parse, tm.pack, tm.map, eng->t_kernel, eng->t_copy, tm.record, t4 - t3,
                on_ctg.t_deflate + in_gap.t_deflate, t4 - t_start);
    if (env_user("PG_HOST_VERBOSE") && !eng->ranks.empty()) {
        std::string keys, load, probe;
        char t[64];
        for (const MapEngine::Rank& r : eng->ranks) {
            const char* sep = keys.empty() ? "" : " / ";
            keys += sep + std::to_string(r.keys);
            snprintf(t, sizeof t, "%s%.3f", sep, (double)r.keys / (double)r.slots); load += t;
            snprintf(t, sizeof t, "%s%.6f", sep, r.t_probe); probe += t;
        }
        fprintf(stderr, "[map] index sharded over %zu ranks: keys %s, load %s; probe %s s, merge %.6fs, decide %.6fs\n", eng->ranks.size(),
                keys.c_str(), load.c_str(), probe.c_str(), eng->t_merge, eng->t_decide);
    }
    fprintf(stderr, "Overall time spent on alignment: %dm.\n\n", (int)(t4 - t_start) / 60);
    return 0;
}

}  // namespace
}  // namespace pg

// map.c:94 call_align -- the 63-mer build
extern "C" int call_align(int argc, char** argv) { return pg::run_map(argc, argv, false); }
// map.c:94 call_align -- the 127-mer build
extern "C" int call_align_127mer(int argc, char** argv) { return pg::run_map(argc, argv, true); }
