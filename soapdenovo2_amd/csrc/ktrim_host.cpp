// ktrim_host.cpp -- pg_kindex_trim's C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index, one table or a
// list of -1s): the rule of ktrim.hpp over host memory, the scan as a serial loop.  What the CPU tests run, and the device path's
// yardstick.  A file of its own beside kindex_host.cpp: a program that links the index's host half alone with stubs for its device
// engine (tests/kindex_sharded_asan.cpp) keeps linking.
#include <string>

#include "../../include/soapdenovo2_amd.h"
#include "kindex.hpp"
#include "ktrim.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

// the host twin of pg_kindex_trim: every read's span (every k-mer asks its owner's table: kidx_host_find), then the kept reads one after
// the other -- the serial form of the scan -- and their words through ktrim_pack_word
template <int NW>
void ktrim_host_trim(const pg_kindex* ix, const KidxBatch& b, uint32_t min_cov, uint32_t min_len, uint64_t* out_span, uint64_t* packed_out,
                     uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* src_out, uint64_t* out_totals) {
    const int K = ix->K;
    KidxCounts total{{0, 0, 0, 0}};
    for (uint64_t r = 0; r < b.n_seqs; r++) {
        const KidxSeq q = kidx_seq(b, K, r);
        KtrimRun t = ktrim_run_none();
        map_roll<NW>(q.rd, 0, q.nk, K, [&](const Kmer<NW>& ck, bool, int j) { ktrim_run_add(t, kcor_solid_word(kidx_host_find<NW>(ix, ck), min_cov), j); });
        const uint64_t span = ktrim_span_word(t, K);
        if (out_span) out_span[r] = span;
        if (!packed_out) continue;
        const KidxCounts c = ktrim_counts(span, q.nk, K, min_len);
        if (c.c[0]) {
            word_off_out[total.c[0]] = total.c[1];
            kmer_base_out[total.c[0]] = total.c[2];
            if (src_out) src_out[total.c[0]] = r;
            for (uint64_t w = 0; w < c.c[1]; w++) packed_out[total.c[1] + w] = ktrim_pack_word(q.rd, ktrim_start(span), ktrim_len(span), w);
        }
        for (int i = 0; i < KIDX_COUNTS; i++) total.c[i] += c.c[i];
    }
    if (!packed_out) return;
    kmer_base_out[total.c[0]] = total.c[2];
    for (int i = 0; i < NW + 1; i++) packed_out[total.c[1] + i] = 0;
    for (int i = 0; i < KIDX_COUNTS; i++) out_totals[i] = total.c[i];
}

}  // namespace
}  // namespace pg

extern "C" int pg_kindex_trim(pg_kindex* ix, const uint64_t* packed, uint64_t n_words, const uint64_t* word_off, const uint64_t* kmer_base,
                              uint64_t n_seqs, uint32_t uniform_len, uint64_t n_kmers, uint32_t min_cov, uint32_t min_len, uint64_t* out_span,
                              uint64_t* packed_out, uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* src_out, uint64_t* out_totals,
                              void* stream) {
    if (!ix) { pg_set_error("pg_kindex_trim: null index"); return PG_EINVAL; }
    if (!min_cov || min_len < (uint32_t)ix->K) { pg_set_error("pg_kindex_trim: min_cov is at least 1 and min_len at least K"); return PG_EINVAL; }
    if (packed_out && packed_out == packed) { pg_set_error("pg_kindex_trim: packed_out == packed: a batch is not trimmed in place"); return PG_EINVAL; }
    if (packed_out && (!word_off_out || !kmer_base_out || !out_totals)) {
        pg_set_error("pg_kindex_trim: packed_out needs word_off_out, kmer_base_out and out_totals");
        return PG_EINVAL;
    }
    if (!packed_out && !out_span) { pg_set_error("pg_kindex_trim: out_span and packed_out are both null"); return PG_EINVAL; }
    const pg::KidxBatch b{packed, word_off, kmer_base, n_seqs, uniform_len, n_words, n_kmers};
    // (an empty batch's counts are not looked at)
    if (int rc = pg::kidx_batch_args("pg_kindex_trim", ix, b, "read", n_seqs ? pg::KIDX_ARGS_KMERS | pg::KIDX_ARGS_WORDS | pg::KIDX_ARGS_TAIL : 0u)) return rc;
    if (ix->device >= 0)
        return pg::ktrim_device_trim(ix, b, min_cov, min_len, out_span, packed_out, word_off_out, kmer_base_out, src_out, out_totals, stream);
    if (!n_seqs) {
        if (packed_out) for (int i = 0; i < pg::KIDX_COUNTS; i++) out_totals[i] = 0;
        return PG_OK;
    }
    pg::kidx_with_nw(ix->nw, [&](auto nw) {
        pg::ktrim_host_trim<decltype(nw)::value>(ix, b, min_cov, min_len, out_span, packed_out, word_off_out, kmer_base_out, src_out, out_totals);
    });
    return PG_OK;
}

extern "C" int pg_kindex_trim_times(pg_kindex* ix, double out[4]) {
    if (!ix || !out) { pg_set_error("pg_kindex_trim_times: null argument"); return PG_EINVAL; }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ix->device < 0) return PG_OK;
    return pg::ktrim_device_times(ix, out);
}
