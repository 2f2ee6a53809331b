// kcorrect_rows_host.cpp -- pg_kindex_correct_rows' C ABI (include/soapdenovo2_amd.h section 3) and its host twin (an index cut over a
// list of -1s): the rounds of kcorrect_rows.hpp over host memory, with the same PG_HD steps as the kernels and the rows of the twin's own
// query (pg_kindex_query_words) -- it does not call kcor_read with another lookup, so the CPU tests run the round logic itself.  A file
// of its own beside kindex_host.cpp for ktrim_host.cpp's reason: a program that links the index's host half alone with stubs for its
// device engine (tests/kindex_sharded_asan.cpp) keeps linking.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "env.hpp"
#include "kcorrect_rows.hpp"
#include "kindex.hpp"

void pg_set_error(const std::string& s);

namespace pg {

uint64_t kcor_round_trials() {
    if (const char* e = env_test("SOAPDENOVO2_AMD_KCOR_ROUND_TRIALS")) { const long long v = atoll(e); if (v > 0) return (uint64_t)v; }
    return KCOR_ROUND_TRIALS;
}

namespace {

// the host twin of kcor_device_correct_rows: the copy first, the rows of the read as given, then rounds of plan, query, decide, every
// kernel a serial loop.  Reads take a round's slots in batch order
int kcor_rows_host(pg_kindex* ix, KidxBatch b, const KcorParams& pr, uint64_t* packed_out, uint64_t* report, uint64_t* stats) {
    const int K = ix->K, tw = kcor_rows_trial_words(K);
    if (packed_out != b.packed) memmove(packed_out, b.packed, b.n_words * sizeof(uint64_t));
    b.packed = packed_out;
    std::vector<uint64_t> rows(std::max<uint64_t>(b.n_kmers, 1)), state(b.n_seqs * KCOR_ROWS_STATE_WORDS), bits(kcor_rows_bit_words(b.n_kmers, b.n_seqs));
    if (int rc = pg_kindex_query_words(ix, b.packed, b.n_words, b.word_off, b.kmer_base, b.n_seqs, b.uniform_len, b.n_kmers, 0, rows.data(), nullptr, nullptr))
        return rc;
    for (uint64_t r = 0; r < b.n_seqs; r++) {
        const KidxRow w = kidx_row(b, K, r);
        const KcorRowsRead s = kcor_rows_begin(rows.data() + w.base, w.nk, pr.min_cov, bits.data() + kcor_rows_bits_at(w.base, r));
        kcor_rows_store(&state[r * KCOR_ROWS_STATE_WORDS], s);
        if (s.phase == KCOR_ROWS_DONE && report) report[r] = kcor_rows_report(s);
    }
    const uint64_t cap = std::min<uint64_t>(kcor_round_trials(), b.n_seqs);
    std::vector<uint64_t> trial(kcor_rows_batch_words(cap, K, ix->nw)), trows(cap * 3 * (uint64_t)K), trial_read(cap);
    for (;;) {
        uint64_t claimed = 0;
        for (uint64_t r = 0; r < b.n_seqs; r++) {
            uint64_t* st = &state[r * KCOR_ROWS_STATE_WORDS];
            KcorRowsRead s = kcor_rows_load(st);
            if (s.phase == KCOR_ROWS_DONE) continue;
            const KidxSeq q = kidx_seq(b, K, r);
            const bool due = kcor_rows_settle(s, q.nk, pr.max_fixes, bits.data() + kcor_rows_bits_at(q.base, r));
            if (due && claimed < cap) {            // (a read that finds no slot stays as it is and takes one in a later round)
                trial_read[claimed] = r;
                kcor_rows_trial_write(q.rd, q.nk, K, s, trial.data() + claimed * 3 * (uint64_t)tw);
                claimed++;
            }
            kcor_rows_store(st, s);
            if (!due && report) report[r] = kcor_rows_report(s);
        }
        stats[3]++;                                // (where the device engine reads the claim counter back)
        if (!claimed) break;
        stats[0]++;
        stats[1] += claimed;
        stats[2] += claimed * 3 * (uint64_t)K;
        if (int rc = pg_kindex_query_words(ix, trial.data(), kcor_rows_batch_words(claimed, K, ix->nw), nullptr, nullptr, claimed * 3, (uint32_t)(2 * K - 1),
                                           claimed * 3 * (uint64_t)K, 0, trows.data(), nullptr, nullptr))
            return rc;
        for (uint64_t t = 0; t < claimed; t++) {
            const uint64_t r = trial_read[t];
            uint64_t* st = &state[r * KCOR_ROWS_STATE_WORDS];
            KcorRowsRead s = kcor_rows_load(st);
            const KidxSeq q = kidx_seq(b, K, r);
            const bool more = kcor_rows_decide(s, trows.data() + t * 3 * (uint64_t)K, packed_out + (q.rd - packed_out), q.nk, K, pr,
                                               bits.data() + kcor_rows_bits_at(q.base, r));
            kcor_rows_store(st, s);
            if (!more && report) report[r] = kcor_rows_report(s);
        }
    }
    return PG_OK;
}

}  // namespace
}  // namespace pg

extern "C" int pg_kindex_correct_rows(pg_kindex* ix, const uint64_t* packed, uint64_t n_words, const uint64_t* word_off, const uint64_t* kmer_base,
                                      uint64_t n_seqs, uint32_t uniform_len, uint64_t n_kmers, uint32_t min_cov, uint32_t max_fixes, uint32_t min_run,
                                      uint64_t* packed_out, uint64_t* out_report, void* stream) {
    if (!ix) { pg_set_error("pg_kindex_correct_rows: null index"); return PG_EINVAL; }
    for (uint64_t& s : ix->cor_stats) s = 0;
    if (!ix->cut) return pg_kindex_correct(ix, packed, word_off, kmer_base, n_seqs, uniform_len, n_words, min_cov, max_fixes, min_run, packed_out, out_report, stream);
    if (!min_cov || !min_run || max_fixes > pg::KCOR_MAX_FIXES) {
        pg_set_error("pg_kindex_correct_rows: min_cov and min_run are at least 1, max_fixes at most 255");
        return PG_EINVAL;
    }
    if (!packed_out) { pg_set_error("pg_kindex_correct_rows: null packed_out"); return PG_EINVAL; }
    if (!n_seqs) return PG_OK;
    const pg::KidxBatch b{packed, word_off, kmer_base, n_seqs, uniform_len, n_words, n_kmers};
    if (int rc = pg::kidx_batch_args("pg_kindex_correct_rows", ix, b, "read", pg::KIDX_ARGS_KMERS | pg::KIDX_ARGS_WORDS | pg::KIDX_ARGS_TAIL)) return rc;
    const pg::KcorParams pr{min_cov, max_fixes, min_run};
    if (ix->device >= 0) return pg::kcor_device_correct_rows(ix, b, pr, packed_out, out_report, stream, ix->cor_stats);
    if (!uniform_len && kmer_base[n_seqs] != n_kmers) {   // (the twin can look; a device batch's kmer_base is not read on the host)
        pg_set_error("pg_kindex_correct_rows: n_kmers does not match kmer_base[n_seqs]");
        return PG_EINVAL;
    }
    return pg::kcor_rows_host(ix, b, pr, packed_out, out_report, ix->cor_stats);
}

extern "C" int pg_kindex_correct_rows_stats(pg_kindex* ix, uint64_t out[4]) {
    if (!ix || !out) { pg_set_error("pg_kindex_correct_rows_stats: null argument"); return PG_EINVAL; }
    for (int i = 0; i < pg::KCOR_ROWS_STATS; i++) out[i] = ix->cor_stats[i];
    return PG_OK;
}
