// ktrim.hpp -- reads trimmed to their longest solid stretch on the k-mer index (pg_kindex_trim, include/soapdenovo2_amd.h section 3;
// DESIGN.md §12).  The reference has no such stage: the spectrum corrector SOAPdenovo2's pipeline runs in front of pregraph ends with a
// trimming pass of this kind.  The rule, for a read of nk = max(0, len - K + 1) k-mers (k-mer j = bases [j, j + K)):
//   solid(j)   as the corrector's (kcor_solid_word, kcorrect.hpp): the index's answer for the canonical k-mer j is not 0 and its coverage
//              is >= min_cov
//   span       the longest run of consecutive solid k-mers, the leftmost one among equals.  A run of n k-mers from k-mer j0 on is the
//              bases j0 .. j0 + n + K - 2: start = j0, len = n + K - 1.  No solid k-mer, or no k-mer at all: start = 0, len = 0
//   span word  start | len << 32
//   kept       len >= min_len (min_len >= K, so a read without a solid k-mer is never kept)
// A kept read comes out as the words pg_pack_read gives for its span: ceil(len / 32) words, the first base in the most significant bits,
// pad bits zero, and it has len - K + 1 k-mers, all of them solid.
//
// One piece of PG_HD code for the kernels (kindex_kernels.hip: ktrim_span_kernel, ktrim_span_rows_kernel, the scan's kernels and
// ktrim_pack_kernel) and the host twin (ktrim_host.cpp): the run tracker, the three counts the scan sums, and one output word.  The
// tracker keeps the current run's length and the best run in registers and is written with selects: a store under a branch inside
// map_roll's loop is what became scratch in the corrector.
#pragma once
#include "kcorrect.hpp"

namespace pg {

struct KtrimRun {
    int cur;                       // solid k-mers that end the walk so far
    int best_start, best;          // the longest run met, the first one of that length
};

PG_HD KtrimRun ktrim_run_none() { return KtrimRun{0, 0, 0}; }

// k-mer j, the next one of the walk, is solid or not
PG_HD void ktrim_run_add(KtrimRun& t, bool solid, int j) {
    t.cur = solid ? t.cur + 1 : 0;
    const bool better = t.cur > t.best;            // (strictly: the leftmost of equal runs stays)
    t.best_start = better ? j - t.cur + 1 : t.best_start;
    t.best = better ? t.cur : t.best;
}

PG_HD uint64_t ktrim_span_word(const KtrimRun& t, int K) {
    return t.best ? (uint64_t)(uint32_t)t.best_start | (uint64_t)(uint32_t)(t.best + K - 1) << 32 : 0;
}

PG_HD uint32_t ktrim_start(uint64_t span) { return (uint32_t)span; }
PG_HD uint32_t ktrim_len(uint64_t span) { return (uint32_t)(span >> 32); }

// the span of a read whose k-mers are looked up in one table: kidx_stretch's walk, one slot read a k-mer
template <int NW>
PG_HD uint64_t ktrim_span_probe(const uint64_t* rd, int nk, int K, const uint64_t* tab, uint64_t mask, uint32_t min_cov) {
    KtrimRun t = ktrim_run_none();
    map_roll<NW>(rd, 0, nk, K, [&](const Kmer<NW>& ck, bool, int j) { ktrim_run_add(t, kcor_solid_word(kidx_find<NW>(tab, mask, ck), min_cov), j); });
    return ktrim_span_word(t, K);
}

// the span of a read whose answers lie in a row (an index cut over ranks: the merged rows)
PG_HD uint64_t ktrim_span_row(const uint64_t* row, int nk, int K, uint32_t min_cov) {
    KtrimRun t = ktrim_run_none();
    for (int j = 0; j < nk; j++) ktrim_run_add(t, kcor_solid_word(row[j], min_cov), j);
    return ktrim_span_word(t, K);
}

// What the scan sums over the reads, all from the span word: kept reads, their output words, their k-mers, and the bases that go --
// those cut off a kept read and all of a dropped one.  A read's own length is nk + K - 1; a read without k-mers (shorter than K) has
// no length in a ragged batch's layout and counts as 0 bases, in a uniform batch too.  (KidxCounts: kindex.hpp, the scan's type)
PG_HD KidxCounts ktrim_counts(uint64_t span, int nk, int K, uint32_t min_len) {
    const uint32_t len = ktrim_len(span);
    const bool kept = len >= min_len;
    const uint64_t given = nk > 0 ? (uint64_t)nk + (uint64_t)K - 1 : 0;
    return KidxCounts{{kept ? 1u : 0u, kept ? (uint64_t)((len + 31) / 32) : 0, kept ? (uint64_t)(len - (uint32_t)K + 1) : 0, given - (kept ? len : 0)}};
}

// Output word q of a kept read: bases start + 32 q .. of the source read rd, a 128-bit funnel of two source words.  The second word is
// loaded whether the shift needs it or not: it is the read's next word, the next read's first, or -- behind the batch's last read --
// one of the nw + 1 readable tail words.  The last word's pad bits are cleared
PG_HD uint64_t ktrim_pack_word(const uint64_t* rd, uint32_t start, uint32_t len, uint64_t q) {
    const uint64_t s = (uint64_t)(start >> 5) + q;
    const int sh = 2 * (int)(start & 31);
    const uint64_t a = rd[s], b = rd[s + 1];
    const uint64_t w = sh ? a << sh | b >> (64 - sh) : a;
    const uint64_t rem = (uint64_t)len - 32 * q;   // bases of this word and the ones behind it
    return rem < 32 ? w & ~(~0ull >> (2 * rem)) : w;
}

// the device engine (kindex_kernels.hip): one table or cut over ranks alike.  d_packed_out null: spans only
int ktrim_device_trim(::pg_kindex* ix, const KidxBatch& b, uint32_t min_cov, uint32_t min_len, uint64_t* d_span, uint64_t* d_packed_out,
                      uint64_t* d_word_off_out, uint64_t* d_kmer_base_out, uint64_t* d_src_out, uint64_t* d_totals, void* stream);
// the last trim's milliseconds from its events, after waiting for its end: span (a cut index: probes and merge included), scan, pack, all of it
int ktrim_device_times(::pg_kindex* ix, double out[4]);

}  // namespace pg
