// kcorrect.hpp -- substitution errors of reads corrected against the k-mer index (pg_kindex_correct, include/soapdenovo2_amd.h
// section 3).  The reference has no such stage: SOAPdenovo2's pipeline puts a separate k-mer-spectrum corrector in front
// of pregraph.  The rule, for a read of nk = max(0, len - K + 1) k-mers (k-mer j = bases [j, j + K)):
//   solid(j)   the index's answer for the canonical k-mer j of the read as it currently stands is not 0 and its coverage is >= min_cov
//   anchor s   the first solid k-mer of the read as given.  nk == 0: KCOR_NO_KMERS, no solid k-mer: KCOR_NO_ANCHOR; the read stays as it is
//   right sweep  j = s + 1 .. nk - 1: a solid k-mer is passed; a weak one puts base p = j + K - 1 (the one that entered) on trial
//   left sweep   j = s - 1 .. 0, after the right one: the same with p = j, the first base of k-mer j
//   trial at p   for each of the three other bases x, ext(x) = the consecutive solid k-mers from j on in the sweep's direction among
//                the `full` (<= K) k-mers that hold p, with p replaced by x.  The best x is written iff ext >= min(min_run, full) and
//                it beats both others; else the sweep stops (KCOR_STOP_RIGHT / KCOR_STOP_LEFT) and what was fixed stays.
//   limit        a weak k-mer met with fixes == max_fixes ends the sweep with KCOR_LIMIT and no trial; both sweeps share the count
// The two sweeps touch disjoint bases and k-mers, so only the limit couples them.
//
// One piece of PG_HD code for the kernel (kindex_kernels.hip: kcor_kernel) and the host twin (kindex_host.cpp): kcor_read works on the
// read's own words of the OUTPUT batch, in memory -- nothing holds the read in an array indexed at run time.  A sweep going down is a sweep
// going up over the reverse complement: KcorCursor keeps a k-mer as (a, b) = (the k-mer in the sweep's orientation, its reverse
// complement), so the base on trial is always the last one of `a`, the canonical key is the smaller of the two either way, and both
// directions roll with kmer_roll.  What is not looked up: the k-mers between the anchor and the first weak one behind it (the first pass
// saw them), the k-mers a trial has just shown solid, the k-mer a trial ended on (weak, with the base that was written), and every
// k-mer below the anchor that holds no fixed base (weak as given: the anchor is the first solid one).
#pragma once
#include "kindex.hpp"

namespace pg {

constexpr uint64_t KCOR_NO_KMERS = 1ull << 8, KCOR_NO_ANCHOR = 1ull << 9, KCOR_STOP_RIGHT = 1ull << 10, KCOR_STOP_LEFT = 1ull << 11,
                   KCOR_LIMIT = 1ull << 12;
constexpr uint32_t KCOR_MAX_FIXES = 255;           // the report's fixes field is bits 7:0

struct KcorParams {
    uint32_t min_cov, max_fixes, min_run;
};

PG_HD bool kcor_solid_word(uint64_t cnt, uint32_t min_cov) { return cnt != 0 && kidx_coverage(cnt) >= min_cov; }

template <int NW>
struct KcorCursor {
    Kmer<NW> a, b;
};

template <int NW>
PG_HD bool kcor_solid(const KcorCursor<NW>& c, const uint64_t* tab, uint64_t mask, uint32_t min_cov) {
    return kcor_solid_word(kidx_find<NW>(tab, mask, kmer_less<NW>(c.a, c.b) ? c.a : c.b), min_cov);
}

// k-mer j of the read as it stands, for a sweep going up (up) or down
template <int NW>
PG_HD KcorCursor<NW> kcor_at(const uint64_t* rd, int j, int K, const Kmer<NW>& filter, bool up) {
    const Kmer<NW> word = read_kmer<NW>(rd, j, K, filter), bal = kmer_rc<NW>(word, K);
    return up ? KcorCursor<NW>{word, bal} : KcorCursor<NW>{bal, word};
}

// the base that enters when the sweep steps to k-mer j, in the sweep's orientation
PG_HD int kcor_entering(const uint64_t* rd, int j, int K, bool up) { return up ? read_base(rd, j + K - 1) : read_base(rd, j) ^ 2; }

// the last base of c.a (the first of c.b, complemented) becomes code xo
template <int NW>
PG_HD void kcor_replace(KcorCursor<NW>& c, int xo, int K) {
    const int topw = NW - 1 - (2 * (K - 1)) / 64, tops = (2 * (K - 1)) % 64;
    c.a.w[NW - 1] = (c.a.w[NW - 1] & ~3ull) | (uint64_t)xo;
#pragma unroll
    for (int i = 0; i < NW; i++) {                 // (masks, not an `if` around the word: that became an array in scratch indexed by topw)
        const uint64_t clear = i == topw ? 3ull << tops : 0, set = i == topw ? (uint64_t)(xo ^ 2) << tops : 0;
        c.b.w[i] = (c.b.w[i] & ~clear) | set;
    }
}

PG_HD void kcor_write_base(uint64_t* rd, int p, int x) {
    const int sh = 62 - 2 * (p & 31);
    rd[p >> 5] = (rd[p >> 5] & ~(3ull << sh)) | ((uint64_t)x << sh);
}

// One sweep from k-mer j on (weak_first: k-mer j is known to be weak).  fixes is shared by the two sweeps; returns the flags it raised
template <int NW>
PG_HD uint64_t kcor_sweep(uint64_t* rd, int nk, int K, const uint64_t* tab, uint64_t mask, const KcorParams& pr, int j, bool up,
                          bool weak_first, uint32_t& fixes) {
    if (j < 0 || j >= nk) return 0;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const int dir = up ? 1 : -1;
    KcorCursor<NW> cur = kcor_at<NW>(rd, j, K, filter, up);
    bool weak = weak_first;
    for (;;) {                                     // cur = k-mer j as the read stands
        if (!weak && kcor_solid<NW>(cur, tab, mask, pr.min_cov)) {
            j += dir;
            if (j < 0 || j >= nk) return 0;
            kmer_roll<NW>(cur.a, cur.b, kcor_entering(rd, j, K, up), K, filter);
            continue;
        }
        if (fixes == pr.max_fixes) return KCOR_LIMIT;
        // the trial: the k-mers that hold base p are j, j + dir, .. (`full` of them); the count for a base ends at the first weak one
        const int full = up ? (nk - j < K ? nk - j : K) : (j + 1 < K ? j + 1 : K);
        const int now = (int)(cur.a.w[NW - 1] & 3);
        int best = -1, second = -1, best_xo = 0;
        for (int d = 1; d < 4; d++) {
            const int xo = (now + d) & 3;
            KcorCursor<NW> t = cur;
            kcor_replace<NW>(t, xo, K);
            int ext = 0;
            while (kcor_solid<NW>(t, tab, mask, pr.min_cov)) {
                if (++ext == full) break;
                kmer_roll<NW>(t.a, t.b, kcor_entering(rd, j + dir * ext, K, up), K, filter);
            }
            if (ext > best) { second = best; best = ext; best_xo = xo; }
            else if (ext > second) second = ext;
        }
        const int need = (int)pr.min_run < full ? (int)pr.min_run : full;
        if (best < need || best == second) return up ? KCOR_STOP_RIGHT : KCOR_STOP_LEFT;
        kcor_write_base(rd, up ? j + K - 1 : j, up ? best_xo : best_xo ^ 2);
        fixes++;
        // k-mers j .. j + dir (best - 1) are solid now.  The next one was the trial's last lookup when best < full (weak, with this
        // base); below the anchor it is weak anyway: it holds no base that was changed and was weak as given
        j += dir * best;
        if (j < 0 || j >= nk) return 0;
        weak = best < full || !up;
        cur = kcor_at<NW>(rd, j, K, filter, up);
    }
}

// One read: rd = its words in the output batch (already a copy of the input), nk its k-mers.  Returns the report word
template <int NW>
PG_HD uint64_t kcor_read(uint64_t* rd, int nk, int K, const uint64_t* tab, uint64_t mask, const KcorParams& pr) {
    if (nk <= 0) return KCOR_NO_KMERS;
    // the read as given: weak k-mers, the anchor, the first weak k-mer behind it -- kidx_stretch's walk, and all a clean read costs
    int anchor = -1, first_weak = nk;
    uint32_t n_weak = 0;
    map_roll<NW>(rd, 0, nk, K, [&](const Kmer<NW>& ck, bool, int j) {
        const bool solid = kcor_solid_word(kidx_find<NW>(tab, mask, ck), pr.min_cov);   // (selects: two stores under branches became scratch)
        n_weak += solid ? 0 : 1;
        anchor = solid && anchor < 0 ? j : anchor;
        first_weak = !solid && anchor >= 0 && first_weak == nk ? j : first_weak;
    });
    uint64_t rep = (uint64_t)n_weak << 32;
    if (!n_weak) return rep;
    if (anchor < 0) return rep | KCOR_NO_ANCHOR;
    uint32_t fixes = 0;
    rep |= kcor_sweep<NW>(rd, nk, K, tab, mask, pr, first_weak, true, true, fixes);
    rep |= kcor_sweep<NW>(rd, nk, K, tab, mask, pr, anchor - 1, false, true, fixes);
    return rep | fixes;
}

// the device engine (kindex_kernels.hip): d_out already holds the batch
int kcor_device_correct(::pg_kindex* ix, const KidxBatch& b, const KcorParams& pr, uint64_t* d_packed_out, uint64_t* d_report, void* stream);

}  // namespace pg
