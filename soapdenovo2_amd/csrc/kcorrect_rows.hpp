// kcorrect_rows.hpp -- the corrector's rule (kcorrect.hpp) on an index cut over ranks (pg_kindex_correct_rows, include/soapdenovo2_amd.h
// section 3; DESIGN.md §11 "On an index cut over ranks").  kcor_read chases one lookup after the other in one table; a cut index answers
// whole batches only (kidx_query_ranks: every rank probes the k-mers it owns, the rows are ORed together).  The rule itself needs no
// chain:
//   * a k-mer that holds no changed base is answered by the read as given.  Right sweep: a fix at p = j + K - 1 is held by k-mers
//     j .. j + K - 1 only, the sweep jumps over these by `best`, and the next plain lookup holds no changed base.  Left sweep: it makes
//     no plain lookup at all (every k-mer below the anchor is weak as given, and the one a trial ended on is weak with the base written)
//   * a k-mer that holds a changed base is answered inside a trial
//   * a trial's questions are fixed before any of its answers is known: for each of the three other bases, the `full` (<= K) k-mers that
//     hold p, read off the read as it stands
// So a read's correction is a short series of rounds -- plan a trial, query, decide -- with at most one trial a round and at most
// max_fixes + 2 trials in all (every accepted trial is a fix, a rejected one ends its sweep).  The steps, one piece of PG_HD code for the
// kernels (kindex_kernels.hip: kcor_rows_begin_kernel, kcor_rows_plan_kernel, kcor_rows_decide_kernel) and the host twin
// (kcorrect_rows_host.cpp):
//   begin    a lane a read over its row of the read as given: weak count, anchor, first weak k-mer behind the anchor, and a bit a k-mer
//            (solid as given) in words of the read's own -- the row buffer is reused by every later query
//   plan     a lane a read: walk over as-given solid k-mers to the next weak one, end the right sweep, start the left one, raise
//            KCOR_LIMIT; a read with a trial due takes a slot of the round and writes its three trial sequences
//   decide   a lane a trial: ext of the three bases from the trial's rows, kcor_sweep's acceptance, the base written, the state moved on
// A trial is three sequences of 2K - 1 bases, K k-mers each, with the base on trial at index K - 1: bases [j, j + 2K - 2] for the right
// sweep (ext counts rows 0 up), [j - K + 1, j + K - 1] for the left one (ext counts rows K - 1 down); only the first `full` rows count
// either way, and where the window passes the read's ends its bases are zeros, never loaded.
#pragma once
#include "kcorrect.hpp"

namespace pg {

// Trials of a round: the trial batch and its rows are cap * 3 * (packed words of 2K - 1 bases + K) * 8 bytes whatever the batch's size
// (K = 63: 4 + 63 words a sequence, 402 MiB; K = 127: 8 + 127 words, 810 MiB), and never more than a trial a read of the batch.
// SOAPDENOVO2_AMD_KCOR_ROUND_TRIALS (env_test) makes it small, so that reads wait for a slot at test sizes
constexpr uint64_t KCOR_ROUND_TRIALS = 1ull << 18;
uint64_t kcor_round_trials();

constexpr uint32_t KCOR_ROWS_DONE = 0, KCOR_ROWS_RIGHT = 1, KCOR_ROWS_LEFT = 2;
constexpr int KCOR_ROWS_STATE_WORDS = 2;           // a read's state: j | anchor << 32, and the report so far with phase and `weak` in bits 18:16
constexpr int KCOR_ROWS_STATS = 4;                 // rounds, trials, k-mers asked in trials, host waits

struct KcorRowsRead {
    int j, anchor;                 // the sweep's next k-mer; the first solid k-mer of the read as given
    uint32_t phase;                // KCOR_ROWS_*
    bool weak;                     // k-mer j is known to be weak
    uint32_t fixes, n_weak;
    uint64_t flags;
};

PG_HD KcorRowsRead kcor_rows_load(const uint64_t* st) {
    const uint64_t a = st[0], b = st[1];
    return KcorRowsRead{(int)(uint32_t)a, (int)(uint32_t)(a >> 32), (uint32_t)(b >> 16) & 3u, ((b >> 18) & 1) != 0, (uint32_t)b & 0xffu,
                        (uint32_t)(b >> 32), b & (KCOR_NO_KMERS | KCOR_NO_ANCHOR | KCOR_STOP_RIGHT | KCOR_STOP_LEFT | KCOR_LIMIT)};
}

PG_HD uint64_t kcor_rows_report(const KcorRowsRead& s) { return (uint64_t)s.n_weak << 32 | s.flags | s.fixes; }

PG_HD void kcor_rows_store(uint64_t* st, const KcorRowsRead& s) {
    st[0] = (uint64_t)(uint32_t)s.j | (uint64_t)(uint32_t)s.anchor << 32;
    st[1] = kcor_rows_report(s) | (uint64_t)s.phase << 16 | (uint64_t)(s.weak ? 1 : 0) << 18;
}

// Where read r's bits lie: a read of nk k-mers whose answers start at `base` has ceil(nk / 64) words from base / 64 + r on, which the
// next read's never reach (floor((base + nk) / 64) + 1 >= floor(base / 64) + ceil(nk / 64)); all reads fit kcor_rows_bit_words
PG_HD uint64_t kcor_rows_bits_at(uint64_t base, uint64_t r) { return (base >> 6) + r; }
PG_HD uint64_t kcor_rows_bit_words(uint64_t n_kmers, uint64_t n_seqs) { return (n_kmers >> 6) + n_seqs + 1; }

// packed words of a trial sequence, and the words of a round's trial batch with its readable tail
PG_HD int kcor_rows_trial_words(int K) { return (2 * K - 1 + 31) / 32; }
PG_HD uint64_t kcor_rows_batch_words(uint64_t trials, int K, int nw) { return trials * 3 * (uint64_t)kcor_rows_trial_words(K) + (uint64_t)nw + 1; }

// begin: the read as given.  row = its nk answers, bits = its words (kcor_rows_bits_at).  The state is left in s; a read that is
// KCOR_ROWS_DONE here has its report in kcor_rows_report(s)
PG_HD KcorRowsRead kcor_rows_begin(const uint64_t* row, int nk, uint32_t min_cov, uint64_t* bits) {
    KcorRowsRead s{0, 0, KCOR_ROWS_DONE, true, 0, 0, 0};
    if (nk <= 0) {
        s.flags = KCOR_NO_KMERS;
        return s;
    }
    int anchor = -1, first_weak = nk;
    for (int j0 = 0; j0 < nk; j0 += 64) {
        uint64_t word = 0;
        const int n = nk - j0 < 64 ? nk - j0 : 64;
        for (int i = 0; i < n; i++) {              // (selects, as in kcor_read's first pass)
            const int j = j0 + i;
            const bool solid = kcor_solid_word(row[j], min_cov);
            word |= (uint64_t)(solid ? 1 : 0) << i;
            s.n_weak += solid ? 0 : 1;
            anchor = solid && anchor < 0 ? j : anchor;
            first_weak = !solid && anchor >= 0 && first_weak == nk ? j : first_weak;
        }
        bits[j0 >> 6] = word;
    }
    if (!s.n_weak) return s;
    if (anchor < 0) {
        s.flags = KCOR_NO_ANCHOR;
        return s;
    }
    s.phase = KCOR_ROWS_RIGHT;
    s.j = first_weak;                              // (nk: every weak k-mer lies below the anchor, and the right sweep ends at once)
    s.anchor = anchor;
    return s;
}

// The moves that need no answer: true when a trial is due at k-mer s.j (s.weak is set then), false when the read is done.  Calling it
// again on its own result changes nothing
PG_HD bool kcor_rows_settle(KcorRowsRead& s, int nk, uint32_t max_fixes, const uint64_t* bits) {
    if (s.phase == KCOR_ROWS_RIGHT) {
        if (!s.weak) {                             // over the as-given solid k-mers: none of them holds a changed base
            int j = s.j;
            while (j < nk) {
                const uint64_t weak_from = ~bits[j >> 6] >> (j & 63);   // (bits past nk are 0: the walk ends there at the latest)
                if (weak_from) { j += __builtin_ctzll(weak_from); break; }
                j = (j | 63) + 1;
            }
            s.j = j < nk ? j : nk;
        }
        const bool end = s.j >= nk, limit = !end && s.fixes == max_fixes;
        s.weak = true;
        if (!end && !limit) return true;
        s.flags |= limit ? KCOR_LIMIT : 0;
        s.phase = KCOR_ROWS_LEFT;                  // every k-mer below the anchor is weak as given
        s.j = s.anchor - 1;
    }
    if (s.phase == KCOR_ROWS_LEFT) {
        const bool end = s.j < 0, limit = !end && s.fixes == max_fixes;
        if (!end && !limit) return true;
        s.flags |= limit ? KCOR_LIMIT : 0;
        s.phase = KCOR_ROWS_DONE;
    }
    return false;
}

// the base on trial and the `full` k-mers that hold it, for the sweep s is in
PG_HD int kcor_rows_base(const KcorRowsRead& s, int K) { return s.phase == KCOR_ROWS_RIGHT ? s.j + K - 1 : s.j; }
PG_HD int kcor_rows_full(const KcorRowsRead& s, int nk, int K) {
    const int have = s.phase == KCOR_ROWS_RIGHT ? nk - s.j : s.j + 1;
    return have < K ? have : K;
}

// 32 bases of a read of len bases from base `from` on (any value, in front of the read and behind it included): ktrim_pack_word's
// funnel of two words, but a word is loaded only where it is one of the read's own ceil(len / 32), and every base outside the read --
// pad bits with it -- is zero
PG_HD uint64_t kcor_rows_window_word(const uint64_t* rd, int len, int64_t from) {
    const int64_t words = ((int64_t)len + 31) >> 5, wi = from >> 5;    // (an arithmetic shift: floor for a negative `from`)
    const int sh = 2 * (int)(from & 31);
    const bool has_a = wi >= 0 && wi < words, has_b = wi + 1 >= 0 && wi + 1 < words;
    const uint64_t la = rd[has_a ? wi : 0], lb = rd[has_b ? wi + 1 : 0];       // (the read's word 0 exists: len >= K)
    const uint64_t a = has_a ? la : 0, b = has_b ? lb : 0;
    uint64_t w = sh ? a << sh | b >> (64 - sh) : a;
    const int64_t before = -from, rem = (int64_t)len - from;   // bases of this word in front of the read; bases of the read from `from` on
    w = before >= 32 ? 0 : before > 0 ? w & (~0ull >> (2 * before)) : w;
    w = rem <= 0 ? 0 : rem < 32 ? w & ~(~0ull >> (2 * rem)) : w;
    return w;
}

// plan: the three trial sequences of the trial due at s (kcor_rows_settle said so), from the read as it stands: dst = 3 sequences of
// kcor_rows_trial_words(K) words, sequence d - 1 with base (now + d) & 3 at index K - 1
PG_HD void kcor_rows_trial_write(const uint64_t* rd, int nk, int K, const KcorRowsRead& s, uint64_t* dst) {
    const int len = nk + K - 1, tw = kcor_rows_trial_words(K), p = kcor_rows_base(s, K), now = read_base(rd, p);
    const int64_t from = (int64_t)p - (K - 1);
    const int at = (K - 1) >> 5, sh = 62 - 2 * ((K - 1) & 31);
    for (int q = 0; q < tw; q++) {
        uint64_t w = kcor_rows_window_word(rd, len, from + 32 * q);
        const int rem = 2 * K - 1 - 32 * q;        // bases of the trial sequence from this word on
        w = rem < 32 ? w & ~(~0ull >> (2 * rem)) : w;
        for (int d = 1; d < 4; d++) {
            const uint64_t x = (uint64_t)((now + d) & 3);
            dst[(d - 1) * tw + q] = q == at ? (w & ~(3ull << sh)) | x << sh : w;
        }
    }
}

// decide: rows = the 3 * K answers of the trial planned at s; rd = the read's own words of the output.  kcor_sweep's acceptance and
// what follows it, then the moves that need no answer.  False: the read is done, its report in kcor_rows_report(s)
PG_HD bool kcor_rows_decide(KcorRowsRead& s, const uint64_t* rows, uint64_t* rd, int nk, int K, const KcorParams& pr, const uint64_t* bits) {
    const bool up = s.phase == KCOR_ROWS_RIGHT;
    const int full = kcor_rows_full(s, nk, K), p = kcor_rows_base(s, K), now = read_base(rd, p);
    int best = -1, second = -1, best_x = 0;
    for (int d = 1; d < 4; d++) {
        const uint64_t* row = rows + (d - 1) * K;
        int ext = 0;
        bool run = true;
        for (int i = 0; i < full; i++) {           // (every row is loaded: a select a k-mer, no early way out)
            run = run && kcor_solid_word(row[up ? i : K - 1 - i], pr.min_cov);
            ext += run ? 1 : 0;
        }
        const bool first = ext > best, next = !first && ext > second;
        second = first ? best : next ? ext : second;
        best_x = first ? (now + d) & 3 : best_x;
        best = first ? ext : best;
    }
    const int need = (int)pr.min_run < full ? (int)pr.min_run : full;
    if (best < need || best == second) {
        s.flags |= up ? KCOR_STOP_RIGHT : KCOR_STOP_LEFT;
        s.j = up ? nk : -1;                        // the sweep ends; settle starts the left one behind the right one
    } else {
        kcor_write_base(rd, p, best_x);
        s.fixes++;
        // k-mers j .. j + dir (best - 1) are solid now; the next one is weak where kcor_sweep says it is
        s.j += up ? best : -best;
        s.weak = best < full || !up;
    }
    return kcor_rows_settle(s, nk, pr.max_fixes, bits);
}

// the device engine (kindex_kernels.hip): an index cut over ranks; d_packed_out may be b.packed.  stats = KCOR_ROWS_STATS words
int kcor_device_correct_rows(::pg_kindex* ix, const KidxBatch& b, const KcorParams& pr, uint64_t* d_packed_out, uint64_t* d_report, void* stream,
                             uint64_t* stats);

}  // namespace pg
