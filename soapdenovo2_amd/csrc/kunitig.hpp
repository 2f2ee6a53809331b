// kunitig.hpp -- the whole graph of the k-mer index compacted into unitigs (pg_kindex_unitigs, include/soapdenovo2_amd.h section 3; DESIGN.md
// §14).  kwalk.hpp extends sequences the caller already has; this is the operator that asks nothing of the caller but two thresholds and
// returns every maximal unambiguous path of the graph exactly once, as a ragged batch the other operators take where it lies.  The
// reference does the same once for the whole graph, from the same counters (node2edge.c).
//
// Solid, the arc sets out_x and in_x of an oriented k-mer x, min_cov (1..255) and min_arc (1..63) are kwalk.hpp's: kcor_solid_word,
// kwalk_out_set, kwalk_in_set.
//
// The right side of a solid oriented k-mer x is OPEN when all of
//     out_x holds exactly one base b                      else KWALK_DEAD_END (none) or KWALK_BRANCH_OUT (several)
//     y = next(x, b) is solid                             else KWALK_WEAK_NEXT
//     in_y is exactly { first base of x }                 else KWALK_BRANCH_IN
//     canon(y) != canon(x)                                else KUNITIG_HAIRPIN
// hold, and otherwise it is an END with the first reason of that list that applies.  HAIRPIN covers x -> rc(x) (K odd: K - 1 is even,
// so the (K-1)-mer the two share can be its own reverse complement) and the self-loop x -> x; without it a path could run back over its
// own reverse complement and every node would come out twice.  The left side of x is the right side of rc(x).
// Open is symmetric: the right side of x is open towards y exactly when the left side of y is open towards x.  The test reads x's record
// for out_x and y's for in_y, and the left side of y -- the right side of rc(y) -- reads y's record for out_rc(y) = the complement of in_y and
// x's for in_rc(x) = the complement of out_x: the same two sets, whatever the counters hold.
//
// A LINEAR unitig is a maximal chain x0 -> x1 -> ... -> x(n-1), n >= 1, every step through an open right side, the left side of x0 and
// the right side of x(n-1) ends.  Its text is x0 followed by the appended bases, n + K - 1 of them.  It is found from both ends, from
// s = x0 and from e = rc(x(n-1)) as its reverse complement, and emitted once: from s iff !kmer_less(e, s).
// With K odd a chain from an end never meets a canonical k-mer twice (DESIGN.md §14 has the argument), so s != e and n is at most the
// number of solid k-mers.
// A CYCLIC unitig is a set of solid k-mers none of which has an end side: a ring.  It is emitted once, from the member with the least
// canonical key in that key's canonical orientation, walking right; n + K - 1 bases, both reasons KUNITIG_CYCLE.  A member that meets a
// smaller canonical key, a covered k-mer or an end knows that it is not that member and stops there.
// The guard: a walk stops after max_kmers (1 .. 2^26) k-mers.  A linear chain that is longer comes out from both of its ends, each with
// KUNITIG_CUT on the cut side, and the k-mers between the two cuts (or, where the two overlap, under both) are not in exactly one
// unitig; a ring that is longer is not emitted at all -- its least member cannot tell it from the inside of a cut chain.  The totals
// count the cut unitigs.  When nothing was cut, every solid k-mer lies in exactly one emitted unitig in exactly one orientation.
//
// One piece of PG_HD code for the kernels (kindex_kernels.hip: kunitig_*_kernel) and the host twin (kunitig_host.cpp): kunitig_side is
// the side test -- the walk's step (kwalk.hpp: kwalk_step over a KwalkNode) and the HAIRPIN comparison --, kunitig_chain the one walk
// that measures (row == null) or writes through the walk's base writer (KwalkText); both take the lookup as a function of the canonical
// k-mer that also returns the slot, for the covered bit a slot.  Reason and length are kept with selects (DESIGN.md §11 on what stores
// under branches inside such a loop became).
// Behind the rule, what the two unitig engines and the edit rounds state once: the finish of a compaction (kunitig_finish,
// kunitig_finish_tail) and the scratch of ix->uni (KunitigScratch, kunitig_plan, kunitig_bind) -- plain host code a program built
// without the device engine can call.
#pragma once
#include "kwalk.hpp"

namespace pg {

constexpr uint32_t KUNITIG_MAX_KMERS = 1u << 26;
constexpr int KUNITIG_TOTALS = 8;
// end reasons: KWALK_DEAD_END (3), KWALK_BRANCH_OUT (4), KWALK_WEAK_NEXT (5), KWALK_BRANCH_IN (6) and
enum : uint32_t { KUNITIG_HAIRPIN = 9, KUNITIG_CYCLE = 10, KUNITIG_CUT = 11 };
// out_totals
enum : int {
    KUNITIG_T_UNITIGS = 0, KUNITIG_T_WORDS = 1, KUNITIG_T_BASES = 2, KUNITIG_T_COVERED = 3, KUNITIG_T_SOLID = 4, KUNITIG_T_CYCLIC = 5,
    KUNITIG_T_CUT = 6, KUNITIG_T_OVERFLOW = 7,
};

struct KunitigParams {
    uint32_t min_cov, min_arc, max_kmers;
};

// A start: the slot of x0's canonical key, whether x0 is that key (else its reverse complement), and the reason of x0's left side (an
// end reason, or KUNITIG_CYCLE for the least member of a ring)
constexpr int KUNITIG_START_FWD = 62, KUNITIG_START_REASON = 56;
PG_HD uint64_t kunitig_start(uint64_t slot, bool fwd, uint32_t reason) {
    return slot | (uint64_t)(fwd ? 1 : 0) << KUNITIG_START_FWD | (uint64_t)reason << KUNITIG_START_REASON;
}
PG_HD uint64_t kunitig_start_slot(uint64_t s) { return s & ((1ull << KUNITIG_START_REASON) - 1); }
PG_HD bool kunitig_start_fwd(uint64_t s) { return (s >> KUNITIG_START_FWD & 1) != 0; }
PG_HD uint32_t kunitig_start_reason(uint64_t s) { return (uint32_t)(s >> KUNITIG_START_REASON) & 15u; }

// words of a unitig of n k-mers, and its first report word
PG_HD uint64_t kunitig_row_words(uint32_t n, int K) { return ((uint64_t)n + (uint64_t)K - 1 + 31) / 32; }
PG_HD uint64_t kunitig_report_word(uint64_t bases, uint32_t left, uint32_t right) { return bases | (uint64_t)left << 32 | (uint64_t)right << 40; }

// kidx_find that also says where: the word of canonical key ck and its slot; 0 (and the slot untouched) when the table has no such key
template <int NW>
PG_HD uint64_t kunitig_probe(const uint64_t* tab, uint64_t mask, const Kmer<NW>& ck, uint64_t& slot) {
    const uint64_t* sl = map_probe<NW>(tab, mask, ck);
    if (!sl) return 0;
    slot = (uint64_t)(sl - tab) / map_slot_words<NW>();
    return sl[NW];
}

// the k-mer's first base in the top bits of word 0: the first words of its packed text
template <int NW>
PG_HD Kmer<NW> kunitig_left_aligned(Kmer<NW> a, int K) {
    int d = 64 * NW - 2 * K;
#pragma unroll
    for (int step = 0; step < NW - 1; step++) {
        if (d >= 64) {
#pragma unroll
            for (int i = 0; i < NW - 1; i++) a.w[i] = a.w[i + 1];
            a.w[NW - 1] = 0;
            d -= 64;
        }
    }
    if (d > 0) {
#pragma unroll
        for (int i = 0; i < NW - 1; i++) a.w[i] = (a.w[i] << d) | (a.w[i + 1] >> (64 - d));
        a.w[NW - 1] <<= d;
    }
    return a;
}

// the node (kwalk.hpp) of the canonical key c stored at `slot` with word w, as itself (fwd) or as its reverse complement
template <int NW>
PG_HD KwalkNode<NW> kunitig_node(const Kmer<NW>& c, uint64_t w, uint64_t slot, bool fwd, int K) {
    const Kmer<NW> r = kmer_rc<NW>(c, K);
    return KwalkNode<NW>{fwd ? c : r, fwd ? r : c, w, slot, fwd};
}

// The side test: 0 when the right side of the solid node x is open, and then y is the node behind it and base the base that leads
// there; else the end's reason: the step's, or HAIRPIN behind a good step.  find(ck, slot) = kunitig_probe
template <int NW, typename Find>
PG_HD uint32_t kunitig_side(const KwalkNode<NW>& x, int K, const Kmer<NW>& filter, const KunitigParams& pr, Find find, KwalkNode<NW>& y, int& base) {
    y = x;
    const uint32_t reason = kwalk_step<NW>(y, K, filter, pr.min_cov, pr.min_arc, find, base);
    const bool same = kmer_eq<NW>(kwalk_canon<NW>(y), kwalk_canon<NW>(x));      // (an end before the lookup: y is x, and the reason stands)
    return reason ? reason : same ? KUNITIG_HAIRPIN : 0;
}

// What a walk found.  n == 0: the start is not the one its unitig is emitted from (the losing end of a chain; not the least member of a
// ring, or no ring at all) and nothing of the rest counts
struct KunitigWalk {
    uint32_t n, reason;            // k-mers, and the reason on the right
    uint64_t cov;                  // the sum of their coverage
};

// One walk to the right of the solid node x0.  cyclic: x0 is a canonical k-mer that asks whether it is the least member of a ring.
// mark(slot) is called for every k-mer of a chain (not of a ring), covered(slot) asked of every k-mer a ring's walk meets.
// row (may be null): the unitig's kunitig_row_words(n, K) words
template <int NW, typename Find, typename Mark, typename Covered>
PG_HD KunitigWalk kunitig_chain(const KwalkNode<NW>& x0, bool cyclic, int K, const KunitigParams& pr, Find find, Mark mark, Covered covered,
                                uint64_t* row) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const Kmer<NW> first = kunitig_left_aligned<NW>(x0.a, K), c0 = kwalk_canon<NW>(x0);
    KwalkNode<NW> x = x0;
    uint32_t n = 1, reason = 0;
    uint64_t cov = kidx_coverage(x0.w);
    bool lost = false;
    KwalkText text{row, 0, (uint32_t)K};          // x0's bases: its full words stored, the partial one in hand
#pragma unroll
    for (int q = 0; q < NW; q++) {
        if (row && q < K / 32) row[q] = first.w[q];
        text.acc = q == K / 32 ? first.w[q] : text.acc;
    }
    if (!cyclic) mark(x0.slot);
    for (;;) {
        KwalkNode<NW> y;                           // (an end before the lookup leaves it x)
        int base = 0;
        reason = kunitig_side<NW>(x, K, filter, pr, find, y, base);
        if (cyclic) {
            const Kmer<NW> cy = kwalk_canon<NW>(y);
            const bool closes = !reason && kmer_eq<NW>(cy, c0);
            // an end: a chain, not a ring; a smaller key: not the least member; a covered k-mer: a chain that was cut; the guard: too long to tell
            lost = !closes && (reason || kmer_less<NW>(cy, c0) || covered(y.slot) || n == pr.max_kmers);
            reason = closes ? KUNITIG_CYCLE : reason;
            if (lost) break;
        }
        reason = !reason && n == pr.max_kmers ? KUNITIG_CUT : reason;
        if (reason) break;
        text.append(base);
        cov += kidx_coverage(y.w);
        n++;
        x = y;
        if (!cyclic) mark(x.slot);
    }
    (void)text.finish();
    // a chain is emitted from the end that is not greater; a cut one from both
    lost = lost || (!cyclic && reason != KUNITIG_CUT && kmer_less<NW>(x.b, x0.a));
    return KunitigWalk{lost ? 0u : n, reason, cov};
}

// The ends of the solid canonical k-mer c at `slot`: bit 0 of the result says its left side is an end (c starts a walk), bit 1 that
// its right side is (rc(c) starts one); reasons[0], reasons[1] are the two sides' reasons, left first.  At most two lookups
template <int NW, typename Find>
PG_HD uint32_t kunitig_ends(const Kmer<NW>& c, uint64_t w, uint64_t slot, int K, const KunitigParams& pr, Find find, uint32_t reasons[2]) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const KwalkNode<NW> f = kunitig_node<NW>(c, w, slot, true, K), r = kunitig_node<NW>(c, w, slot, false, K);
    KwalkNode<NW> y;
    int base = 0;
    reasons[1] = kunitig_side<NW>(f, K, filter, pr, find, y, base);
    reasons[0] = kunitig_side<NW>(r, K, filter, pr, find, y, base);
    return (reasons[0] ? 1u : 0u) | (reasons[1] ? 2u : 0u);
}

// what a start of n k-mers (0: the copy that is not emitted) adds to the scan: kept, words, k-mers
PG_HD KidxCounts kunitig_counts(uint32_t n, int K) { return KidxCounts{{n ? 1ull : 0ull, n ? kunitig_row_words(n, K) : 0ull, n, 0}}; }

// The finish of a compaction, for both engines, their kernels and their host twins.  kunitig_finish: the eight totals from the scan's
// sums (kept, words, k-mers) and the counts, and the go decision: full mode, and the unitigs and their words with the tail fit the
// capacities.  kunitig_finish_tail, where the decision was go: the batch's last offsets and the tail's zero words
PG_HD bool kunitig_finish(const KidxCounts& all, int K, int tail, uint64_t solid, uint64_t cyclic, uint64_t cut, uint64_t cap_unitigs,
                          uint64_t cap_words, bool full, uint64_t* totals) {
    const uint64_t unitigs = all.c[0], words = all.c[1], kmers = all.c[2];
    const bool overflow = full && (unitigs > cap_unitigs || words + (uint64_t)tail > cap_words);
    totals[KUNITIG_T_UNITIGS] = unitigs;
    totals[KUNITIG_T_WORDS] = words + (uint64_t)tail;
    totals[KUNITIG_T_BASES] = kmers + unitigs * (uint64_t)(K - 1);
    totals[KUNITIG_T_COVERED] = kmers;
    totals[KUNITIG_T_SOLID] = solid;
    totals[KUNITIG_T_CYCLIC] = cyclic;
    totals[KUNITIG_T_CUT] = cut;
    totals[KUNITIG_T_OVERFLOW] = overflow ? 1 : 0;
    return full && !overflow;
}
PG_HD void kunitig_finish_tail(const KidxCounts& all, int tail, uint64_t* packed_out, uint64_t* word_off_out, uint64_t* kmer_base_out) {
    if (word_off_out) word_off_out[all.c[0]] = all.c[1];
    if (kmer_base_out) kmer_base_out[all.c[0]] = all.c[2];
    for (int q = 0; q < tail; q++) packed_out[all.c[1] + q] = 0;
}

// ---- the scratch of ix->uni, for the three operators that use it: the unitigs by walking, by list ranking, and an edit round ----
// The counters at its head: the unitigs' and, behind them, an edit round's (unitigs removed, k-mers removed, candidates kept)
enum : int {
    KUNITIG_C_STARTS = 0, KUNITIG_C_CYCLIC = 1, KUNITIG_C_SOLID = 2, KUNITIG_C_CUT = 3, KUNITIG_C_GO = 4,
    KEDIT_C_REMOVED = 5, KEDIT_C_KMERS = 6, KEDIT_C_KEPT = 7, KUNITIG_CTRS = 8
};
// ctr: KUNITIG_C_*; starts / lens: `cap` entries, the chains' starts first and the rings' behind them; sums: the scan's, KIDX_COUNTS a
// block of 256 starts; bits: a covered bit a slot.  An array the operator does not have is null
struct KunitigScratch {
    unsigned long long* ctr;
    uint64_t* starts;
    uint32_t* lens;
    uint64_t* sums;
    uint32_t* bits;
    uint64_t cap;
};

// The plan: where every array lies, in 64-bit words from the scratch's base, decided on the host from keys and slots before anything is
// counted.  cap = the start list's entries: 2 * keys hold every start -- a stored k-mer has two sides, a chain's start is an end side,
// and a ring's least member has none --, and the ranked engine's two oriented nodes a key, of which it wants two at least.  The first
// `zero` words (the counters, the ranked engine's control words) are zeroed before a call, and the walk's covered bits.  The ranked
// engine's arrays are krank.hpp's: the control words (KUNITIG_PLAN_CTL words of two), the records (two generations of cap, two words
// each), succ0, slot_of and node_of (32-bit, two a word).  An array a kind does not have: KUNITIG_ABSENT
enum KunitigKind : int { KUNITIG_KIND_WALK = 0, KUNITIG_KIND_RANK = 1, KUNITIG_KIND_EDIT = 2 };
constexpr uint64_t KUNITIG_ABSENT = ~0ull, KUNITIG_PLAN_CTL = 96;
static_assert(KUNITIG_CTRS % 2 == 0 && (KUNITIG_CTRS + KUNITIG_PLAN_CTL) % 2 == 0, "the records are 16-byte aligned, whatever the kind");
struct KunitigPlan {
    uint64_t cap, start_blocks, zero, total;
    uint64_t ctr, ctl, rec, starts, lens, sums, bits, succ0, slot_of, node_of;
};
inline KunitigPlan kunitig_plan(uint64_t keys, uint64_t slots, KunitigKind kind) {
    const bool rank = kind == KUNITIG_KIND_RANK;
    const uint64_t least = rank ? 2 : 1;
    KunitigPlan p;
    p.cap = 2 * keys > least ? 2 * keys : least;
    p.start_blocks = (p.cap + 255) / 256;
    uint64_t at = 0;
    auto take = [&at](bool has, uint64_t words) {
        const uint64_t off = has ? at : KUNITIG_ABSENT;
        at += has ? words : 0;
        return off;
    };
    p.ctr = take(true, KUNITIG_CTRS);
    p.ctl = take(rank, KUNITIG_PLAN_CTL);
    p.zero = at;
    p.rec = take(rank, 4 * p.cap);
    p.starts = take(true, p.cap);
    p.lens = take(true, (p.cap + 1) / 2);
    p.sums = take(kind != KUNITIG_KIND_EDIT, p.start_blocks * KIDX_COUNTS);
    p.bits = take(kind == KUNITIG_KIND_WALK, (slots + 63) / 64);
    p.succ0 = take(rank, p.cap / 2);
    p.slot_of = take(rank, (keys + 2) / 2);
    p.node_of = take(rank, (slots + 1) / 2);
    p.total = at;
    return p;
}
// the array at word `off` of the scratch at `base`, null when the plan has none
template <typename T>
inline T* kunitig_at(uint64_t* base, uint64_t off) { return off == KUNITIG_ABSENT ? nullptr : (T*)(base + off); }
inline KunitigScratch kunitig_bind(uint64_t* base, const KunitigPlan& p) {
    return KunitigScratch{kunitig_at<unsigned long long>(base, p.ctr), kunitig_at<uint64_t>(base, p.starts), kunitig_at<uint32_t>(base, p.lens),
                          kunitig_at<uint64_t>(base, p.sums), kunitig_at<uint32_t>(base, p.bits), p.cap};
}

// The caller's side of the device engine (kindex_kernels.hip), asynchronous on `stream`: count mode when d_packed_out is null
int kunitig_device_unitigs(::pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* d_packed_out,
                           uint64_t* d_word_off_out, uint64_t* d_kmer_base_out, uint64_t* d_report, uint64_t* d_totals, void* stream);

}  // namespace pg
