// ktip.hpp -- minor tips clipped from the graph of the k-mer index (pg_kindex_clip_tips, include/soapdenovo2_amd.h section 3; DESIGN.md
// §15).  The unitigs of kunitig.hpp are those of the graph as counted and thresholded, and on real reads nearly all of their ends are
// error tips: a short dead-ending chain that hangs off the real path by one arc weaker than the real one.  The reference clips them
// before it builds its edges (removeSingleTips, removeMinorTips); this is that step for the index, and the first operator that writes
// to the table after it was built.
//
// Solid, out_x, in_x, min_cov (1..255), min_arc (1..63), the side test and the end reasons are kunitig.hpp's (kunitig_side).
//
// A TIP CANDIDATE is a linear unitig x0 -> ... -> x(n-1) of that rule, oriented so that
//     the left side of x0 is FREE: its reason is KWALK_DEAD_END or KWALK_WEAK_NEXT
//     the right side of x(n-1) has reason KWALK_BRANCH_IN
//     n <= max_tip (1 .. 2^16 k-mers)
// and every other pair of reasons is none: both sides free (an island), BRANCH_OUT (the path before a fork), HAIRPIN, CYCLE, a chain
// longer than max_tip.  A candidate has exactly one such orientation -- a side is free or BRANCH_IN, not both --, so it is found once,
// from the start (kunitig.hpp: kunitig_start) whose left reason is free, and no duplicate rule is needed.
// y, the JUNCTION, is the solid node behind the attached side, in the orientation the step reaches it; a = the first base of x(n-1);
// c_t = the 6-bit in-counter of y for a: the left counter a when y is its canonical form, the right counter a ^ 2 otherwise
// (kwalk_in_set reads the same).  The candidate is MINOR, and clipped, iff c_t is strictly smaller than the largest of y's other three
// in-counters: raw counters, not thresholded ones, and ties are kept, 63 against 63 included.  So the strongest arc into a junction
// side always survives, and two short dead ends that fork from one k-mer never both vanish.
//
// A ROUND decides over the index as it stood when the round began, then applies:
//     the value word of every k-mer of every minor tip becomes 0.  The slot's state stays published: a tombstone -- map_probe stops at
//     an empty state only, so probes for other keys pass over it, and kidx_find answers 0, "not in the set", for the key itself
//     in y's word the one counter c_t becomes 0
// and nothing else is written.  Arcs below min_arc that point at a clipped k-mer from elsewhere stay: a clipped index is meant to be
// used at the same or higher thresholds.  Clipping a tip can make the path it hung on a tip in turn, so a caller runs rounds until one
// clips nothing (KmerIndex.clip_tips).
//
// Why the apply pass needs no locks.  A tip's k-mers belong to no other tip: a linear unitig's k-mers lie in that unitig alone
// (kunitig.hpp).  A junction is never a tip member: pass 1 counts an arc at both of its ends, so a is in in_y, BRANCH_IN says in_y holds
// another base too, and y's side towards the tip -- the right side of rc(y), whose out set is the complement of in_y -- is BRANCH_OUT,
// neither free nor BRANCH_IN, while an interior side is open.  So the only word two lanes may write together is a junction's, each
// clearing a different counter of its in-half: a vector atomicAnd on that 32-bit half, in plain C++.  Every other write is a lane's own
// plain store.  The apply walk follows each k-mer's single out arc as read from the k-mer's OWN word, which no other lane writes, and
// does not test the successor again: another lane may be changing the junction just then.  (Hand-made records whose arcs disagree at
// their two ends can make y a member of another tip.  The result is still one: that tip's walk reads y's out-half, the atomicAnd clears
// a counter of its in-half that was below min_arc already, and a zeroed word stays zero under the AND in either order.)
//
// One piece of PG_HD code for the round's kernels (kindex_kernels.hip: kedit_decide_kernel, kedit_apply_kernel) and its host twin
// (kedit_host.cpp), which see it as KtipOp (kedit.hpp): ktip_decide reads, ktip_apply writes through two functions of the caller.  Loop
// state is kept with selects (DESIGN.md §11 on what stores under branches inside such a loop became).
#pragma once
#include "kedit.hpp"

namespace pg {

constexpr uint32_t KTIP_MAX_TIP = 1u << 16;

struct KtipParams {
    uint32_t min_cov, min_arc, max_tip;
};

PG_HD bool ktip_free(uint32_t reason) { return reason == KWALK_DEAD_END || reason == KWALK_WEAK_NEXT; }

// the minor test on the junction's word: c_t strictly below the largest of the other three in-counters
PG_HD bool ktip_minor(uint64_t w, bool fwd, int a) {
    const uint32_t half = kedit_in_half(fwd) ? (uint32_t)(w >> 32) : (uint32_t)w;
    const int t = kedit_in_index(fwd, a);
    uint32_t c_t = 0, other = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t c = (half >> (6 * b)) & 63u;
        c_t = b == t ? c : c_t;
        other = b != t && c > other ? c : other;
    }
    return c_t < other;
}

// The decision for the start x0 whose left side has reason `left`: at most max_tip k-mers to the right through open sides; candidate:
// free on the left, BRANCH_IN on the right, n <= max_tip.  Only reads
template <int NW, typename Find>
PG_HD KeditDecision ktip_decide(const KwalkNode<NW>& x0, uint32_t left, int K, const KtipParams& pr, Find find) {
    if (!ktip_free(left)) return KeditDecision{1, false, false};
    KwalkNode<NW> x = x0, y;
    const KeditPath P = kedit_path<NW>(x, y, K, kmer_filter<NW>(K), KunitigParams{pr.min_cov, pr.min_arc, pr.max_tip}, find);
    const bool candidate = P.reason == KWALK_BRANCH_IN;                          // (y is the junction, its word in hand)
    const int a = (int)(x.b.w[NW - 1] & 3) ^ 2;                                  // (x's first base: the complement of its reverse complement's last)
    return KeditDecision{P.n, candidate, candidate && ktip_minor(y.w, y.fwd, a)};
}

// The minor tip of n k-mers from x0 applied: every k-mer's successor is named by the single out arc of the k-mer's own word and looked
// up -- find(ck, slot) = kunitig_probe --, then zero(slot) is called for the k-mer just left; behind the n-th, clear(slot, fwd, a)
// for the junction, which takes the counter kedit_keep_mask(fwd, a) leaves out from half kedit_in_half(fwd) of its word
template <int NW, typename Find, typename Zero, typename Clear>
PG_HD void ktip_apply(const KwalkNode<NW>& x0, uint32_t n, int K, const KtipParams& pr, Find find, Zero zero, Clear clear) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    KwalkNode<NW> x = x0;
    int a = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t left = x.slot;
        const int base = kwalk_lowest(kwalk_out_set(x.w, x.fwd, pr.min_arc));
        a = (int)(x.b.w[NW - 1] & 3) ^ 2;
        kmer_roll<NW>(x.a, x.b, base, K, filter);
        x.fwd = !kmer_less<NW>(x.b, x.a);
        x.slot = 0;
        x.w = find(kwalk_canon<NW>(x), x.slot);
        zero(left);
    }
    clear(x.slot, x.fwd, a);
}

// The tips as the round sees them (kedit.hpp)
struct KtipOp {
    using Params = KtipParams;
    static PG_HD KunitigParams ends(const Params& pr) { return KunitigParams{pr.min_cov, pr.min_arc, pr.max_tip}; }
    static PG_HD bool starts(uint32_t left) { return ktip_free(left); }
    template <int NW, typename Find>
    static PG_HD KeditDecision decide(const KwalkNode<NW>& x0, uint32_t left, int K, const Params& pr, Find find) {
        return ktip_decide<NW>(x0, left, K, pr, find);
    }
    template <int NW, typename Find, typename Zero, typename Clear>
    static PG_HD void apply(const KwalkNode<NW>& x0, uint32_t n, int K, const Params& pr, Find find, Zero zero, Clear clear) {
        ktip_apply<NW>(x0, n, K, pr, find, zero, clear);
    }
};

}  // namespace pg
