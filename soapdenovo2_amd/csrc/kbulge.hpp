// kbulge.hpp -- bubbles popped on their strongest paths (pg_kindex_pop_bulges, include/soapdenovo2_amd.h section 3).  The
// simple rule (kbubble.hpp) pops a branch only beside a SIBLING, a second simple linear unitig between the same two junctions.  Two
// errors less than K apart on different reads, a bubble on an arm, a tip on an arm: the alternative is then no simple unitig, and the
// weak arm waits for ever.  This operator asks less of the alternative: that the strongest arcs lead from the fork to the join.
//
// Solid, min_cov (1..255), min_arc (1..63), the side test and the end reasons are kunitig.hpp's.  The ARM P = x0 -> ... -> x(n-1), its
// fork u, its join v, L, max_len and max_diff are exactly kbubble.hpp's branch: kbubble_arm, steps 1 and 2 of kbubble_decide.
//
// A STRONG STEP x -> y:
//     b is the one base whose out-counter in x's word is at least min_arc and STRICTLY greater than the other three (one arc qualifies)
//     y = next(x, b) is solid, and canon(y) != canon(x)
//     in y's word the in-counter for x's first base is at least min_arc and strictly greater than y's other three in-counters
// Raw counters are read, and ties end the path.  The test reads the same two counter sets whichever way it is read, so x -> y is strong
// exactly when rc(y) -> rc(x) is; every oriented k-mer has at most one strong successor and at most one strong predecessor; and an open
// step (kunitig.hpp) is a strong step.
// The STRONGEST PATH S: from u by strong steps.  It succeeds when the node reached is v, in v's slot and v's orientation, with m k-mers
// strictly between u and v; it fails when there is no strong step, when the walk reaches u's slot or v's slot in the other orientation,
// or when m would exceed n_P + max_diff.
// P is MINOR, and popped, iff S succeeds, m >= 1, S's first k-mer is not x0, |n_P - m| <= max_diff, and cov_P * m < cov_S * n_P in 64-bit
// integers, the sums over the k-mers strictly between u and v (at most 255 * 2^17 times 2^17: no overflow).  The arm is decided once,
// from its emitting start, as in kbubble.hpp; the mirrored view walks the same path.  The deciding lane makes at most
// n + 1 + (n + max_diff + 1) dependent slot reads, fewer than the simple rule's three siblings.  The decide pass only reads.
// The round's totals (kedit.hpp): arms popped, k-mers removed, solid k-mers before the round, arms kept.
//
// A ROUND decides over the index as it stood when the round began, then applies exactly as the bubbles do (kbubble_apply): the arm's
// words become 0 and its two counters leave the junctions' words.  The locks argument is kbubble.hpp's: an arm's k-mers lie in that
// unitig alone, and a junction's counters leave by the vector atomicAnd.
//
// SURVIVAL: no k-mer of any S is removed in the round that uses it.  A removed k-mer lies in a minor arm B.  B's members have one arc
// in and one arc out, so S can only run through B from u_B to v_B, through all of it.  Then the arc u_B -> B is the strong step out of
// u_B and B -> v_B the strong step into v_B, so B's own strongest path, from either end, is B itself: its first k-mer is B's x0, B is
// not minor, and it stays.  A junction on S only loses counters that were weaker than its strong one -- a popped arm's counter at u_B
// is not the strict maximum there, or S_B would start with B's x0 --, so S stays strong and u stays connected to v.  S cannot enter P
// either: the only arc into x0 comes from u, and S never returns to u.
//
// One piece of PG_HD code for the round's kernels (kindex_kernels.hip) and its host twin (kedit_host.hpp), which see it as KbulgeOp
// (kedit.hpp).  Loop state is kept with selects.
#pragma once
#include "kbubble.hpp"

namespace pg {

// Of the four 6-bit counters of `half`: the index of the one that is at least min_arc and strictly greater than the other three; 4
// when there is none
PG_HD int kbulge_top(uint32_t half, uint32_t min_arc) {
    uint32_t best = 0;
    int at = 4;
    bool tie = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t c = (half >> (6 * i)) & 63u;
        tie = c == best ? true : c > best ? false : tie;
        at = c > best ? i : at;
        best = c > best ? c : best;
    }
    return best >= min_arc && !tie ? at : 4;
}

// The strong step out of the solid node x, in place: true, and x is y; false: no strong step (x is then whatever the lookup left)
template <int NW, typename Find>
PG_HD bool kbulge_step(KwalkNode<NW>& x, int K, const Kmer<NW>& filter, uint32_t min_cov, uint32_t min_arc, Find find) {
    const int t = kbulge_top(x.fwd ? (uint32_t)(x.w >> 32) : (uint32_t)x.w, min_arc);
    if (t == 4) return false;
    const int base = x.fwd ? t : t ^ 2, first = (int)(x.b.w[NW - 1] & 3) ^ 2;
    const Kmer<NW> from = kwalk_canon<NW>(x);
    kmer_roll<NW>(x.a, x.b, base, K, filter);
    x.fwd = !kmer_less<NW>(x.b, x.a);
    x.slot = 0;
    x.w = find(kwalk_canon<NW>(x), x.slot);
    const int in = kbulge_top(kedit_in_half(x.fwd) ? (uint32_t)(x.w >> 32) : (uint32_t)x.w, min_arc);
    return kcor_solid_word(x.w, min_cov) && !kmer_eq<NW>(kwalk_canon<NW>(x), from) && in == kedit_in_index(x.fwd, first);
}

// The decision for the start x0 whose left side has reason `left`; candidate: an arm in its deciding orientation.  Only reads
template <int NW, typename Find>
PG_HD KeditDecision kbulge_decide(const KwalkNode<NW>& x0, uint32_t left, int K, const KbubbleParams& pr, Find find) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const KbubbleArm<NW> arm = kbubble_arm<NW>(x0, left, K, filter, KunitigParams{pr.min_cov, pr.min_arc, pr.max_len}, find);
    if (!arm.branch) return KeditDecision{arm.P.n, false, false};
    const KeditPath& P = arm.P;
    const KwalkNode<NW>&v = arm.v, &L = arm.L;
    const KwalkNode<NW> u = kbubble_flip<NW>(L);
    // S, from u by strong steps to v; m k-mers between, their coverage summed
    KwalkNode<NW> y = u;
    const uint64_t most = (uint64_t)P.n + pr.max_diff;
    uint64_t m = 0, cov = 0;
    bool reached = false;
    for (;;) {
        if (!kbulge_step<NW>(y, K, filter, pr.min_cov, pr.min_arc, find)) break;
        reached = y.slot == v.slot && y.fwd == v.fwd;
        // v either way, back at u, S's first k-mer is x0 (S is then P itself), or too long
        if (y.slot == v.slot || y.slot == u.slot || (m == 0 && y.slot == x0.slot && y.fwd == x0.fwd) || m == most) break;
        m++;
        cov += kidx_coverage(y.w);
    }
    const uint64_t diff = P.n > m ? P.n - m : m - P.n;
    const bool minor = reached && m >= 1 && diff <= pr.max_diff && P.cov * m < cov * (uint64_t)P.n;
    return KeditDecision{P.n, true, minor};
}

// The bulges as the round sees them (kedit.hpp): the bubbles' thresholds and the bubbles' apply
struct KbulgeOp {
    using Params = KbubbleParams;
    static PG_HD KunitigParams ends(const Params& pr) { return KunitigParams{pr.min_cov, pr.min_arc, pr.max_len}; }
    static PG_HD bool starts(uint32_t left) { return left == KWALK_BRANCH_IN; }
    template <int NW, typename Find>
    static PG_HD KeditDecision decide(const KwalkNode<NW>& x0, uint32_t left, int K, const Params& pr, Find find) {
        return kbulge_decide<NW>(x0, left, K, pr, find);
    }
    template <int NW, typename Find, typename Zero, typename Clear>
    static PG_HD void apply(const KwalkNode<NW>& x0, uint32_t n, int K, const Params& pr, Find find, Zero zero, Clear clear) {
        kbubble_apply<NW>(x0, n, K, pr, find, zero, clear);
    }
};

}  // namespace pg
