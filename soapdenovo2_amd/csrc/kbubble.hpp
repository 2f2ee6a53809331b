// kbubble.hpp -- simple bubbles popped from the graph of the k-mer index (pg_kindex_pop_bubbles, include/soapdenovo2_amd.h section 3;
// DESIGN.md §16).  A substitution in the middle of a read is no tip (ktip.hpp): its K k-mers leave the real path at one k-mer and rejoin
// it at another, a BUBBLE, and until the weaker side of it is gone the unitigs of kunitig.hpp end at both of its junctions.  The
// reference pops them on its edges (bubblePinch); this is that step for the index, and the second operator that writes to the table.
//
// Solid, out_x, in_x, min_cov (1..255), min_arc (1..63), the side test, the end reasons and a linear unitig are kunitig.hpp's
// (kunitig_side).
//
// A BRANCH is a linear unitig P = x0 -> ... -> x(n-1) of that rule with
//     both of its sides of reason KWALK_BRANCH_IN
//     n <= max_len (1 .. 2^16 k-mers)
//     two junctions that are different canonical k-mers
// The junctions: v is the solid node behind the right side, as the step from x(n-1) reaches it, and L the node behind the left side, as
// the step from rc(x0) reaches it.  u = rc(L) is the FORK: with arcs counted at both of their ends out_u holds the last base of x0 and
// at least one other base.  A unitig whose two junctions are one canonical k-mer -- a loop u -> P -> u, or u -> P -> rc(u) -- is no
// branch and is never touched.
// Two branches P and Q are SIBLINGS when they have the same u and the same v, each the same slot in the same orientation, and
// |n_P - n_Q| <= max_diff (0 .. 2^16).  Both are branches in the sense above: a weak path beside an alternative that is no simple linear
// unitig of at most max_len k-mers is kept.
// P is MINOR, and popped, iff some sibling Q has a strictly greater mean coverage: cov_P * n_Q < cov_Q * n_P in 64-bit integers, cov
// the sum of kidx_coverage over the branch (at most 255 * 2^16 times 2^16: no overflow), no division, no floating point.  Ties are kept,
// 255 against 255 included, so the strongest branch of every bubble survives and u stays connected to v; of three siblings A < B < C,
// A and B go in one round.
//
// DECIDED ONCE.  A branch has two starts in the unitigs' start list (kunitig.hpp: kunitig_start), one from each end, both with left
// reason BRANCH_IN.  It is decided from the start s from which kunitig_chain would emit it -- !kmer_less(e, s), e = rc(x(n-1)) --; the
// other start ends after its walk.  Seen from there the mirrored bubble gives the same answer: open is symmetric, and so are the two
// BRANCH_IN sides wherever an arc has its counter at both of its ends.  The deciding lane
//     1. walks P, at most max_len k-mers, to v
//     2. takes L from the step out of rc(x0), and u = rc(L)
//     3. for every other base c of out_u (at most three): q0 = next(u, c) must be solid, and the left side of q0 must have reason
//        BRANCH_IN with L, in L's orientation, behind it
//     4. walks from q0 to the right through open sides, at most max_len k-mers
//     5. Q is a sibling when that walk ends with BRANCH_IN at v in v's orientation and the lengths are within max_diff
// which is at most n + 1 + 3 (max_len + 2) dependent slot reads.  The decide pass only reads.
// Corners, decided here: the candidates a round KEEPS (out_totals[3]) are the branches, in their deciding orientation, that were not
// popped, whether they have a sibling or not.  A fork that reaches v by an arc with no k-mer between is no sibling (step 3 needs a
// solid q0 with u behind it, step 5 a walk that ends at v), so a branch beside such an arc is kept.
//
// A ROUND decides over the index as it stood when the round began, then applies:
//     the value word of every k-mer of every minor branch becomes 0: ktip.hpp's tombstone, so no read-side code changes
//     the branch is cut from BOTH junctions as a tip is cut from its one: in v's word the in-counter for the first base of x(n-1)
//     becomes 0, and in L's word the in-counter for the first base of rc(x0), which is u's out-counter for the branch
// and nothing else is written.  A popped index is meant to be used at the same or higher thresholds.  A branch with a tip on it, or a
// bubble inside a branch, is not linear and waits: the caller alternates rounds of the two operators (KmerIndex.simplify).
//
// Why the apply pass needs no locks.  A branch's k-mers lie in that unitig alone (kunitig.hpp).  A junction is a member of no branch:
// v has BRANCH_IN towards P, so in_v holds another base beside P's, and the side of v that faces P -- the right side of rc(v), whose out
// set is the complement of in_v -- is BRANCH_OUT; the same holds for L.  A member's sides are open or, at the two ends, BRANCH_IN, never
// BRANCH_OUT.  So the only words two lanes may write together are junction words, each lane clearing its own counter -- two branches
// that enter v by the same base would share their last k-mer --, with a vector atomicAnd on the 32-bit half that holds it, in plain
// C++.  v's in-half and L's in-half of one k-mer that is v of one bubble and u of the next are the two different halves of its word.
// Every other write is a lane's own plain store.  The apply walk follows each k-mer's single out arc as read from the k-mer's OWN word,
// which no other lane writes, and does not test the successor again: another lane may be changing the junction just then.
// (Hand-made records whose arcs disagree at their two ends can make a junction a member of another branch: in_v is then one base that
// is not P's.  The result is still one: the cleared counter was below min_arc already, so the thresholded out set that branch's walk
// reads from that half is the same before and after the atomicAnd, and a zeroed word stays zero under the AND in either order.  With
// such records the mirrored view may also see other siblings than this one; a branch is decided from one start only, so the round is
// a function of the index all the same.)
//
// One piece of PG_HD code for the round's kernels (kindex_kernels.hip: kedit_decide_kernel, kedit_apply_kernel) and its host twin
// (kedit_host.cpp), which see it as KbubbleOp (kedit.hpp): kbubble_decide reads, kbubble_apply writes through two functions of the caller
// and leaves the right side and the zeroing to ktip_apply.  Loop state is kept with selects (DESIGN.md §11 on what stores under branches
// inside such a loop became).
#pragma once
#include "ktip.hpp"

namespace pg {

constexpr uint32_t KBUBBLE_MAX_LEN = 1u << 16, KBUBBLE_MAX_DIFF = 1u << 16;

struct KbubbleParams {
    uint32_t min_cov, min_arc, max_len, max_diff;
};

// the node read the other way: its reverse complement, with the same word and slot
template <int NW>
PG_HD KwalkNode<NW> kbubble_flip(const KwalkNode<NW>& x) { return KwalkNode<NW>{x.b, x.a, x.w, x.slot, !x.fwd}; }

// Steps 1 and 2 of the decision, which the bulges (kbulge.hpp) share.  branch: the start is a branch in its deciding orientation, and then
// v and L are its junctions; P.n is the k-mers walked (0: the left side is not BRANCH_IN)
template <int NW>
struct KbubbleArm {
    bool branch;
    KeditPath P;
    KwalkNode<NW> v, L;
};

// The arm of the start x0 whose left side has reason `left`.  Only reads
template <int NW, typename Find>
PG_HD KbubbleArm<NW> kbubble_arm(const KwalkNode<NW>& x0, uint32_t left, int K, const Kmer<NW>& filter, const KunitigParams& up, Find find) {
    KbubbleArm<NW> arm{};
    if (left != KWALK_BRANCH_IN) return arm;
    // 1. P, to v; decided from the start that is not greater
    KwalkNode<NW> x = x0;
    arm.P = kedit_path<NW>(x, arm.v, K, filter, up, find);
    if (arm.P.reason != KWALK_BRANCH_IN || kmer_less<NW>(x.b, x0.a)) return arm;
    // 2. L behind the left side, and the fork u = rc(L)
    int base = 0;
    const uint32_t behind = kunitig_side<NW>(kbubble_flip<NW>(x0), K, filter, up, find, arm.L, base);
    arm.branch = behind == KWALK_BRANCH_IN && !kmer_eq<NW>(kwalk_canon<NW>(arm.L), kwalk_canon<NW>(arm.v));
    return arm;
}

// The decision for the start x0 whose left side has reason `left`; candidate: a branch in its deciding orientation.  Only reads
template <int NW, typename Find>
PG_HD KeditDecision kbubble_decide(const KwalkNode<NW>& x0, uint32_t left, int K, const KbubbleParams& pr, Find find) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const KunitigParams up{pr.min_cov, pr.min_arc, pr.max_len};
    const KbubbleArm<NW> arm = kbubble_arm<NW>(x0, left, K, filter, up, find);
    if (!arm.branch) return KeditDecision{arm.P.n, false, false};
    const KeditPath& P = arm.P;
    const KwalkNode<NW>&v = arm.v, &L = arm.L;
    int base = 0;
    const KwalkNode<NW> u = kbubble_flip<NW>(L);
    const uint32_t others = kwalk_out_set(u.w, u.fwd, pr.min_arc) & ~(1u << (int)(x0.a.w[NW - 1] & 3));
    bool minor = false;
    for (int c = 0; c < 4; c++) {
        if (!(others >> c & 1u)) continue;
        // 3. q0 = next(u, c): solid, and attached to u by BRANCH_IN on its left
        KwalkNode<NW> q = u, y;
        kmer_roll<NW>(q.a, q.b, c, K, filter);
        q.fwd = !kmer_less<NW>(q.b, q.a);
        q.slot = 0;
        q.w = find(kwalk_canon<NW>(q), q.slot);
        if (!kcor_solid_word(q.w, pr.min_cov)) continue;
        const uint32_t back = kunitig_side<NW>(kbubble_flip<NW>(q), K, filter, up, find, y, base);
        if (back != KWALK_BRANCH_IN || !kmer_eq<NW>(y.a, L.a)) continue;
        // 4., 5. Q, to v in v's orientation, the lengths within max_diff; the means compared by cross-multiplication
        const KeditPath Q = kedit_path<NW>(q, y, K, filter, up, find);
        const uint32_t diff = P.n > Q.n ? P.n - Q.n : Q.n - P.n;
        const bool sibling = Q.reason == KWALK_BRANCH_IN && kmer_eq<NW>(y.a, v.a) && diff <= pr.max_diff;
        minor = sibling && P.cov * (uint64_t)Q.n < Q.cov * (uint64_t)P.n ? true : minor;
    }
    return KeditDecision{P.n, true, minor};
}

// The minor branch of n k-mers from x0 applied: L is named by the single out arc of rc(x0) as x0's own word has it and looked up
// -- find(ck, slot) = kunitig_probe --, clear(slot, fwd, a) takes L's in-counter for the first base of rc(x0); then ktip_apply: zero(slot)
// for each of the n k-mers, and clear for v behind the n-th
template <int NW, typename Find, typename Zero, typename Clear>
PG_HD void kbubble_apply(const KwalkNode<NW>& x0, uint32_t n, int K, const KbubbleParams& pr, Find find, Zero zero, Clear clear) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    KwalkNode<NW> r = kbubble_flip<NW>(x0);
    const int base = kwalk_lowest(kwalk_out_set(r.w, r.fwd, pr.min_arc));
    const int a = (int)(r.b.w[NW - 1] & 3) ^ 2;                                   // (the first base of rc(x0))
    kmer_roll<NW>(r.a, r.b, base, K, filter);
    r.fwd = !kmer_less<NW>(r.b, r.a);
    r.slot = 0;
    (void)find(kwalk_canon<NW>(r), r.slot);
    clear(r.slot, r.fwd, a);
    ktip_apply<NW>(x0, n, K, KtipParams{pr.min_cov, pr.min_arc, pr.max_len}, find, zero, clear);
}

// The bubbles as the round sees them (kedit.hpp)
struct KbubbleOp {
    using Params = KbubbleParams;
    static PG_HD KunitigParams ends(const Params& pr) { return KunitigParams{pr.min_cov, pr.min_arc, pr.max_len}; }
    static PG_HD bool starts(uint32_t left) { return left == KWALK_BRANCH_IN; }
    template <int NW, typename Find>
    static PG_HD KeditDecision decide(const KwalkNode<NW>& x0, uint32_t left, int K, const Params& pr, Find find) {
        return kbubble_decide<NW>(x0, left, K, pr, find);
    }
    template <int NW, typename Find, typename Zero, typename Clear>
    static PG_HD void apply(const KwalkNode<NW>& x0, uint32_t n, int K, const Params& pr, Find find, Zero zero, Clear clear) {
        kbubble_apply<NW>(x0, n, K, pr, find, zero, clear);
    }
};

}  // namespace pg
