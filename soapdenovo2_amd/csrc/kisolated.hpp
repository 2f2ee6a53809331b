// kisolated.hpp -- short isolated unitigs dropped from the graph of the k-mer index (pg_kindex_drop_isolated, include/soapdenovo2_amd.h
// section 3).  The arcs, the tips, the bubbles and the bulges (karc.hpp, ktip.hpp, kbubble.hpp, kbulge.hpp) take the
// errors off the real path; what they leave beside it on real reads is debris that hangs on nothing: short chains of error k-mers that
// passed min_cov and touch no other solid k-mer.  ktip.hpp names the case -- "both sides free (an island)" -- and passes it by; this is
// the operator that removes it, the fifth that writes to the table.
//
// Solid, out_x, in_x, min_cov (1..255), min_arc (1..63), the side test, the end reasons and linear unitigs are kunitig.hpp's
// (kunitig_side); FREE is ktip.hpp's ktip_free: KWALK_DEAD_END or KWALK_WEAK_NEXT.
//
// An ISLAND is a linear unitig x0 -> ... -> x(n-1) of that rule with
//     the left side of x0 free
//     the right side of x(n-1) free
//     n <= max_len (1 .. 2^16 k-mers)
// and it is REMOVED iff cov <= max_cov * n, cov the sum of its k-mers' coverage bytes, both sides of the comparison 64-bit integers;
// max_cov is 1 .. 255.  The coverage byte saturates at 255, so max_cov = 255 removes every island within max_len; a smaller bound keeps
// a short fragment of high coverage -- a plasmid piece, a contig between two coverage dips -- while error debris goes.
// Every other pair of reasons is no island and nothing of it is written: a tip (free / BRANCH_IN), the path before a fork (BRANCH_OUT),
// a chain with KUNITIG_HAIRPIN on either side, a ring (it has no end, so no start in this round), a chain longer than max_len -- the walk
// runs with max_kmers = max_len and reports it as KUNITIG_CUT.
//
// The duplicate rule.  Unlike a tip, an island has both of its orientations in the start list: s = x0 and e = rc(x(n-1)) are both
// starts that are free on the left.  The walk from s ends with e in hand, and the start is a candidate only when !kmer_less(e, s):
// kunitig_chain's emit rule, so the copy that decides is the one the unitigs emit.  The other copy is no candidate and not minor, so
// neither `removed` nor `kept` counts an island twice.  n = 1 is the sharp case: the two starts are the two orientations of one slot,
// and with K odd no k-mer is its own reverse complement, so s != e and exactly one of the two decides.
//
// A ROUND decides over the index as it stood when the round began, then applies: the value word of every k-mer of every removed island
// becomes 0, a tombstone as the tips leave it (ktip.hpp), and nothing else is written -- an island has no junction.  Arcs below min_arc
// or into k-mers below min_cov that point at a removed k-mer from elsewhere stay: an edited index is meant to be used at the same or
// higher thresholds.  On records whose arcs agree at their two ends (pass 1 counts an arc at both) removing an island makes nothing
// else an island -- no solid k-mer has an arc to it --, so the second round removes nothing; a caller still runs rounds until one does
// (KmerIndex.drop_isolated), as for the siblings.
// The totals: islands removed, k-mers removed, solid k-mers before the round, islands kept: those within max_len but above max_cov.
//
// Why the apply pass needs no locks.  An island's k-mers lie in that unitig alone: a linear unitig's k-mers lie in no other unitig
// (kunitig.hpp), so no two removed islands share a word.  Only one of an island's two starts is minor, so one lane walks it, and that
// lane reads each k-mer's word before it zeroes it.  No junction word is written: the walk stops behind the n-th k-mer and never calls
// clear, so every write is the lane's own plain store of 0 to a word no other lane reads or writes in this pass.
//
// One piece of PG_HD code for the round's kernels (kindex_kernels.hip: kedit_decide_kernel, kedit_apply_kernel) and its host twin
// (kedit_host.hpp), which see it as KisolatedOp (kedit.hpp).  Loop state is kept with selects (DESIGN.md §11 on what stores under branches
// inside such a loop became).
#pragma once
#include "ktip.hpp"

namespace pg {

constexpr uint32_t KISOLATED_MAX_LEN = 1u << 16;

struct KisolatedParams {
    uint32_t min_cov, min_arc, max_len, max_cov;
};

// The decision for the start x0 whose left side has reason `left`: at most max_len k-mers to the right through open sides; candidate:
// free on both sides, n <= max_len, and the copy the unitigs emit; minor: its coverage sum is at most max_cov a k-mer.  Only reads
template <int NW, typename Find>
PG_HD KeditDecision kisolated_decide(const KwalkNode<NW>& x0, uint32_t left, int K, const KisolatedParams& pr, Find find) {
    if (!ktip_free(left)) return KeditDecision{1, false, false};
    KwalkNode<NW> x = x0, y;
    const KeditPath P = kedit_path<NW>(x, y, K, kmer_filter<NW>(K), KunitigParams{pr.min_cov, pr.min_arc, pr.max_len}, find);
    const bool candidate = ktip_free(P.reason) && !kmer_less<NW>(x.b, x0.a);     // (x is the last k-mer: x.b = e, x0.a = s)
    return KeditDecision{P.n, candidate, candidate && P.cov <= (uint64_t)pr.max_cov * (uint64_t)P.n};
}

// The removed island of n k-mers from x0 applied: the tip's walk (ktip_apply) without the junction -- every k-mer's successor is named by
// the single out arc of the k-mer's own word and looked up, find(ck, slot) = kunitig_probe, then zero(slot) is called for the k-mer just
// left.  The n-th k-mer has no arc to follow and nothing behind it is looked up
template <int NW, typename Find, typename Zero>
PG_HD void kisolated_apply(const KwalkNode<NW>& x0, uint32_t n, int K, const KisolatedParams& pr, Find find, Zero zero) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    KwalkNode<NW> x = x0;
    for (uint32_t i = 1; i < n; i++) {
        const uint64_t left = x.slot;
        const int base = kwalk_lowest(kwalk_out_set(x.w, x.fwd, pr.min_arc));
        kmer_roll<NW>(x.a, x.b, base, K, filter);
        x.fwd = !kmer_less<NW>(x.b, x.a);
        x.slot = 0;
        x.w = find(kwalk_canon<NW>(x), x.slot);
        zero(left);
    }
    zero(x.slot);
}

// The islands as the round sees them (kedit.hpp)
struct KisolatedOp {
    using Params = KisolatedParams;
    static PG_HD KunitigParams ends(const Params& pr) { return KunitigParams{pr.min_cov, pr.min_arc, pr.max_len}; }
    static PG_HD bool starts(uint32_t left) { return ktip_free(left); }
    template <int NW, typename Find>
    static PG_HD KeditDecision decide(const KwalkNode<NW>& x0, uint32_t left, int K, const Params& pr, Find find) {
        return kisolated_decide<NW>(x0, left, K, pr, find);
    }
    template <int NW, typename Find, typename Zero, typename Clear>
    static PG_HD void apply(const KwalkNode<NW>& x0, uint32_t n, int K, const Params& pr, Find find, Zero zero, Clear) {
        kisolated_apply<NW>(x0, n, K, pr, find, zero);
    }
};

}  // namespace pg
