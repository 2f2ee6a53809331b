// karc.hpp -- arcs to weak k-mers dropped from the graph of the k-mer index (pg_kindex_drop_weak_arcs, include/soapdenovo2_amd.h section 3;
// DESIGN.md §17).  The arc counters and the coverage are thresholded independently, so a solid k-mer can hold an arc, its counter at
// least min_arc, to a k-mer that every operator reads as absent: an error arm whose first k-mer has coverage below min_cov.  The fork
// then has several arcs out for ever -- the tips (ktip.hpp) and the bubbles (kbubble.hpp) remove k-mers, never an arc alone --, and the
// unitigs of kunitig.hpp end there.  This is the third operator that writes to the table, and the first that removes no k-mer.
//
// Solid, out_x, min_cov (1..255), min_arc (1..63), the side test and the end reasons are kunitig.hpp's (kunitig_side).
//
// The arc of a solid oriented k-mer r by base b, its out-counter in r's word at least min_arc, is DANGLING when next(r, b) is not solid:
// the table has no such key, its word is 0 (a tombstone), or its coverage is below min_cov (the deleted bit reads as coverage 0).
// A ROUND decides over the index as it stood when the round began, then applies: every dangling arc's out-counter becomes 0, in r's own
// word only.  The weak k-mer's word is not touched, and neither is a counter below min_arc.
//
// A side holds a dangling arc only if its reason is BRANCH_OUT (several arcs, some may dangle) or WEAK_NEXT (one arc, and it dangles), so
// those are the starts taken (kunitig.hpp: kunitig_start), and the side is that of r = rc(x0), x0 the start's node.  The decision's n is
// the number of dangling arcs of the side, at most 4; every side taken is a candidate and one with n > 0 is "minor", so the round's
// totals (kedit.hpp) read: sides pruned, arcs cleared, solid k-mers before the round, sides kept -- BRANCH_OUT sides without a dangling arc.
//
// Why the apply pass needs no locks.  A side is exactly one start, so one lane owns the out-half of r's word, one 32-bit half of it; the
// two sides of a k-mer are the two halves.  An out-counter of r is the in-counter of rc(r) for the complemented base (kedit_in_half,
// kedit_in_index), so the write is the round's clear(slot, !r.fwd, b ^ 2): the vector atomicAnd on that half, in plain C++.  Clearing
// arc counters never changes whether a k-mer is solid -- the coverage byte is not touched, and a solid word, coverage at least 1, never
// becomes 0 --, so the apply pass, which looks the targets up again, sees what the decide pass saw, whatever other lanes have written.
// For the same reason a second round finds nothing: no target became weak, and the dangling counters are 0.
//
// One piece of PG_HD code for the round's kernels (kindex_kernels.hip: kedit_decide_kernel, kedit_apply_kernel) and its host twin
// (kedit_host.hpp), which see it as KarcOp (kedit.hpp).  The up-to-four lookups are independent: all four targets are computed first,
// then probed, with no exit between them, and the set is kept with selects.
#pragma once
#include "kbubble.hpp"

namespace pg {

struct KarcParams {
    uint32_t min_cov, min_arc;
};

// The bases b whose arc out of the solid node r dangles, as a set of four bits.  Only reads; find(ck, slot) = kunitig_probe
template <int NW, typename Find>
PG_HD uint32_t karc_dangling(const KwalkNode<NW>& r, int K, const KarcParams& pr, Find find) {
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const uint32_t out = kwalk_out_set(r.w, r.fwd, pr.min_arc);
    Kmer<NW> target[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        Kmer<NW> a = r.a, c = r.b;
        kmer_roll<NW>(a, c, b, K, filter);
        target[b] = kmer_less<NW>(c, a) ? c : a;
    }
    uint32_t dangling = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        uint64_t slot = 0, w = 0;
        if (out >> b & 1u) w = find(target[b], slot);                            // (a base with no arc is not looked up: it cannot dangle)
        dangling |= (out >> b & 1u) && !kcor_solid_word(w, pr.min_cov) ? 1u << b : 0u;
    }
    return dangling;
}

PG_HD uint32_t karc_count(uint32_t set) { return (set & 1u) + (set >> 1 & 1u) + (set >> 2 & 1u) + (set >> 3 & 1u); }

// The arcs as the round sees them (kedit.hpp)
struct KarcOp {
    using Params = KarcParams;
    static PG_HD KunitigParams ends(const Params& pr) { return KunitigParams{pr.min_cov, pr.min_arc, 1}; }
    static PG_HD bool starts(uint32_t left) { return left == KWALK_BRANCH_OUT || left == KWALK_WEAK_NEXT; }
    template <int NW, typename Find>
    static PG_HD KeditDecision decide(const KwalkNode<NW>& x0, uint32_t, int K, const Params& pr, Find find) {
        const uint32_t n = karc_count(karc_dangling<NW>(kbubble_flip<NW>(x0), K, pr, find));
        return KeditDecision{n, true, n > 0};
    }
    // the side's dangling arcs found again and cleared: each is r's out-counter for b, the in-counter of rc(r) for b ^ 2
    template <int NW, typename Find, typename Zero, typename Clear>
    static PG_HD void apply(const KwalkNode<NW>& x0, uint32_t, int K, const Params& pr, Find find, Zero, Clear clear) {
        const KwalkNode<NW> r = kbubble_flip<NW>(x0);
        const uint32_t dangling = karc_dangling<NW>(r, K, pr, find);
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (dangling >> b & 1u) clear(r.slot, !r.fwd, b ^ 2);
    }
};

}  // namespace pg
