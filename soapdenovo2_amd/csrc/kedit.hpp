// kedit.hpp -- what the operators that write to the table of the k-mer index share: the tips (ktip.hpp),
// the bubbles (kbubble.hpp), the arcs (karc.hpp), the bulges (kbulge.hpp) and the islands (kisolated.hpp).  A ROUND of such an operator is the unitigs' ends sweep (kunitig.hpp: the start list), a decide pass that
// only reads -- every start over the index as it stood when the round began --, an apply pass that writes, and four totals.  The round
// exists once for the device (kindex_kernels.hip: kedit_decide_kernel, kedit_apply_kernel, kedit_device_round) and once for the host
// (kedit_host.hpp: kedit_host_round); the operator is a stateless struct Op, and this is all of it that either sees:
//     using Params                            the ABI entry's thresholds, passed to the kernels by value
//     static KunitigParams ends(pr)           what the ends sweep runs with
//     static bool starts(left)                the pre-filter on a start's left reason: any other start ends at once, its slot not even read
//     static KeditDecision decide<NW>(x0, left, K, pr, find)              only reads; find(ck, slot) = kunitig_probe
//     static void apply<NW>(x0, n, K, pr, find, zero, clear)              writes through zero(slot): the value word becomes 0, a tombstone,
//                                                                          and clear(slot, fwd, a): one in-counter leaves a junction's word
// The operator's header states its rule and why its apply pass needs no locks.
#pragma once
#include "kunitig.hpp"

namespace pg {

constexpr int KEDIT_TOTALS = 4;
// out_totals: unitigs removed (tips clipped, branches popped, islands dropped), k-mers removed, solid k-mers before the round, candidates kept
enum : int { KEDIT_T_REMOVED = 0, KEDIT_T_KMERS = 1, KEDIT_T_SOLID = 2, KEDIT_T_KEPT = 3 };

// What the decide pass says of a start: n k-mers walked; candidate: the operator's rule names it; minor: a candidate that is removed
struct KeditDecision {
    uint32_t n;
    bool candidate, minor;
};

// the in-counter for base a of a node whose canonical form has word w: which 32-bit half of w (0 the low one), and which of its four
PG_HD int kedit_in_half(bool fwd) { return fwd ? 0 : 1; }
PG_HD int kedit_in_index(bool fwd, int a) { return fwd ? a : a ^ 2; }
// what the atomicAnd leaves of that half: everything but the counter
PG_HD uint32_t kedit_keep_mask(bool fwd, int a) { return ~(63u << (6 * kedit_in_index(fwd, a))); }

// What a walk found: n k-mers, the reason of the side behind the n-th, the sum of their coverage
struct KeditPath {
    uint32_t n, reason;
    uint64_t cov;
};

// From the solid node x to the right through open sides, at most pr.max_kmers k-mers.  Afterwards x is the last k-mer and y the node
// behind its right side (BRANCH_IN: the junction, its word in hand)
template <int NW, typename Find>
PG_HD KeditPath kedit_path(KwalkNode<NW>& x, KwalkNode<NW>& y, int K, const Kmer<NW>& filter, const KunitigParams& pr, Find find) {
    uint32_t n = 1, reason = 0;
    uint64_t cov = kidx_coverage(x.w);
    for (;;) {
        int base = 0;
        reason = kunitig_side<NW>(x, K, filter, pr, find, y, base);
        reason = !reason && n == pr.max_kmers ? KUNITIG_CUT : reason;
        if (reason) break;
        n++;
        cov += kidx_coverage(y.w);
        x = y;
    }
    return KeditPath{n, reason, cov};
}

// The caller's side of the device engine (kindex_kernels.hip, which instantiates it for every operator): one round, asynchronous on `stream`
template <class Op>
int kedit_device_round(::pg_kindex* ix, const typename Op::Params& pr, uint64_t* d_totals, void* stream);

}  // namespace pg
