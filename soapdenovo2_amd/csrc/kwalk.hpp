// kwalk.hpp -- unitigs walked from sequence ends over the arc counters of the k-mer index (pg_kindex_walk, include/soapdenovo2_amd.h
// section 3).  The index's value is the reference's kmer_t counter word (kmer.hpp, "node counter word"): four 6-bit left-arc
// counters in word A and four 6-bit right-arc counters in word B, so the table is the de Bruijn graph of the read set with its arc
// multiplicities, and a walk follows it while it is unambiguous.  The reference builds its unitigs from the same counters once, for the
// whole graph (node2edge.c); this is the operator for a batch of chosen ends: gap closing, contig-end extension, a bait's neighbourhood.
//
// Sequence r of a batch (KidxBatch, kindex.hpp) yields two walks, both "extend to the right of an oriented k-mer":
//   walk 2r      starts at the sequence's last k-mer, as read
//   walk 2r + 1  starts at the reverse complement of its first k-mer: the sequence's left extension is the reverse complement of this walk's text
// A sequence of exactly K bases is a seed k-mer (its first and last k-mer coincide); one without a k-mer gives two empty walks.
//
// Arcs of an oriented k-mer x whose canonical form c has word w (the convention of pass 1's counting: a k-mer met as its reverse complement
// takes the complement of the next base as its left neighbour):
//   x == c       out(b) = right counter b        in(a) = left counter a
//   x == rc(c)   out(b) = left counter b ^ 2     in(a) = right counter a ^ 2
// An arc exists when its counter is >= min_arc (1..63).  Solid is the corrector's kcor_solid_word: present, coverage >= min_cov (1..255).
// (K is odd wherever pass 1 made the records, so x == rc(x) does not occur; it would read as x == c.)
//
// A walk:
//   1. the start k-mer is looked up.  No k-mer: KWALK_NO_KMER; not solid: KWALK_SEED_WEAK; both with length 0
//   2. from the current x, whose word is in hand:
//        B = { b : out_x(b) >= min_arc }        empty: KWALK_DEAD_END, more than one: KWALK_BRANCH_OUT
//        y = next(x, b), canon(y) is looked up  not solid: KWALK_WEAK_NEXT
//        { a : in_y(a) >= min_arc } must be exactly { first base of x }      else KWALK_BRANCH_IN
//        canon(y) == the start's canonical k-mer                             KWALK_LOOP, the base is not appended
//        b is appended, y's coverage joins the walk's sum, x = y;  length == max_ext: KWALK_MAX_EXT_REACHED
// One dependent slot read per appended base: the current word names the only candidate successor.
//
// max_ext is 1 .. KWALK_MAX_EXT = 2^20 bases: a row of the output is pg_packed_words(max_ext) words, 256 KiB at the bound, and a length
// fits the report's low 32 bits many times over; values above it are refused.
//
// Outputs of walk v (either may be null):
//   ext[v * pg_packed_words(max_ext) + q]   the appended bases as pg_pack_read lays them out, pad bits zero, every word of the row written
//   report[2 v]      length in bits 31:0, stop reason (1..8) in bits 39:32
//   report[2 v + 1]  the sum of coverage of the appended k-mers
//
// One piece of PG_HD code for the kernel (kindex_kernels.hip: kwalk_kernel) and the host twin (kwalk_host.cpp), and the two pieces the
// unitigs (kunitig.hpp) share with the walk: kwalk_step, step 2 above up to BRANCH_IN -- what follows a good step is the caller's: the
// walk compares with its start (LOOP), the unitigs with x (HAIRPIN) and, for rings, with their first k-mer -- and KwalkText, the base
// writer.  The lookup is a function find(ck, slot&) of the canonical k-mer that may also say where the key lies; the walk's callers
// pass one that leaves the slot alone.  The 32 bases being filled stay in one word and are stored when it is full; stop reason and
// length are kept with selects (DESIGN.md §11 on what stores under branches inside such a loop became).
#pragma once
#include "kcorrect.hpp"

namespace pg {

constexpr uint32_t KWALK_MAX_EXT = 1u << 20;
enum : uint32_t {
    KWALK_NO_KMER = 1, KWALK_SEED_WEAK = 2, KWALK_DEAD_END = 3, KWALK_BRANCH_OUT = 4, KWALK_WEAK_NEXT = 5, KWALK_BRANCH_IN = 6, KWALK_LOOP = 7,
    KWALK_MAX_EXT_REACHED = 8,
};

struct KwalkParams {
    uint32_t min_cov, min_arc, max_ext;
};

PG_HD uint64_t kwalk_row_words(uint32_t max_ext) { return ((uint64_t)max_ext + 31) / 32; }
PG_HD uint64_t kwalk_report_word(uint32_t len, uint32_t reason) { return (uint64_t)len | (uint64_t)reason << 32; }

// bit b is set when the 6-bit counter b of `links` (four of them, counter b at bits 6 b + 5 : 6 b) is >= min_arc
PG_HD uint32_t kwalk_arc_set(uint32_t links, uint32_t min_arc) {
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) m |= ((links >> (6 * b)) & 63u) >= min_arc ? 1u << b : 0u;
    return m;
}
// the set with every base complemented: bit b becomes bit b ^ 2
PG_HD uint32_t kwalk_complement_set(uint32_t m) { return ((m >> 2) | (m << 2)) & 15u; }

// the bases that may follow / precede an oriented k-mer whose canonical form has word w; fwd: the k-mer is its canonical form
PG_HD uint32_t kwalk_out_set(uint64_t w, bool fwd, uint32_t min_arc) {
    const uint32_t r = kwalk_arc_set((uint32_t)(w >> 32), min_arc), l = kwalk_arc_set((uint32_t)w, min_arc);
    return fwd ? r : kwalk_complement_set(l);
}
PG_HD uint32_t kwalk_in_set(uint64_t w, bool fwd, uint32_t min_arc) {
    const uint32_t r = kwalk_arc_set((uint32_t)(w >> 32), min_arc), l = kwalk_arc_set((uint32_t)w, min_arc);
    return fwd ? l : kwalk_complement_set(r);
}

// the lowest base of a set that is not empty, and whether a set holds exactly one base
PG_HD int kwalk_lowest(uint32_t m) { return m & 1u ? 0 : m & 2u ? 1 : m & 4u ? 2 : 3; }
PG_HD bool kwalk_single(uint32_t m) { return m != 0 && (m & (m - 1)) == 0; }

// An oriented k-mer with its word in hand: a = the k-mer, b = its reverse complement (KcorCursor's pair: both roll with kmer_roll, the
// canonical key is the smaller), fwd: a is the canonical one, slot: what the lookup said of where the key lies
template <int NW>
struct KwalkNode {
    Kmer<NW> a, b;
    uint64_t w, slot;
    bool fwd;
};
template <int NW>
PG_HD Kmer<NW> kwalk_canon(const KwalkNode<NW>& x) { return x.fwd ? x.a : x.b; }

// The graph step, in place: 0 when the solid node x has one arc out, to a solid y, and that arc is the only one into y; else the first
// of KWALK_DEAD_END, KWALK_BRANCH_OUT, KWALK_WEAK_NEXT, KWALK_BRANCH_IN that applies.  DEAD_END and BRANCH_OUT leave x as it is and
// look nothing up; behind the one lookup x is y whatever is returned, and base the base that led there.  A caller that needs x
// afterwards steps a copy (kunitig.hpp: kunitig_side)
template <int NW, typename Find>
PG_HD uint32_t kwalk_step(KwalkNode<NW>& x, int K, const Kmer<NW>& filter, uint32_t min_cov, uint32_t min_arc, Find find, int& base) {
    const uint32_t out = kwalk_out_set(x.w, x.fwd, min_arc);
    if (!kwalk_single(out)) return !out ? KWALK_DEAD_END : KWALK_BRANCH_OUT;
    base = kwalk_lowest(out);
    const int first = (int)(x.b.w[NW - 1] & 3) ^ 2;                              // (x's first base: the complement of its reverse complement's last)
    kmer_roll<NW>(x.a, x.b, base, K, filter);
    x.fwd = !kmer_less<NW>(x.b, x.a);
    x.slot = 0;
    x.w = find(kwalk_canon<NW>(x), x.slot);
    const bool solid = kcor_solid_word(x.w, min_cov), joined = kwalk_in_set(x.w, x.fwd, min_arc) == 1u << first;
    return !solid ? KWALK_WEAK_NEXT : !joined ? KWALK_BRANCH_IN : 0;
}

// The base writer: a text of `pos` bases so far in the words of row (may be null: nothing is stored), the bases of word pos / 32 in acc
struct KwalkText {
    uint64_t* row;
    uint64_t acc;
    uint32_t pos;
    PG_HD void append(int base) {
        acc |= (uint64_t)base << (62 - 2 * (int)(pos & 31));
        pos++;
        if (!(pos & 31)) {
            if (row) row[pos / 32 - 1] = acc;
            acc = 0;
        }
    }
    // the last word where it is a partial one; the words of the text
    PG_HD uint64_t finish() {
        if (row && (pos & 31)) row[pos / 32] = acc;
        return ((uint64_t)pos + 31) / 32;
    }
};

// One walk.  rd / nk: the sequence's words and k-mers; second: walk 2r + 1 (from the reverse complement of the first k-mer) and not walk 2r
// (from the last one).  find(ck, slot) = the index's word of canonical k-mer ck, 0 when it has none.  row (may be null): the walk's
// kwalk_row_words(max_ext) words; rep (may be null): its two report words
template <int NW, typename Find>
PG_HD void kwalk_one(const uint64_t* rd, int nk, int K, bool second, const KwalkParams& pr, Find find, uint64_t* row, uint64_t* rep) {
    uint32_t reason = KWALK_NO_KMER;
    uint64_t cov = 0;
    KwalkText text{row, 0, 0};
    if (nk > 0) {
        const Kmer<NW> filter = kmer_filter<NW>(K);
        const Kmer<NW> seed = read_kmer<NW>(rd, second ? 0 : nk - 1, K, filter), seed_rc = kmer_rc<NW>(seed, K);
        KwalkNode<NW> x{second ? seed_rc : seed, second ? seed : seed_rc, 0, 0, false};
        x.fwd = !kmer_less<NW>(x.b, x.a);
        const Kmer<NW> start = kwalk_canon<NW>(x);
        x.w = find(start, x.slot);
        reason = kcor_solid_word(x.w, pr.min_cov) ? 0 : KWALK_SEED_WEAK;
        while (!reason) {
            int base = 0;
            reason = kwalk_step<NW>(x, K, filter, pr.min_cov, pr.min_arc, find, base);
            reason = reason ? reason : kmer_eq<NW>(kwalk_canon<NW>(x), start) ? KWALK_LOOP : 0;
            if (reason) break;
            text.append(base);
            cov += kidx_coverage(x.w);
            reason = text.pos == pr.max_ext ? KWALK_MAX_EXT_REACHED : 0;
        }
    }
    if (row)
        for (uint64_t q = text.finish(), row_words = kwalk_row_words(pr.max_ext); q < row_words; q++) row[q] = 0;
    if (rep) {
        rep[0] = kwalk_report_word(text.pos, reason);
        rep[1] = cov;
    }
}

// the device engine (kindex_kernels.hip: kwalk_kernel, a lane per walk): an index in one table, asynchronous on `stream`
int kwalk_device_walk(::pg_kindex* ix, const KidxBatch& b, const KwalkParams& pr, uint64_t* d_ext, uint64_t* d_report, void* stream);

}  // namespace pg
