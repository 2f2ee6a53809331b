// map_decide.hpp -- the `map` stage's per-read decision (parse1read, standardPregraph/prlRead2Ctg.c:260-361), host + device (PG_HD).
//
// A read's k-mers are looked up in the contig k-mer index (map_kernels.hip); every k-mer position j gets one 64-bit hit word:
//   0                                       no node: the canonical k-mer is not in the index, or it is deleted (searchKmer, :233-246)
//   ctg | (pos << 2 | twin << 1 | smaller) << 32
//                                           ctg = the contig id the index keeps (> 0, prlHashCtg.c:436), pos = the k-mer's position on
//                                           that contig (the reference's 24-bit r_links field, inc/newhash.h:95: positions wrap at 2^24),
//                                           twin = which strand of the contig is canonical there, smaller = which strand of the read is
// The decision is the reference's: every distinct contig id counts its hits (`flag`) at its FIRST hit; ids with flag >= multi count
// (`counter`), and the chosen one is the first, in first-hit order, whose flag is strictly the largest; `counter2` (ids with two hits or
// more when K < 32, every id when K > 32) above one sets the read's footprint.  The device runs it in registers for up to MAP_FAST_IDS
// distinct ids and falls back to the reference's quadratic scan over the row beyond that; the CPU tests run this same function.
#pragma once
#include <stdint.h>

#include "kmer.hpp"

namespace pg {

constexpr int MAP_FAST_IDS = 8;
constexpr uint32_t MAP_POS_MASK = 0xFFFFFFu;          // r_links: 4 * EDGE_BIT_SIZE = 24 bits

PG_HD uint64_t map_hit(uint32_t ctg, uint32_t pos, int twin, int smaller) {
    return (uint64_t)ctg | ((uint64_t)(((pos & MAP_POS_MASK) << 2) | ((uint32_t)twin << 1) | (uint32_t)smaller) << 32);
}

// contig_array[].length / .bal_edge (basicContigInfo, prlRead2Ctg.c:727-770), indexed by contig id; ids past n read as length 0,
// bal_edge 1 (the reference would read past its array)
struct MapCtgs {
    const int32_t* len;
    const int8_t* bal;
    uint32_t n;                                        // entries: ids 0 .. n - 1
};

// what parse1read leaves for the read: ctgIdArray (after getTwinCtg), posArray, orienArray, footprint.  ctg = 0: not mapped (pos and
// orien are then not looked at by the writers, and stay 0 here)
struct MapOut {
    uint32_t ctg;
    int32_t pos;
    uint8_t orien;                                     // '+' or '-'
    uint8_t footprint;
};

// multi threshold of a read (prlRead2Ctg.c:272-273); align_len = the batch's ALIGNLEN
PG_HD int map_multi(int len, int align_len, int K) {
    const int alldgn = len > align_len ? align_len : len;
    return alldgn - K + 1 < 2 ? 2 : alldgn - K + 1;
}

// The tail of parse1read (:328-360) for a read that maps: h = the hit word of the chosen id's first hit, best = that k-mer's index in the
// read, counter2 = the ids that count towards the footprint.  Shared by map_decide, the wave-per-read kernel and the host twin.
PG_HD MapOut map_place(uint64_t h, int best, int K, int counter2, const MapCtgs& ctgs) {
    MapOut o{0, 0, 0, 0};
    o.footprint = counter2 > 1 ? 1 : 0;
    const uint32_t contig = (uint32_t)h, i = (uint32_t)best + 1;
    const uint32_t hi = (uint32_t)(h >> 32), pos = hi >> 2;
    const int twin = (int)((hi >> 1) & 1), smaller = (int)(hi & 1);
    const uint32_t ctg_len = contig < ctgs.n ? (uint32_t)ctgs.len[contig] : 0u;
    if (twin == smaller) {                                         // unsigned arithmetic as the reference's (:351)
        o.orien = '-';
        o.ctg = contig + (uint32_t)(contig < ctgs.n ? (int)ctgs.bal[contig] : 1) - 1u;      // getTwinCtg, attachPEinfo.c:666
        o.pos = (int32_t)(ctg_len - pos - (uint32_t)K - i + 1u);
    } else {
        o.orien = '+';
        o.ctg = contig;
        o.pos = (int32_t)(pos - i + 1u);
    }
    return o;
}

// a read's row of hit words in memory, as map_decide's Row
struct MapRow {
    const uint64_t* p;
    PG_HD uint64_t operator()(int j) const { return p[j]; }
};

// row(j) = hit word of k-mer j, nk = number of k-mers (0 for reads shorter than K + 1)
template <typename Row>
PG_HD MapOut map_decide(const Row& row, int nk, int K, int multi, const MapCtgs& ctgs) {
    MapOut o{0, 0, 0, 0};
    if (nk <= 0) return o;
    uint32_t id[MAP_FAST_IDS];
    int cnt[MAP_FAST_IDS], first[MAP_FAST_IDS];
    int n = 0;
    bool over = false;
#pragma unroll
    for (int q = 0; q < MAP_FAST_IDS; q++) { id[q] = 0; cnt[q] = 0; first[q] = 0; }
    for (int j = 0; j < nk && !over; j++) {
        const uint32_t c = (uint32_t)row(j);
        if (!c) continue;
        bool found = false;
#pragma unroll
        for (int q = 0; q < MAP_FAST_IDS; q++)
            if (q < n && id[q] == c) { cnt[q]++; found = true; }
        if (found) continue;
        if (n == MAP_FAST_IDS) { over = true; break; }
#pragma unroll
        for (int q = 0; q < MAP_FAST_IDS; q++)
            if (q == n) { id[q] = c; cnt[q] = 1; first[q] = j; }
        n++;
    }
    int counter = 0, counter2 = 0, max_occ = 0, best = -1;
    auto visit = [&](int flag, int j) {
        if ((K < 32 && flag >= 2) || K > 32) counter2++;
        if (flag < multi) return;
        counter++;
        if (flag > max_occ) { max_occ = flag; best = j; }
    };
    if (!over) {
#pragma unroll
        for (int q = 0; q < MAP_FAST_IDS; q++)
            if (q < n) visit(cnt[q], first[q]);
    } else {                                                       // the reference's own scan (:282-326)
        for (int j = 0; j < nk; j++) {
            const uint32_t c = (uint32_t)row(j);
            if (!c) continue;
            bool seen = false;
            for (int i = 0; i < j && !seen; i++) seen = (uint32_t)row(i) == c;
            if (seen) continue;
            int flag = 1;
            for (int s = j + 1; s < nk; s++) flag += (uint32_t)row(s) == c ? 1 : 0;
            visit(flag, j);
        }
    }
    if (!counter) return o;
    return map_place(row(best), best, K, counter2, ctgs);
}

}  // namespace pg
