// kunitig_host.hpp -- what the host twins of the operators on the graph of the k-mer index share (kunitig_host.cpp and
// kunitig_rank_host.cpp: the two unitig engines; kedit_host.hpp: an edit round), over a device = -1 index in one table: the table as a
// twin reaches it, the ends sweep that fills a start list (kunitig_ends_kernel's), and the sequential counterpart of the scan with the
// finish behind it (kunitig_scan_sums_kernel's, and what kidx_scan_before hands a lane).  Host only, beside kedit_host.hpp.
#pragma once
#include <vector>

#include "kindex.hpp"
#include "kunitig.hpp"

namespace pg {

template <int NW>
struct KunitigHostTable {
    static constexpr int SW = map_slot_words<NW>();
    const uint64_t* tab;
    uint64_t slots, mask;
    int K;
    explicit KunitigHostTable(const pg_kindex* ix) : tab(ix->ranks[0].tab.data()), slots(ix->ranks[0].slots), mask(ix->ranks[0].slots - 1), K(ix->K) {}
    const uint64_t* slot(uint64_t e) const { return tab + e * SW; }
    bool solid_at(uint64_t e, uint32_t min_cov) const { return slot(e)[NW + 1] != KIDX_EMPTY && kcor_solid_word(slot(e)[NW], min_cov); }
    // every lookup of a twin: kunitig_probe
    auto find() const {
        return [tab = tab, mask = mask](const Kmer<NW>& ck, uint64_t& at) { return kunitig_probe<NW>(tab, mask, ck, at); };
    }
    // the node a start names
    KwalkNode<NW> node_of(uint64_t start) const {
        const uint64_t* sl = slot(kunitig_start_slot(start));
        return kunitig_node<NW>(kidx_record_key<NW>(sl), sl[NW], kunitig_start_slot(start), kunitig_start_fwd(start), K);
    }
};

// the ends: every end side of a solid k-mer becomes a start, in slot order.  Returns the solid k-mers
template <int NW>
uint64_t kunitig_host_ends(const KunitigHostTable<NW>& t, const KunitigParams& pr, std::vector<uint64_t>& starts) {
    uint64_t solid = 0;
    for (uint64_t e = 0; e < t.slots; e++) {
        if (!t.solid_at(e, pr.min_cov)) continue;
        solid++;
        uint32_t reasons[2];
        const uint32_t ends = kunitig_ends<NW>(kidx_record_key<NW>(t.slot(e)), t.slot(e)[NW], e, t.K, pr, t.find(), reasons);
        for (int side = 0; side < 2; side++)
            if (ends >> side & 1) starts.push_back(kunitig_start(e, side == 0, reasons[side]));
    }
    return solid;
}

// the scan's sums over a length list
inline KidxCounts kunitig_host_sums(const std::vector<uint32_t>& lens, int K) {
    KidxCounts total{{0, 0, 0, 0}};
    for (uint32_t n : lens)
        for (int i = 0; i < KIDX_COUNTS; i++) total.c[i] += kunitig_counts(n, K).c[i];
    return total;
}

// The scan in full mode, where the finish said go: each(i, u, at, base) for every start i, in order -- the unitigs, words and k-mers of
// the kept starts before it --, then the last offsets and the tail
template <typename Each>
void kunitig_host_scan(const std::vector<uint32_t>& lens, int K, int tail, uint64_t* packed_out, uint64_t* word_off_out, uint64_t* kmer_base_out, Each each) {
    KidxCounts before{{0, 0, 0, 0}};
    for (size_t i = 0; i < lens.size(); i++) {
        each(i, before.c[0], before.c[1], before.c[2]);
        for (int q = 0; q < KIDX_COUNTS; q++) before.c[q] += kunitig_counts(lens[i], K).c[q];
    }
    kunitig_finish_tail(before, tail, packed_out, word_off_out, kmer_base_out);
}

}  // namespace pg
