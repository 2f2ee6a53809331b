// kunitig_rank_host.cpp -- pg_kindex_unitigs_ranked's C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index in
// one table): the bodies of krank.hpp over host memory, the kernels' passes one after the other -- number, sweep, the rounds with their
// control words, the rings, measure, scan, place, emit -- so that the CPU tests run the rounds the kernels run and not another
// algorithm.  A file of its own, as kunitig_host.cpp is: a program that links the index's host half and the walking engine's alone with
// stubs for their device engines keeps linking.
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "kindex.hpp"
#include "krank.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
void krank_host_unitigs(const pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* packed_out,
                        uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* report, uint64_t* totals) {
    constexpr int SW = map_slot_words<NW>();
    const int K = ix->K, R = krank_rounds(ix->ranks[0].keys);
    const KidxRank& t = ix->ranks[0];
    const uint64_t* tab = t.tab.data();
    const uint64_t mask = t.slots - 1, n2 = 2 * t.keys > 2 ? 2 * t.keys : 2;
    std::vector<KrankRec> rec((size_t)(2 * n2));
    std::vector<uint32_t> succ0((size_t)n2), node_of((size_t)t.slots), slot_of((size_t)(t.keys + 1)), ctl(KRANK_CTL, 0u), lens;
    std::vector<uint64_t> starts;
    const KrankView v{rec.data(), succ0.data(), node_of.data(), slot_of.data(), n2};
    auto find = [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); };
    auto solid_at = [&](uint64_t e) { return tab[e * SW + NW + 1] != KIDX_EMPTY && kcor_solid_word(tab[e * SW + NW], pr.min_cov); };
    auto append = [&starts](uint64_t start) { starts.push_back(start); };
    // number, sweep
    uint32_t solid = 0;
    for (uint64_t e = 0; e < t.slots; e++)
        if (solid_at(e)) {
            node_of[(size_t)e] = solid;
            slot_of[solid++] = (uint32_t)e;
        }
    for (uint64_t e = 0; e < t.slots; e++)
        if (solid_at(e) && krank_sweep<NW>(v, tab + e * SW, e, K, pr, find, append)) ctl[KRANK_GO] = 1;
    const uint64_t n = 2 * (uint64_t)solid;
    // round j, as krank_jump_kernel runs it
    auto round = [&](int j) {
        const uint32_t g = ctl[KRANK_GEN + j];
        if (!ctl[KRANK_GO + j]) { ctl[KRANK_GEN + j + 1] = g; return; }
        const KrankRec* src = v.rec + (uint64_t)g * n2;
        KrankRec* dst = v.rec + (uint64_t)(g ^ 1u) * n2;
        for (uint64_t x = 0; x < n; x++) {
            bool became;
            dst[x] = krank_jump(src[x], src, became);
            if (became) ctl[KRANK_GO + j + 1] = 1;
        }
        ctl[KRANK_GEN + j + 1] = g ^ 1u;
    };
    for (int j = 0; j < R; j++) round(j);
    // the rings: windows, the cut, the rounds again
    uint64_t cyclic = 0;
    {
        const uint32_t g = ctl[KRANK_GEN + R];
        KrankRec *fin = v.rec + (uint64_t)g * n2, *spare = v.rec + (uint64_t)(g ^ 1u) * n2;
        for (uint64_t x = 0; x < n; x++)
            if (!krank_done(fin[x])) {
                krank_min_store(spare + x, 0, KrankMin{succ0[(size_t)x], (uint32_t)x});
                ctl[KRANK_RING] = 1;
            }
        for (int r = 0; r < R && ctl[KRANK_RING]; r++)
            for (uint64_t x = 0; x < n; x++)
                if (!krank_done(fin[x]))
                    krank_min_store(spare + x, (r & 1) ^ 1, krank_min_jump<NW>(krank_min_load(spare + x, r & 1), spare, r & 1, tab, v));
        if (ctl[KRANK_RING]) {
            for (uint64_t x = 0; x < n; x++) {
                if (krank_done(fin[x])) continue;
                const uint32_t best = krank_min_load(spare + x, R & 1).best;
                fin[x] = krank_ring_cut((uint32_t)x, best, succ0[(size_t)x], [tab, &v](uint32_t y) { return kidx_coverage(krank_slot<NW>(tab, v, y)[NW]); });
                if (best == (uint32_t)x && krank_fwd(best)) {
                    starts.push_back(kunitig_start(slot_of[(size_t)(x >> 1)], true, KUNITIG_CYCLE));
                    cyclic++;
                }
            }
            ctl[KRANK_GO + R] = 1;
        }
    }
    for (int j = R; j < 2 * R; j++) round(j);
    const uint32_t g = ctl[KRANK_GEN + 2 * R];
    const KrankRec* fin = v.rec + (uint64_t)g * n2;
    KrankRec* place = v.rec + (uint64_t)(g ^ 1u) * n2;
    // measure, the scan and the decision
    KidxCounts total{{0, 0, 0, 0}};
    for (uint64_t s : starts) {
        lens.push_back(krank_measure<NW>(s, tab, v, fin, K));
        for (int i = 0; i < KIDX_COUNTS; i++) total.c[i] += kunitig_counts(lens.back(), K).c[i];
    }
    const uint64_t unitigs = total.c[0], words = total.c[1], kmers = total.c[2];
    const uint64_t tail = (uint64_t)ix->nw + 1;
    const bool overflow = packed_out && (unitigs > cap_unitigs || words + tail > cap_words);
    totals[KUNITIG_T_UNITIGS] = unitigs;
    totals[KUNITIG_T_WORDS] = words + tail;
    totals[KUNITIG_T_BASES] = kmers + unitigs * (uint64_t)(K - 1);
    totals[KUNITIG_T_COVERED] = kmers;
    totals[KUNITIG_T_SOLID] = solid;
    totals[KUNITIG_T_CYCLIC] = cyclic;
    totals[KUNITIG_T_CUT] = 0;
    totals[KUNITIG_T_OVERFLOW] = overflow ? 1 : 0;
    if (!packed_out || overflow) return;
    // zero, place, emit
    for (uint64_t q = 0; q < words + tail; q++) packed_out[q] = 0;
    uint64_t u = 0, at = 0, base = 0;
    for (size_t i = 0; i < starts.size(); i++) {
        krank_place<NW>(starts[i], lens[i], u, at, base, tab, v, fin, place, K, word_off_out, kmer_base_out, report);
        if (!lens[i]) continue;
        at += kunitig_row_words(lens[i], K);
        base += lens[i];
        u++;
    }
    if (word_off_out) word_off_out[u] = at;
    if (kmer_base_out) kmer_base_out[u] = base;
    for (uint32_t node = 0; node < solid; node++)
        krank_emit<NW>(node, tab, v, fin, place, K, [packed_out](uint64_t w, uint64_t bits) { packed_out[w] |= bits; });
}

}  // namespace
}  // namespace pg

extern "C" int pg_kindex_unitigs_ranked(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* packed_out,
                                        uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* out_report, uint64_t* out_totals, void* stream) {
    if (!ix) { pg_set_error("pg_kindex_unitigs_ranked: null index"); return PG_EINVAL; }
    if (ix->cut) {
        pg_set_error("pg_kindex_unitigs_ranked: the index is cut over ranks; a record's pointer names a node of one table: compact an index in one table");
        return PG_ESTATE;
    }
    if (!min_cov || min_cov > 255 || !min_arc || min_arc > 63) {
        pg_set_error("pg_kindex_unitigs_ranked: min_cov is 1 to 255 and min_arc 1 to 63");
        return PG_EINVAL;
    }
    if (!out_totals) { pg_set_error("pg_kindex_unitigs_ranked: out_totals is null"); return PG_EINVAL; }
    if (ix->ranks[0].keys > pg::KRANK_MAX_KEYS) {
        pg_set_error("pg_kindex_unitigs_ranked: an index of more than " + std::to_string(pg::KRANK_MAX_KEYS) + " keys: node ids and lengths are 32-bit");
        return PG_EINVAL;
    }
    const pg::KunitigParams pr{min_cov, min_arc, pg::KUNITIG_MAX_KMERS};
    if (ix->device >= 0)
        return pg::kunitig_device_unitigs_ranked(ix, pr, cap_unitigs, cap_words, packed_out, word_off_out, kmer_base_out, out_report, out_totals, stream);
    pg::kidx_with_nw(ix->nw, [&](auto nw) {
        pg::krank_host_unitigs<decltype(nw)::value>(ix, pr, cap_unitigs, cap_words, packed_out, word_off_out, kmer_base_out, out_report, out_totals);
    });
    return PG_OK;
}
