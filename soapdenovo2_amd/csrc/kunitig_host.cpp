// kunitig_host.cpp -- pg_kindex_unitigs' C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index in one table):
// the rule of kunitig.hpp over host memory, the kernels' passes one after the other -- ends, measure, rings, scan, write -- every lookup
// kunitig_probe.  What the CPU tests run, and the kernels' yardstick.  A file of its own beside kindex_host.cpp, as kwalk_host.cpp is: a
// program that links the index's host half alone with stubs for its device engine keeps linking.
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "kindex.hpp"
#include "kunitig.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
void kunitig_host_unitigs(const pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* packed_out,
                          uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* report, uint64_t* totals) {
    constexpr int SW = map_slot_words<NW>();
    const int K = ix->K;
    const KidxRank& t = ix->ranks[0];
    const uint64_t* tab = t.tab.data();
    const uint64_t mask = t.slots - 1;
    std::vector<uint32_t> bits((size_t)((t.slots + 31) / 32), 0);               // a covered bit a slot
    std::vector<uint64_t> starts;
    std::vector<uint32_t> lens;
    auto find = [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); };
    auto mark = [&bits](uint64_t slot) { bits[(size_t)(slot >> 5)] |= 1u << (slot & 31); };
    auto covered = [&bits](uint64_t slot) { return (bits[(size_t)(slot >> 5)] >> (slot & 31) & 1u) != 0; };
    auto nothing = [](uint64_t) {};
    auto solid_at = [&](uint64_t e) { return tab[e * SW + NW + 1] != KIDX_EMPTY && kcor_solid_word(tab[e * SW + NW], pr.min_cov); };
    auto node_of = [&](uint64_t start) {
        const uint64_t* sl = tab + kunitig_start_slot(start) * SW;
        return kunitig_node<NW>(kidx_record_key<NW>(sl), sl[NW], kunitig_start_slot(start), kunitig_start_fwd(start), K);
    };
    uint64_t solid = 0, cyclic = 0, cut = 0;
    // 1. the ends: every end side of a solid k-mer starts a walk
    for (uint64_t e = 0; e < t.slots; e++) {
        if (!solid_at(e)) continue;
        solid++;
        uint32_t reasons[2];
        const uint32_t ends = kunitig_ends<NW>(kidx_record_key<NW>(tab + e * SW), tab[e * SW + NW], e, K, pr, find, reasons);
        for (int side = 0; side < 2; side++)
            if (ends >> side & 1) starts.push_back(kunitig_start(e, side == 0, reasons[side]));
    }
    // 2. measure: every chain from both of its ends, the losing copy's length 0
    for (uint64_t s : starts) {
        const KunitigWalk w = kunitig_chain<NW>(node_of(s), false, K, pr, find, mark, covered, nullptr);
        lens.push_back(w.n);
        cut += w.n && w.reason == KUNITIG_CUT;
    }
    // 3. the rings: a solid k-mer no chain covered asks whether it is the least member of one
    for (uint64_t e = 0; e < t.slots; e++) {
        if (!solid_at(e) || covered(e)) continue;
        const uint64_t s = kunitig_start(e, true, KUNITIG_CYCLE);
        const KunitigWalk w = kunitig_chain<NW>(node_of(s), true, K, pr, find, nothing, covered, nullptr);
        if (!w.n) continue;
        starts.push_back(s);
        lens.push_back(w.n);
        cyclic++;
    }
    // 4. the scan and the decision
    KidxCounts total{{0, 0, 0, 0}};
    for (uint32_t n : lens)
        for (int i = 0; i < KIDX_COUNTS; i++) total.c[i] += kunitig_counts(n, K).c[i];
    const uint64_t unitigs = total.c[0], words = total.c[1], kmers = total.c[2];
    const uint64_t tail = (uint64_t)ix->nw + 1;
    const bool overflow = packed_out && (unitigs > cap_unitigs || words + tail > cap_words);
    totals[KUNITIG_T_UNITIGS] = unitigs;
    totals[KUNITIG_T_WORDS] = words + tail;
    totals[KUNITIG_T_BASES] = kmers + unitigs * (uint64_t)(K - 1);
    totals[KUNITIG_T_COVERED] = kmers;
    totals[KUNITIG_T_SOLID] = solid;
    totals[KUNITIG_T_CYCLIC] = cyclic;
    totals[KUNITIG_T_CUT] = cut;
    totals[KUNITIG_T_OVERFLOW] = overflow ? 1 : 0;
    if (!packed_out || overflow) return;
    // 5. write: the kept starts' rows one behind the other
    uint64_t u = 0, at = 0, base = 0;
    for (size_t i = 0; i < starts.size(); i++) {
        if (!lens[i]) continue;
        const uint32_t left = kunitig_start_reason(starts[i]);
        const KunitigWalk w = kunitig_chain<NW>(node_of(starts[i]), left == KUNITIG_CYCLE, K, pr, find, nothing, covered, packed_out + at);
        if (word_off_out) word_off_out[u] = at;
        if (kmer_base_out) kmer_base_out[u] = base;
        if (report) {
            report[2 * u] = kunitig_report_word((uint64_t)w.n + (uint64_t)K - 1, left, w.reason);
            report[2 * u + 1] = w.cov;
        }
        at += kunitig_row_words(lens[i], K);
        base += lens[i];
        u++;
    }
    if (word_off_out) word_off_out[u] = at;
    if (kmer_base_out) kmer_base_out[u] = base;
    for (uint64_t q = 0; q < tail; q++) packed_out[at + q] = 0;
}

}  // namespace
}  // namespace pg

extern "C" int pg_kindex_unitigs(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint32_t max_kmers, uint64_t cap_unitigs, uint64_t cap_words,
                                 uint64_t* packed_out, uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* out_report, uint64_t* out_totals,
                                 void* stream) {
    if (!ix) { pg_set_error("pg_kindex_unitigs: null index"); return PG_EINVAL; }
    if (ix->cut) {
        pg_set_error("pg_kindex_unitigs: the index is cut over ranks; a walk chases one lookup after the other in one table, each step's key "
                     "named by the answer before it: compact an index in one table");
        return PG_ESTATE;
    }
    if (!min_cov || min_cov > 255 || !min_arc || min_arc > 63 || !max_kmers || max_kmers > pg::KUNITIG_MAX_KMERS) {
        pg_set_error("pg_kindex_unitigs: min_cov is 1 to 255, min_arc 1 to 63 and max_kmers 1 to " + std::to_string(pg::KUNITIG_MAX_KMERS));
        return PG_EINVAL;
    }
    if (!out_totals) { pg_set_error("pg_kindex_unitigs: out_totals is null"); return PG_EINVAL; }
    const pg::KunitigParams pr{min_cov, min_arc, max_kmers};
    if (ix->device >= 0)
        return pg::kunitig_device_unitigs(ix, pr, cap_unitigs, cap_words, packed_out, word_off_out, kmer_base_out, out_report, out_totals, stream);
    pg::kidx_with_nw(ix->nw, [&](auto nw) {
        pg::kunitig_host_unitigs<decltype(nw)::value>(ix, pr, cap_unitigs, cap_words, packed_out, word_off_out, kmer_base_out, out_report, out_totals);
    });
    return PG_OK;
}
