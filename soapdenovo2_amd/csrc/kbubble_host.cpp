// kbubble_host.cpp -- pg_kindex_pop_bubbles' C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index in one
// table): the rule of kbubble.hpp over host memory, the kernels' passes one after the other -- ends, decide over every start, then apply:
// the snapshot rule, not a sequential sweep --, every lookup kunitig_probe.  What the CPU tests run, and the kernels' yardstick.  A file of
// its own beside kindex_host.cpp, as ktip_host.cpp is: a program that links the index's host half alone with stubs for its device
// engine keeps linking.
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "kindex.hpp"
#include "kbubble.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
void kbubble_host_pop(pg_kindex* ix, const KbubbleParams& pr, uint64_t* totals) {
    constexpr int SW = map_slot_words<NW>();
    const int K = ix->K;
    KidxRank& t = ix->ranks[0];
    uint64_t* tab = t.tab.data();
    const uint64_t mask = t.slots - 1;
    const KunitigParams up{pr.min_cov, pr.min_arc, pr.max_len};
    std::vector<uint64_t> starts;
    std::vector<uint32_t> lens;
    auto find = [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); };
    auto node_of = [&](uint64_t start) {
        const uint64_t* sl = tab + kunitig_start_slot(start) * SW;
        return kunitig_node<NW>(kidx_record_key<NW>(sl), sl[NW], kunitig_start_slot(start), kunitig_start_fwd(start), K);
    };
    uint64_t solid = 0, branches = 0, kmers = 0, kept = 0;
    // 1. the ends, as the unitigs find them: every end side of a solid k-mer is a start
    for (uint64_t e = 0; e < t.slots; e++) {
        if (tab[e * SW + NW + 1] == KIDX_EMPTY || !kcor_solid_word(tab[e * SW + NW], pr.min_cov)) continue;
        solid++;
        uint32_t reasons[2];
        const uint32_t ends = kunitig_ends<NW>(kidx_record_key<NW>(tab + e * SW), tab[e * SW + NW], e, K, up, find, reasons);
        for (int side = 0; side < 2; side++)
            if (ends >> side & 1) starts.push_back(kunitig_start(e, side == 0, reasons[side]));
    }
    // 2. decide: every start over the table as it stands
    for (uint64_t s : starts) {
        KbubbleDecision d{0, false, false};
        if (kunitig_start_reason(s) == KWALK_BRANCH_IN) d = kbubble_decide<NW>(node_of(s), KWALK_BRANCH_IN, K, pr, find);
        lens.push_back(d.minor ? d.n : 0);
        kept += d.candidate && !d.minor;
    }
    // 3. apply
    for (size_t i = 0; i < starts.size(); i++) {
        if (!lens[i]) continue;
        kbubble_apply<NW>(node_of(starts[i]), lens[i], K, pr, find, [tab](uint64_t slot) { tab[slot * SW + NW] = 0; },
                          [tab](uint64_t slot, bool fwd, int a) {
                              const uint64_t keep = (uint64_t)ktip_keep_mask(fwd, a);
                              tab[slot * SW + NW] &= ktip_in_half(fwd) ? keep << 32 | 0xffffffffull : keep | 0xffffffffull << 32;
                          });
        branches++;
        kmers += lens[i];
    }
    totals[KBUBBLE_T_BRANCHES] = branches;
    totals[KBUBBLE_T_KMERS] = kmers;
    totals[KBUBBLE_T_SOLID] = solid;
    totals[KBUBBLE_T_KEPT] = kept;
}

}  // namespace
}  // namespace pg

extern "C" int pg_kindex_pop_bubbles(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint32_t max_len, uint32_t max_diff, uint64_t* out_totals,
                                     void* stream) {
    if (!ix) { pg_set_error("pg_kindex_pop_bubbles: null index"); return PG_EINVAL; }
    if (ix->cut) {
        pg_set_error("pg_kindex_pop_bubbles: the index is cut over ranks; a walk chases one lookup after the other in one table, each step's key "
                     "named by the answer before it: pop the bubbles of an index in one table");
        return PG_ESTATE;
    }
    if (!min_cov || min_cov > 255 || !min_arc || min_arc > 63 || !max_len || max_len > pg::KBUBBLE_MAX_LEN || max_diff > pg::KBUBBLE_MAX_DIFF) {
        pg_set_error("pg_kindex_pop_bubbles: min_cov is 1 to 255, min_arc 1 to 63, max_len 1 to " + std::to_string(pg::KBUBBLE_MAX_LEN) +
                     " and max_diff 0 to " + std::to_string(pg::KBUBBLE_MAX_DIFF));
        return PG_EINVAL;
    }
    if (!out_totals) { pg_set_error("pg_kindex_pop_bubbles: out_totals is null"); return PG_EINVAL; }
    const pg::KbubbleParams pr{min_cov, min_arc, max_len, max_diff};
    if (ix->device >= 0) return pg::kbubble_device_pop(ix, pr, out_totals, stream);
    pg::kidx_with_nw(ix->nw, [&](auto nw) { pg::kbubble_host_pop<decltype(nw)::value>(ix, pr, out_totals); });
    return PG_OK;
}
