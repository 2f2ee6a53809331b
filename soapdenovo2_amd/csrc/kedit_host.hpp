// kedit_host.hpp -- what the C ABI entries of the operators that edit the graph of the k-mer index share on the host (kedit_host.cpp: the
// tips and the bubbles; kedit_ops_host.cpp: the arcs and the bulges; kisolated_host.cpp: the islands): the round's host twin (a
// device = -1 index in one table) -- the operator's rule (kedit.hpp) over host memory, the kernels' passes one after the other: ends,
// decide over every start, then apply: the snapshot rule, not a sequential sweep, every lookup kunitig_probe --, the refusals every
// entry makes, and the dispatch between the twin and the device engine.  What the CPU tests run, and the kernels' yardstick.
#pragma once
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "kedit.hpp"
#include "kunitig_host.hpp"

void pg_set_error(const std::string& s);

namespace pg {

template <int NW, class Op>
void kedit_host_round(pg_kindex* ix, const typename Op::Params& pr, uint64_t* totals) {
    constexpr int SW = map_slot_words<NW>();
    const int K = ix->K;
    uint64_t* tab = ix->ranks[0].tab.data();
    const KunitigHostTable<NW> t(ix);
    std::vector<uint64_t> starts;
    std::vector<uint32_t> lens;
    auto find = t.find();
    auto zero = [tab](uint64_t slot) { tab[slot * SW + NW] = 0; };
    auto clear = [tab](uint64_t slot, bool fwd, int a) {
        const uint64_t keep = (uint64_t)kedit_keep_mask(fwd, a);
        tab[slot * SW + NW] &= kedit_in_half(fwd) ? keep << 32 | 0xffffffffull : keep | 0xffffffffull << 32;
    };
    uint64_t removed = 0, kmers = 0, kept = 0;
    // 1. the ends, as the unitigs find them: every end side of a solid k-mer is a start
    const uint64_t solid = kunitig_host_ends<NW>(t, Op::ends(pr), starts);
    // 2. decide: every start over the table as it stands
    for (uint64_t s : starts) {
        const uint32_t left = kunitig_start_reason(s);
        KeditDecision d{0, false, false};
        if (Op::starts(left)) d = Op::template decide<NW>(t.node_of(s), left, K, pr, find);
        lens.push_back(d.minor ? d.n : 0);
        kept += d.candidate && !d.minor;
    }
    // 3. apply
    for (size_t i = 0; i < starts.size(); i++) {
        if (!lens[i]) continue;
        Op::template apply<NW>(t.node_of(starts[i]), lens[i], K, pr, find, zero, clear);
        removed++;
        kmers += lens[i];
    }
    totals[KEDIT_T_REMOVED] = removed;
    totals[KEDIT_T_KMERS] = kmers;
    totals[KEDIT_T_SOLID] = solid;
    totals[KEDIT_T_KEPT] = kept;
}

// The refusals every entry shares, in the order they are made: a null index, an index cut over ranks (cut_tail ends that message), the
// operator's own ranges (range: the message, or empty when they hold), null totals.  PG_OK: nothing to refuse
inline int kedit_refuse(const std::string& entry, const pg_kindex* ix, const char* cut_tail, const std::string& range, const uint64_t* out_totals) {
    if (!ix) { pg_set_error(entry + ": null index"); return PG_EINVAL; }
    if (ix->cut) {
        pg_set_error(entry + ": the index is cut over ranks; a walk chases one lookup after the other in one table, each step's key "
                             "named by the answer before it: " + cut_tail);
        return PG_ESTATE;
    }
    if (!range.empty()) { pg_set_error(entry + ": " + range); return PG_EINVAL; }
    if (!out_totals) { pg_set_error(entry + ": out_totals is null"); return PG_EINVAL; }
    return PG_OK;
}

template <class Op>
int kedit_round(pg_kindex* ix, const typename Op::Params& pr, uint64_t* out_totals, void* stream) {
    if (ix->device >= 0) return kedit_device_round<Op>(ix, pr, out_totals, stream);
    kidx_with_nw(ix->nw, [&](auto nw) { kedit_host_round<decltype(nw)::value, Op>(ix, pr, out_totals); });
    return PG_OK;
}

}  // namespace pg
