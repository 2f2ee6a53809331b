// kedit_host.cpp -- the C ABI of the first two operators that edit the graph of the k-mer index, pg_kindex_clip_tips and
// pg_kindex_pop_bubbles (include/soapdenovo2_amd.h section 3), through the round's host half (kedit_host.hpp: the host twin, the
// refusals, the dispatch).  A file of its own beside kindex_host.cpp, as kunitig_host.cpp is: a program that links the index's host half
// alone with stubs for its device engine keeps linking -- and the later operators (kedit_ops_host.cpp) have a file of theirs for the
// same reason: a program that links this file with stubs for these two operators' device rounds keeps linking too.
#include "kbubble.hpp"
#include "kedit_host.hpp"
#include "ktip.hpp"

extern "C" int pg_kindex_clip_tips(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint32_t max_tip, uint64_t* out_totals, void* stream) {
    const bool ok = min_cov && min_cov <= 255 && min_arc && min_arc <= 63 && max_tip && max_tip <= pg::KTIP_MAX_TIP;
    if (int rc = pg::kedit_refuse("pg_kindex_clip_tips", ix, "clip an index in one table",
                                  ok ? "" : "min_cov is 1 to 255, min_arc 1 to 63 and max_tip 1 to " + std::to_string(pg::KTIP_MAX_TIP), out_totals))
        return rc;
    return pg::kedit_round<pg::KtipOp>(ix, pg::KtipParams{min_cov, min_arc, max_tip}, out_totals, stream);
}

extern "C" int pg_kindex_pop_bubbles(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint32_t max_len, uint32_t max_diff, uint64_t* out_totals,
                                     void* stream) {
    const bool ok = min_cov && min_cov <= 255 && min_arc && min_arc <= 63 && max_len && max_len <= pg::KBUBBLE_MAX_LEN && max_diff <= pg::KBUBBLE_MAX_DIFF;
    if (int rc = pg::kedit_refuse("pg_kindex_pop_bubbles", ix, "pop the bubbles of an index in one table",
                                  ok ? "" : "min_cov is 1 to 255, min_arc 1 to 63, max_len 1 to " + std::to_string(pg::KBUBBLE_MAX_LEN) +
                                                " and max_diff 0 to " + std::to_string(pg::KBUBBLE_MAX_DIFF),
                                  out_totals))
        return rc;
    return pg::kedit_round<pg::KbubbleOp>(ix, pg::KbubbleParams{min_cov, min_arc, max_len, max_diff}, out_totals, stream);
}
