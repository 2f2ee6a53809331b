// kedit_ops_host.cpp -- the C ABI of the third and the fourth operator that edit the graph of the k-mer index, pg_kindex_drop_weak_arcs
// and pg_kindex_pop_bulges (include/soapdenovo2_amd.h section 3; karc.hpp, kbulge.hpp), through the round's host half
// (kedit_host.hpp).  Beside kedit_host.cpp and not in it: a program that links that file with stubs for the tips' and the bubbles'
// device rounds alone keeps linking.
#include "karc.hpp"
#include "kbulge.hpp"
#include "kedit_host.hpp"

extern "C" int pg_kindex_drop_weak_arcs(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint64_t* out_totals, void* stream) {
    const bool ok = min_cov && min_cov <= 255 && min_arc && min_arc <= 63;
    if (int rc = pg::kedit_refuse("pg_kindex_drop_weak_arcs", ix, "drop the arcs of an index in one table", ok ? "" : "min_cov is 1 to 255 and min_arc 1 to 63",
                                  out_totals))
        return rc;
    return pg::kedit_round<pg::KarcOp>(ix, pg::KarcParams{min_cov, min_arc}, out_totals, stream);
}

extern "C" int pg_kindex_pop_bulges(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint32_t max_len, uint32_t max_diff, uint64_t* out_totals,
                                    void* stream) {
    const bool ok = min_cov && min_cov <= 255 && min_arc && min_arc <= 63 && max_len && max_len <= pg::KBUBBLE_MAX_LEN && max_diff <= pg::KBUBBLE_MAX_DIFF;
    if (int rc = pg::kedit_refuse("pg_kindex_pop_bulges", ix, "pop the bulges of an index in one table",
                                  ok ? "" : "min_cov is 1 to 255, min_arc 1 to 63, max_len 1 to " + std::to_string(pg::KBUBBLE_MAX_LEN) +
                                                " and max_diff 0 to " + std::to_string(pg::KBUBBLE_MAX_DIFF),
                                  out_totals))
        return rc;
    return pg::kedit_round<pg::KbulgeOp>(ix, pg::KbubbleParams{min_cov, min_arc, max_len, max_diff}, out_totals, stream);
}
