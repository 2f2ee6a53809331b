// kisolated_host.cpp -- the C ABI of the fifth operator that edits the graph of the k-mer index, pg_kindex_drop_isolated
// (include/soapdenovo2_amd.h section 3; kisolated.hpp), through the round's host half (kedit_host.hpp).  Beside
// kedit_host.cpp and kedit_ops_host.cpp and in neither: a program that links one of those files with stubs for its own operators' device
// rounds alone keeps linking.
#include "kedit_host.hpp"
#include "kisolated.hpp"

extern "C" int pg_kindex_drop_isolated(pg_kindex* ix, uint32_t min_cov, uint32_t min_arc, uint32_t max_len, uint32_t max_cov, uint64_t* out_totals,
                                       void* stream) {
    const bool ok = min_cov && min_cov <= 255 && min_arc && min_arc <= 63 && max_len && max_len <= pg::KISOLATED_MAX_LEN && max_cov && max_cov <= 255;
    if (int rc = pg::kedit_refuse("pg_kindex_drop_isolated", ix, "drop the isolated unitigs of an index in one table",
                                  ok ? "" : "min_cov is 1 to 255, min_arc 1 to 63, max_len 1 to " + std::to_string(pg::KISOLATED_MAX_LEN) +
                                                " and max_cov 1 to 255",
                                  out_totals))
        return rc;
    return pg::kedit_round<pg::KisolatedOp>(ix, pg::KisolatedParams{min_cov, min_arc, max_len, max_cov}, out_totals, stream);
}
