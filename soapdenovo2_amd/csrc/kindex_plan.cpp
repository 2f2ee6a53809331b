// kindex_plan.cpp -- pg_host_kindex_plan: the device memory a rank of the k-mer index takes when the index is cut over n_ranks
// (kindex.hpp; 1: one table), computed on the host from the rules the engine allocates by.  No GPU is touched.  It is modelled on
// pg_host_map_plan (map_plan.cpp), and pg_kindex_build_sharded asks it for the fewest ranks when a build does not fit.
//
// What is alive on a rank:
//   the table        map_table_slots(keys) slots of NW + 2 words, cut exactly (no headroom).  One rank: every record.  Several ranks:
//                    map_plan.cpp's even share and a sixteenth on top, plus 1024 -- a run counts the owners first
//                    (kidx_count_owners_kernel) and allocates exactly, so the slack only has to cover the hash's unevenness and never
//                    costs memory
//   while it is built   the chunk buffer a part off the rank's device passes through: KIDX_CHUNK_RECORDS records at most.  It is counted
//                    for one rank too (records that come from host memory); a device array indexed where it lies needs none
//   a batch          the rank's rows (8 B a k-mer), on the lead the staging buffer the other ranks' rows arrive in, on a rank off the
//                    lead's device its copy of the batch (the packed words, and for a ragged batch two offsets a sequence: bounded here
//                    by a sequence a word).  The peak is that of the rank that takes most
// The budget is the partition engine's (e2_plan.hpp): 0.85 of the device's free memory.  The records themselves are the caller's, and
// where they lie on the same device they are not in device_bytes.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/soapdenovo2_amd.h"
#include "kindex.hpp"

void pg_set_error(const std::string& s);

namespace {

void plan_ranks(uint64_t n_records, int mer127, int n_ranks, uint64_t batch_kmers, uint64_t batch_words, uint64_t device_bytes, uint64_t out[12]) {
    memset(out, 0, 12 * sizeof(uint64_t));
    const uint64_t slot_bytes = (uint64_t)((mer127 ? 4 : 2) + 2) * 8;           // a slot and a record are as many words
    const uint64_t n = (uint64_t)n_ranks;
    const uint64_t share = (n_records + n - 1) / n;
    const uint64_t keys = n_ranks > 1 ? share + share / 16 + 1024 : n_records;
    const uint64_t slots = pg::map_table_slots(keys);
    const uint64_t table = slots * slot_bytes;
    const uint64_t chunk = std::min<uint64_t>(pg::KIDX_CHUNK_RECORDS, n_records) * slot_bytes;
    const uint64_t rows = batch_kmers * 8;
    const uint64_t staging = n_ranks > 1 ? rows : 0;
    const uint64_t batch = n_ranks > 1 ? 3 * batch_words * 8 : 0;
    const uint64_t peak = table + std::max(chunk, rows + std::max(staging, batch));
    const uint64_t budget = (uint64_t)((double)device_bytes * 0.85);
    out[0] = table; out[1] = slots; out[2] = keys; out[3] = chunk; out[4] = rows; out[5] = staging; out[6] = batch; out[7] = peak;
    out[8] = budget; out[9] = peak <= budget ? 1 : 0;
    out[10] = pg::map_table_slots(n_records) * slot_bytes;                      // the whole index as one table
}

}  // namespace

extern "C" int pg_host_kindex_plan(uint64_t n_records, int mer127, int n_ranks, uint64_t batch_kmers, uint64_t batch_words, uint64_t device_bytes,
                                   uint64_t out[12]) {
    if (!out || n_ranks < 1 || n_ranks > pg::DEVICE_LIST_MAX_RANKS || device_bytes == 0) { pg_set_error("pg_host_kindex_plan: bad argument"); return PG_EINVAL; }
    uint64_t probe[12];
    uint64_t fewest = 0;                                                        // the fewest ranks whose plan fits; 0: none up to DEVICE_LIST_MAX_RANKS
    for (int n = 1; n <= pg::DEVICE_LIST_MAX_RANKS && !fewest; n++) {
        plan_ranks(n_records, mer127, n, batch_kmers, batch_words, device_bytes, probe);
        if (probe[9]) fewest = (uint64_t)n;
    }
    plan_ranks(n_records, mer127, n_ranks, batch_kmers, batch_words, device_bytes, out);
    out[11] = fewest;
    return PG_OK;
}
