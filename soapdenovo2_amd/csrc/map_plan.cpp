// map_plan.cpp -- pg_host_map_plan: the device memory the `map` stage takes on one rank, computed on the host from the sizing rules the
// engines allocate by (map_index.hpp: map_table_slots; map_kernels.hip: the buffers of a batch).  No GPU is touched.  call_map.cpp asks it,
// once the contigs are counted and before anything is allocated, whether the index fits the first device and, when it does not, over how
// many ranks it has to be cut (map_owner); BASELINE.json's human-scale configs have never met hardware, and this is where a user learns
// what they need.
//
// What is alive on a rank:
//   the table        map_table_slots(keys) slots of NW + 2 words.  One rank: every k-mer, in a block with DevBuf's quarter of headroom (the
//                    single-device engine).  Several ranks: an even share and a sixteenth on top -- a run counts its keys first
//                    (map_count_owned_kernel) and allocates exactly, so the slack only has to cover the hash's unevenness (a binomial
//                    share of 10^8 keys and more is even to a part in 10^4) and never costs memory
//   while it is built   the packed contigs (2 bits a base) and the build's work items, on every rank
//   a batch          the row buffer (8 B a k-mer), on the lead the staging buffer the other ranks' rows arrive in, the packed reads and
//                    the per-read arrays (sized for reads of two k-mers, the shortest that have any)
// The budget is the partition engine's (e2_plan.hpp): 0.85 of the device's free memory.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/soapdenovo2_amd.h"
#include "map_index.hpp"

void pg_set_error(const std::string& s);

namespace {

void plan_ranks(uint64_t n_ctg_kmers, int mer127, int n_ranks, uint64_t batch_kmers, uint64_t device_bytes, uint64_t out[12]) {
    memset(out, 0, 12 * sizeof(uint64_t));
    const uint64_t slot_bytes = (uint64_t)((mer127 ? 4 : 2) + 2) * 8;
    const uint64_t n = (uint64_t)n_ranks;
    const uint64_t share = (n_ctg_kmers + n - 1) / n;
    const uint64_t keys = n_ranks > 1 ? share + share / 16 + 1024 : n_ctg_kmers;
    const uint64_t slots = pg::map_table_slots(keys);
    const auto quarter = [](uint64_t b) { return b + b / 4; };                  // DevBuf::reserve
    const uint64_t table = n_ranks > 1 ? slots * slot_bytes : quarter(slots * slot_bytes);
    const uint64_t build = quarter(n_ctg_kmers / 4 + n_ctg_kmers / 8);          // packed bases; 8 B an item of 64 k-mers
    const uint64_t rows = quarter(std::max<uint64_t>(batch_kmers, 1) * 8);
    const uint64_t staging = n_ranks > 1 ? rows : 0;
    const uint64_t reads = quarter(batch_kmers / 2 + (batch_kmers / 2) * 32);  // 2 bits a base of reads half as long again as their k-mers; off, len, kmer_off, out
    const uint64_t peak = table + std::max(build, rows + staging + reads);
    const uint64_t budget = (uint64_t)((double)device_bytes * 0.85);
    out[0] = table; out[1] = slots; out[2] = keys; out[3] = rows; out[4] = staging; out[5] = reads; out[6] = build; out[7] = peak;
    out[8] = budget; out[9] = peak <= budget ? 1 : 0;
    out[10] = pg::map_table_slots(n_ctg_kmers) * slot_bytes;                    // the whole index as one table
}

}  // namespace

extern "C" int pg_host_map_plan(uint64_t n_ctg_kmers, int mer127, int n_ranks, uint64_t batch_kmers, uint64_t device_bytes, uint64_t out[12]) {
    if (!out || n_ranks < 1 || n_ranks > pg::DEVICE_LIST_MAX_RANKS || device_bytes == 0) { pg_set_error("pg_host_map_plan: bad argument"); return PG_EINVAL; }
    uint64_t probe[12];
    uint64_t fewest = 0;                                                        // the fewest ranks whose plan fits; 0: none up to DEVICE_LIST_MAX_RANKS
    for (int n = 1; n <= pg::DEVICE_LIST_MAX_RANKS && !fewest; n++) {
        plan_ranks(n_ctg_kmers, mer127, n, batch_kmers, device_bytes, probe);
        if (probe[9]) fewest = (uint64_t)n;
    }
    plan_ranks(n_ctg_kmers, mer127, n_ranks, batch_kmers, device_bytes, out);
    out[11] = fewest;
    return PG_OK;
}
