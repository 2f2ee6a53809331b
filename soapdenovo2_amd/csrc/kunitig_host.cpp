// kunitig_host.cpp -- pg_kindex_unitigs' C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index in one table):
// the rule of kunitig.hpp over host memory, the kernels' passes one after the other -- ends, measure, rings, scan, write -- every lookup
// kunitig_probe; the table, the ends sweep and the scan are kunitig_host.hpp's, the finish kunitig.hpp's.  What the CPU tests run, and the kernels' yardstick.  A file of its own beside kindex_host.cpp, as kwalk_host.cpp is: a
// program that links the index's host half alone with stubs for its device engine keeps linking.
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "kunitig_host.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
void kunitig_host_unitigs(const pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* packed_out,
                          uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* report, uint64_t* totals) {
    const int K = ix->K, tail = ix->nw + 1;
    const KunitigHostTable<NW> t(ix);
    std::vector<uint32_t> bits((size_t)((t.slots + 31) / 32), 0);               // a covered bit a slot
    std::vector<uint64_t> starts;
    std::vector<uint32_t> lens;
    auto find = t.find();
    auto mark = [&bits](uint64_t slot) { bits[(size_t)(slot >> 5)] |= 1u << (slot & 31); };
    auto covered = [&bits](uint64_t slot) { return (bits[(size_t)(slot >> 5)] >> (slot & 31) & 1u) != 0; };
    auto nothing = [](uint64_t) {};
    uint64_t cyclic = 0, cut = 0;
    // 1. the ends: every end side of a solid k-mer starts a walk
    const uint64_t solid = kunitig_host_ends<NW>(t, pr, starts);
    // 2. measure: every chain from both of its ends, the losing copy's length 0
    for (uint64_t s : starts) {
        const KunitigWalk w = kunitig_chain<NW>(t.node_of(s), false, K, pr, find, mark, covered, nullptr);
        lens.push_back(w.n);
        cut += w.n && w.reason == KUNITIG_CUT;
    }
    // 3. the rings: a solid k-mer no chain covered asks whether it is the least member of one
    for (uint64_t e = 0; e < t.slots; e++) {
        if (!t.solid_at(e, pr.min_cov) || covered(e)) continue;
        const uint64_t s = kunitig_start(e, true, KUNITIG_CYCLE);
        const KunitigWalk w = kunitig_chain<NW>(t.node_of(s), true, K, pr, find, nothing, covered, nullptr);
        if (!w.n) continue;
        starts.push_back(s);
        lens.push_back(w.n);
        cyclic++;
    }
    // 4. the scan and the decision
    if (!kunitig_finish(kunitig_host_sums(lens, K), K, tail, solid, cyclic, cut, cap_unitigs, cap_words, packed_out != nullptr, totals)) return;
    // 5. write: the kept starts' rows one behind the other
    kunitig_host_scan(lens, K, tail, packed_out, word_off_out, kmer_base_out, [&](size_t i, uint64_t u, uint64_t at, uint64_t base) {
        if (!lens[i]) return;
        const uint32_t left = kunitig_start_reason(starts[i]);
        const KunitigWalk w = kunitig_chain<NW>(t.node_of(starts[i]), left == KUNITIG_CYCLE, K, pr, find, nothing, covered, packed_out + at);
        if (word_off_out) word_off_out[u] = at;
        if (kmer_base_out) kmer_base_out[u] = base;
        if (report) {
            report[2 * u] = kunitig_report_word((uint64_t)w.n + (uint64_t)K - 1, left, w.reason);
            report[2 * u + 1] = w.cov;
        }
    });
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
