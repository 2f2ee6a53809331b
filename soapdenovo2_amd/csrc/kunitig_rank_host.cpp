// kunitig_rank_host.cpp -- pg_kindex_unitigs_ranked's C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index in
// one table): the bodies of krank.hpp over host memory, the kernels' passes one after the other -- number, sweep, the rounds with their
// control words, the rings, measure, scan, place, emit -- so that the CPU tests run the rounds the kernels run and not another
// algorithm.  A file of its own, as kunitig_host.cpp is: a program that links the index's host half and the walking engine's alone with
// stubs for their device engines keeps linking.
#include <string>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "krank.hpp"
#include "kunitig_host.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
void krank_host_unitigs(const pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* packed_out,
                        uint64_t* word_off_out, uint64_t* kmer_base_out, uint64_t* report, uint64_t* totals) {
    const KunitigHostTable<NW> t(ix);
    const uint64_t* tab = t.tab;
    const uint64_t keys = ix->ranks[0].keys, n2 = kunitig_plan(keys, t.slots, KUNITIG_KIND_RANK).cap;
    const int K = ix->K, tail = ix->nw + 1, R = krank_rounds(keys);
    std::vector<KrankRec> rec((size_t)(2 * n2));
    std::vector<uint32_t> succ0((size_t)n2), node_of((size_t)t.slots), slot_of((size_t)(keys + 1)), ctl_words(KRANK_CTL, 0u), lens;
    std::vector<uint64_t> starts;
    uint32_t* ctl = ctl_words.data();
    const KrankView v{rec.data(), succ0.data(), node_of.data(), slot_of.data(), n2};
    auto append = [&starts](uint64_t start) { starts.push_back(start); };
    // number, sweep
    uint32_t solid = 0;
    for (uint64_t e = 0; e < t.slots; e++)
        if (t.solid_at(e, pr.min_cov)) {
            node_of[(size_t)e] = solid;
            slot_of[solid++] = (uint32_t)e;
        }
    for (uint64_t e = 0; e < t.slots; e++)
        if (t.solid_at(e, pr.min_cov)) krank_sweep_done(ctl, krank_sweep<NW>(v, t.slot(e), e, K, pr, t.find(), append));
    const uint64_t n = 2 * (uint64_t)solid;
    // round j, as krank_jump_kernel runs it
    auto round = [&](int j) {
        const KrankPass p = krank_jump_pass(ctl, j);
        bool any = false;
        for (uint64_t x = 0; p.go && x < n; x++) krank_jump_item(krank_cur(v, p), krank_other(v, p), x, any);
        krank_jump_done(p, ctl, j, any, true);
    };
    for (int j = 0; j < R; j++) round(j);
    // the rings: windows, the cut, the rounds again
    uint64_t cyclic = 0;
    {
        const KrankPass p = krank_ring_init_pass(ctl, R);
        bool any = false;
        for (uint64_t x = 0; x < n; x++) krank_ring_init_item(krank_cur(v, p), krank_other(v, p), v, x, any);
        krank_ring_init_done(ctl, any);
    }
    for (int r = 0; r < R; r++) {
        const KrankPass p = krank_ring_pass(ctl, R);
        for (uint64_t x = 0; p.go && x < n; x++) krank_min_item<NW>(krank_cur(v, p), krank_other(v, p), v, tab, r, x);
    }
    if (const KrankPass p = krank_ring_pass(ctl, R); p.go) {
        for (uint64_t x = 0; x < n; x++) krank_ring_cut_item<NW>(krank_cur(v, p), krank_other(v, p), v, tab, R, x, append, [&cyclic] { cyclic++; });
        krank_ring_cut_done(ctl, R, true);
    }
    for (int j = R; j < 2 * R; j++) round(j);
    const KrankPass f = krank_final_pass(ctl, R);
    const KrankRec* fin = krank_cur(v, f);
    KrankRec* place = krank_other(v, f);
    // measure, the scan and the decision
    for (uint64_t s : starts) lens.push_back(krank_measure<NW>(s, tab, v, fin, K));
    const KidxCounts all = kunitig_host_sums(lens, K);
    if (!kunitig_finish(all, K, tail, solid, cyclic, 0, cap_unitigs, cap_words, packed_out != nullptr, totals)) return;
    // zero, place, emit
    for (uint64_t q = 0; q < all.c[1]; q++) packed_out[q] = 0;
    kunitig_host_scan(lens, K, tail, packed_out, word_off_out, kmer_base_out, [&](size_t i, uint64_t u, uint64_t at, uint64_t base) {
        krank_place<NW>(starts[i], lens[i], u, at, base, tab, v, fin, place, K, word_off_out, kmer_base_out, report);
    });
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
