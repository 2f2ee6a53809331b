// kwalk_host.cpp -- pg_kindex_walk's C ABI (include/soapdenovo2_amd.h section 3) and its host twin (a device = -1 index in one table):
// the rule of kwalk.hpp over host memory, a walk after the other, every lookup kidx_host_find.  What the CPU tests run, and the kernel's
// yardstick.  A file of its own beside kindex_host.cpp, as ktrim_host.cpp is: a program that links the index's host half alone with stubs
// for its device engine keeps linking.
#include <string>

#include "../../include/soapdenovo2_amd.h"
#include "kindex.hpp"
#include "kwalk.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
void kwalk_host_walk(const pg_kindex* ix, const KidxBatch& b, const KwalkParams& pr, uint64_t* out_ext, uint64_t* out_report) {
    const int K = ix->K;
    const uint64_t row_words = kwalk_row_words(pr.max_ext);
    auto find = [ix](const Kmer<NW>& ck, uint64_t&) { return kidx_host_find<NW>(ix, ck); };
    for (uint64_t r = 0; r < b.n_seqs; r++) {
        const KidxSeq q = kidx_seq(b, K, r);
        for (uint64_t v = 2 * r; v < 2 * r + 2; v++)
            kwalk_one<NW>(q.rd, q.nk, K, (v & 1) != 0, pr, find, out_ext ? out_ext + v * row_words : nullptr, out_report ? out_report + 2 * v : nullptr);
    }
}

}  // namespace
}  // namespace pg

extern "C" int pg_kindex_walk(pg_kindex* ix, const uint64_t* packed, uint64_t n_words, const uint64_t* word_off, const uint64_t* kmer_base,
                              uint64_t n_seqs, uint32_t uniform_len, uint32_t min_cov, uint32_t min_arc, uint32_t max_ext, uint64_t* out_ext,
                              uint64_t* out_report, void* stream) {
    if (!ix) { pg_set_error("pg_kindex_walk: null index"); return PG_EINVAL; }
    if (ix->cut) {
        pg_set_error("pg_kindex_walk: the index is cut over ranks; the kernel chases one lookup after the other in one table, each step's key "
                     "named by the answer before it: walk an index in one table");
        return PG_ESTATE;
    }
    if (!min_cov || min_cov > 255 || !min_arc || min_arc > 63 || !max_ext || max_ext > pg::KWALK_MAX_EXT) {
        pg_set_error("pg_kindex_walk: min_cov is 1 to 255, min_arc 1 to 63 and max_ext 1 to " + std::to_string(pg::KWALK_MAX_EXT));
        return PG_EINVAL;
    }
    if (!out_ext && !out_report) { pg_set_error("pg_kindex_walk: out_ext and out_report are both null"); return PG_EINVAL; }
    if (n_seqs > 1ull << 40) { pg_set_error("pg_kindex_walk: batch too large"); return PG_EINVAL; }
    const pg::KidxBatch b{packed, word_off, kmer_base, n_seqs, uniform_len, n_words, 0};
    // (an empty batch's words are not looked at)
    if (int rc = pg::kidx_batch_args("pg_kindex_walk", ix, b, "sequence", n_seqs ? pg::KIDX_ARGS_WORDS | pg::KIDX_ARGS_TAIL : 0u)) return rc;
    if (!n_seqs) return PG_OK;
    const pg::KwalkParams pr{min_cov, min_arc, max_ext};
    if (ix->device >= 0) return pg::kwalk_device_walk(ix, b, pr, out_ext, out_report, stream);
    pg::kidx_with_nw(ix->nw, [&](auto nw) { pg::kwalk_host_walk<decltype(nw)::value>(ix, b, pr, out_ext, out_report); });
    return PG_OK;
}
