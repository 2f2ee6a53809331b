// kindex_host.cpp -- the k-mer index's C ABI (pg_kindex_*, include/soapdenovo2_amd.h section 3) and its host twin (device = -1): the same
// tables built by a serial insert, the same lookups and summary (kindex.hpp: kidx_host_find, KidxSummary) over host memory.  What the CPU
// tests run, and the device path's yardstick.  The index cut over ranks (pg_kindex_build_sharded with a device list of -1s) is n such
// tables with the device's cut: a k-mer is looked up in the table of map_owner(key, n); pg_kindex_build's one table is the case n = 1.
#include <stdlib.h>
#include <string.h>
#include <string>

#include "../../include/soapdenovo2_amd.h"
#include "env.hpp"
#include "kcorrect.hpp"
#include "kindex.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

const char* kidx_code_name(int rc) {
    switch (rc) {
        case PG_EINVAL: return "PG_EINVAL";
        case PG_ENODEV: return "PG_ENODEV";
        case PG_ENOMEM: return "PG_ENOMEM";
        case PG_ESTATE: return "PG_ESTATE";
        case PG_ESPIN: return "PG_ESPIN";
    }
    return "PG_E?";
}

// a build that returns null says which code it failed with at the end of pg_last_error's message
pg_kindex* kidx_build_failed(pg_kindex* ix, int rc) {
    if (ix) {
        if (ix->device >= 0) kidx_device_free(ix);
        delete ix;
    }
    pg_set_error(std::string(pg_last_error()) + " (" + kidx_code_name(rc) + ")");
    return nullptr;
}

// the serial insert of a stored record; false: its key is in the table already
template <int NW>
bool kidx_host_put(uint64_t* tab, uint64_t mask, const uint64_t* rec) {
    constexpr int SW = map_slot_words<NW>();
    const Kmer<NW> k = kidx_record_key<NW>(rec);
    for (uint64_t e = map_home<NW>(k, mask);; e = (e + 1) & mask) {
        uint64_t* sl = tab + e * SW;
        if (sl[NW + 1] == KIDX_EMPTY) {
            for (int q = 0; q < NW; q++) sl[q] = k.w[q];
            sl[NW] = rec[NW];
            sl[NW + 1] = KIDX_FULL;
            return true;
        }
        bool eq = true;
        for (int q = 0; q < NW; q++) eq = eq && sl[q] == k.w[q];
        if (eq) return false;
    }
}

// the ranks' serial tables (pg_kindex_build: one rank, one part): the owners counted first, every rank's table made for exactly the
// records it owns, then the inserts
template <int NW>
int kidx_host_build(pg_kindex* ix, const uint64_t* const* parts, const uint64_t* part_records, int n_parts) {
    const uint32_t n = (uint32_t)ix->ranks.size();
    for (int p = 0; p < n_parts; p++)
        for (uint64_t i = 0; i < part_records[p]; i++) ix->ranks[map_owner<NW>(kidx_record_key<NW>(parts[p] + i * (NW + 2)), n)].keys++;
    for (KidxRank& r : ix->ranks) {
        r.slots = map_table_slots(r.keys);
        r.tab.assign(r.slots * map_slot_words<NW>(), 0);
    }
    for (int p = 0; p < n_parts; p++)
        for (uint64_t i = 0; i < part_records[p]; i++) {
            const uint64_t* rec = parts[p] + i * (NW + 2);
            if (!kidx_stored(rec[NW])) continue;
            KidxRank& r = ix->ranks[map_owner<NW>(kidx_record_key<NW>(rec), n)];
            if (!kidx_host_put<NW>(r.tab.data(), r.slots - 1, rec)) { pg_set_error("k-mer index: duplicate key in records"); return PG_EINVAL; }
        }
    return PG_OK;
}

// the query kernel's walk over the ranks' tables: every k-mer asks its owner's
template <int NW>
void kidx_host_query(const pg_kindex* ix, const KidxBatch& b, uint64_t* out, uint64_t* summary) {
    for (uint64_t r = 0; r < b.n_seqs; r++) {
        const KidxSeq q = kidx_seq(b, ix->K, r);
        KidxSummary s = kidx_summary_none();
        map_roll<NW>(q.rd, 0, q.nk, ix->K, [&](const Kmer<NW>& ck, bool, int j) {
            const uint64_t cnt = kidx_host_find<NW>(ix, ck);
            if (out) out[q.base + j] = cnt;
            kidx_summary_add(s, cnt, j);
        });
        if (summary) kidx_summary_store(s, q.nk, summary + r * KIDX_SUMMARY_WORDS);
    }
}

// the host twin of kcor_kernel (an index in one table): the copy first, then kcor_read on every read's own words of the output
template <int NW>
void kcor_host_correct(const pg_kindex* ix, KidxBatch b, const KcorParams& pr, uint64_t* packed_out, uint64_t* report) {
    const KidxRank& t = ix->ranks[0];
    if (packed_out != b.packed) memmove(packed_out, b.packed, b.n_words * sizeof(uint64_t));
    b.packed = packed_out;
    for (uint64_t r = 0; r < b.n_seqs; r++) {
        const KidxSeq q = kidx_seq(b, ix->K, r);
        const uint64_t rep = kcor_read<NW>(packed_out + (q.rd - packed_out), q.nk, ix->K, t.tab.data(), t.slots - 1, pr);
        if (report) report[r] = rep;
    }
}

// a new index of n ranks; rank i's device is devices[i]
pg_kindex* kidx_new(const int* devices, int n, int K, int mer127, bool cut) {
    pg_kindex* ix = new pg_kindex();
    ix->device = devices[0];
    ix->K = K;
    ix->nw = mer127 ? 4 : 2;
    ix->cut = cut;
    ix->ranks.resize((size_t)n);
    for (int i = 0; i < n; i++) ix->ranks[(size_t)i].device = devices[i];
    return ix;
}

}  // namespace

uint64_t kidx_chunk_records() {
    if (const char* e = env_test("SOAPDENOVO2_AMD_KINDEX_CHUNK_RECORDS")) { const long long v = atoll(e); if (v > 0) return (uint64_t)v; }
    return KIDX_CHUNK_RECORDS;
}

}  // namespace pg

extern "C" pg_kindex* pg_kindex_build(int device, int K, int mer127, const uint64_t* records, uint64_t n_records, void* stream) {
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || (K & 1) == 0) {
        pg_set_error("pg_kindex_build: K must be odd and within 13.." + std::to_string(maxK));
        return pg::kidx_build_failed(nullptr, PG_EINVAL);
    }
    if (device < -1 || (!records && n_records)) { pg_set_error("pg_kindex_build: bad device or null records"); return pg::kidx_build_failed(nullptr, PG_EINVAL); }
    pg_kindex* ix = pg::kidx_new(&device, 1, K, mer127, false);
    int rc = PG_OK;
    if (device >= 0) rc = pg::kidx_device_build(ix, records, n_records, stream);
    else pg::kidx_with_nw(ix->nw, [&](auto nw) { rc = pg::kidx_host_build<decltype(nw)::value>(ix, &records, &n_records, 1); });
    return rc == PG_OK ? ix : pg::kidx_build_failed(ix, rc);
}

extern "C" pg_kindex* pg_kindex_build_sharded(const int* devices, int n_devices, int K, int mer127, const uint64_t* const* parts,
                                              const uint64_t* part_records, const int* part_device, int n_parts, void* stream) {
    const auto bad = [](const std::string& why) { pg_set_error("pg_kindex_build_sharded: " + why); return pg::kidx_build_failed(nullptr, PG_EINVAL); };
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || (K & 1) == 0) return bad("K must be odd and within 13.." + std::to_string(maxK));
    if (!devices || n_devices < 1 || n_devices > pg::DEVICE_LIST_MAX_RANKS) return bad("an index is cut over 1 to " + std::to_string(pg::DEVICE_LIST_MAX_RANKS) + " ranks");
    if (n_parts < 0 || (n_parts && (!parts || !part_records || !part_device))) return bad("null parts, part_records or part_device");
    const bool host = devices[0] == -1;
    for (int i = 0; i < n_devices; i++) {
        if (devices[i] < -1) return bad("bad device " + std::to_string(devices[i]));
        if ((devices[i] == -1) != host) return bad("the device list mixes -1 (the host twin) with device ordinals");
    }
    for (int p = 0; p < n_parts; p++) {
        if (!parts[p] && part_records[p]) return bad("part " + std::to_string(p) + " is null and has records");
        if (part_device[p] < -1) return bad("bad device of part " + std::to_string(p));
        if (host && part_device[p] != -1) return bad("part " + std::to_string(p) + " lies on a device and the host twin takes host parts only");
    }
    pg_kindex* ix = pg::kidx_new(devices, n_devices, K, mer127, true);
    int rc = PG_OK;
    if (!host) rc = pg::kidx_device_build_sharded(ix, parts, part_records, part_device, n_parts, stream);
    else pg::kidx_with_nw(ix->nw, [&](auto nw) { rc = pg::kidx_host_build<decltype(nw)::value>(ix, parts, part_records, n_parts); });
    return rc == PG_OK ? ix : pg::kidx_build_failed(ix, rc);
}

int pg::kidx_batch_args(const char* who, const pg_kindex* ix, const KidxBatch& b, const char* noun, unsigned checks) {
    const std::string w = std::string(who) + ": ", s = noun;
    if (!ix) { pg_set_error(w + "null index"); return PG_EINVAL; }
    if (b.n_seqs && !b.packed) { pg_set_error(w + "null " + s + " buffer"); return PG_EINVAL; }
    if (b.n_seqs && !b.uniform_len && (!b.word_off || !b.kmer_base)) { pg_set_error(w + "a ragged batch needs word_off and kmer_base"); return PG_EINVAL; }
    if (b.uniform_len > 0x7FFFFFFFu) { pg_set_error(w + "uniform_len out of range"); return PG_EINVAL; }
    if (b.uniform_len && (checks & KIDX_ARGS_KMERS)) {
        const uint64_t nk = (int)b.uniform_len >= ix->K ? (uint64_t)b.uniform_len - ix->K + 1 : 0;
        if (b.n_kmers != b.n_seqs * nk) { pg_set_error(w + "n_kmers does not match n_seqs * max(0, len - K + 1)"); return PG_EINVAL; }
    }
    if (b.n_seqs && b.uniform_len && (checks & KIDX_ARGS_WORDS) && b.n_words < b.n_seqs * (uint64_t)((b.uniform_len + 31) / 32) + (uint64_t)ix->nw + 1) {
        pg_set_error(w + "n_words is less than the " + s + "s' words and the nw + 1 readable words behind them");
        return PG_EINVAL;
    }
    if (b.n_seqs && (checks & KIDX_ARGS_TAIL) && b.n_words < (uint64_t)ix->nw + 1) { pg_set_error(w + "n_words does not hold the nw + 1 readable words"); return PG_EINVAL; }
    return PG_OK;
}

namespace {

// pg_kindex_query (an index in one table: n_words is not stated) and pg_kindex_query_words (a cut one: KIDX_ARGS_WORDS too)
int kidx_query(const char* who, pg_kindex* ix, const pg::KidxBatch& b, unsigned checks, int wave, uint64_t* out_cnt, uint64_t* out_summary, void* stream) {
    if (ix && !out_cnt && !out_summary) { pg_set_error(std::string(who) + ": out_cnt and out_summary are both null"); return PG_EINVAL; }
    if (int rc = pg::kidx_batch_args(who, ix, b, "sequence", checks)) return rc;
    if (ix->device >= 0)
        return ix->cut ? pg::kidx_device_query_sharded(ix, b, wave, out_cnt, out_summary, stream) : pg::kidx_device_query(ix, b, wave, out_cnt, out_summary, stream);
    pg::kidx_with_nw(ix->nw, [&](auto nw) { pg::kidx_host_query<decltype(nw)::value>(ix, b, out_cnt, out_summary); });
    return PG_OK;
}

}  // namespace

extern "C" int pg_kindex_query_words(pg_kindex* ix, const uint64_t* packed, uint64_t n_words, const uint64_t* word_off, const uint64_t* kmer_base,
                                     uint64_t n_seqs, uint32_t uniform_len, uint64_t n_kmers, int wave, uint64_t* out_cnt, uint64_t* out_summary,
                                     void* stream) {
    if (ix && !ix->cut) return pg_kindex_query(ix, packed, word_off, kmer_base, n_seqs, uniform_len, n_kmers, wave, out_cnt, out_summary, stream);
    return kidx_query("pg_kindex_query_words", ix, pg::KidxBatch{packed, word_off, kmer_base, n_seqs, uniform_len, n_words, n_kmers},
                      pg::KIDX_ARGS_KMERS | pg::KIDX_ARGS_WORDS, wave, out_cnt, out_summary, stream);
}

extern "C" int pg_kindex_query(pg_kindex* ix, const uint64_t* packed, const uint64_t* word_off, const uint64_t* kmer_base, uint64_t n_seqs,
                               uint32_t uniform_len, uint64_t n_kmers, int wave, uint64_t* out_cnt, uint64_t* out_summary, void* stream) {
    if (ix && ix->cut) {
        pg_set_error("pg_kindex_query: the index is cut over ranks and a batch has to be copied to them: call pg_kindex_query_words, which takes the batch's words");
        return PG_EINVAL;
    }
    return kidx_query("pg_kindex_query", ix, pg::KidxBatch{packed, word_off, kmer_base, n_seqs, uniform_len, 0, n_kmers}, pg::KIDX_ARGS_KMERS, wave, out_cnt,
                      out_summary, stream);
}

extern "C" int pg_kindex_correct(pg_kindex* ix, const uint64_t* packed, const uint64_t* word_off, const uint64_t* kmer_base, uint64_t n_seqs,
                                 uint32_t uniform_len, uint64_t n_words, uint32_t min_cov, uint32_t max_fixes, uint32_t min_run,
                                 uint64_t* packed_out, uint64_t* out_report, void* stream) {
    if (!ix) { pg_set_error("pg_kindex_correct: null index"); return PG_EINVAL; }
    if (ix->cut) {
        pg_set_error("pg_kindex_correct: the index is cut over ranks; a read's trials are chains of dependent lookups, which merged rows cannot answer: "
                     "correct against an index in one table");
        return PG_ESTATE;
    }
    if (!min_cov || !min_run || max_fixes > pg::KCOR_MAX_FIXES) { pg_set_error("pg_kindex_correct: min_cov and min_run are at least 1, max_fixes at most 255"); return PG_EINVAL; }
    if (!packed_out) { pg_set_error("pg_kindex_correct: null packed_out"); return PG_EINVAL; }
    if (!n_seqs) return PG_OK;
    const pg::KidxBatch b{packed, word_off, kmer_base, n_seqs, uniform_len, n_words, 0};
    if (int rc = pg::kidx_batch_args("pg_kindex_correct", ix, b, "read", pg::KIDX_ARGS_WORDS)) return rc;
    const pg::KcorParams pr{min_cov, max_fixes, min_run};
    if (ix->device >= 0) return pg::kcor_device_correct(ix, b, pr, packed_out, out_report, stream);
    pg::kidx_with_nw(ix->nw, [&](auto nw) { pg::kcor_host_correct<decltype(nw)::value>(ix, b, pr, packed_out, out_report); });
    return PG_OK;
}

extern "C" int pg_kindex_rank_info(const pg_kindex* ix, int rank, uint64_t out[4]) {
    if (!ix || !out) { pg_set_error("pg_kindex_rank_info: null argument"); return PG_EINVAL; }
    if (rank < 0 || (size_t)rank >= ix->ranks.size()) { pg_set_error("pg_kindex_rank_info: no such rank"); return PG_EINVAL; }
    const pg::KidxRank& r = ix->ranks[(size_t)rank];
    out[0] = r.keys;
    out[1] = r.slots;
    out[2] = r.slots * (uint64_t)(ix->nw + 2) * sizeof(uint64_t);
    out[3] = (uint64_t)(int64_t)r.device;
    return PG_OK;
}

// the sums over the ranks' tables, on the lead's device
extern "C" int pg_kindex_info(const pg_kindex* ix, uint64_t out[4]) {
    if (!ix || !out) { pg_set_error("pg_kindex_info: null argument"); return PG_EINVAL; }
    out[0] = out[1] = out[2] = 0;
    for (int i = 0; i < (int)ix->ranks.size(); i++) {
        uint64_t r[4];
        (void)pg_kindex_rank_info(ix, i, r);
        for (int q = 0; q < 3; q++) out[q] += r[q];
    }
    out[3] = (uint64_t)(int64_t)ix->device;
    return PG_OK;
}

extern "C" int pg_kindex_ranks(const pg_kindex* ix) {
    if (!ix) { pg_set_error("pg_kindex_ranks: null index"); return PG_EINVAL; }
    return ix->cut ? (int)ix->ranks.size() : 0;
}

extern "C" int pg_kindex_query_times(pg_kindex* ix, double out[4]) {
    if (!ix || !out) { pg_set_error("pg_kindex_query_times: null argument"); return PG_EINVAL; }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!ix->cut || ix->device < 0) return PG_OK;
    return pg::kidx_device_query_times(ix, out);
}

extern "C" void pg_kindex_destroy(pg_kindex* ix) {
    if (!ix) return;
    if (ix->device >= 0) pg::kidx_device_free(ix);
    delete ix;
}

extern "C" uint64_t pg_host_kindex_bytes(uint64_t n_records, int mer127) { return pg::kidx_table_bytes(n_records, mer127 ? 4 : 2); }
