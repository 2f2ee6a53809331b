// kindex.hpp -- the k-mer index: a lookup table over the distinct k-mers pass 1 counted, asked with batches of sequences (pg_kindex_*,
// include/soapdenovo2_amd.h section 3).  The reference has no such operator on its own; its multi-k step looks k-mers of reads up in a
// finished set the same way (contig -m: iterate.c, kmerhash.c).
//
// The table is map_index.hpp's: map_table_slots(n_records) slots (a power of two, at most half full, at least 1024), a slot = NW key
// words | value | state, home slot map_home, linear probing.  The value is the record's counter word as the ABI defines it (low 32 bit
// word A = l_links | covs << 24, high 32 bit word B); a stored record has coverage >= 1, so a value of 0 means "not in the set" and
// nothing else.  pg_finalize's -d filter does not take a k-mer out of the export array: it sets the record's `deleted` bit (thread_delow,
// prlHashReads.c:953-996; B_DELETED, kmer.hpp).  Such a record is not stored (kidx_stored), so a filtered k-mer reads as 0 too.
// State: 0 empty, 1 claimed (key being written), 2 published; the keys of the records are distinct by contract, and a
// build that meets a key twice fails.  The build side stays with each engine (kindex_kernels.hip: a CAS protocol, kindex_host.cpp: a
// serial insert); the read side -- kidx_find (map_index.hpp), kidx_stretch and the per-sequence summary below -- is one piece of code
// for the query kernel and the host twin.
//
// A batch of sequences (KidxBatch) is laid out as pg_count_reads' batches are: pg_pack_read words, either all of uniform_len bases
// (sequence r at word r * pg_packed_words(uniform_len)) or with word_off[n] + kmer_base[n + 1].  A sequence of len bases has
// max(0, len - K + 1) k-mers: one of exactly K bases has one (the "K + 1" rule is pregraph's reader's, not the query's).  Behind the
// last sequence NW + 1 words (3 in the 63-mer build, 5 in the 127-mer one) must be readable: read_kmer<NW> loads NW + 1 words from the
// one that holds the k-mer's first base on.  A sequence without k-mers is never read.
//
// The index cut over ranks (pg_kindex_build_sharded): rank i of n holds the stored records whose canonical key has map_owner(key, n) == i
// (map_index.hpp: the hash's bits 40 and up, modulo n) in a table of its own -- map_table_slots(owned_i) slots, the same slot format,
// cut from the arena of devices[i]; owned_i counts the records the rank owns, the deleted ones among them included, so that
// sum(owned_i) == n_records and a one-rank cut is pg_kindex_build's table: map_owner(key, 1) == 0 for every key.  So there is one
// shape of index, pg_kindex::ranks, and pg_kindex_build's single table is ranks[0] of an index that is not `cut`.  A rank that owns
// nothing keeps a zeroed table of the smallest size.  Rank 0 is the lead: a batch and its answers lie on its device.  A key has one
// owner and 0 means "absent", so the ranks' rows of a batch -- each rank probes the keys it owns into zeroed rows -- OR together into
// the answers (map_rows_merge_kernel), and the summary is taken from the finished rows.  The host twin is n serial tables with the
// same cut (kidx_host_find).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <type_traits>
#include <vector>

#include "map_index.hpp"

struct pg_kindex;

namespace pg {

constexpr uint64_t KIDX_EMPTY = MAP_EMPTY, KIDX_CLAIMED = MAP_CLAIMED, KIDX_FULL = MAP_ONCE;   // (map_probe tells empty from not empty only)
constexpr int KIDX_SUMMARY_WORDS = 4;

PG_HD uint32_t kidx_coverage(uint64_t cnt) { return (uint32_t)(cnt >> 24) & 0xffu; }
// a record with this counter word goes into the table: every one but those the -d filter deleted
PG_HD bool kidx_stored(uint64_t cnt) { return ((uint32_t)(cnt >> 32) & B_DELETED) == 0; }

// What a sequence's k-mers add up to: k-mers present, the sum of their coverage, the least coverage among them and the first k-mer
// that is absent.  Sums and minima: the order the k-mers arrive in, and how they are split over lanes, changes nothing
struct KidxSummary {
    uint64_t present, cov_sum;
    uint32_t cov_min;              // over the present k-mers; KIDX_NO_MIN while there is none
    uint32_t first_absent;         // KIDX_NO_ABSENT while every k-mer was present
};
constexpr uint32_t KIDX_NO_MIN = 0xFFFFFFFFu, KIDX_NO_ABSENT = 0xFFFFFFFFu;

PG_HD KidxSummary kidx_summary_none() { return KidxSummary{0, 0, KIDX_NO_MIN, KIDX_NO_ABSENT}; }

PG_HD void kidx_summary_add(KidxSummary& s, uint64_t cnt, int j) {
    if (cnt) {
        const uint32_t c = kidx_coverage(cnt);
        s.present++;
        s.cov_sum += c;
        s.cov_min = c < s.cov_min ? c : s.cov_min;
    } else
        s.first_absent = (uint32_t)j < s.first_absent ? (uint32_t)j : s.first_absent;
}

PG_HD void kidx_summary_merge(KidxSummary& s, const KidxSummary& o) {
    s.present += o.present;
    s.cov_sum += o.cov_sum;
    s.cov_min = o.cov_min < s.cov_min ? o.cov_min : s.cov_min;
    s.first_absent = o.first_absent < s.first_absent ? o.first_absent : s.first_absent;
}

// the four words of a sequence of nk k-mers: present, coverage sum, least coverage (0 when none is present), first absent (nk when none is)
PG_HD void kidx_summary_store(const KidxSummary& s, int nk, uint64_t* out4) {
    out4[0] = s.present;
    out4[1] = s.cov_sum;
    out4[2] = s.cov_min == KIDX_NO_MIN ? 0 : s.cov_min;
    out4[3] = s.first_absent == KIDX_NO_ABSENT ? (uint64_t)nk : s.first_absent;
}

// k-mers j0 .. j1 - 1 of the packed sequence rd: roll, canonicalise, probe (map_roll + kidx_find, map_index.hpp); out[j] = the counter
// word or 0 (out may be null), and every answer goes into s
template <int NW>
PG_HD void kidx_stretch(const uint64_t* rd, int j0, int j1, int K, const uint64_t* tab, uint64_t mask, uint64_t* out, KidxSummary& s) {
    map_roll<NW>(rd, j0, j1, K, [&](const Kmer<NW>& ck, bool, int j) {
        const uint64_t cnt = kidx_find<NW>(tab, mask, ck);
        if (out) out[j] = cnt;
        kidx_summary_add(s, cnt, j);
    });
}

// the key of a record in export format, or of a table slot: its first NW words
template <int NW>
PG_HD Kmer<NW> kidx_record_key(const uint64_t* rec) {
    Kmer<NW> k;
#pragma unroll
    for (int q = 0; q < NW; q++) k.w[q] = rec[q];
    return k;
}

// A batch as the ABI hands it over.  uniform_len != 0: word_off / kmer_base are not read.  n_words (the packed words, the NW + 1 readable
// ones behind the last sequence included) and n_kmers are what the caller states; an entry point that takes neither leaves them 0
struct KidxBatch {
    const uint64_t *packed, *word_off, *kmer_base;
    uint64_t n_seqs;
    uint32_t uniform_len;
    uint64_t n_words, n_kmers;
};

// sequence r of a batch: its k-mers and where its answers go (kidx_row: the words are not touched), and its words (kidx_seq)
struct KidxRow {
    uint64_t base;
    int nk;
};
struct KidxSeq {
    const uint64_t* rd;
    uint64_t base;
    int nk;
};
PG_HD int kidx_uniform_nk(uint32_t len, int K) { return (int)len >= K ? (int)len - K + 1 : 0; }
PG_HD KidxRow kidx_row(const KidxBatch& b, int K, uint64_t r) {
    if (b.uniform_len) {
        const int nk = kidx_uniform_nk(b.uniform_len, K);
        return KidxRow{r * (uint64_t)nk, nk};
    }
    return KidxRow{b.kmer_base[r], (int)(b.kmer_base[r + 1] - b.kmer_base[r])};
}
// (one branch, not kidx_row's and another: a ragged batch's loads of word_off and kmer_base stay in flight together)
PG_HD KidxSeq kidx_seq(const KidxBatch& b, int K, uint64_t r) {
    if (b.uniform_len) {
        const int nk = kidx_uniform_nk(b.uniform_len, K);
        return KidxSeq{b.packed + r * (uint64_t)((b.uniform_len + 31) / 32), r * (uint64_t)nk, nk};
    }
    return KidxSeq{b.packed + b.word_off[r], b.kmer_base[r], (int)(b.kmer_base[r + 1] - b.kmer_base[r])};
}

// f(std::integral_constant<int, NW>) for an index's flavour
template <typename F>
inline void kidx_with_nw(int nw, F f) {
    if (nw == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

inline uint64_t kidx_table_bytes(uint64_t n_records, int nw) { return map_table_slots(n_records) * (uint64_t)(nw + 2) * sizeof(uint64_t); }

// Records of a chunk: a part that does not lie on a rank's device reaches it through one buffer of this many records, an insert launch
// a chunk.  2^22 records are 128 MB in the 63-mer build and 192 MB in the 127-mer one: a copy of 2 to 4 ms over a 64 GB/s link or from
// pinned host memory, against some 10 us to launch it and its kernel, and under a thousandth of a card beside a table of tens of GB.
// SOAPDENOVO2_AMD_KINDEX_CHUNK_RECORDS (env_test, read at build time) makes it small, so that chunk edges run at test sizes
constexpr uint64_t KIDX_CHUNK_RECORDS = 1ull << 22;
uint64_t kidx_chunk_records();

// a rank of an index: the one table of pg_kindex_build, or one of a cut.  The device engine fills the device half, the host twin `tab`.
// The stream, the events and the batch buffers are a cut's: a rank of an index in one table has none
struct KidxRank {
    int device = -1;
    uint64_t keys = 0, slots = 0;  // the records it owns (deleted ones included), the slots of its table
    std::vector<uint64_t> tab;     // host twin
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // its probe of a batch runs from e0 to e1; the caller's stream waits for e1
    uint64_t* d_tab = nullptr;     // exactly slots * (nw + 2) words of the arena of `device`
    uint32_t* d_flags = nullptr;   // the build's flags (KIDX_FLAG_*)
    uint64_t* d_chunk = nullptr;   // the build's chunk buffer; given back when the build ends
    // the rank's copy of a batch (a rank off the lead's device) and its rows; they grow to the largest batch met
    uint64_t *d_packed = nullptr, *d_word_off = nullptr, *d_kmer_base = nullptr, *d_rows = nullptr;
    uint64_t cap_packed = 0, cap_seqs = 0, cap_rows = 0;
};

// what every entry point that takes a batch asks of it alike; `noun` is what the messages call a sequence ("sequence", "read")
enum : unsigned {
    KIDX_ARGS_KMERS = 1u,          // a uniform batch's n_kmers is n_seqs * max(0, len - K + 1)
    KIDX_ARGS_WORDS = 2u,          // a uniform batch's n_words holds the sequences' words and the nw + 1 readable ones
    KIDX_ARGS_TAIL = 4u,           // any batch's n_words holds the nw + 1 readable ones
};
int kidx_batch_args(const char* who, const ::pg_kindex* ix, const KidxBatch& b, const char* noun, unsigned checks);

// What the scans of the operators sum over their items, 256 items a workgroup (kindex_kernels.hip: kidx_block_scan and the kernels round
// it): up to four counts an item.  The trim's are ktrim_counts (ktrim.hpp), the unitigs' kunitig_counts (kunitig.hpp)
constexpr int KIDX_COUNTS = 4;
struct KidxCounts {
    uint64_t c[KIDX_COUNTS];
};

// An operator's scratch on the lead's device: a buffer that grows to the largest call met, the end event of the last call that used it
// -- a call on another stream than that one's waits for it on the device: the scratch is one -- and whether that event was recorded.
// A buffer that has to grow is given back first, and arena_free waits for the device as hipFree does, so no earlier call still uses it:
// the only place the host waits.  (kindex_kernels.hip: kidx_scratch_begin, kidx_scratch_end, kidx_scratch_free)
struct KidxScratch {
    uint64_t* d = nullptr;
    uint64_t cap = 0;              // words
    hipEvent_t e_end = nullptr;
    bool recorded = false;         // e_end has been recorded
};

// the device engine (kindex_kernels.hip); a table is cut from the arena of its rank's device.  PG_OK or a PG_E* code with pg_set_error done
int kidx_device_build(::pg_kindex* ix, const uint64_t* d_records, uint64_t n_records, void* stream);
int kidx_device_query(::pg_kindex* ix, const KidxBatch& b, int wave, uint64_t* d_out, uint64_t* d_summary, void* stream);
void kidx_device_free(::pg_kindex* ix);
// the index cut over ix->ranks (their `device` set): part p = part_records[p] records on device part_device[p], or in host memory (-1)
int kidx_device_build_sharded(::pg_kindex* ix, const uint64_t* const* parts, const uint64_t* part_records, const int* part_device, int n_parts,
                              void* stream);
int kidx_device_query_sharded(::pg_kindex* ix, const KidxBatch& b, int wave, uint64_t* d_out, uint64_t* d_summary, void* stream);
// the last sharded query's milliseconds from its events, after waiting for its end: the slowest rank's probe, the merge, the summary, all of it
int kidx_device_query_times(::pg_kindex* ix, double out[4]);

}  // namespace pg

struct pg_kindex {
    int device = -1;               // the lead's (rank 0's); -1: the host twin
    int K = 0, nw = 2;
    // One entry a rank, never empty, rank 0 the lead.  cut: pg_kindex_build_sharded made the index, a batch is copied to the ranks and
    // their rows merged (pg_kindex_query_words); else pg_kindex_build did and ranks[0] is the one table, asked in place
    std::vector<pg::KidxRank> ranks;
    bool cut = false;
    // the lead's alone: the buffer the other ranks' rows arrive in, and the events of a query on the caller's stream -- its begin, every
    // rank's probe waited for, merged, its end (which the next query's ranks wait for: the row buffers are reused)
    uint64_t* d_staging = nullptr;
    uint64_t cap_staging = 0;
    hipEvent_t e_begin = nullptr, e_probed = nullptr, e_merged = nullptr, e_end = nullptr;
    bool queried = false;          // e_end has been recorded
    // The operators' scratch on `device`, one each: merged into one buffer they would order calls on different streams that are independent.
    // trim (ktrim.hpp): the spans and source indices the caller did not ask for and the scan's block sums; e_trim are a trim's begin,
    // spans done and scan done, and its end is the scratch's.  cor (kcorrect_rows.hpp): the reads' state words and as-given bits, a
    // round's trial batch, its rows, the read of each trial and the claim counter.  uni (kunitig.hpp): the counters, the start list, the
    // lengths, the scan's block sums and a covered bit a slot; a round of tip clipping (ktip.hpp) uses its counters, start list and lengths,
    // and the ranked unitigs (krank.hpp) put their control words, records and node maps behind the counters
    pg::KidxScratch trim, cor, uni;
    hipEvent_t e_trim[3] = {nullptr, nullptr, nullptr};
    uint64_t cor_stats[4] = {0, 0, 0, 0};   // the last pg_kindex_correct_rows: rounds, trials, k-mers asked in trials, host waits
};

namespace pg {

// the host twin's lookup: the canonical k-mer ck in its owner's table (one rank: map_owner is 0)
template <int NW>
inline uint64_t kidx_host_find(const ::pg_kindex* ix, const Kmer<NW>& ck) {
    const KidxRank& r = ix->ranks[map_owner<NW>(ck, (uint32_t)ix->ranks.size())];
    return kidx_find<NW>(r.tab.data(), r.slots - 1, ck);
}

}  // namespace pg
