// map_index.hpp -- the contig k-mer index of the `map` stage, its read side (map_find: the probe, map_stretch: roll / canonicalise / probe
// over a stretch of a read's k-mers, shared by both kernels and the host twin) and the two engines that map reads with it (device:
// map_kernels.hip, host twin: map_host.cpp).  The build side stays with each engine: a CAS protocol on the device, a serial insert on the host.
// The probe loop (map_probe) and the roll (map_roll) are also what the k-mer index of kindex.hpp reads its table with (kidx_find).
//
// The reference (prlContig2nodes, prlHashCtg.c:345-467) puts every canonical K-mer of every contig of K + 2 bases or more into its k-mer
// sets: the first put keeps (contig id, position, twin), a second put of the same key marks it deleted (singleKmer, :131-155), and a deleted
// key reads as "no node" (searchKmer, prlRead2Ctg.c:233-246).  Which put comes first only matters for keys that end up deleted, so the
// index does not depend on insertion order, on -p, or on the sets' layout: here it is one open-addressing table, built fully in parallel.
//   slot = NW key words | value | state        value = map_hit(ctg, pos, twin, 0) (map_decide.hpp)
//   state: 0 empty, 1 claimed (key being written), 2 one put, 3 two puts or more (deleted)
#pragma once
#include <stdint.h>
#include <time.h>
#include <memory>
#include <vector>

#include "device_list.hpp"
#include "extract.hpp"
#include "kmer.hpp"
#include "map_decide.hpp"

namespace pg {

template <int NW> PG_HD constexpr int map_slot_words() { return NW + 2; }
constexpr uint64_t MAP_EMPTY = 0, MAP_CLAIMED = 1, MAP_ONCE = 2, MAP_DELETED = 3;

// 64-bit hash of a canonical key (splitmix64's finaliser over the words)
template <int NW>
PG_HD uint64_t map_hash(const Kmer<NW>& k) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        h ^= k.w[i] + 0x9E3779B97F4A7C15ULL + (h << 6) + (h >> 2);
        h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ULL;
        h ^= h >> 27; h *= 0x94D049BB133111EBULL;
        h ^= h >> 31;
    }
    return h;
}

// home slot of a canonical key
template <int NW>
PG_HD uint64_t map_home(const Kmer<NW>& k, uint64_t mask) { return map_hash<NW>(k) & mask; }

// The rank that holds a key when the index is cut over n ranks (ShardedDeviceMapEngine, the sharded host twin): the hash's bits 40 and
// up, which no slot index of a table that fits a card reaches (2^40 slots are 32 TB), so a rank's keys spread over its own table as the
// whole set does over one.  n need not be a power of two.  Every put of a key reaches the same rank, so "the first put keeps, a second
// put deletes" holds inside a rank's table
constexpr int MAP_OWNER_SHIFT = 40;
template <int NW>
PG_HD uint32_t map_owner(const Kmer<NW>& k, uint32_t n) { return (uint32_t)((map_hash<NW>(k) >> MAP_OWNER_SHIFT) % n); }

// The probe of a finished table, shared by the finds below: the slot that holds canonical key ck, null when the key is not in the table
template <int NW>
PG_HD const uint64_t* map_probe(const uint64_t* tab, uint64_t mask, const Kmer<NW>& ck) {
    constexpr int SW = map_slot_words<NW>();
    for (uint64_t e = map_home<NW>(ck, mask);; e = (e + 1) & mask) {
        const uint64_t* sl = tab + e * SW;
        if (sl[NW + 1] == MAP_EMPTY) return nullptr;
        bool eq = true;
#pragma unroll
        for (int i = 0; i < NW; i++) eq = eq && sl[i] == ck.w[i];
        if (eq) return sl;
    }
}

// The read-side probe over a finished table (searchKmer, prlRead2Ctg.c:233-246): the hit word of canonical key ck, 0 when the key is not
// there or is deleted.  sm = the read's own strand is the canonical one (the hit word's `smaller` bit)
template <int NW>
PG_HD uint64_t map_find(const uint64_t* tab, uint64_t mask, const Kmer<NW>& ck, bool sm) {
    const uint64_t* sl = map_probe<NW>(tab, mask, ck);
    return !sl || sl[NW + 1] == MAP_DELETED ? 0 : sl[NW] | ((uint64_t)(sm ? 1 : 0) << 32);
}

// Its sibling over the k-mer index of kindex.hpp, whose value is a pass-1 record's counter word: the word as it was stored, 0 when the
// key is not in the set (a stored word has coverage >= 1 in bits 31:24; no key of that table is ever taken out of its slot: a k-mer that
// tip clipping removes, ktip.hpp, keeps its slot with the word 0 and so reads as absent here)
template <int NW>
PG_HD uint64_t kidx_find(const uint64_t* tab, uint64_t mask, const Kmer<NW>& ck) {
    const uint64_t* sl = map_probe<NW>(tab, mask, ck);
    return sl ? sl[NW] : 0;
}

// k-mers j0 .. j1 - 1 of the packed read rd (chopKmer4read, prlRead2Ctg.c:153-231): roll, canonicalise, f(canonical key, sm, j) for each.
// Nothing is read when the stretch is empty; else the NW + 1 words from the one that holds base j0 on, and the bases up to j1 + K - 2
template <int NW, typename F>
PG_HD void map_roll(const uint64_t* rd, int j0, int j1, int K, F f) {
    if (j0 >= j1) return;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    Kmer<NW> word = read_kmer<NW>(rd, j0, K, filter);
    Kmer<NW> bal = kmer_rc<NW>(word, K);
    for (int j = j0; j < j1; j++) {
        if (j > j0) kmer_roll<NW>(word, bal, read_base(rd, j + K - 1), K, filter);
        const bool sm = kmer_less<NW>(word, bal);
        f(sm ? word : bal, sm, j);
    }
}

// map_roll + searchKmer (prlRead2Ctg.c:233-246) for the keys that own(key) takes: row[j] = the hit word, then on_hit(hit, j).  A key
// that is not taken leaves row[j] as it is
template <int NW, typename Own, typename OnHit>
PG_HD void map_stretch_if(const uint64_t* rd, int j0, int j1, int K, const uint64_t* tab, uint64_t mask, uint64_t* row, Own own, OnHit on_hit) {
    map_roll<NW>(rd, j0, j1, K, [&](const Kmer<NW>& ck, bool sm, int j) {
        if (!own(ck)) return;
        const uint64_t hit = map_find<NW>(tab, mask, ck, sm);
        row[j] = hit;
        on_hit(hit, j);
    });
}

// the whole index in one table: every key is probed
template <int NW, typename OnHit>
PG_HD void map_stretch(const uint64_t* rd, int j0, int j1, int K, const uint64_t* tab, uint64_t mask, uint64_t* row, OnHit on_hit) {
    map_stretch_if<NW>(rd, j0, j1, K, tab, mask, row, [](const Kmer<NW>&) { return true; }, on_hit);
}

// slots of the table for n k-mers: a power of two, at most half full
inline uint64_t map_table_slots(uint64_t n_kmers) {
    uint64_t s = 1024;
    while (s < 2 * n_kmers) s <<= 1;
    return s;
}

// Contigs as the index takes them: those of K + 2 bases or more, packed with pg_pack_read's layout (every contig on a word boundary,
// `words` padded with NW + 1 zero words), with the id each one's k-mers carry (getID of the name, or the ordinal; prlHashCtg.c:436).
struct MapContigs {
    std::vector<uint64_t> words;
    std::vector<uint64_t> off;            // [n + 1] word offsets
    std::vector<int32_t> len;
    std::vector<uint32_t> id;
    uint64_t n_kmers = 0;
};

// A batch of reads, packed the same way; kmer_off[r] = k-mers of the reads before r (reads shorter than K + 1 have none).
struct MapBatch {
    const uint64_t* words;
    uint64_t n_words;
    const uint64_t* off;
    const int32_t* len;
    const uint64_t* kmer_off;             // [n + 1]
    uint64_t n;
};

// the stage's clock: the engines' copy times and call_map.cpp's report
inline double now_s() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

class MapEngine {
public:
    virtual ~MapEngine() {}
    // build the index of `c`; ctg_len / bal = basicContigInfo's arrays, indexed by contig id (n_ids entries)
    virtual int build(const MapContigs& c, const int32_t* ctg_len, const int8_t* bal, uint32_t n_ids) = 0;
    // map a batch: out[r] = parse1read of read r with the batch's ALIGNLEN.  rows_out (tests, pg_map_hits): when not null, receives
    // the batch's hit words, read r's at rows_out + kmer_off[r] (kmer_off[n] entries)
    // wave: the device runs the wave-per-read kernel of the long-read pass (map_read_wave_kernel) instead of the lane-per-read one; the
    // answers are the same, and the host twin has one form for both
    virtual int map(const MapBatch& b, int align_len, MapOut* out, uint64_t* rows_out = nullptr, bool wave = false) = 0;
    // seconds spent building the index / in the read kernels (device: measured by events), for the stage's report
    double t_index = 0, t_kernel = 0, t_copy = 0;
    // the wave kernel's figures: reads whose ids did not fit its LDS table (done in passes), distinct ids summed over the reads with k-mers
    uint64_t n_passes = 0, n_ids = 0;
    // an index cut over ranks (map_owner): a rank's keys, the slots of its table and the seconds its probe kernel ran; t_kernel is then the
    // lead's probe + its wait for the slowest rank's + merge + decide, with t_merge (the rows' copies to the lead and the OR, from the moment every rank's probe is done) and t_decide apart.  Empty: one table
    struct Rank { uint64_t keys = 0, slots = 0; double t_probe = 0; };
    std::vector<Rank> ranks;
    double t_merge = 0, t_decide = 0;
};

// K and the flavour (nw = 2: the 63-mer build, 4: the 127-mer build)
std::unique_ptr<MapEngine> map_engine_device(int device, int K, int nw);
std::unique_ptr<MapEngine> map_engine_host(int K, int nw);
// the index cut over n ranks (1 to DEVICE_LIST_MAX_RANKS, device_list.hpp) by map_owner: rank i on (devices[i], a stream of its own), rank 0 the lead; an ordinal may repeat.  The
// host form: n serial tables
std::unique_ptr<MapEngine> map_engine_device_sharded(const int* devices, int n, int K, int nw);
std::unique_ptr<MapEngine> map_engine_host_sharded(int n, int K, int nw);
// map_rows_merge_kernel on `stream` of the current device: d_rows[i] |= d_part[i] for n_words words (the sharded engine's merge of another
// rank's rows into the lead's, and the k-mer index's, kindex_kernels.hip); PG_OK or PG_ENODEV
int map_rows_merge(uint64_t* d_rows, const uint64_t* d_part, uint64_t n_words, void* stream);
// free memory of a device as the arena sees it (the plan's device_bytes); PG_OK or PG_ENODEV
int map_device_free_bytes(int device, uint64_t* free_bytes);
// distinct contig ids of a read that the wave kernel's LDS table holds (more: the read is done in passes)
int map_wave_ids();

}  // namespace pg
