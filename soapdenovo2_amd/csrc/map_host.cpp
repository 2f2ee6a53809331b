// map_host.cpp -- host twin of map_kernels.hip: the same contig k-mer index (map_index.hpp) built by one thread, the same lookups
// (map_stretch) and per-read decision (map_decide.hpp) over host threads.  What the CPU tests run, and the device path's yardstick (pg_map_reads, device = -1).
// The index cut over ranks by key (map_owner; the device's ShardedDeviceMapEngine) has its twin here too: n serial tables (a device list of -1s).
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "host_reads.hpp"
#include "map_index.hpp"

void pg_set_error(const std::string& s);

namespace pg {
namespace {

template <int NW>
struct HostIndex {
    std::vector<uint64_t> tab;
    uint64_t mask = 0, keys = 0;
    // f(canonical key, contig, k-mer, the contig's own strand is the canonical one) for every k-mer of the contigs
    template <typename F>
    static void each_kmer(const MapContigs& c, int K, F f) {
        const Kmer<NW> filter = kmer_filter<NW>(K);
        for (size_t i = 0; i < c.len.size(); i++) {
            const uint64_t* rd = c.words.data() + c.off[i];
            const int nk = c.len[i] - K + 1;
            Kmer<NW> word = read_kmer<NW>(rd, 0, K, filter), bal = kmer_rc<NW>(word, K);
            for (int j = 0; j < nk; j++) {
                if (j) kmer_roll<NW>(word, bal, read_base(rd, j + K - 1), K, filter);
                const bool sm = kmer_less<NW>(word, bal);
                f(sm ? word : bal, i, j, sm);
            }
        }
    }
    // the keys that rank `me` of n owns (map_owner), counted first so that the table is made for them; n = 1: every key, one table
    void build(const MapContigs& c, int K, uint32_t n = 1, uint32_t me = 0) {
        constexpr int SW = map_slot_words<NW>();
        keys = c.n_kmers;
        if (n > 1) {
            keys = 0;
            each_kmer(c, K, [&](const Kmer<NW>& ck, size_t, int, bool) { keys += map_owner<NW>(ck, n) == me ? 1 : 0; });
        }
        const uint64_t slots = map_table_slots(keys);
        mask = slots - 1;
        tab.assign(slots * SW, 0);
        each_kmer(c, K, [&](const Kmer<NW>& ck, size_t i, int j, bool sm) {
            if (n > 1 && map_owner<NW>(ck, n) != me) return;
            uint64_t e = map_home<NW>(ck, mask);
            for (;;) {
                uint64_t* sl = tab.data() + e * SW;
                if (sl[NW + 1] == MAP_EMPTY) {
                    for (int q = 0; q < NW; q++) sl[q] = ck.w[q];
                    sl[NW] = map_hit(c.id[i], (uint32_t)j, sm ? 0 : 1, 0);
                    sl[NW + 1] = MAP_ONCE;
                    break;
                }
                bool eq = true;
                for (int q = 0; q < NW; q++) eq = eq && sl[q] == ck.w[q];
                if (eq) { sl[NW + 1] = MAP_DELETED; break; }
                e = (e + 1) & mask;
            }
        });
    }
};

// n_ranks = 0: one table.  n_ranks >= 1: the index cut over that many serial tables by map_owner, as ShardedDeviceMapEngine cuts it over
// devices -- every rank rolls through the read, probes the keys it owns into a zeroed row of its own, and the rows are ORed together
template <int NW>
class HostMapEngine : public MapEngine {
public:
    HostMapEngine(int K, int n_ranks) : K_(K), idx_((size_t)std::max(1, n_ranks)) { ranks.resize((size_t)n_ranks); }
    int build(const MapContigs& c, const int32_t* ctg_len, const int8_t* bal, uint32_t n_ids) override {
        len_.assign(ctg_len, ctg_len + n_ids);
        bal_.assign(bal, bal + n_ids);
        if (ranks.empty()) idx_[0].build(c, K_);
        for (size_t r = 0; r < ranks.size(); r++) {
            idx_[r].build(c, K_, (uint32_t)ranks.size(), (uint32_t)r);
            ranks[r].keys = idx_[r].keys;
            ranks[r].slots = idx_[r].mask + 1;
        }
        return PG_OK;
    }
    int map(const MapBatch& b, int align_len, MapOut* out, uint64_t* rows_out, bool) override {
        const MapCtgs ctgs{len_.data(), bal_.data(), (uint32_t)len_.size()};
        const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)host_threads(0), (b.n + 1023) / 1024));
        const uint32_t n = (uint32_t)ranks.size();
        auto body = [&](int t) {
            std::vector<uint64_t> row, part;
            for (uint64_t r = b.n * t / nt; r < b.n * (t + 1) / nt; r++) {
                const int len = b.len[r];
                const int nk = len >= K_ + 1 ? len - K_ + 1 : 0;
                row.assign((size_t)nk, 0);
                if (!n) map_stretch<NW>(b.words + b.off[r], 0, nk, K_, idx_[0].tab.data(), idx_[0].mask, row.data(), [](uint64_t, int) {});
                for (uint32_t me = 0; me < n; me++) {
                    part.assign((size_t)nk, 0);
                    map_stretch_if<NW>(b.words + b.off[r], 0, nk, K_, idx_[me].tab.data(), idx_[me].mask, part.data(),
                                       [n, me](const Kmer<NW>& ck) { return map_owner<NW>(ck, n) == me; }, [](uint64_t, int) {});
                    for (int j = 0; j < nk; j++) row[(size_t)j] |= part[(size_t)j];
                }
                if (rows_out && nk) memcpy(rows_out + b.kmer_off[r], row.data(), (size_t)nk * sizeof(uint64_t));
                out[r] = map_decide(MapRow{row.data()}, nk, K_, map_multi(len, align_len, K_), ctgs);
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt; t++) th.emplace_back(body, t);
        body(0);
        for (auto& x : th) x.join();
        return PG_OK;
    }

private:
    int K_;
    std::vector<HostIndex<NW>> idx_;
    std::vector<int32_t> len_;
    std::vector<int8_t> bal_;
};

}  // namespace

std::unique_ptr<MapEngine> map_engine_host(int K, int nw) {
    if (nw == 2) return std::unique_ptr<MapEngine>(new HostMapEngine<2>(K, 0));
    return std::unique_ptr<MapEngine>(new HostMapEngine<4>(K, 0));
}

std::unique_ptr<MapEngine> map_engine_host_sharded(int n, int K, int nw) {
    if (n < 1 || n > DEVICE_LIST_MAX_RANKS) { pg_set_error("map: an index is cut over 1 to " + std::to_string(DEVICE_LIST_MAX_RANKS) + " ranks"); return nullptr; }
    if (nw == 2) return std::unique_ptr<MapEngine>(new HostMapEngine<2>(K, n));
    return std::unique_ptr<MapEngine>(new HostMapEngine<4>(K, n));
}

}  // namespace pg

// what the wave kernel reported for the last pg_map_long_reads call (pg_map_long_last_stats)
static uint64_t g_long_stats[2] = {0, 0};

// pg_map_reads / pg_map_hits (include/soapdenovo2_amd.h): one index, one batch
// devices = null: one index on `device` (-1: the host twin); else the index cut over n_devices ranks (all -1: the sharded host twin)
static int map_one_batch(const char* who, int device, const int* devices, int n_devices, int K, int mer127, const uint64_t* ctg_words, const uint64_t* ctg_off,
                         const int32_t* ctg_len_bases, const uint32_t* ctg_ids, uint64_t n_ctg, const int32_t* id_len, const int8_t* id_bal,
                         uint32_t n_ids, const uint64_t* read_words, const uint64_t* read_off, const int32_t* read_len, uint64_t n_reads,
                         int align_len, uint32_t* out_ctg, int32_t* out_pos, uint8_t* out_orien, uint8_t* out_footprint, uint64_t* rows,
                         uint64_t* kmer_off, bool wave = false) {
    const int nw = mer127 ? 4 : 2;
    if (K < 1 || K > (mer127 ? 127 : 63)) { pg_set_error(std::string(who) + ": K out of range"); return PG_EINVAL; }
    pg::MapContigs c;
    c.off.assign(ctg_off, ctg_off + n_ctg + 1);
    c.len.assign(ctg_len_bases, ctg_len_bases + n_ctg);
    c.id.assign(ctg_ids, ctg_ids + n_ctg);
    c.words.assign(ctg_words, ctg_words + (n_ctg ? ctg_off[n_ctg] : 0));
    c.words.resize(c.words.size() + 8, 0);
    for (uint64_t i = 0; i < n_ctg; i++) {
        if (c.len[i] < K + 2) { pg_set_error(std::string(who) + ": the index takes contigs of K + 2 bases or more only"); return PG_EINVAL; }
        c.n_kmers += (uint64_t)(c.len[i] - K + 1);
    }
    std::unique_ptr<pg::MapEngine> e;
    if (!devices) e = device < 0 ? pg::map_engine_host(K, nw) : pg::map_engine_device(device, K, nw);
    else {
        int n_host = 0;
        for (int i = 0; i < n_devices; i++) n_host += devices[i] < 0 ? 1 : 0;
        if (n_devices < 1 || (n_host && n_host != n_devices)) {
            pg_set_error(std::string(who) + ": the device list names one rank or more, all on GPUs or all -1 (the host twin)");
            return PG_EINVAL;
        }
        e = n_host ? pg::map_engine_host_sharded(n_devices, K, nw) : pg::map_engine_device_sharded(devices, n_devices, K, nw);
    }
    if (!e) return PG_ENODEV;
    int rc = e->build(c, id_len, id_bal, n_ids);
    if (rc) return rc;
    std::vector<uint64_t> words(read_words, read_words + (n_reads ? read_off[n_reads] : 0)), koff(n_reads + 1, 0);
    words.resize(words.size() + 8, 0);
    for (uint64_t r = 0; r < n_reads; r++) koff[r + 1] = koff[r] + (read_len[r] >= K + 1 ? (uint64_t)(read_len[r] - K + 1) : 0);
    if (kmer_off) memcpy(kmer_off, koff.data(), (n_reads + 1) * sizeof(uint64_t));
    std::vector<pg::MapOut> out(n_reads);
    rc = e->map(pg::MapBatch{words.data(), words.size(), read_off, read_len, koff.data(), n_reads}, align_len, out.data(), rows, wave);
    if (rc) return rc;
    if (wave) { g_long_stats[0] = e->n_passes; g_long_stats[1] = e->n_ids; }
    for (uint64_t r = 0; r < n_reads; r++) {
        out_ctg[r] = out[r].ctg; out_pos[r] = out[r].pos; out_orien[r] = out[r].orien; out_footprint[r] = out[r].footprint;
    }
    return PG_OK;
}

extern "C" int pg_map_reads(int device, int K, int mer127, const uint64_t* ctg_words, const uint64_t* ctg_off, const int32_t* ctg_len_bases,
                            const uint32_t* ctg_ids, uint64_t n_ctg, const int32_t* id_len, const int8_t* id_bal, uint32_t n_ids,
                            const uint64_t* read_words, const uint64_t* read_off, const int32_t* read_len, uint64_t n_reads, int align_len,
                            uint32_t* out_ctg, int32_t* out_pos, uint8_t* out_orien, uint8_t* out_footprint) {
    return map_one_batch("pg_map_reads", device, nullptr, 0, K, mer127, ctg_words, ctg_off, ctg_len_bases, ctg_ids, n_ctg, id_len, id_bal, n_ids,
                         read_words, read_off, read_len, n_reads, align_len, out_ctg, out_pos, out_orien, out_footprint, nullptr, nullptr);
}

extern "C" int pg_map_hits(int device, int K, int mer127, const uint64_t* ctg_words, const uint64_t* ctg_off, const int32_t* ctg_len_bases,
                           const uint32_t* ctg_ids, uint64_t n_ctg, const int32_t* id_len, const int8_t* id_bal, uint32_t n_ids,
                           const uint64_t* read_words, const uint64_t* read_off, const int32_t* read_len, uint64_t n_reads, int align_len,
                           uint32_t* out_ctg, int32_t* out_pos, uint8_t* out_orien, uint8_t* out_footprint, uint64_t* rows,
                           uint64_t* kmer_off) {
    if (!rows || !kmer_off) { pg_set_error("pg_map_hits: rows and kmer_off are required"); return PG_EINVAL; }
    return map_one_batch("pg_map_hits", device, nullptr, 0, K, mer127, ctg_words, ctg_off, ctg_len_bases, ctg_ids, n_ctg, id_len, id_bal, n_ids,
                         read_words, read_off, read_len, n_reads, align_len, out_ctg, out_pos, out_orien, out_footprint, rows, kmer_off);
}

// prlLongRead2Ctg's batch (prlRead2Ctg.c:1080): the wave-per-read kernel on the device, the host twin's one form with device = -1
extern "C" int pg_map_long_reads(int device, int K, int mer127, const uint64_t* ctg_words, const uint64_t* ctg_off, const int32_t* ctg_len_bases,
                                 const uint32_t* ctg_ids, uint64_t n_ctg, const int32_t* id_len, const int8_t* id_bal, uint32_t n_ids,
                                 const uint64_t* read_words, const uint64_t* read_off, const int32_t* read_len, uint64_t n_reads,
                                 int align_len, uint32_t* out_ctg, int32_t* out_pos, uint8_t* out_orien, uint8_t* out_footprint,
                                 uint64_t* rows, uint64_t* kmer_off) {
    return map_one_batch("pg_map_long_reads", device, nullptr, 0, K, mer127, ctg_words, ctg_off, ctg_len_bases, ctg_ids, n_ctg, id_len, id_bal, n_ids,
                         read_words, read_off, read_len, n_reads, align_len, out_ctg, out_pos, out_orien, out_footprint, rows, kmer_off, true);
}

// the same three with the index cut over the ranks of a device list
#define MAP_BATCH_ARGS                                                                                                                    \
    int K, int mer127, const uint64_t *ctg_words, const uint64_t *ctg_off, const int32_t *ctg_len_bases, const uint32_t *ctg_ids,         \
        uint64_t n_ctg, const int32_t *id_len, const int8_t *id_bal, uint32_t n_ids, const uint64_t *read_words, const uint64_t *read_off, \
        const int32_t *read_len, uint64_t n_reads, int align_len, uint32_t *out_ctg, int32_t *out_pos, uint8_t *out_orien,                \
        uint8_t *out_footprint
#define MAP_BATCH_PASS                                                                                                                    \
    K, mer127, ctg_words, ctg_off, ctg_len_bases, ctg_ids, n_ctg, id_len, id_bal, n_ids, read_words, read_off, read_len, n_reads,         \
        align_len, out_ctg, out_pos, out_orien, out_footprint

extern "C" int pg_map_reads_sharded(const int* devices, int n_devices, MAP_BATCH_ARGS) {
    if (!devices) { pg_set_error("pg_map_reads_sharded: devices is required"); return PG_EINVAL; }
    return map_one_batch("pg_map_reads_sharded", 0, devices, n_devices, MAP_BATCH_PASS, nullptr, nullptr);
}

extern "C" int pg_map_hits_sharded(const int* devices, int n_devices, MAP_BATCH_ARGS, uint64_t* rows, uint64_t* kmer_off) {
    if (!devices || !rows || !kmer_off) { pg_set_error("pg_map_hits_sharded: devices, rows and kmer_off are required"); return PG_EINVAL; }
    return map_one_batch("pg_map_hits_sharded", 0, devices, n_devices, MAP_BATCH_PASS, rows, kmer_off);
}

extern "C" int pg_map_long_reads_sharded(const int* devices, int n_devices, MAP_BATCH_ARGS, uint64_t* rows, uint64_t* kmer_off) {
    if (!devices) { pg_set_error("pg_map_long_reads_sharded: devices is required"); return PG_EINVAL; }
    return map_one_batch("pg_map_long_reads_sharded", 0, devices, n_devices, MAP_BATCH_PASS, rows, kmer_off, true);
}

// map_owner of n packed canonical keys (NW words each, as Kmer<NW>::w), for tests
extern "C" int pg_host_map_owner(const uint64_t* keys, uint64_t n, int mer127, int n_ranks, uint32_t* out) {
    if ((!keys && n) || (!out && n) || n_ranks < 1) { pg_set_error("pg_host_map_owner: bad argument"); return PG_EINVAL; }
    for (uint64_t i = 0; i < n; i++) {
        if (mer127) { pg::Kmer<4> k; for (int q = 0; q < 4; q++) k.w[q] = keys[i * 4 + q]; out[i] = pg::map_owner<4>(k, (uint32_t)n_ranks); }
        else { pg::Kmer<2> k; for (int q = 0; q < 2; q++) k.w[q] = keys[i * 2 + q]; out[i] = pg::map_owner<2>(k, (uint32_t)n_ranks); }
    }
    return PG_OK;
}

#undef MAP_BATCH_ARGS
#undef MAP_BATCH_PASS

extern "C" void pg_map_long_last_stats(uint64_t out[2]) { out[0] = g_long_stats[0]; out[1] = g_long_stats[1]; }

extern "C" int pg_map_wave_ids(int) { return pg::map_wave_ids(); }
