// map_kernels.hip -- the `map` stage on the GPU: the contig k-mer index (prlContig2nodes, standardPregraph/prlHashCtg.c:345-467) and the
// read kernel (chopKmer4read + searchKmer + parse1read, prlRead2Ctg.c:153-361), one lane a read like pass 2's p2_thread_kernel.
//
//   map_index_kernel  a lane per stretch of MAP_ITEM k-mers of one contig: roll the k-mer, canonicalise, insert into the open-addressing
//                     table of map_index.hpp.  A new key is claimed with a CAS on its state word, its words are written, and the state is
//                     published with a release store; a lane that meets a claimed slot tries the same slot again on its next trip round the
//                     loop (no lane waits inside a branch for another lane of its own wavefront).  An equal key moves the state to
//                     "deleted", so the table is a function of the contigs alone.  The trips a lane spends on one claimed slot are capped
//                     (MAP_SPIN_CAP): a lane that gives up raises a device flag, and build() fails instead of the card hanging.
//   map_read_kernel   a lane per read: roll, canonicalise, probe (map_stretch, map_index.hpp: the loop both read kernels and the host twin
//                     run); every k-mer's hit word goes to the read's row of the batch's hit buffer (the reference's nodeBuffer), then
//                     map_decide (map_decide.hpp) picks the contig from the row.
//   map_read_wave_kernel  a wavefront per read, for long reads (prlLongRead2Ctg, prlRead2Ctg.c:1080): the lanes share the read's k-mers and the
//                     decision is linear in them, through a per-wave table in LDS keyed by contig id (count, first hit).  Same rows, same
//                     out[] as map_read_kernel.
//   ShardedDeviceMapEngine  the index cut over ranks by key (map_owner, map_index.hpp) for a contig set whose one table does not fit a
//                     card: map_count_owned_kernel / map_index_owned_kernel build a rank's table from the keys it owns,
//                     map_probe_owned_kernel looks a batch's owned keys up into the rank's zeroed rows, map_rows_merge_kernel ORs the
//                     ranks' rows together on the lead, and map_decide_rows_kernel / map_decide_rows_wave_kernel run the decision
//                     halves of the two read kernels (map_lane_decide, map_wave_decide) from the finished rows.
// All of them wait for random 32- / 48-byte slot reads of a table that is many times the L2: the bound is HBM random-access latency and rate,
// not arithmetic.  Memory comes from the device arena (arena.hpp).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/soapdenovo2_amd.h"
#include "arena.hpp"
#include "map_index.hpp"

void pg_set_error(const std::string& s);

namespace pg {

constexpr int MAP_ITEM = 64;                      // k-mers of a contig a lane of the index build rolls through
// Trips round map_insert's loop a lane may spend on one claimed slot before it gives up.  A claim is held for NW + 1 stores; the most any
// lane needed in the homopolymer / tandem-repeat contention case on an MI355X is in DESIGN.md's map section, and this is > 1000 times it.
constexpr uint32_t MAP_SPIN_CAP = 1u << 20;

#define MAP_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            pg_set_error(std::string("map: ") + #call + ": " + hipGetErrorString(e_));                  \
            return PG_ENODEV;                                                                           \
        }                                                                                               \
    } while (0)

__device__ __forceinline__ uint64_t map_state_acquire(const uint64_t* p) {
    return __hip_atomic_load((uint64_t*)p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
}

template <int NW>
__device__ __forceinline__ void map_insert(uint64_t* tab, uint64_t mask, const Kmer<NW>& k, uint64_t value, uint32_t* gave_up) {
    constexpr int SW = map_slot_words<NW>();
    uint64_t e = map_home<NW>(k, mask);
    uint32_t waits = 0;                            // trips spent on slot e while it was claimed
    for (;;) {
        uint64_t* sl = tab + e * SW;
        uint64_t* st = sl + NW + 1;
        const uint64_t s = map_state_acquire(st);
        if (s == MAP_EMPTY) {
            if (atomicCAS((unsigned long long*)st, (unsigned long long)MAP_EMPTY, (unsigned long long)MAP_CLAIMED) == MAP_EMPTY) {
#pragma unroll
                for (int i = 0; i < NW; i++) sl[i] = k.w[i];
                sl[NW] = value;
                __hip_atomic_store(st, MAP_ONCE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            continue;                              // somebody claimed it first: look again
        }
        if (s == MAP_CLAIMED) {                    // its key is still being written
            if (++waits > MAP_SPIN_CAP) { atomicOr(gave_up, 1u); return; }
            continue;
        }
        bool eq = true;
#pragma unroll
        for (int i = 0; i < NW; i++) eq = eq && sl[i] == k.w[i];
        if (eq) {
            if (s == MAP_ONCE) __hip_atomic_store(st, MAP_DELETED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        e = (e + 1) & mask;
        waits = 0;
    }
}

// work item t of the index build: k-mers j0 .. j0 + MAP_ITEM - 1 of one contig, rolled and canonicalised; put(key, hit word) for each
template <int NW, typename Put>
__device__ __forceinline__ void map_index_item(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                               const int32_t* __restrict__ len, const uint32_t* __restrict__ ids,
                                               const uint32_t* __restrict__ item_ctg, const uint32_t* __restrict__ item_j0, uint64_t t, int K,
                                               Put put) {
    const uint32_t c = item_ctg[t];
    const int j0 = (int)item_j0[t];
    const int nk = len[c] - K + 1;
    const int j1 = nk < j0 + MAP_ITEM ? nk : j0 + MAP_ITEM;
    const uint64_t* rd = words + off[c];
    const uint32_t id = ids[c];
    const Kmer<NW> filter = kmer_filter<NW>(K);
    Kmer<NW> word = read_kmer<NW>(rd, j0, K, filter);
    Kmer<NW> bal = kmer_rc<NW>(word, K);
    for (int j = j0; j < j1; j++) {
        if (j > j0) kmer_roll<NW>(word, bal, read_base(rd, j + K - 1), K, filter);
        const bool sm = kmer_less<NW>(word, bal);
        put(sm ? word : bal, map_hit(id, (uint32_t)j, sm ? 0 : 1, 0));                 // twin = 0 when the contig's strand is canonical
    }
}

template <int NW>
__global__ __launch_bounds__(256) void map_index_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                        const int32_t* __restrict__ len, const uint32_t* __restrict__ ids,
                                                        const uint32_t* __restrict__ item_ctg, const uint32_t* __restrict__ item_j0,
                                                        uint64_t n_items, int K, uint64_t* tab, uint64_t mask, uint32_t* gave_up) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    map_index_item<NW>(words, off, len, ids, item_ctg, item_j0, t, K,
                       [=](const Kmer<NW>& k, uint64_t value) { map_insert<NW>(tab, mask, k, value, gave_up); });
}

// ---- the index cut over ranks (ShardedDeviceMapEngine): rank `me` of n keeps the keys with map_owner(key, n) == me ----
// the keys of the work items that rank `me` owns, added to *count: a sum per wavefront, one atomic a wavefront
template <int NW>
__global__ __launch_bounds__(256) void map_count_owned_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                              const int32_t* __restrict__ len, const uint32_t* __restrict__ ids,
                                                              const uint32_t* __restrict__ item_ctg, const uint32_t* __restrict__ item_j0,
                                                              uint64_t n_items, int K, uint32_t n, uint32_t me, unsigned long long* count) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int mine = 0;
    if (t < n_items)
        map_index_item<NW>(words, off, len, ids, item_ctg, item_j0, t, K,
                           [&mine, n, me](const Kmer<NW>& k, uint64_t) { mine += map_owner<NW>(k, n) == me ? 1u : 0u; });
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);                 // (every lane of the wavefront is here: nobody returned)
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);
}

// map_index_kernel for the keys rank `me` owns; tab is that rank's table
template <int NW>
__global__ __launch_bounds__(256) void map_index_owned_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                              const int32_t* __restrict__ len, const uint32_t* __restrict__ ids,
                                                              const uint32_t* __restrict__ item_ctg, const uint32_t* __restrict__ item_j0,
                                                              uint64_t n_items, int K, uint32_t n, uint32_t me, uint64_t* tab, uint64_t mask,
                                                              uint32_t* gave_up) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    map_index_item<NW>(words, off, len, ids, item_ctg, item_j0, t, K, [=](const Kmer<NW>& k, uint64_t value) {
        if (map_owner<NW>(k, n) == me) map_insert<NW>(tab, mask, k, value, gave_up);
    });
}

// k-mers of a read (prlRead2Ctg.c:159-162: a read shorter than K + 1 has none)
__device__ __forceinline__ int map_read_kmers(int len, int K) { return len >= K + 1 ? len - K + 1 : 0; }

// the lane-per-read decision from a finished row (parse1read): the half of map_read_kernel behind its lookups, and all of map_decide_rows_kernel
__device__ __forceinline__ MapOut map_lane_decide(const uint64_t* row, int len, int nk, int K, int align_len, const MapCtgs& ctgs) {
    return map_decide(MapRow{row}, nk, K, map_multi(len, align_len, K), ctgs);
}

template <int NW>
__global__ __launch_bounds__(256) void map_read_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                       const int32_t* __restrict__ lens, const uint64_t* __restrict__ koff, uint64_t n, int K,
                                                       int align_len, const uint64_t* __restrict__ tab, uint64_t mask, MapCtgs ctgs,
                                                       uint64_t* __restrict__ rows, MapOut* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int len = lens[r];
    const int nk = map_read_kmers(len, K);
    uint64_t* row = rows + koff[r];
    map_stretch<NW>(words + off[r], 0, nk, K, tab, mask, row, [](uint64_t, int) {});
    out[r] = map_lane_decide(row, len, nk, K, align_len, ctgs);
}

// the decision alone, a lane a read, from rows that are finished (the sharded engine: merged on the lead)
__global__ __launch_bounds__(256) void map_decide_rows_kernel(const int32_t* __restrict__ lens, const uint64_t* __restrict__ koff, uint64_t n, int K,
                                                              int align_len, MapCtgs ctgs, const uint64_t* __restrict__ rows,
                                                              MapOut* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int len = lens[r];
    out[r] = map_lane_decide(rows + koff[r], len, map_read_kmers(len, K), K, align_len, ctgs);
}

// A rank's lookups: k-mers of the batch's reads whose keys rank `me` of n owns are probed in its table and their hit words written to its
// row buffer, which was zeroed before (a key of another rank leaves its word 0).  WAVE = false: a lane a read, as map_read_kernel; true: a
// wavefront a read, a lane a stretch of ceil(nk / 64) k-mers, as map_read_wave_kernel (the long-read pass)
template <int NW, bool WAVE>
__global__ __launch_bounds__(256) void map_probe_owned_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                              const int32_t* __restrict__ lens, const uint64_t* __restrict__ koff, uint64_t n,
                                                              int K, uint32_t n_ranks, uint32_t me, const uint64_t* __restrict__ tab,
                                                              uint64_t mask, uint64_t* __restrict__ rows) {
    const uint64_t r = WAVE ? (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6) : (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int nk = map_read_kmers(lens[r], K);
    int j0 = 0, j1 = nk;
    if (WAVE) {
        const int per = (nk + 63) / 64;
        j0 = (int)(threadIdx.x & 63) * per;
        j1 = nk < j0 + per ? nk : j0 + per;
    }
    map_stretch_if<NW>(words + off[r], j0, j1, K, tab, mask, rows + koff[r],
                       [n_ranks, me](const Kmer<NW>& ck) { return map_owner<NW>(ck, n_ranks) == me; }, [](uint64_t, int) {});
}

// rows |= part: another rank's hit words into the lead's.  A k-mer's key has one owner, so at most one rank brings a word that is not 0
__global__ __launch_bounds__(256) void map_rows_merge_kernel(uint64_t* __restrict__ rows, const uint64_t* __restrict__ part, uint64_t n_words) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) {
        const uint64_t w = part[i];
        if (w) rows[i] |= w;
    }
}


// ---- a wavefront per read ----
// The decision needs, per distinct contig id of the row, the number of hits and the first hit (map_decide.hpp).  A wave gathers them in an
// open-addressing table in LDS keyed by id: an atomic add for the count, an atomic min over (position << 32 | the hit word's high half)
// for the first hit -- neither depends on the order the lanes arrive in.  MAP_WAVE_IDS distinct ids fit, in twice as many slots: a lane
// that meets an empty slot draws a number from the id counter before it claims the slot, and with a number of MAP_WAVE_IDS or more it
// raises t.over instead.  So never more than MAP_WAVE_IDS slots are taken, every probe ends at an empty or an equal slot, and a read with
// more ids than that always raises t.over.  (Two lanes that bring the same new id at once both draw; the loser gives its number back.  At
// exactly MAP_WAVE_IDS ids that can raise t.over too, which costs time and changes no answer.)
// A read with t.over raised is done again from its row in passes: pass (P, p) takes the ids with id % P == p, P = 2, 4, ...
// MAP_WAVE_CLASSES, until every class fits; the sums and the winner are the same whatever P is.  Contig ids are the contigs' numbers, so
// a read of n ids needs P ~ n / MAP_WAVE_IDS.  Ids that agree in their low bits can defeat every P: then the wave runs the reference's
// own scan over the row, the lanes sharing each inner loop.  That bounds a read's work: 2 * MAP_WAVE_CLASSES passes of nk / 64 row loads
// a lane, then nk^2 / 32.  There is no workgroup barrier: the four waves of a workgroup share nothing.
constexpr int MAP_WAVE_IDS = 128;                 // 256 slots x 16 B + 8 B = 4 104 B a wave, 16 416 B a workgroup: 8 workgroups (32 waves,
constexpr int MAP_WAVE_SLOTS = 2 * MAP_WAVE_IDS;  // the most a CU holds) take 128.25 of the CU's 160 KiB; twice the ids would leave 16 waves
constexpr int MAP_WAVES = 4;                      // reads of a 256-thread workgroup
constexpr int MAP_WAVE_CLASSES = 64;              // the most id classes the passes try before the scan

struct MapWaveTable {
    uint32_t id[MAP_WAVE_SLOTS];
    uint32_t cnt[MAP_WAVE_SLOTS];
    unsigned long long first[MAP_WAVE_SLOTS];     // k-mer index << 32 | hit word >> 32 of the id's first hit
    uint32_t n_ids, over;
};

// the phases of one wave's LDS work are ordered by the wave's own instruction order; this keeps the compiler from moving LDS accesses
// across a phase's end
__device__ __forceinline__ void map_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void map_wave_clear(MapWaveTable& t, int lane) {
    for (int q = lane; q < MAP_WAVE_SLOTS; q += 64) { t.id[q] = 0; t.cnt[q] = 0; t.first[q] = ~0ull; }
    if (lane == 0) { t.n_ids = 0; t.over = 0; }
    map_wave_sync();
}

// one hit of k-mer j.  A new id that draws a number past the table's capacity raises t.over instead (the read is then done in passes)
__device__ __forceinline__ void map_wave_put(MapWaveTable& t, uint64_t hit, int j) {
    const uint32_t c = (uint32_t)hit;
    uint32_t e = (c * 2654435761u) >> 16 & (MAP_WAVE_SLOTS - 1);
    bool drawn = false, placed = false;
    for (;;) {
        uint32_t cur = __hip_atomic_load(&t.id[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) {
            if (!drawn) {
                if (atomicAdd(&t.n_ids, 1u) >= (uint32_t)MAP_WAVE_IDS) {
                    __hip_atomic_store(&t.over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    return;
                }
                drawn = true;
            }
            cur = atomicCAS(&t.id[e], 0u, c);
            if (cur == 0) { placed = true; cur = c; }
        }
        if (cur == c) break;
        e = (e + 1) & (MAP_WAVE_SLOTS - 1);        // another id's slot
    }
    if (drawn && !placed) atomicSub(&t.n_ids, 1u); // another lane brought the same id first
    atomicAdd(&t.cnt[e], 1u);
    atomicMin(&t.first[e], (unsigned long long)(uint32_t)j << 32 | (hit >> 32));
}

struct MapWaveSum {
    int counter, counter2;
    unsigned long long key;                        // count << 32 | ~first index: the largest is the winner
    uint32_t id, hi;                               // the winner's hit word
};

// this lane's share of the table into s
__device__ __forceinline__ void map_wave_collect(const MapWaveTable& t, int lane, int K, int multi, MapWaveSum& s) {
    for (int q = lane; q < MAP_WAVE_SLOTS; q += 64) {
        if (!t.id[q]) continue;
        const uint32_t flag = t.cnt[q];
        const unsigned long long f = t.first[q];
        if ((K < 32 && flag >= 2) || K > 32) s.counter2++;
        if ((int)flag < multi) continue;
        s.counter++;
        const unsigned long long key = (unsigned long long)flag << 32 | (0xFFFFFFFFu - (uint32_t)(f >> 32));
        if (key > s.key) { s.key = key; s.id = t.id[q]; s.hi = (uint32_t)f; }
    }
}

// The decision half of the wave-per-read kernels: the read's ids are in the wave's table t (or t.over is raised) and its hit words in
// row; the sums over the table, the passes and the scan of a read whose ids did not fit, the wave's butterfly, and out[r] from lane 0
__device__ __forceinline__ void map_wave_decide(MapWaveTable& t, const uint64_t* row, int nk, int lane, int K, int multi, const MapCtgs& ctgs,
                                                MapOut* out_r, unsigned long long* __restrict__ stats) {
    MapWaveSum s{0, 0, 0ull, 0u, 0u};
    uint32_t n_ids = t.n_ids;
    const bool over = t.over != 0;
    if (!over) map_wave_collect(t, lane, K, multi, s);
    else {
        __threadfence_block();                     // the row is read back by other lanes than those that wrote it
        uint32_t P = 1;
        bool again = true;
        while (again && P < (uint32_t)MAP_WAVE_CLASSES) {
            P <<= 1;
            again = false;
            s = MapWaveSum{0, 0, 0ull, 0u, 0u};
            n_ids = 0;
            for (uint32_t p = 0; p < P; p++) {
                map_wave_sync();
                map_wave_clear(t, lane);
                for (int j = lane; j < nk; j += 64) {
                    const uint64_t hit = row[j];
                    if ((uint32_t)hit && ((uint32_t)hit & (P - 1)) == p) map_wave_put(t, hit, j);
                }
                map_wave_sync();
                if (t.over) { again = true; break; }
                n_ids += t.n_ids;
                map_wave_collect(t, lane, K, multi, s);
            }
        }
        if (again) {                               // no P gave classes that fit: the reference's scan (:282-326), a wave wide
            s = MapWaveSum{0, 0, 0ull, 0u, 0u};
            n_ids = 0;
            for (int j = 0; j < nk; j++) {
                const uint64_t h = row[j];
                const uint32_t c = (uint32_t)h;
                if (!c) continue;
                bool seen = false;
                for (int i0 = 0; i0 < j && !seen; i0 += 64) seen = __any(i0 + lane < j && (uint32_t)row[i0 + lane] == c) != 0;
                if (seen) continue;
                int flag = 0;
                for (int q = j + 1 + lane; q < nk; q += 64) flag += (uint32_t)row[q] == c ? 1 : 0;
                for (int d = 32; d > 0; d >>= 1) flag += __shfl_xor(flag, d);
                flag++;
                n_ids++;
                if (lane) continue;                // lane 0 keeps the sums; the other lanes add nothing below
                if ((K < 32 && flag >= 2) || K > 32) s.counter2++;
                if (flag < multi) continue;
                s.counter++;
                const unsigned long long key = (unsigned long long)(uint32_t)flag << 32 | (0xFFFFFFFFu - (uint32_t)j);
                if (key > s.key) { s.key = key; s.id = c; s.hi = (uint32_t)(h >> 32); }
            }
        }
    }
    // the wave's sums
    for (int d = 32; d > 0; d >>= 1) {
        const int c1 = __shfl_xor(s.counter, d), c2 = __shfl_xor(s.counter2, d);
        const unsigned long long key = __shfl_xor(s.key, d);
        const uint32_t id = __shfl_xor(s.id, d), hi = __shfl_xor(s.hi, d);
        s.counter += c1;
        s.counter2 += c2;
        if (key > s.key) { s.key = key; s.id = id; s.hi = hi; }
    }
    if (lane == 0) {
        *out_r = s.counter ? map_place((uint64_t)s.id | (uint64_t)s.hi << 32, (int)(0xFFFFFFFFu - (uint32_t)s.key), K, s.counter2, ctgs)
                           : MapOut{0, 0, 0, 0};
        if (stats) {                               // the measurement's figures: reads done in passes, distinct ids
            if (over) atomicAdd(stats, 1ull);
            atomicAdd(stats + 1, (unsigned long long)n_ids);
        }
    }
}

// the wave's prologue: its read, or false when the wave has nothing to decide (no read; a read without k-mers: out[r] is written here)
__device__ __forceinline__ bool map_wave_read(const int32_t* __restrict__ lens, uint64_t n, int K, int lane, int wave, MapOut* __restrict__ out,
                                              uint64_t& r, int& len, int& nk) {
    r = (uint64_t)blockIdx.x * MAP_WAVES + wave;
    if (r >= n) return false;                      // (no workgroup barrier follows)
    len = lens[r];
    nk = map_read_kmers(len, K);
    if (!nk && lane == 0) out[r] = MapOut{0, 0, 0, 0};
    return nk != 0;
}

template <int NW>
__global__ __launch_bounds__(256) void map_read_wave_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                            const int32_t* __restrict__ lens, const uint64_t* __restrict__ koff, uint64_t n,
                                                            int K, int align_len, const uint64_t* __restrict__ tab, uint64_t mask,
                                                            MapCtgs ctgs, uint64_t* rows, MapOut* __restrict__ out,
                                                            unsigned long long* __restrict__ stats) {
    __shared__ MapWaveTable tables[MAP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t r;
    int len, nk;
    if (!map_wave_read(lens, n, K, lane, wave, out, r, len, nk)) return;
    MapWaveTable& t = tables[wave];
    uint64_t* row = rows + koff[r];
    map_wave_clear(t, lane);
    {   // the lookups: a lane rolls through its stretch of the read; every hit goes to the row and to the table
        const int per = (nk + 63) / 64;
        const int j0 = lane * per, j1 = nk < j0 + per ? nk : j0 + per;
        map_stretch<NW>(words + off[r], j0, j1, K, tab, mask, row, [&t](uint64_t hit, int j) {
            if ((uint32_t)hit) map_wave_put(t, hit, j);
        });
    }
    map_wave_sync();
    map_wave_decide(t, row, nk, lane, K, map_multi(len, align_len, K), ctgs, out + r, stats);
}

// the wave-per-read decision alone, from rows that are finished (the sharded engine: merged on the lead): the lanes bring the row's hits
// to the table, then as above
__global__ __launch_bounds__(256) void map_decide_rows_wave_kernel(const int32_t* __restrict__ lens, const uint64_t* __restrict__ koff, uint64_t n,
                                                                   int K, int align_len, MapCtgs ctgs, const uint64_t* rows,
                                                                   MapOut* __restrict__ out, unsigned long long* __restrict__ stats) {
    __shared__ MapWaveTable tables[MAP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t r;
    int len, nk;
    if (!map_wave_read(lens, n, K, lane, wave, out, r, len, nk)) return;
    MapWaveTable& t = tables[wave];
    const uint64_t* row = rows + koff[r];
    map_wave_clear(t, lane);
    for (int j = lane; j < nk; j += 64) {
        const uint64_t hit = row[j];
        if ((uint32_t)hit) map_wave_put(t, hit, j);
    }
    map_wave_sync();
    map_wave_decide(t, row, nk, lane, K, map_multi(len, align_len, K), ctgs, out + r, stats);
}

namespace {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                                 // elements
    int reserve(size_t n) {
        if (n <= cap) return PG_OK;
        if (p) arena_free(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max(n, (size_t)1) + n / 4;
        if (arena_malloc(&p, want * sizeof(T)) != hipSuccess) { pg_set_error("map: device allocation failed"); return PG_ENOMEM; }
        cap = want;
        return PG_OK;
    }
    void release() { if (p) arena_free(p); p = nullptr; cap = 0; }
};

// f(std::integral_constant<int, NW>) for an engine's flavour: a kernel's argument list is written once
template <typename F>
void map_with_nw(int nw, F f) {
    if (nw == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

// the index build's work items: (contig, first k-mer) stretches of MAP_ITEM k-mers
void map_index_items(const MapContigs& c, int K, std::vector<uint32_t>& item_c, std::vector<uint32_t>& item_j) {
    for (size_t i = 0; i < c.len.size(); i++)
        for (int j = 0; j < c.len[i] - K + 1; j += MAP_ITEM) { item_c.push_back((uint32_t)i); item_j.push_back((uint32_t)j); }
}

int map_check_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { pg_set_error("map: no HIP device"); return PG_ENODEV; }
    if (dev < 0 || dev >= n) { pg_set_error("map: HIP device " + std::to_string(dev) + " does not exist"); return PG_ENODEV; }
    return PG_OK;
}

class DeviceMapEngine : public MapEngine {
public:
    DeviceMapEngine(int device, int K, int nw) : dev_(device), K_(K), nw_(nw) {}
    ~DeviceMapEngine() override {
        if (!ready_) return;
        (void)hipSetDevice(dev_);
        tab_.release(); flag_.release(); len_.release(); bal_.release(); rwords_.release(); roff_.release(); rlen_.release(); rkoff_.release();
        rows_.release(); out_.release(); stats_.release();
        if (st_) (void)hipStreamDestroy(st_);
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
        arena_unpin(dev_);
    }
    int begin() {
        if (int rc = map_check_device(dev_)) return rc;
        MAP_HIP(hipSetDevice(dev_));
        arena_pin(dev_);
        ready_ = true;
        MAP_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
        MAP_HIP(hipEventCreate(&e0_));
        MAP_HIP(hipEventCreate(&e1_));
        return PG_OK;
    }
    int build(const MapContigs& c, const int32_t* ctg_len, const int8_t* bal, uint32_t n_ids) override {
        MAP_HIP(hipSetDevice(dev_));
        const size_t n_ctg = c.len.size();
        int rc;
        if ((rc = len_.reserve(n_ids)) || (rc = bal_.reserve(n_ids))) return rc;
        if (n_ids) {
            MAP_HIP(hipMemcpyAsync(len_.p, ctg_len, n_ids * sizeof(int32_t), hipMemcpyHostToDevice, st_));
            MAP_HIP(hipMemcpyAsync(bal_.p, bal, n_ids * sizeof(int8_t), hipMemcpyHostToDevice, st_));
        }
        ctgs_ = MapCtgs{len_.p, bal_.p, n_ids};
        slots_ = map_table_slots(c.n_kmers);
        const int SW = nw_ + 2;
        if ((rc = tab_.reserve(slots_ * SW)) || (rc = flag_.reserve(1))) return rc;
        // the contigs go through the read buffers; the work items are (contig, first k-mer) stretches of MAP_ITEM k-mers
        std::vector<uint32_t> item_c, item_j;
        map_index_items(c, K_, item_c, item_j);
        const uint64_t n_items = item_c.size();
        DevBuf<uint32_t> d_ic, d_ij, d_id;
        DevBuf<uint64_t> d_w, d_off;
        DevBuf<int32_t> d_len;
        if ((rc = d_ic.reserve(n_items)) || (rc = d_ij.reserve(n_items)) || (rc = d_id.reserve(n_ctg)) || (rc = d_w.reserve(c.words.size())) ||
            (rc = d_off.reserve(n_ctg + 1)) || (rc = d_len.reserve(n_ctg))) return rc;
        MAP_HIP(hipEventRecord(e0_, st_));
        MAP_HIP(hipMemsetAsync(tab_.p, 0, slots_ * SW * sizeof(uint64_t), st_));
        MAP_HIP(hipMemsetAsync(flag_.p, 0, sizeof(uint32_t), st_));
        if (n_items) {
            MAP_HIP(hipMemcpyAsync(d_ic.p, item_c.data(), n_items * 4, hipMemcpyHostToDevice, st_));
            MAP_HIP(hipMemcpyAsync(d_ij.p, item_j.data(), n_items * 4, hipMemcpyHostToDevice, st_));
            MAP_HIP(hipMemcpyAsync(d_id.p, c.id.data(), n_ctg * 4, hipMemcpyHostToDevice, st_));
            MAP_HIP(hipMemcpyAsync(d_w.p, c.words.data(), c.words.size() * 8, hipMemcpyHostToDevice, st_));
            MAP_HIP(hipMemcpyAsync(d_off.p, c.off.data(), (n_ctg + 1) * 8, hipMemcpyHostToDevice, st_));
            MAP_HIP(hipMemcpyAsync(d_len.p, c.len.data(), n_ctg * 4, hipMemcpyHostToDevice, st_));
            const dim3 grid((unsigned)((n_items + 255) / 256)), block(256);
            with_nw([&](auto nw) {
                hipLaunchKernelGGL((map_index_kernel<decltype(nw)::value>), grid, block, 0, st_, d_w.p, d_off.p, d_len.p, d_id.p, d_ic.p, d_ij.p,
                                   n_items, K_, tab_.p, slots_ - 1, flag_.p);
            });
            MAP_HIP(hipGetLastError());
        }
        MAP_HIP(hipEventRecord(e1_, st_));
        uint32_t gave_up = 0;
        MAP_HIP(hipMemcpyAsync(&gave_up, flag_.p, sizeof gave_up, hipMemcpyDeviceToHost, st_));
        MAP_HIP(hipStreamSynchronize(st_));
        float ms = 0;
        MAP_HIP(hipEventElapsedTime(&ms, e0_, e1_));
        t_index += ms * 1e-3;
        d_ic.release(); d_ij.release(); d_id.release(); d_w.release(); d_off.release(); d_len.release();
        if (gave_up) {
            pg_set_error("map: the index build gave up on a claimed slot after " + std::to_string(MAP_SPIN_CAP) +
                         " trips (the slot's key was never published); the index is not complete");
            return PG_ESPIN;
        }
        return PG_OK;
    }
    int map(const MapBatch& b, int align_len, MapOut* out, uint64_t* rows_out, bool wave) override {
        if (!b.n) return PG_OK;
        MAP_HIP(hipSetDevice(dev_));
        int rc;
        const uint64_t n_k = b.kmer_off[b.n];
        if (wave && (rc = stats_.reserve(2))) return rc;
        if ((rc = rwords_.reserve(b.n_words)) || (rc = roff_.reserve(b.n)) || (rc = rlen_.reserve(b.n)) || (rc = rkoff_.reserve(b.n + 1)) ||
            (rc = rows_.reserve(std::max<uint64_t>(n_k, 1))) || (rc = out_.reserve(b.n))) return rc;
        const double c0 = now_s();
        MAP_HIP(hipMemcpyAsync(rwords_.p, b.words, b.n_words * 8, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipMemcpyAsync(roff_.p, b.off, b.n * 8, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipMemcpyAsync(rlen_.p, b.len, b.n * 4, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipMemcpyAsync(rkoff_.p, b.kmer_off, (b.n + 1) * 8, hipMemcpyHostToDevice, st_));
        if (wave) MAP_HIP(hipMemsetAsync(stats_.p, 0, 2 * sizeof(unsigned long long), st_));
        MAP_HIP(hipEventRecord(e0_, st_));
        const dim3 grid((unsigned)(wave ? (b.n + MAP_WAVES - 1) / MAP_WAVES : (b.n + 255) / 256)), block(256);
        with_nw([&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            if (wave) hipLaunchKernelGGL((map_read_wave_kernel<NW>), grid, block, 0, st_, rwords_.p, roff_.p, rlen_.p, rkoff_.p, b.n, K_, align_len,
                                         tab_.p, slots_ - 1, ctgs_, rows_.p, out_.p, stats_.p);
            else hipLaunchKernelGGL((map_read_kernel<NW>), grid, block, 0, st_, rwords_.p, roff_.p, rlen_.p, rkoff_.p, b.n, K_, align_len, tab_.p,
                                    slots_ - 1, ctgs_, rows_.p, out_.p);
        });
        MAP_HIP(hipGetLastError());
        MAP_HIP(hipEventRecord(e1_, st_));
        MAP_HIP(hipMemcpyAsync(out, out_.p, b.n * sizeof(MapOut), hipMemcpyDeviceToHost, st_));
        if (rows_out && n_k) MAP_HIP(hipMemcpyAsync(rows_out, rows_.p, n_k * sizeof(uint64_t), hipMemcpyDeviceToHost, st_));
        unsigned long long stats[2] = {0, 0};
        if (wave) MAP_HIP(hipMemcpyAsync(stats, stats_.p, sizeof stats, hipMemcpyDeviceToHost, st_));
        MAP_HIP(hipStreamSynchronize(st_));
        n_passes += stats[0];
        n_ids += stats[1];
        float ms = 0;
        MAP_HIP(hipEventElapsedTime(&ms, e0_, e1_));
        t_kernel += ms * 1e-3;
        t_copy += now_s() - c0 - ms * 1e-3;
        return PG_OK;
    }

private:
    template <typename F> void with_nw(F f) const { map_with_nw(nw_, f); }
    int dev_, K_, nw_;
    bool ready_ = false;
    hipStream_t st_ = nullptr;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
    uint64_t slots_ = 0;
    MapCtgs ctgs_{nullptr, nullptr, 0};
    DevBuf<uint64_t> tab_, rwords_, roff_, rkoff_, rows_;
    DevBuf<uint32_t> flag_;                         // raised by a lane of the index build that gave up on a claimed slot
    DevBuf<int32_t> len_, rlen_;
    DevBuf<int8_t> bal_;
    DevBuf<MapOut> out_;
    DevBuf<unsigned long long> stats_;              // the wave kernel's two figures
};

// The index cut over n ranks by map_owner (map_index.hpp), for a contig set whose one table does not fit a card.  One process, one host
// thread; rank i is (devices[i], a stream of its own), rank 0 the lead, and an ordinal may repeat (several ranks on one GPU: how this is
// tested).  Ranks on more than one physical GPU have never run.
//   build   every rank receives the packed contigs and counts the keys it owns (map_count_owned_kernel); its table is made for exactly
//           that many (arena_malloc, no headroom), zeroed, and filled by map_index_owned_kernel.  A rank without keys launches nothing
//           and keeps a table of the smallest size, zeroed.  Any rank's spin flag fails the build
//   map     every rank receives the batch's reads, zeroes its row buffer and probes the keys it owns (map_probe_owned_kernel).  The lead
//           waits for each other rank's event (hipStreamWaitEvent), copies its rows into the staging buffer (hipMemcpyPeerAsync across
//           devices, hipMemcpyAsync on its own) and ORs them in (map_rows_merge_kernel): all on the lead's stream, so one staging buffer
//           serves every rank.  The decision runs on the lead from the finished rows (map_decide_rows_kernel / _wave_kernel).  The host
//           waits once a batch, for the lead's stream; there is no spin loop and no atomic across ranks
class ShardedDeviceMapEngine : public MapEngine {
public:
    ShardedDeviceMapEngine(const int* devices, int n, int K, int nw) : K_(K), nw_(nw), rk_((size_t)n) {
        for (int i = 0; i < n; i++) rk_[(size_t)i].dev = devices[i];
        ranks.resize((size_t)n);
    }
    ~ShardedDeviceMapEngine() override {
        for (R& r : rk_) {
            if (!r.pinned) continue;
            (void)hipSetDevice(r.dev);
            if (r.st) (void)hipStreamSynchronize(r.st);
            if (r.tab) arena_free(r.tab);
            r.flag.release(); r.count.release(); r.rwords.release(); r.roff.release(); r.rlen.release(); r.rkoff.release(); r.rows.release();
            if (&r == &rk_[0]) { len_.release(); bal_.release(); staging_.release(); out_.release(); stats_.release(); }
            if (r.st) (void)hipStreamDestroy(r.st);
            for (hipEvent_t e : {r.e0, r.e1, r.e2, r.e3, r.e4}) if (e) (void)hipEventDestroy(e);
            arena_unpin(r.dev);
        }
    }
    int begin() {
        for (R& r : rk_) {
            if (int rc = map_check_device(r.dev)) return rc;
            MAP_HIP(hipSetDevice(r.dev));
            arena_pin(r.dev);
            r.pinned = true;
            MAP_HIP(hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking));
            for (hipEvent_t* e : {&r.e0, &r.e1, &r.e2, &r.e3, &r.e4}) MAP_HIP(hipEventCreate(e));
        }
        return PG_OK;
    }
    int build(const MapContigs& c, const int32_t* ctg_len, const int8_t* bal, uint32_t n_ids) override {
        const size_t n = rk_.size();
        std::vector<uint32_t> item_c, item_j;
        map_index_items(c, K_, item_c, item_j);
        std::vector<Ctg> ctg(n);
        std::vector<unsigned long long> share(n, 0);
        std::vector<uint32_t> gave_up(n, 0);
        const int rc = build_ranks(c, ctg_len, bal, n_ids, item_c, item_j, ctg, share, gave_up);
        // However it ended: a failure on one rank leaves the others' streams copying out of the vectors above and the caller's arrays and
        // into share / gave_up, so every stream is waited for before they go, and the ranks' copies of the contigs are given back
        if (rc) sync_all();
        for (size_t i = 0; i < n; i++) {
            (void)hipSetDevice(rk_[i].dev);
            ctg[i].release();
        }
        return rc;
    }
    int map(const MapBatch& b, int align_len, MapOut* out, uint64_t* rows_out, bool wave) override {
        if (!b.n) return PG_OK;
        const int rc = map_ranks(b, align_len, out, rows_out, wave);
        if (rc) sync_all();                         // no stream is left reading the caller's batch or writing its results
        return rc;
    }

private:
    void sync_all() {
        for (R& r : rk_) {
            (void)hipSetDevice(r.dev);
            if (r.st) (void)hipStreamSynchronize(r.st);
        }
    }
    int map_ranks(const MapBatch& b, int align_len, MapOut* out, uint64_t* rows_out, bool wave) {
        const uint32_t n = (uint32_t)rk_.size();
        const uint64_t n_k = b.kmer_off[b.n];
        R& lead = rk_[0];
        int rc;
        const double c0 = now_s();
        const dim3 block(256);
        const dim3 grid_reads((unsigned)(wave ? (b.n + MAP_WAVES - 1) / MAP_WAVES : (b.n + 255) / 256));
        // 1. every rank: the reads, a zeroed row buffer, its lookups
        for (uint32_t i = 0; i < n; i++) {
            R& r = rk_[i];
            MAP_HIP(hipSetDevice(r.dev));
            if ((rc = r.rwords.reserve(b.n_words)) || (rc = r.roff.reserve(b.n)) || (rc = r.rlen.reserve(b.n)) || (rc = r.rkoff.reserve(b.n + 1)) ||
                (rc = r.rows.reserve(std::max<uint64_t>(n_k, 1)))) return rc;
            MAP_HIP(hipMemcpyAsync(r.rwords.p, b.words, b.n_words * 8, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(r.roff.p, b.off, b.n * 8, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(r.rlen.p, b.len, b.n * 4, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(r.rkoff.p, b.kmer_off, (b.n + 1) * 8, hipMemcpyHostToDevice, r.st));
            if (n_k) MAP_HIP(hipMemsetAsync(r.rows.p, 0, n_k * sizeof(uint64_t), r.st));
            MAP_HIP(hipEventRecord(r.e0, r.st));
            map_with_nw(nw_, [&](auto nw) {
                constexpr int NW = decltype(nw)::value;
                if (wave) hipLaunchKernelGGL((map_probe_owned_kernel<NW, true>), grid_reads, block, 0, r.st, r.rwords.p, r.roff.p, r.rlen.p, r.rkoff.p,
                                             b.n, K_, n, i, r.tab, r.slots - 1, r.rows.p);
                else hipLaunchKernelGGL((map_probe_owned_kernel<NW, false>), grid_reads, block, 0, r.st, r.rwords.p, r.roff.p, r.rlen.p, r.rkoff.p,
                                        b.n, K_, n, i, r.tab, r.slots - 1, r.rows.p);
            });
            MAP_HIP(hipGetLastError());
            MAP_HIP(hipEventRecord(r.e1, r.st));
        }
        // 2. the lead: the other ranks' rows, one after the other through the staging buffer
        MAP_HIP(hipSetDevice(lead.dev));
        if ((rc = out_.reserve(b.n)) || (n > 1 && n_k && (rc = staging_.reserve(n_k))) || (wave && (rc = stats_.reserve(2)))) return rc;
        // the lead's stream goes behind every other rank's probe, k-mers or none: the host's one wait below then covers every rank's
        // events and its copies out of the caller's batch.  e4 marks where the waiting ends, so that t_merge is the copies and the OR alone
        for (uint32_t i = 1; i < n; i++) MAP_HIP(hipStreamWaitEvent(lead.st, rk_[i].e1, 0));
        MAP_HIP(hipEventRecord(lead.e4, lead.st));
        for (uint32_t i = 1; i < n && n_k; i++) {
            R& r = rk_[i];
            if (r.dev == lead.dev) MAP_HIP(hipMemcpyAsync(staging_.p, r.rows.p, n_k * sizeof(uint64_t), hipMemcpyDeviceToDevice, lead.st));
            else MAP_HIP(hipMemcpyPeerAsync(staging_.p, lead.dev, r.rows.p, r.dev, n_k * sizeof(uint64_t), lead.st));
            if ((rc = map_rows_merge(lead.rows.p, staging_.p, n_k, lead.st))) return rc;
        }
        MAP_HIP(hipEventRecord(lead.e2, lead.st));
        // 3. the decision, from the finished rows
        if (wave) {
            MAP_HIP(hipMemsetAsync(stats_.p, 0, 2 * sizeof(unsigned long long), lead.st));
            hipLaunchKernelGGL(map_decide_rows_wave_kernel, grid_reads, block, 0, lead.st, lead.rlen.p, lead.rkoff.p, b.n, K_, align_len, ctgs_,
                               lead.rows.p, out_.p, stats_.p);
        } else
            hipLaunchKernelGGL(map_decide_rows_kernel, grid_reads, block, 0, lead.st, lead.rlen.p, lead.rkoff.p, b.n, K_, align_len, ctgs_,
                               lead.rows.p, out_.p);
        MAP_HIP(hipGetLastError());
        MAP_HIP(hipEventRecord(lead.e3, lead.st));
        MAP_HIP(hipMemcpyAsync(out, out_.p, b.n * sizeof(MapOut), hipMemcpyDeviceToHost, lead.st));
        if (rows_out && n_k) MAP_HIP(hipMemcpyAsync(rows_out, lead.rows.p, n_k * sizeof(uint64_t), hipMemcpyDeviceToHost, lead.st));
        unsigned long long stats[2] = {0, 0};
        if (wave) MAP_HIP(hipMemcpyAsync(stats, stats_.p, sizeof stats, hipMemcpyDeviceToHost, lead.st));
        // the batch's one wait: the lead's stream is behind every other rank's e1
        MAP_HIP(hipStreamSynchronize(lead.st));
        n_passes += stats[0];
        n_ids += stats[1];
        float ms = 0, all = 0;
        for (uint32_t i = 0; i < n; i++) {
            MAP_HIP(hipEventElapsedTime(&ms, rk_[i].e0, rk_[i].e1));
            ranks[i].t_probe += ms * 1e-3;
        }
        MAP_HIP(hipEventElapsedTime(&ms, lead.e4, lead.e2));
        t_merge += ms * 1e-3;
        MAP_HIP(hipEventElapsedTime(&ms, lead.e2, lead.e3));
        t_decide += ms * 1e-3;
        MAP_HIP(hipEventElapsedTime(&all, lead.e0, lead.e3));
        t_kernel += all * 1e-3;
        t_copy += now_s() - c0 - all * 1e-3;
        return PG_OK;
    }
    struct Ctg {                                    // a rank's copy of the contigs, alive while its table is built
        DevBuf<uint32_t> ic, ij, id;
        DevBuf<uint64_t> w, off;
        DevBuf<int32_t> len;
        void release() { ic.release(); ij.release(); id.release(); w.release(); off.release(); len.release(); }
    };
    // build()'s work; build() owns what the ranks' streams read and write meanwhile, and cleans up after every way out of here
    int build_ranks(const MapContigs& c, const int32_t* ctg_len, const int8_t* bal, uint32_t n_ids, const std::vector<uint32_t>& item_c,
                    const std::vector<uint32_t>& item_j, std::vector<Ctg>& ctg, std::vector<unsigned long long>& share,
                    std::vector<uint32_t>& gave_up) {
        const uint32_t n = (uint32_t)rk_.size();
        const size_t n_ctg = c.len.size();
        const int SW = nw_ + 2;
        int rc;
        R& lead = rk_[0];
        MAP_HIP(hipSetDevice(lead.dev));
        if ((rc = len_.reserve(n_ids)) || (rc = bal_.reserve(n_ids))) return rc;
        if (n_ids) {
            MAP_HIP(hipMemcpyAsync(len_.p, ctg_len, n_ids * sizeof(int32_t), hipMemcpyHostToDevice, lead.st));
            MAP_HIP(hipMemcpyAsync(bal_.p, bal, n_ids * sizeof(int8_t), hipMemcpyHostToDevice, lead.st));
        }
        ctgs_ = MapCtgs{len_.p, bal_.p, n_ids};
        const uint64_t n_items = item_c.size();
        const dim3 grid((unsigned)((n_items + 255) / 256)), block(256);
        // 1. the contigs to every rank, and its count
        for (uint32_t i = 0; i < n; i++) {
            R& r = rk_[i];
            Ctg& g = ctg[i];
            MAP_HIP(hipSetDevice(r.dev));
            if ((rc = r.flag.reserve(1)) || (rc = r.count.reserve(1))) return rc;
            MAP_HIP(hipEventRecord(r.e0, r.st));
            MAP_HIP(hipMemsetAsync(r.flag.p, 0, sizeof(uint32_t), r.st));
            MAP_HIP(hipMemsetAsync(r.count.p, 0, sizeof(unsigned long long), r.st));
            if (!n_items) continue;
            if ((rc = g.ic.reserve(n_items)) || (rc = g.ij.reserve(n_items)) || (rc = g.id.reserve(n_ctg)) || (rc = g.w.reserve(c.words.size())) ||
                (rc = g.off.reserve(n_ctg + 1)) || (rc = g.len.reserve(n_ctg))) return rc;
            MAP_HIP(hipMemcpyAsync(g.ic.p, item_c.data(), n_items * 4, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(g.ij.p, item_j.data(), n_items * 4, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(g.id.p, c.id.data(), n_ctg * 4, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(g.w.p, c.words.data(), c.words.size() * 8, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(g.off.p, c.off.data(), (n_ctg + 1) * 8, hipMemcpyHostToDevice, r.st));
            MAP_HIP(hipMemcpyAsync(g.len.p, c.len.data(), n_ctg * 4, hipMemcpyHostToDevice, r.st));
            map_with_nw(nw_, [&](auto nw) {
                hipLaunchKernelGGL((map_count_owned_kernel<decltype(nw)::value>), grid, block, 0, r.st, g.w.p, g.off.p, g.len.p, g.id.p, g.ic.p,
                                   g.ij.p, n_items, K_, n, i, r.count.p);
            });
            MAP_HIP(hipGetLastError());
            MAP_HIP(hipMemcpyAsync(&share[i], r.count.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, r.st));
        }
        // 2. a table of exactly that share, and the keys
        for (uint32_t i = 0; i < n; i++) {
            R& r = rk_[i];
            Ctg& g = ctg[i];
            MAP_HIP(hipSetDevice(r.dev));
            MAP_HIP(hipStreamSynchronize(r.st));
            r.slots = map_table_slots(share[i]);
            ranks[i].keys = share[i];
            ranks[i].slots = r.slots;
            if (r.tab) arena_free(r.tab);
            r.tab = nullptr;
            if (arena_malloc(&r.tab, r.slots * SW * sizeof(uint64_t)) != hipSuccess) {
                pg_set_error("map: device allocation failed (rank " + std::to_string(i) + ": a table of " + std::to_string(r.slots) + " slots)");
                return PG_ENOMEM;
            }
            MAP_HIP(hipMemsetAsync(r.tab, 0, r.slots * SW * sizeof(uint64_t), r.st));
            if (share[i]) {                         // (a rank that owns nothing launches nothing)
                map_with_nw(nw_, [&](auto nw) {
                    hipLaunchKernelGGL((map_index_owned_kernel<decltype(nw)::value>), grid, block, 0, r.st, g.w.p, g.off.p, g.len.p, g.id.p,
                                       g.ic.p, g.ij.p, n_items, K_, n, i, r.tab, r.slots - 1, r.flag.p);
                });
                MAP_HIP(hipGetLastError());
            }
            MAP_HIP(hipEventRecord(r.e1, r.st));
            MAP_HIP(hipMemcpyAsync(&gave_up[i], r.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, r.st));
        }
        uint64_t total = 0;
        double t_max = 0;
        bool spun = false;
        for (uint32_t i = 0; i < n; i++) {
            R& r = rk_[i];
            MAP_HIP(hipSetDevice(r.dev));
            MAP_HIP(hipStreamSynchronize(r.st));
            float ms = 0;
            MAP_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
            t_max = std::max(t_max, (double)ms * 1e-3);
            total += share[i];
            spun = spun || gave_up[i];
        }
        t_index += t_max;                           // (the ranks build side by side: the longest)
        if (spun) {
            pg_set_error("map: the index build gave up on a claimed slot after " + std::to_string(MAP_SPIN_CAP) +
                         " trips (the slot's key was never published); the index is not complete");
            return PG_ESPIN;
        }
        if (total != c.n_kmers) {
            pg_set_error("map: the ranks own " + std::to_string(total) + " keys of " + std::to_string(c.n_kmers));
            return PG_EINVAL;
        }
        return PG_OK;
    }
    struct R {                                      // a rank
        int dev = 0;
        bool pinned = false;
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr, e4 = nullptr;   // probe / build from e0 to e1; the lead: every rank's probe done at e4, merge to e2, decide to e3
        uint64_t* tab = nullptr;                    // exactly slots * (NW + 2) words
        uint64_t slots = 0;
        DevBuf<uint32_t> flag;                      // raised by a lane of the index build that gave up on a claimed slot
        DevBuf<unsigned long long> count;           // the keys it owns
        DevBuf<uint64_t> rwords, roff, rkoff, rows;
        DevBuf<int32_t> rlen;
    };
    int K_, nw_;
    std::vector<R> rk_;
    MapCtgs ctgs_{nullptr, nullptr, 0};
    // the lead's alone
    DevBuf<int32_t> len_;
    DevBuf<int8_t> bal_;
    DevBuf<uint64_t> staging_;
    DevBuf<MapOut> out_;
    DevBuf<unsigned long long> stats_;
};

}  // namespace

int map_wave_ids() { return MAP_WAVE_IDS; }

std::unique_ptr<MapEngine> map_engine_device(int device, int K, int nw) {
    std::unique_ptr<DeviceMapEngine> e(new DeviceMapEngine(device, K, nw));
    if (e->begin() != PG_OK) return nullptr;
    return std::unique_ptr<MapEngine>(e.release());
}

std::unique_ptr<MapEngine> map_engine_device_sharded(const int* devices, int n, int K, int nw) {
    if (!devices || n < 1 || n > DEVICE_LIST_MAX_RANKS) { pg_set_error("map: an index is cut over 1 to " + std::to_string(DEVICE_LIST_MAX_RANKS) + " ranks"); return nullptr; }
    std::unique_ptr<ShardedDeviceMapEngine> e(new ShardedDeviceMapEngine(devices, n, K, nw));
    if (e->begin() != PG_OK) return nullptr;
    return std::unique_ptr<MapEngine>(e.release());
}

int map_rows_merge(uint64_t* d_rows, const uint64_t* d_part, uint64_t n_words, void* stream) {
    if (!n_words) return PG_OK;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_words + 255) / 256, 65536);
    hipLaunchKernelGGL(map_rows_merge_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_rows, d_part, n_words);
    MAP_HIP(hipGetLastError());
    return PG_OK;
}

int map_device_free_bytes(int device, uint64_t* free_bytes) {
    if (int rc = map_check_device(device)) return rc;
    MAP_HIP(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    MAP_HIP(arena_mem_info(&free_b, &total_b));
    *free_bytes = free_b;
    return PG_OK;
}

}  // namespace pg
