// host_graph.cpp -- the graph stages after pass 1, host side: rebuild the reference's k-mer-set layout from the
// device's distinct k-mers, then tip clipping, edge construction, pass 2 (read threading, pre-arcs) and the writers.
//
// Why a layout replay: .vertex and .edge.gz are emitted by walking KmerSets[0..P-1] slot by slot
// (node2edge.c:383-406, output_pregraph.c:60-75) and tip clipping mutates nodes in that order
// (cutTipPreGraph.c:374-395,428-455), so the bytes of the outputs are a function of the slot every k-mer
// occupies.  A slot is decided by (key mod prime) + linear probing + the whole grow/rehash history
// (newhash.c:340-528), which depends only on the per-set sequence of distinct keys in first-occurrence
// order.  The device provides that order (first-occurrence ordinal per key, set id), this file replays it.
//
// Who does what:
//   layout replay     here, one thread per set (sequential by construction); records pulled from the device in chunks
//   tips              walks: graph_kernels.hip (or Graph::tip_walk on all host threads); the order-dependent clipping
//                     is replayed here in slot order (Graph::tip_scan)
//   edges             graph_kernels.hip (GraphHandle::dev_build_edges formats the text), or ParallelEdgeBuilder /
//                     EdgeBuilder on the host
//   pass 2            graph_kernels.hip (GraphHandle::dev_add_packed / dev_finish), or ReadThreader + PreArcs on the host
//   writers           .vertex / .preGraphBasic / .edge.gz / .preArc / .path / .markOnEdge
// The host forms exist for the CPU-only ABI (pg_host_*), the tests that need no GPU and A/B runs; the executable uses the
// device forms.  Templated on NW = words per k-mer (2 = 63-mer binary flavour, 4 = 127-mer flavour); no HIP in this file
// (the device stages sit behind graph_dev.hpp).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <zlib.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <queue>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "kmer.hpp"
#include "p2_walk.hpp"
#include "env.hpp"
#include "host_graph.hpp"
#include "graph_dev.hpp"
#include "backend.hpp"
#include "dev_tips.hpp"
#include "ref_sizes.hpp"
#include "dev_rehash.hpp"
#include "../../include/soapdenovo2_amd.h"

namespace pg {
// SOAPDENOVO2_AMD_TIPS=host: the tip stage on the host threads (the A/B twin of the device form; =replay: device walks, host decisions)
static bool tips_on_host() { const char* e = env_user("SOAPDENOVO2_AMD_TIPS"); return e && !strcmp(e, "host"); }

static uint32_t g_crc_tab[256];
static std::atomic<bool> g_crc_ready{false};
static thread_local int g_edge_file_in_background = 0;    // pg_host_edge_file_in_background: the calling thread's choice for the graphs it begins
// host threads for the parallel stages: the caller's count, else SOAPDENOVO2_AMD_HOST_THREADS, else every hardware thread
int host_threads(int n_threads);
static int pick_threads(int n_threads) { return host_threads(n_threads); }
int host_threads(int n_threads) {
    if (n_threads > 0) return n_threads;
    if (const char* e = pg::env_user("SOAPDENOVO2_AMD_HOST_THREADS")) { const int v = atoi(e); if (v > 0) return v; }
    static const int usable = []() {
        int hw = (int)std::thread::hardware_concurrency();
        if (hw < 1) hw = 1;
        // a container's CPU quota (cgroup v2 cpu.max "quota period", v1 cfs_quota_us / cfs_period_us): more runnable
        // threads than that only get throttled
        double quota = -1, period = 0;
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[64];
            if (fscanf(f, "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0) quota = atof(q);
            fclose(f);
        } else {
            FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r");
            FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
            if (fq && fp && fscanf(fq, "%lf", &quota) == 1 && fscanf(fp, "%lf", &period) == 1) {}
            if (fq) fclose(fq);
            if (fp) fclose(fp);
        }
        if (quota > 0 && period > 0) {
            const int cores = (int)((quota + period - 1) / period);
            if (cores >= 1 && cores < hw) hw = cores;
        }
        return hw;
    }();
    return usable;
}

// the same CRC eight bytes at a time (slicing-by-8 tables derived from the byte table)
static uint32_t g_crc8[8][256];
static std::atomic<bool> g_crc8_ready{false};
const uint32_t* host_crc_table();
static void host_crc8_init() {
    if (g_crc8_ready.load(std::memory_order_acquire)) return;
    const uint32_t* t0 = host_crc_table();
    uint32_t tmp[8][256];
    for (uint32_t i = 0; i < 256; i++) tmp[0][i] = t0[i];
    for (int k = 1; k < 8; k++)
        for (uint32_t i = 0; i < 256; i++) tmp[k][i] = (tmp[k - 1][i] >> 8) ^ t0[tmp[k - 1][i] & 0xff];
    static std::atomic_flag lock = ATOMIC_FLAG_INIT;
    while (lock.test_and_set(std::memory_order_acquire)) {}
    if (!g_crc8_ready.load(std::memory_order_relaxed)) {
        memcpy(g_crc8, tmp, sizeof(tmp));
        g_crc8_ready.store(true, std::memory_order_release);
    }
    lock.clear(std::memory_order_release);
}
template <int NW>
static inline uint32_t host_crc32(const Kmer<NW>& a) {
    uint32_t crc = 0;
    for (int i = 0; i < NW; i++) {
        const uint64_t v = a.w[i] ^ crc;
        crc = g_crc8[7][v & 0xff] ^ g_crc8[6][(v >> 8) & 0xff] ^ g_crc8[5][(v >> 16) & 0xff] ^ g_crc8[4][(v >> 24) & 0xff] ^
              g_crc8[3][(v >> 32) & 0xff] ^ g_crc8[2][(v >> 40) & 0xff] ^ g_crc8[1][(v >> 48) & 0xff] ^ g_crc8[0][v >> 56];
    }
    return crc ^ 0xffffffffu;
}

const uint32_t* host_crc_table() {
    if (!g_crc_ready.load(std::memory_order_acquire)) {
        for (uint32_t i = 0; i < 256; i++) g_crc_tab[i] = crc32_table_entry(i);
        g_crc_ready.store(true, std::memory_order_release);
    }
    return g_crc_tab;
}

// (the reference's size schedule: ref_sizes.hpp)
uint64_t ref_initial_set_size(int a_gb, int n_sets, int mer127) {     // prlHashReads.c:369-390 + init_kmerset
    uint64_t init = 1024;
    if (a_gb) {
        const uint64_t want = (uint64_t)((double)a_gb * 1024.0f * 1024.0f * 1024.0f / (double)n_sets / (mer127 ? 40 : 24));
        uint64_t k = 0;
        do { ++k; } while (k * 0xFFFFFFULL < want);
        init = k * 0xFFFFFFULL;
    }
    return init < 3 ? 3 : ref_next_prime(init);
}

template <int NW>
struct HNode {
    Kmer<NW> seq;
    uint32_t A, B;
};

// A big zero-filled array on 2 MiB-aligned anonymous memory with transparent huge pages requested: the k-mer sets are
// probed at random, and with 4 KiB pages nearly every probe also misses the TLB.
template <typename T>
struct HugeArray {
    T* p = nullptr;
    size_t n = 0, bytes = 0;
    HugeArray() {}
    HugeArray(const HugeArray&) = delete;
    HugeArray& operator=(const HugeArray&) = delete;
    HugeArray(HugeArray&& o) noexcept : p(o.p), n(o.n), bytes(o.bytes) { o.p = nullptr; o.n = o.bytes = 0; }
    HugeArray& operator=(HugeArray&& o) noexcept { release(); p = o.p; n = o.n; bytes = o.bytes; o.p = nullptr; o.n = o.bytes = 0; return *this; }
    ~HugeArray() { release(); }
    void release() { if (p) munmap(p, bytes); p = nullptr; n = bytes = 0; }
    // new zeroed storage of `count` elements; the first `keep` old elements are carried over
    void reset(size_t count, size_t keep = 0) {
        const size_t HP = (size_t)2 << 20;
        size_t nb = (count * sizeof(T) + HP - 1) / HP * HP;
        if (nb == 0) nb = HP;
        void* q = mmap(nullptr, nb + HP, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (q == MAP_FAILED) { fprintf(stderr, "out of memory (%zu bytes for a k-mer set)\n", nb); exit(1); }
        // trim to a 2 MiB boundary so that whole huge pages can back the range
        uintptr_t a = (uintptr_t)q, al = (a + HP - 1) / HP * HP;
        if (al > a) munmap(q, al - a);
        if (al + nb < a + nb + HP) munmap((void*)(al + nb), a + HP - al);
        // (huge pages make the host replay's random accesses cheaper where the kernel hands them out quickly; SOAPDENOVO2_AMD_THP=0 for hosts where it does not --
        //  the build container's VM takes 80 s to touch 2 GB in 2 MB pages and 8 s in 4 KB ones, and several threads touching at once are slower still)
        static const bool thp = [] { const char* v = pg::env_user("SOAPDENOVO2_AMD_THP"); return !(v && atoi(v) == 0) && !pg::env_measure("PG_NO_THP"); }();
        if (thp) madvise((void*)al, nb, MADV_HUGEPAGE);
        T* np = (T*)al;
        if (keep) memcpy((void*)np, (const void*)p, keep * sizeof(T));
        release();
        p = np; n = count; bytes = nb;
    }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
    T* data() { return p; }
    const T* data() const { return p; }
};

template <int NW>
struct HSet {
    HugeArray<HNode<NW>> array;
    std::vector<uint8_t> occ;
    // An empty slot carries a key no k-mer can have (K <= 63 / 127 leaves the two top bits of word 0 clear), so that a
    // lookup touches the slot array only; `occ` mirrors it for the in-order scans and the in-place rehash.
    static constexpr uint64_t EMPTY = ~0ULL;
    uint64_t size = 0, count = 0, max = 0;
    float lf = 0.77f;

    // home slot (modular, newhash.c:36-57): exact 128-bit modulus for NW = 2; the 127-mer build reduces the
    // key in 32-bit chunks, which is a true modulus only while size < 2^32 -- restated as is.
    // While size < 2^32 (always, short of ~3 G keys a set) every reduction is a Barrett step with the reciprocal kept
    // beside the size: a multiply-high, a multiply and two corrections instead of a division.  In the in-place rehash the
    // home of a kicked element sits on the critical path in front of a cache miss, and a 128-by-64 division has ~4x the
    // latency of this.
    uint64_t bar_m = 0, bar_c64 = 0;                               // floor(2^64 / size), 2^64 mod size
    void set_size(uint64_t sz) {
        size = sz;
        bar_m = sz > 1 ? (uint64_t)((((unsigned __int128)1) << 64) / sz) : 0;
        bar_c64 = sz > 1 ? (uint64_t)((((unsigned __int128)1) << 64) % sz) : 0;
    }
    uint64_t bred(uint64_t x) const {                              // x mod size, size < 2^32
        const uint64_t q = (uint64_t)(((unsigned __int128)x * bar_m) >> 64);
        uint64_t r = x - q * size;
        if (r >= size) r -= size;
        if (r >= size) r -= size;
        return r;
    }
    uint64_t home(const Kmer<NW>& k) const {
        if (size > 1 && size < (1ULL << 32)) {
            if (NW == 2) {                                            // (hi mod p) * (2^64 mod p) + (lo mod p), all below 2^64
                uint64_t r = bred(bred(k.w[0]) * bar_c64) + bred(k.w[1]);
                if (r >= size) r -= size;
                return r;
            }
            uint64_t t = bred(k.w[0]);
            for (int i = 1; i < NW; i++) {
                t = bred(t << 32 | (k.w[i] >> 32));
                t = bred(t << 32 | (k.w[i] & 0xffffffffULL));
            }
            return t;
        }
        if (NW == 2) {
#if defined(__x86_64__)
            // (hi * 2^64 + lo) % size as two 64-bit divisions (the generic 128-bit modulus is a slow library call)
            uint64_t hi = k.w[0] % size, q, r;
            __asm__("divq %4" : "=a"(q), "=d"(r) : "a"(k.w[1]), "d"(hi), "r"(size) : "cc");
            return r;
#else
            unsigned __int128 t = ((unsigned __int128)k.w[0] << 64) | k.w[1];
            return (uint64_t)(t % size);
#endif
        }
        uint64_t t = k.w[0] % size;
        for (int i = 1; i < NW; i++) {
            t = (t << 32 | (k.w[i] >> 32)) % size;
            t = (t << 32 | (k.w[i] & 0xffffffffULL)) % size;
        }
        return t;
    }
    // the size after `puts` growth tests starting from an empty set of `sz` slots (the schedule depends on counts only)
    static uint64_t final_size(uint64_t sz, uint64_t puts, bool static_pool) {
        if (static_pool) return sz;
        const float lf = 0.77f;
        uint64_t max = (uint64_t)((float)sz * lf);
        while (puts > max) {                                   // the put with count + 1 == max + 1 grows the set
            uint64_t n = sz;
            do {
                n = (n < 0xFFFFFFFULL) ? (n << 1) : (n + 0xFFFFFFULL);
                n = ref_next_prime(n);
            } while ((float)n * lf < (float)(max + 1));
            sz = n;
            max = (uint64_t)((float)sz * lf);
        }
        return sz;
    }
    // `capacity` slots are reserved up front (untouched pages cost nothing) so that growing never has to move the array
    void init(uint64_t sz, uint64_t capacity = 0) {
        set_size(sz); count = 0; lf = 0.77f;
        max = (uint64_t)((float)size * lf);
        array.reset(std::max(size, capacity));
        for (uint64_t i = 0; i < size; i++) array[i].seq.w[0] = EMPTY;
        occ.assign(size, 0);
    }
    // storage for a layout made elsewhere (the device's K6 layout is downloaded into it): `sz` slots, `n` of them occupied
    void adopt(uint64_t sz, uint64_t n) {
        set_size(sz); count = n; lf = 0.77f;
        max = (uint64_t)((float)size * lf);
        array.reset(size);
        occ.assign(size, 0);
    }
    // encap_kmerset, growable case (newhash.c:368-454): next size, then re-home in place in old-slot order,
    // an element that lands on a not-yet-moved old element kicks it out and that one is placed next
    double t_grow = 0;
    void grow() {
        const auto tg0 = std::chrono::steady_clock::now();
        struct Acc { double& t; std::chrono::steady_clock::time_point t0; ~Acc() { t += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } acc{t_grow, tg0};
        uint64_t n = size;
        do {
            n = (n < 0xFFFFFFFULL) ? (n << 1) : (n + 0xFFFFFFULL);
            n = ref_next_prime(n);
        } while ((float)n * lf < (float)(count + 1));
        const uint64_t old = size;
        if (n > array.n) array.reset(n, old);
        for (uint64_t i = old; i < n; i++) array[i].seq.w[0] = EMPTY;
        // one state byte a slot: 0 free, 1 placed, 2 old element not moved yet -- the occupancy bytes themselves, shifted
        // for the duration of the move (so there is no pass to build them and none to turn them back).  The old slots are
        // visited in index order (that order is what the reference's layout depends on); the cache misses are taken
        // ahead of time in two steps: LOOK_FAR slots ahead the home of the element is computed and its state byte and slot are
        // prefetched; LOOK_NEAR slots ahead that state byte is looked at, and if an unmoved old element sits there -- it will
        // be kicked out and re-homed next (a fifth of all moves), a home that depends on a slot not read yet -- its own
        // home is computed and prefetched too.
        enum : uint8_t { FREE = 0, PLACED = 1, PENDING = 2 };
        std::vector<uint8_t> st = std::move(occ);
        st.resize(n, FREE);
        for (uint64_t i = 0; i < old; i++) st[i] <<= 1;
        set_size(n);
        max = (uint64_t)((float)n * lf);
        constexpr uint64_t LOOK_NEAR = 16, LOOK_FAR = 40;
        uint64_t ring[LOOK_FAR];
        auto look_far = [&](uint64_t j) {
            if (j < old && st[j] == PENDING) {
                const uint64_t h = home(array[j].seq);
                ring[j % LOOK_FAR] = h;
                __builtin_prefetch(&st[h], 1);
                __builtin_prefetch(&array[h], 1);
                __builtin_prefetch((const char*)&array[h] + sizeof(HNode<NW>) - 1, 1);   // (a slot may straddle two lines)
            }
        };
        auto look_near = [&](uint64_t j) {
            if (j < old && st[j] == PENDING) {
                const uint64_t h = ring[j % LOOK_FAR];
                if (st[h] == PENDING && h != j) {
                    const uint64_t h2 = home(array[h].seq);
                    __builtin_prefetch(&st[h2], 1);
                    __builtin_prefetch(&array[h2], 1);
                    __builtin_prefetch((const char*)&array[h2] + sizeof(HNode<NW>) - 1, 1);
                }
            }
        };
        const auto tg1 = std::chrono::steady_clock::now();
        uint64_t n_kick = 0, n_moved = 0;
        for (uint64_t j = 0; j < std::min<uint64_t>(LOOK_FAR, old); j++) look_far(j);
        for (uint64_t j = 0; j < std::min<uint64_t>(LOOK_NEAR, old); j++) look_near(j);
        for (uint64_t i = 0; i < old; i++) {
            const bool mine = st[i] == PENDING;
            uint64_t hc = mine ? ring[i % LOOK_FAR] : 0;
            look_far(i + LOOK_FAR);                                    // reuses ring slot i % LOOK_FAR, read just above
            look_near(i + LOOK_NEAR);
            if (!mine) continue;
            HNode<NW> cur = array[i];
            st[i] = FREE;
            array[i].seq.w[0] = EMPTY;                            // vacated (whoever lands here later overwrites it)
            for (;;) {
                while (st[hc] == PLACED) { if (++hc == size) hc = 0; }
                const bool kick = st[hc] == PENDING;              // an old element still sits there: it goes next
                st[hc] = PLACED;
                n_moved++;
                if (kick) {
                    n_kick++;
                    std::swap(cur, array[hc]);
                    hc = home(cur.seq);
                } else {
                    array[hc] = cur;
                    break;
                }
            }
        }
        occ = std::move(st);
        if (pg::env_measure("PG_GROW_VERBOSE")) {
            auto d = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
            fprintf(stderr, "grow %llu -> %llu: prepare %.3fs, re-home %.3fs (%llu moved, %llu kicks)\n", (unsigned long long)old, (unsigned long long)n, d(tg0, tg1),
                    d(tg1, std::chrono::steady_clock::now()), (unsigned long long)n_moved, (unsigned long long)n_kick);
        }
    }
    // the growth test of put_kmerset (newhash.c:477) for a static (-a) pool only raises the load factor: the reference
    // compares its float load_factor with the double 0.88 (newhash.c:355), which stays true after the assignment, so its
    // "Static memory pool exploded" exit is never taken and a pool that fills up makes put_kmerset probe forever.  Here a
    // full pool is reported instead (`full`), the callers fail with that message.
    bool full = false;
    void before_put(bool static_pool) {
        if (count + 1 <= max) return;
        if (static_pool) { lf = 0.88f; max = (uint64_t)((float)size * lf); if (count >= size) full = true; return; }
        grow();
    }
    void put_new(const HNode<NW>& nd, bool static_pool) {
        before_put(static_pool);
        put_new_at(nd, home(nd.seq));
    }
    void prefetch_put(uint64_t hc) const {
        __builtin_prefetch(&array[hc], 1);
        __builtin_prefetch((const char*)&array[hc] + sizeof(HNode<NW>) - 1, 1);      // (a slot may straddle two lines)
        __builtin_prefetch(&occ[hc], 1);
    }
    void put_new_at(const HNode<NW>& nd, uint64_t hc) {                 // the caller ran before_put
        while (occ[hc]) { if (++hc == size) hc = 0; }
        occ[hc] = 1;
        array[hc] = nd;
        count++;
    }
    HNode<NW>* find(const Kmer<NW>& k) { return find_from(k, home(k)); }   // search_kmerset, newhash.c:277-318
    void prefetch(uint64_t hc) const { __builtin_prefetch(&array[hc]); }
    HNode<NW>* find_from(const Kmer<NW>& k, uint64_t hc) {
        for (;;) {
            if (array[hc].seq.w[0] == EMPTY) return nullptr;
            if (kmer_eq<NW>(array[hc].seq, k)) return &array[hc];
            if (++hc == size) hc = 0;
        }
    }
};

template <int NW> static inline int nL(const HNode<NW>& n, int i) { return (n.A >> (6 * i)) & 63; }
template <int NW> static inline int nR(const HNode<NW>& n, int i) { return (n.B >> (6 * i)) & 63; }
template <int NW> static inline void clrL(HNode<NW>& n, int i) { n.A &= ~(63u << (6 * i)); }
template <int NW> static inline void clrR(HNode<NW>& n, int i) { n.B &= ~(63u << (6 * i)); }
template <int NW> static inline int n_in(const HNode<NW>& n) { int c = 0; for (int i = 0; i < 4; i++) c += nL(n, i) > 0; return c; }
template <int NW> static inline int n_out(const HNode<NW>& n) { int c = 0; for (int i = 0; i < 4; i++) c += nR(n, i) > 0; return c; }

template <int NW>
struct KmerHash {
    size_t operator()(const Kmer<NW>& k) const { return (size_t)kmer_mix<NW>(k); }
};
template <int NW>
struct KmerEq {
    bool operator()(const Kmer<NW>& a, const Kmer<NW>& b) const { return kmer_eq<NW>(a, b); }
};

struct PatchVal { uint32_t id; uint32_t twin; };

template <int NW>
struct Graph {
    int K, P;
    int n_threads = 0;             // host threads for the parallel scans (0 = all)
    // with the sets mirrored in HBM the tip walks run there (graph_kernels.hip: tip_walk_kernel); the host keeps the
    // order-dependent replay and sends the nodes it changed back
    P2Device* tip_dev = nullptr;
    std::vector<uint64_t> set_base;   // global slot of every set's slot 0 (+ the total)
    int tip_error = PG_OK;
    Kmer<NW> filter;
    uint32_t bias;
    const uint32_t* crc;
    std::vector<HSet<NW>> sets;
    // KmerSetsPatch (node2edge.c:371-376,481-542): canonical (K+1)-mer of every length-1 edge -> edge id, twin.  Only
    // looked up by key (prlRead2path.c:558-596), so a plain map replaces the reference's second family of hash sets.
    std::unordered_map<Kmer<NW>, PatchVal, KmerHash<NW>, KmerEq<NW>> patch;

    int set_of(const Kmer<NW>& k) const { return (int)set_of_crc(host_crc32<NW>(k), (uint32_t)P, bias); }

    struct Hit { HNode<NW>* node; Kmer<NW> oriented; bool smaller; int set; };
    // canonicalise a walk-oriented k-mer and look its node up
    Hit lookup(const Kmer<NW>& word) {
        Kmer<NW> bal = kmer_rc<NW>(word, K);
        Hit h;
        h.oriented = word;
        if (kmer_less<NW>(bal, word)) { h.smaller = false; h.set = set_of(bal); h.node = sets[h.set].find(bal); }
        else { h.smaller = true; h.set = set_of(word); h.node = sets[h.set].find(word); }
        return h;
    }
    // the single outgoing base of a linear node in walk orientation
    static int only_out(const HNode<NW>& n, bool smaller) {
        int ch;
        if (smaller) { for (ch = 0; ch < 4; ch++) if (nR(n, ch)) break; return ch; }
        for (ch = 0; ch < 4; ch++) if (nL(n, ch)) break;
        return ch ^ 2;
    }
    // dislink2prevUncertain / dislink2nextUncertain (newhash.c:681-717)
    static void cut_prev(HNode<NW>& n, int ch, bool smaller) { if (smaller) clrL(n, ch); else clrR(n, ch ^ 2); }
    static void cut_next(HNode<NW>& n, int ch, bool smaller) { if (smaller) clrR(n, ch); else clrL(n, ch ^ 2); }

    // Mark1in1outNode of cutTipPreGraph.c:532-564,603-639
    void remark_linear() {
        int nt = pick_threads(n_threads);
        if (nt < 1) nt = 1;
        std::atomic<uint64_t> next{0};
        const uint64_t STEP = 1 << 18;
        std::vector<std::pair<int, uint64_t>> chunks;
        for (int si = 0; si < (int)sets.size(); si++)
            for (uint64_t lo = 0; lo < sets[si].size; lo += STEP) chunks.emplace_back(si, lo);
        auto body = [&]() {
            for (;;) {
                const uint64_t ci = next.fetch_add(1);
                if (ci >= chunks.size()) break;
                HSet<NW>& s = sets[chunks[ci].first];
                const uint64_t hi = std::min<uint64_t>(s.size, chunks[ci].second + STEP);
                for (uint64_t i = chunks[ci].second; i < hi; i++) {
                    if (!s.occ[i]) continue;
                    HNode<NW>& n = s.array[i];
                    if (n.B & (B_DELETED | B_LINEAR)) continue;
                    if (n_in(n) == 1 && n_out(n) == 1) n.B |= B_LINEAR;
                }
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(body);
        body();
        for (auto& th : pool) th.join();
    }

    // The same marking after a round of tip clipping: only the ends of clipped tips changed their arcs since the last
    // marking, so only they can have become 1-in-1-out; every other node is marked (or not) as it was.
    std::vector<uint64_t> phase_touched;           // set << 40 | slot of every node the scans of this phase changed
    void remark_touched() {
        int nt = pick_threads(n_threads);
        if (nt < 1) nt = 1;
        auto body = [&](int t) {
            for (size_t i = phase_touched.size() * t / nt; i < phase_touched.size() * (t + 1) / nt; i++) {
                HNode<NW>& n = sets[phase_touched[i] >> 40].array[phase_touched[i] & ((1ULL << 40) - 1)];
                if (n.B & (B_DELETED | B_LINEAR)) continue;
                if (n_in(n) == 1 && n_out(n) == 1) __atomic_fetch_or(&n.B, B_LINEAR, __ATOMIC_RELAXED);   // (a node may be listed twice)
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
        body(0);
        for (auto& th : pool) th.join();
        std::vector<uint64_t>().swap(phase_touched);
    }

    // clipTipFromNode (cutTipPreGraph.c:43-346), split into the read-only walk and the mutation it decides on, so
    // that the walks can run ahead of the (order-dependent) mutations
    struct TipDecision {
        int action = 0;                // 0 nothing, 1 both ends dead, 2 thin cut, 3 minority cut
        HNode<NW>* far = nullptr;      // where the walk stopped (null: no walk, or longer than the cut-off)
        int far_set = 0, first = 0;
        bool far_smaller = false;
    };
    static bool dead_end(const HNode<NW>& n) {
        const int in = n_in(n), out = n_out(n);
        return (in == 0 && out == 1) || (in == 1 && out == 0);
    }
    // the walk: from a dead-end start over linear nodes to the node it stops at
    TipDecision tip_walk(const HNode<NW>& start, int cut_len, bool thin) {
        TipDecision d;
        const int in = n_in(start), out = n_out(start);
        Kmer<NW> prev;
        int ch;
        if (in == 0 && out == 1) {
            prev = start.seq;
            for (ch = 0; ch < 4; ch++) if (nR(start, ch)) break;
        } else if (in == 1 && out == 0) {
            prev = kmer_rc<NW>(start.seq, K);
            for (ch = 0; ch < 4; ch++) if (nL(start, ch)) break;
            ch ^= 2;
        } else return d;
        int count = 1;
        Hit h = lookup(kmer_next<NW>(prev, ch, filter));
        if (!h.node) { fprintf(stderr, "Kmer is not found while clipping a tip.\n"); exit(1); }
        while (h.node->B & B_LINEAR) {
            count++;
            if (thin && !(h.node->B & B_SINGLE)) break;
            if (count > cut_len) return d;
            prev = h.oriented;
            h = lookup(kmer_next<NW>(prev, only_out(*h.node, h.smaller), filter));
            if (!h.node) { fprintf(stderr, "Kmer is not found while clipping a tip.\n"); exit(1); }
        }
        d.far = h.node; d.far_set = h.set; d.far_smaller = h.smaller;
        d.first = kmer_first<NW>(prev, K);
        return d;
    }
    // would a walk arriving at `far` still stop there?
    static bool walk_stops_at(const HNode<NW>& far, bool thin) { return !(far.B & B_LINEAR) || (thin && !(far.B & B_SINGLE)); }
    // the verdict, from the stop node as it is now
    void tip_decide(TipDecision& d, bool thin) const {
        d.action = 0;
        if (!d.far) return;
        const HNode<NW>& far = *d.far;
        if (n_in(far) + n_out(far) == 1) { d.action = 1; return; }
        if (thin) { d.action = 2; return; }
        int strongest = 0;
        for (int c = 0; c < 4; c++) strongest = std::max(strongest, d.far_smaller ? nL(far, c) : nR(far, c));
        const int mine = d.far_smaller ? nL(far, d.first) : nR(far, d.first ^ 2);
        if (mine < strongest) d.action = 3;
    }
    TipDecision tip_evaluate(const HNode<NW>& start, int cut_len, bool thin) {
        TipDecision d = tip_walk(start, cut_len, thin);
        tip_decide(d, thin);
        return d;
    }
    bool tip_apply(HNode<NW>& start, const TipDecision& d, long long& tips) {
        if (!d.action) return false;
        HNode<NW>& far = *d.far;
        tips++;
        start.B |= B_DELETED;
        if (d.action == 1) { far.B |= B_DELETED; return true; }
        cut_prev(far, d.first, d.far_smaller);
        if (d.action == 2) far.B &= ~B_LINEAR;
        else if (n_in(far) == 1 && n_out(far) == 1) far.B |= B_LINEAR;
        return true;
    }
    bool clip_tip(HNode<NW>& start, int cut_len, bool thin, long long& tips) {
        return tip_apply(start, tip_evaluate(start, cut_len, thin), tips);
    }

    // One scan of removeSingleTips / removeMinorTips over all sets (cutTipPreGraph.c:363-399,414-488) with the walks done
    // by all host threads.  A walk reads its start node, linear interior nodes and the node it stops at; a clipped tip
    // changes only its start node and its stop node, and neither was the interior of any walk when the scan began.  So:
    // every dead-end start is walked in parallel up front; the scan order is then replayed serially, taking the
    // precomputed decision when neither end of the walk has been touched since and walking again otherwise.  A stop node
    // that becomes a dead end further down the scan is visited there, as the sequential scan would.
    long long tip_scan(int cut_len, bool thin, long long& tips) {
        int nt = pick_threads(n_threads);
        if (nt < 1) nt = 1;
        struct Cand { uint64_t pos; TipDecision d; };
        struct Chunk { int set; uint64_t lo, hi; std::vector<Cand> c; };
        std::vector<Chunk> chunks;
        const uint64_t STEP = 1 << 16;
        for (int si = 0; si < (int)sets.size(); si++)
            for (uint64_t lo = 0; lo < sets[si].size; lo += STEP) chunks.push_back(Chunk{si, lo, std::min<uint64_t>(sets[si].size, lo + STEP), {}});
        auto startable = [thin](const HNode<NW>& n) { return !(n.B & (B_LINEAR | B_DELETED)) && (!thin || (n.B & B_SINGLE)); };
        auto nowt = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double tt0 = nowt();
        std::vector<Cand> from_device;
        if (tip_dev) {
            std::vector<P2TipWalk> walks;
            const int rc = p2_tip_walks(tip_dev, cut_len, thin, walks);
            if (rc) { tip_error = rc; return 0; }
            from_device.resize(walks.size());
            auto body = [&](int t) {
                for (size_t i = walks.size() * t / nt; i < walks.size() * (t + 1) / nt; i++) {
                    const P2TipWalk& w = walks[i];
                    const int si = (int)(std::upper_bound(set_base.begin(), set_base.end(), (uint64_t)w.pos) - set_base.begin()) - 1;
                    Cand& c = from_device[i];
                    c.pos = ((uint64_t)si << 40) | (w.pos - set_base[si]);
                    c.d = TipDecision();
                    if (w.far != ~0ULL) {
                        const int fs = (int)(std::upper_bound(set_base.begin(), set_base.end(), (uint64_t)w.far) - set_base.begin()) - 1;
                        c.d.far = &sets[fs].array[w.far - set_base[fs]];
                        c.d.far_set = fs; c.d.first = (int)w.first; c.d.far_smaller = w.far_smaller != 0;
                        tip_decide(c.d, thin);
                    }
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
            body(0);
            for (auto& th : pool) th.join();
        } else {
            std::atomic<size_t> next{0};
            auto body = [&]() {
                for (;;) {
                    const size_t ci = next.fetch_add(1);
                    if (ci >= chunks.size()) break;
                    Chunk& ck = chunks[ci];
                    HSet<NW>& s = sets[ck.set];
                    for (uint64_t i = ck.lo; i < ck.hi; i++) {
                        if (!s.occ[i]) continue;
                        const HNode<NW>& n = s.array[i];
                        if (!startable(n) || !dead_end(n)) continue;
                        ck.c.push_back(Cand{((uint64_t)ck.set << 40) | i, tip_evaluate(n, cut_len, thin)});
                    }
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body);
            body();
            for (auto& th : pool) th.join();
        }
        const double tt1 = nowt();
        // nodes changed during this scan: a spare bit of the node itself (only the ends of clipped tips ever get it; cleared
        // again from the list below before anything else looks at the word).  A byte map beside the sets did the same with
        // two more cache misses per candidate in a loop that is nothing but cache misses.
        std::vector<uint64_t> touched_list;
        // whichever way this function is left, no node keeps the scratch bit (B_TOUCHED is the reference's `checked` bit)
        struct ClearTouched {
            Graph& g; std::vector<uint64_t>& list;
            ~ClearTouched() { for (uint64_t tp : list) g.sets[tp >> 40].array[tp & ((1ULL << 40) - 1)].B &= ~B_TOUCHED; }
        } clear_touched{*this, touched_list};
        auto is_touched = [&](int, const HNode<NW>* n) { return (n->B & B_TOUCHED) != 0; };
        // positions to come back to, smallest first.  Millions of them are pending at a time on a large graph, so they wait
        // unsorted in buckets of 65536 slots and only the bucket the scan is in is kept as a heap.
        struct LaterQueue {
            typedef std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> Heap;
            std::vector<std::vector<uint64_t>> bucket;
            std::vector<size_t> first;                  // first bucket of every set
            Heap heap;                                  // the pending positions of bucket `cur`
            size_t cur = 0, pending = 0;
            size_t index(uint64_t pos) const { return first[pos >> 40] + (size_t)((pos & ((1ULL << 40) - 1)) >> 16); }
            void push(uint64_t pos) {
                const size_t b = index(pos);
                pending++;
                if (b == cur) { heap.push(pos); return; }
                if (b < cur) {                          // the heap had run ahead of the scan: put it back
                    while (!heap.empty()) { bucket[cur].push_back(heap.top()); heap.pop(); }
                    cur = b;
                    heap.push(pos);
                    return;
                }
                bucket[b].push_back(pos);
            }
            void settle() {
                while (heap.empty()) {
                    if (!bucket[cur].empty()) { for (uint64_t x : bucket[cur]) heap.push(x); std::vector<uint64_t>().swap(bucket[cur]); }
                    else cur++;
                }
            }
            bool empty() const { return pending == 0; }
            uint64_t top() { settle(); return heap.top(); }
            void pop() { settle(); heap.pop(); pending--; }
        } later;
        later.first.assign(sets.size() + 1, 0);
        for (size_t si = 0; si < sets.size(); si++) later.first[si + 1] = later.first[si] + (size_t)((sets[si].size >> 16) + 1);
        later.bucket.resize(later.first[sets.size()] + 1);
        long long removed = 0, rewalked = 0, redecided = 0;
        std::vector<uint64_t> changed;                              // global slots of the nodes this scan changed
        auto node_at = [&](uint64_t pos) -> HNode<NW>& { return sets[pos >> 40].array[pos & ((1ULL << 40) - 1)]; };
        auto visit = [&](uint64_t pos, const TipDecision* spec) {
            HNode<NW>& n = node_at(pos);
            if (!startable(n)) return;
            TipDecision d;
            const int nset = (int)(pos >> 40);
            if (spec && !is_touched(nset, &n)) {
                d = *spec;
                if (d.far && is_touched(d.far_set, d.far)) {
                    // the walk itself only crossed nodes nothing changes; if it still ends where it did, only the verdict
                    // has to be taken again from that node's present state
                    if (walk_stops_at(*d.far, thin)) { tip_decide(d, thin); redecided++; }
                    else { d = tip_evaluate(n, cut_len, thin); rewalked++; }
                }
            } else { d = tip_evaluate(n, cut_len, thin); rewalked++; }
            if (!tip_apply(n, d, tips)) return;
            removed++;
            n.B |= B_TOUCHED;
            const uint64_t fslot = (uint64_t)(d.far - sets[d.far_set].array.data());
            d.far->B |= B_TOUCHED;
            touched_list.push_back(pos);
            touched_list.push_back(((uint64_t)d.far_set << 40) | fslot);
            if (tip_dev) { changed.push_back(set_base[nset] + (pos & ((1ULL << 40) - 1))); changed.push_back(set_base[d.far_set] + fslot); }
            if (d.action != 1) {
                const uint64_t fpos = ((uint64_t)d.far_set << 40) | fslot;
                if (fpos > pos) later.push(fpos);
            }
        };
        // the replay is serial and every step touches a handful of random cache lines (start node, stop node, their
        // "touched" bytes): flatten the candidates and prefetch those lines a few steps ahead
        std::vector<Cand*> flat;
        {
            size_t n_cand = from_device.size();
            for (Chunk& ck : chunks) n_cand += ck.c.size();
            flat.reserve(n_cand);
            touched_list.reserve(2 * n_cand);                   // (most candidates are clipped: no regrowing copies in the loop)
            if (tip_dev) changed.reserve(2 * n_cand);
        }
        for (Chunk& ck : chunks) for (Cand& cd : ck.c) flat.push_back(&cd);
        for (Cand& cd : from_device) flat.push_back(&cd);
        auto warm = [&](const Cand& cd) {
            const int cs = (int)(cd.pos >> 40);
            const uint64_t slot = cd.pos & ((1ULL << 40) - 1);
            __builtin_prefetch(&sets[cs].array[slot], 1);
            if (cd.d.far) __builtin_prefetch(cd.d.far, 1);
        };
        constexpr size_t WARM = 12;
        for (size_t i = 0; i < std::min(WARM, flat.size()); i++) warm(*flat[i]);
        for (size_t fi = 0; fi < flat.size(); fi++) {
            if (fi + WARM < flat.size()) warm(*flat[fi + WARM]);
            {
                Cand& cd = *flat[fi];
                while (!later.empty() && later.top() < cd.pos) {
                    const uint64_t p = later.top();
                    while (!later.empty() && later.top() == p) later.pop();
                    visit(p, nullptr);
                }
                while (!later.empty() && later.top() == cd.pos) later.pop();     // already on the list: visited once
                visit(cd.pos, &cd.d);
            }
        }
        while (!later.empty()) {
            const uint64_t p = later.top();
            while (!later.empty() && later.top() == p) later.pop();
            visit(p, nullptr);
        }
        for (uint64_t tp : touched_list) node_at(tp).B &= ~B_TOUCHED;        // (before the words are read for the device mirror below)
        phase_touched.insert(phase_touched.end(), touched_list.begin(), touched_list.end());
        if (tip_dev && !changed.empty()) {                          // bring the device copy up to date
            std::vector<uint64_t> ab(changed.size());
            {   // the present counter words of those nodes (random reads: all threads)
                auto body = [&](int t) {
                    for (size_t i = changed.size() * t / nt; i < changed.size() * (t + 1) / nt; i++) {
                        const int si = (int)(std::upper_bound(set_base.begin(), set_base.end(), changed[i]) - set_base.begin()) - 1;
                        const HNode<NW>& n = sets[si].array[changed[i] - set_base[si]];
                        ab[i] = (uint64_t)n.A | ((uint64_t)n.B << 32);
                    }
                };
                std::vector<std::thread> pool;
                for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
                body(0);
                for (auto& th : pool) th.join();
            }
            const int rc = p2_mirror_nodes(tip_dev, changed.data(), ab.data(), changed.size());
            if (rc) { tip_error = rc; return removed; }
        }
        if (pg::env_user("PG_HOST_VERBOSE"))
            fprintf(stderr, "tip scan: %lld removed, %lld walked again, %lld decided again; walks %.2fs, replay %.2fs (%d threads)\n", removed, rewalked,
                    redecided, tt1 - tt0, nowt() - tt1, nt);
        return removed;
    }

    // removeSingleTips (cutTipPreGraph.c:363-399)
    void remove_single_tips() {
        const int cut = 2 * K;
        long long tips = 0;
        fprintf(stderr, "Start to remove frequency-one-kmer tips shorter than %d.\n", cut);
        tip_scan(cut, true, tips);
        fprintf(stderr, "Total %lld tip(s) removed.\n", tips);
        last_single = tips;
        remark_touched();
        if (tip_dev && !tip_error) tip_error = p2_remark_linear(tip_dev);
    }
    // removeMinorTips (cutTipPreGraph.c:414-488)
    void remove_minor_tips() {
        const int cut = 2 * K;
        long long tips = 0;
        fprintf(stderr, "Start to remove tips with minority links.\n");
        int round = 1;
        for (;;) {
            const long long removed = tip_scan(cut, false, tips);
            fprintf(stderr, "%lld tip(s) removed in cycle %d.\n", removed, round++);
            if (!removed || tip_error) break;
        }
        fprintf(stderr, "Total %lld tip(s) removed.\n", tips);
        last_minor = tips;
        remark_touched();
        if (tip_dev && !tip_error) tip_error = p2_remark_linear(tip_dev);
    }
    long long last_single = 0, last_minor = 0;
};

// ---- writers -------------------------------------------------------------------------------------------
struct GzText {
    gzFile f = nullptr;
    std::string buf;
    bool open(const std::string& path) {
        f = gzopen(path.c_str(), "w");                   // default level, as gzopen(...,"w") in node2edge.c:66
        if (f) gzbuffer(f, 1 << 20);
        buf.reserve(1 << 22);
        return f != nullptr;
    }
    void flush() { if (!buf.empty()) { gzwrite(f, buf.data(), (unsigned)buf.size()); buf.clear(); } }
    void put(const char* s, size_t n) { buf.append(s, n); if (buf.size() > (1u << 22) - 65536) flush(); }
    void close() { flush(); gzclose(f); f = nullptr; }
};

template <int NW>
static int fmt_kmer(char* dst, const Kmer<NW>& k, char tail) {             // print_kmer, kmer.c:807-817 / 495-505
    int n = 0;
    for (int i = 0; i < NW; i++) n += sprintf(dst + n, i ? " %llx" : "%llx", (unsigned long long)k.w[i]);
    dst[n++] = tail;
    return n;
}

template <int NW>
struct EdgeBuilder {
    Graph<NW>& g;
    GzText& out;
    struct Bead { HNode<NW>* node; Kmer<NW> kmer; bool smaller; };
    std::vector<Bead> beads;
    std::string seq;
    int edge_c = 0;        // running edge id (both strands)
    long long records = 0, extra_nodes = 0;

    EdgeBuilder(Graph<NW>& g_, GzText& o) : g(g_), out(o) {}

    // stringBeads (node2edge.c:86-218)
    void walk(int nextch) {
        typename Graph<NW>::Hit h = g.lookup(kmer_next<NW>(beads[0].kmer, nextch, g.filter));
        while (h.node && (h.node->B & B_LINEAR)) {
            beads.push_back(Bead{h.node, h.oriented, h.smaller});
            h = g.lookup(kmer_next<NW>(h.oriented, Graph<NW>::only_out(*h.node, h.smaller), g.filter));
        }
        if (!h.node) { fprintf(stderr, "Kmer is not found while building an edge.\n"); exit(1); }
        beads.push_back(Bead{h.node, h.oriented, h.smaller});
    }
    // check_iden_kmerList (node2edge.c:624-649)
    bool palindrome() const {
        const size_t n = beads.size();
        for (size_t i = 0; i < n; i++)
            if (!kmer_eq<NW>(beads[i].kmer, kmer_rc<NW>(beads[n - 1 - i].kmer, g.K))) return false;
        return true;
    }
    // merge_linearV2 + output_1edge (node2edge.c:430-609, output_pregraph.c:88-110)
    void emit() {
        const int bal = palindrome() ? 0 : 1;
        const int count = (int)beads.size(), length = count - 1;
        Bead& first = beads[0];
        Bead& last = beads[count - 1];
        Graph<NW>::cut_prev(*last.node, kmer_first<NW>(beads[count - 2].kmer, g.K), last.smaller);
        Graph<NW>::cut_next(*first.node, kmer_last<NW>(beads[1].kmer), first.smaller);
        edge_c++;
        records++;
        if (length == 1) {                   // the (K+1)-mer joining two branch nodes (node2edge.c:481-542)
            extra_nodes++;
            const Kmer<NW> plus = kmer_plus<NW>(first.kmer, kmer_last<NW>(last.kmer));
            const Kmer<NW> bal_plus = rc_plus<NW>(plus, g.K);
            if (kmer_less<NW>(plus, bal_plus)) g.patch[plus] = PatchVal{(uint32_t)edge_c, (uint32_t)(bal + 1)};
            else g.patch[bal_plus] = PatchVal{(uint32_t)(edge_c + bal), (uint32_t)(1 - bal)};
        }
        long long sum = 0;
        for (int i = 1; i < count - 1; i++) {
            const HNode<NW>& n = *beads[i].node;
            sum += nL(n, 0) + nL(n, 1) + nL(n, 2) + nL(n, 3);
        }
        for (int i = 1; i < count - 1; i++) {
            HNode<NW>& n = *beads[i].node;
            const uint32_t twin = beads[i].smaller ? (uint32_t)(bal + 1) : (uint32_t)(1 - bal);
            n.A = beads[i].smaller ? (uint32_t)edge_c : (uint32_t)(edge_c + bal);   // edge id replaces word A
            n.B = (n.B & 0x0FFFFFFFu) | (twin << B_TWIN_SHIFT) | (1u << B_INEDGE_SHIFT);
        }
        int cvg = 0;
        if (length > 1) { long long v = sum / (length - 1) * 10; cvg = v > 16000 ? 16000 : (int)v; }
        char head[256];
        int n = sprintf(head, ">length %d,", length);
        n += fmt_kmer<NW>(head + n, first.kmer, ',');
        n += fmt_kmer<NW>(head + n, last.kmer, ',');
        n += sprintf(head + n, "cvg %d, %d\n", cvg, bal);
        out.put(head, n);
        seq.clear();
        for (int i = 0; i < length; i++) {
            seq.push_back("ACTG"[kmer_last<NW>(beads[i + 1].kmer)]);
            if ((i + 1) % 100 == 0) seq.push_back('\n');
        }
        if (length % 100 != 0) seq.push_back('\n');
        out.put(seq.data(), seq.size());
        edge_c += bal;
    }
    // make_edge + startEdgeFromNode (node2edge.c:237-411)
    void run() {
        for (auto& s : g.sets)
            for (uint64_t i = 0; i < s.size; i++) {
                if (!s.occ[i]) continue;
                HNode<NW>& n = s.array[i];
                if (n.B & (B_LINEAR | B_DELETED)) continue;
                const Kmer<NW> fwd = n.seq, rev = kmer_rc<NW>(n.seq, g.K);
                for (int ch = 0; ch < 4; ch++) {
                    if (!nR(n, ch)) continue;
                    beads.clear();
                    beads.push_back(Bead{&n, fwd, true});
                    walk(ch);
                    emit();
                }
                for (int ch = 0; ch < 4; ch++) {
                    if (!nL(n, ch)) continue;
                    beads.clear();
                    beads.push_back(Bead{&n, rev, false});
                    walk(ch ^ 2);
                    emit();
                }
            }
    }
};


// ---------------------------------------------------------------------------------------------------------------------
// The same edges, built by all host threads.  Every chain of linear nodes between two branch nodes can be entered
// from exactly two (node, arc) positions -- its two ends -- and the sequential scan (make_edge, node2edge.c:237-411)
// emits it from whichever end it meets first and unlinks the other.  A walk only reads state that no emit changes
// before the chain itself is emitted, so the walks are independent:
//   1. the slot ranges are walked in parallel; a walk whose other end precedes it in scan order is dropped, the
//      others are formatted (text record, interior nodes, arcs to unlink, (K+1)-mer of a length-1 edge);
//   2. edge ids are a prefix sum over the ranges in scan order;
//   3. in parallel again: unlink the end arcs, tag the interior nodes with their edge id, deflate each range's text
//      into its own gzip member;
//   4. serially: the (K+1)-mer patch entries in scan order, the gzip members in scan order.
// ---------------------------------------------------------------------------------------------------------------------
template <int NW>
struct ParallelEdgeBuilder {
    Graph<NW>& g;
    int edge_c = 0;
    long long records = 0, extra_nodes = 0;
    explicit ParallelEdgeBuilder(Graph<NW>& g_) : g(g_) {}

    struct Cand {
        HNode<NW>* first; HNode<NW>* last;
        uint64_t inner_off; uint32_t n_inner;
        uint8_t next_ch, prev_ch; bool first_smaller, last_smaller;
        uint8_t bal; bool len1, plus_smaller;
        uint32_t plus_idx;
    };
    struct Chunk {
        int set; uint64_t lo, hi;
        std::vector<Cand> cands;
        std::vector<uintptr_t> inner;                // interior node pointer | smaller
        std::vector<Kmer<NW>> plus;                  // canonical (K+1)-mers of the length-1 edges
        std::string text;
        std::vector<uint8_t> gz;
        std::vector<std::pair<Kmer<NW>, PatchVal>> patch;
        int ids = 0, base = 0;
        long long extra = 0;
    };

    struct Walker {
        Graph<NW>& g;
        struct Bead { HNode<NW>* node; Kmer<NW> kmer; bool smaller; int set; };
        std::vector<Bead> beads;
        explicit Walker(Graph<NW>& g_) : g(g_) {}
        void walk(int nextch) {                      // stringBeads (node2edge.c:86-218)
            typename Graph<NW>::Hit h = g.lookup(kmer_next<NW>(beads[0].kmer, nextch, g.filter));
            while (h.node && (h.node->B & B_LINEAR)) {
                beads.push_back(Bead{h.node, h.oriented, h.smaller, h.set});
                h = g.lookup(kmer_next<NW>(h.oriented, Graph<NW>::only_out(*h.node, h.smaller), g.filter));
            }
            if (!h.node) { fprintf(stderr, "Kmer is not found while building an edge.\n"); exit(1); }
            beads.push_back(Bead{h.node, h.oriented, h.smaller, h.set});
        }
        bool palindrome() const {                    // check_iden_kmerList (node2edge.c:624-649)
            const size_t n = beads.size();
            for (size_t i = 0; i < n; i++)
                if (!kmer_eq<NW>(beads[i].kmer, kmer_rc<NW>(beads[n - 1 - i].kmer, g.K))) return false;
            return true;
        }
    };

    // one start (node, arc): walk, decide, format
    void consider(Walker& w, Chunk& c, int set, uint64_t slot, int arc_order) {
        const int count = (int)w.beads.size(), length = count - 1;
        typename Walker::Bead& first = w.beads[0];
        typename Walker::Bead& last = w.beads[count - 1];
        const int prev_ch = kmer_first<NW>(w.beads[count - 2].kmer, g.K);
        const int next_ch = kmer_last<NW>(w.beads[1].kmer);
        // where the sequential scan would start the same chain from its other end
        const uint64_t tslot = (uint64_t)(last.node - g.sets[last.set].array.data());
        const int torder = last.smaller ? 4 + prev_ch : (prev_ch ^ 2);
        if (last.set != set ? last.set < set : (tslot != slot ? tslot < slot : torder < arc_order)) return;
        Cand cd;
        cd.first = first.node; cd.last = last.node;
        cd.first_smaller = first.smaller; cd.last_smaller = last.smaller;
        cd.next_ch = (uint8_t)next_ch; cd.prev_ch = (uint8_t)prev_ch;
        cd.bal = w.palindrome() ? 0 : 1;
        cd.len1 = length == 1;
        cd.plus_smaller = false; cd.plus_idx = 0;
        if (cd.len1) {                               // the (K+1)-mer joining two branch nodes (node2edge.c:481-542)
            const Kmer<NW> plus = kmer_plus<NW>(first.kmer, kmer_last<NW>(last.kmer));
            const Kmer<NW> bal_plus = rc_plus<NW>(plus, g.K);
            cd.plus_smaller = kmer_less<NW>(plus, bal_plus);
            cd.plus_idx = (uint32_t)c.plus.size();
            c.plus.push_back(cd.plus_smaller ? plus : bal_plus);
            c.extra++;
        }
        cd.inner_off = c.inner.size();
        cd.n_inner = (uint32_t)(count - 2);
        long long sum = 0;
        for (int i = 1; i < count - 1; i++) {
            const HNode<NW>& n = *w.beads[i].node;
            sum += nL(n, 0) + nL(n, 1) + nL(n, 2) + nL(n, 3);
            c.inner.push_back((uintptr_t)w.beads[i].node | (uintptr_t)(w.beads[i].smaller ? 1 : 0));
        }
        int cvg = 0;
        if (length > 1) { long long v = sum / (length - 1) * 10; cvg = v > 16000 ? 16000 : (int)v; }
        char head[256];
        int n = sprintf(head, ">length %d,", length);
        n += fmt_kmer<NW>(head + n, first.kmer, ',');
        n += fmt_kmer<NW>(head + n, last.kmer, ',');
        n += sprintf(head + n, "cvg %d, %d\n", cvg, (int)cd.bal);
        c.text.append(head, n);
        for (int i = 0; i < length; i++) {
            c.text.push_back("ACTG"[kmer_last<NW>(w.beads[i + 1].kmer)]);
            if ((i + 1) % 100 == 0) c.text.push_back('\n');
        }
        if (length % 100 != 0) c.text.push_back('\n');
        c.ids += 1 + cd.bal;
        c.cands.push_back(cd);
    }

    void scan(Walker& w, Chunk& c) {
        HSet<NW>& s = g.sets[c.set];
        for (uint64_t i = c.lo; i < c.hi; i++) {
            if (!s.occ[i]) continue;
            HNode<NW>& n = s.array[i];
            if (n.B & (B_LINEAR | B_DELETED)) continue;
            const Kmer<NW> fwd = n.seq, rev = kmer_rc<NW>(n.seq, g.K);
            for (int ch = 0; ch < 4; ch++) {
                if (!nR(n, ch)) continue;
                w.beads.clear();
                w.beads.push_back(typename Walker::Bead{&n, fwd, true, c.set});
                w.walk(ch);
                consider(w, c, c.set, i, ch);
            }
            for (int ch = 0; ch < 4; ch++) {
                if (!nL(n, ch)) continue;
                w.beads.clear();
                w.beads.push_back(typename Walker::Bead{&n, rev, false, c.set});
                w.walk(ch ^ 2);
                consider(w, c, c.set, i, 4 + ch);
            }
        }
    }

    static void clear_arc(uint32_t& word, int i) { __atomic_fetch_and(&word, ~(63u << (6 * i)), __ATOMIC_RELAXED); }
    static bool gz_member(const std::string& text, std::vector<uint8_t>& out) {
        z_stream z;
        memset(&z, 0, sizeof(z));
        // Level 1 by default.  The reference's gzopen(..., "w") (node2edge.c:66) writes at zlib's default, 6: the same text in a file a quarter smaller --
        // measured in round 5 with the members deflated by all host threads beside pass 2: pg_host_graph_finish waited 1.2 s for the file at 60 M reads
        // (a 3.5 s command instead of 2.4) and 2.5 s at 200 M (profiles/r05f_cli_200M_arena_gzip_ab.json); at level 1 it waits 0.00 s.  The file is a
        // multi-member gzip here anyway (never the reference's bytes, always its text; the later stages only gzread it).
        // Round 6: the default is Huffman coding WITHOUT string matching (Z_HUFFMAN_ONLY): an edge file is DNA, which a 32 KB window finds next to nothing
        // to match in -- on 200 MB of edge-like text 98 MB/s a thread against 52 at level 1, and a file 6 % SMALLER (ratio 0.383 against 0.408; level 6:
        // 0.362 at 9 MB/s).  The writer had become the last thing pass 2's finish waits for once the pre-arcs were folded on the device.
        // SOAPDENOVO2_AMD_GZIP_LEVEL=0..9 (zlib's usual strategy at that level; 6 = the reference's file size); anything else is refused loudly.
        static const int level = []() {
            const char* e = pg::env_user("SOAPDENOVO2_AMD_GZIP_LEVEL");
            if (!e) return -1;
            char* end = nullptr;
            const long v = strtol(e, &end, 10);
            if (end == e || *end || v < 0 || v > 9) { fprintf(stderr, "SOAPDENOVO2_AMD_GZIP_LEVEL must be 0..9 (got '%s')\n", e); exit(-1); }
            return (int)v;
        }();
        if (deflateInit2(&z, level < 0 ? 1 : level, Z_DEFLATED, 15 + 16, 8, level < 0 ? Z_HUFFMAN_ONLY : Z_DEFAULT_STRATEGY) != Z_OK) return false;
        out.resize(deflateBound(&z, (uLong)text.size()) + 64);
        z.next_in = (Bytef*)text.data(); z.avail_in = (uInt)text.size();
        z.next_out = out.data(); z.avail_out = (uInt)out.size();
        const int rc = deflate(&z, Z_FINISH);
        out.resize(z.total_out);
        deflateEnd(&z);
        return rc == Z_STREAM_END;
    }
    // merge_linearV2 (node2edge.c:430-609) for the walks of one range, ids starting after c.base
    bool apply(Chunk& c) {
        int id = c.base;
        for (const Cand& cd : c.cands) {
            id++;
            const int bal = cd.bal;
            // dislink2prevUncertain / dislink2nextUncertain on the two end nodes (other ranges may touch the same words)
            if (cd.last_smaller) clear_arc(cd.last->A, cd.prev_ch); else clear_arc(cd.last->B, cd.prev_ch ^ 2);
            if (cd.first_smaller) clear_arc(cd.first->B, cd.next_ch); else clear_arc(cd.first->A, cd.next_ch ^ 2);
            if (cd.len1) {
                const PatchVal v = cd.plus_smaller ? PatchVal{(uint32_t)id, (uint32_t)(bal + 1)} : PatchVal{(uint32_t)(id + bal), (uint32_t)(1 - bal)};
                c.patch.emplace_back(c.plus[cd.plus_idx], v);
            }
            for (uint32_t i = 0; i < cd.n_inner; i++) {
                const uintptr_t v = c.inner[cd.inner_off + i];
                HNode<NW>& n = *(HNode<NW>*)(v & ~(uintptr_t)1);
                const bool smaller = v & 1;
                const uint32_t twin = smaller ? (uint32_t)(bal + 1) : (uint32_t)(1 - bal);
                // a linear node can sit on one chain only -- which passes it twice, there and back, when the chain is its own reverse
                // complement (bal 0: a hairpin between one arc of a branch node and itself); both passes write the same tag
                if ((n.B >> B_INEDGE_SHIFT) & 3) {
                    if (bal == 0 && n.A == (uint32_t)id && ((n.B >> B_TWIN_SHIFT) & 3) == twin) continue;
                    return false;
                }
                n.A = smaller ? (uint32_t)id : (uint32_t)(id + bal);          // edge id replaces word A
                n.B = (n.B & 0x0FFFFFFFu) | (twin << B_TWIN_SHIFT) | (1u << B_INEDGE_SHIFT);
            }
            id += bal;
        }
        std::vector<uintptr_t>().swap(c.inner);
        std::vector<Kmer<NW>>().swap(c.plus);
        if (!c.text.empty() && !gz_member(c.text, c.gz)) return false;
        std::string().swap(c.text);
        return true;
    }

    int run(const std::string& path, int n_threads) {
        int nt = pick_threads(n_threads);
        if (nt < 1) nt = 1;
        std::vector<Chunk> chunks;
        const uint64_t STEP = 1 << 15;
        for (int si = 0; si < (int)g.sets.size(); si++)
            for (uint64_t lo = 0; lo < g.sets[si].size; lo += STEP) {
                chunks.emplace_back();
                chunks.back().set = si; chunks.back().lo = lo; chunks.back().hi = std::min<uint64_t>(g.sets[si].size, lo + STEP);
            }
        auto for_chunks = [&](const std::function<void(Chunk&, Walker&)>& fn) {
            std::atomic<size_t> next{0};
            auto body = [&]() {
                Walker w(g);
                for (;;) {
                    const size_t i = next.fetch_add(1);
                    if (i >= chunks.size()) break;
                    fn(chunks[i], w);
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body);
            body();
            for (auto& th : pool) th.join();
        };
        const bool verbose = pg::env_user("PG_HOST_VERBOSE") != nullptr;
        auto nowf = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double te0 = nowf();
        for_chunks([&](Chunk& c, Walker& w) { scan(w, c); });
        const double te1 = nowf();
        int base = 0;
        for (Chunk& c : chunks) { c.base = base; base += c.ids; records += (long long)c.cands.size(); extra_nodes += c.extra; }
        edge_c = base;
        std::atomic<int> failed{0};
        for_chunks([&](Chunk& c, Walker&) { if (!apply(c)) failed.store(1); });
        if (failed.load()) { pg_set_error("edge construction: inconsistent arcs or deflate failure (PG_SERIAL_EDGES=1 runs the sequential builder)"); return PG_EINVAL; }
        const double te2 = nowf();
        FILE* fp = fopen(path.c_str(), "wb");
        if (!fp) { pg_set_error("cannot open " + path); return PG_EIO; }
        bool any = false;
        for (Chunk& c : chunks) {
            for (auto& kv : c.patch) g.patch[kv.first] = kv.second;
            if (!c.gz.empty()) { any = true; if (fwrite(c.gz.data(), 1, c.gz.size(), fp) != c.gz.size()) { fclose(fp); pg_set_error("short write on " + path); return PG_EIO; } }
            std::vector<uint8_t>().swap(c.gz);
        }
        if (!any) {                                  // no edge at all: still a valid (empty) gzip file
            std::vector<uint8_t> e;
            gz_member(std::string(), e);
            fwrite(e.data(), 1, e.size(), fp);
        }
        fclose(fp);
        if (verbose) fprintf(stderr, "edges: walks %.2fs, tagging + deflate %.2fs, patch table + file %.2fs (%d threads)\n", te1 - te0, te2 - te1, nowf() - te2, nt);
        return PG_OK;
    }
};

// make_edge over all sets -> <prefix>.edge.gz; fills the counters of the stderr banner
template <int NW>
static int construct_edges(Graph<NW>& g, const std::string& prefix, int n_threads, int& edge_c, long long& records, long long& extra_nodes) {
    const char* serial = pg::env_test("PG_SERIAL_EDGES");
    if (serial && atoi(serial)) {
        GzText gz;
        if (!gz.open(prefix + ".edge.gz")) { pg_set_error("cannot open " + prefix + ".edge.gz"); return PG_EIO; }
        EdgeBuilder<NW> eb(g, gz);
        eb.run();
        gz.close();
        edge_c = eb.edge_c; records = eb.records; extra_nodes = eb.extra_nodes;
        return PG_OK;
    }
    ParallelEdgeBuilder<NW> eb(g);
    const int rc = eb.run(prefix + ".edge.gz", n_threads);
    edge_c = eb.edge_c; records = eb.records; extra_nodes = eb.extra_nodes;
    return rc;
}

// output_vertex (output_pregraph.c:50-86)
template <int NW>
static int write_vertex_file(Graph<NW>& g, const std::string& prefix, int& num_vt, bool quiet);
static int write_basic_file(const std::string& prefix, int num_vt, int K, int num_ed, int max_read_len) {
    FILE* fp = fopen((prefix + ".preGraphBasic").c_str(), "w");
    if (!fp) { pg_set_error("cannot open " + prefix + ".preGraphBasic"); return PG_EIO; }
    fprintf(fp, "VERTEX %d K %d\n", num_vt, K);
    fprintf(fp, "\nEDGEs %d\n", num_ed);
    fprintf(fp, "\nMaxReadLen %d MinReadLen %d MaxNameLen %d\n", max_read_len, 0, 256);
    fclose(fp);
    return PG_OK;
}
template <int NW>
static int write_vertex(Graph<NW>& g, const std::string& prefix, int num_ed, int max_read_len, int& num_vt) {
    int rc = write_vertex_file<NW>(g, prefix, num_vt, false);
    if (rc) return rc;
    return write_basic_file(prefix, num_vt, g.K, num_ed, max_read_len);
}
template <int NW>
static int write_vertex_file(Graph<NW>& g, const std::string& prefix, int& num_vt, bool quiet) {
    FILE* fp = fopen((prefix + ".vertex").c_str(), "w");
    if (!fp) { pg_set_error("cannot open " + prefix + ".vertex"); return PG_EIO; }
    std::vector<char> big(1 << 22);
    setvbuf(fp, big.data(), _IOFBF, big.size());
    // the slot ranges are scanned by all host threads: count the vertices per range first (the line break after every
    // eighth vertex depends on the running count), then format
    struct Range { int set; uint64_t lo, hi; long long n; std::string text; };
    std::vector<Range> ranges;
    const uint64_t STEP = 1 << 18;
    for (int si = 0; si < (int)g.sets.size(); si++)
        for (uint64_t lo = 0; lo < g.sets[si].size; lo += STEP) ranges.push_back(Range{si, lo, std::min<uint64_t>(g.sets[si].size, lo + STEP), 0, std::string()});
    const int nt = std::max(1, pick_threads(g.n_threads));
    auto for_ranges = [&](const std::function<void(Range&)>& fn) {
        std::atomic<size_t> next{0};
        auto body = [&]() { for (;;) { const size_t i = next.fetch_add(1); if (i >= ranges.size()) break; fn(ranges[i]); } };
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(body);
        body();
        for (auto& th : pool) th.join();
    };
    for_ranges([&](Range& r) {
        const HSet<NW>& s = g.sets[r.set];
        long long n = 0;
        for (uint64_t i = r.lo; i < r.hi; i++) n += s.occ[i] && !(s.array[i].B & (B_LINEAR | B_DELETED));
        r.n = n;
    });
    long long run = 0;
    std::vector<long long> before(ranges.size());
    for (size_t i = 0; i < ranges.size(); i++) { before[i] = run; run += ranges[i].n; }
    for_ranges([&](Range& r) {
        const HSet<NW>& s = g.sets[r.set];
        long long c = before[&r - ranges.data()];
        char tmp[128];
        r.text.reserve((size_t)r.n * (NW == 2 ? 34 : 68));
        for (uint64_t i = r.lo; i < r.hi; i++) {
            if (!s.occ[i]) continue;
            const HNode<NW>& n = s.array[i];
            if (n.B & (B_LINEAR | B_DELETED)) continue;
            c++;
            int len = fmt_kmer<NW>(tmp, n.seq, ' ');
            if (c % 8 == 0) tmp[len++] = '\n';
            r.text.append(tmp, (size_t)len);
        }
    });
    const int cnt = (int)run;
    for (Range& r : ranges)
        if (!r.text.empty()) fwrite(r.text.data(), 1, r.text.size(), fp);
    fputc('\n', fp);
    fclose(fp);
    if (!quiet) fprintf(stderr, "%d vertex(es) output.\n", cnt);
    num_vt = cnt;
    return PG_OK;
}

// <prefix>.vertex from the vertices' k-mers in slot order (the device lists them: p2_list_vertices), NW words each
template <int NW>
static int write_vertex_keys(const std::string& prefix, const std::vector<uint64_t>& keys, int n_threads, int& num_vt) {
    FILE* fp = fopen((prefix + ".vertex").c_str(), "w");
    if (!fp) { pg_set_error("cannot open " + prefix + ".vertex"); return PG_EIO; }
    const size_t n = keys.size() / NW;
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)pick_threads(n_threads), n / 65536 + 1));
    std::vector<std::string> text(nt);
    auto body = [&](int t) {
        std::string& out = text[t];
        const size_t lo = n * t / nt, hi = n * (t + 1) / nt;
        out.reserve((hi - lo) * (NW == 2 ? 34 : 68));
        char tmp[128];
        for (size_t i = lo; i < hi; i++) {
            Kmer<NW> k;
            for (int w = 0; w < NW; w++) k.w[w] = keys[i * NW + w];
            int len = fmt_kmer<NW>(tmp, k, ' ');
            if ((i + 1) % 8 == 0) tmp[len++] = '\n';
            out.append(tmp, (size_t)len);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
    body(0);
    for (auto& th : pool) th.join();
    bool ok = true;
    for (auto& tx : text) ok = ok && (tx.empty() || fwrite(tx.data(), 1, tx.size(), fp) == tx.size());
    fputc('\n', fp);
    fclose(fp);
    if (!ok) { pg_set_error("short write on " + prefix + ".vertex"); return PG_EIO; }
    num_vt = (int)n;
    return PG_OK;
}

// Replay put_kmerset / encap_kmerset slot placement for all sets (newhash.c:340-528): group the records by
// set, order each group by first-occurrence ordinal, insert in that order (sets in parallel).
template <int NW>
static int replay_layout(Graph<NW>& g, const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int K, int P,
                         int a_gb, int n_threads) {
    constexpr int RW = NW + 2;
    g.K = K; g.P = P; g.filter = kmer_filter<NW>(K); g.bias = set_bias((uint32_t)P); g.crc = host_crc_table();
    host_crc8_init();
    g.n_threads = n_threads;
    g.sets.clear();
    g.sets.resize(P);
    std::vector<uint64_t> per_set(P + 1, 0);
    // Records that already come in replay order -- by set, then by ordinal (pg_sort_records does that on the device) --
    // are inserted as they lie; anything else is bucketed and sorted here.
    bool presorted = true;
    {
        const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)pick_threads(n_threads), n / 65536 + 1));
        std::vector<std::vector<uint64_t>> cnt(nt, std::vector<uint64_t>(P + 1, 0));
        std::atomic<int> unsorted{0}, bad{0};
        auto body = [&](int t) {
            const uint64_t lo = n * t / nt, hi = n * (t + 1) / nt;
            uint64_t prev = lo ? records[(lo - 1) * RW + NW + 1] : 0;
            bool ok = true;
            for (uint64_t i = lo; i < hi; i++) {
                const uint64_t tag = records[i * RW + NW + 1];
                const uint64_t s = tag >> PG_ORD_BITS;
                if (s >= (uint64_t)P) { bad.store(1); return; }
                cnt[t][s + 1]++;
                ok = ok && tag >= prev;
                prev = tag;
            }
            if (!ok) unsorted.store(1);
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
        body(0);
        for (auto& th : pool) th.join();
        if (bad.load()) { pg_set_error("record with set id >= n_sets"); return PG_EINVAL; }
        presorted = !unsorted.load();
        for (int t = 0; t < nt; t++) for (int s = 0; s < P; s++) per_set[s + 1] += cnt[t][s + 1];
    }
    for (int s = 0; s < P; s++) per_set[s + 1] += per_set[s];
    struct Ref { uint64_t ord; uint64_t idx; };
    std::vector<Ref> order(presorted ? 0 : n);
    if (!presorted) {
        std::vector<uint64_t> cur(per_set.begin(), per_set.end() - 1);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t tag = records[i * RW + NW + 1];
            order[cur[tag >> PG_ORD_BITS]++] = Ref{tag & PG_ORD_MASK, i};
        }
    }
    const uint64_t init_size = ref_initial_set_size(a_gb, P, NW == 4);
    if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "replay: bucketing done\n");
    const bool verbose = pg::env_user("PG_HOST_VERBOSE") != nullptr;
    auto nowf = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    std::atomic<int> next{0}, pool_full{0};
    auto worker = [&]() {
        for (;;) {
            const int s = next.fetch_add(1);
            if (s >= P) break;
            std::vector<Ref> own;
            if (presorted) {                                  // the set's records lie in order: refer to them in place
                own.resize(per_set[s + 1] - per_set[s]);
                for (uint64_t i = per_set[s]; i < per_set[s + 1]; i++) own[i - per_set[s]] = Ref{records[i * RW + NW + 1] & PG_ORD_MASK, i};
            }
            Ref* lo = presorted ? own.data() : order.data() + per_set[s];
            Ref* hi = lo + (per_set[s + 1] - per_set[s]);
            const double ts0 = nowf();
            if (!presorted) {   // LSD radix sort on the ordinal, 16 bits a pass (ordinals are distinct within a set)
                const size_t cnt = (size_t)(hi - lo);
                uint64_t top = 0;
                for (Ref* r = lo; r != hi; ++r) top |= r->ord;
                std::vector<Ref> tmp(cnt);
                Ref* src = lo;
                Ref* dst = tmp.data();
                std::vector<size_t> hist(65536);
                for (int shift = 0; shift < 64 && (top >> shift); shift += 16) {
                    std::fill(hist.begin(), hist.end(), 0);
                    for (size_t i = 0; i < cnt; i++) hist[(src[i].ord >> shift) & 0xffff]++;
                    size_t run = 0;
                    for (size_t d = 0; d < 65536; d++) { const size_t c = hist[d]; hist[d] = run; run += c; }
                    for (size_t i = 0; i < cnt; i++) dst[hist[(src[i].ord >> shift) & 0xffff]++] = src[i];
                    std::swap(src, dst);
                }
                if (src != lo) memcpy((void*)lo, (const void*)src, cnt * sizeof(Ref));
            }
            const double ts1 = nowf();
            HSet<NW>& hs = g.sets[s];
            hs.init(init_size, HSet<NW>::final_size(init_size, (uint64_t)(hi - lo) + 1, a_gb != 0));
            // the inserts are strictly ordered, but their cache misses need not be: the record and the home slot of the
            // insert AHEAD steps further on are prefetched (a home computed for an outgrown size is simply recomputed)
            constexpr int AHEAD = 16;
            uint64_t ring_home[AHEAD], ring_size[AHEAD];
            for (int i = 0; i < AHEAD; i++) ring_size[i] = 0;
            const int64_t cnt = hi - lo;
            auto key_of = [&](const Ref* r) { Kmer<NW> k; const uint64_t* rec = records + r->idx * RW; for (int w = 0; w < NW; w++) k.w[w] = rec[w]; return k; };
            for (int64_t i = 0; i < std::min<int64_t>(cnt, 2 * AHEAD); i++) __builtin_prefetch(records + lo[i].idx * RW);
            for (int64_t i = 0; i < std::min<int64_t>(cnt, AHEAD); i++) {
                ring_home[i] = hs.home(key_of(lo + i)); ring_size[i] = hs.size; hs.prefetch_put(ring_home[i]);
            }
            for (int64_t i = 0; i < cnt; i++) {
                const Ref* r = lo + i;
                const uint64_t* rec = records + r->idx * RW;
                HNode<NW> nd;
                for (int w = 0; w < NW; w++) nd.seq.w[w] = rec[w];
                nd.A = (uint32_t)rec[NW];
                nd.B = (uint32_t)(rec[NW] >> 32);
                hs.before_put(a_gb != 0);
                if (hs.full) { pool_full.store(1); break; }
                const int slot = (int)(i % AHEAD);
                hs.put_new_at(nd, ring_size[slot] == hs.size ? ring_home[slot] : hs.home(nd.seq));
                if (i + 2 * AHEAD < cnt) __builtin_prefetch(records + lo[i + 2 * AHEAD].idx * RW);
                if (i + AHEAD < cnt) {
                    ring_home[slot] = hs.home(key_of(lo + i + AHEAD)); ring_size[slot] = hs.size; hs.prefetch_put(ring_home[slot]);
                }
            }
            // a duplicate put that arrived after the set's last new key still ran the growth test (newhash.c:477)
            if (lo != hi && set_last_put && set_last_put[s] > (hi - 1)->ord + 1) hs.before_put(a_gb != 0);
            if (verbose) fprintf(stderr, "replay set %d: %lld keys, sort %.2fs, inserts %.2fs (of which growing %.2fs)\n", s, (long long)(hi - lo), ts1 - ts0, nowf() - ts1, hs.t_grow);
        }
    };
    int nt = pick_threads(n_threads);
    nt = std::max(1, std::min(nt, P));
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    if (pool_full.load()) { pg_set_error("-- Static memory pool exploded, please define a larger value. --"); return PG_ENOMEM; }
    return PG_OK;
}

// The same replay for records that are still on the device, already in replay order (pg_sort_records): every set's
// worker pulls its stretch chunk by chunk through `fetch` (a device-to-host copy) and inserts while the other workers'
// copies are in flight, so neither a host copy of all records nor a separate download phase is needed.
typedef int (*pg_fetch_fn)(void* user, uint64_t first_record, uint64_t n_records, uint64_t* dst);
template <int NW>
static int replay_streamed(Graph<NW>& g, pg_fetch_fn fetch, void* user, uint64_t n, const uint64_t* per_set_count, const uint64_t* set_last_put,
                           int K, int P, int a_gb, int n_threads) {
    constexpr int RW = NW + 2;
    g.K = K; g.P = P; g.filter = kmer_filter<NW>(K); g.bias = set_bias((uint32_t)P); g.crc = host_crc_table();
    host_crc8_init();
    g.n_threads = n_threads;
    g.sets.clear();
    g.sets.resize(P);
    std::vector<uint64_t> first(P + 1, 0);
    for (int s = 0; s < P; s++) first[s + 1] = first[s] + per_set_count[s];
    if (first[P] != n) { pg_set_error("per-set counts do not add up to the record count"); return PG_EINVAL; }
    const uint64_t init_size = ref_initial_set_size(a_gb, P, NW == 4);
    const bool verbose = pg::env_user("PG_HOST_VERBOSE") != nullptr;
    auto nowf = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    std::atomic<int> next{0}, failed{0};
    auto worker = [&]() {
        const uint64_t CHUNK = (uint64_t)1 << 21;                           // records a copy (64 / 96 MiB)
        HugeArray<uint64_t> buf;
        for (;;) {
            const int s = next.fetch_add(1);
            if (s >= P) break;
            const double ts0 = nowf();
            double t_fetch = 0;
            HSet<NW>& hs = g.sets[s];
            const uint64_t cnt_all = per_set_count[s];
            hs.init(init_size, HSet<NW>::final_size(init_size, cnt_all + 1, a_gb != 0));
            // one buffer per worker, re-used from set to set: a later, larger set needs a larger one (the caller has the
            // old range page-locked, so it is told to let go first)
            if (cnt_all && buf.n < std::min(CHUNK, cnt_all) * RW + 8) {
                if (buf.p) fetch(user, 0, 0, nullptr);
                buf.reset(std::min(CHUNK, cnt_all) * RW + 8);
            }
            uint64_t last_ord = 0, prev_tag = 0;
            for (uint64_t at = 0; at < cnt_all && !failed.load(); at += CHUNK) {
                const int64_t cnt = (int64_t)std::min(CHUNK, cnt_all - at);
                const double tf0 = nowf();
                if (fetch(user, first[s] + at, (uint64_t)cnt, buf.data()) != PG_OK) { failed.store(1); break; }
                t_fetch += nowf() - tf0;
                const uint64_t* recs = buf.data();
                constexpr int AHEAD = 16;
                uint64_t ring_home[AHEAD], ring_size[AHEAD];
                for (int i = 0; i < AHEAD; i++) ring_size[i] = 0;
                auto key_of = [&](int64_t i) { Kmer<NW> k; for (int w = 0; w < NW; w++) k.w[w] = recs[i * RW + w]; return k; };
                for (int64_t i = 0; i < std::min<int64_t>(cnt, AHEAD); i++) { ring_home[i] = hs.home(key_of(i)); ring_size[i] = hs.size; hs.prefetch_put(ring_home[i]); }
                for (int64_t i = 0; i < cnt; i++) {
                    const uint64_t* rec = recs + i * RW;
                    const uint64_t tag = rec[NW + 1];
                    if ((tag >> PG_ORD_BITS) != (uint64_t)s || (tag < prev_tag && (at || i))) { failed.store(2); break; }   // not in replay order
                    prev_tag = tag;
                    HNode<NW> nd;
                    for (int w = 0; w < NW; w++) nd.seq.w[w] = rec[w];
                    nd.A = (uint32_t)rec[NW];
                    nd.B = (uint32_t)(rec[NW] >> 32);
                    hs.before_put(a_gb != 0);
                    if (hs.full) { failed.store(3); break; }
                    const int slot = (int)(i % AHEAD);
                    hs.put_new_at(nd, ring_size[slot] == hs.size ? ring_home[slot] : hs.home(nd.seq));
                    if (i + AHEAD < cnt) { ring_home[slot] = hs.home(key_of(i + AHEAD)); ring_size[slot] = hs.size; hs.prefetch_put(ring_home[slot]); }
                    last_ord = tag & PG_ORD_MASK;
                }
            }
            // a duplicate put that arrived after the set's last new key still ran the growth test (newhash.c:477)
            if (cnt_all && set_last_put && set_last_put[s] > last_ord + 1) hs.before_put(a_gb != 0);
            if (verbose) fprintf(stderr, "replay set %d: %llu keys, copies %.2fs, inserts %.2fs (of which growing %.2fs)\n", s, (unsigned long long)cnt_all, t_fetch,
                                 nowf() - ts0 - t_fetch, hs.t_grow);
        }
        fetch(user, 0, 0, nullptr);                                       // this thread will not ask again
    };
    int nt = pick_threads(n_threads);
    nt = std::max(1, std::min(nt, P));
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    if (failed.load() == 2) { pg_set_error("streamed records are not ordered by (set, ordinal)"); return PG_EINVAL; }
    if (failed.load() == 3) { pg_set_error("-- Static memory pool exploded, please define a larger value. --"); return PG_ENOMEM; }
    if (failed.load()) return PG_ENODEV;
    return PG_OK;
}

// After the n distinct keys of a set are in, one more put (a duplicate: nothing is inserted) still runs the growth test of
// newhash.c:477; it changes the layout exactly when the table would grow, i.e. when n sits at the threshold of its size.
extern "C" int pg_host_last_put_matters(const uint64_t* set_counts, int n_sets, int a_gb, int mer127) {
    if (!set_counts || a_gb != 0) return 0;                         // static pools never grow
    const uint64_t init = ref_initial_set_size(0, n_sets, mer127);
    for (int s = 0; s < n_sets; s++) {
        const uint64_t n = set_counts[s];
        if (n && HSet<2>::final_size(init, n + 1, false) != HSet<2>::final_size(init, n, false)) return 1;
    }
    return 0;
}

template <int NW>
static int layout_only(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int P, int a_gb, uint64_t* out_slot,
                       uint64_t* out_size) {
    constexpr int RW = NW + 2;
    Graph<NW> g;
    int rc = replay_layout<NW>(g, records, n, set_last_put, 13, P, a_gb, 0);
    if (rc) return rc;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t* rec = records + i * RW;
        Kmer<NW> k;
        for (int w = 0; w < NW; w++) k.w[w] = rec[w];
        HSet<NW>& hs = g.sets[rec[NW + 1] >> PG_ORD_BITS];
        out_slot[i] = (uint64_t)(hs.find(k) - hs.array.data());
    }
    if (out_size) for (int s = 0; s < P; s++) out_size[s] = g.sets[s].size;
    return PG_OK;
}

// ---- pass 2: read -> edge threading and pre-arcs (prlRead2edge, prlRead2path.c:786-1370) ----------------------
// Per read: every k-mer -> its node (chopKmer4read + searchKmer, prlRead2path.c:271-368); parse1read
// (prlRead2path.c:598-745) turns the node list into edge ids: a deleted node or a linear node outside any edge restarts
// the list while it has fewer than two items and ends it otherwise; a linear node contributes its (oriented) edge id
// once; two consecutive branch nodes contribute the (K+1)-mer joining them, resolved through the patch map to the id
// of the length-1 edge (search1kmerPlus, prlRead2path.c:558-596; a miss truncates the list).  Every adjacent pair
// (a, b) of the list then counts one pre-arc a -> b (thread_add1preArc, prlRead2path.c:388-403).
template <int NW>
struct ReadThreader {
    Graph<NW>& g;
    explicit ReadThreader(Graph<NW>& g_) : g(g_) {}

    struct Probe { Kmer<NW> key; uint64_t home; int set; bool smaller; };
    std::vector<Probe> probes;

    // what p2_walk_step sends out: (K+1)-mers to the patch map, pairs to `out`, the items to `ids` (for recordPathBin)
    struct Sink {
        Graph<NW>& g;
        std::vector<std::pair<uint32_t, uint32_t>>& out;
        std::vector<uint32_t>& ids;
        uint32_t kplus(const Kmer<NW>& plus, bool smaller) const {
            auto f = g.patch.find(plus);
            return f == g.patch.end() ? 0u : (smaller ? f->second.id : f->second.id + f->second.twin - 1);
        }
        void pair(uint32_t from, uint32_t to, int) const { out.emplace_back(from, to); }
        void item(int i, uint32_t id) const { if ((size_t)i >= ids.size()) ids.resize((size_t)i + 1); ids[i] = id; }
    };

    // appends the read's pairs (from, to) to `out`; returns false when the read yielded no usable item at all
    // (the reference's "read(s) deleted" counter, prlRead2path.c:722-725)
    // With `path` set (-R, prlRead2path.c:478-543 recordPathBin) the read's edge walk is also appended to *path as
    // <count:u8><count x u32 edge id> and every id on it to *marks, when its first three entries are resolved.
    bool thread_read(const uint8_t* codes, int len, std::vector<uint32_t>& ids, std::vector<std::pair<uint32_t, uint32_t>>& out,
                     std::vector<uint8_t>* path = nullptr, std::vector<uint32_t>* marks = nullptr) {
        const int K = g.K;
        // stage 1: every canonical k-mer of the read, its set and home slot; the slots are prefetched so that the
        // probes of stage 2 overlap their cache misses (chopKmer4read + searchKmer, prlRead2path.c:159-330)
        const int nk = len - K + 1;
        if ((int)probes.size() < nk) probes.resize(nk);
        {
            Kmer<NW> word, bal;
            for (int i = 0; i < NW; i++) word.w[i] = 0;
            for (int i = 0; i < K - 1; i++) word = kmer_next<NW>(word, codes[i], g.filter);
            bal = kmer_rc<NW>(word, K - 1);                       // reverse complement of the first K - 1 bases
            const int top = 2 * (K - 1), tw = NW - 1 - top / 64, ts = top % 64;
            for (int j = 0; j < nk; j++) {
                const int c = codes[j + K - 1];
                word = kmer_next<NW>(word, c, g.filter);
                if (j) bal = kmer_shr<NW>(bal, 2);
                bal.w[tw] |= (uint64_t)(c ^ 2) << ts;
                Probe& pr = probes[j];
                pr.smaller = kmer_less<NW>(word, bal);
                pr.key = pr.smaller ? word : bal;
                pr.set = g.set_of(pr.key);
                pr.home = g.sets[pr.set].home(pr.key);
                g.sets[pr.set].prefetch(pr.home);
            }
        }
        // stage 2: parse1read over the nodes (p2_walk.hpp)
        P2Walk<NW> w;
        Sink sink{g, out, ids};
        for (int j = 0; j < nk && !w.stop; j++) {
            const Probe& pr = probes[j];
            const HNode<NW>* node = g.sets[pr.set].find_from(pr.key, pr.home);
            if (!node) { fprintf(stderr, "SearchKmer: kmer is not found.\n"); exit(1); }
            p2_walk_step<NW>(w, pr.key, pr.smaller, (uint64_t)node->A | (uint64_t)node->B << 32, K, sink);
        }
        const P2WalkEnd end = p2_walk_end<NW>(w);
        if (path && end.walk) {
            // the reference counts with an unsigned char that also indexes its staging buffer, so a walk longer than
            // 255 entries wraps around and overwrites the front (prlRead2path.c:481, 529)
            uint32_t buf[256];
            uint8_t counter = 0;
            for (int i = 0; i < end.walk; i++) {
                buf[counter++] = ids[i];
                marks->push_back(ids[i]);
            }
            path->push_back(counter);
            const uint8_t* b = reinterpret_cast<const uint8_t*>(buf);
            path->insert(path->end(), b, b + 4 * (size_t)counter);
        }
        return !end.deleted;
    }
};

// pre-arc lists: new targets go to the head of their source's list (prlRead2path.c:388-403), output walks from the
// head (output_arcs, prlRead2path.c:426-476)
struct PreArcs {
    // The order of a list depends only on the order in which the pairs of its own source edge arrive, so the source
    // edges are cut into NP contiguous ranges that are folded independently (each range owns its pools).
    static constexpr int NP = 64;
    struct Pool { std::vector<uint32_t> to, mult, next; long long count = 0; };
    std::vector<uint32_t> head;            // per from-edge, index + 1 into its range's pools, 0 = empty
    Pool pool[NP];
    uint64_t n_from = 1;
    void init(uint32_t num_ed) { head.assign((size_t)num_ed + 1, 0); n_from = (uint64_t)num_ed + 1; }
    int part_of(uint32_t from) const { return (int)((uint64_t)from * NP / n_from); }
    void add(Pool& p, uint32_t from, uint32_t t) {
        for (uint32_t i = head[from]; i; i = p.next[i - 1])
            if (p.to[i - 1] == t) { p.mult[i - 1]++; return; }
        p.to.push_back(t); p.mult.push_back(1); p.next.push_back(head[from]);
        head[from] = (uint32_t)p.to.size();
        p.count++;
    }
    long long count() const { long long c = 0; for (const Pool& p : pool) c += p.count; return c; }
    int write(const std::string& path) const {
        FILE* fp = fopen(path.c_str(), "w");
        if (!fp) { pg_set_error("cannot open " + path); return PG_EIO; }
        std::vector<char> big(1 << 22);
        setvbuf(fp, big.data(), _IOFBF, big.size());
        for (size_t e = 1; e < head.size(); e++) {
            if (!head[e]) continue;
            const Pool& p = pool[part_of((uint32_t)e)];
            fprintf(fp, "%u", (unsigned)e);
            for (uint32_t i = head[e]; i; i = p.next[i - 1]) fprintf(fp, " %u %u", p.to[i - 1], p.mult[i - 1]);
            fputc('\n', fp);
        }
        fclose(fp);
        return PG_OK;
    }
};

// The graph kept alive between edge construction and pass 2.
struct GraphHandleBase {
    virtual ~GraphHandleBase() {}
    virtual void shutdown() = 0;
    virtual int add_reads(const uint8_t* codes, const int32_t* lens, uint64_t n, uint64_t stride, int n_threads) = 0;
    virtual int add_packed(const uint64_t* words, const int32_t* lens, uint64_t n, int n_threads) = 0;
    virtual int add_packed_device(const uint64_t* d_words, uint64_t n, int read_len, int device) = 0;
    virtual int add_packed_device_segments(const uint64_t* const* d_segs, const uint64_t* seg_reads, int n_segs, int read_len, int device) = 0;
    virtual int add_packed_device_ragged(const uint64_t* d_words, const uint64_t* d_word_off, const uint64_t* d_kmer_base, uint64_t n, uint64_t n_kmers, int max_len, int device) = 0;
    virtual int finish(long long* n_arcs) = 0;
    virtual int resolve_repeats(int on) = 0;
    virtual int use_device(int device) = 0;
    int num_vt = 0, num_ed = 0;
};

template <int NW>
struct GraphHandle : GraphHandleBase {
    Graph<NW> g;
    PreArcs arcs;
    std::string prefix;
    int max_read_len = 0;
    long long reads_seen = 0, reads_deleted = 0;
    // -R (pregraph.c:181-184): <prefix>.path is appended batch by batch, the per-edge marker counts go to
    // <prefix>.markOnEdge at the end (prlRead2path.c:813-818, 435-449)
    FILE* path_fp = nullptr;
    std::vector<uint8_t> marker;
    long long mark_count = 0;
    double t_thread = 0, t_fold = 0;
    struct Scratch {
        std::unique_ptr<ReadThreader<NW>> rt;
        std::vector<uint32_t> items;
        std::vector<std::pair<uint32_t, uint32_t>> pairs, sorted;
        std::vector<uint32_t> marks;
        std::vector<uint8_t> unpacked, path;
        size_t off[PreArcs::NP + 1];
        long long deleted = 0, marked = 0;
    };
    std::vector<Scratch> scratch;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

    // pass 2 on a HIP device (graph_kernels.hip) instead of the host threads
    bool dev_on = false;
    int dev_id = 0;
    P2Device* dev = nullptr;
    std::vector<uint32_t> dev_walks;
    std::vector<uint16_t> dev_walk_len;

    ~GraphHandle() override { shutdown(); }
    // everything but the memory: threads, files, the device copy
    void shutdown() override {
        // a graph given up before finish(): the edge writer's verdict has no caller to go to any more -- say it at least
        if (join_edge_writer() != PG_OK) fprintf(stderr, "%s.edge.gz was not written: %s\n", prefix.c_str(), edge_err.c_str());
        if (vertex_thread.joinable()) vertex_thread.join();
        if (path_fp) { fclose(path_fp); path_fp = nullptr; }
        if (dev) { p2_destroy(dev); dev = nullptr; }
    }
    int use_device(int device) override {
        if (dev_edges) {                             // the sets live on the device, tagged there: pass 2 stays there
            if (device == dev_id) return PG_OK;
            pg_set_error("the edges were built on another device");
            return PG_ESTATE;
        }
        if (dev) { pg_set_error("pass 2 already started"); return PG_ESTATE; }
        dev_on = device >= 0; dev_id = device;
        return PG_OK;
    }
    int max_nk() const { return std::max(1, max_read_len - g.K + 1); }
    // edges on the device (graph_kernels.hip: eb_*): upload the sets, build, then format output_1edge's text here
    // the k-mer sets into HBM as they are now (after the layout replay: the tips then walk on the device copy)
    std::vector<int> set_devices;                // sharded run: the HIP device every set lives on (empty: all on dev_id)
    std::vector<int> lane_devices;               // sharded run: the ranks' devices, lane 0 = the lead (graph_kernels.hip: P2Lane)
    int dev_open(int device) {
        dev_on = true; dev_id = device;
        P2Sets sets;
        g.set_base.assign((size_t)g.P + 1, 0);
        for (int si = 0; si < g.P; si++) {
            sets.nodes[si] = g.sets[si].array.data(); sets.size[si] = g.sets[si].size;
            g.set_base[si + 1] = g.set_base[si] + g.sets[si].size;
        }
        dev = p2_open(dev_id, g.K, NW, g.P, sets, max_nk(), set_devices.empty() ? nullptr : set_devices.data());
        if (!dev) return PG_ENODEV;
        if (lane_devices.size() > 1 && lane_devices[0] == dev_id && p2_use_lanes(dev, lane_devices.data(), (int)lane_devices.size()) != PG_OK) { p2_destroy(dev); dev = nullptr; return PG_ENODEV; }
        g.tip_dev = dev;
        return PG_OK;
    }
    int dev_build_edges(int device, int n_threads, int& edge_c, long long& records_c, long long& extra_nodes) {
        const double tv0 = now();
        start_vertex_writer();
        if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "vertex list from the device: %.2fs\n", now() - tv0);
        if (!dev) { const int rc0 = dev_open(device); if (rc0) return rc0; }
        g.tip_dev = nullptr;                         // the device copy is about to be tagged: no more tip walks on it
        P2Edges ed;
        const double te0 = now();
        int rc = p2_build_edges(dev, ed);
        if (rc) return rc;
        const double te1 = now();
        edge_c = (int)ed.n_ids; records_c = (long long)ed.recs.size(); extra_nodes = ed.n_len1;
        dev_edges = true;
        // <prefix>.edge.gz is text made from what the device handed back; nothing that follows reads it.  A caller that said so
        // (pg_host_edge_file_in_background: call_pregraph) gets it written beside pass 2 and waits for it in finish.
        if (g_edge_file_in_background) {
            auto* held = new P2Edges(std::move(ed));
            edge_started = true;
            edge_thread = std::thread([this, held, n_threads, te0, te1] {
                edge_rc = write_edge_file(*held, n_threads, te0, te1);
                if (edge_rc) edge_err = pg_last_error();
                delete held;
            });
            return PG_OK;
        }
        return write_edge_file(ed, n_threads, te0, te1);
    }
    std::thread edge_thread;
    bool edge_started = false;
    int edge_rc = PG_OK;
    std::string edge_err;
    int join_edge_writer() {
        if (!edge_started) return PG_OK;
        const double tw0 = now();
        if (edge_thread.joinable()) edge_thread.join();
        if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "finish: waited %.2fs for the edge file\n", now() - tw0);
        edge_started = false;
        if (edge_rc) pg_set_error(edge_err);
        return edge_rc;
    }
    int write_edge_file(const P2Edges& ed, int n_threads, double te0, double te1) {
        // text records, one gzip member per range of edges, formatted and deflated by all host threads
        const size_t STEP = 1 << 15, n_chunks = (ed.recs.size() + STEP - 1) / STEP;
        std::vector<std::vector<uint8_t>> gz(n_chunks);
        std::atomic<size_t> next{0};
        std::atomic<int> failed{0};
        auto body = [&]() {
            std::string text;
            for (;;) {
                const size_t c = next.fetch_add(1);
                if (c >= n_chunks) break;
                text.clear();
                for (size_t i = c * STEP; i < std::min(ed.recs.size(), (c + 1) * STEP); i++) {
                    const P2EdgeRec& r = ed.recs[i];
                    const int length = (int)r.length;
                    int cvg = 0;
                    if (length > 1) { long long v = (long long)(r.sum / (unsigned long long)(length - 1)) * 10; cvg = v > 16000 ? 16000 : (int)v; }
                    Kmer<NW> fk, lk;
                    for (int k = 0; k < NW; k++) { fk.w[k] = r.first_kmer[k]; lk.w[k] = r.last_kmer[k]; }
                    char head[256];
                    int n = sprintf(head, ">length %d,", length);
                    n += fmt_kmer<NW>(head + n, fk, ',');
                    n += fmt_kmer<NW>(head + n, lk, ',');
                    n += sprintf(head + n, "cvg %d, %d\n", cvg, (int)r.bal);
                    text.append(head, n);
                    const char* b = ed.text.data() + r.text_off;
                    for (int at = 0; at < length; at += 100) {
                        text.append(b + at, (size_t)std::min(100, length - at));
                        text.push_back('\n');
                    }
                }
                if (!text.empty() && !ParallelEdgeBuilder<NW>::gz_member(text, gz[c])) failed.store(1);
            }
        };
        {
            const int nt = std::max(1, pick_threads(n_threads));
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body);
            body();
            for (auto& th : pool) th.join();
        }
        if (failed.load()) { pg_set_error("deflate failed"); return PG_EIO; }
        FILE* fp = fopen((prefix + ".edge.gz").c_str(), "wb");
        if (!fp) { pg_set_error("cannot open " + prefix + ".edge.gz"); return PG_EIO; }
        bool any = false;
        for (auto& m : gz)
            if (!m.empty()) { any = true; if (fwrite(m.data(), 1, m.size(), fp) != m.size()) { fclose(fp); pg_set_error("short write on " + prefix + ".edge.gz"); return PG_EIO; } }
        if (!any) { std::vector<uint8_t> e; ParallelEdgeBuilder<NW>::gz_member(std::string(), e); fwrite(e.data(), 1, e.size(), fp); }
        fclose(fp);
        if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "edges: device (walk, sort, tag, download) %.2fs, text + deflate + file %.2fs\n", te1 - te0, now() - te1);
        return PG_OK;
    }
    bool dev_edges = false;
    // with the edges on the device nothing changes the host copy of the sets after the tips: <prefix>.vertex is written
    // by a background thread while the GPU builds edges and threads reads
    std::thread vertex_thread;
    int vertex_rc = PG_OK, vertex_count = 0;
    bool vertex_started = false;
    bool sets_on_device_only = false;            // tips were clipped on the device: the host copy of the sets (if any) is stale
    std::vector<uint64_t> vertex_keys;
    int dev_clip_tips(bool cut_single) {
        const int cut = 2 * g.K;
        P2TipTotals tot;
        const double t0 = now();
        const int rc = p2_clip_tips(dev, cut_single, tot);
        if (rc) return rc;
        // the reference's banner (cutTipPreGraph.c:363-399, 414-488)
        if (cut_single) {
            fprintf(stderr, "Start to remove frequency-one-kmer tips shorter than %d.\n", cut);
            fprintf(stderr, "Total %llu tip(s) removed.\n", tot.single);
        }
        fprintf(stderr, "Start to remove tips with minority links.\n");
        for (size_t i = 0; i < tot.per_cycle.size(); i++) fprintf(stderr, "%llu tip(s) removed in cycle %d.\n", tot.per_cycle[i], (int)i + 1);
        fprintf(stderr, "Total %llu tip(s) removed.\n", tot.minor);
        if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "tips decided on the device: %d scan(s), %d fixed-point round(s), %.2fs\n", (int)tot.per_cycle.size() + (cut_single ? 1 : 0), tot.rounds, now() - t0);
        sets_on_device_only = true;
        g.tip_dev = nullptr;
        return PG_OK;
    }
    void start_vertex_writer() {
        vertex_started = true;
        if (sets_on_device_only) {
            vertex_rc = p2_list_vertices(dev, vertex_keys);
            if (vertex_rc) return;
            vertex_thread = std::thread([this]() {
                const double tv0 = now();
                vertex_rc = write_vertex_keys<NW>(prefix, vertex_keys, g.n_threads, vertex_count);
                std::vector<uint64_t>().swap(vertex_keys);
                if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "vertex writer: %.2fs (beside the edges)\n", now() - tv0);
            });
            return;
        }
        vertex_thread = std::thread([this]() {
            const double tv0 = now();
            vertex_rc = write_vertex_file<NW>(g, prefix, vertex_count, true);
            if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "vertex writer: %.2fs (beside the edges)\n", now() - tv0);
        });
    }
    // (Releasing the host copy of the sets as soon as <prefix>.vertex is written -- nothing reads it after that in device mode --
    // was tried, beside the edge text and beside pass 2: an munmap of tens of gigabytes holds the address-space lock for over a
    // second, and whatever else allocates, frees or page-faults meanwhile waits for it; the stage it ran beside grew by as much
    // as the end of the process shrank.)
    int dev_begin() {
        if (dev_ready) return PG_OK;
        if (dev) {                                   // opened for the edges: the (K+1)-mer table is on the device already
            int rc = p2_begin_reads(dev, (uint32_t)num_ed, path_fp != nullptr);
            if (rc == PG_OK) dev_ready = true;
            return rc;
        }
        P2Sets sets;
        for (int si = 0; si < g.P; si++) { sets.nodes[si] = g.sets[si].array.data(); sets.size[si] = g.sets[si].size; }
        // KmerSetsPatch as an open-addressing table the device can probe
        uint64_t cap = 1024;
        while (cap < 2 * (uint64_t)g.patch.size() + 2) cap <<= 1;
        std::vector<uint64_t> keys(cap * NW, 0);
        std::vector<uint32_t> val(cap * 2, 0);
        for (auto& kv : g.patch) {
            uint64_t h = kmer_mix<NW>(kv.first) & (cap - 1);
            while (val[2 * h]) h = (h + 1) & (cap - 1);
            for (int w = 0; w < NW; w++) keys[h * NW + w] = kv.first.w[w];
            val[2 * h] = kv.second.id; val[2 * h + 1] = kv.second.twin;
        }
        dev = p2_create(dev_id, g.K, NW, g.P, sets, keys.data(), val.data(), cap, (uint32_t)num_ed, max_nk(), path_fp != nullptr);
        if (dev) dev_ready = true;
        return dev ? PG_OK : PG_ENODEV;
    }
    bool dev_ready = false;
    // reads already packed: straight to the device, in slices when the walks have to come back (-R)
    int dev_add_packed(const uint64_t* words, const int32_t* lens, uint64_t n) {
        const double t0 = now();
        int rc = dev_begin();
        if (rc) return rc;
        const bool reps = path_fp != nullptr;
        const int mnk = max_nk();
        std::vector<uint64_t> off(n + 1, 0);
        for (uint64_t r = 0; r < n; r++) {
            if (lens[r] - g.K + 1 > mnk) { pg_set_error("a read is longer than the maximum read length given at pg_host_graph_begin"); return PG_EINVAL; }
            off[r + 1] = off[r] + ((uint64_t)std::max(lens[r], 0) + 31) / 32;
        }
        const uint64_t step = reps ? std::max<uint64_t>(1, ((uint64_t)64 << 20) / (uint64_t)mnk) : n;
        for (uint64_t lo = 0; lo < n; lo += step) {
            const uint64_t m = std::min(step, n - lo);
            std::vector<uint64_t> rel;
            const uint64_t* offp = off.data() + lo;
            if (lo) { rel.resize(m); for (uint64_t i = 0; i < m; i++) rel[i] = off[lo + i] - off[lo]; offp = rel.data(); }
            if (reps) {
                if (dev_walks.size() < m * (size_t)mnk) dev_walks.resize(m * (size_t)mnk);
                if (dev_walk_len.size() < m) dev_walk_len.resize(m);
            }
            rc = p2_add_packed(dev, words + off[lo], offp, lens + lo, m, off[lo + m] - off[lo], reps ? dev_walks.data() : nullptr,
                               reps ? dev_walk_len.data() : nullptr);
            if (rc) return rc;
            if (reps) {                              // recordPathBin's record format, with its one-byte counter (prlRead2path.c:478-543)
                std::vector<uint8_t> bytes;
                for (uint64_t r = 0; r < m; r++) {
                    const int upto = dev_walk_len[r];
                    if (!upto) continue;
                    const uint32_t* row = dev_walks.data() + r * (size_t)mnk;
                    uint32_t buf[256];
                    uint8_t counter = 0;
                    for (int i = 0; i < upto; i++) buf[counter++] = row[i];
                    bytes.push_back(counter);
                    const uint8_t* b = reinterpret_cast<const uint8_t*>(buf);
                    bytes.insert(bytes.end(), b, b + 4 * (size_t)counter);
                }
                if (!bytes.empty() && fwrite(bytes.data(), 1, bytes.size(), path_fp) != bytes.size()) { pg_set_error("short write on " + prefix + ".path"); return PG_EIO; }
            }
        }
        reads_seen += (long long)n;
        t_thread += now() - t0;
        return PG_OK;
    }
    int dev_finish() {
        const double t0 = now();
        int rc = dev_begin();                        // no read at all: still an (empty) result
        if (rc) return rc;
        P2Result res;
        rc = p2_finish(dev, res);
        if (rc) return rc;
        const double t_dev = now();
        reads_deleted = res.reads_deleted;
        mark_count = res.markers;
        const int nt = std::max(1, pick_threads(0));
        std::vector<std::string> text(nt);
        std::vector<size_t> merged_n(nt, 0);
        if (res.folded) {
            // folded on the device: (from, to, multiplicity) in file order; the host threads print ranges cut where the source edge changes
            const size_t n = res.folded3.size() / 3;
            const uint32_t* a3 = res.folded3.data();
            std::vector<size_t> cut(nt + 1, n);
            cut[0] = 0;
            for (int t = 1; t < nt; t++) {
                size_t i = std::max(cut[t - 1], n * (size_t)t / nt);
                while (i < n && i > 0 && a3[3 * i] == a3[3 * (i - 1)]) i++;
                cut[t] = i;
            }
            auto body3 = [&](int t) {
                // (a raw buffer of the worst-case size, pointer writes, two digits a division: push_back a character and a division a digit were 0.26 s
                //  of the 0.42 s the fold took at 26 M pre-arcs)
                static const char D2[201] = "0001020304050607080910111213141516171819202122232425262728293031323334353637383940414243444546474849"
                                            "5051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
                std::string& out = text[t];
                const size_t n_t = cut[t + 1] - cut[t];
                out.resize(n_t * 33 + 16);
                char* const base = &out[0];
                char* p = base;
                auto put = [&](uint32_t v) {
                    char tmp[10];
                    int k = 10;
                    while (v >= 100) { const uint32_t q = v / 100, r2 = v - q * 100; v = q; tmp[--k] = D2[2 * r2 + 1]; tmp[--k] = D2[2 * r2]; }
                    if (v >= 10) { tmp[--k] = D2[2 * v + 1]; tmp[--k] = D2[2 * v]; } else tmp[--k] = (char)('0' + v);
                    memcpy(p, tmp + k, (size_t)(10 - k));
                    p += 10 - k;
                };
                for (size_t i = cut[t]; i < cut[t + 1];) {
                    const uint32_t from = a3[3 * i];
                    put(from);
                    for (; i < cut[t + 1] && a3[3 * i] == from; ++i) { *p++ = ' '; put(a3[3 * i + 1]); *p++ = ' '; put(a3[3 * i + 2]); }
                    *p++ = '\n';
                }
                out.resize((size_t)(p - base));
                merged_n[t] = n_t;
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body3, t);
            body3(0);
            for (auto& th : pool) th.join();
        } else {
        // a list shows its targets latest first-met first (prlRead2path.c:388-403, 443-467); the source edges are cut
        // into ranges that are sorted and printed by all host threads
        const uint64_t n_from = (uint64_t)num_ed + 1;
        std::vector<size_t> start(nt + 1, 0);
        for (const P2Arc& a : res.arcs) start[(size_t)((uint64_t)a.from * nt / n_from) + 1]++;
        for (int t = 0; t < nt; t++) start[t + 1] += start[t];
        std::vector<P2Arc> sorted(res.arcs.size());
        {
            std::vector<size_t> cur(start.begin(), start.end() - 1);
            for (const P2Arc& a : res.arcs) sorted[cur[(size_t)((uint64_t)a.from * nt / n_from)]++] = a;
        }
        const bool merge = res.lanes > 1;
        auto body = [&](int t) {
            P2Arc* lo = sorted.data() + start[t];
            P2Arc* hi = sorted.data() + start[t + 1];
            if (merge) {
                // several lanes threaded the reads: a (from, to) pair may have an entry from each -- multiplicities add up, the first
                // meeting is the earliest (thread_add1preArc counts and keeps the list order of the first insertion, prlRead2path.c:388-403)
                std::sort(lo, hi, [](const P2Arc& a, const P2Arc& b) { return a.from != b.from ? a.from < b.from : a.to < b.to; });
                P2Arc* w = lo;
                for (P2Arc* a = lo; a != hi; ++a) {
                    if (w != lo && w[-1].from == a->from && w[-1].to == a->to) { w[-1].mult += a->mult; w[-1].first = std::min(w[-1].first, a->first); }
                    else *w++ = *a;
                }
                hi = w;
            }
            merged_n[t] = (size_t)(hi - lo);
            std::sort(lo, hi, [](const P2Arc& a, const P2Arc& b) { return a.from != b.from ? a.from < b.from : a.first > b.first; });
            std::string& out = text[t];
            out.reserve((size_t)(hi - lo) * 12);
            char tmp[16];
            auto put = [&](uint32_t v) { int n = 0; do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) out.push_back(tmp[--n]); };
            for (P2Arc* a = lo; a != hi;) {
                const uint32_t from = a->from;
                put(from);
                for (; a != hi && a->from == from; ++a) { out.push_back(' '); put(a->to); out.push_back(' '); put(a->mult); }
                out.push_back('\n');
            }
        };
        {
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
            body(0);
            for (auto& th : pool) th.join();
        }
        }
        const double t_text = now();
        {   // every thread writes its own stretch of the file (the offsets are the prefix sums of the text sizes)
            const int fd = open((prefix + ".preArc").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fd < 0) { pg_set_error("cannot open " + prefix + ".preArc"); return PG_EIO; }
            std::vector<size_t> off(nt + 1, 0);
            for (int t = 0; t < nt; t++) off[t + 1] = off[t] + text[t].size();
            std::atomic<int> bad{0};
            auto wr = [&](int t) {
                size_t done = 0;
                while (done < text[t].size()) {
                    const ssize_t w = pwrite(fd, text[t].data() + done, text[t].size() - done, (off_t)(off[t] + done));
                    if (w <= 0) { bad.store(1); return; }
                    done += (size_t)w;
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(wr, t);
            wr(0);
            for (auto& th : pool) th.join();
            if (close(fd) != 0 || bad.load()) { pg_set_error("short write on " + prefix + ".preArc"); return PG_EIO; }
        }
        if (pg::env_user("PG_HOST_VERBOSE"))
            fprintf(stderr, "pre-arcs: %s, table read out + sorted + downloaded %.2fs, text %.2fs, file %.2fs\n", res.folded ? "folded on the device" : "folded on the host", t_dev - t0, t_text - t_dev, now() - t_text);
        dev_arc_count = 0;
        for (int t = 0; t < nt; t++) dev_arc_count += (long long)merged_n[t];
        if (path_fp) for (size_t e = 0; e < marker.size() && e < res.marker.size(); e++) marker[e] = (uint8_t)std::min(255u, res.marker[e]);
        t_fold += now() - t0;
        return PG_OK;
    }
    long long dev_arc_count = 0;
    int resolve_repeats(int on) override {
        if (path_fp) { fclose(path_fp); path_fp = nullptr; }
        marker.clear();
        if (!on) return PG_OK;
        path_fp = fopen((prefix + ".path").c_str(), "wb");
        if (!path_fp) { pg_set_error("cannot open " + prefix + ".path"); return PG_EIO; }
        marker.assign((size_t)num_ed + 1, 0);
        return PG_OK;
    }

    int add_reads(const uint8_t* codes, const int32_t* lens, uint64_t n, uint64_t stride, int n_threads) override {
        if (dev_on) {                                // pack (pg_pack_read's layout) with the host threads, thread on the device
            std::vector<int32_t> ls(n);
            std::vector<uint64_t> off(n + 1, 0);
            for (uint64_t r = 0; r < n; r++) { ls[r] = lens ? lens[r] : (int32_t)stride; off[r + 1] = off[r] + ((uint64_t)std::max(ls[r], 0) + 31) / 32; }
            std::vector<uint64_t> words(off[n] + 1, 0);
            const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)pick_threads(n_threads), (n + 4095) / 4096));
            auto body = [&](int t) {
                for (uint64_t r = n * t / nt; r < n * (t + 1) / nt; r++) {
                    const uint8_t* c = codes + r * stride;
                    uint64_t* w = words.data() + off[r];
                    for (int i = 0; i < ls[r]; i++) w[i >> 5] |= (uint64_t)(c[i] & 3) << (62 - 2 * (i & 31));
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(body, t);
            body(0);
            for (auto& th : pool) th.join();
            return dev_add_packed(words.data(), ls.data(), n);
        }
        return add_any(n, n_threads, [&](uint64_t r, std::vector<uint8_t>&, int& len) -> const uint8_t* {
            len = lens ? lens[r] : (int)stride;
            return codes + r * stride;
        });
    }
    // reads packed 2 bits a base, 32 bases a word, first base in the top bits (pg_pack_read), back to back
    // reads that pass 1 left on the device (one length, back to back): threaded where they are
    int add_packed_device(const uint64_t* d_words, uint64_t n, int read_len, int device) override {
        if (!dev_on) { pg_set_error("pg_graph_add_packed_device: the graph is not on a device (pg_graph_use_device first)"); return PG_ESTATE; }
        if (path_fp) { pg_set_error("pg_graph_add_packed_device: not with -R (the walks come back through the host path)"); return PG_ESTATE; }
        if (read_len - g.K + 1 > max_nk()) { pg_set_error("a read is longer than the maximum read length given at pg_host_graph_begin"); return PG_EINVAL; }
        const double t0 = now();
        int rc = dev_begin();
        if (rc) return rc;
        rc = p2_add_packed_device(dev, d_words, n, read_len, device);      // (a lane of the graph on that device, or an error)
        if (rc) return rc;
        reads_seen += (long long)n;
        t_thread += now() - t0;
        return PG_OK;
    }
    int add_packed_device_segments(const uint64_t* const* d_segs, const uint64_t* seg_reads, int n_segs, int read_len, int device) override {
        if (!dev_on) { pg_set_error("pg_graph_add_packed_device_segments: the graph is not on a device (pg_graph_use_device first)"); return PG_ESTATE; }
        if (path_fp) { pg_set_error("pg_graph_add_packed_device_segments: not with -R (the walks come back through the host path)"); return PG_ESTATE; }
        if (read_len - g.K + 1 > max_nk()) { pg_set_error("a read is longer than the maximum read length given at pg_host_graph_begin"); return PG_EINVAL; }
        const double t0 = now();
        int rc = dev_begin();
        if (rc) return rc;
        rc = p2_add_packed_device_segments(dev, d_segs, seg_reads, n_segs, read_len, device);
        if (rc) return rc;
        for (int q = 0; q < n_segs; q++) reads_seen += (long long)seg_reads[q];
        t_thread += now() - t0;
        return PG_OK;
    }
    int add_packed_device_ragged(const uint64_t* d_words, const uint64_t* d_word_off, const uint64_t* d_kmer_base, uint64_t n, uint64_t n_kmers, int max_len, int device) override {
        if (!dev_on) { pg_set_error("pg_graph_add_packed_device_ragged: the graph is not on a device (pg_graph_use_device first)"); return PG_ESTATE; }
        if (path_fp) { pg_set_error("pg_graph_add_packed_device_ragged: not with -R (the walks come back through the host path)"); return PG_ESTATE; }
        if (max_len - g.K + 1 > max_nk()) { pg_set_error("a read is longer than the maximum read length given at pg_host_graph_begin"); return PG_EINVAL; }
        const double t0 = now();
        int rc = dev_begin();
        if (rc) return rc;
        rc = p2_add_packed_device_ragged(dev, d_words, d_word_off, d_kmer_base, n, n_kmers, device);
        if (rc) return rc;
        reads_seen += (long long)n;
        t_thread += now() - t0;
        return PG_OK;
    }
    int add_packed(const uint64_t* words, const int32_t* lens, uint64_t n, int n_threads) override {
        if (dev_on) return dev_add_packed(words, lens, n);
        std::vector<uint64_t> off(n + 1, 0);
        for (uint64_t r = 0; r < n; r++) off[r + 1] = off[r] + ((uint64_t)lens[r] + 31) / 32;
        return add_any(n, n_threads, [&](uint64_t r, std::vector<uint8_t>& buf, int& len) -> const uint8_t* {
            len = lens[r];
            if ((int)buf.size() < len + 32) buf.resize((size_t)len + 32);
            const uint64_t* w = words + off[r];
            for (int i = 0; i < len; i += 32) {
                const uint64_t v = w[i >> 5];
                for (int j = 0; j < 32; j++) buf[i + j] = (uint8_t)((v >> (62 - 2 * j)) & 3);
            }
            return buf.data();
        });
    }
    template <typename Get>
    int add_any(uint64_t n, int n_threads, Get get) {
        int nt = pick_threads(n_threads);
        nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)nt, (n + 255) / 256));
        constexpr int NP = PreArcs::NP;
        if ((int)scratch.size() < nt) scratch.resize(nt);                    // buffers live across batches: no fresh pages
        const bool reps = path_fp != nullptr;
        std::atomic<int> bad{0};
        const uint32_t id_end = (uint32_t)arcs.head.size();
        auto worker = [&](int t) {
            Scratch& sc = scratch[t];
            if (!sc.rt) sc.rt.reset(new ReadThreader<NW>(g));
            sc.pairs.clear(); sc.path.clear(); sc.deleted = 0; sc.marked = 0;
            const uint64_t lo = n * t / nt, hi = n * (t + 1) / nt;
            for (uint64_t r = lo; r < hi; r++) {
                int len = 0;
                const uint8_t* rd = get(r, sc.unpacked, len);
                if (len < g.K + 1) continue;                                  // prlRead2path.c:1103 (same filter as pass 1)
                sc.marks.clear();
                if (!sc.rt->thread_read(rd, len, sc.items, sc.pairs, reps ? &sc.path : nullptr, reps ? &sc.marks : nullptr)) sc.deleted++;
                // saturating per-edge marker counts: increments commute, so they are applied right here
                for (uint32_t e : sc.marks) {
                    if (e >= marker.size()) { bad.store(1); continue; }
                    uint8_t v = __atomic_load_n(&marker[e], __ATOMIC_RELAXED);
                    while (v < 255 && !__atomic_compare_exchange_n(&marker[e], &v, (uint8_t)(v + 1), true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
                }
                sc.marked += (long long)sc.marks.size();
            }
            // stable counting sort of this thread's pairs by source-edge range
            for (int i = 0; i <= NP; i++) sc.off[i] = 0;
            for (auto& pr : sc.pairs) {
                if (pr.first >= id_end) { bad.store(1); return; }
                sc.off[arcs.part_of(pr.first) + 1]++;
            }
            for (int i = 0; i < NP; i++) sc.off[i + 1] += sc.off[i];
            sc.sorted.resize(sc.pairs.size());
            size_t cur[NP];
            for (int i = 0; i < NP; i++) cur[i] = sc.off[i];
            for (auto& pr : sc.pairs) sc.sorted[cur[arcs.part_of(pr.first)]++] = pr;
        };
        const double t0 = now();
        {
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++) pool.emplace_back(worker, t);
            worker(0);
            for (auto& th : pool) th.join();
        }
        const double t1 = now();
        t_thread += t1 - t0;
        if (bad.load()) { pg_set_error("edge id out of range in pass 2"); return PG_EINVAL; }
        // fold: every source-edge range takes its pairs thread by thread, i.e. in read order
        {
            std::atomic<int> next{0};
            auto folder = [&]() {
                for (;;) {
                    const int part = next.fetch_add(1);
                    if (part >= NP) break;
                    PreArcs::Pool& pl = arcs.pool[part];
                    for (int t = 0; t < nt; t++) {
                        const Scratch& sc = scratch[t];
                        for (size_t i = sc.off[part]; i < sc.off[part + 1]; i++) arcs.add(pl, sc.sorted[i].first, sc.sorted[i].second);
                    }
                }
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < std::min(nt, NP); t++) pool.emplace_back(folder);
            folder();
            for (auto& th : pool) th.join();
        }
        for (int t = 0; t < nt; t++) {
            const Scratch& sc = scratch[t];
            reads_deleted += sc.deleted;
            if (reps) {
                if (!sc.path.empty() && fwrite(sc.path.data(), 1, sc.path.size(), path_fp) != sc.path.size()) {
                    pg_set_error("short write on " + prefix + ".path");
                    return PG_EIO;
                }
                mark_count += sc.marked;
            }
        }
        reads_seen += (long long)n;
        t_fold += now() - t1;
        return PG_OK;
    }
    int finish(long long* n_arcs) override {
        // whatever else goes wrong, the background edge writer is waited for and its error is not lost (the first error wins)
        const int rc = finish_files(n_arcs);
        const std::string why = rc ? pg_last_error() : std::string();
        const int erc = join_edge_writer();
        if (rc) pg_set_error(why);
        return rc ? rc : erc;
    }
    int finish_files(long long* n_arcs) {
        int rc = dev_on ? dev_finish() : arcs.write(prefix + ".preArc");
        if (rc) return rc;
        const long long arc_count = dev_on ? dev_arc_count : arcs.count();
        if (path_fp) {
            fclose(path_fp);
            path_fp = nullptr;
            fprintf(stderr, "%lld marker(s) output.\n", mark_count);
            FILE* fp = fopen((prefix + ".markOnEdge").c_str(), "w");
            if (!fp) { pg_set_error("cannot open " + prefix + ".markOnEdge"); return PG_EIO; }
            for (size_t e = 1; e < marker.size(); e++) fprintf(fp, "%d\n", (int)marker[e]);
            fclose(fp);
        }
        fprintf(stderr, "Reads alignment done, %lld read(s) deleted, %lld pre-arc(s) added.\n", reads_deleted, arc_count);
        fprintf(stderr, "Time spent on threading reads: %.1fs, on folding pre-arcs: %.1fs.\n", t_thread, t_fold);
        if (n_arcs) *n_arcs = arc_count;
        { const int erc = join_edge_writer(); if (erc) return erc; }
        if (vertex_started) {
            const double tw0 = now();
            if (vertex_thread.joinable()) vertex_thread.join();
            if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "finish: waited %.2fs for the vertex writer\n", now() - tw0);
            if (vertex_rc) return vertex_rc;
            num_vt = vertex_count;
            fprintf(stderr, "%d vertex(es) output.\n", num_vt);
            return write_basic_file(prefix, num_vt, g.K, num_ed, max_read_len);
        }
        return write_vertex<NW>(g, prefix, num_ed, max_read_len, num_vt);
    }
};

// records that lie in device memory (device `rec_device`, replay order): pulled by the replay's workers chunk by chunk
struct DeviceRecords { const uint64_t* d_rec; int rw, device; };
static int fetch_device_records(void* user, uint64_t first, uint64_t n, uint64_t* dst) {
    const DeviceRecords* f = (const DeviceRecords*)user;
    return p2_fetch_words(f->device, f->d_rec + first * (uint64_t)f->rw, n * (uint64_t)f->rw, dst);
}

// a duplicate put arrived after set s's last new key? (it still ran the growth test, newhash.c:477) -- set_last_put against the
// ordinal of the set's last record, which lies on `device`
template <int NW>
static int trailing_puts(int device, const uint64_t* d_records, const uint64_t* counts, int n_sets, const uint64_t* last_put /*per set, may be null*/,
                         std::vector<unsigned char>& out) {
    out.assign((size_t)n_sets, 0);
    uint64_t first = 0;
    int rc = PG_OK;
    for (int s = 0; s < n_sets && rc == PG_OK; s++) {
        first += counts[s];
        if (!counts[s] || !last_put || !last_put[s]) continue;
        uint64_t tag = 0;
        rc = p2_fetch_words(device, d_records + (first - 1) * (uint64_t)(NW + 2) + NW + 1, 1, &tag);
        if (rc == PG_OK) out[s] = last_put[s] > (tag & PG_ORD_MASK) + 1;
    }
    (void)p2_fetch_words(device, nullptr, 0, nullptr);
    return rc;
}

// SURVEY.md App. C "K6": the layout of the k-mer sets is made on the device from the records as they lie there
// (graph_kernels.hip: p2_layout_rank / p2_layout_rank_growable) -- with -a the sets never grow (dev_graph.hpp: layout_static),
// without they end at the size the reference's growth schedule gives them and every key where the in-place rehashes leave it
// (dev_rehash.hpp: layout_growable).  The host copy (SOAPDENOVO2_AMD_TIPS=replay only) is a download of that image.
// Returns PG_OK, 1 = unsuited (the caller replays on the host), or PG_E*.
template <int NW>
static int layout_on_device(GraphHandle<NW>* h, const uint64_t* d_records, const uint64_t* per_set_count, const uint64_t* set_last_put, int K, int P,
                            int a_gb, int n_threads, int device, bool host_copy) {
    Graph<NW>& g = h->g;
    g.K = K; g.P = P; g.filter = kmer_filter<NW>(K); g.bias = set_bias((uint32_t)P); g.crc = host_crc_table();
    host_crc8_init();
    g.n_threads = n_threads;
    const uint64_t S = ref_initial_set_size(a_gb, P, NW == 4);
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    std::vector<uint64_t> sizes((size_t)P, S);
    P2Device* dev = nullptr;
    if (a_gb != 0) {
        bool unsuited = false;
        dev = p2_open_layout(device, K, NW, P, d_records, per_set_count, S, h->max_nk(), &unsuited);
        if (!dev) return unsuited ? 1 : PG_ENODEV;
    } else {
        std::vector<unsigned char> trailing;
        if (trailing_puts<NW>(device, d_records, per_set_count, P, set_last_put, trailing) != PG_OK) return PG_ENODEV;
        uint64_t* nodes = nullptr;
        void* alloc = nullptr;
        const int rc = p2_layout_rank_growable(device, NW, P, d_records, per_set_count, trailing.data(), S, sizes.data(), &nodes, &alloc);
        if (rc) return rc;
        std::vector<int> devs((size_t)P, device);
        std::vector<uint64_t*> ptrs((size_t)P);
        uint64_t at = 0;
        for (int si = 0; si < P; si++) { ptrs[si] = nodes + at * (NW + 1); at += sizes[si]; }
        dev = p2_adopt(device, K, NW, P, sizes.data(), devs.data(), ptrs.data(), {{device, alloc}}, h->max_nk());
        if (!dev) return PG_ENODEV;
    }
    const double t1 = now();
    g.sets.clear();
    g.sets.resize(P);
    g.set_base.assign((size_t)P + 1, 0);
    for (int si = 0; si < P; si++) g.set_base[si + 1] = g.set_base[si] + sizes[si];
    std::atomic<int> next{0}, failed{0};
    auto worker = [&]() {
        for (;;) {
            const int si = next.fetch_add(1);
            if (si >= P || !host_copy) break;
            HSet<NW>& hs = g.sets[si];
            hs.adopt(sizes[si], per_set_count[si]);
            if (p2_download_set(dev, si, hs.array.data()) != PG_OK) { failed.store(1); continue; }
            for (uint64_t i = 0; i < sizes[si]; i++) hs.occ[i] = hs.array[i].seq.w[0] != HSet<NW>::EMPTY;
        }
    };
    {
        const int nt = std::max(1, std::min(pick_threads(n_threads), P));
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(worker);
        worker();
        for (auto& th : pool) th.join();
    }
    if (failed.load()) { p2_destroy(dev); return PG_ENODEV; }
    h->dev = dev; h->dev_on = true; h->dev_id = device;
    g.tip_dev = dev;
    if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "k-mer set layout on the device (%s): %.2fs; host copy %s: %.2fs\n", a_gb ? "static pools" : "growable sets", t1 - t0,
                                           host_copy ? "downloaded" : "not needed", now() - t1);
    return PG_OK;
}

// The sharded form ("reference set id -> GPU"): rank r of n_ranks holds the records of the sets s with
// s mod n_ranks == r, sorted by (set, ordinal), in the memory of its own GPU.
struct ShardedRecords {
    int n_ranks = 0, rw = 0;
    std::vector<int> devices;
    std::vector<const uint64_t*> d_rec;
    std::vector<uint64_t> first_global;          // [P + 1] index of every set's first record in set order
    std::vector<uint64_t> local_off;             // [P] index of the set's first record in its rank's array
};
static int fetch_sharded_records(void* user, uint64_t first, uint64_t n, uint64_t* dst) {
    const ShardedRecords* f = (const ShardedRecords*)user;
    if (n == 0) return p2_fetch_words(f->devices[0], nullptr, 0, nullptr);
    const int s = (int)(std::upper_bound(f->first_global.begin(), f->first_global.end(), first) - f->first_global.begin()) - 1;   // a stretch never spans sets
    const int r = s % f->n_ranks;
    return p2_fetch_words(f->devices[r], f->d_rec[r] + (f->local_off[s] + (first - f->first_global[s])) * (uint64_t)f->rw, n * (uint64_t)f->rw, dst);
}
// K6 on every rank for the sets it owns, then one graph over all of them (the lead = rank 0's GPU runs the kernels)
template <int NW>
static int layout_on_ranks(GraphHandle<NW>* h, const ShardedRecords& sr, const uint64_t* per_set_count, const uint64_t* set_last_put, int K, int P, int a_gb,
                           int n_threads) {
    Graph<NW>& g = h->g;
    g.K = K; g.P = P; g.filter = kmer_filter<NW>(K); g.bias = set_bias((uint32_t)P); g.crc = host_crc_table();
    host_crc8_init();
    g.n_threads = n_threads;
    const uint64_t S = ref_initial_set_size(a_gb, P, NW == 4);
    const int N = sr.n_ranks;
    std::vector<uint64_t*> nodes(N, nullptr);
    std::vector<void*> allocs(N, nullptr);
    std::vector<int> rcs(N, PG_OK);
    std::vector<std::string> why(N);
    std::vector<uint64_t> sizes(P, S);
    std::vector<std::thread> pool;
    // (test hook: SOAPDENOVO2_AMD_TEST_UNSUITED_RANK=r makes rank r report "unsuited" -- as a set of >= 2^32 keys or a pool filled to
    //  the last slot would -- so that the path "some ranks laid out, one did not, everybody replays on the host" can be walked with
    //  small inputs)
    const int forced_unsuited = pg::env_test("SOAPDENOVO2_AMD_TEST_UNSUITED_RANK") ? atoi(pg::env_test("SOAPDENOVO2_AMD_TEST_UNSUITED_RANK")) : -1;
    for (int r = 0; r < N; r++)
        pool.emplace_back([&, r] {
            std::vector<uint64_t> own, own_last, own_sizes;
            for (int s = r; s < P; s += N) { own.push_back(per_set_count[s]); own_last.push_back(set_last_put ? set_last_put[s] : 0); }
            if (r == forced_unsuited) { rcs[r] = 1; return; }                 // (1 = K6_UNSUITED, dev_graph.hpp)
            if (a_gb != 0) rcs[r] = p2_layout_rank(sr.devices[r], NW, (int)own.size(), sr.d_rec[r], own.data(), S, &nodes[r], &allocs[r]);
            else {
                std::vector<unsigned char> trailing;
                own_sizes.assign(own.size(), 0);
                rcs[r] = trailing_puts<NW>(sr.devices[r], sr.d_rec[r], own.data(), (int)own.size(), own_last.data(), trailing);
                if (rcs[r] == PG_OK)
                    rcs[r] = p2_layout_rank_growable(sr.devices[r], NW, (int)own.size(), sr.d_rec[r], own.data(), trailing.data(), S, own_sizes.data(), &nodes[r], &allocs[r]);
                for (size_t i = 0; i < own.size(); i++) sizes[r + (int)i * N] = own_sizes[i];
            }
            if (rcs[r] < 0) why[r] = pg_last_error();
        });
    for (auto& t : pool) t.join();
    int rc = PG_OK;
    for (int r = 0; r < N; r++) if (rcs[r] && rc <= 0) { rc = rcs[r] < 0 ? rcs[r] : (rc ? rc : 1); if (rcs[r] < 0) pg_set_error(why[r]); }
    std::vector<std::pair<int, void*>> owned;
    for (int r = 0; r < N; r++) if (nodes[r]) owned.emplace_back(sr.devices[r], allocs[r]);
    // another rank is unsuited or failed: the host replay that may follow reads every rank's records, and those may lie in the
    // tail of the very block a successful rank laid its sets out in -- such a block goes back on offer, it is not freed here
    if (rc) { for (auto& o : owned) pg_device_release_layout(o.first, o.second); return rc; }
    std::vector<int> devs(P);
    std::vector<uint64_t*> ptrs(P);
    std::vector<uint64_t> rank_at(N, 0);                                 // slots of the rank's earlier sets
    for (int s = 0; s < P; s++) { devs[s] = sr.devices[s % N]; ptrs[s] = nodes[s % N] + rank_at[s % N] * (NW + 1); rank_at[s % N] += sizes[s]; }
    P2Device* dev = p2_adopt(sr.devices[0], K, NW, P, sizes.data(), devs.data(), ptrs.data(), owned, h->max_nk());
    if (!dev) return PG_ENODEV;
    // the ranks become the lanes of the graph: per-set scans on the owner, pass 2's batches dealt to all of them
    if (p2_use_lanes(dev, sr.devices.data(), N) != PG_OK) { p2_destroy(dev); return PG_ENODEV; }
    g.sets.clear();
    g.sets.resize(P);
    g.set_base.assign((size_t)P + 1, 0);
    for (int si = 0; si < P; si++) g.set_base[si + 1] = g.set_base[si] + sizes[si];
    h->dev = dev; h->dev_on = true; h->dev_id = sr.devices[0];
    h->set_devices = devs;
    return PG_OK;
}

template <int NW>
static GraphHandleBase* graph_begin(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int K, int P, int cut_single,
                                    int a_gb, int max_read_len, int n_threads, const char* prefix_c, int device,
                                    pg_fetch_fn fetch = nullptr, void* fetch_user = nullptr, const uint64_t* per_set_count = nullptr,
                                    const uint64_t* d_records = nullptr, int rec_device = -1, const ShardedRecords* sharded = nullptr) {
    GraphHandle<NW>* h = new GraphHandle<NW>();
    h->prefix = prefix_c;
    h->max_read_len = max_read_len;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    int rc_replay = 1;
    DeviceRecords dr{d_records, NW + 2, rec_device};
    // SOAPDENOVO2_AMD_TIPS=replay: round 2's hybrid (walks on the device, decisions replayed by the host in slot order), for A/B runs
    const bool tips_replay = pg::env_user("SOAPDENOVO2_AMD_TIPS") && !strcmp(pg::env_user("SOAPDENOVO2_AMD_TIPS"), "replay");
    if (d_records) {
        // the layout is made where the records are (SOAPDENOVO2_AMD_LAYOUT=host keeps the host replay, for A/B runs)
        const char* where = pg::env_user("SOAPDENOVO2_AMD_LAYOUT");
        if (device >= 0 && device == rec_device && !(where && !strcmp(where, "host")) && !tips_on_host())
            rc_replay = layout_on_device<NW>(h, d_records, per_set_count, set_last_put, K, P, a_gb, n_threads, device, /*host_copy=*/tips_replay);
        if (rc_replay == 1) { fetch = &fetch_device_records; fetch_user = &dr; }
    }
    if (sharded) {
        const char* where = pg::env_user("SOAPDENOVO2_AMD_LAYOUT");
        h->set_devices.resize(P);
        for (int si = 0; si < P; si++) h->set_devices[si] = sharded->devices[si % sharded->n_ranks];
        h->lane_devices = sharded->devices;
        if (!(where && !strcmp(where, "host")) && !tips_replay && !tips_on_host())
            rc_replay = layout_on_ranks<NW>(h, *sharded, per_set_count, set_last_put, K, P, a_gb, n_threads);
        if (rc_replay == 1) { fetch = &fetch_sharded_records; fetch_user = (void*)sharded; }
    }
    if (rc_replay == 1)
        rc_replay = fetch ? replay_streamed<NW>(h->g, fetch, fetch_user, n, per_set_count, set_last_put, K, P, a_gb, n_threads)
                          : replay_layout<NW>(h->g, records, n, set_last_put, K, P, a_gb, n_threads);
    if (rc_replay != PG_OK) { delete h; return nullptr; }
    fprintf(stderr, "Time spent on rebuilding the k-mer set layout: %.1fs.\n", now() - t0);
    t0 = now();
    if (device >= 0 && !tips_on_host() && !h->dev && h->dev_open(device) != PG_OK) { delete h; return nullptr; }
    if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "k-mer sets uploaded to the device: %.2fs\n", now() - t0);
    if (h->dev && !tips_replay) {                // decided on the device (dev_tips.hpp); the host copy of the sets is not touched
        if (h->dev_clip_tips(cut_single != 0) != PG_OK) { delete h; return nullptr; }
    } else {
        if (cut_single) h->g.remove_single_tips();
        h->g.remove_minor_tips();
        if (h->g.tip_error) { delete h; return nullptr; }
    }
    fprintf(stderr, "Time spent on removing tips: %.1fs.\n\n", now() - t0);
    t0 = now();
    int edge_c = 0;
    long long records_c = 0, extra_nodes = 0;
    const int rc_edges = device >= 0 ? h->dev_build_edges(device, n_threads, edge_c, records_c, extra_nodes)
                                     : construct_edges<NW>(h->g, h->prefix, n_threads, edge_c, records_c, extra_nodes);
    if (rc_edges != PG_OK) { delete h; return nullptr; }
    fprintf(stderr, "%d (%lld) edge(s) and %lld extra node(s) constructed.\n", edge_c, records_c, extra_nodes);
    fprintf(stderr, "Time spent on constructing edges: %.1fs.\n\n", now() - t0);
    h->num_ed = edge_c;
    h->arcs.init((uint32_t)edge_c);
    return h;
}

template <int NW>
static int build_graph(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int K, int P, int cut_single,
                       int a_gb, int max_read_len, int n_threads, const char* prefix_c, int* out_vt, int* out_ed) {
    const std::string prefix(prefix_c);
    Graph<NW> g;
    int rc0 = replay_layout<NW>(g, records, n, set_last_put, K, P, a_gb, n_threads);
    if (rc0) return rc0;

    // ---- tips (pregraph.c:106-120)
    if (cut_single) g.remove_single_tips();
    g.remove_minor_tips();

    // ---- edges (pregraph.c:122-127)
    int edge_c = 0;
    long long records_c = 0, extra_nodes = 0;
    int rc = construct_edges<NW>(g, prefix, n_threads, edge_c, records_c, extra_nodes);
    if (rc) return rc;
    fprintf(stderr, "%d (%lld) edge(s) and %lld extra node(s) constructed.\n", edge_c, records_c, extra_nodes);

    int num_vt = 0;
    rc = write_vertex<NW>(g, prefix, edge_c, max_read_len, num_vt);
    if (rc) return rc;
    if (out_vt) *out_vt = num_vt;
    if (out_ed) *out_ed = edge_c;
    return PG_OK;
}

}  // namespace pg

extern "C" int pg_host_build_graph(const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int K, int mer127,
                                   int n_sets, int cut_single, int a_gb, int max_read_len, int n_threads, const char* prefix,
                                   int* out_num_vertex, int* out_num_edge) {
    if ((!records && n_records) || !prefix) { pg_set_error("null argument"); return PG_EINVAL; }
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || !(K & 1)) { pg_set_error("K must be odd and within 13.." + std::to_string(maxK)); return PG_EINVAL; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return PG_EINVAL; }
    if (mer127)
        return pg::build_graph<4>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, out_num_vertex, out_num_edge);
    return pg::build_graph<2>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, out_num_vertex, out_num_edge);
}

extern "C" pg_graph* pg_host_graph_begin(const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int K, int mer127,
                                         int n_sets, int cut_single, int a_gb, int max_read_len, int n_threads, const char* prefix) {
    if ((!records && n_records) || !prefix) { pg_set_error("null argument"); return nullptr; }
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || !(K & 1)) { pg_set_error("K must be odd and within 13.." + std::to_string(maxK)); return nullptr; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return nullptr; }
    pg::GraphHandleBase* h = mer127 ? pg::graph_begin<4>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, -1)
                                    : pg::graph_begin<2>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, -1);
    return (pg_graph*)h;
}
extern "C" pg_graph* pg_graph_begin(const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int K, int mer127,
                                    int n_sets, int cut_single, int a_gb, int max_read_len, int n_threads, const char* prefix, int device) {
    if ((!records && n_records) || !prefix) { pg_set_error("null argument"); return nullptr; }
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || !(K & 1)) { pg_set_error("K must be odd and within 13.." + std::to_string(maxK)); return nullptr; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return nullptr; }
    pg::GraphHandleBase* h = mer127 ? pg::graph_begin<4>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, device)
                                    : pg::graph_begin<2>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, device);
    return (pg_graph*)h;
}
extern "C" int pg_host_edge_file_in_background(int on) {
    pg::g_edge_file_in_background = on ? 1 : 0;
    return PG_OK;
}
extern "C" int pg_host_graph_resolve_repeats(pg_graph* g, int on) {
    if (!g) { pg_set_error("null argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->resolve_repeats(on);
}
extern "C" pg_graph* pg_graph_begin_streamed(int (*fetch)(void*, uint64_t, uint64_t, uint64_t*), void* user, uint64_t n_records,
                                             const uint64_t* per_set_count, const uint64_t* set_last_put, int K, int mer127, int n_sets,
                                             int cut_single, int a_gb, int max_read_len, int n_threads, const char* prefix, int device) {
    if (!fetch || !per_set_count || !prefix) { pg_set_error("null argument"); return nullptr; }
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || !(K & 1)) { pg_set_error("K must be odd and within 13.." + std::to_string(maxK)); return nullptr; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return nullptr; }
    pg::GraphHandleBase* h = mer127 ? pg::graph_begin<4>(nullptr, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, device, fetch, user, per_set_count)
                                    : pg::graph_begin<2>(nullptr, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, device, fetch, user, per_set_count);
    return (pg_graph*)h;
}
extern "C" pg_graph* pg_graph_begin_device(const uint64_t* d_records, int records_device, uint64_t n_records, const uint64_t* per_set_count,
                                           const uint64_t* set_last_put, int K, int mer127, int n_sets, int cut_single, int a_gb, int max_read_len,
                                           int n_threads, const char* prefix, int device) {
    if ((!d_records && n_records) || !per_set_count || !prefix) { pg_set_error("null argument"); return nullptr; }
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || !(K & 1)) { pg_set_error("K must be odd and within 13.." + std::to_string(maxK)); return nullptr; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return nullptr; }
    static const uint64_t none = 0;
    const uint64_t* recs = d_records ? d_records : &none;        // (no records: an address nobody reads)
    pg::GraphHandleBase* h = mer127 ? pg::graph_begin<4>(nullptr, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, device, nullptr, nullptr, per_set_count, recs, records_device)
                                    : pg::graph_begin<2>(nullptr, n_records, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, device, nullptr, nullptr, per_set_count, recs, records_device);
    return (pg_graph*)h;
}
extern "C" pg_graph* pg_graph_begin_sharded(int n_ranks, const int* devices, const uint64_t* const* d_records, const uint64_t* n_records,
                                            const uint64_t* per_set_count, const uint64_t* set_last_put, int K, int mer127, int n_sets, int cut_single,
                                            int a_gb, int max_read_len, int n_threads, const char* prefix) {
    if (n_ranks < 1 || !devices || !d_records || !n_records || !per_set_count || !prefix) { pg_set_error("null argument"); return nullptr; }
    const int maxK = mer127 ? 127 : 63;
    if (K < 13 || K > maxK || !(K & 1)) { pg_set_error("K must be odd and within 13.." + std::to_string(maxK)); return nullptr; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return nullptr; }
    pg::ShardedRecords sr;
    sr.n_ranks = n_ranks; sr.rw = (mer127 ? 4 : 2) + 2;
    sr.devices.assign(devices, devices + n_ranks);
    sr.d_rec.assign(d_records, d_records + n_ranks);
    sr.first_global.assign((size_t)n_sets + 1, 0);
    sr.local_off.assign(n_sets, 0);
    std::vector<uint64_t> held(n_ranks, 0);
    uint64_t total = 0;
    for (int s = 0; s < n_sets; s++) {
        sr.first_global[s] = total;
        sr.local_off[s] = held[s % n_ranks];
        held[s % n_ranks] += per_set_count[s];
        total += per_set_count[s];
    }
    sr.first_global[n_sets] = total;
    for (int r = 0; r < n_ranks; r++)
        if (held[r] != n_records[r]) { pg_set_error("pg_graph_begin_sharded: rank " + std::to_string(r) + " does not hold exactly the records of its sets"); return nullptr; }
    pg::GraphHandleBase* h = mer127 ? pg::graph_begin<4>(nullptr, total, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, devices[0], nullptr, nullptr, per_set_count, nullptr, -1, &sr)
                                    : pg::graph_begin<2>(nullptr, total, set_last_put, K, n_sets, cut_single, a_gb, max_read_len, n_threads, prefix, devices[0], nullptr, nullptr, per_set_count, nullptr, -1, &sr);
    return (pg_graph*)h;
}
extern "C" int pg_graph_use_device(pg_graph* g, int device) {
    if (!g) { pg_set_error("null argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->use_device(device);
}
extern "C" int pg_host_graph_add_packed(pg_graph* g, const uint64_t* words, const int32_t* lens, uint64_t n_reads, int n_threads) {
    if (!g || ((!words || !lens) && n_reads)) { pg_set_error("null argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->add_packed(words, lens, n_reads, n_threads);
}
extern "C" int pg_graph_add_packed_device(pg_graph* g, const uint64_t* d_words, uint64_t n_reads, int read_len, int device) {
    if (!g || (!d_words && n_reads) || read_len < 1) { pg_set_error("bad argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->add_packed_device(d_words, n_reads, read_len, device);
}
extern "C" int pg_graph_add_packed_device_segments(pg_graph* g, const uint64_t* const* d_segs, const uint64_t* seg_reads, int n_segs, int read_len, int device) {
    if (!g || !d_segs || !seg_reads || n_segs < 1 || read_len < 1) { pg_set_error("bad argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->add_packed_device_segments(d_segs, seg_reads, n_segs, read_len, device);
}
extern "C" int pg_graph_add_packed_device_ragged(pg_graph* g, const uint64_t* d_words, const uint64_t* d_word_off, const uint64_t* d_kmer_base, uint64_t n_reads,
                                                uint64_t n_kmers, int max_len, int device) {
    if (!g || ((!d_words || !d_word_off || !d_kmer_base) && n_reads) || max_len < 1) { pg_set_error("bad argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->add_packed_device_ragged(d_words, d_word_off, d_kmer_base, n_reads, n_kmers, max_len, device);
}
extern "C" int pg_host_graph_add_reads(pg_graph* g, const uint8_t* codes, const int32_t* lens, uint64_t n_reads, uint64_t stride, int n_threads) {
    if (!g || (!codes && n_reads)) { pg_set_error("null argument"); return PG_EINVAL; }
    return ((pg::GraphHandleBase*)g)->add_reads(codes, lens, n_reads, stride, n_threads);
}
static bool g_process_exits_next = false;
extern "C" void pg_process_exits_after_this(int yes) { g_process_exits_next = yes != 0; }

extern "C" int pg_host_graph_finish(pg_graph* g, int* out_num_vertex, int* out_num_edge, long long* out_num_prearc) {
    if (!g) { pg_set_error("null argument"); return PG_EINVAL; }
    pg::GraphHandleBase* h = (pg::GraphHandleBase*)g;
    int rc = h->finish(out_num_prearc);
    if (out_num_vertex) *out_num_vertex = h->num_vt;
    if (out_num_edge) *out_num_edge = h->num_ed;
    // Unmapping tens of gigabytes of k-mer sets takes seconds (page by page, with TLB shoot-downs to every core a worker
    // ran on); a process that is about to exit leaves that to the kernel's exit path, which has none of it to do.
    if (pg::env_user("PG_HOST_VERBOSE")) {                       // resident memory, and how much of it sits on huge pages
        if (FILE* fp = fopen("/proc/self/smaps_rollup", "r")) {
            char line[256];
            while (fgets(line, sizeof line, fp))
                if (!strncmp(line, "Rss:", 4) || !strncmp(line, "AnonHugePages:", 14)) fprintf(stderr, "memory at the end: %s", line);
            fclose(fp);
        }
    }
    const auto td0 = std::chrono::steady_clock::now();
    if (g_process_exits_next) h->shutdown();
    else delete h;
    if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "graph released: %.2fs\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - td0).count());
    return rc;
}

extern "C" int pg_host_replay_layout(const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int mer127,
                                     int n_sets, int a_gb, uint64_t* out_slot, uint64_t* out_set_size) {
    if ((!records && n_records) || !out_slot) { pg_set_error("null argument"); return PG_EINVAL; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return PG_EINVAL; }
    if (mer127) return pg::layout_only<4>(records, n_records, set_last_put, n_sets, a_gb, out_slot, out_set_size);
    return pg::layout_only<2>(records, n_records, set_last_put, n_sets, a_gb, out_slot, out_set_size);
}

// Test hook (see include/soapdenovo2_amd.h, section 5): the tip clipping of dev_tips.hpp on the HostBackend next to the
// sequential host scan, on two copies of the same layout; out = tips removed by either (single, minor), nodes whose counter
// words differ afterwards, fixed-point rounds, minor cycles.
template <int NW>
static int emu_clip_tips(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int K, int P, int cut_single, int a_gb, int n_threads,
                         uint64_t out[8]) {
    using namespace pg;
    Graph<NW> g1, g2;
    int rc = replay_layout<NW>(g1, records, n, set_last_put, K, P, a_gb, 1);
    if (rc) return rc;
    rc = replay_layout<NW>(g2, records, n, set_last_put, K, P, a_gb, 1);
    if (rc) return rc;
    if (cut_single) g1.remove_single_tips();
    g1.remove_minor_tips();
    SetsGeo geo;
    geo.P = P;
    std::vector<uint64_t> geo_words(SV_GEO * (size_t)P);
    uint64_t first = 0;
    for (int s = 0; s < P; s++) {
        geo.first.push_back(first); geo.size.push_back(g2.sets[s].size); geo.base.push_back((uint64_t*)g2.sets[s].array.data());
        const ModConst mc = make_modconst(g2.sets[s].size);
        geo_words[SV_GEO * s] = first; geo_words[SV_GEO * s + 1] = g2.sets[s].size; geo_words[SV_GEO * s + 2] = (uint64_t)(uintptr_t)g2.sets[s].array.data();
        geo_words[SV_GEO * s + 3] = mc.v; geo_words[SV_GEO * s + 4] = mc.s;
        first += g2.sets[s].size;
    }
    SetsView view{geo_words.data(), host_crc_table(), (uint32_t)P, set_bias((uint32_t)P), K};
    HostBackend be(n_threads);
    if (const char* e = pg::env_test("PG_EMU_PLACES")) be.places = std::max(1, atoi(e));     // the per-place lists and gathers of a sharded run, on one memory
    TipTotals tot;
    rc = clip_tips<HostBackend, NW>(be, view, geo, cut_single != 0, tot);
    if (rc) { pg_set_error(be.error_text.empty() ? "emulated tip clipping failed" : be.error_text); return rc; }
    uint64_t diff = 0;
    for (int s = 0; s < P; s++)
        for (uint64_t i = 0; i < g1.sets[s].size; i++) {
            if (!g1.sets[s].occ[i]) continue;
            const HNode<NW>&a = g1.sets[s].array[i], &b = g2.sets[s].array[i];
            diff += a.A != b.A || a.B != b.B;
        }
    out[0] = (uint64_t)g1.last_single; out[1] = (uint64_t)g1.last_minor; out[2] = tot.single; out[3] = tot.minor;
    out[4] = diff; out[5] = (uint64_t)tot.rounds; out[6] = (uint64_t)tot.minor_cycles; out[7] = 0;
    return PG_OK;
}
extern "C" int pg_host_emu_clip_tips(const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int K, int mer127, int n_sets,
                                     int cut_single, int a_gb, int n_threads, uint64_t out[8]) {
    if ((!records && n_records) || !out) { pg_set_error("null argument"); return PG_EINVAL; }
    if (n_sets < 1 || n_sets > 255) { pg_set_error("n_sets must be 1..255"); return PG_EINVAL; }
    return mer127 ? emu_clip_tips<4>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, n_threads, out)
                  : emu_clip_tips<2>(records, n_records, set_last_put, K, n_sets, cut_single, a_gb, n_threads, out);
}

// The host half of pg_device_emu_clip_tips (graph_kernels.hip): the same two copies of the replayed layout -- `before` is what goes up to
// the device, `after` is what the sequential scan left.
template <int NW>
static int emu_tip_sets_nw(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int K, int P, int cut_single, int a_gb, pg::EmuTipSets& out) {
    using namespace pg;
    static_assert(sizeof(HNode<NW>) == (NW + 1) * sizeof(uint64_t), "a slot is NW key words and the counter word");
    Graph<NW> g;
    out.before.assign((size_t)P, {}); out.after.assign((size_t)P, {}); out.size.assign((size_t)P, 0);
    for (int pass = 0; pass < 2; pass++) {
        const int rc = replay_layout<NW>(g, records, n, set_last_put, K, P, a_gb, 1);
        if (rc) return rc;
        if (pass == 1) {
            if (cut_single) g.remove_single_tips();
            g.remove_minor_tips();
            if (g.tip_error) return g.tip_error;
            out.single = (unsigned long long)g.last_single; out.minor = (unsigned long long)g.last_minor;
        }
        for (int s = 0; s < P; s++) {
            const uint64_t* w = (const uint64_t*)g.sets[s].array.data();
            out.size[s] = g.sets[s].size;
            (pass ? out.after : out.before)[s].assign(w, w + g.sets[s].size * (uint64_t)(NW + 1));
        }
    }
    return PG_OK;
}
int pg::emu_tip_sets(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int K, int nw, int P, int cut_single, int a_gb, EmuTipSets& out) {
    return nw == 4 ? emu_tip_sets_nw<4>(records, n, set_last_put, K, P, cut_single, a_gb, out)
                   : emu_tip_sets_nw<2>(records, n, set_last_put, K, P, cut_single, a_gb, out);
}

// Test hook: the layout of growable sets as the device computes it (dev_rehash.hpp on the HostBackend) -- per record its slot,
// per set the final size and the fixed-point rounds, optionally the node image (sets back to back, NW + 1 words a slot, empty
// slots = all ones in word 0) -- to be compared with pg_host_replay_layout.  Records sorted by (set, ordinal).
template <int NW>
static int emu_layout_growable(const uint64_t* records, uint64_t n, const uint64_t* set_last_put, int P, int n_threads, uint64_t* out_slot,
                               uint64_t* out_size, uint64_t* out_rounds, uint64_t* out_nodes, uint64_t nodes_cap_slots) {
    using namespace pg;
    HostBackend be(n_threads);
    const uint64_t init = ref_initial_set_size(0, P, NW == 4);
    std::vector<uint64_t> cnt, first_slot(P + 1, 0);
    std::vector<unsigned char> trailing;
    if (!growable_counts_of_records(records, n, NW, set_last_put, P, cnt, trailing)) { pg_set_error("records are not sorted by set"); return PG_EINVAL; }
    for (int s = 0; s < P; s++) {
        const uint64_t fsize = grow_schedule(cnt[s], trailing[s] != 0, init).back().size;
        if (out_size) out_size[s] = fsize;
        first_slot[s + 1] = first_slot[s] + fsize;
    }
    if (out_nodes) {
        if (nodes_cap_slots < first_slot[P]) { pg_set_error("node image too small"); return PG_EINVAL; }
        for (uint64_t i = 0; i < first_slot[P]; i++) { out_nodes[i * (NW + 1)] = ~0ULL; for (int w = 1; w <= NW; w++) out_nodes[i * (NW + 1) + w] = 0; }
    }
    const int rc = layout_growable_sets<HostBackend, NW>(be, records, cnt.data(), trailing.data(), P, init, first_slot.data(), out_nodes,
                                                         (unsigned long long*)out_slot, out_rounds);
    if (rc) pg_set_error(be.error_text.empty() ? "layout_growable failed" : be.error_text);
    return rc;
}
extern "C" int pg_host_emu_layout_growable(const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int mer127, int n_sets, int n_threads,
                                           uint64_t* out_slot, uint64_t* out_set_size, uint64_t* out_rounds, uint64_t* out_nodes, uint64_t nodes_cap_slots) {
    if ((!records && n_records) || !out_slot) { pg_set_error("null argument"); return PG_EINVAL; }
    return mer127 ? emu_layout_growable<4>(records, n_records, set_last_put, n_sets, n_threads, out_slot, out_set_size, out_rounds, out_nodes, nodes_cap_slots)
                  : emu_layout_growable<2>(records, n_records, set_last_put, n_sets, n_threads, out_slot, out_set_size, out_rounds, out_nodes, nodes_cap_slots);
}

extern "C" int pg_host_write_kmerfreq(const uint64_t hist[256], const char* prefix) {
    if (!hist || !prefix) { pg_set_error("null argument"); return PG_EINVAL; }
    FILE* fo = fopen((std::string(prefix) + ".kmerFreq").c_str(), "w");
    if (!fo) { pg_set_error(std::string("cannot open ") + prefix + ".kmerFreq"); return PG_EIO; }
    for (int i = 1; i < 256; i++) fprintf(fo, "%lld\n", (long long)hist[i]);     // rows 1..255 only (prlHashReads.c:1113)
    fclose(fo);
    return PG_OK;
}
