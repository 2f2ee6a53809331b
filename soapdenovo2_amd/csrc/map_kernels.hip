// map_kernels.hip -- the `map` stage on the GPU: the contig k-mer index (prlContig2nodes, standardPregraph/prlHashCtg.c:345-467) and the
// read kernel (chopKmer4read + searchKmer + parse1read, prlRead2Ctg.c:153-361), one lane a read like pass 2's p2_thread_kernel.
//
//   map_index_kernel  a lane per stretch of MAP_ITEM k-mers of one contig: roll the k-mer, canonicalise, insert into the open-addressing
//                     table of map_index.hpp.  A new key is claimed with a CAS on its state word, its words are written, and the state is
//                     published with a release store; a lane that meets a claimed slot tries the same slot again on its next trip round the
//                     loop (no lane waits inside a branch for another lane of its own wavefront).  An equal key moves the state to
//                     "deleted", so the table is a function of the contigs alone.  The trips a lane spends on one claimed slot are capped
//                     (MAP_SPIN_CAP): a lane that gives up raises a device flag, and build() fails instead of the card hanging.
//   map_read_kernel   a lane per read: roll, canonicalise, probe; every k-mer's hit word goes to the read's row of the batch's hit buffer
//                     (the reference's nodeBuffer), then map_decide (map_decide.hpp) picks the contig from the row.
// Both wait for random 32- / 48-byte slot reads of a table that is many times the L2: the bound is HBM random-access latency and rate,
// not arithmetic.  Memory comes from the device arena (arena.hpp).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <string>

#include "../../include/soapdenovo2_amd.h"
#include "arena.hpp"
#include "extract.hpp"
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

template <int NW>
__global__ __launch_bounds__(256) void map_index_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                        const int32_t* __restrict__ len, const uint32_t* __restrict__ ids,
                                                        const uint32_t* __restrict__ item_ctg, const uint32_t* __restrict__ item_j0,
                                                        uint64_t n_items, int K, uint64_t* tab, uint64_t mask, uint32_t* gave_up) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
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
        map_insert<NW>(tab, mask, sm ? word : bal, map_hit(id, (uint32_t)j, sm ? 0 : 1, 0), gave_up);   // twin = 0 when the contig's strand is canonical
    }
}

struct MapRow {
    const uint64_t* p;
    __device__ __forceinline__ uint64_t operator()(int j) const { return p[j]; }
};

template <int NW>
__global__ __launch_bounds__(256) void map_read_kernel(const uint64_t* __restrict__ words, const uint64_t* __restrict__ off,
                                                       const int32_t* __restrict__ lens, const uint64_t* __restrict__ koff, uint64_t n, int K,
                                                       int align_len, const uint64_t* __restrict__ tab, uint64_t mask, MapCtgs ctgs,
                                                       uint64_t* __restrict__ rows, MapOut* __restrict__ out) {
    constexpr int SW = map_slot_words<NW>();
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int len = lens[r];
    const int nk = len >= K + 1 ? len - K + 1 : 0;           // prlRead2Ctg.c:159-162
    uint64_t* row = rows + koff[r];
    if (nk) {
        const uint64_t* rd = words + off[r];
        const Kmer<NW> filter = kmer_filter<NW>(K);
        Kmer<NW> word = read_kmer<NW>(rd, 0, K, filter);
        Kmer<NW> bal = kmer_rc<NW>(word, K);
        for (int j = 0; j < nk; j++) {
            if (j) kmer_roll<NW>(word, bal, read_base(rd, j + K - 1), K, filter);
            const bool sm = kmer_less<NW>(word, bal);
            const Kmer<NW> ck = sm ? word : bal;
            uint64_t e = map_home<NW>(ck, mask), hit = 0;
            for (;;) {
                const uint64_t* sl = tab + e * SW;
                const uint64_t s = sl[NW + 1];
                if (s == MAP_EMPTY) break;
                bool eq = true;
#pragma unroll
                for (int i = 0; i < NW; i++) eq = eq && sl[i] == ck.w[i];
                if (eq) {
                    if (s != MAP_DELETED) hit = sl[NW] | ((uint64_t)(sm ? 1 : 0) << 32);
                    break;
                }
                e = (e + 1) & mask;
            }
            row[j] = hit;
        }
    }
    out[r] = map_decide(MapRow{row}, nk, K, map_multi(len, align_len, K), ctgs);
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

class DeviceMapEngine : public MapEngine {
public:
    DeviceMapEngine(int device, int K, int nw) : dev_(device), K_(K), nw_(nw) {}
    ~DeviceMapEngine() override {
        if (!ready_) return;
        (void)hipSetDevice(dev_);
        tab_.release(); flag_.release(); len_.release(); bal_.release(); rwords_.release(); roff_.release(); rlen_.release(); rkoff_.release();
        rows_.release(); out_.release();
        if (st_) (void)hipStreamDestroy(st_);
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
        arena_unpin(dev_);
    }
    int begin() {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { pg_set_error("map: no HIP device"); return PG_ENODEV; }
        if (dev_ < 0 || dev_ >= n) { pg_set_error("map: HIP device " + std::to_string(dev_) + " does not exist"); return PG_ENODEV; }
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
        for (size_t i = 0; i < n_ctg; i++)
            for (int j = 0; j < c.len[i] - K_ + 1; j += MAP_ITEM) { item_c.push_back((uint32_t)i); item_j.push_back((uint32_t)j); }
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
            if (nw_ == 2) hipLaunchKernelGGL((map_index_kernel<2>), grid, block, 0, st_, d_w.p, d_off.p, d_len.p, d_id.p, d_ic.p, d_ij.p, n_items, K_, tab_.p, slots_ - 1, flag_.p);
            else hipLaunchKernelGGL((map_index_kernel<4>), grid, block, 0, st_, d_w.p, d_off.p, d_len.p, d_id.p, d_ic.p, d_ij.p, n_items, K_, tab_.p, slots_ - 1, flag_.p);
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
    int map(const MapBatch& b, int align_len, MapOut* out, uint64_t* rows_out) override {
        if (!b.n) return PG_OK;
        MAP_HIP(hipSetDevice(dev_));
        int rc;
        const uint64_t n_k = b.kmer_off[b.n];
        if ((rc = rwords_.reserve(b.n_words)) || (rc = roff_.reserve(b.n)) || (rc = rlen_.reserve(b.n)) || (rc = rkoff_.reserve(b.n + 1)) ||
            (rc = rows_.reserve(std::max<uint64_t>(n_k, 1))) || (rc = out_.reserve(b.n))) return rc;
        const double c0 = now_s();
        MAP_HIP(hipMemcpyAsync(rwords_.p, b.words, b.n_words * 8, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipMemcpyAsync(roff_.p, b.off, b.n * 8, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipMemcpyAsync(rlen_.p, b.len, b.n * 4, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipMemcpyAsync(rkoff_.p, b.kmer_off, (b.n + 1) * 8, hipMemcpyHostToDevice, st_));
        MAP_HIP(hipEventRecord(e0_, st_));
        const dim3 grid((unsigned)((b.n + 255) / 256)), block(256);
        if (nw_ == 2) hipLaunchKernelGGL((map_read_kernel<2>), grid, block, 0, st_, rwords_.p, roff_.p, rlen_.p, rkoff_.p, b.n, K_, align_len, tab_.p, slots_ - 1, ctgs_, rows_.p, out_.p);
        else hipLaunchKernelGGL((map_read_kernel<4>), grid, block, 0, st_, rwords_.p, roff_.p, rlen_.p, rkoff_.p, b.n, K_, align_len, tab_.p, slots_ - 1, ctgs_, rows_.p, out_.p);
        MAP_HIP(hipGetLastError());
        MAP_HIP(hipEventRecord(e1_, st_));
        MAP_HIP(hipMemcpyAsync(out, out_.p, b.n * sizeof(MapOut), hipMemcpyDeviceToHost, st_));
        if (rows_out && n_k) MAP_HIP(hipMemcpyAsync(rows_out, rows_.p, n_k * sizeof(uint64_t), hipMemcpyDeviceToHost, st_));
        MAP_HIP(hipStreamSynchronize(st_));
        float ms = 0;
        MAP_HIP(hipEventElapsedTime(&ms, e0_, e1_));
        t_kernel += ms * 1e-3;
        t_copy += now_s() - c0 - ms * 1e-3;
        return PG_OK;
    }

private:
    static double now_s() {
        timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
    }
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
};

}  // namespace

std::unique_ptr<MapEngine> map_engine_device(int device, int K, int nw) {
    std::unique_ptr<DeviceMapEngine> e(new DeviceMapEngine(device, K, nw));
    if (e->begin() != PG_OK) return nullptr;
    return std::unique_ptr<MapEngine>(e.release());
}

}  // namespace pg
