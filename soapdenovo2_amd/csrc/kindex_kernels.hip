// kindex_kernels.hip -- the k-mer index on the GPU (kindex.hpp: layout, sequence rules, the shared read side).
//
//   kidx_build_kernel       a lane per record of a device array in export format ((NW + 2) words a record, any order: what pg_export,
//                           pg_export_peek, pg_export_take and pg_sort_records leave).  The protocol is map_index_kernel's
//                           (map_kernels.hip): a new key is claimed with a CAS on its state word, key and value are written, and the
//                           state is published with a release store; a lane that meets a claimed slot looks at the same slot again on its
//                           next trip round the loop -- nobody waits inside a branch for a lane of its own wavefront.  The trips spent on
//                           one claimed slot are capped (KIDX_SPIN_CAP): a lane that gives up raises KIDX_FLAG_SPIN and the build fails
//                           with PG_ESPIN.  The keys are distinct by contract: a lane that meets its own key published raises
//                           KIDX_FLAG_DUP, leaves the slot as it is, and the build fails with PG_EINVAL.  A record the -d filter deleted
//                           (kidx_stored, kindex.hpp) is passed over.
//   kidx_query_kernel       a lane per sequence, for read-sized sequences: kidx_stretch over the whole sequence, the summary in registers.
//   kidx_query_wave_kernel  a wavefront per sequence, four sequences a 256-thread workgroup, for contig-sized sequences: lane l takes
//                           ceil(nk / 64) consecutive k-mers (one read_kmer, then rolling: map_read_wave_kernel's split), the summary
//                           through a __shfl_xor butterfly, lane 0 writes it.  No LDS, no workgroup barrier: a wave without a sequence
//                           just ends.
//   kcor_kernel             a lane per read of a batch that already lies in the output buffer: kcor_read (kcorrect.hpp) on the lane's own
//                           words, in global memory -- the first pass over the read as given is kidx_query_kernel's walk, and a read
//                           without a weak k-mer ends there; the lanes of a wave diverge in the trials.
// Both query kernels wait for one random slot read per k-mer (32 B a slot in the 63-mer build, 48 B in the 127-mer one) of a table that
// is many times the L2; the roll is arithmetic hidden under it.  Nothing here has been measured.
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>

#include "../../include/soapdenovo2_amd.h"
#include "arena.hpp"
#include "device_ctx.hpp"
#include "kcorrect.hpp"
#include "kindex.hpp"

namespace pg {

// Trips round kidx_insert's loop a lane may spend on one claimed slot before it gives up; a claim is held for NW + 1 stores (MAP_SPIN_CAP's reasoning, map_kernels.hip)
constexpr uint32_t KIDX_SPIN_CAP = 1u << 20;
constexpr uint32_t KIDX_FLAG_SPIN = 1u, KIDX_FLAG_DUP = 2u;
constexpr int KIDX_WAVES = 4;                     // sequences of a 256-thread workgroup of the wave kernel

#define KIDX_HIP(call)                                                                                  \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            pg_set_error(std::string("k-mer index: ") + #call + ": " + hipGetErrorString(e_));          \
            return PG_ENODEV;                                                                           \
        }                                                                                               \
    } while (0)

template <int NW>
__device__ __forceinline__ void kidx_insert(uint64_t* tab, uint64_t mask, const Kmer<NW>& k, uint64_t value, uint32_t* flags) {
    constexpr int SW = map_slot_words<NW>();
    uint64_t e = map_home<NW>(k, mask);
    uint32_t waits = 0;                            // trips spent on slot e while it was claimed
    for (;;) {
        uint64_t* sl = tab + e * SW;
        uint64_t* st = sl + NW + 1;
        const uint64_t s = __hip_atomic_load(st, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (s == KIDX_EMPTY) {
            if (atomicCAS((unsigned long long*)st, (unsigned long long)KIDX_EMPTY, (unsigned long long)KIDX_CLAIMED) == KIDX_EMPTY) {
#pragma unroll
                for (int i = 0; i < NW; i++) sl[i] = k.w[i];
                sl[NW] = value;
                __hip_atomic_store(st, KIDX_FULL, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            continue;                              // somebody claimed it first: look again
        }
        if (s == KIDX_CLAIMED) {                   // its key is still being written
            if (++waits > KIDX_SPIN_CAP) { atomicOr(flags, KIDX_FLAG_SPIN); return; }
            continue;
        }
        bool eq = true;
#pragma unroll
        for (int i = 0; i < NW; i++) eq = eq && sl[i] == k.w[i];
        if (eq) { atomicOr(flags, KIDX_FLAG_DUP); return; }   // the records' keys are not distinct: the slot stays the first one's
        e = (e + 1) & mask;
        waits = 0;
    }
}

template <int NW>
__global__ __launch_bounds__(256) void kidx_build_kernel(const uint64_t* __restrict__ records, uint64_t n_records, uint64_t* tab, uint64_t mask,
                                                         uint32_t* flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_records) return;
    const uint64_t* rec = records + i * (NW + 2);
    const uint64_t cnt = rec[NW];
    if (!kidx_stored(cnt)) return;                 // deleted by the -d filter: reads as 0
    Kmer<NW> k;
#pragma unroll
    for (int q = 0; q < NW; q++) k.w[q] = rec[q];
    kidx_insert<NW>(tab, mask, k, cnt, flags);
}

template <int NW>
__global__ __launch_bounds__(256) void kidx_query_kernel(const uint64_t* __restrict__ packed, const uint64_t* __restrict__ word_off,
                                                         const uint64_t* __restrict__ kmer_base, uint64_t n_seqs, uint32_t uniform_len, int K,
                                                         const uint64_t* __restrict__ tab, uint64_t mask, uint64_t* __restrict__ out,
                                                         uint64_t* __restrict__ summary) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_seqs) return;
    const KidxSeq q = kidx_seq(packed, word_off, kmer_base, uniform_len, K, r);
    KidxSummary s = kidx_summary_none();
    kidx_stretch<NW>(q.rd, 0, q.nk, K, tab, mask, out ? out + q.base : nullptr, s);
    if (summary) kidx_summary_store(s, q.nk, summary + r * KIDX_SUMMARY_WORDS);
}

template <int NW>
__global__ __launch_bounds__(256) void kidx_query_wave_kernel(const uint64_t* __restrict__ packed, const uint64_t* __restrict__ word_off,
                                                              const uint64_t* __restrict__ kmer_base, uint64_t n_seqs, uint32_t uniform_len,
                                                              int K, const uint64_t* __restrict__ tab, uint64_t mask,
                                                              uint64_t* __restrict__ out, uint64_t* __restrict__ summary) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r = (uint64_t)blockIdx.x * KIDX_WAVES + wave;
    if (r >= n_seqs) return;                       // (the whole wave; no workgroup barrier follows)
    const KidxSeq q = kidx_seq(packed, word_off, kmer_base, uniform_len, K, r);
    KidxSummary s = kidx_summary_none();
    if (q.nk) {                                    // (wave-uniform)
        const int per = (q.nk + 63) / 64;
        const int64_t first = (int64_t)lane * per;                                      // (64 * per can pass 2^31 where nk is close to it)
        const int j0 = first < q.nk ? (int)first : q.nk, j1 = first + per < q.nk ? (int)(first + per) : q.nk;
        kidx_stretch<NW>(q.rd, j0, j1, K, tab, mask, out ? out + q.base : nullptr, s);
    }
    if (!summary) return;
    for (int d = 32; d > 0; d >>= 1) {             // (every lane of the wave is here)
        KidxSummary o;
        o.present = __shfl_xor(s.present, d);
        o.cov_sum = __shfl_xor(s.cov_sum, d);
        o.cov_min = __shfl_xor(s.cov_min, d);
        o.first_absent = __shfl_xor(s.first_absent, d);
        kidx_summary_merge(s, o);
    }
    if (lane == 0) kidx_summary_store(s, q.nk, summary + r * KIDX_SUMMARY_WORDS);
}

template <int NW>
__global__ __launch_bounds__(256) void kcor_kernel(uint64_t* packed_out, const uint64_t* __restrict__ word_off, const uint64_t* __restrict__ kmer_base,
                                                   uint64_t n_seqs, uint32_t uniform_len, int K, const uint64_t* __restrict__ tab, uint64_t mask,
                                                   KcorParams pr, uint64_t* __restrict__ report) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_seqs) return;
    const KidxSeq q = kidx_seq(packed_out, word_off, kmer_base, uniform_len, K, r);
    const uint64_t rep = kcor_read<NW>(packed_out + (q.rd - packed_out), q.nk, K, tab, mask, pr);
    if (report) report[r] = rep;
}

namespace {

// f(std::integral_constant<int, NW>) for an index's flavour
template <typename F>
void kidx_with_nw(int nw, F f) {
    if (nw == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
}

int kidx_set_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { pg_set_error("k-mer index: no HIP device"); return PG_ENODEV; }
    if (dev < 0 || dev >= n) { pg_set_error("k-mer index: HIP device " + std::to_string(dev) + " does not exist"); return PG_ENODEV; }
    KIDX_HIP(hipSetDevice(dev));
    return PG_OK;
}

}  // namespace

int kidx_device_build(::pg_kindex* ix, const uint64_t* d_records, uint64_t n_records, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if ((n_records + 255) / 256 > 0x7FFFFFFFULL) { pg_set_error("k-mer index: too many records for one launch"); return PG_EINVAL; }
    arena_pin_for_process(ix->device);
    ix->keys = n_records;
    ix->slots = map_table_slots(n_records);
    const size_t bytes = kidx_table_bytes(n_records, ix->nw);
    if (arena_malloc(&ix->d_tab, bytes) != hipSuccess || arena_malloc(&ix->d_flags, sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        pg_set_error("k-mer index: out of device memory for a table of " + std::to_string(ix->slots) + " slots (" + std::to_string(bytes >> 20) + " MiB)");
        return PG_ENOMEM;
    }
    KIDX_HIP(hipMemsetAsync(ix->d_tab, 0, bytes, st));
    KIDX_HIP(hipMemsetAsync(ix->d_flags, 0, sizeof(uint32_t), st));
    if (n_records) {
        const dim3 grid((unsigned)((n_records + 255) / 256)), block(256);
        kidx_with_nw(ix->nw, [&](auto nw) {
            hipLaunchKernelGGL((kidx_build_kernel<decltype(nw)::value>), grid, block, 0, st, d_records, n_records, ix->d_tab, ix->slots - 1, ix->d_flags);
        });
        KIDX_HIP(hipGetLastError());
    }
    uint32_t flags = 0;
    KIDX_HIP(hipMemcpyAsync(&flags, ix->d_flags, sizeof flags, hipMemcpyDeviceToHost, st));
    KIDX_HIP(hipStreamSynchronize(st));
    if (flags & KIDX_FLAG_DUP) { pg_set_error("k-mer index: duplicate key in records"); return PG_EINVAL; }
    if (flags & KIDX_FLAG_SPIN) {
        pg_set_error("k-mer index: the build gave up on a claimed slot after " + std::to_string(KIDX_SPIN_CAP) +
                     " trips (the slot's key was never published); the index is not complete");
        return PG_ESPIN;
    }
    return PG_OK;
}

int kidx_device_query(::pg_kindex* ix, const uint64_t* d_packed, const uint64_t* d_word_off, const uint64_t* d_kmer_base, uint64_t n_seqs,
                      uint32_t uniform_len, int wave, uint64_t* d_out, uint64_t* d_summary, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!n_seqs) return PG_OK;
    const uint64_t blocks = wave ? (n_seqs + KIDX_WAVES - 1) / KIDX_WAVES : (n_seqs + 255) / 256;
    if (blocks > 0x7FFFFFFFULL) { pg_set_error("k-mer index: batch too large for one launch"); return PG_EINVAL; }
    const dim3 grid((unsigned)blocks), block(256);
    kidx_with_nw(ix->nw, [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        if (wave) hipLaunchKernelGGL((kidx_query_wave_kernel<NW>), grid, block, 0, st, d_packed, d_word_off, d_kmer_base, n_seqs, uniform_len, ix->K,
                                     ix->d_tab, ix->slots - 1, d_out, d_summary);
        else hipLaunchKernelGGL((kidx_query_kernel<NW>), grid, block, 0, st, d_packed, d_word_off, d_kmer_base, n_seqs, uniform_len, ix->K, ix->d_tab,
                                ix->slots - 1, d_out, d_summary);
    });
    KIDX_HIP(hipGetLastError());
    return PG_OK;
}

int kcor_device_correct(::pg_kindex* ix, const uint64_t* d_packed, const uint64_t* d_word_off, const uint64_t* d_kmer_base, uint64_t n_seqs,
                        uint32_t uniform_len, uint64_t n_words, const KcorParams& pr, uint64_t* d_packed_out, uint64_t* d_report, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!n_seqs) return PG_OK;
    const uint64_t blocks = (n_seqs + 255) / 256;
    if (blocks > 0x7FFFFFFFULL) { pg_set_error("k-mer index: batch too large for one launch"); return PG_EINVAL; }
    // the copy first -- pad bits and the readable tail with it -- then every lane works on its own words of the output
    if (d_packed_out != d_packed) KIDX_HIP(hipMemcpyAsync(d_packed_out, d_packed, n_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    const dim3 grid((unsigned)blocks), block(256);
    kidx_with_nw(ix->nw, [&](auto nw) {
        hipLaunchKernelGGL((kcor_kernel<decltype(nw)::value>), grid, block, 0, st, d_packed_out, d_word_off, d_kmer_base, n_seqs, uniform_len, ix->K,
                           ix->d_tab, ix->slots - 1, pr, d_report);
    });
    KIDX_HIP(hipGetLastError());
    return PG_OK;
}

void kidx_device_free(::pg_kindex* ix) {
    if (!ix->d_tab && !ix->d_flags) return;
    (void)hipSetDevice(ix->device);
    if (ix->d_tab) (void)arena_free(ix->d_tab);    // (waits for the device like hipFree: no query still reads the table)
    if (ix->d_flags) (void)arena_free(ix->d_flags);
    ix->d_tab = nullptr;
    ix->d_flags = nullptr;
}

}  // namespace pg

// pg_kindex_build for a context's own records (the host half of the ABI is kindex_host.cpp's)
extern "C" pg_kindex* pg_kindex_from_ctx(pg_ctx* c, void* stream) {
    if (!c) { pg_set_error("pg_kindex_from_ctx: null context (PG_EINVAL)"); return nullptr; }
    if (!c->finalized) { pg_set_error("pg_kindex_from_ctx: call pg_finalize first (PG_ESTATE)"); return nullptr; }
    if (c->engine == 2) {                          // the export array where it lies
        const uint64_t* d_records = nullptr;
        uint64_t n = 0;
        if (pg_export_peek(c, &d_records, &n) != PG_OK) return nullptr;
        return pg_kindex_build(c->device, c->K, c->NW == 4, d_records, n, stream);
    }
    // the global-set engine keeps no export array: one is made for the build and given back
    uint64_t n = 0, got = 0;
    if (pg_distinct(c, &n, stream) != PG_OK) return nullptr;
    uint64_t* d_records = nullptr;
    if (pg::arena_malloc(&d_records, (n ? n : 1) * (uint64_t)(c->NW + 2) * sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        pg_set_error("pg_kindex_from_ctx: out of device memory for the records (PG_ENOMEM)");
        return nullptr;
    }
    pg_kindex* ix = pg_export(c, d_records, n, &got, stream) == PG_OK ? pg_kindex_build(c->device, c->K, c->NW == 4, d_records, got, stream) : nullptr;
    (void)pg::arena_free(d_records);
    return ix;
}
