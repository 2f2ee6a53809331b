// dev_scratch.hpp -- what the host side of the device graph stages holds its scratch in (HIP host code only, no kernels):
//   DevArr<T>        a move-only owner of one block of the device arena: freed when it leaves scope, or where the code says reset()
//   DevEvent         the same for an event
//   dev_sort_* / dev_exclusive_sum / dev_inclusive_scan
//                    rocPRIM's two-call protocol (ask for the size, allocate, run) once per primitive, over a grow-only temporary
//   DevListing<T>    "list into a capped array, count everything, come again with exact room"
// The rule of the stage functions: scratch lives in owners and is released at the points the code states -- arena_free waits for the
// device as hipFree does, so WHERE a block goes is part of a stage's timing, and pg_host_plan_memory plans by the order of these calls.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdio.h>
#include <algorithm>
#include <iterator>
#include "arena.hpp"
#include "env.hpp"

namespace pg {

template <typename T>
struct DevArr {
    T* p = nullptr;
    size_t n = 0;                                    // elements asked for (the block holds max(n, 1))
    int device = 0;                                  // the HIP device the block was cut on
    DevArr() = default;
    DevArr(const DevArr&) = delete; DevArr& operator=(const DevArr&) = delete;
    DevArr(DevArr&& o) noexcept : p(o.p), n(o.n), device(o.device) { o.p = nullptr; o.n = 0; }
    DevArr& operator=(DevArr&& o) noexcept { if (this != &o) { reset(); p = o.p; n = o.n; device = o.device; o.p = nullptr; o.n = 0; } return *this; }
    ~DevArr() { reset(); }
    T* get() const { return p; }
    // a fresh block of max(count, 1) elements on the current device (what the owner held goes first)
    hipError_t alloc(size_t count) {
        reset();
        hipError_t e = hipGetDevice(&device);
        if (e == hipSuccess) e = arena_malloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    // grow-only: room for count elements; a block that is too small is replaced by one of count + headroom (nothing is copied)
    hipError_t reserve(size_t count, size_t headroom) { return p && count <= n ? hipSuccess : alloc(count + headroom); }
    // frees now.  A block of another device than the current one is freed there (the lead's thread releases the lanes' blocks).
    void reset() {
        if (!p) return;
        int cur = device; (void)hipGetDevice(&cur);
        if (cur != device) (void)hipSetDevice(device);
        (void)arena_free((void*)p);
        if (cur != device) (void)hipSetDevice(cur);
        p = nullptr; n = 0;
    }
    T* release() { T* q = p; p = nullptr; n = 0; return q; }                     // the block has a new owner
    void adopt(T* q, size_t count, int dev) { reset(); p = q; n = count; device = dev; }
};

struct DevEvent { hipEvent_t ev = nullptr; DevEvent() = default; DevEvent(const DevEvent&) = delete; DevEvent& operator=(const DevEvent&) = delete;
                  ~DevEvent() { if (ev) (void)hipEventDestroy(ev); } };

// ---- rocPRIM.  f(tmp, bytes) is a primitive's call with everything but its temporary bound: asked for the size with tmp = nullptr, run otherwise.
// dev_*_bytes is the size alone, for a caller that sizes ONE temporary for several primitives (or grows it by a rule of its own) before the calls.
template <typename F> inline size_t dev_tmp_bytes(F f) { size_t b = 0; return f(nullptr, b) == hipSuccess ? b : 0; }
template <typename F> inline hipError_t dev_with_tmp(DevArr<unsigned char>& tmp, F f) {
    size_t b = 0;
    hipError_t e = f(nullptr, b);
    if (e == hipSuccess) e = tmp.reserve(b, 0);
    return e == hipSuccess ? f((void*)tmp.p, b) : e;
}
// (the iterator types are the callers' own, so the kernels rocPRIM instantiates are the ones it always did)
#define PG_DEV_SORT_PAIRS [=](void* t, size_t& b) { return rocprim::radix_sort_pairs<rocprim::default_config, KI, KO, VI, VO, size_t>(t, b, kin, kout, vin, vout, n, 0u, bits, st); }
#define PG_DEV_SORT_KEYS [=](void* t, size_t& b) { return rocprim::radix_sort_keys<rocprim::default_config, KI, KO, size_t>(t, b, kin, kout, n, 0u, bits, st); }
#define PG_DEV_EXCL_SUM [=](void* t, size_t& b) { using V = typename std::iterator_traits<Out>::value_type; return rocprim::exclusive_scan(t, b, in, out, V(0), n, rocprim::plus<V>(), st); }
#define PG_DEV_INCL_SCAN [=](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, n, op, st); }
template <typename KI, typename KO, typename VI, typename VO>
inline size_t dev_sort_pairs_bytes(KI kin, KO kout, VI vin, VO vout, size_t n, unsigned bits, hipStream_t st) { return dev_tmp_bytes(PG_DEV_SORT_PAIRS); }
template <typename KI, typename KO, typename VI, typename VO>
inline hipError_t dev_sort_pairs(DevArr<unsigned char>& tmp, KI kin, KO kout, VI vin, VO vout, size_t n, unsigned bits, hipStream_t st) { return dev_with_tmp(tmp, PG_DEV_SORT_PAIRS); }
template <typename KI, typename KO>
inline hipError_t dev_sort_keys(DevArr<unsigned char>& tmp, KI kin, KO kout, size_t n, unsigned bits, hipStream_t st) { return dev_with_tmp(tmp, PG_DEV_SORT_KEYS); }
template <typename In, typename Out>
inline size_t dev_exclusive_sum_bytes(In in, Out out, size_t n, hipStream_t st) { return dev_tmp_bytes(PG_DEV_EXCL_SUM); }
template <typename In, typename Out>
inline hipError_t dev_exclusive_sum(DevArr<unsigned char>& tmp, In in, Out out, size_t n, hipStream_t st) { return dev_with_tmp(tmp, PG_DEV_EXCL_SUM); }
template <typename In, typename Out, typename Op>
inline hipError_t dev_inclusive_scan(DevArr<unsigned char>& tmp, In in, Out out, size_t n, Op op, hipStream_t st) { return dev_with_tmp(tmp, PG_DEV_INCL_SCAN); }
#undef PG_DEV_SORT_PAIRS
#undef PG_DEV_SORT_KEYS
#undef PG_DEV_EXCL_SUM
#undef PG_DEV_INCL_SCAN

// ---- A listing into a capped array.  The kernels count every hit and write those that fit; a listing that was short comes again, once, with
// exact room (or with `upper`, the caller's bound, where a second run may count differently).  launch(list, cap, stream) zeroes its counters and
// queues the kernels; `d_cnt` is `words` (<= 4) counters of the caller's on the current device, read back behind them, word `at` the hits.
// begin() queues the first attempt and end() waits for it, so several lanes list side by side: begin() on each, then end() on each, either
// with the lane's device current.  PG_EB_LIST_ROOM=n (test hook) is the first attempt's room, so that inputs of test size are short of it.
template <typename T>
struct DevListing {
    DevArr<T> list;
    unsigned long long cap = 0, cnt[4] = {0, 0, 0, 0};
    const unsigned long long* d_cnt = nullptr;
    int words = 1, at = 0;
    unsigned long long n() const { return cnt[at]; }
    bool short_of_room() const { return n() > cap; }                              // (behind end(): the second attempt was short as well)
    template <typename L> hipError_t attempt(unsigned long long room, hipStream_t st, L& launch) {
        cap = room;
        list.reset();
        hipError_t e = list.alloc((size_t)cap);
        if (e == hipSuccess) e = launch(list.p, cap, st);
        return e == hipSuccess ? hipMemcpyAsync(cnt, d_cnt, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) : e;
    }
    template <typename L> hipError_t begin(unsigned long long first_cap, const unsigned long long* counters, int n_words, int hits_at, hipStream_t st, L launch) {
        d_cnt = counters; words = n_words; at = hits_at;
        if (const char* v = env_test("PG_EB_LIST_ROOM")) first_cap = (unsigned long long)std::max(1LL, atoll(v));
        return attempt(first_cap, st, launch);
    }
    template <typename L> hipError_t end(const char* what, unsigned long long upper, hipStream_t st, L launch) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess || !short_of_room()) return e;
        if (env_user("PG_HOST_VERBOSE")) fprintf(stderr, "%s listed again: %llu of them, the first room was for %llu\n", what, n(), cap);
        e = attempt(upper ? upper : n(), st, launch);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }
};

}  // namespace pg
