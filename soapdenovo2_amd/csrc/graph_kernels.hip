// graph_kernels.hip -- the graph stages of pregraph that run on the device, on one copy of the k-mer sets in HBM:
//   tip_*   the walks of tip clipping                 (clipTipFromNode, cutTipPreGraph.c:43-346)
//   eb_*    edge construction                         (make_edge / stringBeads / merge_linearV2, node2edge.c:61-649)
//   p2_*    pass 2: read threading and the pre-arcs   (prlRead2edge, prlRead2path.c:786-1370)
// The sets come over exactly as the host's layout replay left them (slot arrays in the reference's own layout, an empty
// slot carries an impossible key), so every lookup is the reference's: set = signext(crc32) % thrd_num, slot = key mod
// size, linear probing (newhash.c:277-318).
//
// Pass 2: p2_kernels.hpp (its kernels and launches, a part of this file), p2_walk.hpp (parse1read, shared with the host twin), graph_lookup.hpp (sv_node_word).
// All integer work, HBM-latency bound (one random 24/40-byte probe per k-mer); nothing here is shaped for MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "arena.hpp"
#include "dev_scratch.hpp"
#include "env.hpp"
#include "device_ctx.hpp"
#include "extract.hpp"
#include "kmer.hpp"
#include "graph_dev.hpp"
#include "host_graph.hpp"
#include "graph_lookup.hpp"
#include "cmd_plan.hpp"
#include "backend_hip.hpp"
#include "dev_graph.hpp"
#include "dev_rehash.hpp"
#include "dev_tips.hpp"

namespace pg {

// a HIP call of a stage function: on failure the message is set and the function returns (its scratch lives in owners, dev_scratch.hpp)
#define P2_HIP_AS(prefix, call)                                                                              \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            pg_set_error(std::string(prefix) + #call + ": " + hipGetErrorString(e_));                        \
            return PG_ENODEV;                                                                                  \
        }                                                                                                    \
    } while (0)
#define P2_HIP(call) P2_HIP_AS("pass 2: ", call)
#define EB_HIP(call) P2_HIP_AS("edges: ", call)
// (a function that went from lane to lane leaves with the lead's device current, however it leaves)
struct P2BackOn { int device; ~P2BackOn() { (void)hipSetDevice(device); } };

// The kernels are templates over NW (2: the 63-mer build, 4: the 127-mer build): the launch of `kernel`, written with NW in its template arguments.
// (The macro declares a constant named NW in each branch: the kernel argument must spell the width `NW`, as in (eb_walk<NW>), or it does not follow `nw`.)
#define P2_LAUNCH_NW(nw, kernel, ...)                                                  \
    do {                                                                               \
        if ((nw) == 2) { constexpr int NW = 2; hipLaunchKernelGGL(kernel, __VA_ARGS__); } \
        else { constexpr int NW = 4; hipLaunchKernelGGL(kernel, __VA_ARGS__); }           \
    } while (0)

// a copy between two devices of the process (or inside one)
static hipError_t p2r_copy(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
    if (!bytes) return hipSuccess;
    if (dst_dev == src_dev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
}
constexpr uint64_t P2_EMPTY = ~0ULL;
constexpr int P2_MAX_SETS = 255;

struct P2Params {
    const uint64_t* geo3;               // per set (SV_GEO words): first global slot, size, address of its slot 0 ((NW + 1) words a slot: key
                                        // words, then A | B << 32), the size's reciprocal (graph_lookup.hpp: ModConst); the sets of one graph may
                                        // lie on several GPUs of the process
    const uint64_t* look;               // pass 2's lookup table (p2_make_look) or null: every key of the sets with its node word, two 32-byte entries a
    uint64_t look_buckets;              // 64-byte bucket (K <= 63; one 64-byte entry a bucket at K <= 127), probed from the bucket the key hashes to
    uint32_t P, bias;
    int K;
    // (K+1)-mer patch table
    const uint64_t* patch_keys;         // NW words an entry
    const uint32_t* patch_val;          // id, twin an entry; id 0 = empty
    uint64_t patch_mask;
    // pre-arc table
    unsigned long long* arc;            // ARC_WORDS words an entry: from << 32 | to (0 = empty), the earliest meeting (read ordinal << 16 | item), the
    uint64_t arc_mask;                  // multiplicity (32 bits), padding -- 32 bytes, so that one pre-arc touches ONE 64-byte line (add_prearc)
    // -R
    uint32_t* stage;                    // [read in batch][max_nk]
    uint16_t* walk_len;                 // valid entries per read (0 when the walk does not qualify)
    unsigned int* marker;               // per edge
    int max_nk;
    uint32_t id_end;                    // num_ed + 1
    // counters: 0 reads without any usable item, 1 lookups that found nothing, 2 arc table overflow, 3 distinct arcs,
    // 4 markers, 5 edge id out of range
    unsigned long long* counters;
};

// every kernel below starts the same way: CRC table and set geometry into LDS, a SetsView over them (graph_lookup.hpp:
// sv_find / sv_step / sv_node are the reference's search_kmerset on per-set base addresses)
#define P2_PROLOGUE(p)                                                                               \
    __shared__ uint32_t crc_tab[256];                                                                \
    __shared__ uint64_t set_geo[SV_GEO * P2_MAX_SETS];                                               \
    crc_tab[threadIdx.x] = crc32_table_entry(threadIdx.x);                                           \
    for (int q_ = threadIdx.x; q_ < SV_GEO * (int)(p).P; q_ += 256) set_geo[q_] = (p).geo3[q_];      \
    __syncthreads();                                                                                 \
    const SetsView sv{set_geo, crc_tab, (p).P, (p).bias, (p).K}

constexpr int ARC_WORDS = 4;                       // words an entry of the pre-arc table (p2_kernels.hpp: add_prearc)
static_assert(ARC_WORDS * 8 == (int)CMD_PREARC_ENTRY_BYTES, "the plan's entry size");
constexpr int P2R_MAX_LANES = 16;                    // routed pass 2: per-thread counters in LDS, 16 x 256 words

// =====================================================================================================================
// Edge construction on the device (make_edge / startEdgeFromNode / stringBeads / merge_linearV2, node2edge.c:61-649).
// A chain of linear nodes between two branch nodes has exactly two entrances; the reference's slot-order scan emits it
// from the entrance it meets first and unlinks the other.  Walks read nothing an earlier emit changes, hence:
//   eb_list_branch   every occupied, non-linear, non-deleted slot (the vertices), in any order
//   eb_walk          a lane per (vertex, arc): walk to the next branch node; keep the walk unless the position of its other
//                    entrance (global slot, arc order) precedes its own; a walk that is its own twin is a palindrome
//   sort by (slot, arc) + prefix sums    edge ids and text offsets in the reference's order
//   eb_apply         a lane per kept walk: walk again, write the bases, tag the interior nodes with the edge id, unlink the
//                    two end arcs, enter the (K+1)-mer of a length-1 edge into the device copy of KmerSetsPatch
// The host only formats the text records (output_1edge, output_pregraph.c:88-110).
// =====================================================================================================================
struct EdgeRec {                      // one kept walk
    unsigned long long key;           // (global slot of the start node) << 3 | arc order (right arcs 0..3, left arcs 4..7)
    unsigned long long far_slot;
    unsigned long long sum;           // sum of the left-arc counters of the interior nodes (coverage)
    uint32_t length;                  // bases = nodes on the walk - 1
    uint32_t flags;                   // next_ch | prev_ch << 2 | first_smaller << 4 | last_smaller << 5 | bal << 6
    uint64_t first_kmer[4], last_kmer[4];
};

template <int NW>
struct WalkState {
    Kmer<NW> first, cur, prev;        // walk-oriented k-mers: start node, latest node, the one before it
    uint64_t cur_slot;
    uint64_t ab;                      // counter words of the latest node
    bool cur_smaller;
    uint32_t count;                   // nodes on the walk so far
    int next_ch;                      // last base of the second node
};

// ---- waypoints: chains of linear nodes far longer than a lane should walk -------------------------------------------------------
// A walk is serial by nature (the next node is a function of the present one), and the reference's graph of a nearly repeat-free
// genome at a large K is a few hundred chains of millions of nodes: one lane a chain took 23.5 s for the edges of the 60 M-read
// K = 127 run (the reference: 103 s).  So every linear node whose global slot hashes to 0 modulo a period is a WAYPOINT:
//   eb_way_walk   a lane per (waypoint, direction) walks to the next waypoint or branch node: expected `period` steps, all at once;
//   eb_walk       steps node by node until it meets a waypoint, then JUMPS from waypoint to waypoint through those segments (count and
//                 coverage sum added up), noting at every waypoint it passes which walk it is and how many nodes it has behind it;
//   eb_apply      writes the bases and tags the nodes up to the first waypoint; eb_apply_seg, a lane per (waypoint, direction) a KEPT
//                 walk passed, does the segment behind it -- at the text offset and with the edge id the walk's record got.
// Same records, same text, same tags as the node-by-node walk (SOAPDENOVO2_AMD_EB_WAYPOINTS=0; a period of 4 in the tests puts
// waypoints into every chain of the golden cases).
struct EbWay {
    unsigned long long* key;          // open addressing: global slot + 1 of a waypoint, 0 = free; cap = mask + 1 entries
    uint64_t mask;
    unsigned long long* seg_end;      // [2 cap] entry 2 h + d: the stop of the segment that leaves waypoint h forward (d = 0: as its canonical k-mer reads) / backward
    unsigned long long* seg_info;     //         nodes stepped (the stop is the n-th) | stop is a waypoint << 32 | stop's k-mer is canonical in walk direction << 33 |
                                      //         first base of the k-mer in front of the stop << 34
    unsigned long long* seg_sum;      //         left-arc counters of the nodes strictly between (coverage)
    unsigned long long* vis_own;      // [2 cap] the walk (EdgeRec::key) that passed the waypoint leaving that way, ~0 = none
    unsigned int* vis_info;           //         nodes on that walk up to and including the waypoint | the base it leaves by << 30
    uint32_t period_mask;             // waypoint <=> linear, live and (slot_hash(slot) & period_mask) == 0
};
__device__ __forceinline__ bool eb_is_way(uint64_t g, uint32_t pm) { return ((uint32_t)slot_hash(g) & pm) == 0; }
__device__ __forceinline__ uint64_t eb_way_home(uint64_t g, uint64_t mask) { return (slot_hash(g) >> 24) & mask; }      // (other bits than the test above looks at)
__device__ __forceinline__ uint64_t eb_way_find(const EbWay& w, uint64_t g) {           // ~0: not a waypoint (the caller counts an error)
    uint64_t h = eb_way_home(g, w.mask);
    for (uint64_t step = 0; step <= w.mask; step++) {
        const unsigned long long k = w.key[h];
        if (k == g + 1) return h;
        if (k == 0) break;
        h = (h + 1) & w.mask;
    }
    return ~0ULL;
}
__global__ void eb_way_insert(EbWay w, const unsigned long long* list, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long g = list[i];
        uint64_t h = eb_way_home(g, w.mask);
        for (;;) {
            const unsigned long long old = atomicCAS(&w.key[h], 0ULL, g + 1);
            if (old == 0 || old == g + 1) break;
            h = (h + 1) & w.mask;
        }
    }
}

// one set's vertices (live non-linear nodes) as global slots, in any order -- or (way_mask != 0xFFFFFFFF... see `ways`) its waypoints
// (cap: room in `list`; what does not fit is still counted, so the caller can come again with a list that holds them all).
// The hits of a workgroup are collected in LDS and get their room in the list ~1000 at a time: appended one returned atomic apiece,
// 2.6 M vertices took 29 ms at 60 M reads -- the rate ONE address serves atomics at (88 per microsecond), not the scan's.
__global__ __launch_bounds__(256) void eb_list_branch(const uint64_t* nodes, int nw1, uint64_t n_slots, uint64_t first, unsigned long long* list, unsigned long long* n_list,
                                                      unsigned long long cap, int ways = 0, uint32_t period_mask = 0) {
    constexpr unsigned FLUSH = 1024;
    __shared__ unsigned long long buf[FLUSH + 256];
    __shared__ unsigned int s_n;
    __shared__ unsigned long long s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    // `held` = the entries in buf, the same number in every lane (the barrier that ends a trip counts the trip's hits): the decision to flush is
    // taken on it, never on s_n itself -- a wave that is already a trip ahead adds to s_n while a slower one still looks at it, the workgroup would
    // disagree about entering flush() and its barriers would pair up wrongly
    unsigned int held = 0;
    auto flush = [&]() {                                                   // (called by the whole workgroup, behind a barrier)
        if (threadIdx.x == 0 && held) { s_base = atomicAdd(n_list, (unsigned long long)held); s_n = 0; }
        __syncthreads();
        for (unsigned int j = threadIdx.x; j < held; j += 256) { const unsigned long long at = s_base + j; if (at < cap) list[at] = buf[j]; }
        __syncthreads();
        held = 0;
    };
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < n_slots; i0 += (uint64_t)gridDim.x * 256) {
        const uint64_t i = i0 + threadIdx.x;
        bool hit = false;
        if (i < n_slots) {
            const uint64_t* nd = nodes + i * nw1;
            const uint32_t B = (uint32_t)(nd[nw1 - 1] >> 32);
            hit = nd[0] != P2_EMPTY && (ways ? ((B & B_LINEAR) && eb_is_way(first + i, period_mask)) : !(B & (B_LINEAR | B_DELETED)));
        }
        if (hit) buf[atomicAdd(&s_n, 1u)] = first + i;
        held += (unsigned int)__syncthreads_count(hit ? 1 : 0);
        if (held > FLUSH) flush();
    }
    flush();
}

// the segment that leaves waypoint list[t / 2] forward (t even) or backward: to the next waypoint or branch node
template <int NW>
__global__ __launch_bounds__(256) void eb_way_walk(P2Params p, EbWay way, const unsigned long long* list, uint64_t t0, uint64_t n_share, unsigned long long* errors) {
    P2_PROLOGUE(p);
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // this launch's share of the 2 n (waypoint, direction) pairs: [t0, t0 + n_share)
    if (q >= n_share) return;
    const uint64_t t = t0 + q;
    const uint64_t g0 = list[t >> 1];
    const int d = (int)(t & 1);
    const uint64_t h = eb_way_find(way, g0);
    if (h == ~0ULL) { atomicAdd(errors, 1ULL); return; }
    const uint64_t* nd0 = sv_node<NW>(sv, g0);
    const int K = p.K;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    Kmer<NW> seq;
#pragma unroll
    for (int i = 0; i < NW; i++) seq.w[i] = nd0[i];
    Kmer<NW> prev = d ? kmer_rc<NW>(seq, K) : seq;
    Kmer<NW> cur = kmer_next<NW>(prev, linear_out_ab(nd0[NW], d == 0), filter);
    uint64_t slot, ab;
    uint64_t* node;
    bool smaller;
    unsigned long long sum = 0, count = 0;
    for (;;) {
        if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
        ab = node[NW];
        count++;
        const bool linear = ((uint32_t)(ab >> 32) & B_LINEAR) != 0;
        if (!linear || eb_is_way(slot, way.period_mask)) {
            way.seg_end[2 * h + d] = slot;
            way.seg_info[2 * h + d] = count | ((unsigned long long)(linear ? 1 : 0) << 32) | ((unsigned long long)(smaller ? 1 : 0) << 33) |
                                      ((unsigned long long)kmer_first<NW>(prev, K) << 34);
            way.seg_sum[2 * h + d] = sum;
            return;
        }
        const uint32_t A = (uint32_t)ab;
        sum += (A & 63) + ((A >> 6) & 63) + ((A >> 12) & 63) + ((A >> 18) & 63);
        prev = cur;
        cur = kmer_next<NW>(cur, linear_out_ab(ab, smaller), filter);
    }
}

template <int NW>
__global__ __launch_bounds__(256) void eb_walk(P2Params p, const unsigned long long* list, uint64_t t0, uint64_t n_share, EdgeRec* out, uint64_t cap,
                                               unsigned long long* n_out, unsigned long long* n_len1, unsigned long long* errors, EbWay way) {
    P2_PROLOGUE(p);
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // this launch's share of the 8 n_list (vertex, arc) pairs: [t0, t0 + n_share)
    if (q >= n_share) return;
    const uint64_t t = t0 + q;
    const uint64_t slot0 = list[t >> 3];
    const int order = (int)(t & 7);
    const uint64_t* nd0 = sv_node<NW>(sv, slot0);
    const uint64_t ab0 = nd0[NW];
    const int ch = order & 3;
    const bool right = order < 4;
    if (!(((right ? (uint32_t)(ab0 >> 32) : (uint32_t)ab0) >> (6 * ch)) & 63)) return;      // no such arc
    const int K = p.K;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    Kmer<NW> seq;
#pragma unroll
    for (int i = 0; i < NW; i++) seq.w[i] = nd0[i];
    const Kmer<NW> first = right ? seq : kmer_rc<NW>(seq, K);
    const int nextch = right ? ch : (ch ^ 2);
    // stringBeads
    Kmer<NW> prev = first, cur = kmer_next<NW>(first, nextch, filter);
    uint64_t slot, ab;
    uint64_t* node;
    bool smaller;
    if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
    ab = node[NW];
    const int next_ch = kmer_last<NW>(cur);
    uint32_t count = 2;
    unsigned long long sum = 0;
    const unsigned long long own = ((unsigned long long)slot0 << 3) | (unsigned)order;
    int prev_known = -1;                                            // the first base of the k-mer in front of `cur`, when a jump brought us here
    while ((uint32_t)(ab >> 32) & B_LINEAR) {
        const uint32_t A = (uint32_t)ab;
        sum += (A & 63) + ((A >> 6) & 63) + ((A >> 12) & 63) + ((A >> 18) & 63);
        if (way.key && eb_is_way(slot, way.period_mask)) {
            // a waypoint: leave a note (which walk, how far in, which way out) and take its segment in one step
            const uint64_t h = eb_way_find(way, slot);
            if (h == ~0ULL) { atomicAdd(errors, 1ULL); return; }
            const int d = smaller ? 0 : 1;
            way.vis_own[2 * h + d] = own;
            way.vis_info[2 * h + d] = count | ((unsigned int)linear_out_ab(ab, smaller) << 30);
            const unsigned long long info = way.seg_info[2 * h + d];
            count += (uint32_t)info;
            sum += way.seg_sum[2 * h + d];
            slot = way.seg_end[2 * h + d];
            smaller = (info >> 33) & 1;
            prev_known = (int)((info >> 34) & 3);
            node = sv_node<NW>(sv, slot);
            ab = node[NW];
            Kmer<NW> kk;
#pragma unroll
            for (int i = 0; i < NW; i++) kk.w[i] = node[i];
            cur = smaller ? kk : kmer_rc<NW>(kk, K);
            continue;
        }
        prev = cur;
        prev_known = -1;
        cur = kmer_next<NW>(cur, linear_out_ab(ab, smaller), filter);
        if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
        ab = node[NW];
        count++;
    }
    const int prev_ch = prev_known >= 0 ? prev_known : kmer_first<NW>(prev, K);
    // where the slot-order scan would start this chain from its other end
    const unsigned long long twin = ((unsigned long long)slot << 3) | (unsigned)(smaller ? 4 + prev_ch : (prev_ch ^ 2));
    if (twin < own) return;
    EdgeRec r;
    r.key = own; r.far_slot = slot; r.sum = sum; r.length = count - 1;
    const uint32_t bal = twin != own;
    r.flags = (uint32_t)next_ch | ((uint32_t)prev_ch << 2) | ((right ? 1u : 0u) << 4) | ((smaller ? 1u : 0u) << 5) | (bal << 6);
#pragma unroll
    for (int i = 0; i < 4; i++) { r.first_kmer[i] = i < NW ? first.w[i] : 0; r.last_kmer[i] = i < NW ? cur.w[i] : 0; }
    const unsigned long long at = atomicAdd(n_out, 1ULL);
    if (at < cap) out[at] = r;                                      // the host checks the count against the capacity
    if (count == 2) atomicAdd(n_len1, 1ULL);
}

__global__ void eb_keys(const EdgeRec* recs, uint64_t n, unsigned long long* key, uint32_t* idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) { key[i] = recs[i].key; idx[i] = (uint32_t)i; }
}
// per kept walk in slot order: ids it takes (1 + bal) and bases it writes
__global__ void eb_sizes(const EdgeRec* recs, const uint32_t* order, uint64_t n, unsigned long long* ids, unsigned long long* bases) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const EdgeRec& r = recs[order[i]];
        ids[i] = 1 + ((r.flags >> 6) & 1);
        bases[i] = r.length;
    }
}

// what the host formats, in slot order
__global__ void eb_export(const EdgeRec* recs, const uint32_t* order, const unsigned long long* base_before, uint64_t n, P2EdgeRec* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const EdgeRec& r = recs[order[i]];
        P2EdgeRec o;
        o.length = r.length; o.bal = (r.flags >> 6) & 1; o.sum = r.sum; o.text_off = base_before[i];
        for (int k = 0; k < 4; k++) { o.first_kmer[k] = r.first_kmer[k]; o.last_kmer[k] = r.last_kmer[k]; }
        out[i] = o;
    }
}

// the segment behind a waypoint a kept walk passed: bases and tags as eb_apply writes them, at the walk's text offset and with its id
template <int NW>
__global__ __launch_bounds__(256) void eb_apply_seg(P2Params p, EbWay way, const EdgeRec* recs, const uint32_t* order, const unsigned long long* sorted_key, uint64_t n_rec,
                                                    const unsigned long long* id_before, const unsigned long long* base_before, char* text, unsigned long long* errors,
                                                    uint64_t t0, uint64_t n_share) {
    P2_PROLOGUE(p);
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // this launch's share of the table's 2 (mask + 1) entries
    if (q >= n_share) return;
    const uint64_t t = t0 + q;
    const unsigned long long own = way.vis_own[t];
    if (own == ~0ULL) return;
    // the walk's record, if it was kept (binary search over the records' keys in slot order)
    uint64_t lo = 0, hi = n_rec;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (sorted_key[mid] < own) lo = mid + 1; else hi = mid; }
    if (lo >= n_rec || sorted_key[lo] != own) return;
    const EdgeRec& r = recs[order[lo]];
    const uint32_t id = (uint32_t)id_before[lo] + 1, bal = (r.flags >> 6) & 1;
    if (!bal) return;                                                   // a walk that is its own twin passed this waypoint both ways: eb_apply does all of it
    const uint64_t h = t >> 1;
    const int d = (int)(t & 1);
    const unsigned int vi = way.vis_info[t];
    const uint32_t c_w = vi & 0x3FFFFFFFu;                              // nodes on the walk up to and including the waypoint
    const unsigned long long info = way.seg_info[t];
    const uint32_t n = (uint32_t)info;
    const bool end_is_way = (info >> 32) & 1;
    const int K = p.K;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const uint64_t g0 = way.key[h] - 1;
    const uint64_t* nd0 = sv_node<NW>(sv, g0);
    Kmer<NW> seq;
#pragma unroll
    for (int i = 0; i < NW; i++) seq.w[i] = nd0[i];
    Kmer<NW> cur = kmer_next<NW>(d ? kmer_rc<NW>(seq, K) : seq, (int)(vi >> 30), filter);   // (the way out was noted by the walk: the waypoint's own word is being tagged by another lane)
    char* out = text + base_before[lo] + (c_w - 1);                     // the c-th node of a walk writes base c - 2
    uint64_t slot, ab;
    uint64_t* node;
    bool smaller;
    for (uint32_t j = 1; j <= n; j++) {
        if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
        ab = node[NW];
        out[j - 1] = "ACTG"[kmer_last<NW>(cur)];
        if (j == n && !end_is_way) break;                               // the far branch node
        const uint32_t A = smaller ? id : id + bal;
        const uint32_t twin = smaller ? bal + 1 : 1 - bal;
        const uint32_t B = ((uint32_t)(ab >> 32) & 0x0FFFFFFFu) | (twin << B_TWIN_SHIFT) | (1u << B_INEDGE_SHIFT);
        const int o = linear_out_ab(ab, smaller);
        node[NW] = (uint64_t)A | ((uint64_t)B << 32);
        cur = kmer_next<NW>(cur, o, filter);
    }
    if (slot != way.seg_end[t]) atomicAdd(errors, 1ULL);
}

template <int NW>
__global__ __launch_bounds__(256) void eb_apply(P2Params p, const EdgeRec* recs, const uint32_t* order, uint64_t i0, uint64_t n_share,
                                                const unsigned long long* id_before, const unsigned long long* base_before, char* text,
                                                uint64_t* patch_keys, uint32_t* patch_val, uint64_t patch_mask, unsigned long long* errors, EbWay way) {
    P2_PROLOGUE(p);
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // this launch's share of the kept walks (in slot order): [i0, i0 + n_share)
    if (q >= n_share) return;
    const uint64_t i = i0 + q;
    const EdgeRec r = recs[order[i]];
    const int K = p.K;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    const uint32_t id = (uint32_t)id_before[i] + 1;
    const uint32_t bal = (r.flags >> 6) & 1;
    const int next_ch = r.flags & 3, prev_ch = (r.flags >> 2) & 3;
    const bool first_smaller = (r.flags >> 4) & 1, last_smaller = (r.flags >> 5) & 1;
    char* seq = text + base_before[i];
    Kmer<NW> first;
#pragma unroll
    for (int k = 0; k < NW; k++) first.w[k] = r.first_kmer[k];
    const uint64_t slot0 = r.key >> 3;
    // walk again: bases out, interior nodes tagged (edge id replaces word A, twin / inEdge in word B)
    Kmer<NW> cur = kmer_next<NW>(first, next_ch, filter);
    uint64_t slot, ab;
    uint64_t* node;
    bool smaller;
    bool handed_over = false;                                       // the rest of the walk belongs to the lanes of eb_apply_seg
    if (!bal) {
        // A walk that is its own twin passes every interior node twice, there and back, and the way out of a node met against its canonical
        // k-mer is read from word A -- which the tag replaces.  So: the bases first, node by node and past every waypoint, with nothing written;
        // then the tags over the first half of the walk, which is every interior node once (both passes would write the same: id, twin 1).
        for (uint32_t b = 0; b < r.length; b++) {
            if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
            seq[b] = "ACTG"[kmer_last<NW>(cur)];
            if (b + 1 == r.length) break;
            cur = kmer_next<NW>(cur, linear_out_ab(node[NW], smaller), filter);
        }
        if (slot != r.far_slot) { atomicAdd(errors, 1ULL); return; }
        cur = kmer_next<NW>(first, next_ch, filter);
        for (uint32_t b = 0; 2 * (b + 1) < r.length; b++) {
            uint64_t at;
            if (!sv_step<NW>(sv, cur, at, node, smaller)) { atomicAdd(errors, 1ULL); return; }
            ab = node[NW];
            const uint32_t B = ((uint32_t)(ab >> 32) & 0x0FFFFFFFu) | (1u << B_TWIN_SHIFT) | (1u << B_INEDGE_SHIFT);
            node[NW] = (uint64_t)id | ((uint64_t)B << 32);
            cur = kmer_next<NW>(cur, linear_out_ab(ab, smaller), filter);
        }
    }
    for (uint32_t b = 0; bal && b < r.length; b++) {
        if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
        ab = node[NW];
        seq[b] = "ACTG"[kmer_last<NW>(cur)];
        if (b + 1 == r.length) break;                               // the far branch node
        const uint32_t A = smaller ? id : id + bal;
        const uint32_t twin = smaller ? bal + 1 : 1 - bal;
        const uint32_t B = ((uint32_t)(ab >> 32) & 0x0FFFFFFFu) | (twin << B_TWIN_SHIFT) | (1u << B_INEDGE_SHIFT);
        const int out = linear_out_ab(ab, smaller);
        node[NW] = (uint64_t)A | ((uint64_t)B << 32);
        if (way.key && eb_is_way(slot, way.period_mask)) { handed_over = true; break; }
        cur = kmer_next<NW>(cur, out, filter);
    }
    if (!handed_over && slot != r.far_slot) { atomicAdd(errors, 1ULL); return; }
    // dislink2prevUncertain on the far node, dislink2nextUncertain on the start node (64-bit word: A low, B high)
    {
        const int bit = last_smaller ? 6 * prev_ch : 32 + 6 * (prev_ch ^ 2);
        // (system scope: the node may lie in another GPU's memory)
        __hip_atomic_fetch_and((unsigned long long*)(sv_node<NW>(sv, r.far_slot) + NW), ~(63ULL << bit), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int bit0 = first_smaller ? 32 + 6 * next_ch : 6 * (next_ch ^ 2);
        __hip_atomic_fetch_and((unsigned long long*)(sv_node<NW>(sv, slot0) + NW), ~(63ULL << bit0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (r.length == 1) {                                            // KmerSetsPatch (node2edge.c:481-542)
        Kmer<NW> last;
#pragma unroll
        for (int k = 0; k < NW; k++) last.w[k] = r.last_kmer[k];
        const Kmer<NW> plus = kmer_plus<NW>(first, kmer_last<NW>(last));
        const Kmer<NW> bal_plus = rc_plus<NW>(plus, K);
        const bool sm = kmer_less<NW>(plus, bal_plus);
        const Kmer<NW> key = sm ? plus : bal_plus;
        const uint32_t pid = sm ? id : id + bal, ptwin = sm ? bal + 1 : 1 - bal;
        uint64_t h = kmer_mix<NW>(key) & patch_mask;
        for (;;) {
            // (system scope: in a sharded run the walks are dealt to all lanes, and the table is the lead's)
            unsigned int old = 0u;
            (void)__hip_atomic_compare_exchange_strong(&patch_val[2 * h], &old, pid, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (old == 0) {
#pragma unroll
                for (int k = 0; k < NW; k++) patch_keys[h * NW + k] = key.w[k];
                patch_val[2 * h + 1] = ptwin;
                break;
            }
            h = (h + 1) & patch_mask;
        }
    }
}


// =====================================================================================================================
// Tip walks on the device (the read-only half of clipTipFromNode, cutTipPreGraph.c:43-346).  A lane per slot: a dead-end,
// non-linear, non-deleted node (with `thin`: a frequency-one node) walks over linear nodes to the node it stops at.  The
// order-dependent half -- deciding and clipping in slot order -- stays on the host, which mirrors the nodes it changed
// back into the device copy (tip_mirror) and re-marks linear nodes on both sides (tip_remark).
// =====================================================================================================================
template <int NW>
__global__ __launch_bounds__(256) void tip_walk_kernel(P2Params p, const uint64_t* set_nodes, uint64_t first_slot, uint64_t n_slots, int cut_len, int thin,
                                                       P2TipWalk* out, uint64_t cap, unsigned long long* n_out, unsigned long long* errors) {
    P2_PROLOGUE(p);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const uint64_t* nd = set_nodes + i * (NW + 1);
    if (nd[0] == P2_EMPTY) return;
    const uint64_t ab0 = nd[NW];
    const uint32_t A0 = (uint32_t)ab0, B0 = (uint32_t)(ab0 >> 32);
    if (B0 & (B_LINEAR | B_DELETED)) return;
    if (thin && !(B0 & B_SINGLE)) return;
    const int in = count_arcs24(A0), outn = count_arcs24(B0);
    const bool fwd = in == 0 && outn == 1, bwd = in == 1 && outn == 0;
    if (!fwd && !bwd) return;
    const int K = p.K;
    const Kmer<NW> filter = kmer_filter<NW>(K);
    Kmer<NW> seq;
#pragma unroll
    for (int k = 0; k < NW; k++) seq.w[k] = nd[k];
    Kmer<NW> prev = fwd ? seq : kmer_rc<NW>(seq, K);
    int ch;
    if (fwd) { for (ch = 0; ch < 4; ch++) if ((B0 >> (6 * ch)) & 63) break; }
    else { for (ch = 0; ch < 4; ch++) if ((A0 >> (6 * ch)) & 63) break; ch ^= 2; }
    P2TipWalk w;
    w.pos = first_slot + i; w.far = ~0ULL; w.first = 0; w.far_smaller = 0;
    int count = 1;
    Kmer<NW> cur = kmer_next<NW>(prev, ch, filter);
    uint64_t slot, ab;
    uint64_t* node;
    bool smaller;
    if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
    ab = node[NW];
    bool reached = true;
    while ((uint32_t)(ab >> 32) & B_LINEAR) {
        count++;
        if (thin && !((uint32_t)(ab >> 32) & B_SINGLE)) break;
        if (count > cut_len) { reached = false; break; }
        prev = cur;
        cur = kmer_next<NW>(cur, linear_out_ab(ab, smaller), filter);
        if (!sv_step<NW>(sv, cur, slot, node, smaller)) { atomicAdd(errors, 1ULL); return; }
        ab = node[NW];
    }
    if (reached) { w.far = slot; w.first = (uint32_t)kmer_first<NW>(prev, K); w.far_smaller = smaller ? 1u : 0u; }
    const unsigned long long at = atomicAdd(n_out, 1ULL);
    if (at < cap) out[at] = w;
}

__global__ void tip_keys(const P2TipWalk* w, uint64_t n, unsigned long long* key, uint32_t* idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) { key[i] = w[i].pos; idx[i] = (uint32_t)i; }
}
__global__ void tip_gather(const P2TipWalk* w, const uint32_t* order, uint64_t n, P2TipWalk* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = w[order[i]];
}
template <int NW>
__global__ __launch_bounds__(256) void tip_mirror(P2Params p, const uint64_t* slots, const uint64_t* ab, uint64_t n) {
    P2_PROLOGUE(p);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) sv_node<NW>(sv, slots[i])[NW] = ab[i];
}
// Mark1in1outNode (cutTipPreGraph.c:532-564) over one set: a live non-linear node with one arc each way becomes linear
__global__ void tip_remark(uint64_t* nodes, int nw1, uint64_t n_slots) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t* nd = nodes + i * nw1;
        if (nd[0] == P2_EMPTY) continue;
        const uint64_t ab = nd[nw1 - 1];
        const uint32_t A = (uint32_t)ab, B = (uint32_t)(ab >> 32);
        if (B & (B_DELETED | B_LINEAR)) continue;
        if (count_arcs24(A) == 1 && count_arcs24(B) == 1) nd[nw1 - 1] = ab | ((uint64_t)B_LINEAR << 32);
    }
}

// the occupied slots of the pre-arc table: counted (one atomic a workgroup), then written out densely (order does not matter: the host
// sorts; a workgroup reserves room for its slots of a trip with one returned atomic)
__global__ __launch_bounds__(256) void p2_count_arcs(const unsigned long long* key /* the table: ARC_WORDS words an entry */, uint64_t cap, unsigned long long* n_out) {
    __shared__ unsigned int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256) mine += key[i * ARC_WORDS] != 0;
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(n_out, (unsigned long long)s_n);
}
__global__ __launch_bounds__(256) void p2_compact_arcs(const unsigned long long* tab, uint64_t cap, P2Arc* out, unsigned long long* n_out, unsigned long long out_cap) {
    __shared__ unsigned int s_n;
    __shared__ unsigned long long s_base;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < cap; i0 += (uint64_t)gridDim.x * 256) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const uint64_t i = i0 + threadIdx.x;
        const unsigned long long k = i < cap ? tab[i * ARC_WORDS] : 0ULL;
        unsigned int my = 0;
        if (k) my = atomicAdd(&s_n, 1u);
        __syncthreads();
        if (threadIdx.x == 0 && s_n) s_base = atomicAdd(n_out, (unsigned long long)s_n);
        __syncthreads();
        if (k && s_base + my < out_cap) out[s_base + my] = P2Arc{(uint32_t)(k >> 32), (uint32_t)k, (uint32_t)tab[i * ARC_WORDS + 2], tab[i * ARC_WORDS + 1]};
    }
}

// ---- the fold of the pre-arc table on the device (round 6; until then 26 M pre-arcs at 200 M reads went to the host as 24-byte entries and were
// bucketed and std::sort-ed there: 0.8 s of a 5.5 s command).  thread_add1preArc keeps, per source edge, a list with the NEWEST first-met target at
// its head and counts repeats (prlRead2path.c:388-403); output_1edge prints the lists in edge order (:426-476).  Here: the lanes' entries of one
// (from, to) pair are merged (multiplicities add up, the first meeting is the earliest), then two stable radix sorts -- by descending first
// meeting, then by source edge -- give the file order, and (from, to, multiplicity) goes to the host in that order, 12 bytes a pre-arc.
__global__ __launch_bounds__(256) void pf_pair_keys(const P2Arc* a, uint64_t n, unsigned long long* key, uint32_t* idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) { key[i] = ((unsigned long long)a[i].from << 32) | a[i].to; idx[i] = (uint32_t)i; }
}
__global__ __launch_bounds__(256) void pf_heads(const unsigned long long* key_sorted, uint64_t n, unsigned long long* head) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) head[i] = (i == 0 || key_sorted[i] != key_sorted[i - 1]) ? 1ULL : 0ULL;
}
__global__ __launch_bounds__(256) void pf_merge(const P2Arc* a, const unsigned long long* key_sorted, const uint32_t* order, const unsigned long long* head, const unsigned long long* pos,
                                                uint64_t n, P2Arc* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (!head[i]) continue;
        P2Arc m = a[order[i]];
        for (uint64_t j = i + 1; j < n && key_sorted[j] == key_sorted[i]; j++) {           // (at most one entry a lane)
            const P2Arc& b = a[order[j]];
            m.mult += b.mult;
            m.first = b.first < m.first ? b.first : m.first;
        }
        out[pos[i]] = m;
    }
}
__global__ __launch_bounds__(256) void pf_first_keys(const P2Arc* a, uint64_t n, unsigned long long* key, uint32_t* idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) { key[i] = ~a[i].first; idx[i] = (uint32_t)i; }
}
__global__ __launch_bounds__(256) void pf_from_keys(const P2Arc* a, const uint32_t* order, uint64_t n, unsigned long long* key) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) key[i] = a[order[i]].from;
}
__global__ __launch_bounds__(256) void pf_gather(const P2Arc* a, const uint32_t* order, uint64_t n, uint32_t* out3) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const P2Arc& x = a[order[i]];
        out3[3 * i] = x.from; out3[3 * i + 1] = x.to; out3[3 * i + 2] = x.mult;
    }
}
__global__ void p2_arc_init(unsigned long long* tab, uint64_t cap) {                // empty entries: no key, no meeting yet, multiplicity 0
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap * ARC_WORDS; i += (uint64_t)gridDim.x * blockDim.x) tab[i] = (i % ARC_WORDS) == 1 ? ~0ULL : 0ULL;
}

// ---------------------------------------------------------------------------------------------------------------------
// The graph on the device.  Kernels are launched on `device` (the lead rank's GPU); the k-mer sets may be spread over
// several GPUs of the process -- set s on set_dev[s], reached from the lead through peer mappings (xGMI) -- which is how
// the sharded run keeps every rank at its share of the sets ("reference set id -> GPU").
// One lane of the graph stages = one rank of a sharded run: a GPU of the process with a stream of its own.  The scans over the
// slots of a set run on the lane that owns the set (set s -> lane s mod n_lanes, the rank that laid it out; the reference gives
// every set one owner for its scans as well, prlHashReads.c:79-90, cutTipPreGraph.c:603-639), and pass 2 deals its read batches
// to the lanes in turn (every read has one worker, prlRead2path.c:248), each lane with its own pre-arc table, counters and
// batch buffers against the peer-mapped sets.  A pre-arc list is a multiplicity and a first-met order (prlRead2path.c:388-403):
// the lanes' tables merge by sum and minimum.  Lane 0 is the lead (its tables are the P2Device's own).
struct P2Lane {
    int device = 0;
    hipStream_t stream = nullptr;
    bool tables = false;                             // the pass-2 tables below exist
    P2Params prm;
    uint64_t* d_geo3 = nullptr;                      // copies on this lane's device (lane 0 and lanes on the lead's device: the lead's own)
    uint32_t* d_crc = nullptr;                       // (made by p2_use_lanes: the walks of the tip and edge stages run on every lane too)
    unsigned long long* d_wcnt = nullptr;            // [4] this lane's counters of a dealt step: -, kept walks, length-1 walks, errors
    uint64_t* d_patch_keys = nullptr;
    uint32_t* d_patch_val = nullptr;
    bool own_geo = false, own_patch = false;
    unsigned long long* d_arc = nullptr;             // the lane's pre-arc table (P2Params::arc)
    unsigned long long* d_counters = nullptr;
    unsigned int* d_marker = nullptr;
    // grow-only device buffers (the arena makes growing cheap), released with the lane: a batch's reads as the host packed them ...
    DevArr<uint64_t> d_words, d_off;
    DevArr<int32_t> d_lens;
    DevArr<uint32_t> d_stage;                        // ... and, with -R, its walks ([read in batch][max_nk]) and their lengths
    DevArr<uint16_t> d_walk_len;
    hipEvent_t copied = nullptr;
    uint64_t reads = 0, batches = 0, scans = 0;      // what the lane did (PG_HOST_VERBOSE; asserted by the sharded tests)
    uint64_t walks = 0;                              // tip / edge walks that started from a node of this lane's sets and ran here
    // ---- routed pass 2 (p2_route_round): a batch waits here until every lane has one
    struct Pending {
        bool have = false;
        const uint64_t* d_words = nullptr; const uint64_t* d_off = nullptr; const int32_t* d_lens = nullptr;
        uint64_t n_reads = 0, ordinal = 0, q = 0;    // q = k-mers of the batch (the lookups it asks for)
        int uniform_len = 0;
        uint32_t* walks_out = nullptr; uint16_t* walk_len_out = nullptr;
    } pend;
    uint8_t* d_owner_of_set = nullptr;
    DevArr<uint32_t> hist_in, hist;                  // (grow-only as well: reserve(n, n / 4 + 64))
    DevArr<unsigned char> scan_tmp;
    DevArr<uint64_t> send, ans;                      // as a reader of batches: the keys it asks for, the node words that come back
    DevArr<uint32_t> where;                          // starts[owner][read]: where a read's queries for an owner begin (its answers come back at the same places)
    DevArr<uint64_t> rkeys, rans;                    // as an owner of sets: the keys it is asked for, its answers
    uint32_t* h_starts = nullptr;                    // page-locked: where every owner's segment starts in this lane's send buffer, and the total
    uint64_t lookups_sent = 0, lookups_sent_away = 0, lookups_answered = 0, route_rounds = 0;
};

struct P2Device {
    int device = 0, K = 0, nw = 2, P = 1, max_nk = 0;
    std::vector<P2Lane> lanes;                       // lanes[0] = the lead
    std::vector<int> set_lane;                       // the lane that owns set s
    unsigned next_lane = 0;
    bool reps = false;
    uint32_t num_ed = 0;
    P2Params prm;
    std::vector<uint64_t> set_sizes, set_first;      // host copy of the geometry
    std::vector<int> set_dev;
    std::vector<uint64_t*> set_ptr;                  // address of every set's slot 0
    std::vector<std::pair<int, void*>> owned;        // (device, allocation) holding the sets
    uint64_t* d_geo3 = nullptr;                      // per set (first global slot, size, address of slot 0): P2Params::geo3, SetsView::geo
    uint32_t* d_crc = nullptr;                       // CRC-32 byte table for the lookups of the backend-generic stages
    uint64_t* d_patch_keys = nullptr;
    uint32_t* d_patch_val = nullptr;
    unsigned long long* d_counters = nullptr;        // the lead's counters of the stages in front of pass 2
    uint64_t ordinal = 0;
    uint64_t n_slots = 0;
    bool reads_ready = false;
    bool route = false;                              // pass 2's lookups go to the sets' owners (several lanes; SOAPDENOVO2_AMD_P2_ROUTE=0: peer-mapped probes)
    hipStream_t stream = nullptr;
    DevArr<unsigned long long> d_vlist;              // the vertices' global slots as p2_list_vertices left them (the edge builder starts from the same list)
    uint64_t* d_look = nullptr;                      // pass 2's lookup table (p2_make_look); gone again when pass 2 is (p2_finish)
    bool look_plain = false;
};

namespace { void forget_taken(void* ptr); }       // (the offered-block bookkeeping further down)
}  // namespace pg
#include "p2_kernels.hpp"      // pass 2: its kernels and the calls that launch them (p2_make_look / p2_drop_look, p2_add_packed*)
namespace pg {

static void p2_free(P2Device* d) {
    if (!d) return;
    for (auto& o : d->owned) { forget_taken(o.second); (void)hipSetDevice(o.first); (void)pg::arena_free(o.second); }
    for (size_t l = 0; l < d->lanes.size(); l++) {
        P2Lane& ln = d->lanes[l];
        (void)hipSetDevice(ln.device);
        if (ln.own_geo) { pg::arena_free(ln.d_geo3); pg::arena_free(ln.d_crc); }
        pg::arena_free(ln.d_wcnt);
        if (ln.own_patch) { pg::arena_free(ln.d_patch_keys); pg::arena_free(ln.d_patch_val); }
        pg::arena_free(ln.d_arc);
        if (l) pg::arena_free(ln.d_counters);
        pg::arena_free(ln.d_marker);
        pg::arena_free(ln.d_owner_of_set);
        if (ln.h_starts) (void)hipHostFree(ln.h_starts);
        if (ln.copied) (void)hipEventDestroy(ln.copied);
        if (l && ln.stream) (void)hipStreamDestroy(ln.stream);
    }
    hipSetDevice(d->device);
    pg::arena_free(d->d_patch_keys); pg::arena_free(d->d_patch_val);
    pg::arena_free(d->d_counters);
    pg::arena_free(d->d_geo3); pg::arena_free(d->d_crc);
    p2_drop_look(d);
    if (d->stream) hipStreamDestroy(d->stream);
    delete d;
}

// the sets are in place (set_sizes / set_dev / set_ptr filled): geometry to the lead, peer mappings, stream, counters
static int p2_finish_open(P2Device* d) {
    P2_HIP(hipSetDevice(d->device));
    if (!d->stream) P2_HIP(hipStreamCreate(&d->stream));
    memset(&d->prm, 0, sizeof(d->prm));
    std::vector<uint64_t> words(SV_GEO * (size_t)d->P);
    d->set_first.assign(d->P, 0);
    uint64_t first = 0;
    for (int s = 0; s < d->P; s++) {
        d->set_first[s] = first;
        const ModConst mc = make_modconst(d->set_sizes[s]);
        words[SV_GEO * s] = first; words[SV_GEO * s + 1] = d->set_sizes[s]; words[SV_GEO * s + 2] = (uint64_t)(uintptr_t)d->set_ptr[s];
        words[SV_GEO * s + 3] = mc.v; words[SV_GEO * s + 4] = mc.s;
        first += d->set_sizes[s];
        if (d->set_dev[s] != d->device) {                    // the lead reads and writes its peers' sets
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, d->device, d->set_dev[s]) != hipSuccess || !can) { pg_set_error("the GPUs holding the k-mer sets cannot map each other's memory"); return PG_ENODEV; }
            const hipError_t e = hipDeviceEnablePeerAccess(d->set_dev[s], 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { pg_set_error(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e)); return PG_ENODEV; }
            (void)hipGetLastError();
        }
    }
    d->n_slots = first;
    P2_HIP(pg::arena_malloc((void**)&d->d_geo3, words.size() * sizeof(uint64_t)));
    P2_HIP(hipMemcpy(d->d_geo3, words.data(), words.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    P2_HIP(pg::arena_malloc((void**)&d->d_crc, 256 * sizeof(uint32_t)));
    {
        uint32_t tab[256];
        for (uint32_t i = 0; i < 256; i++) tab[i] = crc32_table_entry(i);
        P2_HIP(hipMemcpy(d->d_crc, tab, sizeof tab, hipMemcpyHostToDevice));
    }
    P2_HIP(pg::arena_malloc((void**)&d->d_counters, 8 * sizeof(unsigned long long)));
    P2_HIP(hipMemsetAsync(d->d_counters, 0, 8 * sizeof(unsigned long long), d->stream));
    P2_HIP(hipStreamSynchronize(d->stream));
    P2Params& p = d->prm;
    p.geo3 = d->d_geo3;
    p.P = (uint32_t)d->P; p.bias = set_bias((uint32_t)d->P); p.K = d->K;
    p.max_nk = d->max_nk;
    p.counters = d->d_counters;
    // one lane until the caller names the ranks (p2_use_lanes)
    d->lanes.clear();
    d->lanes.emplace_back();
    d->lanes[0].device = d->device; d->lanes[0].stream = d->stream;
    d->set_lane.assign(d->P, 0);
    return PG_OK;
}

// the two devices can map each other's memory, and `from` has done so
static int p2_peer(int from, int to) {
    if (from == to) return PG_OK;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, from, to) != hipSuccess || !can) { pg_set_error("the GPUs of the sharded graph cannot map each other's memory"); return PG_ENODEV; }
    P2_HIP(hipSetDevice(from));
    const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
    (void)hipGetLastError();
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { pg_set_error(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e)); return PG_ENODEV; }
    return PG_OK;
}
// The ranks of a sharded run, lane 0 = the lead's device: from here on the per-set scans run on the owner's lane and pass 2 deals
// its batches to all of them.  Every lane maps every set's device (it probes all sets) and the lead maps every lane (it gathers
// their lists).  Ranks may share a device (test set-ups on one GPU): they are lanes of their own all the same.
int p2_use_lanes(P2Device* d, const int* lane_devices, int n_lanes) {
    if (n_lanes < 1 || !lane_devices || lane_devices[0] != d->device) { pg_set_error("graph lanes: lane 0 is the lead device"); return PG_EINVAL; }
    if (d->lanes.size() != 1 || d->reads_ready) { pg_set_error("graph lanes: already set"); return PG_ESTATE; }
    for (int l = 1; l < n_lanes; l++) {
        P2Lane ln;
        ln.device = lane_devices[l];
        P2_HIP(hipSetDevice(ln.device));
        P2_HIP(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        d->lanes.push_back(std::move(ln));
    }
    for (int l = 0; l < n_lanes; l++) {
        for (int s = 0; s < d->P; s++) { const int rc = p2_peer(lane_devices[l], d->set_dev[s]); if (rc) return rc; }
        int rc = p2_peer(d->device, lane_devices[l]);
        if (!rc) rc = p2_peer(lane_devices[l], d->device);
        if (rc) return rc;
    }
    for (int s = 0; s < d->P; s++) d->set_lane[s] = s % n_lanes;
    // a lane on another GPU than the lead reads the set geometry and the CRC table from copies of its own
    for (int l = 0; l < n_lanes; l++) {
        P2Lane& ln = d->lanes[l];
        P2_HIP(hipSetDevice(ln.device));
        P2_HIP(pg::arena_malloc((void**)&ln.d_wcnt, 4 * sizeof(unsigned long long)));
        if (ln.device == d->device) continue;
        const size_t gb = (size_t)SV_GEO * d->P * sizeof(uint64_t);
        P2_HIP(pg::arena_malloc((void**)&ln.d_geo3, gb)); ln.own_geo = true;
        P2_HIP(pg::arena_malloc((void**)&ln.d_crc, 256 * sizeof(uint32_t)));
        P2_HIP(hipMemcpyPeerAsync(ln.d_geo3, ln.device, d->d_geo3, d->device, gb, ln.stream));
        P2_HIP(hipMemcpyPeerAsync(ln.d_crc, ln.device, d->d_crc, d->device, 256 * sizeof(uint32_t), ln.stream));
        P2_HIP(hipStreamSynchronize(ln.stream));
    }
    P2_HIP(hipSetDevice(d->device));
    return PG_OK;
}
// the graph's parameters as lane l reads them (the set geometry from its own copy), and an equal share of n work items for every lane
static P2Params p2_lane_params(const P2Device* d, size_t l) {
    P2Params p = d->prm;
    if (l < d->lanes.size() && d->lanes[l].own_geo) p.geo3 = d->lanes[l].d_geo3;
    return p;
}
static void p2_share(const P2Device* d, size_t l, uint64_t n, uint64_t& first, uint64_t& count) {
    const uint64_t N = d->lanes.size();
    first = n * l / N;
    count = n * (l + 1) / N - first;
}
static int p2_sync_lanes(P2Device* d) {
    for (P2Lane& ln : d->lanes) { P2_HIP(hipSetDevice(ln.device)); P2_HIP(hipStreamSynchronize(ln.stream)); }
    P2_HIP(hipSetDevice(d->device));
    return PG_OK;
}

// upload: set s goes to set_device[s] (null: everything to `device`); one allocation per device
static int p2_open_impl(P2Device* d, const P2Sets& sets, const int* set_device) {
    const int NW1 = d->nw + 1;
    d->set_sizes.assign(sets.size, sets.size + d->P);
    d->set_dev.assign(d->P, d->device);
    d->set_ptr.assign(d->P, nullptr);
    if (set_device) for (int s = 0; s < d->P; s++) d->set_dev[s] = set_device[s];
    std::vector<int> devs;
    for (int s = 0; s < d->P; s++) if (std::find(devs.begin(), devs.end(), d->set_dev[s]) == devs.end()) devs.push_back(d->set_dev[s]);
    std::vector<hipStream_t> streams;
    int rc = PG_OK;
    for (int dev : devs) {
        uint64_t total = 0;
        for (int s = 0; s < d->P; s++) if (d->set_dev[s] == dev) total += sets.size[s];
        uint64_t* base = nullptr;
        hipStream_t st = nullptr;
        if (hipSetDevice(dev) != hipSuccess || pg::arena_malloc((void**)&base, std::max<uint64_t>(total, 1) * NW1 * sizeof(uint64_t)) != hipSuccess ||
            hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
            pg_set_error("out of device memory for the k-mer sets (" + std::to_string(total * NW1 * 8 >> 20) + " MiB on device " + std::to_string(dev) + ")");
            if (base) (void)pg::arena_free(base);
            rc = PG_ENOMEM;
            break;
        }
        d->owned.emplace_back(dev, (void*)base);
        streams.push_back(st);
        uint64_t at = 0;
        for (int s = 0; s < d->P && rc == PG_OK; s++) {
            if (d->set_dev[s] != dev) continue;
            d->set_ptr[s] = base + at * NW1;
            if (sets.size[s] && hipMemcpyAsync(d->set_ptr[s], sets.nodes[s], sets.size[s] * NW1 * sizeof(uint64_t), hipMemcpyHostToDevice, st) != hipSuccess) { pg_set_error("upload of a k-mer set failed"); rc = PG_ENODEV; }
            at += sets.size[s];
        }
    }
    for (size_t i = 0; i < streams.size(); i++) {                   // the devices' uploads ran side by side
        (void)hipSetDevice(devs[i]);
        if (hipStreamSynchronize(streams[i]) != hipSuccess && rc == PG_OK) { pg_set_error("upload of the k-mer sets failed"); rc = PG_ENODEV; }
        (void)hipStreamDestroy(streams[i]);
    }
    if (rc) return rc;
    return p2_finish_open(d);
}

P2Device* p2_open(int device, int K, int nw, int n_sets, const P2Sets& sets, int max_nk, const int* set_device) {
    if (n_sets < 1 || n_sets > P2_MAX_SETS || (nw != 2 && nw != 4)) { pg_set_error("pass 2: bad arguments"); return nullptr; }
    P2Device* d = new P2Device();
    d->device = device; d->K = K; d->nw = nw; d->P = n_sets; d->max_nk = std::max(max_nk, 1);
    if (p2_open_impl(d, sets, set_device) != PG_OK) { p2_free(d); return nullptr; }
    return d;
}

// nodes of an empty image: first key word all-ones, the rest zero
__global__ void p2_empty_image(uint64_t* nodes, int nw1, uint64_t n_slots) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots * nw1; i += (uint64_t)gridDim.x * blockDim.x)
        nodes[i] = (i % nw1) ? 0ULL : P2_EMPTY;
}

// Device memory a caller is done with and offers for reuse (pg_device_scratch_offer): a hipMalloc of tens of gigabytes right
// behind a hipFree of as much takes seconds on this stack, so pass 1's record pool becomes the k-mer set image instead of being
// freed and allocated anew.  One block per device; whoever takes it AND SUCCEEDS owns it.  A taker that fails or finds itself
// unsuited hands the block back (the caller may still have live data in the same allocation -- call_pregraph keeps the
// regrouped records in the pool's tail, and the host replay that follows an unsuited layout reads them), so a taken block is
// remembered until its new owner releases it.
namespace {
struct Offered { int device; void* ptr; uint64_t bytes; };
std::vector<Offered> g_offered, g_taken;
std::mutex g_offered_mu;
void* take_offered(int device, uint64_t need) {
    std::lock_guard<std::mutex> lk(g_offered_mu);
    for (size_t i = 0; i < g_offered.size(); i++)
        if (g_offered[i].device == device && g_offered[i].bytes >= need + 256) {
            void* p = g_offered[i].ptr;
            g_taken.push_back(g_offered[i]);
            g_offered.erase(g_offered.begin() + i);
            return p;
        }
    return nullptr;
}
// a taken block goes back on offer (true), or the pointer was never one (false)
bool hand_back_offered(void* ptr) {
    std::lock_guard<std::mutex> lk(g_offered_mu);
    for (size_t i = 0; i < g_taken.size(); i++)
        if (g_taken[i].ptr == ptr) { g_offered.push_back(g_taken[i]); g_taken.erase(g_taken.begin() + i); return true; }
    return false;
}
// the new owner frees the block itself: nothing to remember any more
void forget_taken(void* ptr) {
    std::lock_guard<std::mutex> lk(g_offered_mu);
    for (size_t i = 0; i < g_taken.size(); i++) if (g_taken[i].ptr == ptr) { g_taken.erase(g_taken.begin() + i); return; }
}
}  // namespace
extern "C" int pg_device_scratch_offer(int device, void* d_ptr, uint64_t bytes) {
    if (!d_ptr) return PG_EINVAL;
    std::lock_guard<std::mutex> lk(g_offered_mu);
    for (auto& o : g_offered) if (o.device == device) return PG_ESTATE;       // one block per device
    g_offered.push_back(Offered{device, d_ptr, bytes});
    return PG_OK;
}
extern "C" void* pg_device_scratch_withdraw(int device) {
    std::lock_guard<std::mutex> lk(g_offered_mu);
    for (size_t i = 0; i < g_offered.size(); i++)
        if (g_offered[i].device == device) { void* p = g_offered[i].ptr; g_offered.erase(g_offered.begin() + i); return p; }
    return nullptr;
}

// SURVEY.md App. C "K6", one rank's share: the sets this rank owns (n_own of them, set_size slots each, back to back in a
// fresh allocation on `device`), laid out from the rank's records as they lie there sorted by (set, first ordinal) -- no host
// replay, no upload (dev_graph.hpp: layout_static).  PG_OK, 1 = unsuited (nothing allocated), or PG_E*.
// What the two layouts below share: the image of a rank's sets -- the block pass 1 offered, if it is large enough, or an allocation -- aligned
// and emptied on a stream of its own, with the times of the verbose lines.  A layout that succeeds publish()es the image; one that leaves
// any other way rolls back: the offered block goes back on offer, only what was allocated here is freed here.
struct LayoutImage {
    const int device, NW1;
    uint64_t total = 0;
    uint64_t* nodes = nullptr;
    void* block = nullptr;
    hipStream_t st = nullptr;
    bool published = false;
    double t0, t1 = 0;
    static double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
    LayoutImage(int device_, int nw) : device(device_), NW1(nw + 1), t0(now()) {}
    LayoutImage(const LayoutImage&) = delete; LayoutImage& operator=(const LayoutImage&) = delete;
    int open(uint64_t total_slots) {
        total = total_slots;
        P2_HIP(hipSetDevice(device));
        P2_HIP(hipStreamCreate(&st));
        block = take_offered(device, total * NW1 * sizeof(uint64_t));        // memory pass 1 is done with, if it was offered and is large enough
        if (block) nodes = (uint64_t*)(((uintptr_t)block + 255) & ~(uintptr_t)255);
        else if (pg::arena_malloc((void**)&nodes, total * NW1 * sizeof(uint64_t)) != hipSuccess) {
            nodes = nullptr;
            pg_set_error("layout: out of device memory for the k-mer sets (" + std::to_string(total * NW1 * 8 >> 20) + " MiB on device " + std::to_string(device) + ")");
            return PG_ENOMEM;
        }
        t1 = now();
        hipLaunchKernelGGL(p2_empty_image, dim3(8192), dim3(256), 0, st, nodes, NW1, total);
        return PG_OK;
    }
    const char* source() const { return block ? "memory taken over from pass 1" : "allocation"; }
    void publish(uint64_t** d_nodes_out, void** alloc_out) { *d_nodes_out = nodes; if (alloc_out) *alloc_out = block ? block : (void*)nodes; published = true; }
    ~LayoutImage() {
        if (st) (void)hipStreamDestroy(st);
        if (!published) { if (block) hand_back_offered(block); else if (nodes) (void)pg::arena_free(nodes); }
    }
};

int p2_layout_rank(int device, int nw, int n_own, const uint64_t* d_records, const uint64_t* own_counts, uint64_t set_size, uint64_t** d_nodes_out,
                   void** alloc_out) {
    *d_nodes_out = nullptr;
    if (alloc_out) *alloc_out = nullptr;
    if (n_own < 1) return PG_OK;
    LayoutImage im(device, nw);
    for (int s = 0; s < n_own; s++) if (own_counts[s] >= set_size || own_counts[s] >= 0xFFFFFFFFULL) return K6_UNSUITED;
    int rc = im.open((uint64_t)n_own * set_size);
    if (rc) return rc;
    std::string why;
    {
        HipBackend be(device, im.st);
        rc = nw == 2 ? layout_static<HipBackend, 2>(be, d_records, own_counts, n_own, set_size, im.nodes)
                     : layout_static<HipBackend, 4>(be, d_records, own_counts, n_own, set_size, im.nodes);
        why = be.error_text;
    }
    if (rc == PG_OK && hipStreamSynchronize(im.st) != hipSuccess) { rc = PG_ENODEV; why = "kernel failure"; }
    if (rc) {
        if (rc < 0) pg_set_error("layout: " + (why.empty() ? std::string("failed") : why));
        return rc;
    }
    if (pg::env_user("PG_HOST_VERBOSE"))
        fprintf(stderr, "K6 on device %d: %d set(s) of %llu slots, %s %.2fs, layout %.2fs\n", device, n_own, (unsigned long long)set_size, im.source(), im.t1 - im.t0, im.now() - im.t1);
    im.publish(d_nodes_out, alloc_out);
    return PG_OK;
}

// The same for GROWABLE sets (-a 0): every set ends at the size the reference's growth schedule gives it for its key count
// (sizes_out), and every key in the slot the whole history of in-place rehashes leaves it in (dev_rehash.hpp: layout_growable).
// The sets lie back to back in one allocation, set i at sizes_out[0] + ... + sizes_out[i - 1] slots.
int p2_layout_rank_growable(int device, int nw, int n_own, const uint64_t* d_records, const uint64_t* own_counts, const unsigned char* own_trailing,
                            uint64_t init_size, uint64_t* sizes_out, uint64_t** d_nodes_out, void** alloc_out, uint64_t* rounds_out) {
    *d_nodes_out = nullptr;
    if (alloc_out) *alloc_out = nullptr;
    if (n_own < 1) return PG_OK;
    const bool verbose = pg::env_user("PG_HOST_VERBOSE") != nullptr;
    LayoutImage im(device, nw);
    std::vector<uint64_t> first_slot((size_t)n_own + 1, 0);
    for (int s = 0; s < n_own; s++) {
        if (own_counts[s] >= 0xFFFFFFF0ULL) return K6_UNSUITED;
        sizes_out[s] = grow_schedule(own_counts[s], own_trailing && own_trailing[s], init_size).back().size;
        first_slot[s + 1] = first_slot[s] + sizes_out[s];
    }
    int rc = im.open(first_slot[n_own]);
    if (rc) return rc;
    uint64_t* const nodes = im.nodes;
    std::string why;
    std::vector<uint64_t> rounds((size_t)n_own, 0);
    // A round of a set's fixed point is a handful of small dependent launches and two reads of a counter: latency, not work.
    // Several sets side by side, each on its own stream, as many as the free memory holds scratch for (SOAPDENOVO2_AMD_LAYOUT_LANES)
    int lanes = 1;
    {
        uint64_t n_max = 0, owner_max = 0;
        for (int s = 0; s < n_own; s++) {
            n_max = std::max(n_max, own_counts[s]);
            owner_max = std::max(owner_max, grow_owner_slots(grow_schedule(own_counts[s], own_trailing && own_trailing[s], init_size)));
        }
        size_t free_b = 0, total_b = 0;
        const uint64_t one = growable_scratch_bytes(n_max, owner_max);
        // (two: 1.15 s -> 1.0 s at 60 M reads; eight bought another 0.05 s for four times the scratch -- and a fresh process pays for its
        //  allocations by the gigabyte)
        if (pg::arena_mem_info(&free_b, &total_b) == hipSuccess) lanes = (int)std::min<uint64_t>(2, (uint64_t)((double)free_b * 0.85) / std::max<uint64_t>(one, 1));
        if (const char* v = pg::env_measure("SOAPDENOVO2_AMD_LAYOUT_LANES")) lanes = atoi(v);
        lanes = std::max(1, std::min(lanes, n_own));
    }
    if (hipStreamSynchronize(im.st) != hipSuccess) { rc = PG_ENODEV; why = "kernel failure"; }      // the image is empty before anybody writes to it
    if (rc == PG_OK) {
        std::vector<int> rcs((size_t)lanes, PG_OK);
        std::vector<std::string> whys((size_t)lanes);
        auto lane = [&](int t) {
            hipStream_t ls = nullptr;
            if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ls, hipStreamNonBlocking) != hipSuccess) { rcs[t] = PG_ENODEV; whys[t] = "no stream"; return; }
            {
                HipBackend be(device, ls);
                rcs[t] = nw == 2 ? layout_growable_sets<HipBackend, 2>(be, d_records, own_counts, own_trailing, n_own, init_size, first_slot.data(), nodes, nullptr, rounds.data(), t, lanes)
                                 : layout_growable_sets<HipBackend, 4>(be, d_records, own_counts, own_trailing, n_own, init_size, first_slot.data(), nodes, nullptr, rounds.data(), t, lanes);
                whys[t] = be.error_text;
                if (verbose) fprintf(stderr, "growable layout, lane %d: %llu read-backs of a counter, %.2fs waiting for them\n", t, be.n_readback, be.t_readback);
            }
            if (rcs[t] == PG_OK && hipStreamSynchronize(ls) != hipSuccess) { rcs[t] = PG_ENODEV; whys[t] = "kernel failure"; }
            (void)hipStreamDestroy(ls);
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < lanes; t++) pool.emplace_back(lane, t);
        lane(0);
        for (auto& th : pool) th.join();
        for (int t = 0; t < lanes; t++) if (rcs[t] && !rc) { rc = rcs[t]; why = whys[t]; }
    }
    if (rc) {
        if (rc == PG_ENOMEM) {                                          // no room for the scratch beside the image: the sequential host replay needs none
            fprintf(stderr, "growable sets on device %d: out of device memory for the layout's scratch; replaying on the host\n", device);
            return K6_UNSUITED;
        }
        pg_set_error("layout: " + (why.empty() ? std::string("failed") : why));
        return rc < 0 ? rc : PG_ENODEV;
    }
    if (verbose) {
        uint64_t r_all = 0;
        for (uint64_t r : rounds) r_all += r;
        fprintf(stderr, "growable sets on device %d: %d set(s), %llu slots in all, %s %.2fs, layout %.2fs (%llu rounds over all sizes, %d set(s) side by side)\n", device, n_own,
                (unsigned long long)im.total, im.source(), im.t1 - im.t0, im.now() - im.t1, (unsigned long long)r_all, lanes);
    }
    if (rounds_out) for (int s = 0; s < n_own; s++) rounds_out[s] = rounds[s];
    im.publish(d_nodes_out, alloc_out);
    return PG_OK;
}

// the graph over sets that are already in device memory: set s = set_size[s] slots at set_ptr[s] on set_device[s]; the
// allocations in `owned` (device, pointer) change hands
P2Device* p2_adopt(int lead_device, int K, int nw, int n_sets, const uint64_t* set_size, const int* set_device, uint64_t* const* set_ptr,
                   const std::vector<std::pair<int, void*>>& owned, int max_nk) {
    P2Device* d = new P2Device();
    d->device = lead_device; d->K = K; d->nw = nw; d->P = n_sets; d->max_nk = std::max(max_nk, 1);
    d->set_sizes.assign(set_size, set_size + n_sets);
    d->set_dev.assign(set_device, set_device + n_sets);
    d->set_ptr.assign(set_ptr, set_ptr + n_sets);
    d->owned = owned;
    if (n_sets < 1 || n_sets > P2_MAX_SETS || (nw != 2 && nw != 4)) { pg_set_error("graph: bad arguments"); p2_free(d); return nullptr; }
    if (p2_finish_open(d) != PG_OK) { p2_free(d); return nullptr; }
    return d;
}

P2Device* p2_open_layout(int device, int K, int nw, int n_sets, const uint64_t* d_records, const uint64_t* per_set_count, uint64_t set_size,
                         int max_nk, bool* unsuited) {
    *unsuited = false;
    uint64_t* nodes = nullptr;
    void* alloc = nullptr;
    const int rc = p2_layout_rank(device, nw, n_sets, d_records, per_set_count, set_size, &nodes, &alloc);
    if (rc == K6_UNSUITED) { *unsuited = true; return nullptr; }
    if (rc) return nullptr;
    std::vector<uint64_t> sizes(n_sets, set_size);
    std::vector<int> devs(n_sets, device);
    std::vector<uint64_t*> ptrs(n_sets);
    for (int s = 0; s < n_sets; s++) ptrs[s] = nodes + (uint64_t)s * set_size * (nw + 1);
    return p2_adopt(device, K, nw, n_sets, sizes.data(), devs.data(), ptrs.data(), {{device, alloc}}, max_nk);
}

// one set's slots, as they are on the device now, into host memory (size * (nw + 1) words)
int p2_download_set(P2Device* d, int set, void* dst) {
    P2_HIP(hipSetDevice(d->set_dev[set]));
    const size_t bytes = (size_t)d->set_sizes[set] * (d->nw + 1) * sizeof(uint64_t);
    hipStream_t st = nullptr;
    P2_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const bool reg = hipHostRegister(dst, bytes, hipHostRegisterDefault) == hipSuccess;       // plain DMA instead of staged copies
    hipError_t e = hipMemcpyAsync(dst, d->set_ptr[set], bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (reg) (void)hipHostUnregister(dst);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) { pg_set_error(std::string("download of a k-mer set: ") + hipGetErrorString(e)); return PG_ENODEV; }
    return PG_OK;
}

// a stretch of device-resident records into host memory; called from the layout replay's worker threads: each keeps its own
// stream and has its chunk buffer page-locked once, so the copies are plain DMA that run side by side (pageable copies on
// the null stream queue up behind each other).  n_words = 0: the calling thread will not ask again.
int p2_fetch_words(int device, const uint64_t* d_src, uint64_t n_words, uint64_t* dst) {
    struct PerThread {
        std::vector<std::pair<int, hipStream_t>> st;      // one stream per device this thread has pulled from (a worker's sets may lie on several)
        void* reg = nullptr; size_t bytes = 0;
        ~PerThread() { if (reg) (void)hipHostUnregister(reg); for (auto& q : st) { (void)hipSetDevice(q.first); (void)hipStreamDestroy(q.second); } }
    };
    static thread_local PerThread t;
    if (hipSetDevice(device) != hipSuccess) return PG_ENODEV;
    if (n_words == 0) {                                   // let go of the buffer before its owner unmaps it
        if (t.reg) { (void)hipHostUnregister(t.reg); t.reg = nullptr; t.bytes = 0; }
        return PG_OK;
    }
    const size_t bytes = (size_t)n_words * sizeof(uint64_t);
    hipStream_t st = nullptr;
    for (auto& q : t.st) if (q.first == device) st = q.second;
    if (!st) {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return PG_ENODEV;
        t.st.emplace_back(device, st);
    }
    if (t.reg != (void*)dst || t.bytes < bytes) {
        if (t.reg) { (void)hipHostUnregister(t.reg); t.reg = nullptr; }
        if (hipHostRegister(dst, bytes, hipHostRegisterPortable) == hipSuccess) { t.reg = dst; t.bytes = bytes; }
    }
    if (hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return PG_ENODEV;
    return hipStreamSynchronize(st) == hipSuccess ? PG_OK : PG_ENODEV;
}

void pg_device_free_on(int device, void* d_ptr) { if (d_ptr) { (void)hipSetDevice(device); (void)pg::arena_free(d_ptr); } }
// a layout's allocation that is not going to be used after all: back on offer if it was taken over from a caller, freed otherwise
void pg_device_release_layout(int device, void* d_ptr) { if (d_ptr && !hand_back_offered(d_ptr)) pg_device_free_on(device, d_ptr); }

// The (K+1)-mer table of the graph (raw members: a lane's are the lead's or its own, own_patch): the old one goes; a new one, complete, changes hands
static void p2_drop_patch(P2Device* d) {
    pg::arena_free(d->d_patch_keys); pg::arena_free(d->d_patch_val);
    d->d_patch_keys = nullptr; d->d_patch_val = nullptr;
}
static void p2_take_patch(P2Device* d, DevArr<uint64_t>& keys, DevArr<uint32_t>& val, uint64_t patch_cap) {
    d->d_patch_keys = keys.release(); d->d_patch_val = val.release();
    d->prm.patch_keys = d->d_patch_keys; d->prm.patch_val = d->d_patch_val; d->prm.patch_mask = patch_cap - 1;
}
// KmerSetsPatch as the host built it
int p2_set_patch(P2Device* d, const uint64_t* patch_keys, const uint32_t* patch_val, uint64_t patch_cap) {
    if ((patch_cap & (patch_cap - 1)) || !patch_cap) { pg_set_error("pass 2: patch table size must be a power of two"); return PG_EINVAL; }
    P2_HIP(hipSetDevice(d->device));
    DevArr<uint64_t> keys; DevArr<uint32_t> val;
    p2_drop_patch(d);
    P2_HIP(keys.alloc(patch_cap * d->nw)); P2_HIP(val.alloc(patch_cap * 2));
    P2_HIP(hipMemcpy(keys.p, patch_keys, patch_cap * d->nw * sizeof(uint64_t), hipMemcpyHostToDevice));
    P2_HIP(hipMemcpy(val.p, patch_val, patch_cap * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
    p2_take_patch(d, keys, val, patch_cap);
    return PG_OK;
}


// the pre-arc table and, with -R, the marker counts: one of each per lane; lanes on another device than the lead's get their own
// copy of the set geometry and of the (K+1)-mer table (a few MB: every probe of them would otherwise cross xGMI)
int p2_begin_reads(P2Device* d, uint32_t num_ed, bool reps) {
    P2_HIP(hipSetDevice(d->device));
    if (!d->d_patch_val) { pg_set_error("pass 2: no (K+1)-mer table yet"); return PG_ESTATE; }
    d->num_ed = num_ed; d->reps = reps;
    // several lanes: the lookups are routed to the sets' owners (SOAPDENOVO2_AMD_P2_ROUTE=0: every lane probes the peer-mapped sets itself, the A/B form)
    d->route = d->lanes.size() > 1 && (int)d->lanes.size() <= P2R_MAX_LANES;
    if (const char* e = pg::env_user("SOAPDENOVO2_AMD_P2_ROUTE")) d->route = d->route && atoi(e) != 0;
    // every edge has a handful of successors: eight slots an edge id keep the load low; the kernel counts overflows
    uint64_t arc_cap;
    {
        size_t free_b = 0, total_b = 0;
        P2_HIP(hipMemGetInfo(&free_b, &total_b));
        arc_cap = pg::cmd_prearc_entries((uint64_t)d->num_ed, (uint64_t)total_b);      // (cmd_plan.hpp: the rule pg_host_plan_memory plans by)
    }
    // PG_P2_ARC_ROOM=n (test hook): every lane's table has n entries -- the loads of 50 - 100 % the rule above reaches when device memory is short
    if (const char* v = pg::env_test("PG_P2_ARC_ROOM")) {
        const long long room = atoll(v);
        if (room < 1 || (room & (room - 1))) { pg_set_error("pass 2: pre-arc table size must be a power of two"); return PG_EINVAL; }
        arc_cap = (uint64_t)room;
        if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "pass 2: pre-arc tables of %llu entries a lane (PG_P2_ARC_ROOM)\n", (unsigned long long)arc_cap);
    }
    const uint64_t patch_cap = d->prm.patch_mask + 1;
    for (size_t l = 0; l < d->lanes.size(); l++) {
        P2Lane& ln = d->lanes[l];
        P2_HIP(hipSetDevice(ln.device));
        ln.prm = d->prm;
        if (ln.device != d->device) {
            const size_t gb = (size_t)SV_GEO * d->P * sizeof(uint64_t), kb = patch_cap * d->nw * sizeof(uint64_t), vb = patch_cap * 2 * sizeof(uint32_t);
            if (!ln.own_geo) { P2_HIP(pg::arena_malloc((void**)&ln.d_geo3, gb)); ln.own_geo = true; }
            P2_HIP(pg::arena_malloc((void**)&ln.d_patch_keys, kb)); ln.own_patch = true;
            P2_HIP(pg::arena_malloc((void**)&ln.d_patch_val, vb));
            P2_HIP(hipMemcpyPeerAsync(ln.d_geo3, ln.device, d->d_geo3, d->device, gb, ln.stream));
            P2_HIP(hipMemcpyPeerAsync(ln.d_patch_keys, ln.device, d->d_patch_keys, d->device, kb, ln.stream));
            P2_HIP(hipMemcpyPeerAsync(ln.d_patch_val, ln.device, d->d_patch_val, d->device, vb, ln.stream));
            ln.prm.geo3 = ln.d_geo3; ln.prm.patch_keys = ln.d_patch_keys; ln.prm.patch_val = ln.d_patch_val;
        }
        if (l == 0) ln.d_counters = d->d_counters;
        else P2_HIP(pg::arena_malloc((void**)&ln.d_counters, 8 * sizeof(unsigned long long)));
        P2_HIP(pg::arena_malloc((void**)&ln.d_arc, arc_cap * ARC_WORDS * sizeof(unsigned long long)));
        hipLaunchKernelGGL(p2_arc_init, dim3(2048), dim3(256), 0, ln.stream, ln.d_arc, arc_cap);
        P2_HIP(hipMemsetAsync(ln.d_counters, 0, 8 * sizeof(unsigned long long), ln.stream));
        if (d->reps) {
            P2_HIP(pg::arena_malloc((void**)&ln.d_marker, ((size_t)d->num_ed + 1) * sizeof(unsigned int)));
            P2_HIP(hipMemsetAsync(ln.d_marker, 0, ((size_t)d->num_ed + 1) * sizeof(unsigned int), ln.stream));
        }
        P2_HIP(hipEventCreateWithFlags(&ln.copied, hipEventDisableTiming));
        if (d->route) {
            std::vector<uint8_t> own(256, 0);
            for (int s2 = 0; s2 < d->P; s2++) own[s2] = (uint8_t)d->set_lane[s2];
            P2_HIP(pg::arena_malloc((void**)&ln.d_owner_of_set, 256));
            P2_HIP(hipMemcpy(ln.d_owner_of_set, own.data(), 256, hipMemcpyHostToDevice));      // (synchronous: `own` is pageable and leaves scope before the stream is waited for)
            P2_HIP(hipHostMalloc((void**)&ln.h_starts, (P2R_MAX_LANES + 1) * sizeof(uint32_t), hipHostMallocPortable));
        }
        P2_HIP(hipStreamSynchronize(ln.stream));
        P2Params& p = ln.prm;
        p.counters = ln.d_counters;
        p.arc = ln.d_arc; p.arc_mask = arc_cap - 1;
        p.marker = ln.d_marker; p.id_end = d->num_ed + 1;
        ln.tables = true;
    }
    P2_HIP(hipSetDevice(d->device));
    d->prm = d->lanes[0].prm;
    // (the opt-in lookup table takes what is free AFTER the tables pass 2 cannot do without)
    { const int rc = p2_make_look(d); if (rc) return rc; d->lanes[0].prm.look = d->prm.look; d->lanes[0].prm.look_buckets = d->prm.look_buckets; }
    d->reads_ready = true;
    return PG_OK;
}

P2Device* p2_create(int device, int K, int nw, int n_sets, const P2Sets& sets, const uint64_t* patch_keys, const uint32_t* patch_val,
                    uint64_t patch_cap, uint32_t num_ed, int max_nk, bool reps) {
    P2Device* d = p2_open(device, K, nw, n_sets, sets, max_nk);
    if (!d) return nullptr;
    if (p2_set_patch(d, patch_keys, patch_val, patch_cap) != PG_OK || p2_begin_reads(d, num_ed, reps) != PG_OK) { p2_free(d); return nullptr; }
    return d;
}

// ---- tips ---------------------------------------------------------------------------------------------------------------
int p2_tip_walks(P2Device* d, int cut_len, bool thin, std::vector<P2TipWalk>& out) {
    hipStream_t st = d->stream;
    DevArr<unsigned long long> cnt, key, key2;             // cnt: walks, errors
    DevListing<P2TipWalk> walks;
    DevArr<uint32_t> idx, order; DevArr<P2TipWalk> sorted; DevArr<unsigned char> tmp;
    out.clear();
    if (hipSetDevice(d->device) != hipSuccess) { pg_set_error("tips: hipSetDevice failed"); return PG_ENODEV; }
    for (int si = 0; si < d->P; si++) if (d->set_sizes[si] / 256 >= 0x7FFFFFFFULL) { pg_set_error("tips: too many slots for one launch"); return PG_EINVAL; }
    EB_HIP(cnt.alloc(2));
    auto list = [&](P2TipWalk* d_w, unsigned long long cap, hipStream_t s) {
        hipError_t e = hipMemsetAsync(cnt.p, 0, 2 * sizeof(unsigned long long), s);
        for (int si = 0; si < d->P && e == hipSuccess; si++) {
            if (!d->set_sizes[si]) continue;
            const dim3 grid((unsigned)((d->set_sizes[si] + 255) / 256));
            P2_LAUNCH_NW(d->nw, (tip_walk_kernel<NW>), grid, dim3(256), 0, s, d->prm, d->set_ptr[si], d->set_first[si], d->set_sizes[si], cut_len, thin ? 1 : 0, d_w, cap, cnt.p, cnt.p + 1);
            e = hipGetLastError();
        }
        return e;
    };
    EB_HIP(walks.begin(d->n_slots / 8 + 4096, cnt.p, 2, 0, st, list));      // dead ends are a small share of the slots; listed again when short
    EB_HIP(walks.end("tip walks", 0, st, list));
    if (walks.cnt[1]) { pg_set_error("Kmer is not found while clipping a tip."); return PG_EINVAL; }
    if (walks.short_of_room()) { pg_set_error("tips: walk buffer too small"); return PG_ENOMEM; }
    if (walks.n() >= 0x7FFFFFFFULL) { pg_set_error("tips: more than 2^31 - 1 dead ends"); return PG_EINVAL; }
    if (const uint64_t n = walks.n()) {
        EB_HIP(key.alloc(n)); EB_HIP(key2.alloc(n));
        EB_HIP(idx.alloc(n)); EB_HIP(order.alloc(n)); EB_HIP(sorted.alloc(n));
        hipLaunchKernelGGL(tip_keys, dim3(1024), dim3(256), 0, st, walks.list.p, n, key.p, idx.p);
        EB_HIP(dev_sort_pairs(tmp, key.p, key2.p, idx.p, order.p, (size_t)n, 64u, st));
        hipLaunchKernelGGL(tip_gather, dim3(1024), dim3(256), 0, st, walks.list.p, order.p, n, sorted.p);
        out.resize(n);
        EB_HIP(hipMemcpyAsync(out.data(), sorted.p, n * sizeof(P2TipWalk), hipMemcpyDeviceToHost, st));
        EB_HIP(hipStreamSynchronize(st));
    }
    return PG_OK;
}

int p2_mirror_nodes(P2Device* d, const uint64_t* slots, const uint64_t* ab, uint64_t n) {
    if (!n) return PG_OK;
    P2_HIP(hipSetDevice(d->device));
    DevArr<uint64_t> d_s, d_ab;
    P2_HIP(d_s.alloc(n)); P2_HIP(d_ab.alloc(n));
    P2_HIP(hipMemcpyAsync(d_s.p, slots, n * sizeof(uint64_t), hipMemcpyHostToDevice, d->stream));
    P2_HIP(hipMemcpyAsync(d_ab.p, ab, n * sizeof(uint64_t), hipMemcpyHostToDevice, d->stream));
    P2_LAUNCH_NW(d->nw, (tip_mirror<NW>), dim3(1024), dim3(256), 0, d->stream, d->prm, d_s.p, d_ab.p, n);
    P2_HIP(hipStreamSynchronize(d->stream));
    return PG_OK;
}

int p2_remark_linear(P2Device* d) {
    P2_HIP(hipSetDevice(d->device));
    P2_HIP(hipStreamSynchronize(d->stream));
    for (int si = 0; si < d->P; si++) {
        if (!d->set_sizes[si]) continue;
        P2Lane& ln = d->lanes[d->set_lane[si]];                      // every set on the lane that owns it
        P2_HIP(hipSetDevice(ln.device));
        hipLaunchKernelGGL(tip_remark, dim3(4096), dim3(256), 0, ln.stream, d->set_ptr[si], d->nw + 1, d->set_sizes[si]);
        ln.scans++;
    }
    for (auto& ln : d->lanes) { P2_HIP(hipSetDevice(ln.device)); P2_HIP(hipStreamSynchronize(ln.stream)); }
    P2_HIP(hipSetDevice(d->device));
    return PG_OK;
}

// ---- the sets as the backend-generic stages see them (dev_tips.hpp) ---------------------------------------------------------
static int p2_sets_view(P2Device* d, SetsView& view, SetsGeo& geo) {
    P2_HIP(hipSetDevice(d->device));
    geo.P = d->P; geo.first = d->set_first; geo.size = d->set_sizes; geo.base = d->set_ptr;
    view = SetsView{d->d_geo3, d->d_crc, (uint32_t)d->P, set_bias((uint32_t)d->P), d->K};
    return PG_OK;
}

// removeSingleTips + removeMinorTips decided on the device (dev_tips.hpp)
int p2_clip_tips(P2Device* d, bool cut_single, P2TipTotals& out) {
    SetsView view;
    SetsGeo geo;
    int rc = p2_sets_view(d, view, geo);
    if (rc) return rc;
    HipBackend be(d->device, d->stream);
    if (d->lanes.size() > 1) {                                       // the scans over a set's slots run on the lane that owns the set
        std::vector<HipBackend::Place> pl;
        std::vector<HipBackend::PlaceView> pv;
        for (auto& ln : d->lanes) {
            pl.push_back(HipBackend::Place{ln.device, ln.stream});
            pv.push_back(ln.own_geo && ln.d_crc ? HipBackend::PlaceView{ln.d_geo3, ln.d_crc} : HipBackend::PlaceView{nullptr, nullptr});
        }
        be.use_places(pl, d->set_lane, pv);
        be.timing = pg::env_user("PG_HOST_VERBOSE") != nullptr;
    }
    TipTotals tot;
    rc = d->nw == 2 ? clip_tips<HipBackend, 2>(be, view, geo, cut_single, tot) : clip_tips<HipBackend, 4>(be, view, geo, cut_single, tot);
    if (rc) { pg_set_error(be.error_text.empty() ? "tip clipping on the device failed" : be.error_text); return rc; }
    if (be.timing) {                                                 // what of the stage's device time the lead spent alone (its sorts and node steps are not dealt)
        be.sync(); be.sync_places();
        double lead_ms = 0;
        std::vector<double> at;
        be.lead_share(lead_ms, at);
        double dealt = 0;
        for (double x : at) dealt += x;
        fprintf(stderr, "tips, sharded: device time of the steps on the lead alone (sorts, node steps, lists) %.1f ms; of the steps dealt to the lanes (scans on a set's owner, walks in equal shares)", lead_ms);
        for (double x : at) fprintf(stderr, " %.1f", x);
        fprintf(stderr, " ms = %.1f ms in all: the lead-only share is %.0f %% of the stage's kernel time\n", dealt, lead_ms + dealt > 0 ? 100.0 * lead_ms / (lead_ms + dealt) : 0.0);
    }
    for (size_t l = 0; l < be.launches_at.size() && l < d->lanes.size(); l++) { d->lanes[l].scans += be.launches_at[l]; d->lanes[l].walks += be.walks_at[l]; }
    out.single = tot.single; out.minor = tot.minor; out.cycles = tot.minor_cycles; out.rounds = tot.rounds;
    out.per_cycle.assign(tot.per_cycle.begin(), tot.per_cycle.end());
    return PG_OK;
}

// the vertices (live non-linear nodes) in slot order, NW key words each (output_vertex, output_pregraph.c:50-86)
template <int NW>
__global__ __launch_bounds__(256) void vx_gather(P2Params p, const unsigned long long* slots, uint64_t n, uint64_t* out) {
    P2_PROLOGUE(p);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * NW; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = sv_node<NW>(sv, slots[i / NW])[i % NW];
}
// The vertices of every set, listed ON THE LANE THAT OWNS THE SET into a list and a counter of that lane (room for one slot in 32
// -- a vertex is a node that is not linear: one in a few hundred; a lane that runs short says how many and scans again), then
// gathered into one list on the lead (*d_list_out, *n_out; any order).  A list for every slot was a 17 GB allocation at 200 M reads.
static int p2_list_branch_nodes(P2Device* d, DevArr<unsigned long long>& list_out, unsigned long long* n_out) {
    *n_out = 0;
    const int NL = (int)d->lanes.size();
    P2BackOn back{d->device};
    std::vector<DevArr<unsigned long long>> l_cnt(NL);
    std::vector<DevListing<unsigned long long>> l_list(NL);
    std::vector<unsigned long long> l_slots(NL, 0);
    unsigned long long total = 0, at = 0;
    for (int s = 0; s < d->P; s++) l_slots[d->set_lane[s]] += d->set_sizes[s];
    if (hipSetDevice(d->device) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess) { pg_set_error("vertices: the lead's stream failed"); return PG_ENODEV; }
    auto scan_of = [&](int l) {                            // lane l's sets into a list of that lane
        return [&, l](unsigned long long* list, unsigned long long cap, hipStream_t st) {
            const hipError_t e = hipMemsetAsync(l_cnt[l].p, 0, sizeof(unsigned long long), st);
            if (e != hipSuccess) return e;
            for (int si = 0; si < d->P; si++)
                if (d->set_lane[si] == l && d->set_sizes[si]) {
                    hipLaunchKernelGGL(eb_list_branch, dim3(4096), dim3(256), 0, st, d->set_ptr[si], d->nw + 1, d->set_sizes[si], d->set_first[si], list, l_cnt[l].p, cap);
                    d->lanes[l].scans++;
                }
            return hipGetLastError();
        };
    };
    for (int l = 0; l < NL; l++) {
        if (!l_slots[l]) continue;
        EB_HIP(hipSetDevice(d->lanes[l].device));
        EB_HIP(l_cnt[l].alloc(1));
        const unsigned long long cap = std::min<unsigned long long>(std::max<unsigned long long>(l_slots[l] / 32, 1 << 20), l_slots[l]);
        EB_HIP(l_list[l].begin(cap, l_cnt[l].p, 1, 0, d->lanes[l].stream, scan_of(l)));
    }
    for (int l = 0; l < NL; l++) {
        if (!l_slots[l]) continue;
        EB_HIP(hipSetDevice(d->lanes[l].device));
        EB_HIP(l_list[l].end("vertices", 0, d->lanes[l].stream, scan_of(l)));
        if (l_list[l].short_of_room()) { pg_set_error("vertices: a lane's list is too small"); return PG_ENOMEM; }
        total += l_list[l].n();
    }
    EB_HIP(hipSetDevice(d->device));
    if (total) {
        EB_HIP(list_out.alloc(total));
        for (int l = 0; l < NL; l++) {
            if (!l_list[l].n()) continue;
            EB_HIP(hipMemcpyAsync(list_out.p + at, l_list[l].list.p, l_list[l].n() * sizeof(unsigned long long), hipMemcpyDefault, d->stream));
            at += l_list[l].n();
        }
        EB_HIP(hipStreamSynchronize(d->stream));
    }
    *n_out = total;
    return PG_OK;
}

int p2_list_vertices(P2Device* d, std::vector<uint64_t>& keys) {
    hipStream_t st = d->stream;
    DevArr<unsigned long long> list, sorted; DevArr<uint64_t> d_keys; DevArr<unsigned char> tmp;
    unsigned long long n = 0;
    int bits = 1;
    keys.clear();
    if (hipSetDevice(d->device) != hipSuccess) { pg_set_error("vertices: hipSetDevice failed"); return PG_ENODEV; }
    const int rc = p2_list_branch_nodes(d, list, &n);
    if (rc || !n) return rc;
    while (bits < 64 && (d->n_slots >> bits)) bits++;
    EB_HIP(sorted.alloc(n));
    EB_HIP(d_keys.alloc(n * d->nw));
    EB_HIP(dev_sort_keys(tmp, list.p, sorted.p, (size_t)n, (unsigned)bits, st));
    P2_LAUNCH_NW(d->nw, (vx_gather<NW>), dim3(4096), dim3(256), 0, st, d->prm, sorted.p, (uint64_t)n, d_keys.p);
    keys.resize((size_t)n * d->nw);
    EB_HIP(hipMemcpyAsync(keys.data(), d_keys.p, keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    EB_HIP(hipStreamSynchronize(st));
    d->d_vlist = std::move(sorted);                                // the edges are built from these very nodes: no second scan of the sets
    return PG_OK;
}

// ---- edges ------------------------------------------------------------------------------------------------------------
// What the steps of p2_build_edges hand to each other: the stage's scratch in its owners (all of it lives to the end of the stage, the lanes'
// records aside, which go behind the gather) and the counts.
struct EbBuild {
    DevArr<unsigned long long> list, cnt;                       // the vertices; the lead's counters
    DevArr<unsigned long long> way_cnt, way_key, seg_end, seg_info, seg_sum, vis_own; DevArr<unsigned int> vis_info;
    DevListing<unsigned long long> way_list;
    EbWay way;                                                  // (plain pointers into the six owners above, for the kernels)
    std::vector<DevListing<EdgeRec>> lane_recs;
    DevArr<EdgeRec> recs;                                       // the lanes' records, one behind the other (the sort puts them in slot order)
    DevArr<unsigned long long> key, key2, ids, bases, id_before, base_before;
    DevArr<uint32_t> idx, order; DevArr<unsigned char> tmp; DevArr<char> text; DevArr<P2EdgeRec> exported;
    DevEvent ev_lead0, ev_lead1;
    uint64_t n_list = 0, n_way = 0, n_rec = 0, patch_cap = 1024;
    unsigned long long n_len1 = 0, total_ids = 0, total_bases = 0;
};

// ---- waypoints (see EbWay): list them, map them, walk their segments
static int eb_waypoint_table(P2Device* d, EbBuild& b) {
    hipStream_t st = d->stream;
    EbWay& way = b.way;
    // on by itself where chains are long on average (slots per vertex; a 60 M-read K = 63 graph has ~300, the K = 127 one over a
    // million): the segment walks probe every linear node twice more, which a graph of short chains need not pay for
    uint32_t period = d->n_slots / (b.n_list + 1) > 4096 ? 512 : 0;
    if (const char* v = pg::env_test("SOAPDENOVO2_AMD_EB_WAYPOINTS")) period = (uint32_t)std::max(0, atoi(v));
    while (period & (period - 1)) period &= period - 1;           // (a power of two)
    if (!period) return PG_OK;
    way.period_mask = period - 1;
    EB_HIP(b.way_cnt.alloc(1));
    auto scan = [&](unsigned long long* list, unsigned long long cap, hipStream_t s) {
        const hipError_t e = hipMemsetAsync(b.way_cnt.p, 0, sizeof(unsigned long long), s);
        if (e != hipSuccess) return e;
        for (int si = 0; si < d->P; si++)
            if (d->set_sizes[si]) hipLaunchKernelGGL(eb_list_branch, dim3(4096), dim3(256), 0, s, d->set_ptr[si], d->nw + 1, d->set_sizes[si], d->set_first[si], list, b.way_cnt.p, cap, 1, way.period_mask);
        return hipGetLastError();
    };
    EB_HIP(b.way_list.begin(d->n_slots / period * 2 + 65536, b.way_cnt.p, 1, 0, st, scan));
    EB_HIP(b.way_list.end("waypoints", 0, st, scan));
    if (b.way_list.short_of_room()) { pg_set_error("edges: the waypoint list is too small"); return PG_ENOMEM; }
    b.n_way = b.way_list.n();
    if (!b.n_way) return PG_OK;
    uint64_t cap_m = 1024;
    while (cap_m < 2 * b.n_way) cap_m <<= 1;
    way.mask = cap_m - 1;
    EB_HIP(b.way_key.alloc(cap_m)); EB_HIP(b.seg_end.alloc(2 * cap_m)); EB_HIP(b.seg_info.alloc(2 * cap_m));
    EB_HIP(b.seg_sum.alloc(2 * cap_m)); EB_HIP(b.vis_own.alloc(2 * cap_m)); EB_HIP(b.vis_info.alloc(2 * cap_m));
    way.key = b.way_key.p; way.seg_end = b.seg_end.p; way.seg_info = b.seg_info.p; way.seg_sum = b.seg_sum.p; way.vis_own = b.vis_own.p; way.vis_info = b.vis_info.p;
    EB_HIP(hipMemsetAsync(way.key, 0, cap_m * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(eb_way_insert, dim3(1024), dim3(256), 0, st, way, b.way_list.list.p, b.n_way);
    // the segment walks: every lane an equal share (the table, the list and what the walks write are the lead's, read and written
    // through the peer mapping; the walk itself probes sets everywhere, whoever runs it)
    EB_HIP(hipStreamSynchronize(st));
    for (size_t l = 0; l < d->lanes.size(); l++) {
        P2Lane& ln = d->lanes[l];
        uint64_t t0, cnt_l;
        p2_share(d, l, 2 * b.n_way, t0, cnt_l);
        if (!cnt_l) continue;
        EB_HIP(hipSetDevice(ln.device));
        const dim3 grid((unsigned)((cnt_l + 255) / 256));
        P2_LAUNCH_NW(d->nw, (eb_way_walk<NW>), grid, dim3(256), 0, ln.stream, p2_lane_params(d, l), way, b.way_list.list.p, t0, cnt_l, ln.d_wcnt + 3);
        EB_HIP(hipGetLastError());
        ln.walks += cnt_l;
    }
    return p2_sync_lanes(d);
}

// ---- the first walks.  A vertex has at most eight arcs and every chain is kept from one of its two ends (palindromes aside, which are few):
// room for five walks a vertex, and a second go with room for all eight should that ever be short.  Every lane walks an equal share of the
// (vertex, arc) pairs into records and counters of its own; the lead gathers the records.
static int eb_first_walks(P2Device* d, EbBuild& b) {
    hipStream_t st = d->stream;
    const size_t NL = d->lanes.size();
    if (b.n_list * 8 / 256 >= 0x7FFFFFFFULL) { pg_set_error("edges: too many vertices for one launch"); return PG_EINVAL; }
    EB_HIP(hipSetDevice(d->device));
    if (b.way.key) EB_HIP(hipMemsetAsync(b.way.vis_own, 0xFF, 2 * (b.way.mask + 1) * sizeof(unsigned long long), st));
    EB_HIP(hipStreamSynchronize(st));
    auto walks_of = [&](size_t l) {
        return [&, l](EdgeRec* recs, unsigned long long cap, hipStream_t s) {
            P2Lane& ln = d->lanes[l];
            uint64_t t0, cnt_l;
            p2_share(d, l, b.n_list * 8, t0, cnt_l);
            const hipError_t e = hipMemsetAsync(ln.d_wcnt, 0, 3 * sizeof(unsigned long long), s);      // (the error counter stays: the segment walks may have used it)
            if (e != hipSuccess || !cnt_l) return e;
            const dim3 grid((unsigned)((cnt_l + 255) / 256));
            P2_LAUNCH_NW(d->nw, (eb_walk<NW>), grid, dim3(256), 0, s, p2_lane_params(d, l), b.list.p, t0, cnt_l, recs, cap, ln.d_wcnt + 1, ln.d_wcnt + 2, ln.d_wcnt + 3, b.way);
            ln.walks += cnt_l;
            return hipGetLastError();
        };
    };
    auto room = [&](size_t l, unsigned a_vertex) { uint64_t t0, cnt_l; p2_share(d, l, b.n_list * 8, t0, cnt_l); return cnt_l / 8 * a_vertex + a_vertex + 1024; };
    b.lane_recs = std::vector<DevListing<EdgeRec>>(NL);
    for (size_t l = 0; l < NL; l++) {
        EB_HIP(hipSetDevice(d->lanes[l].device));
        EB_HIP(b.lane_recs[l].begin(room(l, 5), d->lanes[l].d_wcnt, 4, 1, d->lanes[l].stream, walks_of(l)));
    }
    unsigned long long errors = 0;
    bool short_of_room = false;
    for (size_t l = 0; l < NL; l++) {
        DevListing<EdgeRec>& lr = b.lane_recs[l];
        EB_HIP(hipSetDevice(d->lanes[l].device));
        EB_HIP(lr.end("walk records", room(l, 8), d->lanes[l].stream, walks_of(l)));
        b.n_rec += lr.cnt[1]; b.n_len1 += lr.cnt[2]; errors += lr.cnt[3];
        short_of_room = short_of_room || lr.short_of_room();
    }
    EB_HIP(hipSetDevice(d->device));
    if (errors) { pg_set_error("Kmer is not found while building an edge."); return PG_EINVAL; }
    if (short_of_room) { pg_set_error("edges: more walks than arcs"); return PG_EINVAL; }
    if (b.n_rec) {
        EB_HIP(b.recs.alloc(b.n_rec));
        uint64_t at = 0;
        for (size_t l = 0; l < NL; l++) {
            const uint64_t c = b.lane_recs[l].n();
            if (c) EB_HIP(p2r_copy(b.recs.p + at, d->device, b.lane_recs[l].list.p, d->lanes[l].device, c * sizeof(EdgeRec), st));
            at += c;
        }
        EB_HIP(hipStreamSynchronize(st));
    }
    for (size_t l = 0; l < NL; l++) b.lane_recs[l].list.reset();
    if (b.n_rec >= 0x7FFFFFFFULL) { pg_set_error("edges: more than 2^31 - 1 edge records"); return PG_EINVAL; }
    return PG_OK;
}

// ---- ids and offsets: the sort by (slot, arc) and the prefix sums over ids and bases give edge ids and text offsets in the reference's order
static int eb_ids_and_offsets(P2Device* d, EbBuild& b) {
    hipStream_t st = d->stream;
    const uint64_t n_rec = b.n_rec;
    unsigned long long last_ids = 0, last_bases = 0, last_idb = 0, last_bb = 0;
    EB_HIP(b.key.alloc(n_rec)); EB_HIP(b.key2.alloc(n_rec)); EB_HIP(b.idx.alloc(n_rec)); EB_HIP(b.order.alloc(n_rec));
    EB_HIP(b.ids.alloc(n_rec)); EB_HIP(b.bases.alloc(n_rec)); EB_HIP(b.id_before.alloc(n_rec)); EB_HIP(b.base_before.alloc(n_rec));
    // (PG_HOST_VERBOSE, several lanes: the device time of this block -- the sort by (slot, arc) and the prefix sums over ids and bases, on the lead alone --
    //  is said at the end: VERDICT r5, 3c)
    if (d->lanes.size() > 1 && pg::env_user("PG_HOST_VERBOSE") && hipEventCreate(&b.ev_lead0.ev) == hipSuccess && hipEventCreate(&b.ev_lead1.ev) == hipSuccess) (void)hipEventRecord(b.ev_lead0.ev, st);
    hipLaunchKernelGGL(eb_keys, dim3(2048), dim3(256), 0, st, b.recs.p, n_rec, b.key.p, b.idx.p);
    EB_HIP(b.tmp.alloc(std::max(dev_sort_pairs_bytes(b.key.p, b.key2.p, b.idx.p, b.order.p, (size_t)n_rec, 64u, st), dev_exclusive_sum_bytes(b.ids.p, b.id_before.p, (size_t)n_rec, st))));
    EB_HIP(dev_sort_pairs(b.tmp, b.key.p, b.key2.p, b.idx.p, b.order.p, (size_t)n_rec, 64u, st));
    hipLaunchKernelGGL(eb_sizes, dim3(2048), dim3(256), 0, st, b.recs.p, b.order.p, n_rec, b.ids.p, b.bases.p);
    EB_HIP(dev_exclusive_sum(b.tmp, b.ids.p, b.id_before.p, (size_t)n_rec, st));
    EB_HIP(dev_exclusive_sum(b.tmp, b.bases.p, b.base_before.p, (size_t)n_rec, st));
    if (b.ev_lead1.ev) (void)hipEventRecord(b.ev_lead1.ev, st);
    EB_HIP(hipMemcpyAsync(&last_ids, b.ids.p + n_rec - 1, 8, hipMemcpyDeviceToHost, st)); EB_HIP(hipMemcpyAsync(&last_bases, b.bases.p + n_rec - 1, 8, hipMemcpyDeviceToHost, st));
    EB_HIP(hipMemcpyAsync(&last_idb, b.id_before.p + n_rec - 1, 8, hipMemcpyDeviceToHost, st)); EB_HIP(hipMemcpyAsync(&last_bb, b.base_before.p + n_rec - 1, 8, hipMemcpyDeviceToHost, st));
    EB_HIP(hipStreamSynchronize(st));
    b.total_ids = last_idb + last_ids;
    b.total_bases = last_bb + last_bases;
    if (b.total_ids >= 0xFFFFFFFFULL) { pg_set_error("edges: edge ids exceed 32 bits"); return PG_EINVAL; }
    return PG_OK;
}

// ---- the second walk of every kept chain (bases, tags, unlinking), dealt like the first: a lane of the graph an equal share of the walks in
// slot order, then of the waypoint table's entries
static int eb_second_walks(P2Device* d, EbBuild& b) {
    hipStream_t st = d->stream;
    const size_t NL = d->lanes.size();
    std::vector<unsigned long long> lane_cnt(4 * NL, 0);
    EB_HIP(b.text.alloc(b.total_bases));
    EB_HIP(hipStreamSynchronize(st));
    for (size_t l = 0; l < NL; l++) {
        P2Lane& ln = d->lanes[l];
        uint64_t i0, cnt_l;
        p2_share(d, l, b.n_rec, i0, cnt_l);
        EB_HIP(hipSetDevice(ln.device));
        if (cnt_l) {
            const dim3 grid((unsigned)((cnt_l + 255) / 256));
            P2_LAUNCH_NW(d->nw, (eb_apply<NW>), grid, dim3(256), 0, ln.stream, p2_lane_params(d, l), b.recs.p, b.order.p, i0, cnt_l, b.id_before.p, b.base_before.p, b.text.p,
                                               d->d_patch_keys, d->d_patch_val, b.patch_cap - 1, ln.d_wcnt + 3, b.way);
            EB_HIP(hipGetLastError());
            ln.walks += cnt_l;
        }
        if (b.way.key) {                                              // the segments behind the waypoints the kept walks passed
            uint64_t t0, cnt_s;
            p2_share(d, l, 2 * (b.way.mask + 1), t0, cnt_s);
            const dim3 gs((unsigned)((cnt_s + 255) / 256));
            if (cnt_s) P2_LAUNCH_NW(d->nw, (eb_apply_seg<NW>), gs, dim3(256), 0, ln.stream, p2_lane_params(d, l), b.way, b.recs.p, b.order.p, b.key2.p, b.n_rec, b.id_before.p, b.base_before.p, b.text.p, ln.d_wcnt + 3, t0, cnt_s);
            EB_HIP(hipGetLastError());
        }
        EB_HIP(hipMemcpyAsync(&lane_cnt[4 * l], ln.d_wcnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ln.stream));
    }
    const int rc = p2_sync_lanes(d);
    if (rc) return rc;
    for (size_t l = 0; l < NL; l++) if (lane_cnt[4 * l + 3]) { pg_set_error("edges: a walk did not repeat itself"); return PG_EINVAL; }
    return PG_OK;
}

// ---- export: what the host needs for the text records -- the walks in slot order with their text offsets, and the bases
static int eb_export_edges(P2Device* d, EbBuild& b, P2Edges& out) {
    hipStream_t st = d->stream;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    EB_HIP(b.exported.alloc(b.n_rec));
    hipLaunchKernelGGL(eb_export, dim3(2048), dim3(256), 0, st, b.recs.p, b.order.p, b.base_before.p, b.n_rec, b.exported.p);
    out.recs.resize(b.n_rec);
    out.text.resize(b.total_bases);
    EB_HIP(hipMemcpyAsync(out.recs.data(), b.exported.p, b.n_rec * sizeof(P2EdgeRec), hipMemcpyDeviceToHost, st));
    if (b.total_bases) EB_HIP(hipMemcpyAsync(&out.text[0], b.text.p, b.total_bases, hipMemcpyDeviceToHost, st));
    EB_HIP(hipMemcpyAsync(cnt, b.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    EB_HIP(hipStreamSynchronize(st));
    if (cnt[3]) { pg_set_error("edges: a walk did not repeat itself"); return PG_EINVAL; }
    return PG_OK;
}

int p2_build_edges(P2Device* d, P2Edges& out) {
    int rc = PG_OK;
    hipStream_t st = d->stream;
    const size_t NL = d->lanes.size();
    const auto t_stage0 = std::chrono::steady_clock::now();
    if (hipSetDevice(d->device) != hipSuccess) { pg_set_error("edges: hipSetDevice failed"); return PG_ENODEV; }
    P2BackOn back{d->device};
    EbBuild b;
    memset(&b.way, 0, sizeof b.way);
    b.way.period_mask = 0xFFFFFFFFu;
    for (size_t l = 0; l < NL; l++) {                                     // the lanes' counters of this stage (lane 0's d_wcnt exists from p2_use_lanes on, or now)
        P2Lane& ln = d->lanes[l];
        EB_HIP(hipSetDevice(ln.device));
        if (!ln.d_wcnt) EB_HIP(pg::arena_malloc((void**)&ln.d_wcnt, 4 * sizeof(unsigned long long)));
        EB_HIP(hipMemsetAsync(ln.d_wcnt, 0, 4 * sizeof(unsigned long long), ln.stream));
        EB_HIP(hipStreamSynchronize(ln.stream));
    }
    EB_HIP(hipSetDevice(d->device));
    EB_HIP(b.cnt.alloc(4));
    EB_HIP(hipMemsetAsync(b.cnt.p, 0, 4 * sizeof(unsigned long long), st));
    if (d->d_vlist.p) {                                            // listed for <prefix>.vertex a moment ago (nothing changed a flag since)
        b.list = std::move(d->d_vlist);
        b.n_list = b.list.n;
    } else {
        unsigned long long n_listed = 0;
        if ((rc = p2_list_branch_nodes(d, b.list, &n_listed)) != PG_OK) return rc;
        b.n_list = n_listed;
    }
    if ((rc = eb_waypoint_table(d, b)) != PG_OK) return rc;
    if ((rc = eb_first_walks(d, b)) != PG_OK) return rc;
    // the (K+1)-mer table the length-1 edges enter (eb_apply).  PG_EB_PATCH_ROOM=n (test hook): its first size is n, so that the rule below decides the
    // size at test sizes as well -- loads of 25 - 50 %
    if (const char* v = pg::env_test("PG_EB_PATCH_ROOM")) {
        const long long room = atoll(v);
        if (room < 1 || (room & (room - 1))) { pg_set_error("pass 2: patch table size must be a power of two"); return PG_EINVAL; }
        b.patch_cap = (uint64_t)room;
    }
    while (b.patch_cap < 2 * b.n_len1 + 2) b.patch_cap <<= 1;
    {
        DevArr<uint64_t> keys; DevArr<uint32_t> val;
        p2_drop_patch(d);
        EB_HIP(keys.alloc(b.patch_cap * d->nw)); EB_HIP(val.alloc(b.patch_cap * 2));
        EB_HIP(hipMemsetAsync(keys.p, 0, b.patch_cap * d->nw * sizeof(uint64_t), st));
        EB_HIP(hipMemsetAsync(val.p, 0, b.patch_cap * 2 * sizeof(uint32_t), st));
        p2_take_patch(d, keys, val, b.patch_cap);
    }
    out.recs.clear(); out.text.clear();
    out.n_ids = 0; out.n_len1 = (long long)b.n_len1;
    if (b.n_rec) {
        if ((rc = eb_ids_and_offsets(d, b)) != PG_OK) return rc;
        if ((rc = eb_second_walks(d, b)) != PG_OK) return rc;
        if ((rc = eb_export_edges(d, b, out)) != PG_OK) return rc;
    }
    out.n_ids = (long long)b.total_ids;
    if (b.ev_lead0.ev && b.ev_lead1.ev) {
        float ms = 0;
        if (hipEventSynchronize(b.ev_lead1.ev) == hipSuccess && hipEventElapsedTime(&ms, b.ev_lead0.ev, b.ev_lead1.ev) == hipSuccess)
            fprintf(stderr, "edges, sharded: the sort by (slot, arc) and the prefix sums run on the lead alone: %.1f ms of device time, of %.1f ms the stage took on the device side in all (walks and applies dealt to %zu lane(s))\n",
                    ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_stage0).count(), NL);
    }
    if (pg::env_user("PG_HOST_VERBOSE") && b.n_way) fprintf(stderr, "edges: %llu waypoint(s) (about every %u-th linear node): chains walked by jumps\n", (unsigned long long)b.n_way, b.way.period_mask + 1);
    return PG_OK;
}

void p2_destroy(P2Device* d) { p2_free(d); }

// all: n entries on the current device (consumed: released when the fold is over); merge: entries of one pair may repeat (several lanes)
static int p2_fold_arcs(DevArr<P2Arc> all, uint64_t n, bool merge, hipStream_t st, std::vector<uint32_t>& out3) {
    out3.clear();
    if (!n) return PG_OK;
    if (n >= 0xFFFFFFFFull) { pg_set_error("pass 2: more than 2^32 pre-arcs in one fold"); return PG_EINVAL; }
    using SortP = unsigned long long;
    DevArr<SortP> key, key2, head, pos; DevArr<uint32_t> idx, ord, ord2, d_out3; DevArr<P2Arc> merged; DevArr<unsigned char> tmp;
    const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 8192);
    EB_HIP(tmp.alloc(std::max(dev_sort_pairs_bytes(key.p, key2.p, idx.p, ord.p, (size_t)n, 64u, st), dev_exclusive_sum_bytes(head.p, pos.p, (size_t)n, st))));
    EB_HIP(key.alloc(n)); EB_HIP(key2.alloc(n));
    EB_HIP(idx.alloc(n)); EB_HIP(ord.alloc(n)); EB_HIP(ord2.alloc(n));
    if (merge) {
        EB_HIP(head.alloc(n)); EB_HIP(pos.alloc(n));
        EB_HIP(merged.alloc(n));
        hipLaunchKernelGGL(pf_pair_keys, dim3(grid), dim3(256), 0, st, all.p, n, key.p, idx.p);
        EB_HIP(dev_sort_pairs(tmp, key.p, key2.p, idx.p, ord.p, (size_t)n, 64u, st));
        hipLaunchKernelGGL(pf_heads, dim3(grid), dim3(256), 0, st, key2.p, n, head.p);
        EB_HIP(dev_exclusive_sum(tmp, head.p, pos.p, (size_t)n, st));
        hipLaunchKernelGGL(pf_merge, dim3(grid), dim3(256), 0, st, all.p, key2.p, ord.p, head.p, pos.p, n, merged.p);
        unsigned long long last[2] = {0, 0};
        EB_HIP(hipMemcpyAsync(&last[0], pos.p + n - 1, 8, hipMemcpyDeviceToHost, st));
        EB_HIP(hipMemcpyAsync(&last[1], head.p + n - 1, 8, hipMemcpyDeviceToHost, st));
        EB_HIP(hipStreamSynchronize(st));
        n = last[0] + last[1];
        std::swap(all, merged);                                      // (both are released at the end)
    }
    hipLaunchKernelGGL(pf_first_keys, dim3(grid), dim3(256), 0, st, all.p, n, key.p, idx.p);
    EB_HIP(dev_sort_pairs(tmp, key.p, key2.p, idx.p, ord.p, (size_t)n, 64u, st));
    hipLaunchKernelGGL(pf_from_keys, dim3(grid), dim3(256), 0, st, all.p, ord.p, n, key.p);
    EB_HIP(dev_sort_pairs(tmp, key.p, key2.p, ord.p, ord2.p, (size_t)n, 32u, st));
    EB_HIP(d_out3.alloc(n * 3));
    hipLaunchKernelGGL(pf_gather, dim3(grid), dim3(256), 0, st, all.p, ord2.p, n, d_out3.p);
    EB_HIP(hipGetLastError());
    out3.resize((size_t)n * 3);
    EB_HIP(hipMemcpyAsync(out3.data(), d_out3.p, n * 12, hipMemcpyDeviceToHost, st));
    EB_HIP(hipStreamSynchronize(st));
    return PG_OK;
}

int p2_finish(P2Device* d, P2Result& out) {
    if (d->route) { const int rc = p2_route_round(d); if (rc) return rc; }        // the batches still waiting for a full round
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<unsigned long long> lane_arcs(d->lanes.size(), 0);
    for (size_t l = 0; l < d->lanes.size(); l++) {
        P2Lane& ln = d->lanes[l];
        if (!ln.tables) continue;
        P2_HIP(hipSetDevice(ln.device));
        P2_HIP(hipStreamSynchronize(ln.stream));
        P2_HIP(hipMemsetAsync(ln.d_counters + 3, 0, sizeof(unsigned long long), ln.stream));
        hipLaunchKernelGGL(p2_count_arcs, dim3(2048), dim3(256), 0, ln.stream, ln.d_arc, ln.prm.arc_mask + 1, ln.d_counters + 3);
        P2_HIP(hipGetLastError());
        P2_HIP(hipStreamSynchronize(ln.stream));
        unsigned long long cl[8];
        P2_HIP(hipMemcpy(cl, ln.d_counters, sizeof(cl), hipMemcpyDeviceToHost));
        for (int q = 0; q < 8; q++) c[q] += cl[q];
        lane_arcs[l] = cl[3];
    }
    p2_drop_look(d);                                   // (every batch is through: the room goes to the fold)
    if (pg::env_user("PG_HOST_VERBOSE"))
        for (size_t l = 0; l < d->lanes.size(); l++)
            fprintf(stderr, "graph lane %zu (device %d): pass 2 threaded %llu read(s) in %llu batch(es), %llu distinct pre-arc(s); %llu per-set scan(s) ran here; %llu tip / edge walk(s) ran here\n", l, d->lanes[l].device,
                    (unsigned long long)d->lanes[l].reads, (unsigned long long)d->lanes[l].batches, lane_arcs[l], (unsigned long long)d->lanes[l].scans, (unsigned long long)d->lanes[l].walks);
    if (pg::env_user("PG_HOST_VERBOSE") && d->lanes.size() > 1) {
        if (d->route) {
            unsigned long long reads = 0, sent = 0, away = 0;
            for (const P2Lane& ln : d->lanes) {
                fprintf(stderr, "pass 2 routed, lane of device %d: asked %llu lookup(s), %llu of them of other lanes, in %llu round(s); answered %llu from its own sets; 0 probes of peer-mapped sets\n", ln.device,
                        (unsigned long long)ln.lookups_sent, (unsigned long long)ln.lookups_sent_away, (unsigned long long)ln.route_rounds, (unsigned long long)ln.lookups_answered);
                reads += ln.reads; sent += ln.lookups_sent; away += ln.lookups_sent_away;
            }
            fprintf(stderr, "pass 2 routed: %.1f bytes a read crossed between lanes (%d-byte keys out, 8-byte node words back; %.1f lookups a read, %.0f %% of them of another lane)\n",
                    reads ? (double)away * (d->nw * 8 + 8) / (double)reads : 0.0, d->nw * 8, reads ? (double)sent / (double)reads : 0.0, sent ? 100.0 * (double)away / (double)sent : 0.0);
        } else fprintf(stderr, "pass 2 direct: every lane probed the peer-mapped sets itself (about %d of %d probes remote)\n", (int)d->lanes.size() - 1, (int)d->lanes.size());
    }
    if (c[1]) { pg_set_error("pass 2: " + std::to_string(c[1]) + " k-mer(s) of the reads are not in the sets"); return PG_EINVAL; }
    if (c[2]) { pg_set_error("pass 2: pre-arc table overflow"); return PG_ENOMEM; }
    if (c[5]) { pg_set_error("pass 2: edge id out of range"); return PG_EINVAL; }
    out.reads_deleted = (long long)c[0];
    out.markers = (long long)c[4];
    out.lanes = (int)d->lanes.size();
    const size_t n_arcs = (size_t)c[3];                            // (a pair met on several lanes is counted by each: merged below, or by the caller)
    // SOAPDENOVO2_AMD_PREARC_FOLD=host: the round-5 form (24-byte entries to the host, bucketed and sorted there), for the A/B
    const char* fold_env = pg::env_user("SOAPDENOVO2_AMD_PREARC_FOLD");
    const bool dev_fold = !(fold_env && !strcmp(fold_env, "host")) && n_arcs > 0 && n_arcs < 0xFFFFFFFFull;
    out.folded = false; out.folded3.clear(); out.arcs.clear();
    if (!dev_fold) out.arcs.assign(n_arcs, P2Arc{0, 0, 0, 0});
    out.marker.clear();
    if (d->reps) out.marker.assign((size_t)d->num_ed + 1, 0u);
    DevArr<P2Arc> d_all;                                           // on the lead device: every lane's entries, one after the other
    if (dev_fold) { P2_HIP(hipSetDevice(d->device)); P2_HIP(d_all.alloc(n_arcs)); }
    size_t at = 0;
    for (size_t l = 0; l < d->lanes.size(); l++) {
        P2Lane& ln = d->lanes[l];
        if (!ln.tables) continue;
        P2_HIP(hipSetDevice(ln.device));
        const uint64_t cap = ln.prm.arc_mask + 1;
        const size_t n_l = (size_t)lane_arcs[l];
        if (n_l) {
            DevArr<P2Arc> own_arcs;
            const bool in_place = dev_fold && ln.device == d->device;      // a lane of the lead's GPU writes straight into the common array
            if (!in_place) P2_HIP(own_arcs.alloc(n_l));
            P2Arc* const d_arcs = in_place ? d_all.p + at : own_arcs.p;
            P2_HIP(hipMemsetAsync(ln.d_counters + 6, 0, sizeof(unsigned long long), ln.stream));
            hipLaunchKernelGGL(p2_compact_arcs, dim3(2048), dim3(256), 0, ln.stream, ln.d_arc, cap, d_arcs, ln.d_counters + 6, (unsigned long long)n_l);
            if (!dev_fold) P2_HIP(hipMemcpyAsync(out.arcs.data() + at, d_arcs, n_l * sizeof(P2Arc), hipMemcpyDeviceToHost, ln.stream));
            else if (!in_place) P2_HIP(hipMemcpyPeerAsync(d_all.p + at, d->device, d_arcs, ln.device, n_l * sizeof(P2Arc), ln.stream));
            unsigned long long got = 0;
            P2_HIP(hipMemcpyAsync(&got, ln.d_counters + 6, sizeof(got), hipMemcpyDeviceToHost, ln.stream));
            P2_HIP(hipStreamSynchronize(ln.stream));
            own_arcs.reset();
            if (got != n_l) { pg_set_error("pass 2: pre-arc table is inconsistent"); return PG_EINVAL; }
            at += n_l;
        }
        if (d->reps) {
            std::vector<unsigned int> m((size_t)d->num_ed + 1);
            P2_HIP(hipMemcpy(m.data(), ln.d_marker, m.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
            for (size_t e = 0; e < m.size(); e++) out.marker[e] += m[e];
        }
    }
    if (dev_fold) {
        P2_HIP(hipSetDevice(d->device));
        const int rc = p2_fold_arcs(std::move(d_all), n_arcs, d->lanes.size() > 1, d->lanes[0].stream, out.folded3);      // (releases d_all)
        if (rc) return rc;
        out.folded = true;
    }
    P2_HIP(hipSetDevice(d->device));
    return PG_OK;
}

// ---- TEST HOOKS ONLY (pg_device_emu_*): the device twins of pg_host_emu_* (host_emu.cpp, host_graph.cpp).  Host arrays go up, the
// product's own entry points run (p2_layout_rank, p2_layout_rank_growable, HipBackend::launch of home_slot, HipBackend::append_at), the
// result comes down; tests/test_gpu_dev_graph.py holds them to the models the CPU tests hold the HostBackend to.  Nothing in the product
// path calls these.
static int emu_device(int device, const char* who) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { pg_set_error(std::string(who) + ": no HIP device"); return PG_ENODEV; }
    if (device < 0 || device >= n) { pg_set_error(std::string(who) + ": HIP device " + std::to_string(device) + " does not exist"); return PG_ENODEV; }
    P2_HIP(hipSetDevice(device));
    return PG_OK;
}
// host words into a fresh device block (nothing for n = 0)
template <typename T>
static int emu_upload(const T* src, uint64_t n, DevArr<T>& d_out) {
    if (!n) return PG_OK;
    if (d_out.alloc(n) != hipSuccess) { pg_set_error("test hook: out of device memory"); return PG_ENOMEM; }
    if (hipMemcpy(d_out.p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { d_out.reset(); pg_set_error("test hook: upload failed"); return PG_ENODEV; }
    return PG_OK;
}
static int emu_download(int device, const uint64_t* d_src, uint64_t n_words, uint64_t* dst) {
    int rc = n_words ? p2_fetch_words(device, d_src, n_words, dst) : PG_OK;
    (void)p2_fetch_words(device, nullptr, 0, nullptr);                 // (the caller's array stays page-locked no longer than this call)
    if (rc) pg_set_error("test hook: download failed");
    return rc;
}

extern "C" int pg_device_emu_layout_static(int device, const uint64_t* records, const uint64_t* per_set_count, int n_sets, uint64_t set_size, int mer127,
                                           uint64_t* nodes_out) {
    if (!records || !per_set_count || !nodes_out || n_sets < 1 || set_size < 2) { pg_set_error("pg_device_emu_layout_static: bad argument"); return PG_EINVAL; }
    int rc = emu_device(device, "pg_device_emu_layout_static");
    if (rc) return rc;
    pg::ArenaPin pin(device);                                          // (one life of the arena for the call's blocks, not one for every block)
    const int nw = mer127 ? 4 : 2;
    uint64_t n = 0;
    for (int s = 0; s < n_sets; s++) n += per_set_count[s];
    DevArr<uint64_t> d_rec;
    if ((rc = emu_upload(records, n * (uint64_t)(nw + 2), d_rec)) != PG_OK) return rc;
    uint64_t* nodes = nullptr;
    void* alloc = nullptr;
    rc = p2_layout_rank(device, nw, n_sets, d_rec.p, per_set_count, set_size, &nodes, &alloc);
    if (rc == PG_OK) {
        rc = emu_download(device, nodes, (uint64_t)n_sets * set_size * (uint64_t)(nw + 1), nodes_out);
        pg_device_release_layout(device, alloc);
    }
    return rc;
}

extern "C" int pg_device_emu_layout_growable(int device, const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int mer127, int n_sets,
                                             uint64_t* out_set_size, uint64_t* out_rounds, uint64_t* out_nodes, uint64_t nodes_cap_slots) {
    if ((!records && n_records) || !out_nodes || n_sets < 1 || n_sets > P2_MAX_SETS) { pg_set_error("pg_device_emu_layout_growable: bad argument"); return PG_EINVAL; }
    int rc = emu_device(device, "pg_device_emu_layout_growable");
    if (rc) return rc;
    pg::ArenaPin pin(device);                                          // (one life of the arena for the call's blocks, not one for every block)
    const int nw = mer127 ? 4 : 2;
    std::vector<uint64_t> cnt;
    std::vector<unsigned char> trailing;
    if (!growable_counts_of_records(records, n_records, nw, set_last_put, n_sets, cnt, trailing)) { pg_set_error("records are not sorted by set"); return PG_EINVAL; }
    DevArr<uint64_t> d_rec;
    if ((rc = emu_upload(records, n_records * (uint64_t)(nw + 2), d_rec)) != PG_OK) return rc;
    std::vector<uint64_t> sizes((size_t)n_sets, 0), rounds((size_t)n_sets, 0);
    uint64_t* nodes = nullptr;
    void* alloc = nullptr;
    rc = p2_layout_rank_growable(device, nw, n_sets, d_rec.p, cnt.data(), trailing.data(), ref_initial_set_size(0, n_sets, mer127 ? 1 : 0), sizes.data(), &nodes, &alloc,
                                 rounds.data());
    if (rc == PG_OK) {
        uint64_t total = 0;
        for (int s = 0; s < n_sets; s++) {
            total += sizes[s];
            if (out_set_size) out_set_size[s] = sizes[s];
            if (out_rounds) out_rounds[s] = rounds[s];
        }
        if (nodes_cap_slots < total) { pg_set_error("node image too small"); rc = PG_EINVAL; }
        else rc = emu_download(device, nodes, total * (uint64_t)(nw + 1), out_nodes);
        pg_device_release_layout(device, alloc);
    }
    return rc;
}

template <int NW>
int emu_home_slots_on(HipBackend& be, const uint64_t* d_keys, uint64_t n, uint64_t size, unsigned long long* d_out) {
    const ModConst mc = make_modconst(size);
    be.launch(n, [=] PG_LAMBDA(uint64_t i) {
        Kmer<NW> k;
#pragma unroll
        for (int w = 0; w < NW; w++) k.w[w] = d_keys[(uint64_t)NW * i + w];
        d_out[i] = home_slot<NW>(k, mc);
    });
    be.sync();
    return be.error;
}
extern "C" int pg_device_emu_home_slots(int device, const uint64_t* keys, uint64_t n, int mer127, uint64_t size, uint64_t* out) {
    if (!keys || !out || size < 1 || (size >> 63)) { pg_set_error("pg_device_emu_home_slots: bad argument"); return PG_EINVAL; }
    int rc = emu_device(device, "pg_device_emu_home_slots");
    if (rc || !n) return rc;
    pg::ArenaPin pin(device);                                          // (one life of the arena for the call's blocks, not one for every block)
    const int nw = mer127 ? 4 : 2;
    DevArr<uint64_t> d_keys;
    if ((rc = emu_upload(keys, n * (uint64_t)nw, d_keys)) != PG_OK) return rc;
    DevArr<unsigned long long> d_out;
    hipStream_t st = nullptr;
    if (d_out.alloc(n) != hipSuccess) { pg_set_error("test hook: out of device memory"); rc = PG_ENOMEM; }
    else if (hipStreamCreate(&st) != hipSuccess) { st = nullptr; pg_set_error("test hook: no stream"); rc = PG_ENODEV; }
    else {
        std::string why;
        {
            HipBackend be(device, st);
            rc = mer127 ? emu_home_slots_on<4>(be, d_keys.p, n, size, d_out.p) : emu_home_slots_on<2>(be, d_keys.p, n, size, d_out.p);
            why = be.error_text;
        }
        if (rc) pg_set_error("pg_device_emu_home_slots: " + why);
        else rc = emu_download(device, (const uint64_t*)d_out.p, n, out);
    }
    if (st) (void)hipStreamDestroy(st);
    return rc;
}

int emu_append_on(HipBackend& be, const unsigned char* d_flags, uint64_t n, unsigned long long* d_list, unsigned long long* d_cnt, uint64_t cap) {
    be.append_at(0, n, [=] PG_LAMBDA(uint64_t i) -> unsigned long long { return d_flags[i] ? PG_EMU_APPEND_BASE + i : ~0ULL; }, d_list, d_cnt, cap);
    be.sync_places();
    return be.error;
}
extern "C" int pg_device_emu_append(int device, const unsigned char* flags, uint64_t n, uint64_t cap, uint64_t* list_out, uint64_t* count_out) {
    if ((!flags && n) || (!list_out && cap) || !count_out || n >= ~0ULL - PG_EMU_APPEND_BASE) { pg_set_error("pg_device_emu_append: bad argument"); return PG_EINVAL; }
    int rc = emu_device(device, "pg_device_emu_append");
    if (rc) return rc;
    pg::ArenaPin pin(device);                                          // (one life of the arena for the call's blocks, not one for every block)
    for (uint64_t i = 0; i < cap; i++) list_out[i] = ~0ULL;
    *count_out = 0;
    if (!n) return PG_OK;
    // the list lies in front of GUARD words the kernel has no business with: a write behind `cap` is an error of this call, not a stray store
    constexpr uint64_t GUARD = 1024;
    DevArr<unsigned char> d_flags;
    if ((rc = emu_upload(flags, n, d_flags)) != PG_OK) return rc;
    DevArr<unsigned long long> d_list;                                 // [cap + GUARD] list, then [1] counter
    hipStream_t st = nullptr;
    std::vector<uint64_t> back;
    if (d_list.alloc(cap + GUARD + 1) != hipSuccess) { pg_set_error("test hook: out of device memory"); rc = PG_ENOMEM; }
    else if (hipStreamCreate(&st) != hipSuccess) { st = nullptr; pg_set_error("test hook: no stream"); rc = PG_ENODEV; }
    else {
        std::string why;
        {
            HipBackend be(device, st);
            be.fill(d_list.p, (size_t)(cap + GUARD), ~0ULL);
            be.fill(d_list.p + cap + GUARD, 1, 0ULL);
            rc = emu_append_on(be, d_flags.p, n, d_list.p, d_list.p + cap + GUARD, cap);
            why = be.error_text;
        }
        if (rc) pg_set_error("pg_device_emu_append: " + why);
        else {
            back.resize((size_t)(cap + GUARD + 1));
            rc = emu_download(device, (const uint64_t*)d_list.p, cap + GUARD + 1, back.data());
        }
    }
    if (rc == PG_OK) {
        for (uint64_t i = 0; i < cap; i++) list_out[i] = back[i];
        *count_out = back[cap + GUARD];
        for (uint64_t i = cap; i < cap + GUARD; i++) if (back[i] != ~0ULL) { pg_set_error("pg_device_emu_append: the kernel wrote behind cap"); rc = PG_ESTATE; break; }
    }
    if (st) (void)hipStreamDestroy(st);
    return rc;
}

// Pass 2's pre-arc path on caller-given triples: triple `first + t * stride` goes into the table of p through the product's add_prearc (p carries arc,
// arc_mask and counters, nothing else), one lane a triple -- neighbours in the input are neighbours in a wave.
__global__ __launch_bounds__(256) void emu_prearc_insert(P2Params p, const uint32_t* __restrict__ from, const uint32_t* __restrict__ to, const unsigned long long* __restrict__ seq,
                                                         uint64_t first, uint64_t stride, uint64_t n) {
    const uint64_t i = first + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * stride;
    if (i < n) add_prearc(p, from[i], to[i], seq[i]);
}
// the tables of `lanes` lanes filled, then read out, gathered and folded as p2_finish does it (count, compact into one array, p2_fold_arcs)
static int emu_prearcs_on(const uint32_t* d_from, const uint32_t* d_to, const unsigned long long* d_seq, uint64_t n, uint64_t room, int lanes, hipStream_t st,
                          std::vector<uint32_t>& out3, unsigned long long* overflow) {
    std::vector<DevArr<unsigned long long>> arc((size_t)lanes), counters((size_t)lanes);
    std::vector<unsigned long long> lane_arcs((size_t)lanes, 0);
    unsigned long long n_arcs = 0;
    *overflow = 0;
    for (int l = 0; l < lanes; l++) {
        P2_HIP(arc[l].alloc(room * ARC_WORDS)); P2_HIP(counters[l].alloc(8));
        hipLaunchKernelGGL(p2_arc_init, dim3(2048), dim3(256), 0, st, arc[l].p, room);
        P2_HIP(hipMemsetAsync(counters[l].p, 0, 8 * sizeof(unsigned long long), st));
        P2Params p{};
        p.arc = arc[l].p; p.arc_mask = room - 1; p.counters = counters[l].p;
        const uint64_t mine = n > (uint64_t)l ? (n - l + lanes - 1) / lanes : 0;
        if (mine) hipLaunchKernelGGL(emu_prearc_insert, dim3((unsigned)((mine + 255) / 256)), dim3(256), 0, st, p, d_from, d_to, d_seq, (uint64_t)l, (uint64_t)lanes, n);
        hipLaunchKernelGGL(p2_count_arcs, dim3(2048), dim3(256), 0, st, arc[l].p, room, counters[l].p + 3);
        P2_HIP(hipGetLastError());
        unsigned long long cl[8];
        P2_HIP(hipMemcpyAsync(cl, counters[l].p, sizeof(cl), hipMemcpyDeviceToHost, st));
        P2_HIP(hipStreamSynchronize(st));
        *overflow += cl[2];
        lane_arcs[l] = cl[3];
        n_arcs += cl[3];
    }
    out3.clear();
    if (*overflow || !n_arcs) return PG_OK;
    DevArr<P2Arc> d_all;
    P2_HIP(d_all.alloc((size_t)n_arcs));
    size_t at = 0;
    for (int l = 0; l < lanes; l++) {
        const unsigned long long n_l = lane_arcs[l];
        if (!n_l) continue;
        hipLaunchKernelGGL(p2_compact_arcs, dim3(2048), dim3(256), 0, st, arc[l].p, room, d_all.p + at, counters[l].p + 6, n_l);
        unsigned long long got = 0;
        P2_HIP(hipMemcpyAsync(&got, counters[l].p + 6, sizeof(got), hipMemcpyDeviceToHost, st));
        P2_HIP(hipStreamSynchronize(st));
        if (got != n_l) { pg_set_error("pg_device_emu_prearcs: pre-arc table is inconsistent"); return PG_EINVAL; }
        at += (size_t)n_l;
        arc[l].reset(); counters[l].reset();
    }
    return p2_fold_arcs(std::move(d_all), n_arcs, lanes > 1, st, out3);
}
extern "C" int pg_device_emu_prearcs(int device, const uint32_t* from, const uint32_t* to, const uint64_t* seq, uint64_t n, uint64_t room, int lanes,
                                     uint32_t* out3, uint64_t* count_out, uint64_t* overflow_out) {
    if ((n && (!from || !to || !seq || !out3)) || !count_out || !overflow_out || room < 2 || (room & (room - 1)) || room > (1ULL << 32) || lanes < 1 ||
        n >= 0xFFFFFFFFull) { pg_set_error("pg_device_emu_prearcs: bad argument"); return PG_EINVAL; }
    for (uint64_t i = 0; i < n; i++) if (!from[i] && !to[i]) { pg_set_error("pg_device_emu_prearcs: the pair (0, 0) is the table's empty key"); return PG_EINVAL; }
    *count_out = 0; *overflow_out = 0;
    int rc = emu_device(device, "pg_device_emu_prearcs");
    if (rc || !n) return rc;
    pg::ArenaPin pin(device);                                          // (one life of the arena for the call's blocks, not one for every block)
    DevArr<uint32_t> d_from, d_to; DevArr<unsigned long long> d_seq;
    if ((rc = emu_upload(from, n, d_from)) != PG_OK || (rc = emu_upload(to, n, d_to)) != PG_OK || (rc = emu_upload((const unsigned long long*)seq, n, d_seq)) != PG_OK) return rc;
    hipStream_t st = nullptr;
    if (hipStreamCreate(&st) != hipSuccess) { pg_set_error("test hook: no stream"); return PG_ENODEV; }
    std::vector<uint32_t> folded;
    unsigned long long overflow = 0;
    rc = emu_prearcs_on(d_from.p, d_to.p, d_seq.p, n, room, lanes, st, folded, &overflow);
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (rc) return rc;
    *overflow_out = overflow;
    if (overflow) { pg_set_error("pg_device_emu_prearcs: pre-arc table overflow"); return PG_ENOMEM; }
    if (folded.size() > 3 * n) { pg_set_error("pg_device_emu_prearcs: more pre-arcs than triples"); return PG_ESTATE; }
    std::copy(folded.begin(), folded.end(), out3);
    *count_out = folded.size() / 3;
    return PG_OK;
}

// pg_host_emu_clip_tips on the HipBackend: the layout is replayed on the host (host_graph.cpp: emu_tip_sets), the sets go up as a run without a
// device layout uploads them (p2_open), the tips are decided by p2_clip_tips -- the product's call of clip_tips<HipBackend, NW> -- and the node
// words come down to be held against the sequential scan's.  out[] as the host hook's.
extern "C" int pg_device_emu_clip_tips(int device, const uint64_t* records, uint64_t n_records, const uint64_t* set_last_put, int K, int mer127, int n_sets,
                                       int cut_single, int a_gb, uint64_t out[8]) {
    if ((!records && n_records) || !out || n_sets < 1 || n_sets > P2_MAX_SETS) { pg_set_error("pg_device_emu_clip_tips: bad argument"); return PG_EINVAL; }
    int rc = emu_device(device, "pg_device_emu_clip_tips");
    if (rc) return rc;
    pg::ArenaPin pin(device);                                          // (one life of the arena for the call's blocks, not one for every block)
    const int nw = mer127 ? 4 : 2;
    EmuTipSets hs;
    if ((rc = emu_tip_sets(records, n_records, set_last_put, K, nw, n_sets, cut_single, a_gb, hs)) != PG_OK) return rc;
    P2Sets sets;
    for (int s = 0; s < n_sets; s++) { sets.nodes[s] = hs.before[s].data(); sets.size[s] = hs.size[s]; }
    P2Device* d = p2_open(device, K, nw, n_sets, sets, 1);
    if (!d) return PG_ENODEV;
    P2TipTotals tot;
    rc = p2_clip_tips(d, cut_single != 0, tot);
    uint64_t diff = 0;
    std::vector<uint64_t> got;
    for (int s = 0; s < n_sets && rc == PG_OK; s++) {
        got.assign(hs.after[s].size(), 0);
        if (hs.size[s] && (rc = p2_download_set(d, s, got.data())) != PG_OK) break;
        for (uint64_t i = 0; i < hs.size[s]; i++) {
            const uint64_t at = i * (uint64_t)(nw + 1);
            if (hs.before[s][at] != P2_EMPTY) diff += got[at + nw] != hs.after[s][at + nw];      // A | B << 32 of an occupied slot
        }
    }
    p2_destroy(d);
    if (rc) return rc;
    out[0] = hs.single; out[1] = hs.minor; out[2] = tot.single; out[3] = tot.minor;
    out[4] = diff; out[5] = (uint64_t)tot.rounds; out[6] = (uint64_t)tot.cycles; out[7] = 0;
    return PG_OK;
}

}  // namespace pg
