// p2_kernels.hpp -- pass 2 of pregraph on the device: read threading and the pre-arcs (prlRead2edge, prlRead2path.c:786-1370).  Device only; a part
// of graph_kernels.hip, included there once P2Params, P2Lane and P2Device are defined (it is not a header for anybody else).
// Pass 2, one lane per read: what the reference does with a 100 M-k-mer buffer and thrd_num threads per batch
// (chopKmer4read, searchKmer, parse1read, search1kmerPlus, thread_add1preArc, recordPathBin) is one kernel:
//   * parse1read's little state machine (prlRead2path.c:598-745) runs in registers; the (K+1)-mers of branch-to-branch
//     steps are resolved on the spot in a device copy of KmerSetsPatch;
//   * a pre-arc list is ordered by the first time each target was met (new targets go to the head,
//     prlRead2path.c:388-403), so the device keeps, per (from, to), the multiplicity and the smallest sequence number
//     (read ordinal, position) in an open-addressing table; the host only sorts and prints;
//   * -R: the walk of every read goes to a row of a staging matrix (the host writes .path), the per-edge marker
//     counts are atomic adds (saturated to 255 when written).
// parse1read itself is p2_walk.hpp's (shared with the host twin), the probe of a set image graph_lookup.hpp's sv_node_word; the forms differ only in where a
// node word comes from: the set images (p2_thread_kernel<NW, false>), the lookup table (<NW, true>), the sets' owners (routed), the partition engine (ordered).
#pragma once
#include "p2_walk.hpp"

namespace pg {

template <int NW>
__device__ inline uint32_t find_patch(const P2Params& p, const Kmer<NW>& key, bool smaller) {
    uint64_t h = kmer_mix<NW>(key) & p.patch_mask;
    for (;;) {
        const uint32_t id = p.patch_val[2 * h];
        if (!id) return 0;
        const uint64_t* k = p.patch_keys + h * NW;
        bool eq = true;
#pragma unroll
        for (int i = 0; i < NW; i++) eq = eq && k[i] == key.w[i];
        if (eq) return smaller ? id : id + p.patch_val[2 * h + 1] - 1;
        h = (h + 1) & p.patch_mask;
    }
}
// the bases of a packed read one after the other: the 32-base word at hand stays in a register (read_base loads it anew for every base -- a load in
// every step of a lane's walk, 88 a read of 150 bases where 3 do)
// (P2Words: the reads are device memory; through a pointer read from a table of segments every load would be a flat load, waited for with the LDS traffic)
typedef const __attribute__((address_space(1))) uint64_t* P2Words;
struct ReadBases {
    P2Words rd;
    uint64_t w = 0;
    int wi = -1;
    __device__ __forceinline__ explicit ReadBases(P2Words r) : rd(r) {}
    __device__ __forceinline__ int at(int i) {
        if ((i >> 5) != wi) { wi = i >> 5; w = rd[wi]; }
        return (int)((w >> (62 - 2 * (i & 31))) & 3);
    }
};
// One pre-arc of one read into the lane's table (thread_add1preArc, prlRead2path.c:388-403: a multiplicity and who met it first).  Until round 6 the key,
// the multiplicity and the first meeting were three arrays -- three random lines and three atomics a call, 167 ms of p2_thread_kernel's 729 ms at 200 M
// reads (measured by leaving the calls out).  Now an entry is 32 bytes in one line: key and first meeting are read together, the multiplicity goes up with
// an atomic nobody waits for, and the minimum is only taken by a read that is earlier than what it saw (first meetings only ever go down, so a stale
// value can make a read take a minimum it need not have, never skip one it needed).
__device__ inline void add_prearc(const P2Params& p, uint32_t from, uint32_t to, unsigned long long seq) {
    const unsigned long long key = ((unsigned long long)from << 32) | to;
    uint64_t h = (key * 0x9E3779B97F4A7C15ULL) >> 20;
    h &= p.arc_mask;
    for (uint64_t step = 0; step <= p.arc_mask; step++) {
        unsigned long long* e = p.arc + h * ARC_WORDS;
        unsigned long long cur = __hip_atomic_load(&e[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long seen = __hip_atomic_load(&e[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            unsigned long long expected = 0;
            // (the distinct pairs are counted when the table is read out, p2_count_arcs: a counter bumped here would take one atomic on
            //  ONE address per new pair -- a billion of them at configs[3], at the 88 per microsecond an address serves)
            if (__hip_atomic_compare_exchange_strong(&e[0], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) cur = key;
            else cur = expected;
        }
        if (cur == key) {
            atomicAdd((unsigned int*)&e[2], 1u);
            if (seq < seen) atomicMin(&e[1], seq);
            return;
        }
        h = (h + 1) & p.arc_mask;
    }
    atomicAdd(&p.counters[2], 1ULL);
}

// ---- a lane a read (chopKmer4read + searchKmer + parse1read + search1kmerPlus + thread_add1preArc + recordPathBin) ------------------------
// The reads of a launch in an order of the caller's (round 6: p2_add_packed_device_segments): read i of the launch is read perm[i] of the reads that lie, one
// length, back to back, in segments of `per_seg` reads each (the batches pass 1 kept on the device).
struct P2Order { const uint32_t* perm; const uint64_t* const* segs; uint32_t per_seg; };
// One read of a launch: its words, its k-mers (nk = 0: past the launch's reads, or shorter than K + 1, prlRead2path.c:1103), its -R row, its sequence numbers' upper bits.
struct P2Read {
    bool in_launch;
    uint64_t r;                        // the read's place in read order: its ordinal, its row of walks
    P2Words rd;
    int len, nk;
    uint32_t* row;
    unsigned long long seq0;
    // `lane` = the read's place in the launch; `walks`: the kernels that thread zero the read's walk_len (those that only route its k-mers do not)
    __device__ __forceinline__ P2Read(const P2Params& p, const uint64_t* words, const uint64_t* word_off, const int32_t* lens, uint64_t n_reads, uint64_t first_ordinal,
                                      int uniform_len, const P2Order& order, uint64_t lane, bool walks)
        : in_launch(lane < n_reads), r(lane), rd((P2Words)words), len(0), nk(0), row(nullptr), seq0(0) {
        if (!in_launch) return;
        if (order.perm) r = (uint64_t)order.perm[lane];
        len = uniform_len ? uniform_len : lens[r];                       // (uniform_len: reads of one length back to back, no index arrays)
        if (walks && p.walk_len) p.walk_len[r] = 0;
        if (len < p.K + 1) return;                                       // prlRead2path.c:1103
        nk = len - p.K + 1;
        if (order.perm) {
            const uint32_t sg = (uint32_t)(r / order.per_seg);
            rd = (P2Words)(order.segs[sg] + (r - (uint64_t)sg * order.per_seg) * (uint64_t)((uniform_len + 31) / 32));
        } else rd = (P2Words)(words + (uniform_len ? r * (uint64_t)((uniform_len + 31) / 32) : word_off[r]));
        row = p.stage ? p.stage + r * (uint64_t)p.max_nk : nullptr;
        seq0 = (first_ordinal + r) << 16;
    }
};
constexpr P2Order p2_file_order() { return P2Order{nullptr, nullptr, 0}; }      // the reads as they lie
// the k-mers of a read one after the other, rolled: key(j) once for each of j = 0, 1, 2, ...
template <int NW>
struct P2Cursor {
    const Kmer<NW> filter;
    Kmer<NW> word, bal, ck;            // k-mer `at` as the read spells it, its reverse complement, the canonical one of the two
    bool smaller = false;              // the read spells the canonical form
    ReadBases bases;
    int K;
    __device__ __forceinline__ P2Cursor(P2Words rd, int K_) : filter(kmer_filter<NW>(K_)), bases(rd), K(K_) {
        // read_kmer takes a plain pointer: the NW + 1 words it asks for at base 0, loaded as global memory.  The last of them may lie behind the read's own:
        // every caller keeps 8 readable words behind the last read of a batch (p2_add_packed's padding, the device-resident batches' tails)
        uint64_t first[NW + 1];
#pragma unroll
        for (int i = 0; i <= NW; i++) first[i] = rd[i];
        word = read_kmer<NW>(first, 0, K, filter);
        bal = kmer_rc<NW>(word, K);
    }
    __device__ __forceinline__ const Kmer<NW>& key(int j) {
        if (j) kmer_roll<NW>(word, bal, bases.at(j + K - 1), K, filter);
        smaller = kmer_less<NW>(word, bal);
#pragma unroll
        for (int i = 0; i < NW; i++) ck.w[i] = smaller ? word.w[i] : bal.w[i];      // (word by word: a copy of `smaller ? word : bal` keeps all three in scratch memory)
        return ck;
    }
};
// where p2_walk_step's results go on the device: the (K+1)-mer patch table, the lane's pre-arc table, the read's row of the -R staging matrix
template <int NW>
struct P2Sink {
    const P2Params& p;
    uint32_t* row;
    unsigned long long seq0;
    __device__ __forceinline__ uint32_t kplus(const Kmer<NW>& key, bool smaller) const { return find_patch<NW>(p, key, smaller); }
    __device__ __forceinline__ void pair(uint32_t from, uint32_t to, int i) const {
        if (from >= p.id_end || to >= p.id_end) atomicAdd(&p.counters[5], 1ULL);
        else add_prearc(p, from, to, seq0 | (unsigned)i);
    }
    __device__ __forceinline__ void item(int i, uint32_t id) const { if (row && i < p.max_nk) row[i] = id; }
};
// One read being threaded, resumable (the ordered kernel leaves it between two tiles):
//   for (j = 0; j < nk; j++) { ab = the node word of key(j), from wherever the form has it; if (!step(ab)) break; }   end();
template <int NW>
struct P2Threader {
    const P2Params& p;
    const P2Read& read;
    P2Cursor<NW> cur;
    P2Walk<NW> w;
    bool lost = false;                 // a k-mer was not in the sets (w.stop is set with it: the read is over either way)
    __device__ __forceinline__ P2Threader(const P2Params& p_, const P2Read& read_) : p(p_), read(read_), cur(read_.rd, p_.K) {
        if (!read.nk) lost = w.stop = true;                              // nothing to thread, nothing to end
    }
    __device__ __forceinline__ bool over() const { return w.stop; }
    __device__ __forceinline__ const Kmer<NW>& key(int j) { return cur.key(j); }
    // the k-mer key() gave last has node word ab (~0: not in the sets -- the read ends without the end step, its pre-arcs stay).  false: the read is over
    __device__ __forceinline__ bool step(uint64_t ab) {
        if (ab == ~0ULL) { atomicAdd(&p.counters[1], 1ULL); lost = w.stop = true; return false; }
        P2Sink<NW> sink{p, read.row, read.seq0};
        p2_walk_step<NW>(w, cur.ck, cur.smaller, ab, p.K, sink);
        return !w.stop;
    }
    // the read is through: recordPathBin (prlRead2path.c:478-543), the walk up to the first unresolved entry if its first three are resolved
    __device__ __forceinline__ void end() {
        if (lost) return;
        const P2WalkEnd e = p2_walk_end<NW>(w);
        if (e.deleted) atomicAdd(&p.counters[0], 1ULL);
        if (!e.walk || !read.row) return;
        p.walk_len[read.r] = (uint16_t)e.walk;
        for (int i = 0; i < e.walk; i++) {
            const uint32_t id = read.row[i];
            if (id < p.id_end) atomicAdd(&p.marker[id], 1u); else atomicAdd(&p.counters[5], 1ULL);
        }
        atomicAdd(&p.counters[4], (unsigned long long)e.walk);
    }
};
// what a workgroup keeps in LDS for its lookups: the CRC-32 table sliced by four, the sets' geometry, the lane that owns every set (before a barrier)
__device__ __forceinline__ void p2_lds_crc4(uint32_t* crc4) { for (int i = threadIdx.x; i < 1024; i += 256) crc4[i] = crc32_slice_entry(i >> 8, i & 255); }
__device__ __forceinline__ void p2_lds_geo(uint64_t* set_geo, const P2Params& p) { for (int i = threadIdx.x; i < SV_GEO * (int)p.P; i += 256) set_geo[i] = p.geo3[i]; }
__device__ __forceinline__ void p2_lds_owners(uint8_t* owner_s, const uint8_t* owner_of_set, uint32_t P) { owner_s[threadIdx.x] = threadIdx.x < P ? owner_of_set[threadIdx.x] : (uint8_t)0; }
// The direct form: roll the k-mer, canonical form, set (CRC-32 sliced by four: four independent table reads a step instead of a chain of
// sixteen), home slot (key mod size by the set's precomputed reciprocal), linear probing in the set image (newhash.c:277-318; graph_lookup.hpp:
// sv_node_word) -- one random 24 / 40-byte probe in flight a lane.  With 58 registers (eight waves a SIMD) that already asks the memory system for random lines at the
// rate it serves them (23.7 G lookups/s x ~1.6 lines = 38 G lines/s, profiles/r01_membench_random_access.log); blocks of 4 / 8 k-mers
// looked up together were built and measured slower (230.9 / 304.9 ms against 222.7 per 60 M reads, profiles/r04a_p2_block_ab.csv) and are gone.
// (The reference looks every k-mer of its buffer up before it threads any read, prlRead2path.c:159-248; here a read that the state machine
// gives up is not looked up further.)
// Round 6, opt-in (SOAPDENOVO2_AMD_P2_LOOK=1): LOOK = the node word comes from pass 2's lookup table (p2_make_look) instead of the reference's set
// image.  The idea: a lookup costs the 64-byte lines it touches, and the image is not laid out for that (24-byte slots at a load of 0.64, linear
// probing from any slot); the table has every key once more in entries of 32 bytes, two a line, at a load of at most 0.5, a key's probes starting
// at the FIRST entry of its line -- and needs no set selection (CRC-32, set geometry, key mod size).  Measured at 200 M reads
// (profiles/r06_p2_lookup_ab.json): FETCH_SIZE 97 -> 94 B a lookup (90 B at a load of 0.33), kernel 730 -> 937 ms (745 ms at 0.33) + 105 ms to build
// it.  The memory side fetches ~1.5 requests a lookup whatever the alignment, and time follows the random PLACES a lookup visits, not its bytes:
// one place a lookup either way.  So the default stays the probe of the image; this form is kept for the A/B (scripts/p2_look_ab.sh).
template <int NW> constexpr int p2_look_words() { return NW == 2 ? 4 : 8; }            // words an entry
template <int NW> constexpr int p2_look_epb() { return NW == 2 ? 2 : 1; }              // entries a 64-byte bucket
template <int NW>
__device__ __forceinline__ uint64_t p2_look_home(const Kmer<NW>& ck, uint64_t n_buckets) { return __umul64hi(kmer_mix<NW>(ck), n_buckets) * p2_look_epb<NW>(); }
// occupied slots of one set image
__global__ __launch_bounds__(256) void p2_look_count(const uint64_t* __restrict__ src, int nw1, uint64_t n_slots, unsigned long long* n_keys) {
    unsigned long long mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * 256) mine += src[i * nw1] != SV_EMPTY;
    for (int o = 32; o; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_keys, mine);
}
// every key of one set image into the table (the table is all ~0 when the first set comes; nobody reads it before the last is in)
template <int NW>
__global__ __launch_bounds__(256) void p2_look_build(const uint64_t* __restrict__ src, uint64_t n_slots, unsigned long long* tab, uint64_t n_buckets) {
    constexpr int ES = p2_look_words<NW>();
    const uint64_t n_entries = n_buckets * p2_look_epb<NW>();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * 256) {
        const uint64_t* nd = src + i * (NW + 1);
        Kmer<NW> k;
        k.w[0] = nd[0];
        if (k.w[0] == SV_EMPTY) continue;
#pragma unroll
        for (int q = 1; q < NW; q++) k.w[q] = nd[q];
        const uint64_t ab = nd[NW];
        uint64_t e = p2_look_home<NW>(k, n_buckets);
        for (;;) {
            if (atomicCAS(&tab[e * ES], (unsigned long long)SV_EMPTY, (unsigned long long)k.w[0]) == SV_EMPTY) break;
            if (++e == n_entries) e = 0;
        }
#pragma unroll
        for (int q = 1; q < NW; q++) tab[e * ES + q] = k.w[q];
        tab[e * ES + NW] = ab;
    }
}
// the node word of a canonical key in the table, ~0 when the key is absent (the table has empty entries: 1.4 entries a key at the least, p2_make_look)
template <int NW>
__device__ __forceinline__ uint64_t p2_look_word(const uint64_t* look, uint64_t n_buckets, const Kmer<NW>& ck) {
    constexpr int ES = p2_look_words<NW>();
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    const uint64_t n_entries = n_buckets * p2_look_epb<NW>();
    uint64_t e = p2_look_home<NW>(ck, n_buckets);
    for (;;) {
        const uint64_t* nd = look + e * ES;                               // (entries aligned to their size: 16-byte loads)
        uint64_t d[NW + 1];
#pragma unroll
        for (int i = 0; i < NW; i += 2) {
            const u64x2 v = *(const __attribute__((address_space(1))) u64x2*)(nd + i);
            d[i] = v.x; d[i + 1] = v.y;
        }
        d[NW] = sv_word(nd + NW);
        if (d[0] == SV_EMPTY) return ~0ULL;
        bool eq = true;
#pragma unroll
        for (int i = 0; i < NW; i++) eq = eq && d[i] == ck.w[i];
        if (eq) return d[NW];
        if (++e == n_entries) e = 0;
    }
}
template <int NW, bool LOOK>
__global__ __launch_bounds__(256) void p2_thread_kernel(P2Params p, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                        const int32_t* __restrict__ lens, uint64_t n_reads, uint64_t first_ordinal, int uniform_len, P2Order order) {
    __shared__ uint32_t crc4[LOOK ? 1 : 4 * 256];
    __shared__ uint64_t set_geo[LOOK ? 1 : SV_GEO * P2_MAX_SETS];
    if constexpr (!LOOK) {
        p2_lds_crc4(crc4);
        p2_lds_geo(set_geo, p);
        __syncthreads();
    }
    const P2Read read(p, words, word_off, lens, n_reads, first_ordinal, uniform_len, order, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, true);
    if (!read.nk) return;
    P2Threader<NW> th(p, read);
    for (int j = 0; j < read.nk; j++) {
        const Kmer<NW>& ck = th.key(j);
        uint64_t ab;
        if constexpr (LOOK) ab = p2_look_word<NW>(p.look, p.look_buckets, ck);
        else ab = sv_node_word<NW>(set_geo, crc4, p.P, p.bias, ck);
        if (!th.step(ab)) break;
    }
    th.end();
}
static void p2_launch_thread_kernel(int nw, dim3 grid, hipStream_t st, const P2Params& p, const uint64_t* words, const uint64_t* word_off, const int32_t* lens,
                                    uint64_t n_reads, uint64_t first_ordinal, int uniform_len, P2Order order = p2_file_order()) {
    if (p.look) P2_LAUNCH_NW(nw, (p2_thread_kernel<NW, true>), grid, dim3(256), 0, st, p, words, word_off, lens, n_reads, first_ordinal, uniform_len, order);
    else P2_LAUNCH_NW(nw, (p2_thread_kernel<NW, false>), grid, dim3(256), 0, st, p, words, word_off, lens, n_reads, first_ordinal, uniform_len, order);
}
// a read's place in the genome, as far as a read can tell: its smallest hashed canonical 16-mer (the partition engine's m-mer hash, skm.hpp).  Reads that
// overlap share it when it lies in their overlap -- at 30 x coverage some 130 reads have the same one, and between them they look up the same few hundred k-mers.
__global__ __launch_bounds__(256) void p2_read_place_keys(const uint64_t* const* segs, uint32_t per_seg, uint64_t n_reads, int read_len, uint32_t* keys, uint32_t* idx) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t sg = (uint32_t)(r / per_seg);
    const uint64_t* rd = segs[sg] + (r - (uint64_t)sg * per_seg) * (uint64_t)((read_len + 31) / 32);
    const int m = read_len < 16 ? read_len : 16;
    uint32_t best = 0xFFFFFFFFu;
    for (int q = 0; q + m <= read_len; q++) { const uint32_t v = mmer_value(rd, q, m); best = v < best ? v : best; }
    keys[r] = best;
    idx[r] = (uint32_t)r;
}

// ---- pass 2, routed: the lookups go to the sets' owners ---------------------------------------------------------------------------------
// In a sharded run set s lives on lane s mod N, and a lane that threads a batch by probing the peer-mapped sets sends 7 of 8 probes over
// xGMI as random 64-byte reads (~10 s a GPU at configs[3] against ~1 s for the whole hash-insert path).  The reference gives
// every read one worker and every set one owner (prlRead2path.c:159-248, :248 `mixBuffer[j].low % thrd_num != id`); so does this form:
//   p2_route_hist      a lane a read: roll the k-mers, owner(k-mer) = lane of its set; per workgroup and owner, how many
//   (exclusive sum over the owner-major histogram: where every workgroup's queries for every owner start in the send buffer)
//   p2_route_scatter   roll again: the canonical k-mers (NW words each) go out grouped by owner.  A read's queries for one owner lie back to
//                      back, in read order, from starts[owner][read] on -- and so will its answers
//   (the owners pull their segments of every lane's send buffer: streamed copies, 16 / 32 bytes a lookup)
//   p2_answer_kernel   the owner probes ITS sets -- local HBM -- and writes the node words (8 bytes a lookup; ~0 = not in the sets)
//   (the lanes pull their answers back)
//   p2_thread_routed_kernel   a lane a read: roll once more (which strand is canonical; the read-oriented k-mer of a branch node), node
//                      word = the next answer of the k-mer's owner (a cursor per owner, from starts[][]), parse1read's state machine as in the
//                      direct form.  (Until round 6 scatter wrote where[k-mer] = the place of its query and this kernel read answers[where[k-mer]]:
//                      a second random 8-byte read per lookup, on the reading side; 391 ms of 36 launches at 60 M reads on three lanes.)
// Every k-mer is rolled three times and probed once, where it lives; nothing crosses xGMI but two streams.  No atomics on the way: the
// places are prefix sums, so a batch's buffers are a function of the batch.
struct P2Route {
    int n_own;
    uint32_t nblocks;
    const uint8_t* owner_of_set;                     // [P]
    uint32_t* hist;                                  // [n_own * nblocks + 1] owner-major; after the sum: first place of (owner, workgroup)
    uint64_t* send;                                  // [Q * NW]
    uint32_t* starts;                                // [n_own][nblocks * 256] where a read's queries for an owner start in the send buffer
};
template <int NW>
__device__ __forceinline__ uint32_t p2r_owner(const P2Params& p, const uint32_t* crc4, const uint8_t* owner_s, const Kmer<NW>& ck) {
    return (uint32_t)owner_s[set_of_crc(kmer_crc32_sliced<NW>(ck, crc4), p.P, p.bias)];
}
// the k-mers of a read, in read order: f(canonical k-mer, owner)
template <int NW, typename F>
__device__ __forceinline__ void p2r_for_kmers(const P2Params& p, const uint32_t* crc4, const uint8_t* owner_s, const P2Read& read, F f) {
    P2Cursor<NW> cur(read.rd, p.K);
    for (int j = 0; j < read.nk; j++) {
        const Kmer<NW>& ck = cur.key(j);
        f(ck, p2r_owner<NW>(p, crc4, owner_s, ck));
    }
}
#define P2R_PROLOGUE()                                                                                                     \
    __shared__ uint32_t crc4[4 * 256];                                                                                     \
    __shared__ uint8_t owner_s[256];                                                                                       \
    __shared__ uint32_t cnt[P2R_MAX_LANES * 256];                                                                          \
    p2_lds_crc4(crc4);                                                                                                     \
    p2_lds_owners(owner_s, ro.owner_of_set, p.P);                                                                          \
    for (int o = 0; o < ro.n_own; o++) cnt[o * 256 + threadIdx.x] = 0;                                                     \
    __syncthreads();                                                                                                       \
    const P2Read read(p, words, word_off, lens, n_reads, 0, uniform_len, p2_file_order(), (uint64_t)blockIdx.x * 256 + threadIdx.x, false)
template <int NW>
__global__ __launch_bounds__(256) void p2_route_hist(P2Params p, P2Route ro, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                     const int32_t* __restrict__ lens, uint64_t n_reads, int uniform_len) {
    P2R_PROLOGUE();
    if (read.nk) p2r_for_kmers<NW>(p, crc4, owner_s, read, [&](const Kmer<NW>&, uint32_t o) { cnt[o * 256 + threadIdx.x]++; });
    __syncthreads();
    if ((int)threadIdx.x < ro.n_own) {
        uint32_t sum = 0;
        for (int t = 0; t < 256; t++) sum += cnt[threadIdx.x * 256 + ((t + threadIdx.x) & 255)];       // (rotated: the owners' threads start in different banks)
        ro.hist[(uint64_t)threadIdx.x * ro.nblocks + blockIdx.x] = sum;
    }
}
template <int NW>
__global__ __launch_bounds__(256) void p2_route_scatter(P2Params p, P2Route ro, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                        const int32_t* __restrict__ lens, uint64_t n_reads, int uniform_len) {
    P2R_PROLOGUE();
    if (read.nk) p2r_for_kmers<NW>(p, crc4, owner_s, read, [&](const Kmer<NW>&, uint32_t o) { cnt[o * 256 + threadIdx.x]++; });
    __syncthreads();
    if ((int)threadIdx.x < ro.n_own) {                       // exclusive sum over the threads, from the place the workgroup's segment for this owner starts at
        uint32_t at = ro.hist[(uint64_t)threadIdx.x * ro.nblocks + blockIdx.x];
        for (int t = 0; t < 256; t++) { const uint32_t c = cnt[threadIdx.x * 256 + t]; cnt[threadIdx.x * 256 + t] = at; at += c; }
    }
    __syncthreads();
    for (int o = 0; o < ro.n_own; o++) ro.starts[((uint64_t)o * ro.nblocks + blockIdx.x) * 256 + threadIdx.x] = cnt[o * 256 + threadIdx.x];
    if (!read.nk) return;
    p2r_for_kmers<NW>(p, crc4, owner_s, read, [&](const Kmer<NW>& ck, uint32_t o) {
        const uint32_t at = cnt[o * 256 + threadIdx.x]++;
#pragma unroll
        for (int i = 0; i < NW; i++) ro.send[(uint64_t)at * NW + i] = ck.w[i];
    });
}
// the owner's side: n canonical k-mers, all of sets that live here
template <int NW>
__global__ __launch_bounds__(256) void p2_answer_kernel(P2Params p, const uint64_t* __restrict__ keys, uint64_t n, uint64_t* __restrict__ answers) {
    __shared__ uint32_t crc4[4 * 256];
    __shared__ uint64_t set_geo[SV_GEO * P2_MAX_SETS];
    p2_lds_crc4(crc4);
    p2_lds_geo(set_geo, p);
    __syncthreads();
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256) {
        Kmer<NW> ck;
#pragma unroll
        for (int i = 0; i < NW; i++) ck.w[i] = keys[q * NW + i];
        answers[q] = sv_node_word<NW>(set_geo, crc4, p.P, p.bias, ck);
    }
}
// The routed form's reading side: a read's answers from owner o lie back to back from ro.starts[o][read] on (the owner of a k-mer from its CRC, as in
// the scatter).
template <int NW>
__global__ __launch_bounds__(256) void p2_thread_routed_kernel(P2Params p, P2Route ro, const uint64_t* __restrict__ answers,
                                                               const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const int32_t* __restrict__ lens,
                                                               uint64_t n_reads, uint64_t first_ordinal, int uniform_len) {
    __shared__ uint32_t crc4[4 * 256];
    __shared__ uint8_t owner_s[256];
    __shared__ uint32_t cur[P2R_MAX_LANES * 256];
    p2_lds_crc4(crc4);
    p2_lds_owners(owner_s, ro.owner_of_set, p.P);
    for (int o = 0; o < ro.n_own; o++) cur[o * 256 + threadIdx.x] = ro.starts[((uint64_t)o * ro.nblocks + blockIdx.x) * 256 + threadIdx.x];
    __syncthreads();
    const P2Read read(p, words, word_off, lens, n_reads, first_ordinal, uniform_len, p2_file_order(), (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, true);
    if (!read.nk) return;
    P2Threader<NW> th(p, read);
    for (int j = 0; j < read.nk; j++) {
        const uint32_t o = p2r_owner<NW>(p, crc4, owner_s, th.key(j));
        if (!th.step(answers[cur[o * 256 + threadIdx.x]++])) break;
    }
    th.end();
}
// Pass 2 through the partitions (SOAPDENOVO2_AMD_P2_PARTITIONED=1): the answers lie in k-mer order, read r's nk of them from r x nk on (reads of one
// length).  A lane a read walking its own row visits every 64-byte line eight times with 45 KB of rows a wave between the visits -- the lines do not
// stay in L2 (419 ms per 200 M reads).  So a workgroup brings its 256 rows in through LDS, P2O_CHUNK answers a row at a time: the loads are whole
// 128-byte pieces of rows, the walk reads LDS.
constexpr int P2O_CHUNK = 16;
template <int NW>
__global__ __launch_bounds__(256) void p2_thread_ordered_kernel(P2Params p, const uint64_t* __restrict__ answers, const uint64_t* __restrict__ words,
                                                                uint64_t n_reads, uint64_t first_ordinal, int uniform_len) {
    __shared__ uint64_t tile[256 * (P2O_CHUNK + 1)];
    const uint64_t r0 = (uint64_t)blockIdx.x * 256;
    const int nk = uniform_len - p.K + 1;                                 // (the caller sees to it that the reads have K + 1 bases)
    const P2Read read(p, words, nullptr, nullptr, n_reads, first_ordinal, uniform_len, p2_file_order(), r0 + threadIdx.x, true);
    P2Threader<NW> th(p, read);
    const uint64_t rows_here = n_reads - r0 < 256 ? n_reads - r0 : 256;
    for (int c0 = 0; c0 < nk; c0 += P2O_CHUNK) {
        const int cn = nk - c0 < P2O_CHUNK ? nk - c0 : P2O_CHUNK;
        for (int i = threadIdx.x; i < 256 * P2O_CHUNK; i += 256) {
            const int rr = i / P2O_CHUNK, cc = i % P2O_CHUNK;
            if ((uint64_t)rr < rows_here && cc < cn) tile[rr * (P2O_CHUNK + 1) + cc] = answers[(r0 + rr) * (uint64_t)nk + c0 + cc];
        }
        __syncthreads();
        if (!th.over())
            for (int j = c0; j < c0 + cn; j++) {
                th.key(j);
                if (!th.step(tile[threadIdx.x * (P2O_CHUNK + 1) + (j - c0)])) break;
            }
        __syncthreads();
    }
    th.end();
}

// Pass 2's lookup table (round 6, opt-in: SOAPDENOVO2_AMD_P2_LOOK=1; the kernels, the reasoning and what was measured: above p2_thread_kernel).
// Pass 2 reads the sets and writes none of their words (parse1read, prlRead2path.c:598-745: the node words are what the edge builder left), so for
// its length every key can be entered once more, with its node word, into ONE table laid out for lookups -- when a single GPU holds all sets and
// has the room (2 entries a key; down to 1.4 when memory is short).  Same node words, same results; p2_finish releases it.
static double p2_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int p2_make_look(P2Device* d) {
    if (d->d_look || d->lanes.size() != 1) return PG_OK;
    const char* on = pg::env_user("SOAPDENOVO2_AMD_P2_LOOK");                       // opt-in: measured no faster than the probes it replaces (above p2_thread_kernel)
    if (!on || atoi(on) == 0) return PG_OK;
    for (int s = 0; s < d->P; s++) if (d->set_dev[s] != d->device) return PG_OK;
    const bool verbose = pg::env_user("PG_HOST_VERBOSE") != nullptr;
    const double t0 = p2_now();
    DevArr<unsigned long long> d_n;
    P2_HIP(d_n.alloc(1));
    P2_HIP(hipMemsetAsync(d_n.p, 0, sizeof(unsigned long long), d->stream));
    for (int s = 0; s < d->P; s++)
        hipLaunchKernelGGL(p2_look_count, dim3((unsigned)std::min<uint64_t>((d->set_sizes[s] + 255) / 256, 1u << 15)), dim3(256), 0, d->stream, d->set_ptr[s], d->nw + 1, d->set_sizes[s], d_n.p);
    unsigned long long n_keys = 0;
    P2_HIP(hipMemcpyAsync(&n_keys, d_n.p, sizeof n_keys, hipMemcpyDeviceToHost, d->stream));
    P2_HIP(hipStreamSynchronize(d->stream));
    d_n.reset();
    const int ES = d->nw == 2 ? 4 : 8, EPB = d->nw == 2 ? 2 : 1;
    size_t free_b = 0, total_b = 0;
    P2_HIP(pg::arena_mem_info(&free_b, &total_b));
    const uint64_t room = free_b > ((uint64_t)8 << 30) ? free_b - ((uint64_t)8 << 30) : 0;
    double per_key = 2.0;
    if (const char* e = pg::env_measure("PG_P2_LOOK_PER_KEY")) per_key = std::max(1.1, atof(e));   // (A/B knobs of round 6, -DPG_MEASURE library: table size, plain hipMalloc)
    const bool plain = pg::env_measure("PG_P2_LOOK_MALLOC") != nullptr;
    if ((double)n_keys * per_key * ES * 8 > (double)room) per_key = (double)room / ((double)n_keys * ES * 8 + 1);
    if (n_keys == 0 || per_key < 1.4) {
        if (verbose) fprintf(stderr, "pass 2: no lookup table (%llu keys, %.1f GB free): probing the sets as they lie\n", n_keys, free_b / 1e9);
        return PG_OK;
    }
    const uint64_t n_buckets = std::max<uint64_t>(64, (uint64_t)((double)n_keys * per_key) / EPB);
    const uint64_t bytes = n_buckets * EPB * ES * 8;
    if ((plain ? hipMalloc((void**)&d->d_look, bytes) : pg::arena_malloc((void**)&d->d_look, bytes)) != hipSuccess) { (void)hipGetLastError(); d->d_look = nullptr; return PG_OK; }
    d->look_plain = plain;
    P2_HIP(hipMemsetAsync(d->d_look, 0xFF, bytes, d->stream));
    for (int s = 0; s < d->P; s++) {
        const dim3 grid((unsigned)std::min<uint64_t>((d->set_sizes[s] + 255) / 256, 1u << 16));
        P2_LAUNCH_NW(d->nw, (p2_look_build<NW>), grid, dim3(256), 0, d->stream, d->set_ptr[s], d->set_sizes[s], (unsigned long long*)d->d_look, n_buckets);
    }
    P2_HIP(hipGetLastError());
    P2_HIP(hipStreamSynchronize(d->stream));
    d->prm.look = d->d_look; d->prm.look_buckets = n_buckets;
    if (verbose) fprintf(stderr, "pass 2: lookup table of %llu keys in %llu entries of %d bytes (%.1f GB), built in %.3fs\n", n_keys, (unsigned long long)(n_buckets * EPB), ES * 8, bytes / 1e9, p2_now() - t0);
    return PG_OK;
}
static void p2_drop_look(P2Device* d) {
    if (!d->d_look) return;
    (void)hipSetDevice(d->device);
    if (d->look_plain) (void)hipFree(d->d_look); else pg::arena_free(d->d_look);
    d->d_look = nullptr; d->prm.look = nullptr;
    for (P2Lane& ln : d->lanes) ln.prm.look = nullptr;
}
// ---- routed pass 2: one round = the batches that wait on the lanes (one each at most), all lanes working at once ---------------------------
// a lane's index rows of a batch (word offsets, lengths): room for n_reads, a quarter more when they grow -- both rows go before either comes again
static hipError_t p2_reserve_read_rows(P2Lane& ln, size_t n_reads) {
    if (n_reads > ln.d_off.n) { ln.d_off.reset(); ln.d_lens.reset(); }
    const hipError_t e = ln.d_off.reserve(n_reads, n_reads / 4);
    return e == hipSuccess ? ln.d_lens.reserve(n_reads, n_reads / 4) : e;
}
// -R: the walks of a lane's batch (its rows of the staging matrix, their lengths) on their way to the caller, behind the kernel that writes them
static int p2_download_walks(const P2Device* d, P2Lane& ln, uint64_t n_reads, uint32_t* walks_out, uint16_t* walk_len_out) {
    P2_HIP(hipMemcpyAsync(walks_out, ln.d_stage.p, n_reads * (size_t)d->max_nk * sizeof(uint32_t), hipMemcpyDeviceToHost, ln.stream));
    P2_HIP(hipMemcpyAsync(walk_len_out, ln.d_walk_len.p, n_reads * sizeof(uint16_t), hipMemcpyDeviceToHost, ln.stream));
    return PG_OK;
}
// the next lane in turn among those on `device`
static P2Lane* p2_lane_on(P2Device* d, int device) {
    for (size_t q = 0; q < d->lanes.size(); q++) {
        P2Lane& c = d->lanes[(d->next_lane + q) % d->lanes.size()];
        if (c.device == device) { d->next_lane = (unsigned)((d->next_lane + q + 1) % d->lanes.size()); return &c; }
    }
    pg_set_error("pass 2: no lane of the graph runs on the device the reads lie on");
    return nullptr;
}
// a call's reads are through (or on their way through) lane ln: the ordinal of the next read, what the lane did, back to the lead's device
static int p2_batch_done(P2Device* d, P2Lane& ln, uint64_t n_reads, uint64_t n_batches = 1) {
    d->ordinal += n_reads;
    ln.reads += n_reads; ln.batches += n_batches;
    P2_HIP(hipSetDevice(d->device));
    return PG_OK;
}
static int p2_route_round(P2Device* d) {
    const int N = (int)d->lanes.size(), nw = d->nw;
    bool any = false;
    for (P2Lane& ln : d->lanes) any = any || ln.pend.have;
    if (!any) return PG_OK;
    // A: every lane cuts its batch's lookups by owner
    for (P2Lane& ln : d->lanes) {
        if (!ln.pend.have) continue;
        P2Lane::Pending& b = ln.pend;
        P2_HIP(hipSetDevice(ln.device));
        const uint32_t nblocks = (uint32_t)((b.n_reads + 255) / 256);
        const size_t nh = (size_t)N * nblocks + 1;
        const size_t nwh = (size_t)N * nblocks * 256, nq = (size_t)b.q, nk = nq * nw;      // (the lane's buffers of the rounds grow by a quarter more than asked)
        P2_HIP(ln.hist_in.reserve(nh, nh / 4 + 64));
        P2_HIP(ln.hist.reserve(nh, nh / 4 + 64));
        P2_HIP(ln.where.reserve(nwh, nwh / 4 + 64));
        P2_HIP(ln.ans.reserve(nq, nq / 4 + 64));
        P2_HIP(ln.send.reserve(nk, nk / 4 + 64));
        P2Route ro{N, nblocks, ln.d_owner_of_set, ln.hist_in.p, ln.send.p, ln.where.p};
        const dim3 grid(nblocks), block(256);
        P2_HIP(hipMemsetAsync(ln.hist_in.p + (nh - 1), 0, sizeof(uint32_t), ln.stream));
        P2_LAUNCH_NW(nw, (p2_route_hist<NW>), grid, block, 0, ln.stream, ln.prm, ro, b.d_words, b.d_off, b.d_lens, b.n_reads, b.uniform_len);
        P2_HIP(hipGetLastError());
        const size_t need = dev_exclusive_sum_bytes(ln.hist_in.p, ln.hist.p, nh, ln.stream);
        P2_HIP(ln.scan_tmp.reserve(need, need / 4 + 64));
        P2_HIP(dev_exclusive_sum(ln.scan_tmp, ln.hist_in.p, ln.hist.p, nh, ln.stream));
        ro.hist = ln.hist.p;
        P2_LAUNCH_NW(nw, (p2_route_scatter<NW>), grid, block, 0, ln.stream, ln.prm, ro, b.d_words, b.d_off, b.d_lens, b.n_reads, b.uniform_len);
        P2_HIP(hipGetLastError());
        // the owners' segments start at hist[o * nblocks]; the total behind the last
        for (int o = 0; o <= N; o++) P2_HIP(hipMemcpyAsync(ln.h_starts + o, ln.hist.p + (size_t)o * nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, ln.stream));
    }
    for (P2Lane& ln : d->lanes) if (ln.pend.have) { P2_HIP(hipSetDevice(ln.device)); P2_HIP(hipStreamSynchronize(ln.stream)); }
    // who sends how much to whom
    std::vector<uint64_t> cnt((size_t)N * N, 0), recv_off((size_t)N * N, 0), recv_total(N, 0);
    for (int l = 0; l < N; l++) {
        P2Lane& ln = d->lanes[l];
        if (!ln.pend.have) continue;
        if (ln.h_starts[N] != ln.pend.q) { pg_set_error("pass 2 (routed): a batch's lookups do not add up"); return PG_EINVAL; }
        for (int o = 0; o < N; o++) cnt[(size_t)l * N + o] = (uint64_t)ln.h_starts[o + 1] - ln.h_starts[o];
    }
    for (int o = 0; o < N; o++)
        for (int l = 0; l < N; l++) { recv_off[(size_t)o * N + l] = recv_total[o]; recv_total[o] += cnt[(size_t)l * N + o]; }
    // B: the owners pull their segments and answer
    for (int o = 0; o < N; o++) {
        P2Lane& ow = d->lanes[o];
        if (!recv_total[o]) continue;
        P2_HIP(hipSetDevice(ow.device));
        const size_t na = (size_t)recv_total[o], nk = na * nw;
        P2_HIP(ow.rans.reserve(na, na / 4 + 64));
        P2_HIP(ow.rkeys.reserve(nk, nk / 4 + 64));
        for (int l = 0; l < N; l++) {
            const uint64_t c = cnt[(size_t)l * N + o];
            if (!c) continue;
            P2Lane& ln = d->lanes[l];
            P2_HIP(p2r_copy(ow.rkeys.p + recv_off[(size_t)o * N + l] * nw, ow.device, ln.send.p + (uint64_t)ln.h_starts[o] * nw, ln.device, c * nw * sizeof(uint64_t), ow.stream));
            ln.lookups_sent += c;
            if (l != o) ln.lookups_sent_away += c;
        }
        // (a workgroup builds the CRC table and the set geometry in LDS before its first probe: a few thousand workgroups that stride over the keys, not one per 256 keys --
        //  36 launches of 147 M keys took 509 ms with half a million workgroups each, profiles/r05n_kernel_stats_cli_60M_sh3_routed.csv)
        const dim3 grid((unsigned)std::min<uint64_t>((recv_total[o] + 255) / 256, 256u * 16u)), block(256);
        P2_LAUNCH_NW(nw, (p2_answer_kernel<NW>), grid, block, 0, ow.stream, ow.prm, ow.rkeys.p, recv_total[o], ow.rans.p);
        P2_HIP(hipGetLastError());
        ow.lookups_answered += recv_total[o];
    }
    for (int o = 0; o < N; o++) if (recv_total[o]) { P2_HIP(hipSetDevice(d->lanes[o].device)); P2_HIP(hipStreamSynchronize(d->lanes[o].stream)); }
    // C: the answers go home, the lanes thread their reads
    for (int l = 0; l < N; l++) {
        P2Lane& ln = d->lanes[l];
        if (!ln.pend.have) continue;
        P2Lane::Pending& b = ln.pend;
        P2_HIP(hipSetDevice(ln.device));
        for (int o = 0; o < N; o++) {
            const uint64_t c = cnt[(size_t)l * N + o];
            if (c) P2_HIP(p2r_copy(ln.ans.p + ln.h_starts[o], ln.device, d->lanes[o].rans.p + recv_off[(size_t)o * N + l], d->lanes[o].device, c * sizeof(uint64_t), ln.stream));
        }
        P2Params p = ln.prm;
        p.stage = d->reps ? ln.d_stage.p : nullptr;
        p.walk_len = d->reps ? ln.d_walk_len.p : nullptr;
        const uint32_t nblocks = (uint32_t)((b.n_reads + 255) / 256);
        const dim3 grid(nblocks), block(256);
        const P2Route ro{N, nblocks, ln.d_owner_of_set, nullptr, nullptr, ln.where.p};
        P2_LAUNCH_NW(nw, (p2_thread_routed_kernel<NW>), grid, block, 0, ln.stream, p, ro, ln.ans.p, b.d_words, b.d_off, b.d_lens, b.n_reads, b.ordinal, b.uniform_len);
        P2_HIP(hipGetLastError());
        if (d->reps && b.walks_out && b.walk_len_out) { const int rc = p2_download_walks(d, ln, b.n_reads, b.walks_out, b.walk_len_out); if (rc) return rc; }
        ln.route_rounds++;
    }
    // (the owners' answer buffers are read by the lanes' copies: everybody is through before the next round writes them)
    for (P2Lane& ln : d->lanes) if (ln.pend.have) { P2_HIP(hipSetDevice(ln.device)); P2_HIP(hipStreamSynchronize(ln.stream)); ln.pend.have = false; }
    P2_HIP(hipSetDevice(d->device));
    return PG_OK;
}
// a batch is in a lane's buffers: thread it now (the direct form), or let it wait for the round (the routed form)
static int p2_batch_ready(P2Device* d, P2Lane& ln, const uint64_t* d_words, const uint64_t* d_off, const int32_t* d_lens, uint64_t n_reads, uint64_t q, int uniform_len,
                          uint32_t* walks_out, uint16_t* walk_len_out, bool round_now) {
    if (!d->route) {
        P2Params p = ln.prm;
        p.stage = d->reps && !uniform_len ? ln.d_stage.p : nullptr;
        p.walk_len = d->reps && !uniform_len ? ln.d_walk_len.p : nullptr;
        const dim3 grid((unsigned)((n_reads + 255) / 256));
        p2_launch_thread_kernel(d->nw, grid, ln.stream, p, d_words, d_off, d_lens, n_reads, d->ordinal, uniform_len);
        P2_HIP(hipGetLastError());
        return PG_OK;
    }
    if (q >= 0xFFFFFFFFull) { pg_set_error("pass 2 (routed): more than 2^32 k-mers in one batch"); return PG_EINVAL; }
    if (ln.pend.have) { const int rc = p2_route_round(d); if (rc) return rc; P2_HIP(hipSetDevice(ln.device)); }
    ln.pend.have = true;
    ln.pend.d_words = d_words; ln.pend.d_off = d_off; ln.pend.d_lens = d_lens;
    ln.pend.n_reads = n_reads; ln.pend.ordinal = d->ordinal; ln.pend.q = q; ln.pend.uniform_len = uniform_len;
    ln.pend.walks_out = walks_out; ln.pend.walk_len_out = walk_len_out;
    bool all = true;
    for (const P2Lane& o : d->lanes) all = all && o.pend.have;
    if (all || round_now) return p2_route_round(d);
    return PG_OK;
}

// One batch of reads goes to the next lane in turn.  Without -R the call returns as soon as the batch has left the host buffers
// (the lane threads it while the caller fetches the next batch for the next lane); with -R the walks come back, so it waits.
int p2_add_packed(P2Device* d, const uint64_t* words, const uint64_t* word_off, const int32_t* lens, uint64_t n_reads, uint64_t n_words,
                  uint32_t* walks_out, uint16_t* walk_len_out) {
    if (!d->reads_ready) { pg_set_error("pass 2: p2_begin_reads was not called"); return PG_ESTATE; }
    if (!n_reads) return PG_OK;
    P2Lane& ln = d->lanes[d->next_lane++ % d->lanes.size()];
    if (d->route && ln.pend.have) { const int rc = p2_route_round(d); if (rc) return rc; }      // (its buffers still hold a batch that waits for its round)
    P2_HIP(hipSetDevice(ln.device));
    const size_t nwp = n_words + 8, nst = d->reps ? (size_t)n_reads : 0;
    if (nwp > ln.d_words.n || n_reads > ln.d_off.n || nst > ln.d_walk_len.n) P2_HIP(hipStreamSynchronize(ln.stream));   // nobody reads the buffers that go
    // (words and index rows grow by a quarter more than asked, the -R rows to the batch; a pair of rows goes before either comes again)
    P2_HIP(ln.d_words.reserve(nwp, nwp / 4));
    P2_HIP(p2_reserve_read_rows(ln, n_reads));
    if (nst > ln.d_walk_len.n) { ln.d_stage.reset(); ln.d_walk_len.reset(); }
    if (d->reps) { P2_HIP(ln.d_stage.reserve(nst * (size_t)d->max_nk, 0)); P2_HIP(ln.d_walk_len.reserve(nst, 0)); }
    // (the copies are ordered behind the lane's previous batch by its stream: that batch read the same buffers)
    P2_HIP(hipMemcpyAsync(ln.d_words.p, words, n_words * sizeof(uint64_t), hipMemcpyHostToDevice, ln.stream));
    P2_HIP(hipMemsetAsync(ln.d_words.p + n_words, 0, 8 * sizeof(uint64_t), ln.stream));      // readable padding for the window loads
    P2_HIP(hipMemcpyAsync(ln.d_off.p, word_off, n_reads * sizeof(uint64_t), hipMemcpyHostToDevice, ln.stream));
    P2_HIP(hipMemcpyAsync(ln.d_lens.p, lens, n_reads * sizeof(int32_t), hipMemcpyHostToDevice, ln.stream));
    uint64_t q = 0;
    if (d->route)                                                     // the lookups the batch asks for (prlRead2path.c:1103: reads shorter than K + 1 have none)
        for (uint64_t r = 0; r < n_reads; r++) if (lens[r] >= d->K + 1) q += (uint64_t)(lens[r] - d->K + 1);
    P2_HIP(hipEventRecord(ln.copied, ln.stream));
    // (-R: the walks come back with the call, so a routed batch does not wait for the other lanes' batches)
    { const int rc = p2_batch_ready(d, ln, ln.d_words.p, ln.d_off.p, ln.d_lens.p, n_reads, q, 0, walks_out, walk_len_out, d->reps); if (rc) return rc; }
    if (d->route) { P2_HIP(hipSetDevice(ln.device)); P2_HIP(hipEventSynchronize(ln.copied)); }
    else if (d->reps && walks_out && walk_len_out) {
        const int rc = p2_download_walks(d, ln, n_reads, walks_out, walk_len_out);
        if (rc) return rc;
        P2_HIP(hipStreamSynchronize(ln.stream));
    } else P2_HIP(hipEventSynchronize(ln.copied));                 // the caller's buffers are its own again
    return p2_batch_done(d, ln, n_reads);
}

// the same for reads that lie on a lane's device already (pass 1 left them there): n_reads reads of read_len bases, packed back to
// back, 8 readable words behind the last; no -R walks on this path.  Calls arrive in read order (the ordinal is the call order).
int p2_add_packed_device(P2Device* d, const uint64_t* d_words, uint64_t n_reads, int read_len, int device) {
    if (!d->reads_ready) { pg_set_error("pass 2: p2_begin_reads was not called"); return PG_ESTATE; }
    if (d->reps) { pg_set_error("pass 2: device-resident reads are not for -R runs"); return PG_ESTATE; }
    if (!n_reads) return PG_OK;
    if (read_len < 1 || !d_words) { pg_set_error("pass 2: bad argument"); return PG_EINVAL; }
    P2Lane* ln = p2_lane_on(d, device);
    if (!ln) return PG_EINVAL;
    P2_HIP(hipSetDevice(ln->device));
    // (the caller may release the reads when the call returns: a routed batch has its round at once)
    { const int rc = p2_batch_ready(d, *ln, d_words, nullptr, nullptr, n_reads, read_len >= d->K + 1 ? n_reads * (uint64_t)(read_len - d->K + 1) : 0, read_len, nullptr, nullptr, true); if (rc) return rc; }
    P2_HIP(hipSetDevice(ln->device));
    P2_HIP(hipStreamSynchronize(ln->stream));
    return p2_batch_done(d, *ln, n_reads);
}

// All of them at once, in GENOME order as far as a read can tell (round 6).  Pass 2 is bound by the random lines its lookups ask HBM for: 17.6 G lookups x 1.6
// lines at 200 M reads, every one of them somewhere else in 45 GB of k-mer sets, because reads come in file order.  But nothing of pass 2 depends on the order
// reads are threaded in -- a pre-arc carries the ordinal of the read that met it first, a read's walk goes to its own row -- so the reads are threaded sorted by
// their smallest hashed 16-mer (p2_read_place_keys): a workgroup's 256 reads then come from two or three places of the genome and ask for the same few hundred
// k-mers, which the L2 serves.  n_segs segments of per_seg reads each (the last may hold fewer), one length, on `device`.
int p2_add_packed_device_segments(P2Device* d, const uint64_t* const* d_segs, const uint64_t* seg_reads, int n_segs, int read_len, int device) {
    if (!d->reads_ready) { pg_set_error("pass 2: p2_begin_reads was not called"); return PG_ESTATE; }
    if (n_segs < 1 || !d_segs || !seg_reads || read_len < 1) { pg_set_error("pass 2: bad argument"); return PG_EINVAL; }
    uint64_t total = 0;
    bool even = true;
    for (int q = 0; q < n_segs; q++) { total += seg_reads[q]; even = even && (q == n_segs - 1 ? seg_reads[q] <= seg_reads[0] : seg_reads[q] == seg_reads[0]) && seg_reads[q] > 0; }
    // NOT the default (SOAPDENOVO2_AMD_P2_SORT=1 asks for it): measured at 200 M reads, p2_thread_kernel 666 ms in one sorted launch against 720 ms in 120 launches in file
    // order, + 61 ms for the keys + the sort -- nothing gained (profiles/r06_p2_genome_order_ab.json).  The lanes of a workgroup meet a shared k-mer up to 135 steps apart, a
    // millisecond at this kernel's pace, and an XCD's 4 MB of L2 turn over every 12 us under the misses of everybody else: the reuse is there, not the residency.
    const char* sw = pg::env_user("SOAPDENOVO2_AMD_P2_SORT");
    const bool sorted = sw && atoi(sw) != 0 && even && total < 0xFFFFFFFFull && total >= 4096 && d->lanes.size() == 1 && !d->route && !d->reps &&
                        d->lanes[0].device == device && read_len >= d->K + 1 && seg_reads[0] < 0xFFFFFFFFull;
    // SOAPDENOVO2_AMD_P2_PARTITIONED=1 (round 6, opt-in): the lookups through the partition engine -- the reads cut into super-k-mer records once more, every distinct
    // k-mer of a partition looked up ONCE (partition_kernels.hip: skm_answer_kernel), the reads threaded over the answers in k-mer order.  Rounds of as many
    // segments as 40 GB of answers (8 bytes a k-mer occurrence) hold.
    const char* pw = pg::env_user("SOAPDENOVO2_AMD_P2_PARTITIONED");
    if (pw && atoi(pw) != 0 && even && total < 0xFFFFFFFFull && d->lanes.size() == 1 && !d->route && !d->reps && d->lanes[0].device == device && read_len >= d->K + 1) {
        P2Lane& ln = d->lanes[0];
        P2_HIP(hipSetDevice(ln.device));
        p2_drop_look(d);                                  // (this form does not read the lookup table: its room goes to the answers)
        hipStream_t st = ln.stream;
        const uint64_t kpr = (uint64_t)(read_len - d->K + 1), per_seg = seg_reads[0];
        uint64_t ans_gb = 40;
        if (const char* e = pg::env_measure("PG_P2_PART_GB")) ans_gb = (uint64_t)std::max(1, atoi(e));   // (A/B knob, -DPG_MEASURE library)
        uint64_t segs_a_round = std::max<uint64_t>(1, ((ans_gb << 30) / 8) / std::max<uint64_t>(1, per_seg * kpr));
        segs_a_round = std::min<uint64_t>(segs_a_round, (uint64_t)n_segs);
        const uint64_t reads_round = segs_a_round * per_seg;
        pg_ctx* ctx = pg_create_planned(ln.device, d->K, d->nw == 4 ? 1 : 0, d->P, 24, 2, reads_round * kpr, reads_round, 1, 1);
        if (!ctx) return PG_ENOMEM;
        unsigned long long* d_ans = nullptr;
        int rc = PG_OK;
        if (pg::arena_malloc((void**)&d_ans, reads_round * kpr * sizeof(unsigned long long)) != hipSuccess) { pg_destroy(ctx); pg_set_error("pass 2 through the partitions: no memory for the answers"); return PG_ENOMEM; }
        uint64_t g_first = 0;                                           // the round's first read among all
        for (int q0 = 0; q0 < n_segs && rc == PG_OK; q0 += (int)segs_a_round) {
            const int q1 = std::min(n_segs, q0 + (int)segs_a_round);
            if (q0 && pg_reset(ctx, st) != PG_OK) { rc = PG_ENODEV; break; }
            uint64_t local = 0;
            for (int q = q0; q < q1 && rc == PG_OK; q++) {
                if (pg_count_reads(ctx, d_segs[q], nullptr, nullptr, seg_reads[q], (uint32_t)read_len, seg_reads[q] * kpr, local * kpr, st) != PG_OK) rc = PG_ENODEV;
                local += seg_reads[q];
            }
            if (rc == PG_OK) rc = pg::e2_answer(ctx, ln.prm.geo3, (uint32_t)d->P, ln.prm.bias, d_ans, 0, st);
            if (rc == PG_OK) rc = pg::e2_answer_check(ctx, st);
            local = 0;
            for (int q = q0; q < q1 && rc == PG_OK; q++) {
                P2Params p = ln.prm;
                p.stage = nullptr; p.walk_len = nullptr;
                const dim3 grid((unsigned)((seg_reads[q] + 255) / 256)), block(256);
                P2_LAUNCH_NW(d->nw, (p2_thread_ordered_kernel<NW>), grid, block, 0, st, p, (const uint64_t*)(d_ans + local * kpr), d_segs[q], seg_reads[q], d->ordinal + g_first + local, read_len);
                if (hipGetLastError() != hipSuccess) { pg_set_error("pass 2 through the partitions: launch failed"); rc = PG_ENODEV; }
                local += seg_reads[q];
            }
            if (hipStreamSynchronize(st) != hipSuccess && rc == PG_OK) { pg_set_error("pass 2 through the partitions: a kernel failed"); rc = PG_ENODEV; }
            g_first += local;
        }
        pg::arena_free(d_ans);
        pg_destroy(ctx);
        if (rc) return rc;
        if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "pass 2: %llu read(s) through the partition engine, %llu segment(s) a round\n", (unsigned long long)total, (unsigned long long)segs_a_round);
        return p2_batch_done(d, ln, total, (uint64_t)n_segs);
    }
    if (!sorted) {                                                  // segment by segment, in file order (the round-5 form; also what several lanes take)
        for (int q = 0; q < n_segs; q++) { const int rc = p2_add_packed_device(d, d_segs[q], seg_reads[q], read_len, device); if (rc) return rc; }
        return PG_OK;
    }
    P2Lane& ln = d->lanes[0];
    P2BackOn back{d->device};
    P2_HIP(hipSetDevice(ln.device));
    DevArr<const uint64_t*> table;                                  // (on the lane's device, all of them)
    DevArr<uint32_t> keys, keys2, idx, perm;
    DevArr<unsigned char> tmp;
    hipStream_t st = ln.stream;
    const unsigned grid = (unsigned)((total + 255) / 256);
    EB_HIP(table.alloc((size_t)n_segs));
    EB_HIP(hipMemcpyAsync(table.p, d_segs, (size_t)n_segs * sizeof(uint64_t*), hipMemcpyHostToDevice, st));
    EB_HIP(keys.alloc(total)); EB_HIP(keys2.alloc(total));
    EB_HIP(idx.alloc(total)); EB_HIP(perm.alloc(total));
    EB_HIP(tmp.alloc(dev_sort_pairs_bytes(keys.p, keys2.p, idx.p, perm.p, (size_t)total, 32u, st)));
    hipLaunchKernelGGL(p2_read_place_keys, dim3(grid), dim3(256), 0, st, (const uint64_t* const*)table.p, (uint32_t)seg_reads[0], total, read_len, keys.p, idx.p);
    EB_HIP(hipGetLastError());
    EB_HIP(dev_sort_pairs(tmp, keys.p, keys2.p, idx.p, perm.p, (size_t)total, 32u, st));
    {
        P2Params p = ln.prm;
        p.stage = nullptr; p.walk_len = nullptr;
        p2_launch_thread_kernel(d->nw, dim3(grid), st, p, nullptr, nullptr, nullptr, total, d->ordinal, read_len, P2Order{perm.p, (const uint64_t* const*)table.p, (uint32_t)seg_reads[0]});
        EB_HIP(hipGetLastError());
    }
    EB_HIP(hipStreamSynchronize(st));
    if (pg::env_user("PG_HOST_VERBOSE")) fprintf(stderr, "pass 2: %llu read(s) of %d segment(s) threaded in one launch, sorted by their smallest hashed 16-mer\n", (unsigned long long)total, n_segs);
    return p2_batch_done(d, ln, total, (uint64_t)n_segs);
}

// ... and for reads of ANY mix of lengths that pass 1 left on the device with their index arrays (the ragged batches of
// pg_count_reads: d_word_off[n_reads], d_kmer_base[n_reads + 1], every read >= K + 1 bases): the lengths pass 2's kernels want come from
// kmer_base on the device, nothing goes through the host.
__global__ __launch_bounds__(256) void p2_lens_from_kbase(const uint64_t* __restrict__ kbase, uint64_t n_reads, int K, int32_t* __restrict__ lens) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n_reads) lens[r] = (int32_t)(kbase[r + 1] - kbase[r]) + K - 1;
}
int p2_add_packed_device_ragged(P2Device* d, const uint64_t* d_words, const uint64_t* d_word_off, const uint64_t* d_kmer_base, uint64_t n_reads, uint64_t n_kmers, int device) {
    if (!d->reads_ready) { pg_set_error("pass 2: p2_begin_reads was not called"); return PG_ESTATE; }
    if (d->reps) { pg_set_error("pass 2: device-resident reads are not for -R runs"); return PG_ESTATE; }
    if (!n_reads) return PG_OK;
    if (!d_words || !d_word_off || !d_kmer_base) { pg_set_error("pass 2: bad argument"); return PG_EINVAL; }
    P2Lane* ln = p2_lane_on(d, device);
    if (!ln) return PG_EINVAL;
    if (d->route && ln->pend.have) { const int rc = p2_route_round(d); if (rc) return rc; }      // (its length row still serves a batch that waits for its round)
    P2_HIP(hipSetDevice(ln->device));
    if (n_reads > ln->d_off.n) P2_HIP(hipStreamSynchronize(ln->stream));
    P2_HIP(p2_reserve_read_rows(*ln, n_reads));
    hipLaunchKernelGGL(p2_lens_from_kbase, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, ln->stream, d_kmer_base, n_reads, d->K, ln->d_lens.p);
    P2_HIP(hipGetLastError());
    { const int rc = p2_batch_ready(d, *ln, d_words, d_word_off, ln->d_lens.p, n_reads, n_kmers, 0, nullptr, nullptr, true); if (rc) return rc; }
    P2_HIP(hipSetDevice(ln->device));
    P2_HIP(hipStreamSynchronize(ln->stream));
    return p2_batch_done(d, *ln, n_reads);
}

}  // namespace pg
