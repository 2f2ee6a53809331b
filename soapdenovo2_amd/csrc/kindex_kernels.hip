// kindex_kernels.hip -- the k-mer index on the GPU (kindex.hpp: layout, sequence rules, the shared read side).
//
//   kidx_build_kernel       a lane per record of a device array in export format ((NW + 2) words a record, any order: what pg_export,
//                           pg_export_peek, pg_export_take and pg_sort_records leave), for rank `me` of n: the records it owns
//                           (map_owner); n == 1, pg_kindex_build's table and a one-rank cut alike, skips the owner under that
//                           launch-uniform condition.  The protocol is map_index_kernel's
//                           (map_kernels.hip): a new key is claimed with a CAS on its state word, key and value are written, and the
//                           state is published with a release store; a lane that meets a claimed slot looks at the same slot again on its
//                           next trip round the loop -- nobody waits inside a branch for a lane of its own wavefront.  The trips spent on
//                           one claimed slot are capped (KIDX_SPIN_CAP): a lane that gives up raises KIDX_FLAG_SPIN and the build fails
//                           with PG_ESPIN.  The keys are distinct by contract: a lane that meets its own key published raises
//                           KIDX_FLAG_DUP, leaves the slot as it is, and the build fails with PG_EINVAL.  A record the -d filter deleted
//                           (kidx_stored, kindex.hpp) is passed over.
//   kidx_query_kernel       <NW, WAVE>, an index in one table.  The lane form: a lane per sequence, for read-sized sequences:
//                           kidx_stretch over the whole sequence, the summary in registers.  The wave form: a wavefront per sequence,
//                           four sequences a 256-thread workgroup, for contig-sized sequences: lane l takes ceil(nk / 64) consecutive
//                           k-mers (kidx_wave_split: one read_kmer, then rolling), the summary through a __shfl_xor butterfly
//                           (kidx_summary_wave_reduce), lane 0 writes it.  No LDS, no workgroup barrier: a wave without a sequence
//                           just ends.
//   kcor_kernel             a lane per read of a batch that already lies in the output buffer: kcor_read (kcorrect.hpp) on the lane's own
//                           words, in global memory -- the first pass over the read as given is the query kernel's lane walk, and a read
//                           without a weak k-mer ends there; the lanes of a wave diverge in the trials.
//   kwalk_kernel            a lane per walk, two walks a sequence (kwalk.hpp; pg_kindex_walk): kwalk_one with kidx_find as its
//                           lookup.  One dependent slot read per appended base, latency-chained within the lane; the word of 32 bases
//                           being filled stays in a register and is stored when full.  No LDS, no barrier; lanes whose walks ended wait
//                           for the longest walk of their wave.
// What the operators below share:
//   the graph step and the base writer   kwalk.hpp: kwalk_step over a KwalkNode and KwalkText, PG_HD code for the walk and the unitigs,
//                              the kernels and the host twins; the lookup is a lambda find(ck, slot&) -- kidx_find for the walk, which
//                              leaves the slot alone, kunitig_probe for the unitigs
//   the scan                   here, for the trim and the unitigs: KidxCounts (kindex.hpp) an item, blocks of 256 items.  kidx_block_scan
//                              (a workgroup's inclusive scan: __shfl_up inside a wave, the four waves' sums through LDS) and the bodies of
//                              the three kernels a scan takes: kidx_block_sums (a workgroup's sums), kidx_scan_block_sums (one workgroup:
//                              the blocks' sums scanned in place, 256 a round with the carry in registers; the totals) and
//                              kidx_scan_before (the scan inside a workgroup again: what the items before a lane add up to).  Each
//                              operator's kernels add where a lane's counts come from and what is done with the offsets
//   the scratch                KidxScratch (kindex.hpp), one each for the trim, the corrector on a cut index and the unitigs:
//                              kidx_scratch_begin / _end / _free.  kidx_settled is the one way out of an entry point over the ranks
//   the scratch of ix->uni     for the unitigs by walking, by list ranking and an edit round: laid out once, by kunitig_plan
//                              (kunitig.hpp: word offsets and the total from keys, slots and the kind), bound by kunitig_bind and
//                              krank_bind; kunitig_call_begin is what the three drivers begin with (device, plan, the two grids with
//                              their refusals, kidx_scratch_begin, the leading words and the walk's covered bits zeroed), kunitig_scan
//                              the scan's two launches of both engines
//   the finish                 kunitig_finish and kunitig_finish_tail (kunitig.hpp): the eight totals, the go decision, the last
//                              offsets and the tail's zero words, for kunitig_scan_sums_kernel's thread 0 and both host twins
//   a published slot's word    kidx_published_word: 0 past the table or where the slot is empty; the ends, number and sweep kernels
// The index cut over ranks (kindex.hpp; pg_kindex_build_sharded, pg_kindex_query_words):
//   kidx_count_owners_kernel   a lane per record of a device part, on the device where the part lies: the owners of all n ranks at once
//                              into an LDS histogram (n <= 256 bins: 1 KB, zeroed and flushed per workgroup), one global atomicAdd per
//                              non-zero bin per workgroup.  Deleted records are counted: owned_i sizes the table as pg_kindex_build does.
//   kidx_probe_owned_kernel    the lane and wave splits of the query kernel; an owned canonical k-mer's answer goes into the rank's
//                              zeroed rows, every other word is left as it is.  No summary.
//   kidx_summary_rows_kernel   a wavefront per sequence, four a workgroup, over the merged rows: lanes stride the row (j = lane, lane + 64,
//                              ...: coalesced), the query kernel's butterfly, lane 0 stores.  Sums and minima: the same words.
// The merge is map_rows_merge_kernel (map_kernels.hip, through map_rows_merge).
// The trim (ktrim.hpp; pg_kindex_trim):
//   ktrim_span_kernel          a lane per read: kidx_query_kernel's walk and launch shape, the current and the best run of solid k-mers in
//                              registers (ktrim_span_probe), one span word stored.  The span word is all the scan wants of a read: kept,
//                              output words and output k-mers are ktrim_counts of it
//   ktrim_span_rows_kernel     the same tracker over a read's row of merged answers (an index cut over ranks), no probe
//   the scan                   over ktrim_counts of the span words: ktrim_block_sums_kernel, ktrim_scan_sums_kernel (the totals,
//                              kmer_base_out's last entry), ktrim_scatter_kernel (every kept read's word_off_out, kmer_base_out and
//                              src_out)
//   ktrim_pack_kernel          a lane per output word, the tail's nw + 1 zero words included: the kept read by binary search in
//                              word_off_out, the word by ktrim_pack_word.  The launch covers the batch's n_words, which the result never
//                              passes; how many of those lanes have a word is read from the totals on the device
// The unitigs (kunitig.hpp; pg_kindex_unitigs): the whole graph compacted, six launches on the caller's stream
//   kunitig_ends_kernel        a lane per table slot: both sides of a published solid key tested (kunitig_ends, two lookups at most), every
//                              end side appended to the start list through an atomic counter; the solid k-mers counted a wave at a time
//   kunitig_measure_kernel     a lane per start: kunitig_chain to the far end with a covered bit a k-mer on the way (atomicOr on 32-bit
//                              words), the length, or 0 for the copy the orientation rule does not emit
//   kunitig_rings_kernel       a lane per slot, solid and not covered: the cyclic form of kunitig_chain, which ends at the first smaller
//                              key; a ring's least member appends its start behind the chains' -- one scan and one write serve both
//   the scan                   over kunitig_counts (kept, words, k-mers) of the starts: kunitig_block_sums_kernel and
//                              kunitig_scan_sums_kernel (the totals, the overflow decision the write kernel obeys, the last offsets and
//                              the tail's zero words)
//   kunitig_write_kernel       a lane per start: its offsets from the scan, and a kept start walks once more into its row
// The unitigs by list ranking (krank.hpp; pg_kindex_unitigs_ranked): the same unitigs, a chain of n k-mers in ceil(log2 n)
// rounds over all k-mers instead of n dependent lookups of one lane; 3 R + 7 launches (R = krank_rounds(keys)), 3 more in full mode
//   krank_number_kernel        a workgroup per 4 096 slots: a solid key takes a node id, one atomicAdd a workgroup
//   krank_sweep_kernel         a lane per slot: kunitig_side on both sides (the ends kernel's two lookups); an end side becomes an end
//                              record and a start, an open one a link to its successor
// Every pass over the nodes is krank.hpp's: its launch-uniform decision (krank_*_pass), its item body (krank_*_item) and what it leaves
// in the control words (krank_*_done); a kernel adds the grid-stride loop, the host twin a plain one.  No control word is named here
//   krank_jump_kernel          round j over the oriented nodes, a grid of at most 4 096 workgroups striding them: krank_jump from the
//                              generation the control words name into the other; a round behind one in which no record became done ends
//                              after one read a workgroup
//   krank_ring_init_kernel, krank_min_kernel, krank_ring_cut_kernel   what is not done lies on a ring: the least canonical key of each
//                              directed ring by windows that double, the ring cut there into a chain, its least member appended to the
//                              starts; then the jump rounds again.  All but the first end at once when there is no ring
//   krank_measure_kernel       a lane per start: length and far end from its record, the orientation rule; then the unitigs' scan
//   krank_zero_kernel, krank_place_kernel, krank_emit_kernel   full mode: the rows zeroed, a lane per start (offsets, report words, a
//                              place record at the start's node), a lane per k-mer (its base ORed into its row at its rank)
// The operators that edit the graph (kedit.hpp): one round of an operator Op, four launches on the caller's stream over the
// unitigs' scratch
//   kunitig_ends_kernel        as above: the start list and the solid count
//   kedit_decide_kernel<Op>    a lane per start: one whose left reason Op::starts refuses ends at once, the others walk (Op::decide); n
//                              into the length list for a minor candidate, else 0; the candidates kept counted a wave at a time.  Reads
//                              the table only
//   kedit_apply_kernel<Op>     a lane per start with n != 0: Op::apply -- a plain store of 0 over each of its n k-mers' words, one
//                              atomicAnd on the 32-bit half of a junction's word that holds the removed arc's in-counter (the one word two
//                              lanes may write together).  Removals and k-mers counted a wave at a time
//   kedit_totals_kernel        the four totals from the counters
// The tips (ktip.hpp: KtipOp; pg_kindex_clip_tips): a start that is free on the left walks at most max_tip k-mers and, at a
// BRANCH_IN, tests the junction's word; apply cuts the tip from that one junction
// The bubbles (kbubble.hpp: KbubbleOp; pg_kindex_pop_bubbles): a start with BRANCH_IN on the left walks its branch, takes the
// fork from the step out of rc(x0) and walks at most three siblings; apply cuts the branch from both junctions
// The arcs (karc.hpp: KarcOp; pg_kindex_drop_weak_arcs): a start with BRANCH_OUT or WEAK_NEXT on the left looks up the
// up-to-four targets of that side's arcs; apply looks them up again and takes the dangling ones out of the start's own word
// The bulges (kbulge.hpp: KbulgeOp; pg_kindex_pop_bulges): the bubbles' start, branch and apply; in place of the siblings one
// walk from the fork along the strictly strongest arcs to the join
// The islands (kisolated.hpp: KisolatedOp; pg_kindex_drop_isolated): the tips' start and walk; a chain that is free at its far
// end too is decided by the copy the unitigs emit, on its coverage sum; apply zeroes its k-mers and writes no junction
// The corrector on an index cut over ranks (kcorrect_rows.hpp; pg_kindex_correct_rows): rounds of plan, query, decide on the
// caller's stream, every query kidx_query_ranks, and the host reads the round's trial count back once a round
//   kcor_rows_begin_kernel     a lane per read over its row of the read as given: weak count, anchor, first weak k-mer behind it, the
//                              state words, and a bit a k-mer in words of the read's own (the row buffer is reused by the trial queries)
//   kcor_rows_plan_kernel      a lane per read: the moves that need no answer (kcor_rows_settle); a read with a trial due takes a slot
//                              from a counter (one atomicAdd) and writes its three sequences of 2K - 1 bases from the output batch
//   kcor_rows_decide_kernel    a lane per trial over its 3 K answers: kcor_sweep's acceptance, one base written into the read's own
//                              words, the state moved on; a read that ends gets its report word
// A batch reaches every kernel as one KidxBatch by value (kindex.hpp), and the host side builds a table the same way whether it is
// pg_kindex_build's or a rank's of a cut (kidx_rank_table, kidx_rank_insert, kidx_build_verdict).
// Both forms of the query kernel wait for one random slot read per k-mer (32 B a slot in the 63-mer build, 48 B in the 127-mer one) of a table that
// is many times the L2; the roll is arithmetic hidden under it.  The measured times, the cut over ranks included, are in DESIGN.md §10.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/soapdenovo2_amd.h"
#include "arena.hpp"
#include "device_ctx.hpp"
#include "env.hpp"
#include "karc.hpp"
#include "kbubble.hpp"
#include "kbulge.hpp"
#include "kcorrect.hpp"
#include "kcorrect_rows.hpp"
#include "kedit.hpp"
#include "kindex.hpp"
#include "kisolated.hpp"
#include "krank.hpp"
#include "ktip.hpp"
#include "ktrim.hpp"
#include "kunitig.hpp"
#include "kwalk.hpp"

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

// rank `me` of n keeps the records with map_owner(key, n) == me; n == 1 (uniform over the launch): every record, and no owner is worked out
template <int NW>
__global__ __launch_bounds__(256) void kidx_build_kernel(const uint64_t* __restrict__ records, uint64_t n_records, uint32_t n, uint32_t me,
                                                         uint64_t* tab, uint64_t mask, uint32_t* flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_records) return;
    const uint64_t* rec = records + i * (NW + 2);
    const uint64_t cnt = rec[NW];
    if (!kidx_stored(cnt)) return;                 // deleted by the -d filter: reads as 0
    const Kmer<NW> k = kidx_record_key<NW>(rec);
    if (n != 1 && map_owner<NW>(k, n) != me) return;
    kidx_insert<NW>(tab, mask, k, cnt, flags);
}

// the sequence of this lane (a lane a sequence) or of its wave (KIDX_WAVES sequences a 256-thread workgroup)
template <bool WAVE>
__device__ __forceinline__ uint64_t kidx_seq_index() {
    return WAVE ? (uint64_t)blockIdx.x * KIDX_WAVES + (threadIdx.x >> 6) : (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
}

// a wave's split of a sequence of nk k-mers: lane l takes the ceil(nk / 64) consecutive k-mers j0 .. j1 - 1 (map_read_wave_kernel's split)
__device__ __forceinline__ void kidx_wave_split(int nk, int lane, int* j0, int* j1) {
    const int per = (nk + 63) / 64;
    const int64_t first = (int64_t)lane * per;     // (64 * per can pass 2^31 where nk is close to it)
    *j0 = first < nk ? (int)first : nk;
    *j1 = first + per < nk ? (int)(first + per) : nk;
}

// the lanes' summaries merged through a __shfl_xor butterfly: every lane of the wave calls it, and every lane ends with the wave's
__device__ __forceinline__ void kidx_summary_wave_reduce(KidxSummary& s) {
    for (int d = 32; d > 0; d >>= 1) {
        KidxSummary o;
        o.present = __shfl_xor(s.present, d);
        o.cov_sum = __shfl_xor(s.cov_sum, d);
        o.cov_min = __shfl_xor(s.cov_min, d);
        o.first_absent = __shfl_xor(s.first_absent, d);
        kidx_summary_merge(s, o);
    }
}

template <int NW, bool WAVE>
__global__ __launch_bounds__(256) void kidx_query_kernel(KidxBatch b, int K, const uint64_t* __restrict__ tab, uint64_t mask, uint64_t* __restrict__ out,
                                                         uint64_t* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = kidx_seq_index<WAVE>();
    if (r >= b.n_seqs) return;                     // (WAVE: the whole wave; no workgroup barrier follows)
    const KidxSeq q = kidx_seq(b, K, r);
    KidxSummary s = kidx_summary_none();
    int j0 = 0, j1 = q.nk;
    if (WAVE) kidx_wave_split(q.nk, lane, &j0, &j1);
    if (!WAVE || q.nk) kidx_stretch<NW>(q.rd, j0, j1, K, tab, mask, out ? out + q.base : nullptr, s);   // (q.nk: wave-uniform)
    if (!summary) return;
    if (WAVE) kidx_summary_wave_reduce(s);         // (every lane of the wave is here)
    if (!WAVE || lane == 0) kidx_summary_store(s, q.nk, summary + r * KIDX_SUMMARY_WORDS);
}

template <int NW>
__global__ __launch_bounds__(256) void kcor_kernel(KidxBatch b, int K, const uint64_t* __restrict__ tab, uint64_t mask, KcorParams pr,
                                                   uint64_t* __restrict__ report) {
    const uint64_t r = kidx_seq_index<false>();
    if (r >= b.n_seqs) return;
    const KidxSeq q = kidx_seq(b, K, r);           // (b.packed is the output buffer, which already holds the batch)
    const uint64_t rep = kcor_read<NW>(const_cast<uint64_t*>(q.rd), q.nk, K, tab, mask, pr);
    if (report) report[r] = rep;
}

// walk v = 2 r + s of sequence r: s = 0 from its last k-mer, s = 1 from the reverse complement of its first (the two lie in neighbouring lanes)
template <int NW>
__global__ __launch_bounds__(256) void kwalk_kernel(KidxBatch b, int K, const uint64_t* __restrict__ tab, uint64_t mask, KwalkParams pr,
                                                    uint64_t* __restrict__ ext, uint64_t* __restrict__ report) {
    const uint64_t v = kidx_seq_index<false>();
    if (v >= 2 * b.n_seqs) return;
    const KidxSeq q = kidx_seq(b, K, v >> 1);
    kwalk_one<NW>(q.rd, q.nk, K, (v & 1) != 0, pr, [tab, mask](const Kmer<NW>& ck, uint64_t&) { return kidx_find<NW>(tab, mask, ck); },
                  ext ? ext + v * kwalk_row_words(pr.max_ext) : nullptr, report ? report + 2 * v : nullptr);
}

// ---- the index cut over ranks ----
template <int NW>
__global__ __launch_bounds__(256) void kidx_count_owners_kernel(const uint64_t* __restrict__ records, uint64_t n_records, uint32_t n,
                                                                unsigned long long* counts) {
    __shared__ uint32_t bins[DEVICE_LIST_MAX_RANKS];
    for (uint32_t b = threadIdx.x; b < n; b += blockDim.x) bins[b] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_records) atomicAdd(&bins[map_owner<NW>(kidx_record_key<NW>(records + i * (NW + 2)), n)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n; b += blockDim.x)
        if (const uint32_t c = bins[b]) atomicAdd(counts + b, (unsigned long long)c);
}

template <int NW, bool WAVE>
__global__ __launch_bounds__(256) void kidx_probe_owned_kernel(KidxBatch b, int K, uint32_t n, uint32_t me, const uint64_t* __restrict__ tab, uint64_t mask,
                                                               uint64_t* __restrict__ rows) {
    const uint64_t r = kidx_seq_index<WAVE>();
    if (r >= b.n_seqs) return;
    const KidxSeq q = kidx_seq(b, K, r);
    int j0 = 0, j1 = q.nk;
    if (WAVE) kidx_wave_split(q.nk, threadIdx.x & 63, &j0, &j1);
    uint64_t* row = rows + q.base;
    map_roll<NW>(q.rd, j0, j1, K, [&](const Kmer<NW>& ck, bool, int j) {
        if (map_owner<NW>(ck, n) == me) row[j] = kidx_find<NW>(tab, mask, ck);
    });
}

__global__ __launch_bounds__(256) void kidx_summary_rows_kernel(KidxBatch b, int K, const uint64_t* __restrict__ rows, uint64_t* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = kidx_seq_index<true>();
    if (r >= b.n_seqs) return;                     // (the whole wave; no workgroup barrier follows)
    const KidxRow w = kidx_row(b, K, r);
    const uint64_t* row = rows + w.base;
    KidxSummary s = kidx_summary_none();
    for (int64_t j = lane; j < w.nk; j += 64) kidx_summary_add(s, row[j], (int)j);   // (j + 64 can pass 2^31 where nk is close to it)
    kidx_summary_wave_reduce(s);                   // (every lane of the wave is here)
    if (lane == 0) kidx_summary_store(s, w.nk, summary + r * KIDX_SUMMARY_WORDS);
}

// ---- the trim: spans, the scan of the kept reads' counts, the pack ----
template <int NW>
__global__ __launch_bounds__(256) void ktrim_span_kernel(KidxBatch b, int K, const uint64_t* __restrict__ tab, uint64_t mask, uint32_t min_cov,
                                                         uint64_t* __restrict__ span) {
    const uint64_t r = kidx_seq_index<false>();
    if (r >= b.n_seqs) return;
    const KidxSeq q = kidx_seq(b, K, r);
    span[r] = ktrim_span_probe<NW>(q.rd, q.nk, K, tab, mask, min_cov);
}

__global__ __launch_bounds__(256) void ktrim_span_rows_kernel(KidxBatch b, int K, const uint64_t* __restrict__ rows, uint32_t min_cov,
                                                              uint64_t* __restrict__ span) {
    const uint64_t r = kidx_seq_index<false>();
    if (r >= b.n_seqs) return;
    const KidxRow w = kidx_row(b, K, r);
    span[r] = ktrim_span_row(rows + w.base, w.nk, K, min_cov);
}

// ---- the scan the trim and the unitigs share: an item's counts summed over blocks of 256 items, three kernels a scan ----
// The inclusive scan of the lanes' counts over a 256-thread workgroup: inside a wave by __shfl_up, the four waves' sums through LDS.
// Every lane of the workgroup calls it.  c becomes the lane's inclusive sums, and the workgroup's sums are returned
__device__ __forceinline__ KidxCounts kidx_block_scan(KidxCounts& c, uint64_t (*wave_sums)[KIDX_COUNTS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < KIDX_COUNTS; i++) {
        uint64_t v = c.c[i];
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up(v, d);
            v += lane >= d ? o : 0;
        }
        c.c[i] = v;
        if (lane == 63) wave_sums[wave][i] = v;
    }
    __syncthreads();
    KidxCounts all{{0, 0, 0, 0}};
#pragma unroll
    for (int i = 0; i < KIDX_COUNTS; i++)
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint64_t s = wave_sums[w][i];
            c.c[i] += w < wave ? s : 0;
            all.c[i] += s;
        }
    __syncthreads();                               // (wave_sums may be written again by the caller's next round)
    return all;
}

// the first kernel: the sums of this workgroup's lanes' counts become block blockIdx.x of `sums`.  Every lane of the workgroup calls it
__device__ __forceinline__ void kidx_block_sums(KidxCounts c, uint64_t* __restrict__ sums) {
    __shared__ uint64_t wave_sums[4][KIDX_COUNTS];
    const KidxCounts all = kidx_block_scan(c, wave_sums);
    if (threadIdx.x < KIDX_COUNTS) sums[(uint64_t)blockIdx.x * KIDX_COUNTS + threadIdx.x] = all.c[threadIdx.x];
}

// the second kernel, one workgroup: sums[b] becomes the sums of the blocks before b, in place, 256 blocks a round with the carry in
// registers.  Every lane calls it, and every lane gets the totals
__device__ __forceinline__ KidxCounts kidx_scan_block_sums(uint64_t* __restrict__ sums, uint64_t n_blocks) {
    __shared__ uint64_t wave_sums[4][KIDX_COUNTS];
    KidxCounts carry{{0, 0, 0, 0}};
    for (uint64_t at = 0; at < n_blocks; at += 256) {                           // (uniform over the workgroup: every lane meets the barriers)
        const uint64_t b = at + threadIdx.x;
        KidxCounts own{{0, 0, 0, 0}};
        if (b < n_blocks)
#pragma unroll
            for (int i = 0; i < KIDX_COUNTS; i++) own.c[i] = sums[b * KIDX_COUNTS + i];
        KidxCounts c = own;
        const KidxCounts all = kidx_block_scan(c, wave_sums);
#pragma unroll
        for (int i = 0; i < KIDX_COUNTS; i++) {
            if (b < n_blocks) sums[b * KIDX_COUNTS + i] = carry.c[i] + c.c[i] - own.c[i];
            carry.c[i] += all.c[i];
        }
    }
    return carry;
}

// the third kernel: the scan inside the workgroup again, and what the items before this lane's add up to over the whole launch -- its
// block's entry of the scanned sums, the lanes before it, itself not.  Every lane of the workgroup calls it
__device__ __forceinline__ KidxCounts kidx_scan_before(const KidxCounts& own, const uint64_t* __restrict__ sums) {
    __shared__ uint64_t wave_sums[4][KIDX_COUNTS];
    KidxCounts c = own;
    (void)kidx_block_scan(c, wave_sums);
#pragma unroll
    for (int i = 0; i < KIDX_COUNTS; i++) c.c[i] += sums[(uint64_t)blockIdx.x * KIDX_COUNTS + i] - own.c[i];
    return c;
}

// read r's counts; a lane past the batch has none
__device__ __forceinline__ KidxCounts ktrim_lane_counts(const uint64_t* span, const KidxBatch& b, int K, uint32_t min_len, uint64_t r) {
    if (r >= b.n_seqs) return KidxCounts{{0, 0, 0, 0}};
    return ktrim_counts(span[r], kidx_row(b, K, r).nk, K, min_len);
}

__global__ __launch_bounds__(256) void ktrim_block_sums_kernel(const uint64_t* __restrict__ span, KidxBatch b, int K, uint32_t min_len,
                                                               uint64_t* __restrict__ sums) {
    kidx_block_sums(ktrim_lane_counts(span, b, K, min_len, (uint64_t)blockIdx.x * 256 + threadIdx.x), sums);
}

// one workgroup: the scan of the workgroups' sums, the totals, kmer_base_out's last entry
__global__ __launch_bounds__(256) void ktrim_scan_sums_kernel(uint64_t* __restrict__ sums, uint64_t n_blocks, uint64_t* __restrict__ kmer_base_out,
                                                              uint64_t* __restrict__ totals) {
    const KidxCounts all = kidx_scan_block_sums(sums, n_blocks);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < KIDX_COUNTS; i++) totals[i] = all.c[i];
        kmer_base_out[all.c[0]] = all.c[2];
    }
}

__global__ __launch_bounds__(256) void ktrim_scatter_kernel(const uint64_t* __restrict__ span, KidxBatch b, int K, uint32_t min_len,
                                                            const uint64_t* __restrict__ sums,
                                                            uint64_t* __restrict__ word_off_out, uint64_t* __restrict__ kmer_base_out,
                                                            uint64_t* __restrict__ src_out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const KidxCounts own = ktrim_lane_counts(span, b, K, min_len, r);
    const KidxCounts before = kidx_scan_before(own, sums);
    if (!own.c[0]) return;                         // (no barrier follows)
    const uint64_t i = before.c[0];                // the kept reads before this one
    word_off_out[i] = before.c[1];
    kmer_base_out[i] = before.c[2];
    src_out[i] = r;
}

__global__ __launch_bounds__(256) void ktrim_pack_kernel(const uint64_t* __restrict__ packed, const uint64_t* __restrict__ word_off, uint32_t uniform_len,
                                                         const uint64_t* __restrict__ span, const uint64_t* __restrict__ word_off_out,
                                                         const uint64_t* __restrict__ src_out, const uint64_t* __restrict__ totals, int tail,
                                                         uint64_t n_words, uint64_t* __restrict__ packed_out) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_kept = totals[0], words = totals[1];
    if (w >= words) {
        if (w < words + (uint64_t)tail && w < n_words) packed_out[w] = 0;       // the readable words behind the last kept read
        return;
    }
    uint64_t lo = 0, hi = n_kept;                  // the last kept read that starts at or before word w: word_off_out[lo] <= w
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const bool up = word_off_out[mid] <= w;
        lo = up ? mid : lo;
        hi = up ? hi : mid;
    }
    const uint64_t r = src_out[lo], sp = span[r];
    const uint64_t* rd = packed + (uniform_len ? r * (uint64_t)((uniform_len + 31) / 32) : word_off[r]);
    // ktrim_pack_word loads two source words whatever the shift: the second one of a read's last output word may be the next read's
    // first word or, for the batch's last read, the first of the nw + 1 readable tail words -- never past the batch
    packed_out[w] = ktrim_pack_word(rd, ktrim_start(sp), ktrim_len(sp), w - word_off_out[lo]);
}

// ---- the unitigs: ends, measure, rings, the scan of the kept starts' counts, write (kunitig.hpp) ----
// The scratch of one compaction is kunitig.hpp's: KunitigScratch, laid out by kunitig_plan
// the word of the published slot at sl; 0 past the table (inside: the slot is one of the table's) or where the slot is empty
template <int NW>
__device__ __forceinline__ uint64_t kidx_published_word(const uint64_t* sl, bool inside) {
    return inside && sl[NW + 1] != KIDX_EMPTY ? sl[NW] : 0;
}
__device__ __forceinline__ uint64_t kunitig_n_starts(const KunitigScratch& s) {
    const uint64_t n = s.ctr[KUNITIG_C_STARTS];
    return n < s.cap ? n : s.cap;
}
__device__ __forceinline__ bool kunitig_covered(const uint32_t* bits, uint64_t slot) { return (bits[slot >> 5] >> (slot & 31) & 1u) != 0; }
// a start takes the next entry of the list (the order is the atomics': it differs from run to run, the set does not)
__device__ __forceinline__ void kunitig_append(const KunitigScratch& s, uint64_t start, uint32_t len) {
    const uint64_t i = atomicAdd(s.ctr + KUNITIG_C_STARTS, 1ull);
    if (i >= s.cap) return;                        // (2 * keys entries hold every start: the bound of kunitig_device_unitigs)
    s.starts[i] = start;
    s.lens[i] = len;
}
template <int NW>
__device__ __forceinline__ KwalkNode<NW> kunitig_start_node(const uint64_t* tab, uint64_t start, int K) {
    const uint64_t slot = kunitig_start_slot(start);
    const uint64_t* sl = tab + slot * map_slot_words<NW>();
    return kunitig_node<NW>(kidx_record_key<NW>(sl), sl[NW], slot, kunitig_start_fwd(start), K);
}

// a lane per table slot: a published solid key has both sides tested, two lookups at most, and every end side becomes a start
template <int NW>
__global__ __launch_bounds__(256) void kunitig_ends_kernel(const uint64_t* __restrict__ tab, uint64_t slots, int K, KunitigParams pr, KunitigScratch s) {
    constexpr int SW = map_slot_words<NW>();
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, mask = slots - 1;
    const uint64_t* sl = tab + e * SW;
    const uint64_t w = kidx_published_word<NW>(sl, e < slots);
    const bool solid = kcor_solid_word(w, pr.min_cov);
    const uint64_t wave_solid = __ballot(solid);   // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0 && wave_solid) atomicAdd(s.ctr + KUNITIG_C_SOLID, (unsigned long long)__popcll(wave_solid));
    if (!solid) return;
    uint32_t reasons[2];
    const uint32_t ends = kunitig_ends<NW>(kidx_record_key<NW>(sl), w, e, K, pr,
                                           [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); }, reasons);
    if (ends & 1u) kunitig_append(s, kunitig_start(e, true, reasons[0]), 0);
    if (ends & 2u) kunitig_append(s, kunitig_start(e, false, reasons[1]), 0);
}

// a lane per start: to the far end, a covered bit a k-mer on the way; the length, or 0 for the copy that is not emitted
template <int NW>
__global__ __launch_bounds__(256) void kunitig_measure_kernel(const uint64_t* __restrict__ tab, uint64_t mask, int K, KunitigParams pr, KunitigScratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kunitig_n_starts(s)) return;
    uint32_t* bits = s.bits;
    const KunitigWalk w = kunitig_chain<NW>(kunitig_start_node<NW>(tab, s.starts[i], K), false, K, pr,
                                            [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); },
                                            [bits](uint64_t slot) { atomicOr(bits + (slot >> 5), 1u << (slot & 31)); }, [](uint64_t) { return false; },
                                            nullptr);
    s.lens[i] = w.n;
    if (w.n && w.reason == KUNITIG_CUT) atomicAdd(s.ctr + KUNITIG_C_CUT, 1ull);
}

// a lane per table slot: a solid key no chain covered walks right until it knows whether it is the least member of a ring
template <int NW>
__global__ __launch_bounds__(256) void kunitig_rings_kernel(const uint64_t* __restrict__ tab, uint64_t slots, int K, KunitigParams pr, KunitigScratch s) {
    constexpr int SW = map_slot_words<NW>();
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, mask = slots - 1;
    if (e >= slots) return;
    const uint64_t* sl = tab + e * SW;
    if (sl[NW + 1] == KIDX_EMPTY || !kcor_solid_word(sl[NW], pr.min_cov) || kunitig_covered(s.bits, e)) return;
    const uint32_t* bits = s.bits;                 // (read only here: a ring's k-mers are not marked)
    const uint64_t start = kunitig_start(e, true, KUNITIG_CYCLE);
    const KunitigWalk w = kunitig_chain<NW>(kunitig_start_node<NW>(tab, start, K), true, K, pr,
                                            [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); },
                                            [](uint64_t) {}, [bits](uint64_t slot) { return kunitig_covered(bits, slot); }, nullptr);
    if (!w.n) return;
    kunitig_append(s, start, w.n);
    atomicAdd(s.ctr + KUNITIG_C_CYCLIC, 1ull);
}

// start i's counts for the scan; a lane past the list has none
__device__ __forceinline__ KidxCounts kunitig_lane_counts(const KunitigScratch& s, uint64_t n_starts, int K, uint64_t i) {
    return kunitig_counts(i < n_starts ? s.lens[i] : 0, K);
}

// the scan over the starts: a workgroup's sums (a workgroup past the list has nothing to say: the next kernel does not read it)
__global__ __launch_bounds__(256) void kunitig_block_sums_kernel(KunitigScratch s, int K) {
    const uint64_t n_starts = kunitig_n_starts(s);
    if ((uint64_t)blockIdx.x * 256 >= n_starts) return;                          // (uniform over the workgroup)
    kidx_block_sums(kunitig_lane_counts(s, n_starts, K, (uint64_t)blockIdx.x * 256 + threadIdx.x), s.sums);
}

// One workgroup: the scan of the workgroups' sums, the totals, and the decision the write kernel obeys: full mode, and the unitigs and
// their words with the tail fit the capacities.  Then the batch's last offsets and the tail's zero words are written here
__global__ __launch_bounds__(256) void kunitig_scan_sums_kernel(KunitigScratch s, int K, int tail, uint64_t cap_unitigs, uint64_t cap_words,
                                                                uint64_t* __restrict__ packed_out, uint64_t* __restrict__ word_off_out,
                                                                uint64_t* __restrict__ kmer_base_out, uint64_t* __restrict__ totals) {
    const KidxCounts all = kidx_scan_block_sums(s.sums, (kunitig_n_starts(s) + 255) / 256);
    if (threadIdx.x != 0) return;
    const bool go = kunitig_finish(all, K, tail, s.ctr[KUNITIG_C_SOLID], s.ctr[KUNITIG_C_CYCLIC], s.ctr[KUNITIG_C_CUT], cap_unitigs, cap_words,
                                   packed_out != nullptr, totals);
    s.ctr[KUNITIG_C_GO] = go ? 1 : 0;
    if (go) kunitig_finish_tail(all, tail, packed_out, word_off_out, kmer_base_out);
}

// a lane per start: the scan inside the workgroup again, and a kept start writes its offsets, walks once more into its row, and reports
template <int NW>
__global__ __launch_bounds__(256) void kunitig_write_kernel(const uint64_t* __restrict__ tab, uint64_t mask, int K, KunitigParams pr, KunitigScratch s,
                                                            uint64_t* __restrict__ packed_out, uint64_t* __restrict__ word_off_out,
                                                            uint64_t* __restrict__ kmer_base_out, uint64_t* __restrict__ report) {
    const uint64_t n_starts = kunitig_n_starts(s);
    if (!s.ctr[KUNITIG_C_GO] || (uint64_t)blockIdx.x * 256 >= n_starts) return;  // (uniform over the workgroup)
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const KidxCounts own = kunitig_lane_counts(s, n_starts, K, i), before = kidx_scan_before(own, s.sums);
    if (!own.c[0]) return;                         // (no barrier follows)
    const uint64_t u = before.c[0], at = before.c[1];
    if (word_off_out) word_off_out[u] = at;
    if (kmer_base_out) kmer_base_out[u] = before.c[2];
    const uint64_t start = s.starts[i];
    const uint32_t left = kunitig_start_reason(start);
    const uint32_t* bits = s.bits;
    // the walk of the measure pass (or of the rings kernel) again, step for step: own.c[1] words, which the scan has counted
    const KunitigWalk w = kunitig_chain<NW>(kunitig_start_node<NW>(tab, start, K), left == KUNITIG_CYCLE, K, pr,
                                            [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); },
                                            [](uint64_t) {}, [bits](uint64_t slot) { return kunitig_covered(bits, slot); }, packed_out + at);
    if (report) {
        report[2 * u] = kunitig_report_word(own.c[2] + (uint64_t)K - 1, left, w.reason);
        report[2 * u + 1] = w.cov;
    }
}

// ---- the unitigs by list ranking: number, sweep, rounds, rings, measure, the unitigs' scan, zero, place, emit (krank.hpp) ----
// The kernels over the nodes stride a grid of at most KRANK_BLOCKS workgroups: a round with nothing to do ends after one read a
// workgroup.  n = the oriented nodes in use, two a solid k-mer
constexpr unsigned KRANK_BLOCKS = 4096;
__device__ __forceinline__ uint64_t krank_n(const KunitigScratch& s) { return 2 * (uint64_t)s.ctr[KUNITIG_C_SOLID]; }
__device__ __forceinline__ uint64_t krank_lane() { return (uint64_t)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ uint64_t krank_stride() { return (uint64_t)gridDim.x * 256; }

// A workgroup per 256 * KRANK_NUMBER_EACH slots, a lane KRANK_NUMBER_EACH of them (coalesced a turn): the published solid keys take the next
// node ids, a workgroup's with one atomicAdd -- one a wave of 64 slots, with its answer waited for, made this pass 33 ms of a 43 ms
// call on a 268 M-slot table.  The lane's solid slots are a bit each in a register between the count and the ids
constexpr int KRANK_NUMBER_EACH = 16;
template <int NW>
__global__ __launch_bounds__(256) void krank_number_kernel(const uint64_t* __restrict__ tab, uint64_t slots, uint32_t min_cov, KunitigScratch s, KrankView v) {
    constexpr int SW = map_slot_words<NW>();
    __shared__ uint32_t wave_sums[4];
    __shared__ unsigned long long block_first;
    const uint64_t base = (uint64_t)blockIdx.x * (256 * KRANK_NUMBER_EACH) + threadIdx.x;
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < KRANK_NUMBER_EACH; k++) {
        const uint64_t e = base + (uint64_t)k * 256;
        mine |= kcor_solid_word(kidx_published_word<NW>(tab + e * SW, e < slots), min_cov) ? 1u << k : 0u;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t upto = (uint32_t)__popc(mine);         // the inclusive scan of the lanes' counts over the workgroup (every lane is here)
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(upto, d);
        upto += lane >= d ? o : 0;
    }
    if (lane == 63) wave_sums[wave] = upto;
    __syncthreads();
    uint32_t before = upto - (uint32_t)__popc(mine), all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        before += w < wave ? wave_sums[w] : 0;
        all += wave_sums[w];
    }
    if (threadIdx.x == 0) block_first = all ? atomicAdd(s.ctr + KUNITIG_C_SOLID, (unsigned long long)all) : 0ull;
    __syncthreads();
    uint32_t node = (uint32_t)block_first + before;
#pragma unroll
    for (int k = 0; k < KRANK_NUMBER_EACH; k++)
        if (mine >> k & 1u) {
            const uint64_t e = base + (uint64_t)k * 256;
            v.node_of[e] = node;
            v.slot_of[node++] = (uint32_t)e;
        }
}

// a lane per table slot: krank_sweep, the unitigs' ends sweep that also writes every oriented node's first record
template <int NW>
__global__ __launch_bounds__(256) void krank_sweep_kernel(const uint64_t* __restrict__ tab, uint64_t slots, int K, KunitigParams pr, KunitigScratch s, KrankView v,
                                                          uint32_t* ctl) {
    const uint64_t e = krank_lane(), mask = slots - 1;
    const uint64_t* sl = tab + e * map_slot_words<NW>();
    const uint64_t w = kidx_published_word<NW>(sl, e < slots);
    bool open = false;
    if (kcor_solid_word(w, pr.min_cov))
        open = krank_sweep<NW>(v, sl, e, K, pr,
                               [tab, mask](const Kmer<NW>& ck, uint64_t& slot) { return kunitig_probe<NW>(tab, mask, ck, slot); },
                               [&s](uint64_t start) { kunitig_append(s, start, 0); });
    krank_sweep_done(ctl, open);
}

// The passes over the nodes are krank.hpp's, each a launch-uniform decision, an item body under a grid-stride loop, and what the pass
// leaves behind in the control words.  Round j: a round behind one in which nothing became done passes the generation on and ends
__global__ __launch_bounds__(256) void krank_jump_kernel(KunitigScratch s, KrankView v, uint32_t* ctl, int j) {
    const KrankPass p = krank_jump_pass(ctl, j);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    bool any = false;
    if (!p.go) {                                   // (uniform over the launch)
        krank_jump_done(p, ctl, j, any, first);
        return;
    }
    const KrankRec* src = krank_cur(v, p);
    KrankRec* dst = krank_other(v, p);
    for (uint64_t x = krank_lane(), n = krank_n(s); x < n; x += krank_stride()) krank_jump_item(src, dst, x, any);
    krank_jump_done(p, ctl, j, any, first);
}

// the rings: a record the R rounds did not finish opens its window in the free generation
__global__ __launch_bounds__(256) void krank_ring_init_kernel(KunitigScratch s, KrankView v, uint32_t* ctl, int R) {
    const KrankPass p = krank_ring_init_pass(ctl, R);
    const KrankRec* fin = krank_cur(v, p);
    KrankRec* spare = krank_other(v, p);
    bool any = false;
    for (uint64_t x = krank_lane(), n = krank_n(s); x < n; x += krank_stride()) krank_ring_init_item(fin, spare, v, x, any);
    krank_ring_init_done(ctl, any);
}

// round r of the rings' windows; ends at once when there is no ring
template <int NW>
__global__ __launch_bounds__(256) void krank_min_kernel(const uint64_t* __restrict__ tab, KunitigScratch s, KrankView v, const uint32_t* ctl, int R, int r) {
    const KrankPass p = krank_ring_pass(ctl, R);
    if (!p.go) return;                             // (uniform over the launch)
    const KrankRec* fin = krank_cur(v, p);
    KrankRec* spare = krank_other(v, p);
    for (uint64_t x = krank_lane(), n = krank_n(s); x < n; x += krank_stride()) krank_min_item<NW>(fin, spare, v, tab, r, x);
}

// the rings become chains from their least members, which are appended to the start list, and the rounds may run again
template <int NW>
__global__ __launch_bounds__(256) void krank_ring_cut_kernel(const uint64_t* __restrict__ tab, KunitigScratch s, KrankView v, uint32_t* ctl, int R) {
    const KrankPass p = krank_ring_pass(ctl, R);
    if (!p.go) return;                             // (uniform over the launch)
    KrankRec* fin = krank_cur(v, p);
    const KrankRec* spare = krank_other(v, p);
    for (uint64_t x = krank_lane(), n = krank_n(s); x < n; x += krank_stride())
        krank_ring_cut_item<NW>(fin, spare, v, tab, R, x, [&s](uint64_t start) { kunitig_append(s, start, 0); },
                                [&s] { atomicAdd(s.ctr + KUNITIG_C_CYCLIC, 1ull); });
    krank_ring_cut_done(ctl, R, blockIdx.x == 0 && threadIdx.x == 0);
}

// a lane per start: its length for the scan from its record
template <int NW>
__global__ __launch_bounds__(256) void krank_measure_kernel(const uint64_t* __restrict__ tab, int K, KunitigScratch s, KrankView v, const uint32_t* ctl, int R) {
    const uint64_t i = krank_lane();
    if (i >= kunitig_n_starts(s)) return;
    s.lens[i] = krank_measure<NW>(s.starts[i], tab, v, krank_cur(v, krank_final_pass(ctl, R)), K);
}

// the rows' words zeroed where the scan said go: the emit pass ORs into them
__global__ __launch_bounds__(256) void krank_zero_kernel(KunitigScratch s, const uint64_t* __restrict__ totals, int tail, uint64_t* __restrict__ packed_out) {
    if (!s.ctr[KUNITIG_C_GO]) return;              // (uniform over the launch)
    for (uint64_t w = krank_lane(), words = totals[KUNITIG_T_WORDS] - (uint64_t)tail; w < words; w += krank_stride()) packed_out[w] = 0;
}

// a lane per start: the scan inside the workgroup again; krank_place
template <int NW>
__global__ __launch_bounds__(256) void krank_place_kernel(const uint64_t* __restrict__ tab, int K, KunitigScratch s, KrankView v, const uint32_t* ctl, int R,
                                                          uint64_t* __restrict__ word_off_out, uint64_t* __restrict__ kmer_base_out,
                                                          uint64_t* __restrict__ report) {
    const uint64_t n_starts = kunitig_n_starts(s);
    if (!s.ctr[KUNITIG_C_GO] || (uint64_t)blockIdx.x * 256 >= n_starts) return;  // (uniform over the workgroup)
    const uint64_t i = krank_lane();
    const KidxCounts own = kunitig_lane_counts(s, n_starts, K, i), before = kidx_scan_before(own, s.sums);
    if (i >= n_starts) return;                     // (no barrier follows)
    const KrankPass f = krank_final_pass(ctl, R);
    krank_place<NW>(s.starts[i], (uint32_t)own.c[2], before.c[0], before.c[1], before.c[2], tab, v, krank_cur(v, f), krank_other(v, f), K, word_off_out, kmer_base_out,
                    report);
}

// every node into its row: krank_emit with a 64-bit atomicOr
template <int NW>
__global__ __launch_bounds__(256) void krank_emit_kernel(const uint64_t* __restrict__ tab, int K, KunitigScratch s, KrankView v, const uint32_t* ctl, int R,
                                                         uint64_t* packed_out) {
    if (!s.ctr[KUNITIG_C_GO]) return;              // (uniform over the launch)
    const KrankPass f = krank_final_pass(ctl, R);
    for (uint64_t node = krank_lane(), n = s.ctr[KUNITIG_C_SOLID]; node < n; node += krank_stride())
        krank_emit<NW>((uint32_t)node, tab, v, krank_cur(v, f), krank_other(v, f), K,
                       [packed_out](uint64_t at, uint64_t bits) { atomicOr((unsigned long long*)packed_out + at, (unsigned long long)bits); });
}

// ---- the operators that edit the graph: ends (the unitigs' kernel), decide, apply, the totals (kedit.hpp; ktip.hpp, kbubble.hpp) ----
// A round's counters lie behind the unitigs' in the same scratch (kunitig.hpp: KEDIT_C_*)

// the table as an operator reaches it: the lookup, a k-mer's word zeroed with a plain store, and a junction's counter taken out with an
// atomicAnd on the 32-bit half that holds it: another lane may clear another counter of that half
template <int NW>
struct KeditFind {
    const uint64_t* tab;
    uint64_t mask;
    __device__ uint64_t operator()(const Kmer<NW>& ck, uint64_t& slot) const { return kunitig_probe<NW>(tab, mask, ck, slot); }
};
template <int NW>
struct KeditZero {
    uint64_t* tab;
    __device__ void operator()(uint64_t slot) const { tab[slot * map_slot_words<NW>() + NW] = 0; }
};
template <int NW>
struct KeditClear {
    uint64_t* tab;
    __device__ void operator()(uint64_t slot, bool fwd, int a) const {
        atomicAnd((unsigned int*)(tab + slot * map_slot_words<NW>() + NW) + kedit_in_half(fwd), kedit_keep_mask(fwd, a));
    }
};

// a lane per start: the decision, n into the length list for a minor candidate and 0 for every other start.  Only reads the table
template <int NW, class Op>
__global__ __launch_bounds__(256) void kedit_decide_kernel(const uint64_t* __restrict__ tab, uint64_t mask, int K, typename Op::Params pr, KunitigScratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    KeditDecision d{0, false, false};
    if (i < kunitig_n_starts(s)) {
        const uint64_t start = s.starts[i];
        const uint32_t left = kunitig_start_reason(start);
        if (Op::starts(left))                      // (any other start ends at once: its slot is not even read)
            d = Op::template decide<NW>(kunitig_start_node<NW>(tab, start, K), left, K, pr, KeditFind<NW>{tab, mask});
        s.lens[i] = d.minor ? d.n : 0;
    }
    const uint64_t wave_kept = __ballot(d.candidate && !d.minor);                 // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0 && wave_kept) atomicAdd(s.ctr + KEDIT_C_KEPT, (unsigned long long)__popcll(wave_kept));
}

// a lane per start with n != 0: its n k-mers' words zeroed -- they are in no other lane's unitig --, its counters taken out of the
// junctions' words
template <int NW, class Op>
__global__ __launch_bounds__(256) void kedit_apply_kernel(uint64_t* tab, uint64_t mask, int K, typename Op::Params pr, KunitigScratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = i < kunitig_n_starts(s) ? s.lens[i] : 0;
    if (n)
        Op::template apply<NW>(kunitig_start_node<NW>(tab, s.starts[i], K), n, K, pr, KeditFind<NW>{tab, mask}, KeditZero<NW>{tab}, KeditClear<NW>{tab});
    const uint64_t wave_removed = __ballot(n != 0);                              // (every lane of the wave is here)
    uint32_t wave_kmers = n;                       // (64 lanes of at most 2^16 k-mers)
#pragma unroll
    for (int d = 32; d; d >>= 1) wave_kmers += __shfl_xor(wave_kmers, d);
    if ((threadIdx.x & 63) == 0 && wave_removed) {
        atomicAdd(s.ctr + KEDIT_C_REMOVED, (unsigned long long)__popcll(wave_removed));
        atomicAdd(s.ctr + KEDIT_C_KMERS, (unsigned long long)wave_kmers);
    }
}

__global__ void kedit_totals_kernel(KunitigScratch s, uint64_t* __restrict__ totals) {
    if (threadIdx.x != 0) return;
    totals[KEDIT_T_REMOVED] = s.ctr[KEDIT_C_REMOVED];
    totals[KEDIT_T_KMERS] = s.ctr[KEDIT_C_KMERS];
    totals[KEDIT_T_SOLID] = s.ctr[KUNITIG_C_SOLID];
    totals[KEDIT_T_KEPT] = s.ctr[KEDIT_C_KEPT];
}

// ---- the corrector on an index cut over ranks: rounds over merged rows (kcorrect_rows.hpp) ----
__global__ __launch_bounds__(256) void kcor_rows_begin_kernel(KidxBatch b, int K, const uint64_t* __restrict__ rows, uint32_t min_cov,
                                                              uint64_t* __restrict__ state, uint64_t* __restrict__ bits, uint64_t* __restrict__ report) {
    const uint64_t r = kidx_seq_index<false>();
    if (r >= b.n_seqs) return;
    const KidxRow w = kidx_row(b, K, r);
    const KcorRowsRead s = kcor_rows_begin(rows + w.base, w.nk, min_cov, bits + kcor_rows_bits_at(w.base, r));
    kcor_rows_store(state + r * KCOR_ROWS_STATE_WORDS, s);
    if (report && s.phase == KCOR_ROWS_DONE) report[r] = kcor_rows_report(s);
}

// (b.packed is the output buffer: the trial sequences are cut from the read as it stands)
__global__ __launch_bounds__(256) void kcor_rows_plan_kernel(KidxBatch b, int K, uint32_t max_fixes, uint64_t* __restrict__ state,
                                                             const uint64_t* __restrict__ bits, uint64_t cap, unsigned long long* __restrict__ claimed,
                                                             uint64_t* __restrict__ trial_read, uint64_t* __restrict__ trial, uint64_t* __restrict__ report) {
    const uint64_t r = kidx_seq_index<false>();
    if (r >= b.n_seqs) return;
    uint64_t* st = state + r * KCOR_ROWS_STATE_WORDS;
    KcorRowsRead s = kcor_rows_load(st);
    if (s.phase == KCOR_ROWS_DONE) return;
    const KidxSeq q = kidx_seq(b, K, r);
    const bool due = kcor_rows_settle(s, q.nk, max_fixes, bits + kcor_rows_bits_at(q.base, r));
    if (due) {
        const uint64_t slot = atomicAdd(claimed, 1ull);   // (which reads get the slots is not deterministic; the result is)
        if (slot < cap) {
            trial_read[slot] = r;
            kcor_rows_trial_write(q.rd, q.nk, K, s, trial + slot * 3 * (uint64_t)kcor_rows_trial_words(K));
        }
    }
    kcor_rows_store(st, s);
    if (!due && report) report[r] = kcor_rows_report(s);
}

__global__ __launch_bounds__(256) void kcor_rows_decide_kernel(KidxBatch b, int K, KcorParams pr, uint64_t n_trials, const uint64_t* __restrict__ trial_read,
                                                               const uint64_t* __restrict__ trial_rows, uint64_t* __restrict__ state,
                                                               const uint64_t* __restrict__ bits, uint64_t* __restrict__ report) {
    const uint64_t t = kidx_seq_index<false>();
    if (t >= n_trials) return;
    const uint64_t r = trial_read[t];
    uint64_t* st = state + r * KCOR_ROWS_STATE_WORDS;
    KcorRowsRead s = kcor_rows_load(st);
    const KidxSeq q = kidx_seq(b, K, r);
    const bool more = kcor_rows_decide(s, trial_rows + t * 3 * (uint64_t)K, const_cast<uint64_t*>(q.rd), q.nk, K, pr, bits + kcor_rows_bits_at(q.base, r));
    kcor_rows_store(st, s);
    if (!more && report) report[r] = kcor_rows_report(s);
}

namespace {

int kidx_set_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { pg_set_error("k-mer index: no HIP device"); return PG_ENODEV; }
    if (dev < 0 || dev >= n) { pg_set_error("k-mer index: HIP device " + std::to_string(dev) + " does not exist"); return PG_ENODEV; }
    KIDX_HIP(hipSetDevice(dev));
    return PG_OK;
}

// the workgroups of a launch over n items, `per` of them a workgroup; `what` is too many or too large for one launch
int kidx_launch_blocks(uint64_t n, unsigned per, const char* what, dim3* grid) {
    const uint64_t blocks = (n + per - 1) / per;
    if (blocks > 0x7FFFFFFFULL) { pg_set_error(std::string("k-mer index: ") + what + " for one launch"); return PG_EINVAL; }
    *grid = dim3((unsigned)blocks);
    return PG_OK;
}
int kidx_record_blocks(uint64_t n_records, dim3* grid) { return kidx_launch_blocks(n_records, 256, "too many records", grid); }
// a lane a sequence, or a wave a sequence
int kidx_batch_blocks(uint64_t n_seqs, bool wave, dim3* grid) { return kidx_launch_blocks(n_seqs, wave ? KIDX_WAVES : 256, "batch too large", grid); }

// f(std::integral_constant<int, NW>) launches a kernel of the index's flavour
template <typename F>
int kidx_launch(const ::pg_kindex* ix, F f) {
    kidx_with_nw(ix->nw, f);
    KIDX_HIP(hipGetLastError());
    return PG_OK;
}

// ---- a rank's build, for pg_kindex_build's one table and a cut's ranks alike: on the rank's device, on stream st ----
// the table for r.keys records and the flags, from the arena, zeroed
int kidx_rank_table(KidxRank& r, int nw, hipStream_t st) {
    r.slots = map_table_slots(r.keys);
    const size_t bytes = kidx_table_bytes(r.keys, nw);
    if (arena_malloc(&r.d_tab, bytes) != hipSuccess || arena_malloc(&r.d_flags, sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        pg_set_error("k-mer index: out of device memory for a table of " + std::to_string(r.slots) + " slots (" + std::to_string(bytes >> 20) + " MiB)");
        return PG_ENOMEM;
    }
    KIDX_HIP(hipMemsetAsync(r.d_tab, 0, bytes, st));
    KIDX_HIP(hipMemsetAsync(r.d_flags, 0, sizeof(uint32_t), st));
    return PG_OK;
}

// the m records at d_records that rank `me` of n owns go into its table
int kidx_rank_insert(const ::pg_kindex* ix, uint32_t me, const uint64_t* d_records, uint64_t m, hipStream_t st) {
    const KidxRank& r = ix->ranks[me];
    dim3 grid;
    if (int rc = kidx_record_blocks(m, &grid)) return rc;
    return kidx_launch(ix, [&](auto nw) {
        hipLaunchKernelGGL((kidx_build_kernel<decltype(nw)::value>), grid, dim3(256), 0, st, d_records, m, (uint32_t)ix->ranks.size(), me, r.d_tab, r.slots - 1,
                           r.d_flags);
    });
}

// what the ranks' flags, read back once their streams were waited for, say of the build
int kidx_build_verdict(uint32_t flags) {
    if (flags & KIDX_FLAG_DUP) { pg_set_error("k-mer index: duplicate key in records"); return PG_EINVAL; }
    if (flags & KIDX_FLAG_SPIN) {
        pg_set_error("k-mer index: the build gave up on a claimed slot after " + std::to_string(KIDX_SPIN_CAP) +
                     " trips (the slot's key was never published); the index is not complete");
        return PG_ESPIN;
    }
    return PG_OK;
}

}  // namespace

// one table: the caller's stream, no owners to count, no stream or event of the index's own
int kidx_device_build(::pg_kindex* ix, const uint64_t* d_records, uint64_t n_records, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    KidxRank& r = ix->ranks[0];
    dim3 grid;
    if (int rc = kidx_set_device(r.device)) return rc;
    if (int rc = kidx_record_blocks(n_records, &grid)) return rc;
    arena_pin_for_process(r.device);
    r.keys = n_records;
    if (int rc = kidx_rank_table(r, ix->nw, st)) return rc;
    if (n_records) if (int rc = kidx_rank_insert(ix, 0, d_records, n_records, st)) return rc;
    uint32_t flags = 0;
    KIDX_HIP(hipMemcpyAsync(&flags, r.d_flags, sizeof flags, hipMemcpyDeviceToHost, st));
    KIDX_HIP(hipStreamSynchronize(st));
    return kidx_build_verdict(flags);
}

int kidx_device_query(::pg_kindex* ix, const KidxBatch& b, int wave, uint64_t* d_out, uint64_t* d_summary, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const KidxRank& t = ix->ranks[0];
    dim3 grid;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!b.n_seqs) return PG_OK;
    if (int rc = kidx_batch_blocks(b.n_seqs, wave, &grid)) return rc;
    return kidx_launch(ix, [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        if (wave) hipLaunchKernelGGL((kidx_query_kernel<NW, true>), grid, dim3(256), 0, st, b, ix->K, t.d_tab, t.slots - 1, d_out, d_summary);
        else hipLaunchKernelGGL((kidx_query_kernel<NW, false>), grid, dim3(256), 0, st, b, ix->K, t.d_tab, t.slots - 1, d_out, d_summary);
    });
}

int kcor_device_correct(::pg_kindex* ix, const KidxBatch& b, const KcorParams& pr, uint64_t* d_packed_out, uint64_t* d_report, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const KidxRank& t = ix->ranks[0];
    dim3 grid;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!b.n_seqs) return PG_OK;
    if (int rc = kidx_batch_blocks(b.n_seqs, false, &grid)) return rc;
    // the copy first -- pad bits and the readable tail with it -- then every lane works on its own words of the output
    if (d_packed_out != b.packed) KIDX_HIP(hipMemcpyAsync(d_packed_out, b.packed, b.n_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    KidxBatch o = b;
    o.packed = d_packed_out;
    return kidx_launch(ix, [&](auto nw) {
        hipLaunchKernelGGL((kcor_kernel<decltype(nw)::value>), grid, dim3(256), 0, st, o, ix->K, t.d_tab, t.slots - 1, pr, d_report);
    });
}

int kwalk_device_walk(::pg_kindex* ix, const KidxBatch& b, const KwalkParams& pr, uint64_t* d_ext, uint64_t* d_report, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const KidxRank& t = ix->ranks[0];
    dim3 grid;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!b.n_seqs) return PG_OK;
    if (int rc = kidx_batch_blocks(2 * b.n_seqs, false, &grid)) return rc;   // a lane a walk
    return kidx_launch(ix, [&](auto nw) {
        hipLaunchKernelGGL((kwalk_kernel<decltype(nw)::value>), grid, dim3(256), 0, st, b, ix->K, t.d_tab, t.slots - 1, pr, d_ext, d_report);
    });
}

// ---- the index cut over ranks ----
namespace {

// a device part's count: the stream it runs on (a rank's where one lies on the part's device, else one of its own) and its n bins
struct KidxPartCount {
    int device = -1;
    hipStream_t st = nullptr;
    bool own_stream = false;
    unsigned long long* d_bins = nullptr;
};

void kidx_sync_ranks(::pg_kindex* ix) {
    for (KidxRank& r : ix->ranks) {
        if (!r.st) continue;
        (void)hipSetDevice(r.device);
        (void)hipStreamSynchronize(r.st);
    }
}

// at least `want` words behind *p (the current device's arena); what was there is given up, not copied
int kidx_reserve(uint64_t** p, uint64_t* cap, uint64_t want) {
    if (want <= *cap) return PG_OK;
    if (*p) (void)arena_free(*p);
    *p = nullptr;
    *cap = 0;
    if (arena_malloc(p, want * sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        pg_set_error("k-mer index: out of device memory for a batch buffer of " + std::to_string(want * sizeof(uint64_t)) + " bytes");
        return PG_ENOMEM;
    }
    *cap = want;
    return PG_OK;
}

// An operator's scratch (KidxScratch, kindex.hpp; the lead's device is current).  A call begins with at least `want` words behind s.d
// and `st` behind the end of the last call that used them, and ends by recording its own end on `st`
int kidx_scratch_begin(KidxScratch& s, uint64_t want, hipStream_t st) {
    if (int rc = kidx_reserve(&s.d, &s.cap, want)) return rc;
    if (!s.e_end) KIDX_HIP(hipEventCreate(&s.e_end));
    if (s.recorded) KIDX_HIP(hipStreamWaitEvent(st, s.e_end, 0));
    return PG_OK;
}
int kidx_scratch_end(KidxScratch& s, hipStream_t st) {
    KIDX_HIP(hipEventRecord(s.e_end, st));
    s.recorded = true;
    return PG_OK;
}
void kidx_scratch_free(KidxScratch& s) {
    if (s.d) (void)arena_free(s.d);                // (waits for the device: no call still uses the scratch)
    if (s.e_end) (void)hipEventDestroy(s.e_end);
    s = KidxScratch();
}

// What an entry point over the ranks returns: after a failure no stream is left reading the caller's batch or the scratch, or writing
// its results
int kidx_settled(::pg_kindex* ix, int rc, void* stream) {
    if (rc) {
        kidx_sync_ranks(ix);
        (void)hipSetDevice(ix->device);
        (void)hipStreamSynchronize((hipStream_t)stream);
    }
    return rc;
}

// the fewest ranks pg_host_kindex_plan says hold n_records on a device with device_bytes free, a rank's table at most table_cap; 0: none
int kidx_fewest_ranks(uint64_t n_records, int nw, uint64_t device_bytes, uint64_t table_cap) {
    uint64_t plan[12];
    for (int n = 1; n <= DEVICE_LIST_MAX_RANKS; n++)
        if (pg_host_kindex_plan(n_records, nw == 4, n, 0, 0, device_bytes, plan) == PG_OK && plan[9] && plan[0] <= table_cap) return n;
    return 0;
}

// kidx_device_build_sharded's work; the caller owns what the streams read and write meanwhile and cleans up after every way out of here
int kidx_build_ranks(::pg_kindex* ix, const uint64_t* const* parts, const uint64_t* part_records, const int* part_device, int n_parts,
                     hipStream_t st, std::vector<KidxPartCount>& pc, std::vector<unsigned long long>& bins, std::vector<uint32_t>& flags) {
    const uint32_t n = (uint32_t)ix->ranks.size();
    const int rw = ix->nw + 2;
    dim3 grid;
    KidxRank& lead = ix->ranks[0];
    for (int p = 0; p < n_parts; p++) {
        if (part_device[p] >= 0) if (int rc = kidx_set_device(part_device[p])) return rc;
        if (int rc = kidx_record_blocks(part_records[p], &grid)) return rc;
    }
    // 1. every rank's stream and events; the caller's stream has made the parts, so every stream that reads one goes behind e_begin
    for (KidxRank& r : ix->ranks) {
        if (int rc = kidx_set_device(r.device)) return rc;
        arena_pin_for_process(r.device);
        KIDX_HIP(hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking));
        KIDX_HIP(hipEventCreate(&r.e0));
        KIDX_HIP(hipEventCreate(&r.e1));
    }
    KIDX_HIP(hipSetDevice(lead.device));
    for (hipEvent_t* e : {&ix->e_begin, &ix->e_probed, &ix->e_merged, &ix->e_end}) KIDX_HIP(hipEventCreate(e));
    KIDX_HIP(hipEventRecord(ix->e_begin, st));
    // 2. the owners of every part's records: a device part where it lies, a host part by a plain loop
    for (int p = 0; p < n_parts; p++) {
        if (!part_records[p]) continue;
        unsigned long long* out = bins.data() + (size_t)p * n;
        if (part_device[p] < 0) {
            kidx_with_nw(ix->nw, [&](auto nw) {
                constexpr int NW = decltype(nw)::value;
                for (uint64_t i = 0; i < part_records[p]; i++) out[map_owner<NW>(kidx_record_key<NW>(parts[p] + i * (NW + 2)), n)]++;
            });
            continue;
        }
        KidxPartCount& c = pc[(size_t)p];
        c.device = part_device[p];
        KIDX_HIP(hipSetDevice(c.device));
        for (KidxRank& r : ix->ranks) if (r.device == c.device && !c.st) c.st = r.st;
        if (!c.st) {
            KIDX_HIP(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
            c.own_stream = true;
        }
        if (arena_malloc(&c.d_bins, n * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            pg_set_error("k-mer index: out of device memory for the owners' counts");
            return PG_ENOMEM;
        }
        KIDX_HIP(hipStreamWaitEvent(c.st, ix->e_begin, 0));
        KIDX_HIP(hipMemsetAsync(c.d_bins, 0, n * sizeof(unsigned long long), c.st));
        (void)kidx_record_blocks(part_records[p], &grid);
        if (int rc = kidx_launch(ix, [&](auto nw) {
                hipLaunchKernelGGL((kidx_count_owners_kernel<decltype(nw)::value>), grid, dim3(256), 0, c.st, parts[p], part_records[p], n, c.d_bins);
            }))
            return rc;
        KIDX_HIP(hipMemcpyAsync(out, c.d_bins, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.st));
    }
    // the host's first wait: the counts
    for (KidxPartCount& c : pc) {
        if (!c.st) continue;
        KIDX_HIP(hipSetDevice(c.device));
        KIDX_HIP(hipStreamSynchronize(c.st));
    }
    uint64_t total = 0, n_records = 0;
    for (int p = 0; p < n_parts; p++) n_records += part_records[p];
    for (uint32_t i = 0; i < n; i++) {
        KidxRank& r = ix->ranks[i];
        r.keys = 0;
        for (int p = 0; p < n_parts; p++) r.keys += bins[(size_t)p * n + i];
        total += r.keys;
    }
    if (total != n_records) {
        pg_set_error("k-mer index: the ranks own " + std::to_string(total) + " records of " + std::to_string(n_records));
        return PG_EINVAL;
    }
    // 3. does every rank's table, exactly sized, and its chunk buffer fit its device?  Asked before either is allocated
    const uint64_t chunk = kidx_chunk_records();
    const char* hook = env_test("SOAPDENOVO2_AMD_KINDEX_BUDGET_MB");
    const uint64_t table_cap = hook ? (uint64_t)atoll(hook) << 20 : ~0ull;
    std::vector<uint64_t> chunk_words(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        KidxRank& r = ix->ranks[i];
        if (r.keys)                                // (a rank that owns nothing reads no part)
            for (int p = 0; p < n_parts; p++)
                if (part_device[p] != r.device) chunk_words[i] = std::max(chunk_words[i], std::min(chunk, part_records[p]) * (uint64_t)rw);
        const uint64_t table = kidx_table_bytes(r.keys, ix->nw), with_chunk = table + chunk_words[i] * sizeof(uint64_t);
        uint64_t free_b = 0;
        if (int rc = map_device_free_bytes(r.device, &free_b)) return rc;
        const uint64_t budget = (uint64_t)((double)free_b * 0.85);
        if (with_chunk <= budget && table <= table_cap) continue;
        const int fewest = kidx_fewest_ranks(n_records, ix->nw, free_b, table_cap);
        std::string msg = "k-mer index: the index does not fit: over " + std::to_string(n) + " rank(s), rank " + std::to_string(i) + "'s table is " +
                          std::to_string(table) + " bytes (" + std::to_string(with_chunk) + " with its chunk buffer) and the budget of device " +
                          std::to_string(r.device) + " is " + std::to_string(budget) + " bytes";
        if (hook) msg += "; SOAPDENOVO2_AMD_KINDEX_BUDGET_MB caps a rank's table at " + std::to_string(table_cap) + " bytes";
        msg += fewest ? ".  " + std::to_string(fewest) + " ranks would hold it" : ".  No number of ranks up to " + std::to_string(DEVICE_LIST_MAX_RANKS) + " holds it";
        pg_set_error(msg);
        return PG_ENOMEM;
    }
    // 4. the tables, zeroed, and the records: a part on the rank's own device where it lies, any other through the chunk buffer
    for (uint32_t i = 0; i < n; i++) {
        KidxRank& r = ix->ranks[i];
        KIDX_HIP(hipSetDevice(r.device));
        if (int rc = kidx_rank_table(r, ix->nw, r.st)) return rc;
        if (chunk_words[i] && arena_malloc(&r.d_chunk, chunk_words[i] * sizeof(uint64_t)) != hipSuccess) {
            (void)hipGetLastError();
            pg_set_error("k-mer index: out of device memory for rank " + std::to_string(i) + "'s chunk buffer");
            return PG_ENOMEM;
        }
        KIDX_HIP(hipStreamWaitEvent(r.st, ix->e_begin, 0));
        for (int p = 0; p < n_parts && r.keys; p++) {                             // (a rank that owns nothing launches no insert)
            const bool in_place = part_device[p] == r.device;
            const uint64_t step = in_place ? part_records[p] : chunk;
            for (uint64_t at = 0; at < part_records[p]; at += step) {
                const uint64_t m = std::min(step, part_records[p] - at);
                const uint64_t* src = parts[p] + at * (uint64_t)rw;
                if (!in_place) {
                    const size_t b = m * (uint64_t)rw * sizeof(uint64_t);
                    if (part_device[p] < 0) KIDX_HIP(hipMemcpyAsync(r.d_chunk, src, b, hipMemcpyHostToDevice, r.st));
                    else KIDX_HIP(hipMemcpyPeerAsync(r.d_chunk, r.device, src, part_device[p], b, r.st));
                    src = r.d_chunk;
                }
                if (int rc = kidx_rank_insert(ix, i, src, m, r.st)) return rc;
            }
        }
        KIDX_HIP(hipMemcpyAsync(&flags[i], r.d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, r.st));
    }
    // the host's second wait: every rank's inserts
    uint32_t any = 0;
    for (uint32_t i = 0; i < n; i++) {
        KIDX_HIP(hipSetDevice(ix->ranks[i].device));
        KIDX_HIP(hipStreamSynchronize(ix->ranks[i].st));
        any |= flags[i];
    }
    return kidx_build_verdict(any);
}

int kidx_query_ranks(::pg_kindex* ix, const KidxBatch& b, int wave, uint64_t* d_out, uint64_t* d_summary, hipStream_t st) {
    const uint32_t n = (uint32_t)ix->ranks.size();
    const uint64_t n_words = b.n_words, n_seqs = b.n_seqs, n_kmers = b.n_kmers;
    KidxRank& lead = ix->ranks[0];
    dim3 grid, grid_waves;
    if (int rc = kidx_batch_blocks(n_seqs, wave, &grid)) return rc;
    if (d_summary) if (int rc = kidx_batch_blocks(n_seqs, true, &grid_waves)) return rc;
    // The buffers grow to the largest batch met.  One that has to grow is given back first, and the previous query may still use it: only
    // then does the host wait, for that query's end
    bool grow = n > 1 && n_kmers > ix->cap_staging;
    for (uint32_t i = 0; i < n; i++) {
        const KidxRank& r = ix->ranks[i];
        grow = grow || ((i || !d_out) && n_kmers > r.cap_rows);
        grow = grow || (r.device != lead.device && (n_words > r.cap_packed || (!b.uniform_len && n_seqs + 1 > r.cap_seqs)));
    }
    if (grow && ix->queried) KIDX_HIP(hipEventSynchronize(ix->e_end));
    KIDX_HIP(hipSetDevice(lead.device));
    if (ix->queried) KIDX_HIP(hipStreamWaitEvent(st, ix->e_end, 0));             // (another stream than last time's: the staging buffer is one)
    KIDX_HIP(hipEventRecord(ix->e_begin, st));
    // every rank: behind the caller's stream and the previous query's end, the batch (in place on the lead's device), zeroed rows, its probe
    for (uint32_t i = 0; i < n; i++) {
        KidxRank& r = ix->ranks[i];
        KIDX_HIP(hipSetDevice(r.device));
        KidxBatch mine = b;                        // the rank's view of the batch: in place on the lead's device, else its copy
        uint64_t* rows = i == 0 && d_out ? d_out : nullptr;
        if (!rows) {
            if (int rc = kidx_reserve(&r.d_rows, &r.cap_rows, std::max<uint64_t>(n_kmers, 1))) return rc;
            rows = r.d_rows;
        }
        KIDX_HIP(hipStreamWaitEvent(r.st, ix->e_begin, 0));
        if (ix->queried) KIDX_HIP(hipStreamWaitEvent(r.st, ix->e_end, 0));
        if (r.device != lead.device) {
            if (int rc = kidx_reserve(&r.d_packed, &r.cap_packed, n_words)) return rc;
            KIDX_HIP(hipMemcpyPeerAsync(r.d_packed, r.device, b.packed, lead.device, n_words * sizeof(uint64_t), r.st));
            mine.packed = r.d_packed;
            if (!b.uniform_len) {
                uint64_t cap = r.cap_seqs;
                if (int rc = kidx_reserve(&r.d_word_off, &cap, n_seqs + 1)) return rc;
                if (int rc = kidx_reserve(&r.d_kmer_base, &r.cap_seqs, n_seqs + 1)) return rc;
                KIDX_HIP(hipMemcpyPeerAsync(r.d_word_off, r.device, b.word_off, lead.device, n_seqs * sizeof(uint64_t), r.st));
                KIDX_HIP(hipMemcpyPeerAsync(r.d_kmer_base, r.device, b.kmer_base, lead.device, (n_seqs + 1) * sizeof(uint64_t), r.st));
                mine.word_off = r.d_word_off;
                mine.kmer_base = r.d_kmer_base;
            }
        }
        if (n_kmers) KIDX_HIP(hipMemsetAsync(rows, 0, n_kmers * sizeof(uint64_t), r.st));
        KIDX_HIP(hipEventRecord(r.e0, r.st));
        if (int rc = kidx_launch(ix, [&](auto nw) {
                constexpr int NW = decltype(nw)::value;
                if (wave) hipLaunchKernelGGL((kidx_probe_owned_kernel<NW, true>), grid, dim3(256), 0, r.st, mine, ix->K, n, i, r.d_tab, r.slots - 1, rows);
                else hipLaunchKernelGGL((kidx_probe_owned_kernel<NW, false>), grid, dim3(256), 0, r.st, mine, ix->K, n, i, r.d_tab, r.slots - 1, rows);
            }))
            return rc;
        KIDX_HIP(hipEventRecord(r.e1, r.st));
    }
    // the caller's stream: behind every rank's probe, the other ranks' rows one after the other through the staging buffer, the summary
    KIDX_HIP(hipSetDevice(lead.device));
    uint64_t* rows = d_out ? d_out : lead.d_rows;
    if (n > 1 && n_kmers) if (int rc = kidx_reserve(&ix->d_staging, &ix->cap_staging, n_kmers)) return rc;
    for (uint32_t i = 0; i < n; i++) KIDX_HIP(hipStreamWaitEvent(st, ix->ranks[i].e1, 0));
    KIDX_HIP(hipEventRecord(ix->e_probed, st));
    for (uint32_t i = 1; i < n && n_kmers; i++) {
        const KidxRank& r = ix->ranks[i];
        if (r.device == lead.device) KIDX_HIP(hipMemcpyAsync(ix->d_staging, r.d_rows, n_kmers * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        else KIDX_HIP(hipMemcpyPeerAsync(ix->d_staging, lead.device, r.d_rows, r.device, n_kmers * sizeof(uint64_t), st));
        if (int rc = map_rows_merge(rows, ix->d_staging, n_kmers, st)) return rc;
    }
    KIDX_HIP(hipEventRecord(ix->e_merged, st));
    if (d_summary) {
        hipLaunchKernelGGL(kidx_summary_rows_kernel, grid_waves, dim3(256), 0, st, b, ix->K, rows, d_summary);
        KIDX_HIP(hipGetLastError());
    }
    KIDX_HIP(hipEventRecord(ix->e_end, st));
    ix->queried = true;
    return PG_OK;
}

}  // namespace

// ShardedDeviceMapEngine::build's discipline (map_kernels.hip): however the build ended, a failure on one rank leaves the others' streams
// copying out of the caller's parts and into the vectors below, so every stream is waited for before those and the buffers go
int kidx_device_build_sharded(::pg_kindex* ix, const uint64_t* const* parts, const uint64_t* part_records, const int* part_device, int n_parts,
                              void* stream) {
    const size_t n = ix->ranks.size();
    std::vector<KidxPartCount> pc((size_t)n_parts);
    std::vector<unsigned long long> bins((size_t)n_parts * n, 0);
    std::vector<uint32_t> flags(n, 0);
    const int rc = kidx_build_ranks(ix, parts, part_records, part_device, n_parts, (hipStream_t)stream, pc, bins, flags);
    if (rc) kidx_sync_ranks(ix);
    for (KidxPartCount& c : pc) {
        if (c.device < 0) continue;
        (void)hipSetDevice(c.device);
        if (rc && c.st) (void)hipStreamSynchronize(c.st);
        if (c.d_bins) (void)arena_free(c.d_bins);
        if (c.own_stream) (void)hipStreamDestroy(c.st);
    }
    for (KidxRank& r : ix->ranks) {
        if (!r.d_chunk) continue;
        (void)hipSetDevice(r.device);
        (void)arena_free(r.d_chunk);
        r.d_chunk = nullptr;
    }
    return rc;
}

int kidx_device_query_sharded(::pg_kindex* ix, const KidxBatch& b, int wave, uint64_t* d_out, uint64_t* d_summary, void* stream) {
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!b.n_seqs) return PG_OK;
    return kidx_settled(ix, kidx_query_ranks(ix, b, wave, d_out, d_summary, (hipStream_t)stream), stream);
}

// ---- the trim ----
int ktrim_device_trim(::pg_kindex* ix, const KidxBatch& b, uint32_t min_cov, uint32_t min_len, uint64_t* d_span, uint64_t* d_packed_out,
                      uint64_t* d_word_off_out, uint64_t* d_kmer_base_out, uint64_t* d_src_out, uint64_t* d_totals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint64_t n_seqs = b.n_seqs;
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!n_seqs) {
        if (d_packed_out) KIDX_HIP(hipMemsetAsync(d_totals, 0, KIDX_COUNTS * sizeof(uint64_t), st));
        return PG_OK;
    }
    dim3 grid, pack_grid;
    if (int rc = kidx_batch_blocks(n_seqs, false, &grid)) return rc;
    if (int rc = kidx_launch_blocks(b.n_words, 256, "batch too large", &pack_grid)) return rc;
    const uint64_t n_blocks = grid.x;
    // Scratch: the spans and the source indices where the caller takes none, and the workgroups' sums
    const uint64_t want = (d_span ? 0 : n_seqs) + (d_packed_out ? (d_src_out ? 0 : n_seqs) + n_blocks * KIDX_COUNTS : 0);
    if (int rc = kidx_scratch_begin(ix->trim, std::max<uint64_t>(want, 1), st)) return rc;
    uint64_t* next = ix->trim.d;
    if (!d_span) { d_span = next; next += n_seqs; }
    if (d_packed_out && !d_src_out) { d_src_out = next; next += n_seqs; }
    uint64_t* d_sums = next;
    for (hipEvent_t& e : ix->e_trim) if (!e) KIDX_HIP(hipEventCreate(&e));       // the timing marks: begin, spans done, scan done
    KIDX_HIP(hipEventRecord(ix->e_trim[0], st));
    const dim3 block(256);
    const KidxRank& lead = ix->ranks[0];
    if (!ix->cut) {
        if (int rc = kidx_launch(ix, [&](auto nw) {
                hipLaunchKernelGGL((ktrim_span_kernel<decltype(nw)::value>), grid, block, 0, st, b, ix->K, lead.d_tab, lead.slots - 1, min_cov, d_span);
            }))
            return rc;
    } else {
        // every rank probes the k-mers it owns and the lead's row buffer receives the merged answers (no counts or summary for the caller)
        if (int rc = kidx_device_query_sharded(ix, b, 0, nullptr, nullptr, stream)) return rc;
        hipLaunchKernelGGL(ktrim_span_rows_kernel, grid, block, 0, st, b, ix->K, lead.d_rows, min_cov, d_span);
        KIDX_HIP(hipGetLastError());
        KIDX_HIP(hipEventRecord(ix->e_end, st));   // the next query's ranks zero the rows: they wait for this read of them too
    }
    KIDX_HIP(hipEventRecord(ix->e_trim[1], st));
    if (d_packed_out) {
        hipLaunchKernelGGL(ktrim_block_sums_kernel, grid, block, 0, st, d_span, b, ix->K, min_len, d_sums);
        hipLaunchKernelGGL(ktrim_scan_sums_kernel, dim3(1), block, 0, st, d_sums, n_blocks, d_kmer_base_out, d_totals);
        hipLaunchKernelGGL(ktrim_scatter_kernel, grid, block, 0, st, d_span, b, ix->K, min_len, d_sums, d_word_off_out,
                           d_kmer_base_out, d_src_out);
        KIDX_HIP(hipGetLastError());
    }
    KIDX_HIP(hipEventRecord(ix->e_trim[2], st));
    if (d_packed_out) {
        hipLaunchKernelGGL(ktrim_pack_kernel, pack_grid, block, 0, st, b.packed, b.word_off, b.uniform_len, d_span, d_word_off_out, d_src_out,
                           d_totals, ix->nw + 1, b.n_words, d_packed_out);
        KIDX_HIP(hipGetLastError());
    }
    return kidx_scratch_end(ix->trim, st);
}

int ktrim_device_times(::pg_kindex* ix, double out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!ix->trim.recorded) return PG_OK;
    if (int rc = kidx_set_device(ix->device)) return rc;
    const hipEvent_t mark[4] = {ix->e_trim[0], ix->e_trim[1], ix->e_trim[2], ix->trim.e_end};
    KIDX_HIP(hipEventSynchronize(mark[3]));
    float ms = 0;
    for (int i = 0; i < 3; i++) {
        KIDX_HIP(hipEventElapsedTime(&ms, mark[i], mark[i + 1]));
        out[i] = ms;
    }
    KIDX_HIP(hipEventElapsedTime(&ms, mark[0], mark[3]));
    out[3] = ms;
    return PG_OK;
}

// ---- the unitigs ----
// What a call on the scratch of ix->uni begins with, whatever its kind: the device, the plan (kunitig.hpp: kunitig_plan), the grids over
// the slots and over the start list with their refusals, the scratch taken on the stream and bound, its leading words zeroed -- and the
// walk's covered bits.  The caller ends with kidx_scratch_end
struct KunitigCall {
    KunitigPlan plan;
    KunitigScratch s;
    dim3 slot_grid, start_grid;
};
int kunitig_call_begin(::pg_kindex* ix, KunitigKind kind, hipStream_t st, KunitigCall& c) {
    const KidxRank& t = ix->ranks[0];
    if (int rc = kidx_set_device(ix->device)) return rc;
    c.plan = kunitig_plan(t.keys, t.slots, kind);
    if (int rc = kidx_launch_blocks(t.slots, 256, "table too large", &c.slot_grid)) return rc;
    if (int rc = kidx_launch_blocks(c.plan.cap, 256, "too many starts", &c.start_grid)) return rc;
    if (int rc = kidx_scratch_begin(ix->uni, c.plan.total, st)) return rc;
    c.s = kunitig_bind(ix->uni.d, c.plan);
    KIDX_HIP(hipMemsetAsync(ix->uni.d, 0, c.plan.zero * sizeof(uint64_t), st));
    if (c.s.bits) KIDX_HIP(hipMemsetAsync(c.s.bits, 0, (t.slots + 63) / 64 * sizeof(uint64_t), st));
    return PG_OK;
}
// the scan over the start list's lengths and the finish, for both engines: two launches
int kunitig_scan(const ::pg_kindex* ix, const KunitigCall& c, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* d_packed_out, uint64_t* d_word_off_out,
                 uint64_t* d_kmer_base_out, uint64_t* d_totals, hipStream_t st) {
    hipLaunchKernelGGL(kunitig_block_sums_kernel, c.start_grid, dim3(256), 0, st, c.s, ix->K);
    hipLaunchKernelGGL(kunitig_scan_sums_kernel, dim3(1), dim3(256), 0, st, c.s, ix->K, ix->nw + 1, cap_unitigs, cap_words, d_packed_out, d_word_off_out,
                       d_kmer_base_out, d_totals);
    KIDX_HIP(hipGetLastError());
    return PG_OK;
}

// Six launches on the caller's stream and no host wait: ends, measure, rings, the scan's two, write (count mode: without the last)
int kunitig_device_unitigs(::pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* d_packed_out,
                           uint64_t* d_word_off_out, uint64_t* d_kmer_base_out, uint64_t* d_report, uint64_t* d_totals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const KidxRank& t = ix->ranks[0];
    KunitigCall c;
    if (int rc = kunitig_call_begin(ix, KUNITIG_KIND_WALK, st, c)) return rc;
    const KunitigScratch& s = c.s;
    const dim3 block(256);
    const int K = ix->K;
    const uint64_t mask = t.slots - 1;
    if (int rc = kidx_launch(ix, [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            hipLaunchKernelGGL((kunitig_ends_kernel<NW>), c.slot_grid, block, 0, st, t.d_tab, t.slots, K, pr, s);
            hipLaunchKernelGGL((kunitig_measure_kernel<NW>), c.start_grid, block, 0, st, t.d_tab, mask, K, pr, s);
            hipLaunchKernelGGL((kunitig_rings_kernel<NW>), c.slot_grid, block, 0, st, t.d_tab, t.slots, K, pr, s);
        }))
        return rc;
    if (int rc = kunitig_scan(ix, c, cap_unitigs, cap_words, d_packed_out, d_word_off_out, d_kmer_base_out, d_totals, st)) return rc;
    if (d_packed_out)
        if (int rc = kidx_launch(ix, [&](auto nw) {
                hipLaunchKernelGGL((kunitig_write_kernel<decltype(nw)::value>), c.start_grid, block, 0, st, t.d_tab, mask, K, pr, s, d_packed_out,
                                   d_word_off_out, d_kmer_base_out, d_report);
            }))
            return rc;
    return kidx_scratch_end(ix->uni, st);
}

// The unitigs by list ranking (krank.hpp): no host wait and no guard.  R = krank_rounds(keys) is all the host knows, so
// it launches 3 R rounds -- the chains', the rings' windows, the rings as chains -- and the device ends the ones with nothing to do:
// 3 R + 7 launches in count mode, 3 more in full mode.  The scratch is the unitigs' with the ranking's arrays in it
int kunitig_device_unitigs_ranked(::pg_kindex* ix, const KunitigParams& pr, uint64_t cap_unitigs, uint64_t cap_words, uint64_t* d_packed_out,
                                  uint64_t* d_word_off_out, uint64_t* d_kmer_base_out, uint64_t* d_report, uint64_t* d_totals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const KidxRank& t = ix->ranks[0];
    KunitigCall c;
    if (int rc = kunitig_call_begin(ix, KUNITIG_KIND_RANK, st, c)) return rc;
    const KunitigScratch& s = c.s;
    const KrankView v = krank_bind(ix->uni.d, c.plan);
    uint32_t* ctl = kunitig_at<uint32_t>(ix->uni.d, c.plan.ctl);
    const uint64_t words_bound = std::max<uint64_t>(std::min(cap_words, krank_words_bound(t.keys, ix->K)), 1);
    const dim3 block(256), number_grid((c.slot_grid.x + KRANK_NUMBER_EACH - 1) / KRANK_NUMBER_EACH), node_grid(std::min(c.start_grid.x, KRANK_BLOCKS)),
        word_grid((unsigned)std::min<uint64_t>((words_bound + 255) / 256, KRANK_BLOCKS));
    const int K = ix->K, tail = ix->nw + 1, R = krank_rounds(t.keys);
    if (int rc = kidx_launch(ix, [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            hipLaunchKernelGGL((krank_number_kernel<NW>), number_grid, block, 0, st, t.d_tab, t.slots, pr.min_cov, s, v);
            hipLaunchKernelGGL((krank_sweep_kernel<NW>), c.slot_grid, block, 0, st, t.d_tab, t.slots, K, pr, s, v, ctl);
            for (int j = 0; j < R; j++) hipLaunchKernelGGL(krank_jump_kernel, node_grid, block, 0, st, s, v, ctl, j);
            hipLaunchKernelGGL(krank_ring_init_kernel, node_grid, block, 0, st, s, v, ctl, R);
            for (int r = 0; r < R; r++) hipLaunchKernelGGL((krank_min_kernel<NW>), node_grid, block, 0, st, t.d_tab, s, v, ctl, R, r);
            hipLaunchKernelGGL((krank_ring_cut_kernel<NW>), node_grid, block, 0, st, t.d_tab, s, v, ctl, R);
            for (int j = R; j < 2 * R; j++) hipLaunchKernelGGL(krank_jump_kernel, node_grid, block, 0, st, s, v, ctl, j);
            hipLaunchKernelGGL((krank_measure_kernel<NW>), c.start_grid, block, 0, st, t.d_tab, K, s, v, ctl, R);
        }))
        return rc;
    if (int rc = kunitig_scan(ix, c, cap_unitigs, cap_words, d_packed_out, d_word_off_out, d_kmer_base_out, d_totals, st)) return rc;
    if (d_packed_out)
        if (int rc = kidx_launch(ix, [&](auto nw) {
                constexpr int NW = decltype(nw)::value;
                hipLaunchKernelGGL(krank_zero_kernel, word_grid, block, 0, st, s, d_totals, tail, d_packed_out);
                hipLaunchKernelGGL((krank_place_kernel<NW>), c.start_grid, block, 0, st, t.d_tab, K, s, v, ctl, R, d_word_off_out, d_kmer_base_out, d_report);
                hipLaunchKernelGGL((krank_emit_kernel<NW>), node_grid, block, 0, st, t.d_tab, K, s, v, ctl, R, d_packed_out);
            }))
            return rc;
    return kidx_scratch_end(ix->uni, st);
}

// ---- the operators that edit the graph ----
// One round of Op, four launches on the caller's stream and no host wait: the unitigs' ends sweep, decide, apply, the totals.  The scratch
// is the unitigs' -- a round and a compaction never run at once on one index, and the scratch's end event orders them across streams --
// with their counters, start list and length list and nothing else: no covered bits, no scan
template <class Op>
int kedit_device_round(::pg_kindex* ix, const typename Op::Params& pr, uint64_t* d_totals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const KidxRank& t = ix->ranks[0];
    KunitigCall c;
    if (int rc = kunitig_call_begin(ix, KUNITIG_KIND_EDIT, st, c)) return rc;
    const KunitigScratch& s = c.s;
    const dim3 block(256);
    const int K = ix->K;
    const uint64_t mask = t.slots - 1;
    if (int rc = kidx_launch(ix, [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            hipLaunchKernelGGL((kunitig_ends_kernel<NW>), c.slot_grid, block, 0, st, t.d_tab, t.slots, K, Op::ends(pr), s);
            hipLaunchKernelGGL((kedit_decide_kernel<NW, Op>), c.start_grid, block, 0, st, t.d_tab, mask, K, pr, s);
            hipLaunchKernelGGL((kedit_apply_kernel<NW, Op>), c.start_grid, block, 0, st, t.d_tab, mask, K, pr, s);
        }))
        return rc;
    hipLaunchKernelGGL(kedit_totals_kernel, dim3(1), dim3(64), 0, st, s, d_totals);
    KIDX_HIP(hipGetLastError());
    return kidx_scratch_end(ix->uni, st);
}
template int kedit_device_round<KtipOp>(::pg_kindex*, const KtipParams&, uint64_t*, void*);
template int kedit_device_round<KbubbleOp>(::pg_kindex*, const KbubbleParams&, uint64_t*, void*);
template int kedit_device_round<KarcOp>(::pg_kindex*, const KarcParams&, uint64_t*, void*);
template int kedit_device_round<KbulgeOp>(::pg_kindex*, const KbubbleParams&, uint64_t*, void*);
template int kedit_device_round<KisolatedOp>(::pg_kindex*, const KisolatedParams&, uint64_t*, void*);

// ---- the corrector on an index cut over ranks ----
namespace {

// the rounds on the caller's stream (the lead's device is current); d_packed_out already holds the batch or is about to
int kcor_rows_rounds(::pg_kindex* ix, const KidxBatch& b, const KcorParams& pr, uint64_t* d_packed_out, uint64_t* d_report, hipStream_t st,
                     uint64_t* stats) {
    const int K = ix->K;
    const uint64_t n_seqs = b.n_seqs, cap = std::min<uint64_t>(kcor_round_trials(), n_seqs);
    dim3 grid;
    if (int rc = kidx_batch_blocks(n_seqs, false, &grid)) return rc;
    // Scratch: the reads' state and bits, the round's trial reads, the claim counter, the trial batch with its readable tail, its rows
    // (where it grows the host waits: the only wait besides the one a round)
    const uint64_t w_state = n_seqs * KCOR_ROWS_STATE_WORDS, w_bits = kcor_rows_bit_words(b.n_kmers, n_seqs), w_trial = kcor_rows_batch_words(cap, K, ix->nw),
                   w_rows = cap * 3 * (uint64_t)K;
    if (int rc = kidx_scratch_begin(ix->cor, w_state + w_bits + cap + 1 + w_trial + w_rows, st)) return rc;
    uint64_t *d_state = ix->cor.d, *d_bits = d_state + w_state, *d_trial_read = d_bits + w_bits, *d_claimed = d_trial_read + cap, *d_trial = d_claimed + 1,
             *d_trial_rows = d_trial + w_trial;
    // the copy first -- pad bits and the readable tail with it -- then every read is worked on in its own words of the output
    if (d_packed_out != b.packed) KIDX_HIP(hipMemcpyAsync(d_packed_out, b.packed, b.n_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    KidxBatch o = b;
    o.packed = d_packed_out;
    const dim3 block(256);
    // the read as given: every rank probes the k-mers it owns and the lead's row buffer receives the merged answers
    if (int rc = kidx_query_ranks(ix, o, 0, nullptr, nullptr, st)) return rc;
    hipLaunchKernelGGL(kcor_rows_begin_kernel, grid, block, 0, st, o, K, ix->ranks[0].d_rows, pr.min_cov, d_state, d_bits, d_report);
    KIDX_HIP(hipGetLastError());
    KIDX_HIP(hipEventRecord(ix->e_end, st));       // the next query's ranks zero the rows: they wait for this read of them too
    for (;;) {
        unsigned long long claimed = 0;
        KIDX_HIP(hipMemsetAsync(d_claimed, 0, sizeof(uint64_t), st));
        hipLaunchKernelGGL(kcor_rows_plan_kernel, grid, block, 0, st, o, K, pr.max_fixes, d_state, d_bits, cap, (unsigned long long*)d_claimed, d_trial_read,
                           d_trial, d_report);
        KIDX_HIP(hipGetLastError());
        // the round's one wait on the host: how many trials it holds sizes the query and the decide
        KIDX_HIP(hipMemcpyAsync(&claimed, d_claimed, sizeof claimed, hipMemcpyDeviceToHost, st));
        KIDX_HIP(hipStreamSynchronize(st));
        stats[3]++;
        const uint64_t n_trials = std::min<uint64_t>(claimed, cap);
        if (!n_trials) break;
        stats[0]++;
        stats[1] += n_trials;
        stats[2] += n_trials * 3 * (uint64_t)K;
        const KidxBatch trials{d_trial, nullptr, nullptr, n_trials * 3, (uint32_t)(2 * K - 1), kcor_rows_batch_words(n_trials, K, ix->nw), n_trials * 3 * (uint64_t)K};
        if (int rc = kidx_query_ranks(ix, trials, 0, d_trial_rows, nullptr, st)) return rc;
        dim3 trial_grid;
        if (int rc = kidx_batch_blocks(n_trials, false, &trial_grid)) return rc;
        hipLaunchKernelGGL(kcor_rows_decide_kernel, trial_grid, block, 0, st, o, K, pr, n_trials, d_trial_read, d_trial_rows, d_state, d_bits, d_report);
        KIDX_HIP(hipGetLastError());
    }
    return kidx_scratch_end(ix->cor, st);
}

}  // namespace

int kcor_device_correct_rows(::pg_kindex* ix, const KidxBatch& b, const KcorParams& pr, uint64_t* d_packed_out, uint64_t* d_report, void* stream,
                             uint64_t* stats) {
    if (int rc = kidx_set_device(ix->device)) return rc;
    if (!b.n_seqs) return PG_OK;
    return kidx_settled(ix, kcor_rows_rounds(ix, b, pr, d_packed_out, d_report, (hipStream_t)stream, stats), stream);
}

int kidx_device_query_times(::pg_kindex* ix, double out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!ix->queried) return PG_OK;
    if (int rc = kidx_set_device(ix->device)) return rc;
    KIDX_HIP(hipEventSynchronize(ix->e_end));
    float ms = 0;
    for (const KidxRank& r : ix->ranks) {
        KIDX_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        out[0] = std::max(out[0], (double)ms);
    }
    KIDX_HIP(hipEventElapsedTime(&ms, ix->e_probed, ix->e_merged));
    out[1] = ms;
    KIDX_HIP(hipEventElapsedTime(&ms, ix->e_merged, ix->e_end));
    out[2] = ms;
    KIDX_HIP(hipEventElapsedTime(&ms, ix->e_begin, ix->e_end));
    out[3] = ms;
    return PG_OK;
}

void kidx_device_free(::pg_kindex* ix) {
    for (KidxScratch* s : {&ix->trim, &ix->cor, &ix->uni}) {
        if (!s->d && !s->e_end) continue;
        (void)hipSetDevice(ix->device);
        kidx_scratch_free(*s);
    }
    for (hipEvent_t& e : ix->e_trim) {             // (created behind the trim's scratch: there are none without it)
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    kidx_sync_ranks(ix);                           // every stream first: the lead's copies read the other ranks' rows
    for (KidxRank& r : ix->ranks) {
        if (!r.st && !r.d_tab && !r.d_flags) continue;   // (a build that failed before this rank began: nothing of it is on a device)
        (void)hipSetDevice(r.device);
        for (void* p : {(void*)r.d_tab, (void*)r.d_flags, (void*)r.d_chunk, (void*)r.d_packed, (void*)r.d_word_off, (void*)r.d_kmer_base, (void*)r.d_rows})
            if (p) (void)arena_free(p);            // (waits for the device like hipFree: no query still reads the table)
        if (r.st) (void)hipStreamDestroy(r.st);    // (a rank of an index in one table has no stream or events)
        for (hipEvent_t e : {r.e0, r.e1}) if (e) (void)hipEventDestroy(e);
        r = KidxRank();
    }
    if (!ix->d_staging && !ix->e_begin) return;
    (void)hipSetDevice(ix->device);
    if (ix->d_staging) (void)arena_free(ix->d_staging);
    for (hipEvent_t e : {ix->e_begin, ix->e_probed, ix->e_merged, ix->e_end}) if (e) (void)hipEventDestroy(e);
    ix->d_staging = nullptr;
    ix->e_begin = ix->e_probed = ix->e_merged = ix->e_end = nullptr;
}

}  // namespace pg

namespace {

// build(d_records, n) for a finalized context's own records: the export array where it lies, or -- the global-set engine keeps none --
// one that is made for the build and given back
template <typename F>
pg_kindex* kidx_from_ctx(const std::string& who, pg_ctx* c, void* stream, F build) {
    if (c->engine == 2) {
        const uint64_t* d_records = nullptr;
        uint64_t n = 0;
        if (pg_export_peek(c, &d_records, &n) != PG_OK) return nullptr;
        return build(d_records, n);
    }
    uint64_t n = 0, got = 0;
    if (pg_distinct(c, &n, stream) != PG_OK) return nullptr;
    uint64_t* d_records = nullptr;
    if (pg::arena_malloc(&d_records, (n ? n : 1) * (uint64_t)(c->NW + 2) * sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        pg_set_error(who + ": out of device memory for the records (PG_ENOMEM)");
        return nullptr;
    }
    pg_kindex* ix = pg_export(c, d_records, n, &got, stream) == PG_OK ? build(d_records, got) : nullptr;
    (void)pg::arena_free(d_records);
    return ix;
}

bool kidx_ctx_ready(const std::string& who, const pg_ctx* c) {
    if (!c) { pg_set_error(who + ": null context (PG_EINVAL)"); return false; }
    if (!c->finalized) { pg_set_error(who + ": call pg_finalize first (PG_ESTATE)"); return false; }
    return true;
}

}  // namespace

// pg_kindex_build for a context's own records (the host half of the ABI is kindex_host.cpp's)
extern "C" pg_kindex* pg_kindex_from_ctx(pg_ctx* c, void* stream) {
    if (!kidx_ctx_ready("pg_kindex_from_ctx", c)) return nullptr;
    return kidx_from_ctx("pg_kindex_from_ctx", c, stream,
                         [&](const uint64_t* d_records, uint64_t n) { return pg_kindex_build(c->device, c->K, c->NW == 4, d_records, n, stream); });
}

// pg_kindex_build_sharded for a context's own records: its export array as one device part
extern "C" pg_kindex* pg_kindex_from_ctx_sharded(pg_ctx* c, const int* devices, int n_devices, void* stream) {
    if (!kidx_ctx_ready("pg_kindex_from_ctx_sharded", c)) return nullptr;
    const int part_device = c->device;
    if (devices && n_devices > 0 && devices[0] != c->device && devices[0] >= 0) {
        // `stream` is the context's, on its device, and the build takes one of the lead's: the records are finished here instead
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            pg_set_error("pg_kindex_from_ctx_sharded: the context's stream could not be waited for (PG_ENODEV)");
            return nullptr;
        }
        stream = nullptr;
    }
    return kidx_from_ctx("pg_kindex_from_ctx_sharded", c, stream, [&](const uint64_t* d_records, uint64_t n) {
        return pg_kindex_build_sharded(devices, n_devices, c->K, c->NW == 4, &d_records, &n, &part_device, 1, stream);
    });
}
