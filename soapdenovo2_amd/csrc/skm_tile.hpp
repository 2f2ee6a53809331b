// skm_tile.hpp -- the per-thread pieces of the tiled super-k-mer cutter (K1, partition_kernels.hip), host + device.
//
// skm_split_read (skm.hpp) is the reference formulation: one serial walk per read.  The tiled kernel computes the same
// runs for a tile of uniform-length reads with every thread doing a short serial piece of work on consecutive positions
// (no per-k-mer shuffles, no per-k-mer control flow):
//
//   A  tile_mmer_chunk      16 consecutive m-mer values of a read from two dwords of its base string
//   B  tile_segment<S>      the sliding-window minima of S consecutive k-mers (+ their predecessor) with w + S reads:
//                           all S + 1 windows share the core [first k-mer + S - 1, first k-mer - 1 + w), so
//                           min(window j) = min(suffix-min up to the core, core, prefix-min behind the core);
//                           then partition ids and the run-start bits of the S k-mers
//      tile_put_items<S>    ... and one item per start bit -- (read, first k-mer) and the partition id -- into the tile's bounded item list
//   E  tile_item_run<S>     the run an item starts: it ends at the read's next start bit (tile_next_start), in this or a later segment
//      tile_make_record<PW> the record of a run from the dword string
// A tile whose runs outnumber its item list drops the list and is taken again in turns of ONE segment of a few reads (one lane a read:
// tile_segment and tile_put_items again, then E), few enough that a turn's items fit for certain: slower, and exactly the same runs.
//   tile_plan               the geometry of a tile for a batch's read length: segment length, row strides, item room, reads a tile
//
// Everything here is plain inline code shared with the CPU harnesses (tests/emu_skm.cpp, tests/emu_k1_items.cpp), which run the same
// phases serially and compare the records with skm_split_read + skm_make_record.
#pragma once
#include "skm.hpp"
#include "occ32.hpp"

namespace pg {

// 32 bits of a dword string (first base in the top bits of dword 0) starting at bit `bit` >= 0; d[bit/32 + 1] readable
PG_HD uint32_t dw_bits32(const uint32_t* d, int bit) {
    const int k = bit >> 5;
    const uint32_t o = (uint32_t)bit & 31u;
    const uint32_t x = alignbit32(d[k], d[k + 1], 32u - o);
    return o ? x : d[k];
}

// A: m-mer values at positions 16 c .. 16 c + 15 of one read; row = its dword string (two readable dwords behind it),
// out = its value row, which has room for 16 * ceil(np / 16) values: positions >= np get junk nobody reads, and the
// sixteen stores need no bound test.  M: the m-mer length at compile time (0: `m`).  Same values as mmer_value(rd, p, m):
// the hashed canonical m-mer, the smaller of the window's top 2 m bits and the low 2 m bits of the window's reverse complement.
// The sixteen windows are cut from the 32 bases d0:d1, and the reverse complement of that string is rc(d1):rc(d0): the
// reverse complement of window i is its bits [2 i, 2 i + 32), one funnel shift -- two rc_dword a chunk instead of sixteen
// (five instructions each: 8.6 vector instructions a read fewer at 150 bp, K = 63, and 1.3 ms of K1's 50: profiles/k1_valu_diet_ab.json).
template <int M = 0>
PG_HD void tile_mmer_chunk(const uint32_t* row, int c, int m, uint32_t* out) {
    const uint32_t d0 = row[c], d1 = row[c + 1];
    const uint32_t r0 = rc_dword(d0), r1 = rc_dword(d1);
    const int mm = M ? M : m;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t x = i ? alignbit32(d0, d1, (uint32_t)(32 - 2 * i)) : d0;
        uint32_t rc = i ? alignbit32(r1, r0, (uint32_t)(2 * i)) : r0;             // = rc_dword(x)
        const uint32_t fwd = x >> (32 - 2 * mm);
        if (mm < 16) rc &= (1u << (2 * mm)) - 1u;
        out[16 * c + i] = mmer_hash(fwd < rc ? fwd : rc);
    }
}

// B: k-mers j0 .. j0 + cnt - 1 of a read (cnt <= S <= w), v = the read's m-mer values (np of them), w m-mers a k-mer.
// Returns the run-start bits (bit i = k-mer j0 + i starts a run: first k-mer, partition change, or a multiple of nmax)
// and the partition ids in pid_out[0 .. S) (those at cnt and above are junk).
// Straight-line on purpose: every load address is clamped into the row instead of being skipped, every "does this window
// exist" is a select -- a wave runs 64 segments in lockstep, and the branchy form spent more instructions on exec masks
// than on minima.  The three parts are cut at places that depend on the segment's FIRST k-mer alone (not on cnt): window q
// = k-mer j0 - 1 + q is  [j0 - 1 + q, J)  +  [J, j0 - 1 + w)  +  [j0 - 1 + w, j0 - 1 + q + w)  with J = j0 + S - 1, so the
// middle part has w - S positions for every lane and, with W = w at compile time, all three loops unroll into loads with
// immediate offsets.
template <int S, int W = 0>
PG_HD uint32_t tile_segment(const uint32_t* v, int np, int j0, int cnt, int w_rt, int nmax, uint32_t part_mul, uint32_t* pid_out) {
    // window q = k-mer j0 - 1 + q, q = 0 .. cnt: q = 0 is the predecessor of the segment's first k-mer (none when j0 = 0),
    // wanted only for the partition comparison.  All indices below are compile-time, so the arrays stay in registers.
    const int w = W ? W : w_rt;
    const int jl = j0 - 1, J = j0 + S - 1;
    uint32_t suf[S + 1], pre[S + 1];
    suf[S] = 0xFFFFFFFFu;                                          // suf[q] = min over positions [jl + q, J)   (J - 1 < np: S <= w)
#pragma unroll
    for (int q = S - 1; q >= 0; q--) {
        const int at = jl + q;
        const uint32_t x = v[at < 0 ? 0 : at];
        const uint32_t mn = x < suf[q + 1] ? x : suf[q + 1];
        suf[q] = at >= 0 ? mn : 0xFFFFFFFFu;                       // (at < 0: q = 0 of the read's first segment, a window nobody uses)
    }
    uint32_t core = 0xFFFFFFFFu;                                   // positions [J, jl + w): inside every window of the segment
    if (W) {
#pragma unroll
        for (int i = 0; i < (W ? W - S : 0); i++) { const uint32_t x = v[J + i]; core = x < core ? x : core; }
    } else {
        for (int p = J; p < jl + w; p++) { const uint32_t x = v[p]; core = x < core ? x : core; }
    }
    pre[0] = 0xFFFFFFFFu;                                          // pre[q] = min over positions [jl + w, jl + q + w)
#pragma unroll
    for (int q = 1; q <= S; q++) {
        const int at = jl + w + q - 1;
        const uint32_t x = v[at < np ? at : np - 1];
        const uint32_t xx = q <= cnt ? x : 0xFFFFFFFFu;
        pre[q] = xx < pre[q - 1] ? xx : pre[q - 1];
    }
    uint32_t mask = 0, prev_pid = 0;
    int next_cut = 0;                                              // first multiple of nmax >= j0
    while (next_cut < j0) next_cut += nmax;
#pragma unroll
    for (int q = 0; q <= S; q++) {
        uint32_t mv = suf[q] < core ? suf[q] : core;
        mv = pre[q] < mv ? pre[q] : mv;
        const uint32_t pid = skm_partition(mv, part_mul);        // (q = 0 without a predecessor, q > cnt: junk nobody uses)
        if (q >= 1) {
            const int j = j0 + q - 1;
            const bool cut = j == next_cut;
            const bool start = (j == 0 || pid != prev_pid || cut) && q <= cnt;
            next_cut += cut ? nmax : 0;
            mask |= start ? 1u << (q - 1) : 0u;
            pid_out[q - 1] = pid;
        }
        prev_pid = pid;
    }
    return mask;
}

// B -> E: the start bits `mk` of the segment at k-mer j0 of read r as items at place `at` of the list: key = r << 24 | j << 12 (r < 256,
// j < 4096) and the partition id beside it.  Compile-time indices into pid[], so the ids stay in registers.
template <int S>
PG_HD void tile_put_items(uint32_t mk, const uint32_t* pid, int r, int j0, uint32_t at, uint32_t* keys, uint32_t* ids) {
#pragma unroll
    for (int i = 0; i < S; i++)
        if ((mk >> i) & 1u) { keys[at] = ((uint32_t)r << 24) | ((uint32_t)(j0 + i) << 12); ids[at] = pid[i]; at++; }
}
// items a read of a tile's list: 2.5 times the records a read is expected to make (2 kpr / (w + 1) + 1, as the record pool is sized), at least 8,
// at most one a k-mer.  The list is pooled over the tile's reads.
inline int tile_item_cap(int kpr, int w) {
    const int want = (int)(2.5 * (2.0 * kpr / (w + 1) + 1.0) + 0.999999);
    const int lo = want < 8 ? 8 : want;
    return lo < kpr ? lo : kpr;
}
// items of a tile's list: `cap` a read (a smaller `forced` one: the test hook PG_K1_ITEM_CAP), and never fewer than 16 -- one segment of one read
// (S <= 15 start bits) always fits, which is what the turns of an overflowed tile rely on
inline int tile_list_items(int cap, int R, int forced) {
    const int n = (forced >= 1 && forced < cap ? forced : cap) * R;
    return n < 16 ? 16 : n;
}

// D: end of the run that starts at bit i of segment `seg`: the next start bit of the read (segments seg .. nseg - 1, S
// k-mers each), or kpr.  masks = the read's segment masks.
PG_HD int tile_next_start(const uint32_t* masks, int seg, int nseg, int S, int i, int kpr) {
    const uint32_t own = masks[seg];
    const uint32_t above = i < 31 ? (own >> (i + 1)) : 0u;
    if (above) return seg * S + i + __builtin_ffs((int)above);
    for (int sg = seg + 1; sg < nseg; sg++) {
        const uint32_t mk = masks[sg];
        if (mk) return sg * S + __builtin_ffs((int)mk) - 1;
    }
    return kpr;
}

// E: the run of an item key: read r, first k-mer j0, n k-mers.  masks = the tile's start bits, mpad words a read; kpr_r = the read's k-mers.
template <int S>
PG_HD void tile_item_run(uint32_t key, const uint32_t* masks, int mpad, int nseg, int kpr_r, int& r, int& j0, int& n) {
    r = (int)(key >> 24); j0 = (int)((key >> 12) & 0xFFF);
    const int seg = j0 / S;
    n = tile_next_start(masks + r * mpad, seg, nseg, S, j0 - seg * S, kpr_r) - j0;
}

// E: the record of the run [j0, j0 + n) of a read of `len` bases given as a dword string (two zero dwords behind it).
// Same words as skm_make_record (skm.hpp).
template <int PW>
PG_HD void tile_make_record(const uint32_t* row, int len, int j0, int n, uint64_t ord0, int K, uint64_t* rec) {
    const int has_left = j0 > 0, has_right = (j0 + n - 1 + K) < len;
    const int b0 = j0 - has_left;
    const int nb = n + K - 1 + has_left + has_right;
    rec[0] = skm_header(ord0 + (uint64_t)j0, n, has_left, has_right);
#pragma unroll
    for (int i = 0; i < PW; i++) {
        const int first = 32 * i;
        uint64_t v = 0;
        if (first < nb) {
            const int bit = 2 * (b0 + first);
            v = ((uint64_t)dw_bits32(row, bit) << 32) | dw_bits32(row, bit + 32);
            const int valid = nb - first;
            if (valid < 32) v &= ~0ULL << (64 - 2 * valid);
        }
        rec[1 + i] = v;
    }
}

// segment length for a read geometry: odd (the m-mer rows are read with stride S between lanes), <= w, least padding
inline int tile_pick_segment(int kpr, int w) {
    int best = 7;
    double best_eff = -1;
    for (int s = 7; s <= 15; s += 2) {
        if (s > w && s != 7) continue;
        const int nseg = (kpr + s - 1) / s;
        const double eff = (double)kpr / (double)(nseg * s) - 0.002 * (15 - s);   // ties: the longer segment (fewer reads per k-mer)
        if (eff > best_eff) { best_eff = eff; best = s; }
    }
    return best;
}

// ---- the geometry of a tile (host side: launch_tiled; the harnesses and the GPU tests ask the same function)
// kpr / wpr / np: k-mers, 64-bit words and m-mers of the batch's (longest) read; w: m-mers a k-mer; block: threads a workgroup.
// route: the tile ranks its items by owner (a third word an item); ragged: a read's first k-mer and length beside its row.
// force_S: a segment length to take instead of the chosen one (measure builds), 0 = none.
struct TilePlan { int S, nseg, nca, npad, wsd, cap, R; size_t row_bytes; };
inline TilePlan tile_plan(int kpr, int w, int wpr, int np, bool route, bool ragged, int block, int force_S = 0) {
    TilePlan p;
    p.nca = (np + 15) / 16; p.npad = (16 * p.nca) | 1; p.wsd = (2 * wpr + 3) | 1;   // value rows: whole 16-position chunks, odd stride
    p.cap = tile_item_cap(kpr, w);
    // a read's rows: dword string, values, start bits, its share of the item list -- key, partition id, rank; ragged: first k-mer + length
    auto row_bytes = [&](int s) { return (size_t)(p.wsd + p.npad + (((kpr + s - 1) / s) | 1) + (route ? 3 : 2) * p.cap) * 4 + (ragged ? 12 : 0); };
    // About 25 KB of LDS a tile.  K1's time follows the reads a CU holds in LDS (profiles/k1_tile_life.json), which is workgroups a CU x reads a
    // tile; a CU takes 160 KB of tiles and at most 7 of these workgroups (28 waves: registers), and a tile takes at most the reads of one pass of phase B
    // (block / nseg: a second, mostly idle pass costs more than its reads bring).  Measured per 200 M reads (profiles/k1_lds_footprint_ab.json):
    //   150 bp, K = 63 (764 B a read, S = 11): 20 / 24 / 28 / 32 / 36 / 40 / 48 reads -> 56.1 / 50.5 / 47.7 / 46.7 / 54.9 / 52.5 / 54.3 ms
    //   150 bp, K = 127 (708 B a read, S = 13): 24 / 32 / 40 / 48 / 64 -> 37.0 / 31.5 / 35.1 / 37.0 / 41.4 ms
    //   100 bp, K = 31 (S = 7: 25 reads a pass; 9: 32; 15: 51): S, reads = 7, 25 / 7, 20 / 9, 28 / 9, 32 / 15, 40 / 15, 51 -> 96.8 / 95.1 / 94.0 / 91.6 / 90.8 / 93.9 ms
    // (with the per-k-mer partition ids in LDS, 1016 B a read at K = 63, the best was 24 reads and 54.7 ms: profiles/r03v_k1_tile_sizes.json)
    auto lds_reads = [&](int s) { return (int)(((25 * 1024) / row_bytes(s)) & ~(size_t)7); };
    p.S = tile_pick_segment(kpr, w);
    // The segment with the least padding may be so short that one pass of phase B holds fewer reads than the LDS target: the next longer ones then.
    // INFERRED FROM ONE SHAPE: 100 bp, K = 31, where S = 7 (25 reads a tile, 7 workgroups a CU) measured 96.8 ms against the parent's 93.5 and S = 9
    // (32 reads) 87.8 - 91.6.  Other geometries the rule moves (250 bp, K = 63: S = 9 -> 13) have not been timed; any S cuts the same records.
    while (p.S + 2 <= 15 && p.S + 2 <= w && block / ((kpr + p.S - 1) / p.S) < lds_reads(p.S)) p.S += 2;
    if (force_S) p.S = force_S;
    p.nseg = (kpr + p.S - 1) / p.S;
    p.row_bytes = row_bytes(p.S);
    p.R = block / p.nseg < 1 ? 1 : (block / p.nseg > 128 ? 128 : block / p.nseg);            // one pass of phase B per tile (the item key holds 8 bits of read)
    if ((size_t)p.R > (60 * 1024) / p.row_bytes) p.R = (int)((60 * 1024) / p.row_bytes);     // (0: the reads are too long for a tile)
    if (lds_reads(p.S) >= 8 && p.R > lds_reads(p.S)) p.R = lds_reads(p.S);
    return p;
}

}  // namespace pg
