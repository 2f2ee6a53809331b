// tests/emu_k1_items.cpp -- CPU harness for the item list of the tiled cutter (K1, skm_scatter_seg_kernel): the phases of a tile run serially
// with the inline pieces of csrc/skm_tile.hpp the kernel calls, in the kernel's order --
//   B      every segment: tile_segment, start bits, ONE reservation in the tile's item list, tile_put_items (or the overflow flag, and nothing stored)
//   ----   (the barrier)
//   E      every item: tile_item_run (tile_next_start from the item's first k-mer), tile_make_record
//   slow   a tile whose list overflowed forgets it and is taken again in turns of one segment of icap / S reads
// -- and the records of every tile compared, as a multiset of (partition id, record words), with skm_split_read + skm_make_record.
// The rows are vectors of exactly the size the kernel's LDS rows have, so the address sanitizer sees a store past the list.
// What is shared with the kernel is the tile_* helpers and tile_plan (segment length, reads a tile, item room).  The loop over turns below
// (whole / turn_seg / turn_r / gsz, the reset of the item count, the ends of the loop) is a COPY of the kernel's, as the phases in
// tests/emu_skm.cpp are: an edit to the kernel's loop has to be made here too, and only the GPU cases (tests/test_gpu_k1_items.py) run the kernel's own.
// Stand-alone program (built by tests/test_k1_items_emu.py with -fsanitize=address,undefined):
//   emu_k1_items K len n_reads R forced_cap ragged dense mer127
//     R           reads a tile; 0: what tile_plan gives for the geometry (the product's tile, with the product's segment length)
//     forced_cap  0: the list as launch_tiled sizes it; q >= 1: PG_K1_ITEM_CAP=q; -1: exactly the items of each tile (the boundary: fits);
//                 -2: one fewer than that (the boundary: overflows)
//     ragged      1: lengths from K + 1 to len
//     dense       1: reads built base by base so that as many k-mers as possible start a run
//   emu_k1_items plan K len mer127 route ragged      prints "S R cap" of tile_plan for that geometry and ends
// Prints what it ran (records a read, the densest read's starts per k-mer, tiles through the slow path) and returns 0, or a negative code's absolute value.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <array>
#include <string>
#include <vector>
#include "../soapdenovo2_amd/csrc/skm.hpp"
#include "../soapdenovo2_amd/csrc/skm_tile.hpp"

using namespace pg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rng_state >> 33); }

static void set_base(std::vector<uint64_t>& rd, int p, int b) {
    const int wd = p >> 5, sh = 62 - 2 * (p & 31);
    rd[wd] = (rd[wd] & ~(3ULL << sh)) | ((uint64_t)b << sh);
}
static int count_runs(const std::vector<uint64_t>& rd, int len, const SkmGeom& g) {
    int n = 0;
    skm_split_read(rd.data(), len, g, [&](int, int, uint32_t) { n++; });
    return n;
}

using Rec = std::array<uint64_t, 9>;          // partition id, then up to 8 record words

template <int NW, int S>
static int check(const std::vector<std::vector<uint64_t>>& reads, const std::vector<int>& lens, int len, int K, int log2_parts, int R, int forced,
                 long* n_records, long* slow_tiles) {
    constexpr int PW = NW == 2 ? 5 : 7, RW = PW + 1;
    const SkmGeom g = skm_geometry(K, log2_parts, NW);
    const int wpr = (len + 31) / 32, kpr = len - K + 1, np = len - g.m + 1;
    const int wsd = (2 * wpr + 3) | 1, nseg = (kpr + S - 1) / S, nca = (np + 15) / 16, npad = (16 * nca) | 1, mpad = nseg | 1;
    const int cap = tile_item_cap(kpr, g.w);
    const long n_reads = (long)reads.size();
    uint64_t kb = 0;
    for (long r0 = 0; r0 < n_reads; r0 += R) {
        const int nr = (int)std::min<long>(R, n_reads - r0);
        std::vector<uint32_t> dw((size_t)R * wsd, 0), v0((size_t)R * npad, 0xABABABABu), smask((size_t)R * mpad, 0xFFFFFFFFu);
        std::vector<int> rlen(nr);
        std::vector<uint64_t> rkb(nr);
        std::vector<Rec> got, want;
        for (int r = 0; r < nr; r++) {
            rlen[r] = lens[r0 + r];
            rkb[r] = kb; kb += (uint64_t)(rlen[r] - K + 1);
            for (int k = 0; k < wpr; k++) {
                const uint64_t wd = 32 * k < rlen[r] ? reads[r0 + r][k] : 0ULL;
                dw[(size_t)r * wsd + 2 * k] = (uint32_t)(wd >> 32); dw[(size_t)r * wsd + 2 * k + 1] = (uint32_t)wd;
            }
            skm_split_read(reads[r0 + r].data(), rlen[r], g, [&](int j0, int n, uint32_t pid) {
                uint64_t rec[RW];
                skm_make_record<PW>(reads[r0 + r].data(), rlen[r], j0, n, rkb[r] + 777, g, rec);
                Rec x{}; x[0] = pid; for (int k = 0; k < RW; k++) x[1 + k] = rec[k];
                want.push_back(x);
            });
        }
        for (int t = 0; t < R * nca; t++) {
            const int c = t / R, r = t % R;
            if (r < nr) tile_mmer_chunk(dw.data() + (size_t)r * wsd, c, g.m, v0.data() + (size_t)r * npad);
        }
        int icap = tile_list_items(cap, R, forced > 0 ? forced : 0);
        if (forced < 0) icap = std::max(16, (int)want.size() + (forced == -2 ? -1 : 0));
        std::vector<uint32_t> ikey(icap, 0), ipid(icap, 0);
        unsigned int n_items = 0, overflow = 0;
        const int gsz = icap / S;
        if (gsz < 1) return -201;
        int turn_seg = -1, turn_r = 0;
        for (;;) {
            const bool whole = turn_seg < 0;
            const int ntask = whole ? R * nseg : std::min(gsz, nr - turn_r);
            for (int t = 0; t < ntask; t++) {
                int seg, r;
                if (whole) { seg = t / R; r = t - seg * R; } else { seg = turn_seg; r = turn_r + t; }
                if (r >= nr) continue;
                const int j0 = seg * S, kpr_r = rlen[r] - K + 1, np_r = rlen[r] - g.m + 1, cnt = std::min(S, kpr_r - j0);
                if (cnt <= 0) { smask[(size_t)r * mpad + seg] = 0; continue; }
                uint32_t pid[S];
                const uint32_t mk = tile_segment<S>(v0.data() + (size_t)r * npad, np_r, j0, cnt, g.w, g.nmax, g.part_mul, pid);
                if (!whole && smask[(size_t)r * mpad + seg] != mk) return -202;
                smask[(size_t)r * mpad + seg] = mk;
                if (mk) {
                    const unsigned int n = (unsigned int)__builtin_popcount(mk), at = n_items;
                    n_items += n;
                    if (at + n > (unsigned int)icap) { if (!whole) return -203; overflow = 1; }
                    else tile_put_items<S>(mk, pid, r, j0, at, ikey.data(), ipid.data());
                }
            }
            const bool over = whole && overflow != 0;
            const int total = over ? 0 : (int)n_items;
            for (int it = 0; it < total; it++) {
                int r, j0, n;
                tile_item_run<S>(ikey[it], smask.data(), mpad, nseg, rlen[(int)(ikey[it] >> 24)] - K + 1, r, j0, n);
                if (r >= nr || n < 1) return -205;
                uint64_t rec[RW];
                tile_make_record<PW>(dw.data() + (size_t)r * wsd, rlen[r], j0, n, rkb[r] + 777, K, rec);
                Rec x{}; x[0] = ipid[it]; for (int k = 0; k < RW; k++) x[1 + k] = rec[k];
                got.push_back(x);
            }
            if (whole) {
                if (!over) break;
                (*slow_tiles)++;
                turn_seg = 0;
            } else {
                turn_r += gsz;
                if (turn_r >= nr) { turn_r = 0; if (++turn_seg == nseg) break; }
            }
            n_items = 0;
        }
        if (forced == -1 && overflow) return -206;                  // a list of exactly the tile's items holds them
        if (forced == -2 && (int)want.size() > 16 && !overflow) return -207;
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        if (got.size() != want.size()) return -208;
        if (got != want) return -209;
        *n_records += (long)got.size();
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && std::string(argv[1]) == "plan") {
        const int K = atoi(argv[2]), len = atoi(argv[3]);
        const SkmGeom g = skm_geometry(K, 12, atoi(argv[4]) ? 4 : 2);
        const TilePlan p = tile_plan(len - K + 1, g.w, (len + 31) / 32, len - g.m + 1, atoi(argv[5]) != 0, atoi(argv[6]) != 0, 256);
        printf("%d %d %d\n", p.S, p.R, p.cap);
        return 0;
    }
    if (argc < 9) { fprintf(stderr, "usage: %s K len n_reads R forced_cap ragged dense mer127\n", argv[0]); return 2; }
    const int K = atoi(argv[1]), len = atoi(argv[2]), n_reads = atoi(argv[3]), forced = atoi(argv[5]);
    const bool ragged = atoi(argv[6]) != 0, dense = atoi(argv[7]) != 0, mer127 = atoi(argv[8]) != 0;
    const int log2_parts = 12, wpr = (len + 31) / 32;
    const SkmGeom g = skm_geometry(K, log2_parts, mer127 ? 4 : 2);
    std::vector<std::vector<uint64_t>> reads(n_reads, std::vector<uint64_t>(wpr + 2, 0));
    std::vector<int> lens(n_reads, len);
    double densest = 0;
    for (int r = 0; r < n_reads; r++) {
        if (ragged) lens[r] = r == 0 ? K + 1 : r == 1 ? len : K + 1 + (int)(rnd() % (uint32_t)(len - K));
        auto& rd = reads[r];
        for (int p = 0; p < lens[r]; p++) {
            int b = (int)(rnd() & 3);
            if (dense && p >= K) {
                // the base that makes the k-mer it completes start a run, if one of the four does
                int best = -1;
                set_base(rd, p, 0);
                const int runs_before = count_runs(rd, p, g);          // (of the k-mers complete without base p)
                for (int q = 0; q < 4 && best < 0; q++) {
                    const int c = (b + q) & 3;
                    set_base(rd, p, c);
                    if (count_runs(rd, p + 1, g) > runs_before) best = c;
                }
                if (best >= 0) b = best;
            }
            set_base(rd, p, b);
        }
        densest = std::max(densest, (double)count_runs(rd, lens[r], g) / (lens[r] - K + 1));
    }
    long n_records = 0, slow_tiles = 0;
    int rc = -100;
    const int kpr = len - K + 1;
    // the product's segment length for this geometry (tile_plan: not always tile_pick_segment's), and its tile when R is given as 0
    const TilePlan plan = tile_plan(kpr, g.w, wpr, len - g.m + 1, false, ragged, 256);
    const int S = plan.S, R = atoi(argv[4]) > 0 ? atoi(argv[4]) : plan.R;
#define TC(NWV, SV) case SV: rc = check<NWV, SV>(reads, lens, len, K, log2_parts, R, forced, &n_records, &slow_tiles); break;
    if (mer127) switch (S) { TC(4, 7) TC(4, 9) TC(4, 11) TC(4, 13) TC(4, 15) }
    else switch (S) { TC(2, 7) TC(2, 9) TC(2, 11) TC(2, 13) TC(2, 15) }
#undef TC
    printf("K %d len %d reads %d R %d S %d cap %d forced %d: rc %d, %.2f records a read, densest read %.3f starts a k-mer, %ld of %d tiles through the slow path\n",
           K, len, n_reads, R, S, tile_item_cap(kpr, g.w), forced, rc, (double)n_records / n_reads, densest, slow_tiles, (n_reads + R - 1) / R);
    return rc ? (rc < 0 ? -rc : rc) & 255 : 0;
}
