// khost_program.hpp -- what the stand-alone programs that run a host twin of the k-mer index under -fsanitize=address,undefined share
// (tests/*_asan.cpp, built and run through tests/host_program.py): the stubs for the device engine (kindex_engine_stubs.hpp), CHECK, the
// generator, sequences and their packed words, k-mers counted into records as pass 1 counts them, and an index built from them.  Included
// once, by the program's one source file, behind its seed: the program defines `static uint64_t g_rng = <seed>;` first, and what it
// draws, in what order, is its own.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "kindex_engine_stubs.hpp"

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "line %d: %s failed: %s\n", __LINE__, #cond, pg_last_error()); exit(1); }   \
    } while (0)

typedef std::vector<uint8_t> Seq;

static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static Seq random_seq(size_t n) {
    Seq s(n);
    for (auto& b : s) b = (uint8_t)(rnd() & 3);
    return s;
}
static Seq revcomp(const Seq& s) {
    Seq r(s.rbegin(), s.rend());
    for (auto& b : r) b ^= 2;
    return r;
}
static Seq cut(const Seq& s, size_t from, size_t to) { return Seq(s.begin() + from, s.begin() + to); }
static Seq joined(Seq a, const Seq& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
// the packed words of a sequence (as pg_pack_read packs them: first base in the most significant bits, 32 a word), pad bits zero, and
// `extra` zero words behind them
static std::vector<uint64_t> pack(const Seq& b, size_t extra) {
    std::vector<uint64_t> w((b.size() + 31) / 32 + extra, 0);
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (int)(i % 32));
    return w;
}
// the same into words of the caller's, whose other bits become ones or zeros
static void pack(const Seq& b, uint64_t* w, bool ones) {
    const size_t nw = (b.size() + 31) / 32;
    for (size_t q = 0; q < nw; q++) w[q] = ones ? ~0ull : 0;
    for (size_t i = 0; i < b.size(); i++) {
        const int sh = 62 - 2 * (int)(i % 32);
        w[i / 32] = (w[i / 32] & ~(3ull << sh)) | (uint64_t)b[i] << sh;
    }
}
static Seq unpack(const uint64_t* w, size_t n) {
    Seq s(n);
    for (size_t i = 0; i < n; i++) s[i] = (uint8_t)(w[i / 32] >> (62 - 2 * (int)(i % 32)) & 3);
    return s;
}
// of a text and its reverse complement, the one whose first K bases are not greater
static Seq oriented(const Seq& t, size_t K) {
    const Seq r = revcomp(t);
    return std::lexicographical_compare(r.begin(), r.begin() + K, t.begin(), t.begin() + K) ? r : t;
}

typedef std::map<std::vector<uint64_t>, uint64_t> Counts;

// k-mers [j0, j1) of src counted `passes` times over with their neighbours, as pass 1 counts them; without j0 and j1, every k-mer
template <int NW>
static void count_into(Counts& cnt, const Seq& src, int j0, int j1, int K, int passes) {
    const std::vector<uint64_t> w = pack(src, NW + 1);
    const pg::Kmer<NW> filter = pg::kmer_filter<NW>(K);
    for (int pass = 0; pass < passes; pass++)
        for (int j = j0; j < j1; j++) {
            pg::Occurrence occ;
            const pg::Kmer<NW> ck = pg::canonical_occurrence<NW>(w.data(), j, (int)src.size(), K, filter, occ);
            const std::vector<uint64_t> key(ck.w, ck.w + NW);
            auto it = cnt.find(key);
            if (it == cnt.end()) cnt[key] = pg::node_first(occ.left, occ.right);
            else it->second = pg::node_update(it->second, occ.left, occ.right);
        }
}
template <int NW>
static void count_into(Counts& cnt, const Seq& src, int K, int passes) {
    count_into<NW>(cnt, src, 0, (int)src.size() - K + 1, K, passes);
}

// the counts as records in export format, on the heap at exactly their size
template <int NW>
static std::vector<uint64_t> records(const Counts& cnt) {
    const int RW = NW + 2;
    std::vector<uint64_t> all(cnt.size() * RW);
    uint64_t i = 0;
    for (const auto& kv : cnt) {
        memcpy(all.data() + i * RW, kv.first.data(), NW * sizeof(uint64_t));
        all[i * RW + NW] = kv.second;
        all[i * RW + NW + 1] = i;
        i++;
    }
    return all;
}
// an index in one table
template <int NW>
static pg_kindex* build(const Counts& cnt, int K) {
    const std::vector<uint64_t> all = records<NW>(cnt);
    pg_kindex* ix = pg_kindex_build(-1, K, NW == 4, all.data(), cnt.size(), nullptr);
    CHECK(ix);
    return ix;
}
// the same records in an index cut over two ranks, which every operator on the graph refuses
template <int NW>
static pg_kindex* build_cut(const Counts& cnt, int K) {
    const uint64_t n = cnt.size();
    const std::vector<uint64_t> all = records<NW>(cnt);
    const uint64_t* parts[1] = {all.data()};
    const int devices[2] = {-1, -1}, part_device[1] = {-1};
    pg_kindex* ix = pg_kindex_build_sharded(devices, 2, K, NW == 4, parts, &n, part_device, 1, nullptr);
    CHECK(ix);
    return ix;
}

// the cnt words of a read's k-mers, into a heap buffer of exactly that many
template <int NW>
static std::vector<uint64_t> query(pg_kindex* ix, const Seq& read, int K) {
    const std::vector<uint64_t> w = pack(read, NW + 1);
    const uint64_t nk = read.size() - K + 1;
    uint64_t* out = new uint64_t[nk];
    CHECK(pg_kindex_query(ix, w.data(), nullptr, nullptr, 1, (uint32_t)read.size(), nk, 0, out, nullptr, nullptr) == PG_OK);
    std::vector<uint64_t> v(out, out + nk);
    delete[] out;
    return v;
}
