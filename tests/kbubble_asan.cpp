// kbubble_asan.cpp -- the host twin of pg_kindex_pop_bubbles (csrc/kbubble_host.cpp, csrc/kbubble.hpp), run in a program of its own so
// that it can be built with -fsanitize=address,undefined (tests/test_kbubble_host.py builds and runs it; nothing loaded into Python is
// sanitised).  Both flavours, two designs, each counted into records with their arc counters as pass 1 counts them and popped by rounds
// to the fixed point:
//   a path read five times over with two copies that have another base at one place, read twice and once: three arms of K k-mers
//   between one fork and one join, the two weaker gone in one round, then one unitig;
//   a path read five times over, a copy that differs in eight bases read twice -- arms of K + 7 k-mers -- and a copy with another base
//   inside that window read once: round 1 pops the inner bubble's weak arm and keeps the outer one's, round 2 pops that, round 3 nothing.
// A popped k-mer reads 0 through pg_kindex_query and the path's k-mers as before; then the refusals, with nothing written.
// The device engine is not linked: its entry points are stubs that fail (kunitig_engine_stubs.hpp, and the bubbles' below).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "kunitig_engine_stubs.hpp"
#include "kbubble.hpp"

namespace pg {
int kbubble_device_pop(::pg_kindex*, const KbubbleParams&, uint64_t*, void*) { return no_device(); }
}  // namespace pg

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "line %d: %s failed: %s\n", __LINE__, #cond, pg_last_error()); exit(1); }   \
    } while (0)

typedef std::vector<uint8_t> Seq;

static uint64_t g_rng = 88172645463325252ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static Seq random_seq(size_t n) {
    Seq s(n);
    for (auto& b : s) b = (uint8_t)(rnd() & 3);
    return s;
}
static Seq cut(const Seq& s, size_t from, size_t to) { return Seq(s.begin() + from, s.begin() + to); }
// the packed words of a sequence, pad bits zero, and `extra` zero words behind them
static std::vector<uint64_t> pack(const Seq& b, size_t extra) {
    std::vector<uint64_t> w((b.size() + 31) / 32 + extra, 0);
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (int)(i % 32));
    return w;
}

typedef std::map<std::vector<uint64_t>, uint64_t> Counts;

// every k-mer of the read src counted `passes` times over with its neighbours, as pass 1 counts them
template <int NW>
static void count_into(Counts& cnt, const Seq& src, int K, int passes) {
    const std::vector<uint64_t> w = pack(src, NW + 1);
    const pg::Kmer<NW> filter = pg::kmer_filter<NW>(K);
    for (int pass = 0; pass < passes; pass++)
        for (int j = 0; j + K <= (int)src.size(); j++) {
            pg::Occurrence occ;
            const pg::Kmer<NW> ck = pg::canonical_occurrence<NW>(w.data(), j, (int)src.size(), K, filter, occ);
            const std::vector<uint64_t> key(ck.w, ck.w + NW);
            auto it = cnt.find(key);
            if (it == cnt.end()) cnt[key] = pg::node_first(occ.left, occ.right);
            else it->second = pg::node_update(it->second, occ.left, occ.right);
        }
}

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

template <int NW>
static pg_kindex* build(const Counts& cnt, int K) {
    const std::vector<uint64_t> all = records<NW>(cnt);
    pg_kindex* ix = pg_kindex_build(-1, K, NW == 4, all.data(), cnt.size(), nullptr);
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

static void round(pg_kindex* ix, uint32_t max_len, uint64_t branches, uint64_t kmers, uint64_t solid, uint64_t kept) {
    uint64_t* t = new uint64_t[pg::KBUBBLE_TOTALS];
    memset(t, 0x5a, pg::KBUBBLE_TOTALS * sizeof(uint64_t));
    CHECK(pg_kindex_pop_bubbles(ix, 1, 1, max_len, 0, t, nullptr) == PG_OK);
    CHECK(t[0] == branches && t[1] == kmers && t[2] == solid && t[3] == kept);
    delete[] t;
}

static uint64_t unitigs(pg_kindex* ix) {
    uint64_t t[8];
    CHECK(pg_kindex_unitigs(ix, 1, 1, 1u << 24, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_OK);
    return t[0];
}

template <int NW>
static void flavour(int K) {
    const int G = 3 * K + 90, p = K + 40;
    const uint64_t n_path = G - K + 1, uK = (uint64_t)K;
    {   // three arms of one bubble
        const Seq g = random_seq(G);
        Seq b = g, c = g;
        b[p] = (uint8_t)((g[p] + 1) & 3);
        c[p] = (uint8_t)((g[p] + 2) & 3);
        const Seq rb = cut(b, p - K - 3, p + K + 4), rc = cut(c, p - K - 3, p + K + 4);
        Counts cnt;
        count_into<NW>(cnt, g, K, 5);
        count_into<NW>(cnt, rb, K, 2);
        count_into<NW>(cnt, rc, K, 1);
        CHECK(cnt.size() == n_path + 2 * uK);                                     // the k-mers are distinct
        pg_kindex* ix = build<NW>(cnt, K);
        CHECK(unitigs(ix) == 5);                                                 // the path before the fork and behind the join, the three arms
        round(ix, K - 1, 0, 0, n_path + 2 * uK, 0);
        round(ix, K, 2, 2 * uK, n_path + 2 * uK, 1);
        for (const Seq& r : {rb, rc}) {
            const std::vector<uint64_t> v = query<NW>(ix, r, K);
            for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4 || j >= 4 + (size_t)K));
        }
        const std::vector<uint64_t> v = query<NW>(ix, g, K);
        for (uint64_t w : v) CHECK(w != 0);
        round(ix, K, 0, 0, n_path, 0);
        CHECK(unitigs(ix) == 1);
        pg_kindex_destroy(ix);
    }
    {   // a bubble on an arm
        const int W = 8;
        const uint64_t n_out = uK + W - 1;
        const Seq g = random_seq(G);
        Seq outer = g, inner = g;
        for (int i = 0; i < W; i++) outer[p + i] = (uint8_t)((g[p + i] + 1 + i % 3) & 3);
        inner[p + 4] = (uint8_t)((g[p + 4] + 1) & 3);
        const Seq ro = cut(outer, p - K - 3, p + W - 1 + K + 4), ri = cut(inner, p + 4 - K - 3, p + 4 + K + 4);
        Counts cnt;
        count_into<NW>(cnt, g, K, 5);
        count_into<NW>(cnt, ro, K, 2);
        count_into<NW>(cnt, ri, K, 1);
        CHECK(cnt.size() == n_path + n_out + uK);
        pg_kindex* ix = build<NW>(cnt, K);
        round(ix, (uint32_t)n_out, 1, uK, n_path + n_out + uK, 2);
        round(ix, (uint32_t)n_out, 1, n_out, n_path + n_out, 1);
        round(ix, (uint32_t)n_out, 0, 0, n_path, 0);
        CHECK(unitigs(ix) == 1);
        const std::vector<uint64_t> v = query<NW>(ix, ro, K);
        for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4 || j >= 4 + n_out));
        // max_len below the outer arms' length: a fresh index pops the inner bubble and keeps the outer one for good
        pg_kindex* again = build<NW>(cnt, K);
        round(again, K, 1, uK, n_path + n_out + uK, 1);
        round(again, K, 0, 0, n_path + n_out, 0);
        pg_kindex_destroy(again);
        // the refusals: nothing is written
        const uint64_t n = cnt.size();
        const std::vector<uint64_t> all = records<NW>(cnt);
        const uint64_t* parts[1] = {all.data()};
        const int devices[2] = {-1, -1}, part_device[1] = {-1};
        pg_kindex* cutix = pg_kindex_build_sharded(devices, 2, K, NW == 4, parts, &n, part_device, 1, nullptr);
        CHECK(cutix);
        uint64_t t[4];
        memset(t, 0x5a, sizeof t);
        CHECK(pg_kindex_pop_bubbles(ix, 0, 1, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 256, 1, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 0, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 64, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 1, 0, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 1, (1u << 16) + 1, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 1, 20, (1u << 16) + 1, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 1, 20, 0, nullptr, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(nullptr, 1, 1, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bubbles(cutix, 1, 1, 20, 0, t, nullptr) == PG_ESTATE);
        for (int q = 0; q < 4; q++) CHECK(t[q] == 0x5a5a5a5a5a5a5a5aull);
        CHECK(pg_kindex_pop_bubbles(ix, 1, 1, 1u << 16, 1u << 16, t, nullptr) == PG_OK && t[0] == 0);
        pg_kindex_destroy(cutix);
        pg_kindex_destroy(ix);
    }
}

int main() {
    flavour<2>(31);
    flavour<4>(65);
    printf("kbubble host twin: ok\n");
    return 0;
}
