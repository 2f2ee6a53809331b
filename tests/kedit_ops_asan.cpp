// kedit_ops_asan.cpp -- the host twin of pg_kindex_drop_weak_arcs and pg_kindex_pop_bulges (csrc/kedit_ops_host.cpp; csrc/karc.hpp,
// csrc/kbulge.hpp), run in a program of its own so that it can be built with -fsanitize=address,undefined (tests/test_karc_host.py builds
// and runs it; nothing loaded into Python is sanitised).  Both flavours, two designs an operator, each counted into records with their
// arc counters as pass 1 counts them.  The arcs, at min_cov 2 and min_arc 1:
//   a path read three times over with 70 reads that follow it and end in a wrong base, each once: 70 weak k-mers, each junction's arc to
//   one of them dropped in one round, a second round finds nothing, then one unitig;
//   a path read five times over and one read with another base at one place: the fork and the join each lose one arc, three unitigs
//   become one, and the weak arm's words are untouched.
// The bulges, at 1 and 1:
//   a path read five times over and two reads with another base at places 11 apart: neither arm has a simple sibling, both go in one
//   round, then one unitig;
//   a path read five times over, a copy that differs in eight bases read twice and a copy with another base inside that window read
//   once: the inner arm and the outer weak arm go in one round.
// Then the refusals, with nothing written.  The device engine is not linked: its entry points are stubs that fail.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "kunitig_engine_stubs.hpp"
#include "karc.hpp"
#include "kbulge.hpp"

namespace pg {
template <class Op>
int kedit_device_round(::pg_kindex*, const typename Op::Params&, uint64_t*, void*) { return no_device(); }
template int kedit_device_round<KarcOp>(::pg_kindex*, const KarcParams&, uint64_t*, void*);
template int kedit_device_round<KbulgeOp>(::pg_kindex*, const KbubbleParams&, uint64_t*, void*);
}  // namespace pg

#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "line %d: %s failed: %s\n", __LINE__, #cond, pg_last_error()); exit(1); }   \
    } while (0)

typedef std::vector<uint8_t> Seq;

static const uint64_t SEED = 88172645463325252ull;
static uint64_t g_rng = SEED;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static Seq random_seq(size_t n) {
    Seq s(n);
    for (auto& b : s) b = (uint8_t)(rnd() & 3);
    return s;
}
static Seq cut(const Seq& s, size_t from, size_t to) { return Seq(s.begin() + from, s.begin() + to); }
static Seq joined(Seq a, const Seq& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
static std::vector<uint64_t> pack(const Seq& b, size_t extra) {
    std::vector<uint64_t> w((b.size() + 31) / 32 + extra, 0);
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (int)(i % 32));
    return w;
}

typedef std::map<std::vector<uint64_t>, uint64_t> Counts;

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

// one round into a heap buffer of exactly the totals
static void drop(pg_kindex* ix, uint64_t sides, uint64_t arcs, uint64_t solid, uint64_t kept) {
    uint64_t* t = new uint64_t[pg::KEDIT_TOTALS];
    memset(t, 0x5a, pg::KEDIT_TOTALS * sizeof(uint64_t));
    CHECK(pg_kindex_drop_weak_arcs(ix, 2, 1, t, nullptr) == PG_OK);
    CHECK(t[0] == sides && t[1] == arcs && t[2] == solid && t[3] == kept);
    delete[] t;
}
static void bulge(pg_kindex* ix, uint32_t max_len, uint64_t arms, uint64_t kmers, uint64_t solid) {
    uint64_t* t = new uint64_t[pg::KEDIT_TOTALS];
    memset(t, 0x5a, pg::KEDIT_TOTALS * sizeof(uint64_t));
    CHECK(pg_kindex_pop_bulges(ix, 1, 1, max_len, 0, t, nullptr) == PG_OK);
    CHECK(t[0] == arms && t[1] == kmers && t[2] == solid);
    delete[] t;
}

static uint64_t unitigs(pg_kindex* ix, uint32_t min_cov) {
    uint64_t t[8];
    CHECK(pg_kindex_unitigs(ix, min_cov, 1, 1u << 24, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_OK);
    return t[0];
}

template <int NW>
static void arcs(int K) {
    {   // 70 weak k-mers off one path
        const int T = 70, G = K + 3 * T + 10;
        const Seq g = random_seq(G);
        Counts cnt;
        count_into<NW>(cnt, g, K, 3);
        for (int i = 0; i < T; i++) {
            const int p = K + 3 + 3 * i;
            count_into<NW>(cnt, joined(cut(g, p - K - 3, p), Seq(1, (uint8_t)((g[p] + 1 + i % 3) & 3))), K, 1);
        }
        const uint64_t n_path = G - K + 1;
        CHECK(cnt.size() == n_path + T);
        pg_kindex* ix = build<NW>(cnt, K);
        CHECK(unitigs(ix, 2) > (uint64_t)T);
        drop(ix, T, T, n_path, 0);
        drop(ix, 0, 0, n_path, 0);
        CHECK(unitigs(ix, 2) == 1);
        pg_kindex_destroy(ix);
    }
    {   // a single-copy read with a substitution
        const int G = 3 * K + 90, p = K + 40;
        const Seq g = random_seq(G);
        Seq b = g;
        b[p] = (uint8_t)((g[p] + 1) & 3);
        const Seq rb = cut(b, p - K - 3, p + K + 4);
        Counts cnt;
        count_into<NW>(cnt, g, K, 5);
        count_into<NW>(cnt, rb, K, 1);
        const uint64_t n_path = G - K + 1;
        CHECK(cnt.size() == n_path + (uint64_t)K);
        pg_kindex* ix = build<NW>(cnt, K);
        const std::vector<uint64_t> before = query<NW>(ix, rb, K);
        CHECK(unitigs(ix, 2) == 3);
        drop(ix, 2, 2, n_path, 0);
        CHECK(unitigs(ix, 2) == 1);
        const std::vector<uint64_t> after = query<NW>(ix, rb, K);
        for (size_t j = 0; j < after.size(); j++) {
            const bool junction = j == 3 || j == 4 + (size_t)K;                  // (the read's fourth k-mer is the fork, the one behind the arm the join)
            CHECK(after[j] != 0 && (after[j] == before[j]) == !junction);
        }
        drop(ix, 0, 0, n_path, 0);
        // the refusals: nothing is written
        pg_kindex* cutix = build_cut<NW>(cnt, K);
        uint64_t t[4];
        memset(t, 0x5a, sizeof t);
        CHECK(pg_kindex_drop_weak_arcs(ix, 0, 1, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_drop_weak_arcs(ix, 256, 1, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_drop_weak_arcs(ix, 1, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_drop_weak_arcs(ix, 1, 64, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_drop_weak_arcs(ix, 1, 1, nullptr, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_drop_weak_arcs(nullptr, 1, 1, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_drop_weak_arcs(cutix, 1, 1, t, nullptr) == PG_ESTATE);
        for (int q = 0; q < 4; q++) CHECK(t[q] == 0x5a5a5a5a5a5a5a5aull);
        CHECK(pg_kindex_drop_weak_arcs(ix, 255, 63, t, nullptr) == PG_OK && t[0] == 0);
        pg_kindex_destroy(cutix);
        pg_kindex_destroy(ix);
    }
}

template <int NW>
static void bulges(int K) {
    const int G = 3 * K + 90, p = K + 40;
    const uint64_t n_path = G - K + 1, uK = (uint64_t)K;
    {   // two errors less than K apart on different reads
        const int q = p + 11;
        const Seq g = random_seq(G);
        Seq a = g, b = g;
        a[p] = (uint8_t)((g[p] + 1) & 3);
        b[q] = (uint8_t)((g[q] + 1) & 3);
        const Seq ra = cut(a, p - K - 3, p + K + 4), rb = cut(b, q - K - 3, q + K + 4);
        Counts cnt;
        count_into<NW>(cnt, g, K, 5);
        count_into<NW>(cnt, ra, K, 1);
        count_into<NW>(cnt, rb, K, 1);
        CHECK(cnt.size() == n_path + 2 * uK);
        pg_kindex* ix = build<NW>(cnt, K);
        CHECK(unitigs(ix, 1) > 5);                                               // (neither arm's alternative is one unitig)
        bulge(ix, K - 1, 0, 0, n_path + 2 * uK);
        bulge(ix, K, 2, 2 * uK, n_path + 2 * uK);
        for (const Seq& r : {ra, rb}) {
            const std::vector<uint64_t> v = query<NW>(ix, r, K);
            for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4 || j >= 4 + (size_t)K));
        }
        for (uint64_t w : query<NW>(ix, g, K)) CHECK(w != 0);
        bulge(ix, K, 0, 0, n_path);
        CHECK(unitigs(ix, 1) == 1);
        pg_kindex_destroy(ix);
    }
    {   // a bubble on an arm: both go in one round
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
        bulge(ix, (uint32_t)n_out, 2, n_out + uK, n_path + n_out + uK);
        bulge(ix, (uint32_t)n_out, 0, 0, n_path);
        CHECK(unitigs(ix, 1) == 1);
        // the refusals: nothing is written
        pg_kindex* cutix = build_cut<NW>(cnt, K);
        uint64_t t[4];
        memset(t, 0x5a, sizeof t);
        CHECK(pg_kindex_pop_bulges(ix, 0, 1, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 256, 1, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 1, 0, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 1, 64, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 1, 1, 0, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 1, 1, (1u << 16) + 1, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 1, 1, 20, (1u << 16) + 1, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(ix, 1, 1, 20, 0, nullptr, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(nullptr, 1, 1, 20, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_pop_bulges(cutix, 1, 1, 20, 0, t, nullptr) == PG_ESTATE);
        for (int q = 0; q < 4; q++) CHECK(t[q] == 0x5a5a5a5a5a5a5a5aull);
        CHECK(pg_kindex_pop_bulges(ix, 1, 1, 1u << 16, 1u << 16, t, nullptr) == PG_OK && t[0] == 0);
        pg_kindex_destroy(cutix);
        pg_kindex_destroy(ix);
    }
}

int main() {
    arcs<2>(31);
    arcs<4>(65);
    printf("karc host twin: ok\n");
    g_rng = SEED;
    bulges<2>(31);
    bulges<4>(65);
    printf("kbulge host twin: ok\n");
    return 0;
}
