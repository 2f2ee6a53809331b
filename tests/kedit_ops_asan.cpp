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

static const uint64_t SEED = 88172645463325252ull;
static uint64_t g_rng = SEED;
#include "khost_program.hpp"

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
