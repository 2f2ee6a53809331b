// kedit_asan.cpp -- the host twin of pg_kindex_clip_tips and pg_kindex_pop_bubbles (csrc/kedit_host.cpp; csrc/ktip.hpp, csrc/kbubble.hpp),
// run in a program of its own so that it can be built with -fsanitize=address,undefined (tests/test_ktip_host.py builds and runs it;
// nothing loaded into Python is sanitised).  Both flavours, two designs an operator, each counted into records with their arc counters as
// pass 1 counts them and edited by rounds to the fixed point.  The tips:
//   a path read three times over with 70 reads that follow it and end in a wrong base: 70 one-k-mer tips, all gone in one round, the
//   path's last stretch -- the stronger arc into the last junction -- the one candidate kept, then one unitig;
//   a path read five times over with a tip of 12 k-mers read twice and, on its sixth k-mer, a tip of 5 read once: round 1 clips the
//   small one and keeps the far half of the large one, round 2 the large one, round 3 nothing.
// The bubbles:
//   a path read five times over with two copies that have another base at one place, read twice and once: three arms of K k-mers
//   between one fork and one join, the two weaker gone in one round, then one unitig;
//   a path read five times over, a copy that differs in eight bases read twice -- arms of K + 7 k-mers -- and a copy with another base
//   inside that window read once: round 1 pops the inner bubble's weak arm and keeps the outer one's, round 2 pops that, round 3 nothing.
// A removed k-mer reads 0 through pg_kindex_query and its neighbours on the path as before; then the refusals, with nothing written.
// The device engine is not linked: its entry points are stubs that fail (kindex_engine_stubs.hpp).
#include <stdint.h>

static const uint64_t SEED = 88172645463325252ull;     // every operator's designs start from it
static uint64_t g_rng = SEED;
#include "khost_program.hpp"

// one round at thresholds 1, 1 (the bubbles' at max_diff 0) into a heap buffer of exactly the totals
static void round(bool bubbles, pg_kindex* ix, uint32_t max, uint64_t removed, uint64_t kmers, uint64_t solid, uint64_t kept) {
    uint64_t* t = new uint64_t[pg::KEDIT_TOTALS];
    memset(t, 0x5a, pg::KEDIT_TOTALS * sizeof(uint64_t));
    CHECK((bubbles ? pg_kindex_pop_bubbles(ix, 1, 1, max, 0, t, nullptr) : pg_kindex_clip_tips(ix, 1, 1, max, t, nullptr)) == PG_OK);
    CHECK(t[0] == removed && t[1] == kmers && t[2] == solid && t[3] == kept);
    delete[] t;
}
static void clip(pg_kindex* ix, uint32_t max_tip, uint64_t tips, uint64_t kmers, uint64_t solid, uint64_t kept) {
    round(false, ix, max_tip, tips, kmers, solid, kept);
}
static void pop(pg_kindex* ix, uint32_t max_len, uint64_t branches, uint64_t kmers, uint64_t solid, uint64_t kept) {
    round(true, ix, max_len, branches, kmers, solid, kept);
}

static uint64_t unitigs(pg_kindex* ix) {
    uint64_t t[8];
    CHECK(pg_kindex_unitigs(ix, 1, 1, 1u << 24, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_OK);
    return t[0];
}

template <int NW>
static void tips(int K) {
    {   // 70 one-k-mer tips on one path
        const int T = 70, G = K + 3 * T + 10;
        const Seq g = random_seq(G);
        Counts cnt;
        count_into<NW>(cnt, g, K, 3);
        std::vector<Seq> wrong;
        for (int i = 0; i < T; i++) {
            const int p = K + 3 + 3 * i;
            wrong.push_back(joined(cut(g, p - K - 3, p), Seq(1, (uint8_t)((g[p] + 1 + i % 3) & 3))));
            count_into<NW>(cnt, wrong.back(), K, 1);
        }
        const uint64_t n_path = G - K + 1;
        CHECK(cnt.size() == n_path + T);                                          // the k-mers are distinct
        pg_kindex* ix = build<NW>(cnt, K);
        CHECK(unitigs(ix) > (uint64_t)T);
        clip(ix, 20, T, T, n_path + T, 1);
        for (const Seq& r : wrong) {
            const std::vector<uint64_t> v = query<NW>(ix, r, K);
            CHECK(v.size() == 5 && v[0] && v[1] && v[2] && v[3] && !v[4]);
        }
        clip(ix, 20, 0, 0, n_path, 0);
        CHECK(unitigs(ix) == 1);
        pg_kindex_destroy(ix);
    }
    {   // a tip on a tip
        const int G = 200, at = 100;
        const Seq g = random_seq(G);
        Seq s1 = random_seq(12), s2 = random_seq(5);
        s1[0] = (uint8_t)(g[at] ^ 1);
        s2[0] = (uint8_t)(s1[6] ^ 1);
        const Seq t1 = joined(cut(g, at - K - 3, at), s1), t2 = joined(cut(t1, 6, K + 9), s2);
        Counts cnt;
        count_into<NW>(cnt, g, K, 5);
        count_into<NW>(cnt, t1, K, 2);
        count_into<NW>(cnt, t2, K, 1);
        const uint64_t n_path = G - K + 1;
        CHECK(cnt.size() == n_path + 17);
        pg_kindex* ix = build<NW>(cnt, K);
        clip(ix, 20, 1, 5, n_path + 17, 1);
        clip(ix, 20, 1, 12, n_path + 12, 0);
        clip(ix, 20, 0, 0, n_path, 0);
        CHECK(unitigs(ix) == 1);
        const std::vector<uint64_t> v = query<NW>(ix, t1, K);
        for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4));
        // max_tip below the tip's length: a fresh index keeps it
        pg_kindex* again = build<NW>(cnt, K);
        clip(again, 4, 0, 0, n_path + 17, 0);
        clip(again, 5, 1, 5, n_path + 17, 0);                                    // (the large tip's far half is 6 k-mers: no candidate at 5)
        pg_kindex_destroy(again);
        // the refusals: nothing is written
        pg_kindex* cutix = build_cut<NW>(cnt, K);
        uint64_t t[4];
        memset(t, 0x5a, sizeof t);
        CHECK(pg_kindex_clip_tips(ix, 0, 1, 20, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(ix, 256, 1, 20, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(ix, 1, 0, 20, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(ix, 1, 64, 20, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(ix, 1, 1, 0, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(ix, 1, 1, (1u << 16) + 1, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(ix, 1, 1, 20, nullptr, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(nullptr, 1, 1, 20, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_clip_tips(cutix, 1, 1, 20, t, nullptr) == PG_ESTATE);
        for (int q = 0; q < 4; q++) CHECK(t[q] == 0x5a5a5a5a5a5a5a5aull);
        CHECK(pg_kindex_clip_tips(ix, 1, 1, 1u << 16, t, nullptr) == PG_OK && t[0] == 0);
        pg_kindex_destroy(cutix);
        pg_kindex_destroy(ix);
    }
}

template <int NW>
static void bubbles(int K) {
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
        pop(ix, K - 1, 0, 0, n_path + 2 * uK, 0);
        pop(ix, K, 2, 2 * uK, n_path + 2 * uK, 1);
        for (const Seq& r : {rb, rc}) {
            const std::vector<uint64_t> v = query<NW>(ix, r, K);
            for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4 || j >= 4 + (size_t)K));
        }
        const std::vector<uint64_t> v = query<NW>(ix, g, K);
        for (uint64_t w : v) CHECK(w != 0);
        pop(ix, K, 0, 0, n_path, 0);
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
        pop(ix, (uint32_t)n_out, 1, uK, n_path + n_out + uK, 2);
        pop(ix, (uint32_t)n_out, 1, n_out, n_path + n_out, 1);
        pop(ix, (uint32_t)n_out, 0, 0, n_path, 0);
        CHECK(unitigs(ix) == 1);
        const std::vector<uint64_t> v = query<NW>(ix, ro, K);
        for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4 || j >= 4 + n_out));
        // max_len below the outer arms' length: a fresh index pops the inner bubble and keeps the outer one for good
        pg_kindex* again = build<NW>(cnt, K);
        pop(again, K, 1, uK, n_path + n_out + uK, 1);
        pop(again, K, 0, 0, n_path + n_out, 0);
        pg_kindex_destroy(again);
        // the refusals: nothing is written
        pg_kindex* cutix = build_cut<NW>(cnt, K);
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
    tips<2>(31);
    tips<4>(65);
    printf("ktip host twin: ok\n");
    g_rng = SEED;
    bubbles<2>(31);
    bubbles<4>(65);
    printf("kbubble host twin: ok\n");
    return 0;
}
