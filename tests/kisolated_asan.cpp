// kisolated_asan.cpp -- the host twin of pg_kindex_drop_isolated (csrc/kisolated_host.cpp; csrc/kisolated.hpp), run in a program of its
// own so that it can be built with -fsanitize=address,undefined (tests/test_kisolated_host.py builds and runs it; nothing loaded into
// Python is sanitised).  Both flavours, two designs, each counted into records with their arc counters as pass 1 counts them, at min_cov 1
// and min_arc 1:
//   the lengths: a path read five times over and one island of n k-mers read once, n = 1 (a read of exactly K bases), 2, max_len and
//   max_len + 1, as it is and reverse complemented: untouched at max_len n - 1, then [1, n, solid, 0], its k-mers read 0 and the path's
//   are as they were, a second round finds nothing and one unitig is left;
//   what is no island: a tip and the path before its fork, a ring, a chain into a hairpin and a chain of max_len + 1 k-mers beside one
//   island: only the island goes, nothing is kept, and every other word is as it was.
// Then the coverage bound on that island, and the refusals, with nothing written.  The device engine is not linked: its entry points are
// stubs that fail, the islands' round among them.
#include <stdint.h>

static const uint64_t SEED = 88172645463325252ull;
static uint64_t g_rng = SEED;
#include "khost_program.hpp"
#include "kisolated.hpp"

namespace pg {
template int kedit_device_round<KisolatedOp>(::pg_kindex*, const KisolatedParams&, uint64_t*, void*);
}

// one round into a heap buffer of exactly the totals
static void isolated(pg_kindex* ix, uint32_t max_len, uint32_t max_cov, uint64_t islands, uint64_t kmers, uint64_t solid, uint64_t kept) {
    uint64_t* t = new uint64_t[pg::KEDIT_TOTALS];
    memset(t, 0x5a, pg::KEDIT_TOTALS * sizeof(uint64_t));
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, max_len, max_cov, t, nullptr) == PG_OK);
    CHECK(t[0] == islands && t[1] == kmers && t[2] == solid && t[3] == kept);
    delete[] t;
}

static uint64_t unitigs(pg_kindex* ix) {
    uint64_t t[8];
    CHECK(pg_kindex_unitigs(ix, 1, 1, 1u << 24, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_OK);
    return t[0];
}

template <int NW>
static void lengths(int K) {
    const int MAX_LEN = 20, G = K + 60;
    const uint64_t n_path = G - K + 1;
    const Seq g = random_seq(G);
    for (int n : {1, 2, MAX_LEN, MAX_LEN + 1})
        for (int back = 0; back < 2; back++) {
            const Seq s = random_seq(n + K - 1), read = back ? revcomp(s) : s;
            Counts cnt;
            count_into<NW>(cnt, back ? revcomp(g) : g, K, 5);
            count_into<NW>(cnt, read, K, 1);
            const uint64_t solid = n_path + (uint64_t)n;
            CHECK(cnt.size() == solid);
            pg_kindex* ix = build<NW>(cnt, K);
            const std::vector<uint64_t> path_before = query<NW>(ix, g, K);
            CHECK(unitigs(ix) == 2);
            if (n > 1) isolated(ix, (uint32_t)n - 1, 255, 0, 0, solid, 0);
            isolated(ix, (uint32_t)n, 255, 1, (uint64_t)n, solid, 0);
            for (uint64_t w : query<NW>(ix, s, K)) CHECK(w == 0);
            CHECK(query<NW>(ix, g, K) == path_before);
            isolated(ix, (uint32_t)n, 255, 0, 0, n_path, 0);
            CHECK(unitigs(ix) == 1);
            pg_kindex_destroy(ix);
        }
}

template <int NW>
static void not_islands(int K) {
    const int MAX_LEN = 64, N_ISLAND = 13, N_TIP = 5;
    // a path of K + 45 bases with a tip of 5 k-mers that leaves it behind its sixth k-mer
    const Seq fork = random_seq(K + 45 + K);
    Seq tip = cut(fork, 2, K + 5 + N_TIP);
    tip[K + 3] = (uint8_t)((tip[K + 3] + 1) & 3);                                 // (fork[K + 5], the first base behind the sixth k-mer)
    const Seq island = random_seq(N_ISLAND + K - 1), ring = random_seq(K + 150), a = random_seq(K + 8), hairpin = joined(a, revcomp(a)),
              longer = random_seq(MAX_LEN + K);
    const Seq round = joined(ring, cut(ring, 0, K + 1));                        // (once round and on: k-mers 1 .. C have both neighbours)
    Counts cnt;
    count_into<NW>(cnt, fork, K, 3);
    count_into<NW>(cnt, tip, K, 1);
    count_into<NW>(cnt, island, K, 3);
    count_into<NW>(cnt, round, 1, (int)ring.size() + 1, K, 2);
    count_into<NW>(cnt, hairpin, K, 2);
    count_into<NW>(cnt, longer, K, 3);
    const uint64_t n_hairpin = (uint64_t)(K + 8 - (K - 1) / 2);
    const uint64_t solid = (uint64_t)(K + 46) + N_TIP + N_ISLAND + ring.size() + n_hairpin + MAX_LEN + 1;
    CHECK(cnt.size() == solid);
    pg_kindex* ix = build<NW>(cnt, K);
    const std::vector<const Seq*> others = {&fork, &tip, &round, &hairpin, &longer};
    std::vector<std::vector<uint64_t>> before;
    for (const Seq* s : others) before.push_back(query<NW>(ix, *s, K));
    // the start before the fork, the tip, the path behind the fork, the island, the ring, the hairpin's chain, the long chain
    CHECK(unitigs(ix) == 7);
    isolated(ix, N_ISLAND - 1, 255, 0, 0, solid, 0);
    isolated(ix, MAX_LEN, 2, 0, 0, solid, 1);                                    // (coverage 3 a k-mer: kept, and counted)
    isolated(ix, MAX_LEN, 3, 1, N_ISLAND, solid, 0);
    for (uint64_t w : query<NW>(ix, island, K)) CHECK(w == 0);
    for (size_t i = 0; i < others.size(); i++) {
        const std::vector<uint64_t> after = query<NW>(ix, *others[i], K);
        CHECK(after == before[i]);
        for (uint64_t w : after) CHECK(w != 0);
    }
    isolated(ix, MAX_LEN, 255, 0, 0, solid - N_ISLAND, 0);
    CHECK(unitigs(ix) == 6);
    // the refusals: nothing is written
    pg_kindex* cutix = build_cut<NW>(cnt, K);
    uint64_t t[4];
    memset(t, 0x5a, sizeof t);
    CHECK(pg_kindex_drop_isolated(ix, 0, 1, 20, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 256, 1, 20, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 0, 20, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 64, 20, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, 0, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, (1u << 16) + 1, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, 20, 0, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, 20, 256, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, 20, 255, nullptr, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(nullptr, 1, 1, 20, 255, t, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_drop_isolated(cutix, 1, 1, 20, 255, t, nullptr) == PG_ESTATE);
    for (int q = 0; q < 4; q++) CHECK(t[q] == 0x5a5a5a5a5a5a5a5aull);
    for (size_t i = 0; i < others.size(); i++) CHECK(query<NW>(ix, *others[i], K) == before[i]);
    CHECK(pg_kindex_drop_isolated(ix, 255, 63, 1u << 16, 255, t, nullptr) == PG_OK && t[0] == 0 && t[2] == 0);
    // the bound itself at 1 / 1: the long chain is an island then, and the only one
    CHECK(pg_kindex_drop_isolated(ix, 1, 1, 1u << 16, 255, t, nullptr) == PG_OK && t[0] == 1 && t[1] == (uint64_t)MAX_LEN + 1 && t[3] == 0);
    pg_kindex_destroy(cutix);
    pg_kindex_destroy(ix);
}

int main() {
    lengths<2>(31);
    lengths<4>(65);
    not_islands<2>(31);
    not_islands<4>(65);
    printf("kisolated host twin: ok\n");
    return 0;
}
