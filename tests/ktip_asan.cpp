// ktip_asan.cpp -- the host twin of pg_kindex_clip_tips (csrc/ktip_host.cpp, csrc/ktip.hpp), run in a program of its own so that it can be
// built with -fsanitize=address,undefined (tests/test_ktip_host.py builds and runs it; nothing loaded into Python is sanitised).  Both
// flavours, two designs, each counted into records with their arc counters as pass 1 counts them and clipped by rounds to the fixed point:
//   a path read three times over with 70 reads that follow it and end in a wrong base: 70 one-k-mer tips, all gone in one round, the
//   path's last stretch -- the stronger arc into the last junction -- the one candidate kept, then one unitig;
//   a path read five times over with a tip of 12 k-mers read twice and, on its sixth k-mer, a tip of 5 read once: round 1 clips the
//   small one and keeps the far half of the large one, round 2 the large one, round 3 nothing.
// A clipped k-mer reads 0 through pg_kindex_query and its neighbours on the path as before; then the refusals, with nothing written.
// The device engine is not linked: its entry points are stubs that fail (kunitig_engine_stubs.hpp, and the tips' below).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "kunitig_engine_stubs.hpp"
#include "ktip.hpp"

namespace pg {
int ktip_device_clip(::pg_kindex*, const KtipParams&, uint64_t*, void*) { return no_device(); }
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
static Seq joined(Seq a, const Seq& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
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
static pg_kindex* build(const Counts& cnt, int K) {
    const int RW = NW + 2;
    std::vector<uint64_t> all(cnt.size() * RW);
    uint64_t i = 0;
    for (const auto& kv : cnt) {
        memcpy(all.data() + i * RW, kv.first.data(), NW * sizeof(uint64_t));
        all[i * RW + NW] = kv.second;
        all[i * RW + NW + 1] = i;
        i++;
    }
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

static void round(pg_kindex* ix, uint32_t max_tip, uint64_t tips, uint64_t kmers, uint64_t solid, uint64_t kept) {
    uint64_t* t = new uint64_t[pg::KTIP_TOTALS];
    memset(t, 0x5a, pg::KTIP_TOTALS * sizeof(uint64_t));
    CHECK(pg_kindex_clip_tips(ix, 1, 1, max_tip, t, nullptr) == PG_OK);
    CHECK(t[0] == tips && t[1] == kmers && t[2] == solid && t[3] == kept);
    delete[] t;
}

static uint64_t unitigs(pg_kindex* ix) {
    uint64_t t[8];
    CHECK(pg_kindex_unitigs(ix, 1, 1, 1u << 24, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_OK);
    return t[0];
}

template <int NW>
static void flavour(int K) {
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
        round(ix, 20, T, T, n_path + T, 1);
        for (const Seq& r : wrong) {
            const std::vector<uint64_t> v = query<NW>(ix, r, K);
            CHECK(v.size() == 5 && v[0] && v[1] && v[2] && v[3] && !v[4]);
        }
        round(ix, 20, 0, 0, n_path, 0);
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
        round(ix, 20, 1, 5, n_path + 17, 1);
        round(ix, 20, 1, 12, n_path + 12, 0);
        round(ix, 20, 0, 0, n_path, 0);
        CHECK(unitigs(ix) == 1);
        const std::vector<uint64_t> v = query<NW>(ix, t1, K);
        for (size_t j = 0; j < v.size(); j++) CHECK((v[j] != 0) == (j < 4));
        // max_tip below the tip's length: a fresh index keeps it
        pg_kindex* again = build<NW>(cnt, K);
        round(again, 4, 0, 0, n_path + 17, 0);
        round(again, 5, 1, 5, n_path + 17, 0);                                   // (the large tip's far half is 6 k-mers: no candidate at 5)
        pg_kindex_destroy(again);
        // the refusals: nothing is written
        const uint64_t n = cnt.size();
        std::vector<uint64_t> all(n * (NW + 2));
        uint64_t i = 0;
        for (const auto& kv : cnt) {
            memcpy(all.data() + i * (NW + 2), kv.first.data(), NW * sizeof(uint64_t));
            all[i * (NW + 2) + NW] = kv.second;
            i++;
        }
        const uint64_t* parts[1] = {all.data()};
        const int devices[2] = {-1, -1}, part_device[1] = {-1};
        pg_kindex* cutix = pg_kindex_build_sharded(devices, 2, K, NW == 4, parts, &n, part_device, 1, nullptr);
        CHECK(cutix);
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

int main() {
    flavour<2>(31);
    flavour<4>(65);
    printf("ktip host twin: ok\n");
    return 0;
}
