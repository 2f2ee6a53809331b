// kunitig_ranked_asan.cpp -- the host twin of pg_kindex_unitigs_ranked (csrc/kunitig_rank_host.cpp, csrc/krank.hpp), run in a program of its
// own so that it can be built with -fsanitize=address,undefined (tests/test_kunitig_ranked_host.py builds and runs it; nothing loaded into
// Python is sanitised).  Both flavours: a random linear genome and a random circular one counted twice over into records with their arc
// counters, and a few k-mers without any arc, in one index; a count call, then the full call into heap buffers of exactly the sizes the
// count call states -- packed_out totals[1] words, word_off_out and kmer_base_out totals[0] + 1, out_report 2 totals[0] -- so that a word
// written past any of them is caught.  The unitigs are checked against the construction: the genome or its reverse complement, the ring
// once round from its least k-mer, every lone k-mer in its canonical orientation.  Then the capacities one short, each nullable output
// null, and the refusals.  The device engines are not linked: their entry points are stubs that fail.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "kindex_engine_stubs.hpp"
#include "krank.hpp"

namespace pg {
int kunitig_device_unitigs_ranked(::pg_kindex*, const KunitigParams&, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, void*) {
    return no_device();
}
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
static Seq revcomp(const Seq& s) {
    Seq r(s.rbegin(), s.rend());
    for (auto& b : r) b ^= 2;
    return r;
}
// the packed words of a sequence, pad bits zero, and `extra` zero words behind them
static std::vector<uint64_t> pack(const Seq& b, size_t extra) {
    std::vector<uint64_t> w((b.size() + 31) / 32 + extra, 0);
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (int)(i % 32));
    return w;
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

// k-mers [j0, j1) of src (len bases) counted `passes` times over with their neighbours, as pass 1 counts them
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

struct Result {
    uint64_t totals[8];
    std::multiset<Seq> texts;
    std::vector<uint64_t> reports;
};

// a count call, the full call into buffers of exactly the stated sizes, the layout checked word for word
static Result run(pg_kindex* ix, int K, int NW, uint32_t min_cov, uint32_t min_arc) {
    Result r;
    uint64_t counted[8];
    memset(counted, 0x5a, sizeof counted);
    CHECK(pg_kindex_unitigs_ranked(ix, min_cov, min_arc, 0, 0, nullptr, nullptr, nullptr, nullptr, counted, nullptr) == PG_OK);
    const uint64_t n = counted[0], words = counted[1];
    CHECK(counted[7] == 0 && words >= (uint64_t)NW + 1);
    uint64_t *packed = new uint64_t[words], *off = new uint64_t[n + 1], *base = new uint64_t[n + 1], *rep = new uint64_t[2 * n + 1];
    memset(packed, 0x5a, words * sizeof(uint64_t));
    CHECK(pg_kindex_unitigs_ranked(ix, min_cov, min_arc, n, words, packed, off, base, rep, r.totals, nullptr) == PG_OK);
    CHECK(!memcmp(counted, r.totals, sizeof counted));
    uint64_t at = 0, kmers = 0;
    for (uint64_t u = 0; u < n; u++) {
        const uint64_t len = rep[2 * u] & 0xffffffffull;
        CHECK(off[u] == at && base[u] == kmers && len >= (uint64_t)K);
        const Seq text = unpack(packed + at, len);
        const std::vector<uint64_t> again = pack(text, 0);
        CHECK(!memcmp(again.data(), packed + at, again.size() * sizeof(uint64_t)));      // pad bits zero
        r.texts.insert(text);
        r.reports.push_back(rep[2 * u]);
        at += again.size();
        kmers += len - K + 1;
    }
    CHECK(off[n] == at && base[n] == kmers && at + NW + 1 == words && kmers == r.totals[3]);
    for (int q = 0; q < NW + 1; q++) CHECK(packed[at + q] == 0);
    // one short in unitigs (where there is one) and in words: the flag, and not a word written
    for (int shorter = 0; shorter < 2; shorter++) {
        if (!shorter && !n) continue;
        uint64_t t2[8];
        memset(packed, 0x5a, words * sizeof(uint64_t));
        CHECK(pg_kindex_unitigs_ranked(ix, min_cov, min_arc, n - (shorter ? 0 : 1), words - (shorter ? 1 : 0), packed, off, base, rep, t2, nullptr) == PG_OK);
        CHECK(t2[7] == 1 && !memcmp(t2, counted, 7 * sizeof(uint64_t)));
        for (uint64_t q = 0; q < words; q++) CHECK(packed[q] == 0x5a5a5a5a5a5a5a5aull);
    }
    // each nullable output null
    CHECK(pg_kindex_unitigs_ranked(ix, min_cov, min_arc, n, words, packed, nullptr, base, rep, r.totals, nullptr) == PG_OK);
    CHECK(pg_kindex_unitigs_ranked(ix, min_cov, min_arc, n, words, packed, off, nullptr, rep, r.totals, nullptr) == PG_OK);
    CHECK(pg_kindex_unitigs_ranked(ix, min_cov, min_arc, n, words, packed, off, base, nullptr, r.totals, nullptr) == PG_OK);
    CHECK(!memcmp(counted, r.totals, sizeof counted));
    delete[] packed;
    delete[] off;
    delete[] base;
    delete[] rep;
    return r;
}

template <int NW>
static void flavour(int K) {
    const int G = 3000, C = 700, RW = NW + 2, LONE = 5;
    const Seq g = random_seq(G), c = random_seq(C);
    Counts cnt;
    count_into<NW>(cnt, g, 0, G - K + 1, K, 2);
    Seq c3(c);
    c3.insert(c3.end(), c.begin(), c.end());
    c3.insert(c3.end(), c.begin(), c.end());
    count_into<NW>(cnt, c3, C, 2 * C, K, 2);                                   // once round, every k-mer with both neighbours
    std::vector<Seq> lone;
    for (int i = 0; i < LONE; i++) {
        lone.push_back(random_seq(K));
        count_into<NW>(cnt, lone.back(), 0, 1, K, 2);
    }
    const uint64_t n = cnt.size();
    CHECK(n == (uint64_t)(G - K + 1 + C + LONE));                              // the k-mers are distinct
    uint64_t* all = new uint64_t[n * RW];
    uint64_t i = 0;
    for (const auto& kv : cnt) {
        memcpy(all + i * RW, kv.first.data(), NW * sizeof(uint64_t));
        all[i * RW + NW] = kv.second;
        all[i * RW + NW + 1] = i;
        i++;
    }
    pg_kindex* one = pg_kindex_build(-1, K, NW == 4, all, n, nullptr);
    const uint64_t* parts[1] = {all};
    const int devices[2] = {-1, -1}, part_device[1] = {-1};
    pg_kindex* cutix = pg_kindex_build_sharded(devices, 2, K, NW == 4, parts, &n, part_device, 1, nullptr);
    pg_kindex* none = pg_kindex_build(-1, K, NW == 4, nullptr, 0, nullptr);
    CHECK(one && cutix && none);
    delete[] all;
    // the ring as the rule emits it: from its least canonical k-mer, as that k-mer reads, once round
    Seq ring;
    for (const Seq& strand : {c, revcomp(c)}) {
        Seq s3(strand);
        s3.insert(s3.end(), strand.begin(), strand.end());
        s3.insert(s3.end(), strand.begin(), strand.end());
        for (int j = 0; j < C; j++) {
            const Seq k(s3.begin() + j, s3.begin() + j + K), t(s3.begin() + j, s3.begin() + j + C + K - 1);
            if (revcomp(k) < k) continue;
            if (ring.empty() || std::lexicographical_compare(k.begin(), k.end(), ring.begin(), ring.begin() + K)) ring = t;
        }
    }
    {
        const Result r = run(one, K, NW, 1, 2);
        std::multiset<Seq> want = {oriented(g, (size_t)K), ring};
        for (const Seq& s : lone) want.insert(oriented(s, (size_t)K));
        CHECK(r.texts == want);
        CHECK(r.totals[0] == (uint64_t)LONE + 2 && r.totals[4] == n && r.totals[3] == n && r.totals[5] == 1 && r.totals[6] == 0);
        CHECK(r.totals[2] == (uint64_t)G + C + K - 1 + (uint64_t)LONE * K);
        for (uint64_t w : r.reports) {
            const uint64_t left = w >> 32 & 0xff, right = w >> 40 & 0xff;
            CHECK((left == 3 && right == 3) || (left == 10 && right == 10));     // DEAD_END twice, or CYCLE twice
        }
    }
    {   // a coverage the records do not reach: nothing is solid; an arc count they do not reach: every k-mer alone
        const Result weak = run(one, K, NW, 3, 1);
        CHECK(weak.totals[0] == 0 && weak.totals[4] == 0 && weak.totals[1] == (uint64_t)NW + 1);
        const Result apart = run(one, K, NW, 1, 3);
        CHECK(apart.totals[0] == n && apart.totals[3] == n && apart.totals[2] == n * (uint64_t)K);
    }
    {   // an empty index
        const Result r = run(none, K, NW, 1, 1);
        CHECK(r.totals[0] == 0 && r.totals[1] == (uint64_t)NW + 1 && r.totals[4] == 0);
    }
    {   // the refusals: nothing is written
        uint64_t t[8];
        memset(t, 0x5a, sizeof t);
        CHECK(pg_kindex_unitigs_ranked(one, 0, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_unitigs_ranked(one, 256, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_unitigs_ranked(one, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_unitigs_ranked(one, 1, 64, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_unitigs_ranked(one, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_unitigs_ranked(nullptr, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_unitigs_ranked(cutix, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, t, nullptr) == PG_ESTATE);
        for (int q = 0; q < 8; q++) CHECK(t[q] == 0x5a5a5a5a5a5a5a5aull);
    }
    pg_kindex_destroy(none);
    pg_kindex_destroy(cutix);
    pg_kindex_destroy(one);
}

int main() {
    flavour<2>(31);
    flavour<4>(65);
    printf("kunitig ranked host twin: ok\n");
    return 0;
}
