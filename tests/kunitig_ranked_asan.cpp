// kunitig_ranked_asan.cpp -- the host twin of pg_kindex_unitigs_ranked (csrc/kunitig_rank_host.cpp, csrc/krank.hpp), run in a program of its
// own so that it can be built with -fsanitize=address,undefined (tests/test_kunitig_ranked_host.py builds and runs it; nothing loaded into
// Python is sanitised).  Both flavours: a random linear genome and a random circular one counted twice over into records with their arc
// counters, and a few k-mers without any arc, in one index; a count call, then the full call into heap buffers of exactly the sizes the
// count call states -- packed_out totals[1] words, word_off_out and kmer_base_out totals[0] + 1, out_report 2 totals[0] -- so that a word
// written past any of them is caught.  The unitigs are checked against the construction: the genome or its reverse complement, the ring
// once round from its least k-mer, every lone k-mer in its canonical orientation.  Then the capacities one short, each nullable output
// null, and the refusals.  The device engines are not linked: their entry points are stubs that fail.
#include <stdint.h>

static uint64_t g_rng = 88172645463325252ull;
#include "khost_program.hpp"

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
    const int G = 3000, C = 700, LONE = 5;
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
    pg_kindex *one = build<NW>(cnt, K), *cutix = build_cut<NW>(cnt, K), *none = pg_kindex_build(-1, K, NW == 4, nullptr, 0, nullptr);
    CHECK(none);
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

// The plan of the scratch (csrc/kunitig.hpp: kunitig_plan), for each kind: the total against the arithmetic written out here, every
// array the kind has inside the total and clear of the others, the records on an even word
static void plan(uint64_t keys, uint64_t slots, uint64_t walk, uint64_t rank, uint64_t edit) {
    const uint64_t C = 8, S = 4;
    for (int kind = 0; kind < 3; kind++) {
        const pg::KunitigPlan p = pg::kunitig_plan(keys, slots, (pg::KunitigKind)kind);
        const uint64_t cap = std::max<uint64_t>(2 * keys, kind == pg::KUNITIG_KIND_RANK ? 2 : 1), blocks = (cap + 255) / 256;
        const uint64_t want = kind == pg::KUNITIG_KIND_WALK   ? C + cap + (cap + 1) / 2 + blocks * S + (slots + 63) / 64
                              : kind == pg::KUNITIG_KIND_RANK ? C + 96 + 4 * cap + cap + (cap + 1) / 2 + blocks * S + cap / 2 + (keys + 2) / 2 + (slots + 1) / 2
                                                              : C + cap + (cap + 1) / 2;
        CHECK(p.total == want && p.total == (kind == 0 ? walk : kind == 1 ? rank : edit));
        CHECK(p.cap == cap && p.start_blocks == blocks && p.zero == (kind == pg::KUNITIG_KIND_RANK ? C + 96 : C));
        // (offset, words) of every array, the absent ones with the words they would have
        const uint64_t arrays[10][2] = {{p.ctr, C},           {p.ctl, 96},          {p.rec, 4 * cap},          {p.starts, cap},
                                        {p.lens, (cap + 1) / 2}, {p.sums, blocks * S}, {p.bits, (slots + 63) / 64}, {p.succ0, cap / 2},
                                        {p.slot_of, (keys + 2) / 2}, {p.node_of, (slots + 1) / 2}};
        const bool has[3][10] = {{1, 0, 0, 1, 1, 1, 1, 0, 0, 0}, {1, 1, 1, 1, 1, 1, 0, 1, 1, 1}, {1, 0, 0, 1, 1, 0, 0, 0, 0, 0}};
        uint64_t sum = 0;
        for (int a = 0; a < 10; a++) {
            CHECK((arrays[a][0] != pg::KUNITIG_ABSENT) == has[kind][a]);
            if (!has[kind][a]) continue;
            CHECK(arrays[a][0] + arrays[a][1] <= p.total);
            sum += arrays[a][1];
            for (int b = 0; b < a; b++)
                if (has[kind][b]) CHECK(arrays[a][0] + arrays[a][1] <= arrays[b][0] || arrays[b][0] + arrays[b][1] <= arrays[a][0]);
        }
        CHECK(sum == p.total && p.ctr == 0);
        if (kind == pg::KUNITIG_KIND_RANK) CHECK(p.rec == C + 96 && p.rec % 2 == 0);
    }
}

int main() {
    plan(0, 16, 15, 129, 10);
    plan(129, 512, 411, 1981, 395);                                            // 2 * keys = 256 + 2
    plan(1000, 4096, 3104, 14685, 3008);
    plan(128, 256, 400, 1837, 392);                                            // cap a multiple of 256
    plan(1, 2, 16, 122, 11);
    plan(383, 1024, 1185, 5416, 1157);                                         // 2 * keys = 3 * 256 - 2
    flavour<2>(31);
    flavour<4>(65);
    printf("kunitig ranked host twin: ok\n");
    return 0;
}
