// kcorrect_rows_asan.cpp -- the host twin of pg_kindex_correct_rows (csrc/kcorrect_rows_host.cpp, csrc/kcorrect_rows.hpp), run in a
// program of its own so that it can be built with -fsanitize=address,undefined (tests/test_kcorrect_rows_host.py builds and runs it;
// nothing loaded into Python is sanitised), with a round capacity of 2.  Both flavours: the k-mers of a random genome as records, an index in
// one table and one cut over 3 ranks, a ragged and a uniform batch of reads with substitutions -- the batch's first read with one at base
// 0, its last read with one at its last base -- whose words lie on the heap with exactly NW + 1 words of tail (ones, like every pad
// bit), packed_out on the heap at exactly n_words.  The cut index's rounds must give the single table's words and reports, in place too.
// The device engine is not linked: its entry points are stubs that fail (kindex_engine_stubs.hpp).
#include <stdint.h>

static uint64_t g_rng = 88172645463325252ull;
#include "khost_program.hpp"

// one batch through both indexes: two buffers and in place, reports and words equal, something fixed, the tail untouched
static void both(pg_kindex* one, pg_kindex* cutix, int NW, const uint64_t* packed, uint64_t n_words, const uint64_t* word_off, const uint64_t* kmer_base,
                 uint64_t n_seqs, uint32_t ulen, uint64_t n_kmers) {
    const uint32_t min_cov = 3, max_fixes = 4, min_run = 5;
    uint64_t *a = new uint64_t[n_words], *b = new uint64_t[n_words], *c = new uint64_t[n_words];
    uint64_t *a_rep = new uint64_t[n_seqs], *b_rep = new uint64_t[n_seqs], *c_rep = new uint64_t[n_seqs];
    CHECK(pg_kindex_correct(one, packed, word_off, kmer_base, n_seqs, ulen, n_words, min_cov, max_fixes, min_run, a, a_rep, nullptr) == PG_OK);
    CHECK(pg_kindex_correct_rows(cutix, packed, n_words, word_off, kmer_base, n_seqs, ulen, n_kmers, min_cov, max_fixes, min_run, b, b_rep, nullptr) == PG_OK);
    memcpy(c, packed, n_words * sizeof(uint64_t));
    CHECK(pg_kindex_correct_rows(cutix, c, n_words, word_off, kmer_base, n_seqs, ulen, n_kmers, min_cov, max_fixes, min_run, c, c_rep, nullptr) == PG_OK);
    CHECK(!memcmp(a, b, n_words * sizeof(uint64_t)) && !memcmp(a, c, n_words * sizeof(uint64_t)));
    CHECK(!memcmp(a_rep, b_rep, n_seqs * sizeof(uint64_t)) && !memcmp(a_rep, c_rep, n_seqs * sizeof(uint64_t)));
    CHECK(memcmp(a, packed, n_words * sizeof(uint64_t)) != 0);
    for (int q = 0; q < NW + 1; q++) CHECK(b[n_words - 1 - q] == ~0ull);
    CHECK((a_rep[0] & 0xff) == 1 && (a_rep[n_seqs - 1] & 0xff) == 1);           // the two edge reads were fixed
    uint64_t stats[4], fixes = 0, stops = 0;
    CHECK(pg_kindex_correct_rows_stats(cutix, stats) == PG_OK);
    for (uint64_t r = 0; r < n_seqs; r++) {
        fixes += a_rep[r] & 0xff;
        stops += ((a_rep[r] & pg::KCOR_STOP_RIGHT) != 0) + ((a_rep[r] & pg::KCOR_STOP_LEFT) != 0);
    }
    CHECK(stats[1] == fixes + stops && stats[0] * 2 >= stats[1] && stats[3] == stats[0] + 1);   // (main sets a capacity of 2)
    CHECK(pg_kindex_correct_rows(one, packed, n_words, word_off, kmer_base, n_seqs, ulen, n_kmers, min_cov, max_fixes, min_run, b, b_rep, nullptr) == PG_OK);
    CHECK(!memcmp(a, b, n_words * sizeof(uint64_t)) && !memcmp(a_rep, b_rep, n_seqs * sizeof(uint64_t)));
    CHECK(pg_kindex_correct_rows(cutix, packed, n_words, word_off, kmer_base, n_seqs, ulen, n_kmers, 0, max_fixes, min_run, b, b_rep, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_correct_rows(cutix, packed, n_words, word_off, kmer_base, n_seqs, ulen, n_kmers + 1, min_cov, max_fixes, min_run, b, b_rep, nullptr) == PG_EINVAL);
    delete[] a; delete[] b; delete[] c; delete[] a_rep; delete[] b_rep; delete[] c_rep;
}

template <int NW>
static void flavour(int K) {
    const int G = 3000, RW = NW + 2;
    std::vector<uint8_t> g(G);
    for (auto& b : g) b = (uint8_t)(rnd() & 3);
    // the genome's distinct canonical k-mers as records at coverage 20
    std::vector<uint64_t> gw((G + 31) / 32 + NW + 1, 0);
    pack(g, gw.data(), true);
    std::set<std::vector<uint64_t>> seen;
    std::vector<uint64_t> rec;
    pg::map_roll<NW>(gw.data(), 0, G - K + 1, K, [&](const pg::Kmer<NW>& ck, bool, int) {
        std::vector<uint64_t> key(ck.w, ck.w + NW);
        if (!seen.insert(key).second) return;
        const uint64_t i = rec.size() / RW;
        rec.insert(rec.end(), key.begin(), key.end());
        rec.push_back((i & 0xffffff) | 20ull << 24);
        rec.push_back(i);
    });
    const uint64_t n = rec.size() / RW;
    CHECK(n > 2000);
    uint64_t* all = new uint64_t[n * RW];
    memcpy(all, rec.data(), n * RW * sizeof(uint64_t));
    const uint64_t* parts[1] = {all};
    const int devices[3] = {-1, -1, -1}, part_device[1] = {-1};
    pg_kindex* cutix = pg_kindex_build_sharded(devices, 3, K, NW == 4, parts, &n, part_device, 1, nullptr);
    pg_kindex* one = pg_kindex_build(-1, K, NW == 4, all, n, nullptr);
    CHECK(cutix && one);
    delete[] all;
    // a ragged batch: the first read's error at base 0, the last read's at its last base, between them reads of many lengths with one
    // or two substitutions anywhere
    const int lens[] = {3 * K, K - 1, K, K + 1, 64, 2 * K + 1, 0, 1000, 97, 4 * K, 32 * 7, 3 * K + 5};
    const uint64_t n_seqs = sizeof lens / sizeof lens[0];
    std::vector<std::vector<uint8_t>> reads(n_seqs);
    uint64_t *word_off = new uint64_t[n_seqs], *kmer_base = new uint64_t[n_seqs + 1];
    uint64_t n_words = 0, n_kmers = 0;
    for (uint64_t r = 0; r < n_seqs; r++) {
        const size_t at = rnd() % (size_t)(G - lens[r]);
        reads[r].assign(g.begin() + at, g.begin() + at + lens[r]);
        if (r == 0) reads[r][0] ^= 1;
        else if (r == n_seqs - 1) reads[r][(size_t)lens[r] - 1] ^= 2;
        else if (lens[r] > 2) {
            reads[r][rnd() % (size_t)lens[r]] ^= 1;
            if (r % 2) reads[r][rnd() % (size_t)lens[r]] ^= 3;
        }
        word_off[r] = n_words;
        kmer_base[r] = n_kmers;
        n_words += (uint64_t)(lens[r] + 31) / 32;
        n_kmers += lens[r] >= K ? (uint64_t)(lens[r] - K + 1) : 0;
    }
    kmer_base[n_seqs] = n_kmers;
    n_words += NW + 1;
    uint64_t* packed = new uint64_t[n_words];
    for (uint64_t r = 0; r < n_seqs; r++) pack(reads[r], packed + word_off[r], true);
    for (int q = 0; q < NW + 1; q++) packed[n_words - 1 - q] = ~0ull;
    both(one, cutix, NW, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers);
    delete[] packed;
    delete[] word_off;
    delete[] kmer_base;
    // a uniform batch: 65 reads of 3 K + 8 bases, the edge reads as above, every third of the others with a substitution
    const uint32_t L = 3 * (uint32_t)K + 8;
    const uint64_t m = 65, wpr = (L + 31) / 32, u_words = m * wpr + NW + 1, u_kmers = m * (uint64_t)(L - K + 1);
    uint64_t* u = new uint64_t[u_words];
    for (uint64_t q = 0; q < u_words; q++) u[q] = ~0ull;
    for (uint64_t r = 0; r < m; r++) {
        const size_t at = rnd() % (size_t)(G - L);
        std::vector<uint8_t> rd(g.begin() + at, g.begin() + at + L);
        if (r == 0) rd[0] ^= 2;
        else if (r == m - 1) rd[L - 1] ^= 1;
        else if (r % 3 == 1) rd[rnd() % L] ^= 2;
        pack(rd, u + r * wpr, true);
    }
    both(one, cutix, NW, u, u_words, nullptr, nullptr, m, L, u_kmers);
    delete[] u;
    pg_kindex_destroy(cutix);
    pg_kindex_destroy(one);
}

int main() {
    setenv("SOAPDENOVO2_AMD_KCOR_ROUND_TRIALS", "2", 1);   // two trials a round: reads wait for a slot
    flavour<2>(31);
    flavour<4>(65);
    printf("kcorrect rows host twin: ok\n");
    return 0;
}
