// kindex_sharded_asan.cpp -- the host twin of the k-mer index cut over ranks (csrc/kindex_host.cpp), run in a program of its own so that it
// can be built with -fsanitize=address,undefined (tests/test_kindex_sharded_host.py builds and runs it; nothing loaded into Python is
// sanitised).  Both flavours: the distinct k-mers of a random genome as records in 3 heap parts of exactly their sizes, an index over 3
// ranks and one in one table, and ragged and uniform batches whose words lie on the heap with exactly NW + 1 words of tail behind the
// last sequence -- the reach read_kmer is allowed.  Every answer and summary word of the two indexes must agree, and some k-mers must be
// present and some absent.  The device engine is not linked: its entry points are stubs that fail (kindex_engine_stubs.hpp).
#include <stdint.h>

static uint64_t g_rng = 88172645463325252ull;
#include "khost_program.hpp"

// bases [at, at + len) of g packed as pg_pack_read packs them: first base in the most significant bits, 32 a word
static void pack(const std::vector<uint8_t>& g, size_t at, size_t len, uint64_t* w) {
    for (size_t i = 0; i < len; i++) w[i / 32] |= (uint64_t)g[at + i] << (62 - 2 * (i % 32));
}

template <int NW>
static void flavour(int K) {
    const int G = 3000, RW = NW + 2;
    std::vector<uint8_t> g(G);
    for (auto& b : g) b = (uint8_t)(rnd() & 3);
    // the genome's distinct canonical k-mers as records, every seventh deleted
    std::vector<uint64_t> gw((G + 31) / 32 + NW + 1, 0);
    pack(g, 0, G, gw.data());
    std::set<std::vector<uint64_t>> seen;
    std::vector<uint64_t> rec;
    pg::map_roll<NW>(gw.data(), 0, G - K + 1 - 200, K, [&](const pg::Kmer<NW>& ck, bool, int) {   // (the last 200 k-mers stay out: absent)
        std::vector<uint64_t> key(ck.w, ck.w + NW);
        if (!seen.insert(key).second) return;
        const uint64_t i = rec.size() / RW;
        rec.insert(rec.end(), key.begin(), key.end());
        rec.push_back((i & 0xffffff) | (1 + i % 255) << 24 | (i % 7 == 3 ? 1ull << (32 + 25) : 0));
        rec.push_back(i);
    });
    const uint64_t n = rec.size() / RW;
    CHECK(n > 2000);
    // three parts on the heap, each of exactly its size
    const uint64_t cut[4] = {0, n / 3, n / 3 + 257, n};
    uint64_t* part[3];
    uint64_t part_records[3];
    const int part_device[3] = {-1, -1, -1};
    for (int p = 0; p < 3; p++) {
        part_records[p] = cut[p + 1] - cut[p];
        part[p] = new uint64_t[part_records[p] * RW];
        memcpy(part[p], rec.data() + cut[p] * RW, part_records[p] * RW * sizeof(uint64_t));
    }
    uint64_t* all = new uint64_t[n * RW];
    memcpy(all, rec.data(), n * RW * sizeof(uint64_t));
    const int devices[3] = {-1, -1, -1};
    pg_kindex* cutix = pg_kindex_build_sharded(devices, 3, K, NW == 4, part, part_records, part_device, 3, nullptr);
    pg_kindex* one = pg_kindex_build(-1, K, NW == 4, all, n, nullptr);
    CHECK(cutix && one);
    for (int p = 0; p < 3; p++) delete[] part[p];                               // (the index owns its tables only)
    delete[] all;
    uint64_t info[4], total = 0;
    CHECK(pg_kindex_ranks(cutix) == 3 && pg_kindex_ranks(one) == 0);
    for (int i = 0; i < 3; i++) {
        CHECK(pg_kindex_rank_info(cutix, i, info) == PG_OK && info[0] > 0);
        total += info[0];
    }
    CHECK(total == n && pg_kindex_info(cutix, info) == PG_OK && info[0] == n);
    // a ragged batch: exactly NW + 1 words behind the last sequence, and every array of exactly its size
    const int lens[] = {K - 1, K, K + 1, 64, 65, 2 * K + 1, 0, 1000, 32 * 7, 32 * 7};
    const int at[] = {0, 5, 9, 100, 200, 300, 0, 1500, G - 224 - 100, G - 224};
    const uint64_t n_seqs = sizeof lens / sizeof lens[0];
    uint64_t *word_off = new uint64_t[n_seqs], *kmer_base = new uint64_t[n_seqs + 1];
    uint64_t n_words = 0, n_kmers = 0;
    for (uint64_t r = 0; r < n_seqs; r++) {
        word_off[r] = n_words;
        kmer_base[r] = n_kmers;
        n_words += (uint64_t)(lens[r] + 31) / 32;
        n_kmers += lens[r] >= K ? (uint64_t)(lens[r] - K + 1) : 0;
    }
    kmer_base[n_seqs] = n_kmers;
    n_words += NW + 1;
    uint64_t* packed = new uint64_t[n_words];
    memset(packed, 0, n_words * sizeof(uint64_t));
    for (uint64_t r = 0; r < n_seqs; r++) pack(g, (size_t)at[r], (size_t)lens[r], packed + word_off[r]);
    for (int q = 0; q < NW + 1; q++) packed[n_words - 1 - q] = ~0ull;           // the tail is read and never interpreted
    uint64_t *a_cnt = new uint64_t[n_kmers], *b_cnt = new uint64_t[n_kmers], *a_sum = new uint64_t[4 * n_seqs], *b_sum = new uint64_t[4 * n_seqs];
    CHECK(pg_kindex_query_words(cutix, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, 0, a_cnt, a_sum, nullptr) == PG_OK);
    CHECK(pg_kindex_query(one, packed, word_off, kmer_base, n_seqs, 0, n_kmers, 0, b_cnt, b_sum, nullptr) == PG_OK);
    CHECK(!memcmp(a_cnt, b_cnt, n_kmers * sizeof(uint64_t)) && !memcmp(a_sum, b_sum, 4 * n_seqs * sizeof(uint64_t)));
    uint64_t present = 0;
    for (uint64_t j = 0; j < n_kmers; j++) present += a_cnt[j] != 0;
    CHECK(present > 0 && present < n_kmers);
    CHECK(pg_kindex_query(cutix, packed, word_off, kmer_base, n_seqs, 0, n_kmers, 0, b_cnt, nullptr, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_correct(cutix, packed, word_off, kmer_base, n_seqs, 0, n_words, 3, 8, 4, packed, nullptr, nullptr) == PG_ESTATE);
    delete[] packed;
    delete[] word_off;
    delete[] kmer_base;
    delete[] a_cnt; delete[] b_cnt; delete[] a_sum; delete[] b_sum;
    // a uniform batch: 5 sequences of 32 * 3 bases, the last one ending at the buffer's last word but the tail
    const uint32_t L = 96;
    const uint64_t m = 5, wpr = L / 32, u_words = m * wpr + NW + 1, u_kmers = m * (uint64_t)(L - K + 1);
    uint64_t* u = new uint64_t[u_words];
    memset(u, 0, u_words * sizeof(uint64_t));
    for (uint64_t r = 0; r < m; r++) pack(g, (size_t)(400 * r + 17), L, u + r * wpr);
    uint64_t *ua = new uint64_t[u_kmers], *ub = new uint64_t[u_kmers], *us = new uint64_t[4 * m], *vs = new uint64_t[4 * m];
    CHECK(pg_kindex_query_words(cutix, u, u_words, nullptr, nullptr, m, L, u_kmers, 0, ua, us, nullptr) == PG_OK);
    CHECK(pg_kindex_query(one, u, nullptr, nullptr, m, L, u_kmers, 0, ub, vs, nullptr) == PG_OK);
    CHECK(!memcmp(ua, ub, u_kmers * sizeof(uint64_t)) && !memcmp(us, vs, 4 * m * sizeof(uint64_t)));
    CHECK(pg_kindex_query_words(cutix, u, u_words - 1, nullptr, nullptr, m, L, u_kmers, 0, ua, us, nullptr) == PG_EINVAL);
    delete[] u;
    delete[] ua; delete[] ub; delete[] us; delete[] vs;
    pg_kindex_destroy(cutix);
    pg_kindex_destroy(one);
}

int main() {
    flavour<2>(31);
    flavour<4>(65);
    printf("kindex sharded host twin: ok\n");
    return 0;
}
