// kwalk_asan.cpp -- the host twin of pg_kindex_walk (csrc/kwalk_host.cpp, csrc/kwalk.hpp), run in a program of its own so that it can be
// built with -fsanitize=address,undefined (tests/test_kwalk_host.py builds and runs it; nothing loaded into Python is sanitised).  Both
// flavours: a random linear genome counted twice over into records with their arc counters, an index in one table, a ragged and a uniform
// batch of stretches of the genome whose words lie on the heap with exactly NW + 1 words of tail (ones, like every pad bit), and the two
// output buffers on the heap at exactly the sizes the header states: 2 n_seqs rows of pg_packed_words(max_ext) words and 4 n_seqs report
// words.  Every walk is checked base by base against the genome's flanks: the k-mers are distinct, so a walk ends at the genome's end or
// at max_ext.  The device engine is not linked: its entry points are stubs that fail (kindex_engine_stubs.hpp).
#include <stdint.h>

static uint64_t g_rng = 88172645463325252ull;
#include "khost_program.hpp"

// walk v of a sequence that is bases [at, at + len) of g: its row and its report against the genome's flank
static void check_walk(const std::vector<uint8_t>& g, int K, size_t at, size_t len, bool second, uint32_t max_ext, const uint64_t* row, const uint64_t* rep) {
    const size_t row_words = (max_ext + 31) / 32;
    std::vector<uint8_t> text;
    uint32_t reason = 1;                                                      // NO_KMER
    if (len >= (size_t)K) {
        const size_t room = second ? at : g.size() - at - len, n = std::min<size_t>(room, max_ext);
        for (size_t i = 0; i < n; i++) text.push_back(second ? g[at - 1 - i] ^ 2 : g[at + len + i]);
        reason = room >= max_ext ? 8 : 3;                                     // MAX_EXT, DEAD_END
    }
    std::vector<uint64_t> want(row_words, 0);
    pack(text, want.data(), false);
    CHECK(!memcmp(want.data(), row, row_words * sizeof(uint64_t)));
    CHECK(rep[0] == ((uint64_t)text.size() | (uint64_t)reason << 32));
    CHECK(rep[1] == 2 * text.size());                                         // every k-mer was counted twice
}

template <int NW>
static void flavour(int K) {
    const int G = 3000;
    const Seq g = random_seq(G);
    // the genome read twice: every canonical k-mer with its neighbours, counted as pass 1 counts them
    Counts cnt;
    count_into<NW>(cnt, g, K, 2);
    CHECK(cnt.size() == (size_t)(G - K + 1));                                 // the k-mers are distinct
    pg_kindex *one = build<NW>(cnt, K), *cutix = build_cut<NW>(cnt, K);
    // a ragged batch: stretches of many lengths, some without a k-mer, the last one a multiple of 32 bases that ends one word before the tail
    const int lens[] = {K - 1, K, K + 1, 64, 65, 2 * K + 1, 0, 1000, 33, 97, 4 * K, 32 * 7};
    const uint64_t n_seqs = sizeof lens / sizeof lens[0];
    std::vector<size_t> at(n_seqs);
    uint64_t *word_off = new uint64_t[n_seqs], *kmer_base = new uint64_t[n_seqs + 1];
    uint64_t n_words = 0, n_kmers = 0;
    for (uint64_t r = 0; r < n_seqs; r++) {
        at[r] = r == 1 ? 0 : r == 2 ? (size_t)(G - lens[r]) : rnd() % (size_t)(G - lens[r]);   // (the genome's two ends among them)
        word_off[r] = n_words;
        kmer_base[r] = n_kmers;
        n_words += (uint64_t)(lens[r] + 31) / 32;
        n_kmers += lens[r] >= K ? (uint64_t)(lens[r] - K + 1) : 0;
    }
    kmer_base[n_seqs] = n_kmers;
    n_words += NW + 1;
    uint64_t* packed = new uint64_t[n_words];
    for (uint64_t r = 0; r < n_seqs; r++) pack(std::vector<uint8_t>(g.begin() + at[r], g.begin() + at[r] + lens[r]), packed + word_off[r], true);
    for (int q = 0; q < NW + 1; q++) packed[n_words - 1 - q] = ~0ull;         // the tail is read and never interpreted
    for (uint32_t max_ext : {1u, 31u, 32u, 33u, 65u, 4096u}) {
        const uint64_t row_words = (max_ext + 31) / 32;
        uint64_t *ext = new uint64_t[2 * n_seqs * row_words], *rep = new uint64_t[4 * n_seqs];
        memset(ext, 0x5a, 2 * n_seqs * row_words * sizeof(uint64_t));
        memset(rep, 0x5a, 4 * n_seqs * sizeof(uint64_t));
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 2, 2, max_ext, ext, rep, nullptr) == PG_OK);
        for (uint64_t v = 0; v < 2 * n_seqs; v++) check_walk(g, K, at[v / 2], (size_t)lens[v / 2], v & 1, max_ext, ext + v * row_words, rep + 2 * v);
        // either output alone: the same words
        uint64_t* rep2 = new uint64_t[4 * n_seqs];
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 2, 2, max_ext, nullptr, rep2, nullptr) == PG_OK);
        CHECK(!memcmp(rep, rep2, 4 * n_seqs * sizeof(uint64_t)));
        delete[] rep2;
        delete[] rep;
        delete[] ext;
    }
    // a coverage or an arc count the records do not reach: the seed is weak, or no arc exists
    {
        uint64_t* rep = new uint64_t[4 * n_seqs];
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 3, 1, 40, nullptr, rep, nullptr) == PG_OK);
        for (uint64_t v = 0; v < 2 * n_seqs; v++) CHECK(rep[2 * v] == (uint64_t)(lens[v / 2] >= K ? 2 : 1) << 32 && rep[2 * v + 1] == 0);
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 1, 3, 40, nullptr, rep, nullptr) == PG_OK);
        for (uint64_t v = 0; v < 2 * n_seqs; v++) CHECK(rep[2 * v] == (uint64_t)(lens[v / 2] >= K ? 3 : 1) << 32);
        // the refusals
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 0, 1, 40, nullptr, rep, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 1, 64, 40, nullptr, rep, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 1, 1, 0, nullptr, rep, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_walk(one, packed, n_words, word_off, kmer_base, n_seqs, 0, 1, 1, 40, nullptr, nullptr, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_walk(one, packed, NW, word_off, kmer_base, n_seqs, 0, 1, 1, 40, nullptr, rep, nullptr) == PG_EINVAL);
        CHECK(pg_kindex_walk(cutix, packed, n_words, word_off, kmer_base, n_seqs, 0, 1, 1, 40, nullptr, rep, nullptr) == PG_ESTATE);
        CHECK(pg_kindex_walk(one, nullptr, 0, nullptr, nullptr, 0, 0, 1, 1, 40, nullptr, rep, nullptr) == PG_OK);
        delete[] rep;
    }
    delete[] packed;
    delete[] word_off;
    delete[] kmer_base;
    // a uniform batch: 65 stretches of 32 * 3 + 5 bases, the last one ending one word before the tail
    const uint32_t L = 101, max_ext = 70;
    const uint64_t m = 65, wpr = (L + 31) / 32, u_words = m * wpr + NW + 1, row_words = (max_ext + 31) / 32;
    uint64_t* u = new uint64_t[u_words];
    for (uint64_t q = 0; q < u_words; q++) u[q] = ~0ull;
    std::vector<size_t> u_at(m);
    for (uint64_t r = 0; r < m; r++) {
        u_at[r] = rnd() % (size_t)(G - L);
        pack(std::vector<uint8_t>(g.begin() + u_at[r], g.begin() + u_at[r] + L), u + r * wpr, true);
    }
    uint64_t *ext = new uint64_t[2 * m * row_words], *rep = new uint64_t[4 * m];
    CHECK(pg_kindex_walk(one, u, u_words, nullptr, nullptr, m, L, 1, 1, max_ext, ext, rep, nullptr) == PG_OK);
    for (uint64_t v = 0; v < 2 * m; v++) check_walk(g, K, u_at[v / 2], (int)L >= K ? L : 0, v & 1, max_ext, ext + v * row_words, rep + 2 * v);
    CHECK(pg_kindex_walk(one, u, u_words - 1, nullptr, nullptr, m, L, 1, 1, max_ext, ext, rep, nullptr) == PG_EINVAL);
    delete[] ext;
    delete[] rep;
    delete[] u;
    pg_kindex_destroy(cutix);
    pg_kindex_destroy(one);
}

int main() {
    flavour<2>(31);
    flavour<4>(65);
    printf("kwalk host twin: ok\n");
    return 0;
}
