// ktrim_asan.cpp -- the host twin of pg_kindex_trim (csrc/ktrim_host.cpp, csrc/ktrim.hpp), run in a program of its own so that it can be
// built with -fsanitize=address,undefined (tests/test_ktrim_host.py builds and runs it; nothing loaded into Python is sanitised).  Both
// flavours: the k-mers of a random genome as records, an index in one table and one cut over 3 ranks, a ragged and a uniform batch of
// reads with substitutions whose words lie on the heap with exactly NW + 1 words of tail (ones, like every pad bit), and every output
// buffer on the heap at exactly the capacity the header states: packed_out n_words, word_off_out and src_out n_seqs, kmer_base_out
// n_seqs + 1, out_totals 4.  The two indexes must agree word for word, and the output is checked against a base-by-base repack of the
// spans.  The device engine is not linked: its entry points are stubs that fail (kindex_engine_stubs.hpp).
#include <stdint.h>

static uint64_t g_rng = 88172645463325252ull;
#include "khost_program.hpp"

struct Out {
    uint64_t n_seqs, n_words;
    uint64_t *span, *packed, *word_off, *kmer_base, *src, *totals;
    Out(uint64_t n_seqs_, uint64_t n_words_) : n_seqs(n_seqs_), n_words(n_words_) {
        span = new uint64_t[n_seqs];
        packed = new uint64_t[n_words];
        word_off = new uint64_t[n_seqs];
        src = new uint64_t[n_seqs];
        kmer_base = new uint64_t[n_seqs + 1];
        totals = new uint64_t[4];
        memset(packed, 0x5a, n_words * sizeof(uint64_t));
    }
    ~Out() { delete[] span; delete[] packed; delete[] word_off; delete[] kmer_base; delete[] src; delete[] totals; }
};

static bool same(const Out& a, const Out& b) {
    const uint64_t kept = a.totals[0], words = a.totals[1];
    return !memcmp(a.totals, b.totals, 4 * sizeof(uint64_t)) && !memcmp(a.span, b.span, a.n_seqs * sizeof(uint64_t)) &&
           !memcmp(a.word_off, b.word_off, kept * sizeof(uint64_t)) && !memcmp(a.src, b.src, kept * sizeof(uint64_t)) &&
           !memcmp(a.kmer_base, b.kmer_base, (kept + 1) * sizeof(uint64_t)) && !memcmp(a.packed, b.packed, words * sizeof(uint64_t));
}

template <int NW>
static void flavour(int K) {
    const int G = 3000, RW = NW + 2;
    const uint32_t min_cov = 3, min_len = (uint32_t)K + 1;
    std::vector<uint8_t> g(G);
    for (auto& b : g) b = (uint8_t)(rnd() & 3);
    // the genome's distinct canonical k-mers as records: every eleventh below min_cov, every seventh deleted
    std::vector<uint64_t> gw((G + 31) / 32 + NW + 1, 0);
    pack(g, gw.data(), false);
    std::set<std::vector<uint64_t>> seen;
    std::vector<uint64_t> rec;
    pg::map_roll<NW>(gw.data(), 0, G - K + 1, K, [&](const pg::Kmer<NW>& ck, bool, int) {
        std::vector<uint64_t> key(ck.w, ck.w + NW);
        if (!seen.insert(key).second) return;
        const uint64_t i = rec.size() / RW;
        rec.insert(rec.end(), key.begin(), key.end());
        rec.push_back((i & 0xffffff) | (uint64_t)(i % 11 == 5 ? min_cov - 1 : min_cov + i % 50) << 24 | (i % 7 == 3 ? 1ull << (32 + 25) : 0));
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
    // a ragged batch: reads of many lengths with a substitution here and there, the last one a multiple of 32 bases that is solid to its end
    const int lens[] = {K - 1, K, K + 1, 64, 65, 2 * K + 1, 0, 1000, 33, 97, 4 * K, 32 * 7, 32 * 7};
    const uint64_t n_seqs = sizeof lens / sizeof lens[0];
    std::vector<std::vector<uint8_t>> reads(n_seqs);
    uint64_t *word_off = new uint64_t[n_seqs], *kmer_base = new uint64_t[n_seqs + 1];
    uint64_t n_words = 0, n_kmers = 0;
    for (uint64_t r = 0; r < n_seqs; r++) {
        const size_t at = rnd() % (size_t)(G - lens[r]);
        reads[r].assign(g.begin() + at, g.begin() + at + lens[r]);
        if (r % 3 == 1 && lens[r] > 2) reads[r][rnd() % (size_t)lens[r]] ^= 1;
        word_off[r] = n_words;
        kmer_base[r] = n_kmers;
        n_words += (uint64_t)(lens[r] + 31) / 32;
        n_kmers += lens[r] >= K ? (uint64_t)(lens[r] - K + 1) : 0;
    }
    kmer_base[n_seqs] = n_kmers;
    n_words += NW + 1;
    uint64_t* packed = new uint64_t[n_words];
    for (uint64_t r = 0; r < n_seqs; r++) pack(reads[r], packed + word_off[r], true);
    for (int q = 0; q < NW + 1; q++) packed[n_words - 1 - q] = ~0ull;           // the tail is read and never interpreted
    Out a(n_seqs, n_words), b(n_seqs, n_words);
    CHECK(pg_kindex_trim(one, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, min_cov, min_len, a.span, a.packed, a.word_off, a.kmer_base,
                         a.src, a.totals, nullptr) == PG_OK);
    CHECK(pg_kindex_trim(cutix, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, min_cov, min_len, b.span, b.packed, b.word_off, b.kmer_base,
                         b.src, b.totals, nullptr) == PG_OK);
    CHECK(same(a, b));
    CHECK(a.totals[0] > 0 && a.totals[0] < n_seqs && a.totals[3] > 0);
    // the output against a base-by-base repack of every kept read's span; the tail is zero; what lies behind it was not touched
    uint64_t kept = 0, words = 0, kmers = 0;
    for (uint64_t r = 0; r < n_seqs; r++) {
        const uint32_t start = (uint32_t)a.span[r], len = (uint32_t)(a.span[r] >> 32);
        CHECK((uint64_t)start + len <= reads[r].size());
        if (len < min_len) continue;
        CHECK(a.src[kept] == r && a.word_off[kept] == words && a.kmer_base[kept] == kmers);
        std::vector<uint8_t> cut(reads[r].begin() + start, reads[r].begin() + start + len);
        std::vector<uint64_t> w((len + 31) / 32);
        pack(cut, w.data(), false);
        CHECK(!memcmp(w.data(), a.packed + words, w.size() * sizeof(uint64_t)));
        kept++;
        words += w.size();
        kmers += len - (uint32_t)K + 1;
    }
    CHECK(a.totals[0] == kept && a.totals[1] == words && a.totals[2] == kmers && a.kmer_base[kept] == kmers);
    for (uint64_t q = words; q < n_words; q++) CHECK(a.packed[q] == (q < words + NW + 1 ? 0 : 0x5a5a5a5a5a5a5a5aull));
    // spans only, and the refusals
    CHECK(pg_kindex_trim(cutix, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, min_cov, min_len, b.span, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr) == PG_OK && !memcmp(a.span, b.span, n_seqs * sizeof(uint64_t)));
    CHECK(pg_kindex_trim(one, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, 0, min_len, a.span, a.packed, a.word_off, a.kmer_base, a.src,
                         a.totals, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_trim(one, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, min_cov, (uint32_t)K - 1, a.span, a.packed, a.word_off,
                         a.kmer_base, a.src, a.totals, nullptr) == PG_EINVAL);
    CHECK(pg_kindex_trim(one, packed, n_words, word_off, kmer_base, n_seqs, 0, n_kmers, min_cov, min_len, a.span, packed, a.word_off, a.kmer_base,
                         a.src, a.totals, nullptr) == PG_EINVAL);
    delete[] packed;
    delete[] word_off;
    delete[] kmer_base;
    // a uniform batch: 65 reads of 32 * 3 + 5 bases, every fourth with a substitution, the last one ending one word before the tail
    const uint32_t L = 101;
    const uint64_t m = 65, wpr = (L + 31) / 32, u_words = m * wpr + NW + 1, u_kmers = (int)L >= K ? m * (uint64_t)(L - K + 1) : 0;
    uint64_t* u = new uint64_t[u_words];
    for (uint64_t q = 0; q < u_words; q++) u[q] = ~0ull;
    for (uint64_t r = 0; r < m; r++) {
        const size_t at = rnd() % (size_t)(G - L);
        std::vector<uint8_t> rd(g.begin() + at, g.begin() + at + L);
        if (r % 4 == 2) rd[rnd() % L] ^= 2;
        pack(rd, u + r * wpr, true);
    }
    Out ua(m, u_words), ub(m, u_words);
    CHECK(pg_kindex_trim(one, u, u_words, nullptr, nullptr, m, L, u_kmers, min_cov, min_len, ua.span, ua.packed, ua.word_off, ua.kmer_base, nullptr,
                         ua.totals, nullptr) == PG_OK);
    CHECK(pg_kindex_trim(cutix, u, u_words, nullptr, nullptr, m, L, u_kmers, min_cov, min_len, nullptr, ub.packed, ub.word_off, ub.kmer_base, ub.src,
                         ub.totals, nullptr) == PG_OK);
    memcpy(ub.span, ua.span, m * sizeof(uint64_t));                              // (the one call took no source indices, the other no spans)
    memcpy(ua.src, ub.src, ub.totals[0] * sizeof(uint64_t));
    CHECK(same(ua, ub) && ua.totals[1] + NW + 1 <= u_words);
    CHECK(pg_kindex_trim(one, u, u_words - 1, nullptr, nullptr, m, L, u_kmers, min_cov, min_len, ua.span, ua.packed, ua.word_off, ua.kmer_base, ua.src,
                         ua.totals, nullptr) == PG_EINVAL);
    delete[] u;
    pg_kindex_destroy(cutix);
    pg_kindex_destroy(one);
}

int main() {
    flavour<2>(31);
    flavour<4>(65);
    printf("ktrim host twin: ok\n");
    return 0;
}
