// p2_walk_asan.cpp -- parse1read as pass 2 runs it (csrc/p2_walk.hpp: p2_walk_step / p2_walk_end, shared by the device kernels and the host
// twin), in a program of its own so that it can be built with -fsanitize=address,undefined (tests/test_pass2.py builds and runs it; nothing
// loaded into Python is sanitised).  The step is driven with a sink that records pairs, items and the end decision, and compared with a model
// in the reference's own two-phase shape (prlRead2path.c): parse1read fills a mixBuffer / flagArray with `pos` and `retain` (:598-745), then
// the (K+1)-mers are resolved (:155-212, search1kmerPlus :558-596), then the pre-arcs are taken pairwise up to the first zero (:218-257), then
// recordPathBin's rule (:478-543).  The model works on strings of bases, the step on packed words: the two share no k-mer arithmetic.
// Inputs: node-word sequences over six kinds of node, designed cases first, then random ones from a fixed seed at NW = 2 and NW = 4.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <utility>
#include <vector>

#include "p2_walk.hpp"

using namespace pg;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (case %s)\n", __FILE__, __LINE__, #c, g_case.c_str()); exit(1); } \
    } while (0)
static std::string g_case;
static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

// ---- nodes and the patch map --------------------------------------------------------------------------------------------------------
enum Kind { DELETED, FLOATING, EDGE, BRANCH };       // FLOATING: linear outside any edge; EDGE: linear in edge `edge` with `twin` 1 or 2
struct Node {
    Kind kind;
    uint32_t edge;
    int twin;
    bool smaller;                                    // the read spells the canonical k-mer
    std::string canon;                               // the canonical k-mer, bases as codes 0..3 (A C T G: complement = code ^ 2)
};
static std::string revcomp(const std::string& s) { std::string r(s.rbegin(), s.rend()); for (char& c : r) c ^= 2; return r; }
static std::string random_canon(int K) {
    std::string s((size_t)K, 0);
    for (char& c : s) c = (char)(rnd() & 3);
    const std::string r = revcomp(s);
    return s < r ? s : r;                            // (right-aligned words of equal length compare as their base strings do)
}
static Node deleted(int K) { return Node{DELETED, 0, 0, (rnd() & 1) != 0, random_canon(K)}; }
static Node floating(int K) { return Node{FLOATING, 0, 0, (rnd() & 1) != 0, random_canon(K)}; }
static Node edge(int K, uint32_t e, int twin, bool smaller) { return Node{EDGE, e, twin, smaller, random_canon(K)}; }
static Node branch(int K) { return Node{BRANCH, 0, 0, (rnd() & 1) != 0, random_canon(K)}; }
static uint64_t node_word(const Node& n) {
    uint32_t A = (uint32_t)(rnd() & 0xFFFFFF), B = (uint32_t)(rnd() & 0xFFFFFF);       // arc counters: whatever
    if (n.kind == DELETED) B |= B_DELETED | ((rnd() & 1) ? B_LINEAR : 0);
    if (n.kind == FLOATING) B |= B_LINEAR;
    if (n.kind == EDGE) { A = n.edge; B |= B_LINEAR | (uint32_t)n.twin << B_TWIN_SHIFT | 1u << B_INEDGE_SHIFT; }
    return (uint64_t)A | (uint64_t)B << 32;
}
// the patch map: holds every (K+1)-mer, none, or those a hash of the key picks; an entry's id and twin are functions of the key
enum PatchMode { NONE, ALL, SOME };
struct PatchEntry { uint32_t id; int twin; };
static bool patch_find(PatchMode mode, const std::string& key, PatchEntry& e) {
    uint64_t h = 1469598103934665603ull;
    for (char c : key) h = (h ^ (uint64_t)(c + 1)) * 1099511628211ull;
    e.id = 1000 + (uint32_t)(h >> 20) % 500;
    e.twin = 1 + (int)((h >> 40) & 1);
    return mode == ALL || (mode == SOME && (h >> 50) % 3 != 0);
}

// ---- what a read comes to ---------------------------------------------------------------------------------------------------------------
struct Outcome {
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    std::vector<uint32_t> walk;                      // the -R walk, empty when the read has none
    bool deleted = false;
    bool operator==(const Outcome& o) const { return pairs == o.pairs && walk == o.walk && deleted == o.deleted; }
};

// the model: prlRead2path.c's buffers and phases, on base strings
static Outcome model(const std::vector<Node>& nodes, PatchMode mode) {
    struct Slot { uint32_t low; bool flag; bool smaller; std::string plus; };
    const size_t start = 0, finish = nodes.size();
    std::vector<Slot> mix(finish);
    for (size_t j = 0; j < finish; j++) mix[j] = Slot{0xDEAD0000u + (uint32_t)j, false, false, ""};      // what chopKmer4read left: k-mers, not zero
    Outcome out;
    // parse1read
    unsigned retain = 0;
    uint32_t edge_index = 0;
    size_t pos = start;
    bool is_prev = false;
    std::string prev_kmer, current;
    for (size_t j = start; j < finish; j++) {
        const Node& node = nodes[j];
        if (node.kind == DELETED || node.kind == FLOATING) {
            if (retain < 2) { retain = 0; pos = start; }
            else break;
            continue;
        }
        if (node.kind == EDGE) {
            edge_index = node.smaller ? node.edge : node.edge + (uint32_t)node.twin - 1;
            if (retain == 0 || is_prev) {
                retain++;
                mix[pos].low = edge_index;
                mix[pos++].flag = false;
                is_prev = false;
            } else if (edge_index != mix[pos - 1].low) {
                retain++;
                mix[pos].low = edge_index;
                mix[pos++].flag = false;
            }
        } else {
            current = node.smaller ? node.canon : revcomp(node.canon);
            if (is_prev) {
                retain++;
                const std::string wordplus = prev_kmer + current.back(), bal = revcomp(wordplus);
                mix[pos].smaller = wordplus < bal;
                mix[pos].plus = mix[pos].smaller ? wordplus : bal;
                mix[pos].low = 0xBEEF0000u + (uint32_t)pos;                               // the low word of a (K+1)-mer: not an id yet
                mix[pos++].flag = true;
            }
            is_prev = true;
            prev_kmer = current;
        }
    }
    if (retain < 1) out.deleted = true;
    if (retain < 2) { mix[start].flag = false; mix[start].low = 0; }
    else if (pos < finish) { mix[pos].flag = false; mix[pos].low = 0; }
    // search1kmerPlus
    for (size_t j = start; j < finish; j++) {
        if (!mix[j].flag) { if (mix[j].low == 0) break; continue; }
        PatchEntry e;
        mix[j].low = patch_find(mode, mix[j].plus, e) ? (mix[j].smaller ? e.id : e.id + (uint32_t)e.twin - 1) : 0;
    }
    // thread_add1preArc
    for (size_t j = start; j + 1 < finish; j++) {
        if (mix[j].low == 0 || mix[j + 1].low == 0) break;
        out.pairs.emplace_back(mix[j].low, mix[j + 1].low);
    }
    // recordPathBin
    if (finish - start >= 3 && mix[start].low && mix[start + 1].low && mix[start + 2].low)
        for (size_t j = start; j < finish && mix[j].low; j++) out.walk.push_back(mix[j].low);
    return out;
}

// the step under test: packed words, a sink that records
template <int NW>
static Kmer<NW> pack(const std::string& s) {
    Kmer<NW> k;
    for (int i = 0; i < NW; i++) k.w[i] = 0;
    for (char c : s) {
        for (int i = 0; i < NW - 1; i++) k.w[i] = (k.w[i] << 2) | (k.w[i + 1] >> 62);
        k.w[NW - 1] = (k.w[NW - 1] << 2) | (uint64_t)c;
    }
    return k;
}
template <int NW>
static std::string unpack(const Kmer<NW>& k, int len) {
    std::string s((size_t)len, 0);
    for (int i = 0; i < len; i++) { const int bit = 2 * (len - 1 - i); s[i] = (char)((k.w[NW - 1 - bit / 64] >> (bit % 64)) & 3); }
    return s;
}
template <int NW>
struct Recorder {
    PatchMode mode;
    int K;
    Outcome& out;
    std::vector<uint32_t> ids;
    uint32_t kplus(const Kmer<NW>& key, bool smaller) {
        const std::string s = unpack<NW>(key, K + 1);
        for (int i = 0; i < NW; i++) CHECK(pack<NW>(s).w[i] == key.w[i]);                 // nothing above the K + 1 bases
        CHECK(!(revcomp(s) < s));                                                         // the canonical one of the two
        PatchEntry e;
        return patch_find(mode, s, e) ? (smaller ? e.id : e.id + (uint32_t)e.twin - 1) : 0;
    }
    void pair(uint32_t from, uint32_t to, int i) {
        CHECK(i == (int)out.pairs.size());                                                // pairs come in order, each once, none behind a gap
        CHECK(i + 1 == (int)ids.size() && ids[i] == from);                                // from = item i; `to` is the item that comes next
        out.pairs.emplace_back(from, to);
    }
    void item(int i, uint32_t id) {
        if (i == 0) { CHECK(out.pairs.empty()); ids.clear(); }                            // a restart: only while nothing has gone out
        CHECK(i == (int)ids.size());
        CHECK(out.pairs.size() <= (size_t)i && (out.pairs.size() < (size_t)i || i == 0 || out.pairs.back().second == id));
        ids.push_back(id);
    }
};
template <int NW>
static Outcome stepped(const std::vector<Node>& nodes, int K, PatchMode mode) {
    Outcome out;
    Recorder<NW> sink{mode, K, out, {}};
    P2Walk<NW> w;
    for (size_t j = 0; j < nodes.size() && !w.stop; j++)
        p2_walk_step<NW>(w, pack<NW>(nodes[j].canon), nodes[j].smaller, node_word(nodes[j]), K, sink);
    const P2WalkEnd end = p2_walk_end<NW>(w);
    out.deleted = end.deleted;
    CHECK(end.walk == 0 || (end.walk >= 3 && end.walk <= (int)sink.ids.size()));
    out.walk.assign(sink.ids.begin(), sink.ids.begin() + end.walk);
    return out;
}

template <int NW>
static Outcome both(const char* name, const std::vector<Node>& nodes, int K, PatchMode mode) {
    g_case = name;
    const Outcome want = model(nodes, mode), got = stepped<NW>(nodes, K, mode);
    CHECK(got.pairs == want.pairs);
    CHECK(got.walk == want.walk);
    CHECK(got.deleted == want.deleted);
    return got;
}

typedef std::vector<std::pair<uint32_t, uint32_t>> Pairs;
template <int NW>
static void designed(int K) {
    Outcome o;
    o = both<NW>("same edge id twice, then another", {edge(K, 7, 1, true), edge(K, 7, 1, true), edge(K, 9, 1, true)}, K, ALL);
    CHECK(o.pairs == Pairs({{7, 9}}) && o.walk.empty() && !o.deleted);
    o = both<NW>("branch, branch only", {branch(K), branch(K)}, K, ALL);
    CHECK(o.pairs.empty() && o.walk.empty() && !o.deleted);                               // one item: no pair, not counted deleted
    o = both<NW>("edge, branch, branch, edge", {edge(K, 3, 1, true), branch(K), branch(K), edge(K, 4, 1, true)}, K, ALL);
    CHECK(o.pairs.size() == 2 && o.pairs[0].first == 3 && o.pairs[1].second == 4 && o.pairs[0].second == o.pairs[1].first && o.pairs[0].second >= 1000);
    CHECK(o.walk.size() == 3 && !o.deleted);
    o = both<NW>("a restart with one item retained", {edge(K, 1, 1, true), deleted(K), edge(K, 2, 1, true), edge(K, 3, 1, true)}, K, ALL);
    CHECK(o.pairs == Pairs({{2, 3}}) && o.walk.empty() && !o.deleted);
    o = both<NW>("a stop with two retained", {edge(K, 1, 1, true), edge(K, 2, 1, true), floating(K), edge(K, 3, 1, true), edge(K, 4, 1, true)}, K, ALL);
    CHECK(o.pairs == Pairs({{1, 2}}) && o.walk.empty() && !o.deleted);
    // the restart keeps is_prev and prev_k: the second branch node makes an item of a (K+1)-mer that spans the deleted node -- no edge has it
    o = both<NW>("branch, deleted, branch, edge", {branch(K), deleted(K), branch(K), edge(K, 5, 1, true)}, K, NONE);
    CHECK(o.pairs.empty() && o.walk.empty() && !o.deleted);
    o = both<NW>("branch, deleted, branch, edge (were the map to hold it)", {branch(K), deleted(K), branch(K), edge(K, 5, 1, true)}, K, ALL);
    CHECK(o.pairs.size() == 1 && o.pairs[0].second == 5 && !o.deleted);
    o = both<NW>("edge, branch, same edge again", {edge(K, 6, 1, true), branch(K), edge(K, 6, 1, true)}, K, ALL);
    CHECK(o.pairs == Pairs({{6, 6}}) && o.walk.empty());
    o = both<NW>("a patch miss as second item", {edge(K, 1, 1, true), branch(K), branch(K), edge(K, 2, 1, true), edge(K, 3, 1, true)}, K, NONE);
    CHECK(o.pairs.empty() && o.walk.empty() && !o.deleted);
    o = both<NW>("three resolved items, then a miss, then more",
                 {edge(K, 1, 1, true), edge(K, 2, 1, true), edge(K, 3, 1, true), branch(K), branch(K), edge(K, 4, 1, true), edge(K, 5, 1, true)}, K, NONE);
    CHECK(o.pairs == Pairs({{1, 2}, {2, 3}}) && o.walk == std::vector<uint32_t>({1, 2, 3}));
    o = both<NW>("twin 2 on the larger strand", {edge(K, 10, 2, false), edge(K, 20, 2, true), edge(K, 30, 1, false)}, K, ALL);
    CHECK(o.pairs == Pairs({{11, 20}, {20, 30}}) && o.walk == std::vector<uint32_t>({11, 20, 30}));
    o = both<NW>("all deleted", {deleted(K), floating(K), deleted(K)}, K, ALL);
    CHECK(o.pairs.empty() && o.walk.empty() && o.deleted);
    o = both<NW>("a single k-mer", {edge(K, 8, 1, true)}, K, ALL);
    CHECK(o.pairs.empty() && o.walk.empty() && !o.deleted);
}

template <int NW>
static void random_cases(int K, int n_cases) {
    unsigned long long pairs = 0, walks = 0, del = 0;
    for (int c = 0; c < n_cases; c++) {
        const int n = 1 + (int)(rnd() % 40);
        const int w_del = (int)(rnd() % 3), w_branch = 1 + (int)(rnd() % 4);               // how often a node is deleted / floating, or a branch node
        std::vector<Node> nodes;
        uint32_t e = 1 + (uint32_t)(rnd() % 50);
        for (int j = 0; j < n; j++) {
            const int x = (int)(rnd() % 12);
            if (x < w_del) nodes.push_back((rnd() & 1) ? deleted(K) : floating(K));
            else if (x < w_del + w_branch) nodes.push_back(branch(K));
            else {
                if (rnd() % 3 == 0) e = 1 + (uint32_t)(rnd() % 50);                       // (else: the edge of the k-mer before, as along a real read)
                nodes.push_back(edge(K, e, 1 + (int)(rnd() & 1), (rnd() & 1) != 0));
            }
        }
        char name[64];
        snprintf(name, sizeof name, "random %d (NW %d, K %d)", c, NW, K);
        const Outcome o = both<NW>(name, nodes, K, (PatchMode)(rnd() % 3));
        pairs += o.pairs.size(); walks += !o.walk.empty(); del += o.deleted;
    }
    CHECK(pairs > (unsigned long long)n_cases && walks > (unsigned long long)n_cases / 20 && del > 0);      // the cases reach every outcome
    printf("NW %d K %d: %d random reads, %llu pairs, %llu walks, %llu deleted\n", NW, K, n_cases, pairs, walks, del);
}

int main() {
    // (K = 127 is left out: there the reference reverses a 128-base (K+1)-mer through a `char` length and gets it wrong, and rc_plus follows it --
    //  kmer.hpp; that rule is the golden cases' to check, test_pass2.py / test_gpu_pregraph.py at K = 127, not this model's)
    designed<2>(31); designed<2>(63); designed<4>(64); designed<4>(125);
    printf("designed cases ok\n");
    random_cases<2>(24, 1000); random_cases<2>(63, 1000); random_cases<4>(71, 1000); random_cases<4>(125, 1000);
    printf("p2_walk ok\n");
    return 0;
}
