"""The unitigs' cases, shared by tests/test_kunitig_host.py (the host twin) and tests/test_gpu_kunitig.py (the kernels): designed read sets
turned into records with the builders of tests/kwalk_cases.py, compacted through pg_kindex_unitigs with output buffers of exactly the
stated sizes, and compared -- as sorted lists, the order of the unitigs being unspecified -- with the model (tests/kunitig_model.py) and
with the texts and reasons the construction dictates.  Every run also checks the layout word for word (rows word-aligned, pad bits and
tail words zero, the offsets), count mode against full mode, and, when nothing was cut, that every solid k-mer of the model lies in
exactly one unitig.  All comparisons are of integers and exact."""
import functools
from collections import Counter, namedtuple

import numpy as np
import pytest

import kindex_cases as KC
import kindex_model as M
import kunitig_model as U
import kwalk_cases as E
import kwalk_model as W
from kwalk_cases import codes, count, forked, linear, linear_counts, random_genome, rc, records_of, tile
from soapdenovo2_amd import api

FLAVOURS = KC.FLAVOURS
flavour_id = KC.flavour_id
FILL = E.FILL
EINVAL, ESTATE = E.EINVAL, E.ESTATE
MAXK = api.UNITIG_MAX_KMERS

# A design: records, the thresholds, and the unitigs the construction dictates as (text, left reason, right reason) in the orientation the
# rule emits (None: the model alone is the yardstick); cut = the cut unitigs expected
Case = namedtuple("Case", "name records min_cov min_arc max_kmers expect cut")


def emitted(text, left, right, K):
    """A linear unitig as the rule emits it: from the end whose first k-mer is not greater."""
    text = [int(c) for c in text]
    back = W.revcomp(text)
    return (tuple(back), right, left) if W.value(back[:K]) < W.value(text[:K]) else (tuple(text), left, right)


def ring(c, K):
    """The cyclic unitig of the circular genome c: from its least canonical k-mer, as that k-mer reads, once round."""
    C = len(c)
    best = None
    for strand in (list(c), W.revcomp(list(c))):
        twice = [int(x) for x in strand] * 3                                  # (room for once round from any start, K - 1 < C)
        assert C >= K
        for j in range(C):
            v = W.value(twice[j:j + K])
            if W.value(W.revcomp(twice[j:j + K])) > v and (best is None or v < best[0]):
                best = (v, tuple(twice[j:j + C + K - 1]))
    return (best[1], U.CYCLE, U.CYCLE)


@functools.lru_cache(maxsize=None)
def circular(K):
    c = random_genome(4300 + K, K + 150)
    assert E.distinct_kmers([np.concatenate([c, c[:K - 1]])], K) == len(c)
    return c


@functools.lru_cache(maxsize=None)
def hairpin(K):
    """A followed by its own reverse complement: the (K-1)-mer across the junction is its own reverse complement, and the k-mer that
    ends with it is followed by its own reverse complement."""
    A = random_genome(4500 + K, K + 60)
    h = np.concatenate([A, rc(A)])
    m = (K - 1) // 2
    assert E.distinct_kmers([h], K) == len(A) - m
    return A, h


@functools.lru_cache(maxsize=None)
def noisy(K):
    """A genome of 2 000 bases with a repeat of 150, read on both strands with 1 % substitutions: branches, tips, bubbles, weak k-mers."""
    rng = np.random.default_rng(4600 + K)
    g = rng.integers(0, 4, size=2000, dtype=np.uint8)
    g[1200:1350] = g[200:350]
    L, reads = max(100, K + 30), []
    for i in range(240):
        at = int(rng.integers(0, len(g) - L + 1))
        r = g[at:at + L].copy()
        hit = rng.random(L) < 0.01
        r[hit] = (r[hit] + rng.integers(1, 4, size=int(hit.sum()))) & 3
        reads.append(rc(r) if i % 2 else r)
    return reads


@functools.lru_cache(maxsize=None)
def singles(K, n, seed):
    """n k-mers read alone, as reads of K bases: no arcs, n isolated unitigs of one k-mer."""
    rng = np.random.default_rng(seed + K)
    out = [rng.integers(0, 4, size=K, dtype=np.uint8) for _ in range(n)]
    assert E.distinct_kmers(out, K) == n
    return out


@functools.lru_cache(maxsize=None)
def cases(K, mer127):
    nw = 4 if mer127 else 2
    g = linear(K)
    out = []
    D, BO, WN, BI, HP, CUT = U.DEAD_END, U.BRANCH_OUT, U.WEAK_NEXT, U.BRANCH_IN, U.HAIRPIN, U.CUT
    lin3 = records_of(*linear_counts(K, 3), nw)

    # a linear genome: one unitig, the genome or its reverse complement by the orientation rule; the same from the reads reverse complemented
    out.append(Case("linear", lin3, 1, 1, MAXK, [emitted(g, D, D, K)], 0))
    out.append(Case("linear-rc-reads", records_of(*count([(tile(rc(g), K), 3)], K), nw), 1, 1, MAXK, [emitted(g, D, D, K)], 0))

    # two genomes that share a prefix: the prefix ends with BRANCH_OUT, either branch begins with BRANCH_IN one k-mer behind it
    P, SA, SB = forked(K)
    g1, g2, nP = np.concatenate([P, SA]), np.concatenate([P, SB]), len(P)
    fork = records_of(*count([(tile(g1, K), 2), (tile(g2, K), 2)], K), nw)
    out.append(Case("shared-prefix", fork, 1, 1, MAXK,
                    [emitted(P, D, BO, K), emitted(g1[nP - K + 1:], BI, D, K), emitted(g2[nP - K + 1:], BI, D, K)], 0))

    # a branch carried by one read beside one carried by five: three unitigs where it counts, one where neither its arc nor its k-mers do
    minor = g2[nP - K - 3:nP + K + 3]
    skew = records_of(*count([(tile(g1, K), 5), ([minor], 1)], K), nw)
    out.append(Case("minor-branch-arc1", skew, 1, 1, MAXK,
                    [emitted(P, D, BO, K), emitted(g1[nP - K + 1:], BI, D, K), emitted(minor[4:], BI, D, K)], 0))
    out.append(Case("minor-branch-arc2", skew, 2, 2, MAXK, [emitted(g1, D, D, K)], 0))
    out.append(Case("minor-branch-arc2-cov1", skew, 1, 2, MAXK, None, 0))      # (the minor branch's k-mers stay solid: isolated ones)

    # one weak k-mer in the middle, by coverage and by the deleted bit: two unitigs with WEAK_NEXT, the weak k-mer in none
    t = 100
    at = lambda j: E.canon(g[j:j + K], K)
    occ, arcs = count([(tile(g[:t + K - 1], K), 3), (tile(g[t + 1:], K), 3), (tile(g, K), 1)], K)
    weak = occ[at(t)]
    assert all(occ[at(j)] > weak for j in range(len(g) - K + 1) if j != t)
    two = [emitted(g[:t + K - 1], D, WN, K), emitted(g[t + 1:], WN, D, K)]
    out.append(Case("weak-middle-coverage", records_of(occ, arcs, nw), weak + 1, 1, MAXK, two, 0))
    out.append(Case("weak-middle-deleted", records_of(*linear_counts(K, 3), nw, deleted={at(t)}), 1, 1, MAXK, two, 0))

    # a circular genome: one cyclic unitig of C k-mers from its least canonical k-mer; and with a separate linear genome in the same index
    c = circular(K)
    out.append(Case("circular", records_of(*count([(tile(c, K, circular=True), 2)], K), nw), 1, 1, MAXK, [ring(c, K)], 0))
    assert E.distinct_kmers([np.concatenate([c, c[:K - 1]]), g], K) == len(c) + len(g) - K + 1
    both = records_of(*count([(tile(c, K, circular=True), 2), (tile(g, K), 3)], K), nw)
    out.append(Case("circular-and-linear", both, 1, 1, MAXK, [ring(c, K), emitted(g, D, D, K)], 0))
    # a ring of more k-mers than max_kmers is not emitted: nothing comes out, and covered < solid says so
    out.append(Case("circular-too-long", records_of(*count([(tile(c, K, circular=True), 2)], K), nw), 1, 1, len(c) - 1, [], 0))
    out.append(Case("circular-exact", records_of(*count([(tile(c, K, circular=True), 2)], K), nw), 1, 1, len(c), [ring(c, K)], 0))

    # a hairpin: the chain ends where its next k-mer would be the reverse complement of its last
    A, h = hairpin(K)
    out.append(Case("hairpin", records_of(*count([(tile(h, K), 2)], K), nw), 1, 1, MAXK, [emitted(h[:len(A) + (K - 1) // 2], D, HP, K)], 0))

    # a homopolymer: one k-mer whose successor is itself
    poly = codes([0] * (K + 20))
    out.append(Case("homopolymer", records_of(*count([(tile(poly, K), 2)], K), nw), 1, 1, MAXK, [(tuple([0] * K), HP, HP)], 0))

    # an isolated k-mer, read alone: n = 1, in its canonical orientation
    one = singles(K, 1, 4700)[0]
    out.append(Case("single", records_of(*count([([one], 3)], K), nw), 1, 1, MAXK, [emitted(one, D, D, K)], 0))

    # texts of 31, 32, 33, 64 and 65 bases beyond a word edge
    for T in (31, 32, 33, 64, 65):
        L = T
        while L < K + 12:
            L += 32
        out.append(Case("text-%d" % L, records_of(*count([(tile(g[:L], K), 2)], K), nw), 1, 1, MAXK, [emitted(g[:L], D, D, K)], 0))

    # max_kmers below the chain's length: a cut unitig from either end, the k-mers between them in none
    m = 50
    out.append(Case("cut", lin3, 1, 1, m, [(tuple(int(x) for x in g[:m + K - 1]), D, CUT), (tuple(int(x) for x in rc(g)[:m + K - 1]), D, CUT)], 2))
    out.append(Case("cut-exact", lin3, 1, 1, len(g) - K + 1, [emitted(g, D, D, K)], 0))           # (the guard at the chain's own length cuts nothing)

    # arc counters at 63
    occ, arcs = linear_counts(K, 100)
    out.append(Case("arc-63", records_of(occ, arcs, nw), 1, 63, MAXK, [emitted(g, D, D, K)], 0))
    out.append(Case("arc-63-absent", lin3, 1, 63, MAXK, None, 0))

    # an empty index
    out.append(Case("empty", np.zeros((0, nw + 2), dtype=np.uint64), 1, 1, MAXK, [], 0))

    # 129 and 513 entries of the start list -- 64 and 256 isolated k-mers, two starts each, and a ring's one behind them -- in a table of
    # more slots than a workgroup has lanes: the scan's block edges
    for n in (64, 256):
        lone = singles(K, n, 4800)
        assert E.distinct_kmers([np.concatenate([c, c[:K - 1]])] + lone, K) == len(c) + n
        recs = records_of(*count([(tile(c, K, circular=True), 2), (lone, 2)], K), nw)
        out.append(Case("starts-%d" % (2 * n + 1), recs, 1, 1, MAXK, [ring(c, K)] + [emitted(s, D, D, K) for s in lone], 0))
    return out


class Compactor:
    """An index under test with its model: device = -1 the host twin over numpy, else the device build over torch tensors.  A call goes
    straight to pg_kindex_unitigs with output buffers of exactly the stated sizes, pre-filled with FILL."""

    def __init__(self, records, K, mer127, device, model=None):
        self.K, self.mer127, self.device = K, mer127, device
        self.nw = 4 if mer127 else 2
        self.model = model if model is not None else M.Model.from_records(records, K, self.nw)
        self.ix = api.KmerIndex.from_records(records, K, mer127, device)

    def close(self):
        self.ix.close()

    def filled(self, n):
        a = np.full(max(n, 1), FILL, dtype=np.uint64)
        if self.device < 0:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64)).to("cuda:%d" % self.device)

    def down(self, a):
        return a if self.device < 0 else a.cpu().numpy().view(np.uint64)

    def call(self, min_cov, min_arc, max_kmers, cap_unitigs, cap_words, packed, word_off, kmer_base, report, totals, ix=None):
        p = self.ix._ptr
        return api.lib().pg_kindex_unitigs((ix or self.ix).h, min_cov, min_arc, max_kmers, cap_unitigs, cap_words, p(packed), p(word_off), p(kmer_base),
                                           p(report), p(totals), self.ix._stream())

    def count(self, min_cov, min_arc, max_kmers):
        totals = self.filled(8)
        assert self.call(min_cov, min_arc, max_kmers, 0, 0, None, None, None, None, totals) == 0, api.lib().pg_last_error()
        return [int(v) for v in self.down(totals)]

    def outputs(self, n, words):
        return self.filled(words), self.filled(n + 1), self.filled(n + 1), self.filled(2 * n), self.filled(8)

    def run(self, min_cov, min_arc, max_kmers=MAXK, what=""):
        """The list of (text, left, right, coverage sum) and the totals, after every check of the layout."""
        K, tail = self.K, self.nw + 1
        counted = self.count(min_cov, min_arc, max_kmers)
        n, words = counted[0], counted[1]
        assert counted[7] == 0 and words >= tail
        packed, word_off, kmer_base, report, totals = self.outputs(n, words)
        assert self.call(min_cov, min_arc, max_kmers, n, words, packed, word_off, kmer_base, report, totals) == 0, api.lib().pg_last_error()
        packed, word_off, kmer_base, report, totals = (self.down(a) for a in (packed, word_off, kmer_base, report, totals))
        assert [int(v) for v in totals] == counted, what + ": the full call's totals differ from the count call's"
        f = api.unitig_fields(report[:2 * n])
        got, at, base, want_words = [], 0, 0, []
        for u in range(n):
            L = int(f["len"][u])
            assert L >= K and int(word_off[u]) == at and int(kmer_base[u]) == base, what
            text = [int(x) for x in api.unpack_seq(packed[at:], L)]
            want_words += W.row_of(text, (L + 31) // 32)
            got.append((tuple(text), int(f["left_code"][u]), int(f["right_code"][u]), int(f["coverage_sum"][u])))
            at += (L + 31) // 32
            base += L - K + 1
        assert int(word_off[n]) == at and int(kmer_base[n]) == base and at + tail == words, what
        assert packed.size == max(words, 1) and [int(v) for v in packed[:words]] == want_words + [0] * tail, what + ": pad bits or tail words"
        assert counted[2] == sum(len(t) for t, _, _, _ in got) and counted[3] == base, what
        return got, counted

    def check(self, min_cov, min_arc, max_kmers=MAXK, what=""):
        """A run against the model, as sorted lists, with the invariant; returns the run."""
        K = self.K
        got, totals = self.run(min_cov, min_arc, max_kmers, what)
        want, n_cut = U.unitigs(self.model, min_cov, min_arc, max_kmers)
        assert sorted(got) == sorted(want), "%s: the unitigs differ from the model's" % what
        assert len(set(t for t, _, _, _ in got)) == len(got), what + ": a unitig came out twice"
        solid = U.solid_keys(self.model, min_cov)
        assert totals[4] == len(solid) and totals[6] == n_cut and totals[5] == sum(1 for _, l, _, _ in got if l == U.CYCLE), what
        if not n_cut and totals[3] == totals[4]:
            met = Counter(k for t, _, _, _ in got for k in U.kmers_of(t, K))
            assert sorted(met) == solid and set(met.values()) <= {1}, what + ": not every solid k-mer in exactly one unitig"
        else:
            assert totals[3] != totals[4] or n_cut, what
        for t, _, _, cov in got:
            assert cov == sum(M.coverage(self.model.cnt[k]) for k in U.kmers_of(t, K)), what
        return got, totals


def check_case(c, K, mer127, device, twin=None):
    what = "%s %s" % (c.name, flavour_id((K, mer127)))
    w = Compactor(c.records, K, mer127, device)
    try:
        got, totals = w.check(c.min_cov, c.min_arc, c.max_kmers, what)
        if c.expect is not None:
            assert sorted((t, l, r) for t, l, r, _ in got) == sorted(c.expect), "%s: not the unitigs the design dictates" % what
        assert totals[6] == c.cut, what
        if c.cut:
            assert totals[3] < totals[4], what + ": a cut run covers fewer k-mers than are solid"
        else:
            assert totals[3] <= totals[4], what
        if twin is not None:
            h = Compactor(c.records, K, mer127, twin, model=w.model)
            try:
                h_got, h_totals = h.run(c.min_cov, c.min_arc, c.max_kmers, what + " (host twin)")
            finally:
                h.close()
            assert sorted(h_got) == sorted(got) and h_totals == totals, what + ": the device differs from the host twin"
    finally:
        w.close()


def check_flavour(K, mer127, device, twin=None):
    for c in cases(K, mer127):
        check_case(c, K, mer127, device, twin)


def check_fuzz(name, K, mer127, device, params):
    """A table of kindex_cases with random counter words (about half of them deleted): a fuzz of the arc decoding, of the symmetry of
    the side test under counters no read set would give and, for "colliding", of long probe runs."""
    records, _ = KC.table(name, K, mer127)
    w = Compactor(records, K, mer127, device)
    try:
        met = set()
        for min_cov, min_arc in params:
            got, _ = w.check(min_cov, min_arc, MAXK, "%s %s min_cov %d min_arc %d" % (name, flavour_id((K, mer127)), min_cov, min_arc))
            met |= {x for _, l, r, _ in got for x in (l, r)}
        assert met >= {U.DEAD_END, U.BRANCH_OUT, U.WEAK_NEXT}, met
    finally:
        w.close()


def check_noisy(K, mer127, device, twin=None):
    """The 2 kb genome with a repeat, read with 1 % substitutions, at min_cov 1 and 3."""
    nw = 4 if mer127 else 2
    records = records_of(*count([(noisy(K), 1)], K), nw)
    w = Compactor(records, K, mer127, device)
    h = Compactor(records, K, mer127, twin, model=w.model) if twin is not None else None
    try:
        for min_cov, min_arc in ((1, 1), (3, 2)):
            what = "noisy %s min_cov %d" % (flavour_id((K, mer127)), min_cov)
            got, totals = w.check(min_cov, min_arc, MAXK, what)
            assert totals[0] > 3 and totals[6] == 0 and totals[3] == totals[4], what
            if h is not None:
                h_got, h_totals = h.run(min_cov, min_arc, MAXK, what)
                assert sorted(h_got) == sorted(got) and h_totals == totals, what + ": the device differs from the host twin"
    finally:
        w.close()
        if h is not None:
            h.close()


# ---- 32 769 isolated k-mers: 65 538 starts, the start list's capacity 2 * keys exactly, in 257 blocks of 256 -- the 257th is the first
# block of the second round of the scan over the blocks' sums ----
ISOLATED, ISOLATED_K, ISOLATED_MIN_COV = 128 * 256 + 1, 31, 2


@functools.lru_cache(maxsize=None)
def isolated():
    """(records, the model, the model's unitigs as a sorted list of (key, left, right, coverage sum)): distinct random canonical 31-mers
    with a coverage of ISOLATED_MIN_COV .. 255 and every arc counter zero.  Built once and shared, and never written to."""
    K, n = ISOLATED_K, ISOLATED
    rng = np.random.default_rng(4900)
    two, three = np.uint64(2), np.uint64(3)
    x = rng.integers(0, 1 << 62, size=n + 64, dtype=np.uint64)
    back = np.zeros_like(x)
    for i in range(K):                                                         # (a step a base, over all keys at once)
        back = (back << two) | (((x >> np.uint64(2 * i)) & three) ^ two)
    keys = np.unique(np.minimum(x, back))
    assert keys.size >= n
    keys = rng.permutation(keys)[:n]
    records = np.zeros((n, 4), dtype=np.uint64)
    records[:, 1] = keys
    records[:, 2] = rng.integers(ISOLATED_MIN_COV, 256, size=n).astype(np.uint64) << np.uint64(24)
    records[:, 3] = np.arange(n, dtype=np.uint64)
    model = M.Model.from_records(records, K, 2)
    want, n_cut = U.unitigs(model, ISOLATED_MIN_COV, 1)
    assert n_cut == 0 and all(len(t) == K for t, _, _, _ in want)
    return records, model, sorted((W.value(t), l, r, c) for t, l, r, c in want)


def check_isolated(device, twin=None):
    """The count call and the full call over the isolated k-mers: the totals, the layout, and -- as sorted lists -- the unitigs the
    construction dictates (every key as it is, K bases, both reasons DEAD_END, its own coverage), the model's and the host twin's."""
    K, n, tail = ISOLATED_K, ISOLATED, 3
    records, model, want = isolated()
    D = U.DEAD_END
    assert want == sorted((int(k), D, D, int(c) >> 24) for k, c in zip(records[:, 1], records[:, 2]))
    totals = [n, n + tail, n * K, n, n, 0, 0, 0]

    def run(dev):
        w = Compactor(records, K, False, dev, model=model)
        try:
            assert w.count(ISOLATED_MIN_COV, 1, MAXK) == totals
            outs = w.outputs(n, n + tail)
            assert w.call(ISOLATED_MIN_COV, 1, MAXK, n, n + tail, *outs) == 0, api.lib().pg_last_error()
            packed, word_off, kmer_base, report, tot = (w.down(a) for a in outs)
        finally:
            w.close()
        assert [int(v) for v in tot] == totals
        assert (word_off == np.arange(n + 1, dtype=np.uint64)).all() and (kmer_base == np.arange(n + 1, dtype=np.uint64)).all()
        assert packed.size == n + tail and not packed[n:].any() and not (packed[:n] & np.uint64(3)).any()
        f = api.unitig_fields(report)
        assert (f["len"] == K).all()
        return sorted(zip((packed[:n] >> np.uint64(2)).tolist(), f["left_code"].tolist(), f["right_code"].tolist(), f["coverage_sum"].tolist()))

    got = run(device)
    assert got == want, "the unitigs differ from the model's"
    if twin is not None:
        assert run(twin) == got, "the device differs from the host twin"


def check_capacities(K, mer127, device):
    """Capacities one short in unitigs and one short in words: the overflow flag, and nothing but the totals written; exact ones: the
    result; each nullable output null in turn: the others as before."""
    nw = 4 if mer127 else 2
    P, SA, SB = forked(K)
    records = records_of(*count([(tile(np.concatenate([P, SA]), K), 2), (tile(np.concatenate([P, SB]), K), 2)], K), nw)
    w = Compactor(records, K, mer127, device)
    try:
        counted = w.count(1, 1, MAXK)
        n, words = counted[0], counted[1]
        assert n == 3
        for cap_n, cap_w in ((n - 1, words), (n, words - 1), (0, 0)):
            packed, word_off, kmer_base, report, totals = w.outputs(n, words)
            assert w.call(1, 1, MAXK, cap_n, cap_w, packed, word_off, kmer_base, report, totals) == 0
            assert [int(v) for v in w.down(totals)] == counted[:7] + [1]
            assert all((w.down(a) == FILL).all() for a in (packed, word_off, kmer_base, report))
        ref = None
        for null in (None, 1, 2, 3):
            outs = list(w.outputs(n, words))
            if null is not None:
                outs[null] = None
            assert w.call(1, 1, MAXK, n, words, *outs) == 0
            assert [int(v) for v in w.down(outs[4])] == counted
            # (the order of the unitigs may differ from call to call: the rows' words are compared as a sorted list)
            rows = sorted(int(v) for v in w.down(outs[0])[:words])
            ref = rows if ref is None else ref
            assert rows == ref and FILL not in rows
            for a in outs[1:3]:
                if a is not None:
                    a = w.down(a).astype(np.int64)
                    assert a.size == n + 1 and a[0] == 0 and (np.diff(a) > 0).all()
            if outs[1] is not None:
                assert int(w.down(outs[1])[n]) + nw + 1 == words
            if outs[2] is not None:
                assert int(w.down(outs[2])[n]) == counted[3]
            if outs[3] is not None:
                f = api.unitig_fields(w.down(outs[3]))
                assert sorted(f["len"]) == sorted([len(P), len(SA) + K - 1, len(SB) + K - 1])
    finally:
        w.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with nothing written: the thresholds' and max_kmers' ranges, null totals, a null index, an index cut over ranks."""
    nw = 4 if mer127 else 2
    records = records_of(*linear_counts(K, 3), nw)
    w = Compactor(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    try:
        outs = w.outputs(4, 64)
        call = lambda min_cov=1, min_arc=1, max_kmers=MAXK, o=outs, ix=None: w.call(min_cov, min_arc, max_kmers, 4, 64, *o, ix=ix)
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64), dict(max_kmers=0), dict(max_kmers=api.UNITIG_KMERS_BOUND + 1)):
            assert call(**bad) == EINVAL and b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert call(o=outs[:4] + (None,)) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_unitigs(None, 1, 1, 1, 0, 0, None, None, None, None, None, None) == EINVAL
        assert call(ix=cut) == ESTATE and b"one lookup after the other in one table" in L.pg_last_error()
        with pytest.raises(api.PgError):
            cut.unitigs(1)
        with pytest.raises(api.PgError):
            w.ix.unitigs(0)
        assert all((w.down(a) == FILL).all() for a in outs)
        assert call(max_kmers=api.UNITIG_KMERS_BOUND) == 0 and int(w.down(outs[4])[0]) == 1     # (the bound itself is taken)
    finally:
        cut.close()
        w.close()


def check_api(K, mer127, device):
    """KmerIndex.unitigs, api.unitig_seqs and the round trip: the returned batch goes into query_ragged as it lies, and every k-mer of it
    is present and solid; into walk_ragged, and no unitig of an uncut run can be extended."""
    nw = 4 if mer127 else 2
    P, SA, SB = forked(K)
    c = circular(K)
    records = records_of(*count([(tile(np.concatenate([P, SA]), K), 3), (tile(np.concatenate([P, SB]), K), 3), (tile(c, K, circular=True), 3)], K), nw)
    w = Compactor(records, K, mer127, device)
    try:
        min_cov = 2
        want, _ = U.unitigs(w.model, min_cov, 1)
        seqs, f, totals = api.unitig_seqs(w.ix, min_cov)
        got = [(tuple(int(x) for x in s), int(l), int(r), int(cv)) for s, l, r, cv in zip(seqs, f["left_code"], f["right_code"], f["coverage_sum"])]
        assert sorted(got) == sorted(want) and totals["unitigs"] == 4 and totals["cyclic"] == 1 and totals["overflow"] == 0
        assert sorted(f["left"] + f["right"]) == sorted(["dead_end"] * 3 + ["branch_out"] + ["branch_in"] * 2 + ["cycle"] * 2)
        u = w.ix.unitigs(min_cov)
        n, n_kmers = int(u.totals[0]), int(u.totals[3])
        assert n_kmers == int(u.totals[4]) == len(U.solid_keys(w.model, min_cov))
        cnt = w.down(w.ix.query_ragged(u.packed, u.word_off, u.kmer_base, n, n_kmers))
        assert cnt.size == n_kmers and (((cnt >> np.uint64(24)) & np.uint64(0xff)) >= min_cov).all()
        assert len(set(int(v) for v in cnt)) > 1
        _, rep = w.ix.walk_ragged(u.packed, u.word_off, u.kmer_base, n, min_cov, 1, 4)
        wf = api.walk_fields(rep)
        uf = api.unitig_fields(u.report)
        for i in range(n):
            if uf["left"][i] != "cycle":
                assert wf["len"][2 * i] == 0 and wf["len"][2 * i + 1] == 0
    finally:
        w.close()
