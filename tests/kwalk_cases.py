"""The walk's cases, shared by tests/test_kwalk_host.py (the host twin) and tests/test_gpu_kwalk.py (kwalk_kernel): designed read sets
turned into records through kindex_model.count_reads (coverage saturating at 255 and arc counters at 63, as node_update does), batches
of sequences, and the comparison of every row and every report word with the model (tests/kwalk_model.py) and with the text and the
stop reason the construction dictates.  Genomes are a few hundred bases of a seeded generator; every builder asserts that the canonical
k-mers of its design are distinct where the design needs that.  All comparisons are of integers and exact."""
import functools
from collections import Counter, namedtuple

import numpy as np
import pytest

import kindex_cases as KC
import kindex_model as M
import kwalk_model as W
from soapdenovo2_amd import api

FLAVOURS = KC.FLAVOURS
flavour_id = KC.flavour_id
FILL = 0x5A5A5A5A5A5A5A5A                  # what the output buffers hold before a call: every word of them must be written
EINVAL, ESTATE = -1, -5                    # PG_EINVAL, PG_ESTATE (include/soapdenovo2_amd.h)

# A design: records, a batch, the parameters, and for some walks (by index: 2r, 2r + 1) the text and the reason the construction dictates
Case = namedtuple("Case", "name records seqs min_cov min_arc max_ext expect")


def codes(a):
    return np.asarray(a, dtype=np.uint8)


def rc(a):
    return codes(W.revcomp(list(a)))


def random_genome(seed, n):
    return np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)


def distinct_kmers(seqs, K):
    return len({k for s in seqs for k in M.canonical_kmers(s, K)})


def tile(g, K, step=4, extra=8, circular=False):
    """Reads of K + extra bases every `step` bases of g (and one that ends with it), alternately as g has them and reverse complemented;
    circular: the reads run on over g's end into its start.  Neighbours overlap by K + extra - step > K bases: every arc is in a read."""
    RL, g = K + extra, list(g)
    if circular:
        src, starts = g + g[:RL], list(range(0, len(g), step))
    else:
        src, starts = g, list(range(0, len(g) - RL + 1, step))
        if starts[-1] != len(g) - RL:
            starts.append(len(g) - RL)
    return [codes(W.revcomp(src[s:s + RL]) if i % 2 else src[s:s + RL]) for i, s in enumerate(starts)]


def count(groups, K):
    """kindex_model.count_reads of the read set that holds every read of groups[i][0] groups[i][1] times."""
    occ, arcs = Counter(), {}
    for reads, copies in groups:
        o, a = M.count_reads(reads, K)
        for k, n in o.items():
            occ[k] += n * copies
        for k, v in a.items():
            t = arcs.setdefault(k, [0] * 8)
            for i in range(8):
                t[i] += v[i] * copies
    return occ, arcs


def records_of(occ, arcs, nw, deleted=()):
    """Export records of counted k-mers: word A = the left counters | coverage << 24, word B = the right counters, `single` (bit 27)
    for a k-mer met once and `deleted` (bit 25) for the keys named; 6-bit counters stop at 63 and the coverage at 255."""
    rec = np.zeros((len(occ), nw + 2), dtype=np.uint64)
    for i, k in enumerate(sorted(occ)):
        a = arcs[k]
        A = sum(min(a[j], 63) << 6 * j for j in range(4)) | min(occ[k], 255) << 24
        B = sum(min(a[4 + j], 63) << 6 * j for j in range(4)) | (1 << 27 if occ[k] == 1 else 0) | (1 << 25 if k in deleted else 0)
        rec[i, :nw] = M.words_of_key(k, nw)
        rec[i, nw] = A | B << 32
        rec[i, nw + 1] = i
    return rec


def canon(a, K):
    assert len(a) == K
    return M.canonical_kmers(a, K)[0]


@functools.lru_cache(maxsize=None)
def linear(K):
    """A genome of K + 170 bases whose 171 canonical k-mers are distinct."""
    g = random_genome(4100 + K, K + 170)
    assert distinct_kmers([g], K) == len(g) - K + 1
    return g


@functools.lru_cache(maxsize=None)
def linear_counts(K, copies):
    return count([(tile(linear(K), K), copies)], K)


@functools.lru_cache(maxsize=None)
def forked(K):
    """(prefix, suffix A, suffix B) of K + 40 bases each, A and B beginning with different bases: prefix + A and prefix + B share the
    prefix's k-mers and no other."""
    rng = np.random.default_rng(4200 + K)
    P, SA, SB = (rng.integers(0, 4, size=K + 40, dtype=np.uint8) for _ in range(3))
    SB[0] = (int(SA[0]) + 1 + int(rng.integers(0, 3))) & 3
    g1, g2 = np.concatenate([P, SA]), np.concatenate([P, SB])
    assert distinct_kmers([g1, g2], K) == 2 * (len(g1) - K + 1) - (len(P) - K + 1)
    return P, SA, SB


@functools.lru_cache(maxsize=None)
def cases(K, mer127):
    nw = 4 if mer127 else 2
    MX = api.WALK_MAX_EXT
    g = linear(K)
    G = len(g)
    out = []
    lin3 = records_of(*linear_counts(K, 3), nw)

    # a linear genome tiled by reads of both strands: a seed in the middle reaches both ends, its reverse complement gives the walks swapped,
    # and a longer sequence walks from its own two ends
    p = 60
    right, left = g[p + K:], rc(g[:p])
    out.append(Case("linear", lin3, [g[p:p + K], rc(g[p:p + K]), g[p:p + K + 37]], 1, 1, MX,
                    {0: (right, W.DEAD_END), 1: (left, W.DEAD_END), 2: (left, W.DEAD_END), 3: (right, W.DEAD_END), 4: (g[p + K + 37:], W.DEAD_END),
                     5: (left, W.DEAD_END)}))

    # two genomes that share a prefix: BRANCH_OUT at the prefix's last k-mer; from inside a branch towards the prefix, BRANCH_IN one k-mer before it
    P, SA, SB = forked(K)
    g1, g2, nP = np.concatenate([P, SA]), np.concatenate([P, SB]), len(P)
    fork = records_of(*count([(tile(g1, K), 2), (tile(g2, K), 2)], K), nw)
    s = nP + 10
    out.append(Case("shared-prefix", fork, [P[5:5 + K], g1[s:s + K]], 1, 1, MX,
                    {0: (P[5 + K:], W.BRANCH_OUT), 1: (rc(P[:5]), W.DEAD_END), 2: (g1[s + K:], W.DEAD_END), 3: (rc(g1[nP - K + 1:s]), W.BRANCH_IN)}))

    # a branch carried by one read beside one carried by five: min_arc = 1 stops at it, min_arc = 2 walks through
    minor = np.concatenate([P, SB])[nP - K - 3:nP + K + 3]
    skew = records_of(*count([(tile(g1, K), 5), ([minor], 1)], K), nw)
    out.append(Case("minor-branch-arc1", skew, [P[5:5 + K]], 1, 1, MX, {0: (P[5 + K:], W.BRANCH_OUT), 1: (rc(P[:5]), W.DEAD_END)}))
    out.append(Case("minor-branch-arc2", skew, [P[5:5 + K]], 1, 2, MX, {0: (g1[5 + K:], W.DEAD_END), 1: (rc(P[:5]), W.DEAD_END)}))

    # WEAK_NEXT: a successor below min_cov while its arc counts -- k-mers 0 .. t - 1 lie in four tilings, k-mer t and the rest in one
    t = 100
    occ, arcs = count([(tile(g[:t + K - 1], K), 3), (tile(g, K), 1)], K)
    at = lambda j: canon(g[j:j + K], K)
    assert all(occ[at(j)] >= 4 for j in range(t)) and occ[at(t)] < 4 and all(occ[at(j)] < 4 for j in range(t, t + 60))
    out.append(Case("weak-next-coverage", records_of(occ, arcs, nw), [g[20:20 + K]], 4, 1, MX,
                    {0: (g[20 + K:t + K - 1], W.WEAK_NEXT), 1: (rc(g[:20]), W.DEAD_END)}))
    # ... and a successor whose record has the deleted bit set, met from either side
    occ, arcs = linear_counts(K, 3)
    s = t + 30
    out.append(Case("weak-next-deleted", records_of(occ, arcs, nw, deleted={at(t)}), [g[20:20 + K], g[s:s + K]], 1, 1, MX,
                    {0: (g[20 + K:t + K - 1], W.WEAK_NEXT), 1: (rc(g[:20]), W.DEAD_END), 2: (g[s + K:], W.DEAD_END), 3: (rc(g[t + 1:s]), W.WEAK_NEXT)}))

    # a circular genome of C bases: LOOP with length C - 1, either way round
    c = random_genome(4300 + K, K + 150)
    C = len(c)
    assert distinct_kmers([np.concatenate([c, c[:K - 1]])], K) == C
    cc = np.concatenate([c, c])
    out.append(Case("circular", records_of(*count([(tile(c, K, circular=True), 2)], K), nw), [c[7:7 + K]], 1, 1, MX,
                    {0: (cc[7 + K:7 + K + C - 1], W.LOOP), 1: (rc(cc[8:C + 7]), W.LOOP)}))

    # max_ext at the packer's word edges: pad bits zero, and the shorter left walk leaves the rest of its row zero
    for m in (1, 31, 32, 33, 64, 65):
        out.append(Case("max-ext-%d" % m, lin3, [g[10:10 + K]], 1, 1, m,
                        {0: (g[10 + K:10 + K + m], W.MAX_EXT), 1: (rc(g[:10])[:m], W.MAX_EXT if m <= 10 else W.DEAD_END)}))

    # SEED_WEAK: a seed that is not in the set, and seeds below min_cov; NO_KMER: sequences shorter than K between others
    foreign = random_genome(4400 + K, K)
    assert canon(foreign, K) not in linear_counts(K, 3)[0]
    out.append(Case("seed-absent", lin3, [foreign, g[20:20 + K]], 1, 1, MX, {0: ([], W.SEED_WEAK), 1: ([], W.SEED_WEAK), 2: (g[20 + K:], W.DEAD_END)}))
    out.append(Case("seed-weak", lin3, [foreign, g[20:20 + K]], 255, 1, MX, {v: ([], W.SEED_WEAK) for v in range(4)}))
    out.append(Case("no-kmer", lin3, [g[:K - 1], codes([]), g[20:20 + K], g[5:8], g[30:30 + K + 1]], 1, 1, MX,
                    {0: ([], W.NO_KMER), 1: ([], W.NO_KMER), 2: ([], W.NO_KMER), 3: ([], W.NO_KMER), 4: (g[20 + K:], W.DEAD_END), 6: ([], W.NO_KMER),
                     7: ([], W.NO_KMER), 9: (rc(g[:30]), W.DEAD_END)}))

    # arc counters at 63: 100 copies of the tiling saturate every counter (and many coverages), and min_arc = 63 still walks; the 3-copy
    # set has no such arc
    occ, arcs = linear_counts(K, 100)
    assert all(v in (0, 63) for a in arcs.values() for v in (min(x, 63) for x in a)) and max(occ.values()) > 255
    out.append(Case("arc-63", records_of(occ, arcs, nw), [g[p:p + K]], 1, 63, MX, {0: (right, W.DEAD_END), 1: (left, W.DEAD_END)}))
    out.append(Case("arc-63-absent", lin3, [g[p:p + K]], 1, 63, MX, {0: ([], W.DEAD_END), 1: ([], W.DEAD_END)}))
    return out


def batch(K, n):
    """n seed k-mers of the linear genome, from places 7 apart."""
    g = linear(K)
    return [g[(7 * i) % (len(g) - K + 1):][:K] for i in range(n)]


def codes_of_key(key, K):
    return codes([(key >> 2 * (K - 1 - i)) & 3 for i in range(K)])


class Walker:
    """An index under test with its model: device = -1 the host twin over numpy, else the device build over torch tensors.  A call goes
    straight to pg_kindex_walk with output buffers of exactly the stated sizes, pre-filled with FILL."""

    def __init__(self, records, K, mer127, device, model=None):
        self.K, self.mer127, self.device = K, mer127, device
        self.nw = 4 if mer127 else 2
        self.model = model if model is not None else M.Model.from_records(records, K, self.nw)
        self.ix = api.KmerIndex.from_records(records, K, mer127, device)

    def close(self):
        self.ix.close()

    def up(self, a):
        if self.device < 0:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64)).to("cuda:%d" % self.device)

    def down(self, a):
        return a if self.device < 0 else a.cpu().numpy().view(np.uint64)

    def pack(self, seqs, uniform):
        """(words, word_off, kmer_base, uniform_len) on the index's side; a uniform batch has no offsets."""
        if uniform:
            stacked = np.stack([codes(s) for s in seqs])
            return self.up(api.pack_reads_uniform(stacked)), None, None, stacked.shape[1]
        words, off, base = api.pack_seqs_ragged(seqs, self.K)
        return self.up(words), self.up(off) if len(seqs) else None, self.up(base), 0

    def call(self, packed, off, base, n, ulen, min_cov, min_arc, max_ext, ext, rep, n_words=None):
        p = self.ix._ptr
        return api.lib().pg_kindex_walk(self.ix.h, p(packed), (packed.size if self.device < 0 else packed.numel()) if n_words is None else n_words,
                                        p(off), p(base), n, ulen, min_cov, min_arc, max_ext, p(ext), p(rep), self.ix._stream())

    def outputs(self, n, max_ext):
        row = (max_ext + 31) // 32
        return self.up(np.full(max(2 * n * row, 1), FILL, dtype=np.uint64)), self.up(np.full(max(4 * n, 1), FILL, dtype=np.uint64))

    def run(self, seqs, min_cov=1, min_arc=1, max_ext=api.WALK_MAX_EXT, uniform=False):
        """(rows (2 n, row words), report (4 n,)) as numpy arrays."""
        n, row = len(seqs), (max_ext + 31) // 32
        packed, off, base, ulen = self.pack(seqs, uniform)
        ext, rep = self.outputs(n, max_ext)
        rc_ = self.call(packed, off, base, n, ulen, min_cov, min_arc, max_ext, ext, rep)
        assert rc_ == 0, api.lib().pg_last_error()
        ext, rep = self.down(ext), self.down(rep)
        assert ext.size == max(2 * n * row, 1) and rep.size == max(4 * n, 1)
        return ext[:2 * n * row].reshape(2 * n, row), rep[:4 * n]

    def check(self, seqs, what, min_cov=1, min_arc=1, max_ext=api.WALK_MAX_EXT, uniform=False):
        """A batch against the model, word for word; returns what came back and the model's walks."""
        rows, rep = self.run(seqs, min_cov, min_arc, max_ext, uniform)
        w_rows, w_rep, walks = W.want(self.model, seqs, min_cov, min_arc, max_ext)
        assert rep.shape == w_rep.shape and (rep == w_rep).all(), "%s: reports differ from the model" % what
        assert rows.shape == w_rows.shape and (rows == w_rows).all(), "%s: rows differ from the model" % what
        return rows, rep, walks


def check_case(c, K, mer127, device, twin=None):
    """One design: the model's words, the text and reason the construction dictates, and -- twin: a host index of the same records --
    the host twin's words."""
    what = "%s %s" % (c.name, flavour_id((K, mer127)))
    w = Walker(c.records, K, mer127, device)
    try:
        rows, rep, walks = w.check(c.seqs, what, c.min_cov, c.min_arc, c.max_ext)
        for v, (text, reason) in c.expect.items():
            got_text, got_reason, _ = walks[v]
            assert got_reason == reason, "%s: walk %d stopped with %s, the design says %s" % (what, v, W.NAMES[got_reason], W.NAMES[reason])
            assert got_text == [int(x) for x in text], "%s: walk %d's text is not the design's" % (what, v)
        f = api.walk_fields(rep)
        assert f["reason"] == [W.NAMES[r] for _, r, _ in walks] and list(f["len"]) == [len(e) for e, _, _ in walks]
        assert list(f["coverage_sum"]) == [cov for _, _, cov in walks]
        # the report alone, the rows alone: the same words, the other buffer untouched
        packed, off, base, ulen = w.pack(c.seqs, False)
        n = len(c.seqs)
        ext, rp = w.outputs(n, c.max_ext)
        assert w.call(packed, off, base, n, ulen, c.min_cov, c.min_arc, c.max_ext, None, rp) == 0 and (w.down(rp)[:4 * n] == rep).all()
        assert w.call(packed, off, base, n, ulen, c.min_cov, c.min_arc, c.max_ext, ext, None) == 0 and (w.down(ext)[:rows.size] == rows.reshape(-1)).all()
        if len({len(s) for s in c.seqs}) == 1:
            u_rows, u_rep = w.run(c.seqs, c.min_cov, c.min_arc, c.max_ext, uniform=True)
            assert (u_rows == rows).all() and (u_rep == rep).all(), what + ": a uniform batch differs from the ragged one"
        if twin is not None:
            h = Walker(c.records, K, mer127, twin, model=w.model)
            try:
                h_rows, h_rep = h.run(c.seqs, c.min_cov, c.min_arc, c.max_ext)
            finally:
                h.close()
            assert (h_rows == rows).all() and (h_rep == rep).all(), what + ": the device differs from the host twin"
    finally:
        w.close()


def check_flavour(K, mer127, device, twin=None):
    for c in cases(K, mer127):
        check_case(c, K, mer127, device, twin)


def check_batches(K, mer127, device):
    """32, 33, 128 and 129 sequences -- 64, 66, 256 and 258 walks, the wave's and the workgroup's edges -- ragged and uniform, with
    max_ext = 40 (a word and a part of one); an empty batch touches nothing; the api's methods give the same words."""
    nw = 4 if mer127 else 2
    w = Walker(records_of(*linear_counts(K, 3), nw), K, mer127, device)
    try:
        for n in (32, 33, 128, 129):
            what = "%d sequences %s" % (n, flavour_id((K, mer127)))
            seqs = batch(K, n)
            rows, rep, walks = w.check(seqs, what, max_ext=40)
            u_rows, u_rep, _ = w.check(seqs, what + " uniform", max_ext=40, uniform=True)
            assert (rows == u_rows).all() and (rep == u_rep).all()
            assert {r for _, r, _ in walks} == {W.MAX_EXT, W.DEAD_END}
        ext, rep = w.outputs(3, 40)
        assert w.call(None, None, None, 0, 0, 1, 1, 40, ext, rep, n_words=0) == 0
        assert (w.down(ext) == FILL).all() and (w.down(rep) == FILL).all()
        seqs = batch(K, 33)
        rows, rep, _ = w.check(seqs, "api", max_ext=api.WALK_MAX_EXT)
        words, off, base = api.pack_seqs_ragged(seqs, K)
        a_rows, a_rep = w.ix.walk_ragged(w.up(words), w.up(off), w.up(base), len(seqs), 1)
        assert (w.down(a_rows) == rows).all() and (w.down(a_rep) == rep).all()
        a_rows, a_rep = w.ix.walk_uniform(w.up(api.pack_reads_uniform(np.stack(seqs))), len(seqs), K, 1, 1, 40)
        assert a_rows.shape == (66, 2) and (w.down(a_rows) == w.run(seqs, max_ext=40)[0]).all()
    finally:
        w.close()


def check_fuzz(name, K, mer127, device, params):
    """A table of kindex_cases with random counter words (about half of them deleted), every key a seed: a fuzz of the arc decoding and,
    for "colliding", of long probe runs."""
    records, keys = KC.table(name, K, mer127)
    w = Walker(records, K, mer127, device)
    try:
        seqs = [codes_of_key(k, K) for k in keys]
        met = set()
        for min_cov, min_arc in params:
            _, _, walks = w.check(seqs, "%s %s min_cov %d min_arc %d" % (name, flavour_id((K, mer127)), min_cov, min_arc), min_cov, min_arc, 64)
            met |= {r for _, r, _ in walks}
        assert met >= {W.SEED_WEAK, W.DEAD_END, W.BRANCH_OUT, W.WEAK_NEXT}, met
    finally:
        w.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with nothing written: the parameter ranges, both outputs null, n_words without the tail, a cut index."""
    nw = 4 if mer127 else 2
    records = records_of(*linear_counts(K, 3), nw)
    w = Walker(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    try:
        seqs = batch(K, 5)
        packed, off, base, _ = w.pack(seqs, False)
        ext, rep = w.outputs(5, 40)
        n_words = int(packed.size if device < 0 else packed.numel())
        call = lambda min_cov=1, min_arc=1, max_ext=40, e=ext, r=rep, n_words=None: w.call(packed, off, base, 5, 0, min_cov, min_arc, max_ext, e, r, n_words)
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64), dict(max_ext=0), dict(max_ext=api.WALK_EXT_BOUND + 1)):
            assert call(**bad) == EINVAL and b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert call(e=None, r=None) == EINVAL and b"both null" in L.pg_last_error()
        assert call(n_words=nw) == EINVAL and b"n_words" in L.pg_last_error()
        u = w.up(api.pack_reads_uniform(np.stack(seqs)))
        assert w.call(u, None, None, 5, K, 1, 1, 40, ext, rep, n_words=5 * ((K + 31) // 32) + nw) == EINVAL
        assert w.call(packed, None, base, 5, 0, 1, 1, 40, ext, rep) == EINVAL
        assert L.pg_kindex_walk(None, None, 0, None, None, 0, 0, 1, 1, 40, None, None, None) == EINVAL
        p = w.ix._ptr
        assert L.pg_kindex_walk(cut.h, p(packed), n_words, p(off), p(base), 5, 0, 1, 1, 40, p(ext), p(rep), w.ix._stream()) == ESTATE
        assert b"one lookup after the other in one table" in L.pg_last_error()
        with pytest.raises(api.PgError):
            cut.walk_ragged(packed, off, base, 5, 1)
        with pytest.raises(api.PgError):
            w.ix.walk_ragged(packed, off, base, 5, 0)
        assert (w.down(ext) == FILL).all() and (w.down(rep) == FILL).all()
        assert call(max_ext=api.WALK_EXT_BOUND, e=None) == 0                 # (the bound itself is taken: the report alone needs no rows)
        assert call(n_words=n_words) == 0
    finally:
        cut.close()
        w.close()
