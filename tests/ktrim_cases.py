"""The trim's cases, shared by tests/test_ktrim_host.py (the host twin) and tests/test_gpu_ktrim.py (the kernels): the genomes and tables
of tests/kcorrect_cases.py -- a random genome with a fixed seed whose k-mers have coverage COV, with the K k-mers round one place at
exactly MIN_COV, round another at MIN_COV - 1, and one record with the `deleted` bit -- reads cut from it with designed weak stretches,
and the comparison of every output array with the model (tests/ktrim_model.py).  Every case names the span it was designed for, and
`designed` asserts that the model gives it: a case that does not do what its name says fails on the CPU.  All comparisons are of integers
and exact.

Batches are packed here with exactly nw + 1 words behind the last read, those words and every read's pad bits filled with ones; the
output's pad bits and its nw + 1 tail words must be zero all the same."""
import functools

import numpy as np

import kcorrect_cases as C
import kindex_model as M
import ktrim_model as T
from soapdenovo2_amd import api

FLAVOURS = C.FLAVOURS
flavour_id = C.flavour_id
MIN_COV = C.MIN_COV
BATCHES = [1, 63, 64, 65, 257, 4097]
RANKS = [1, 2, 3, 8]
STARTS = [0, 1, 31, 32, 33, 63, 64]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def min_len_of(K):
    return K + 5


def _hit(read, positions):
    r = np.array(read, dtype=np.uint8)
    for p in positions:
        r[p] = (r[p] + 2) & 3                    # (never base + 1: the corrector's table holds that variant at two places)
    return r


class Case:
    def __init__(self, name, read, span, kept, min_len=None):
        self.name, self.read, self.span, self.kept, self.min_len = name, np.asarray(read, dtype=np.uint8), span, kept, min_len


@functools.lru_cache(maxsize=None)
def cases(K):
    """The designed reads: (name, read, the (start, len) the rule gives, kept or not with min_len -- min_len_of(K) unless the case has its own)."""
    g, L, m_len = C.genome(K), C.read_len(K), min_len_of(K)
    out = []

    def one(name, read, span, kept, min_len=None):
        out.append(Case(name, read, span, kept, min_len))

    plain = g[C.PLAIN:C.PLAIN + L]
    one("all-solid", plain, (0, L), True)
    one("all-solid-reverse-complement", C.rc(plain), (0, L), True)
    one("no-solid-kmer", np.random.default_rng(9).integers(0, 4, size=L, dtype=np.uint8), (0, 0), False)
    one("shorter-than-K", g[C.PLAIN:C.PLAIN + K - 1], (0, 0), False)
    one("empty", g[:0], (0, 0), False)
    one("exactly-K-dropped", g[C.PLAIN:C.PLAIN + K], (0, K), False, min_len=K + 1)
    one("exactly-K-kept", g[C.PLAIN:C.PLAIN + K], (0, K), True, min_len=K)
    one("exactly-K-weak", _hit(g[C.PLAIN:C.PLAIN + K], [K // 2]), (0, 0), False, min_len=K)
    one("K+1", g[C.PLAIN:C.PLAIN + K + 1], (0, K + 1), True, min_len=K + 1)
    # one substitution at p: the k-mers that hold it are weak, p bases stay on the left and len - p - 1 on the right
    p = L - K - 8
    one("weak-middle-left-longer", _hit(plain, [p]), (0, p), True)
    p = K + 2
    one("weak-middle-right-longer", _hit(plain, [p]), (p + 1, L - p - 1), True)
    p = K + 10
    one("weak-middle-equal-left-wins", _hit(g[C.PLAIN2:C.PLAIN2 + 2 * p + 1], [p]), (0, p), True)
    one("two-weak-stretches-middle-run", _hit(plain, [3, L - 4]), (4, L - 8), True)
    # the last base wrong: only the last k-mer is weak
    one("span-exactly-min-len", _hit(g[C.PLAIN:C.PLAIN + m_len + 1], [m_len]), (0, m_len), True)
    one("span-min-len-minus-1", _hit(g[C.PLAIN:C.PLAIN + m_len], [m_len - 1]), (0, m_len - 1), False)
    long_len = 128 + 3 * K + 7                   # (the run right of base 64 is longer than the one left of it)
    for s in STARTS:
        rd = g[C.PLAIN2:C.PLAIN2 + long_len]
        one("span-starts-at-%d" % s, _hit(rd, [s - 1]) if s else _hit(rd, [long_len - 1]), (s, long_len - s) if s else (0, long_len - 1), True)
    m = (K + 1 + 31) // 32 + 1
    for n in (32 * m, 32 * m + 1):
        one("span-of-%d-bases" % n, _hit(g[C.PLAIN:C.PLAIN + 5 + n], [4]), (5, n), True)
    # the table's designed places: coverage exactly MIN_COV is solid, MIN_COV - 1 is not, a deleted record reads as absent
    at = K + 5
    one("coverage-at-min", g[C.P_AT_MIN - at:C.P_AT_MIN - at + L], (0, L), True)
    one("coverage-below-min", g[C.P_BELOW_MIN - at:C.P_BELOW_MIN - at + L], (at + 1, L - at - 1), True)
    j = at - K + 4                               # (the deleted record is the fourth k-mer that holds base P_DELETED)
    one("deleted-record", g[C.P_DELETED - at:C.P_DELETED - at + L], (j + 1, L - j - 1), True)
    # 4 097 k-mers through the lane kernels: from the first base to the k-mers of P_BELOW_MIN
    one("4097-kmers", g[C.PLAIN:C.PLAIN + 4096 + K], (0, C.P_BELOW_MIN - C.PLAIN), True)
    # the batch's last read: its span ends in its last base, which is the last base of a full word
    one("ends-in-last-base-of-batch", _hit(g[C.PLAIN2:C.PLAIN2 + 32 * m], [2]), (3, 32 * m - 3), True)
    return out


_spans = {}


def model_span(model, read, min_cov=MIN_COV):
    key = (id(model), min_cov, bytes(np.asarray(read, dtype=np.uint8)))
    if key not in _spans:
        _spans[key] = T.span(model, read, min_cov)
    return _spans[key]


def want(model, reads, min_len, min_cov=MIN_COV):
    return T.Trimmed(model, reads, min_cov, min_len, spans=[model_span(model, r, min_cov) for r in reads])


def designed(model, case):
    """The model's answer for a case is the span the case was built for, and it is kept or dropped as designed."""
    got = model_span(model, case.read)
    assert got == case.span, "%s: the model gives %s, designed for %s" % (case.name, got, case.span)
    assert (got[1] >= (case.min_len or min_len_of(model.K))) == case.kept, case.name


# ---- batches ----
def pack(reads, K, nw, uniform):
    """kcorrect_cases.pack, vectorised: (words, word_off, kmer_base, uniform_len) with exactly nw + 1 words behind the last read; those
    and every read's pad bits are ones."""
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    wpr = (lens + 31) // 32
    off = np.concatenate([[0], np.cumsum(wpr)]).astype(np.uint64)
    words = np.full(int(off[-1]) + nw + 1, ONES, dtype=np.uint64)
    shifts = (62 - 2 * np.arange(32)).astype(np.uint64)
    for i, r in enumerate(reads):
        if len(r):
            c = np.full(int(wpr[i]) * 32, 3, dtype=np.uint64)
            c[:len(r)] = r
            words[int(off[i]):int(off[i + 1])] = np.bitwise_or.reduce(c.reshape(-1, 32) << shifts[None, :], axis=1)
    if uniform:
        assert len(set(lens.tolist())) == 1
        return words, None, None, int(lens[0])
    base = np.concatenate([[0], np.cumsum(np.maximum(lens - K + 1, 0))]).astype(np.uint64)
    return words, off[:-1].copy(), base, 0


_check_pack = pack([np.arange(40) % 4, np.zeros(0, dtype=np.uint8), np.array([1])], 13, 2, False)
assert all((a == b).all() for a, b in zip(_check_pack[:3], C.pack([np.arange(40) % 4, np.zeros(0, dtype=np.uint8), np.array([1])], 13, 2, False)[:3]))


class Trimmer:
    """An index under test with its model: device = -1 the host twin over numpy, an ordinal the device build over torch tensors, a tuple
    the index cut over those ranks (all -1: the host twin's cut)."""

    def __init__(self, K, mer127, device, records=None, model=None):
        self.K, self.mer127, self.nw = K, mer127, 4 if mer127 else 2
        self.device = device if isinstance(device, int) else device[0]
        self.model = model or (C.model_of(K, mer127) if records is None else M.Model.from_records(records, K, self.nw))
        self.ix = api.KmerIndex.from_records(C.table(K, mer127) if records is None else records, K, mer127, device)

    def close(self):
        self.ix.close()

    def up(self, a):
        if a is None or self.device < 0:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64)).to("cuda:%d" % self.device)

    def down(self, a):
        return a if self.device < 0 else a.cpu().numpy().view(np.uint64)

    def run(self, reads, min_len, uniform=False, pack_out=True, min_cov=MIN_COV):
        """The outputs of one batch as numpy arrays: the spans alone, or (spans, packed_out, word_off_out, kmer_base_out, src_out, totals)
        at their full capacities."""
        words, off, base, ulen = pack(reads, self.K, self.nw, uniform)
        d_words = self.up(words.copy())
        if uniform:
            got = self.ix.trim_uniform(d_words, len(reads), ulen, min_cov, min_len, pack=pack_out)
        else:
            got = self.ix.trim_ragged(d_words, self.up(off), self.up(base), len(reads), int(base[-1]), min_cov, min_len, pack=pack_out)
        assert (self.down(d_words) == words).all(), "the input batch was written to"
        return [self.down(o) for o in got] if pack_out else self.down(got)

    def check(self, reads, what, min_len=None, uniform=False, min_cov=MIN_COV):
        """One batch against the model: every output array and the totals, whole.  Returns the used part of the outputs."""
        min_len = min_len_of(self.K) if min_len is None else min_len
        w = want(self.model, reads, min_len, min_cov)
        spans, packed, word_off, kmer_base, src, totals = self.run(reads, min_len, uniform, True, min_cov)
        n_kept, n_words = int(w.totals[0]), int(w.totals[1])
        assert spans.shape == w.spans.shape and (spans == w.spans).all(), "%s: spans differ from the model" % what
        assert (totals == w.totals).all(), "%s: totals %s, the model's %s" % (what, totals, w.totals)
        assert (src[:n_kept] == w.src).all(), "%s: src_out differs from the model" % what
        assert (word_off[:n_kept] == w.word_off).all(), "%s: word_off_out differs from the model" % what
        assert (kmer_base[:n_kept + 1] == w.kmer_base).all(), "%s: kmer_base_out differs from the model" % what
        assert len(packed) >= n_words + self.nw + 1
        assert (packed[:n_words + self.nw + 1] == w.words).all(), "%s: output words differ from the model" % what
        assert not packed[n_words + self.nw + 1:].any(), "%s: words behind the tail were written" % what
        only = self.run(reads, min_len, uniform, False, min_cov)
        assert (only == w.spans).all(), "%s: spans alone differ from the model" % what
        return packed[:n_words + self.nw + 1], word_off[:n_kept], kmer_base[:n_kept + 1], src[:n_kept], totals


def batch_of(K, n, seed):
    """n reads of one length with a seeded random keep / drop pattern (reads kept whole, kept trimmed at either end, and dropped ones)."""
    cs = cases(K)
    L = C.read_len(K)
    pool = [c.read for c in cs if len(c.read) == L]
    assert any(c.kept for c in cs if len(c.read) == L) and any(not c.kept for c in cs if len(c.read) == L)
    pick = np.random.default_rng(seed).integers(0, len(pool), size=n)
    return [pool[i] for i in pick]


def check_flavour(K, mer127, device, batches=BATCHES):
    """Every designed case, alone and in batches, against the model."""
    t = Trimmer(K, mer127, device)
    try:
        cs = cases(K)
        for c in cs:
            designed(t.model, c)
            t.check([c.read], c.name, min_len=c.min_len)
            if len(c.read):
                t.check([c.read], c.name + ", uniform", min_len=c.min_len, uniform=True)
        reads = [c.read for c in cs]
        assert len(reads[-1]) % 32 == 0 and cs[-1].span[0] + cs[-1].span[1] == len(reads[-1])
        for min_len in (K, K + 1, min_len_of(K)):
            t.check(reads, "all cases, min_len %d" % min_len, min_len=min_len)
        none = np.zeros(K - 1, dtype=np.uint8)
        t.check([none, reads[0], none, none, reads[9], np.zeros(0, dtype=np.uint8), reads[10], none], "k-mer-less between")
        t.check([none, none], "only k-mer-less")
        for n in batches:
            batch = batch_of(K, n, 100 + n)
            u = t.check(batch, "uniform %d" % n, uniform=True)
            r = t.check(batch, "ragged %d" % n)
            assert all((a == b).all() for a, b in zip(u, r))
        kept = [c.read for c in cs if c.kept and c.min_len is None]
        dropped = [c.read for c in cs if not c.kept and c.min_len is None]
        got = t.check(kept, "all kept")
        assert int(got[4][0]) == len(kept)
        got = t.check(dropped, "all dropped")
        assert int(got[4][0]) == 0 and len(got[0]) == t.nw + 1
    finally:
        t.close()


# ---- batches of 65 536 and 65 537 reads: 256 blocks of 256 are exactly one round of the scan over the blocks' sums, the 257th block is
# the first of its second round ----
ROUND = 256 * 256


def check_rounds(device, twin=None):
    """K = 13, uniform reads of K + 3 bases, each one of two templates by a seeded random bit: a stretch of the genome that is solid
    throughout (kept whole) or the one whose four k-mers all hold the base at P_BELOW_MIN (coverage MIN_COV - 1: dropped).  Every
    output is then a cumulative sum of the bit vector, and the output words are the kept template's word repeated."""
    K, L, nw, nk = 13, 16, 2, 4
    g = C.genome(K)
    t = Trimmer(K, False, device)
    h = Trimmer(K, False, twin, model=t.model) if twin is not None else None
    try:
        keep, drop = g[C.PLAIN:C.PLAIN + L], g[C.P_BELOW_MIN - 3:C.P_BELOW_MIN - 3 + L]
        assert model_span(t.model, keep) == (0, L) and T.solid_flags(t.model, drop, MIN_COV) == [False] * nk
        w_keep, w_drop = pack([keep], K, nw, True)[0][0], pack([drop], K, nw, True)[0][0]
        w_out = w_keep & ~np.uint64(0xFFFFFFFF)                                # (16 bases: the low half of the word is pad)
        for n in (ROUND, ROUND + 1):
            bits = np.random.default_rng(600 + n).integers(0, 2, size=n).astype(bool)
            words = np.concatenate([np.where(bits, w_keep, w_drop), np.full(nw + 1, ONES)]).astype(np.uint64)
            before = (np.cumsum(bits) - bits).astype(np.uint64)               # the kept reads in front of each read
            kept = int(bits.sum())
            assert 0 < kept < n
            want = [np.where(bits, np.uint64(L << 32), np.uint64(0)), np.concatenate([np.full(kept, w_out), np.zeros(nw + 1, dtype=np.uint64)]),
                    before[bits], np.concatenate([before[bits] * np.uint64(nk), [np.uint64(kept * nk)]]), np.flatnonzero(bits).astype(np.uint64),
                    np.array([kept, kept, kept * nk, (n - kept) * L], dtype=np.uint64)]
            sizes = [n, kept + nw + 1, kept, kept + 1, kept, 4]
            for who in (t, h):
                if who is None:
                    continue
                got = [who.down(o) for o in who.ix.trim_uniform(who.up(words.copy()), n, L, MIN_COV, K + 1)]
                for name, a, b, m in zip(("spans", "packed_out", "word_off_out", "kmer_base_out", "src_out", "totals"), got, want, sizes):
                    assert (a[:m] == b).all(), "%d reads: %s differs from the cumulative sums of the bit vector" % (n, name)
                assert not got[1][kept + nw + 1:].any(), "%d reads: words behind the tail were written" % n
    finally:
        t.close()
        if h is not None:
            h.close()


def check_ranks(K, mer127, devices_of):
    """The index cut over 1, 2, 3 and 8 ranks gives the single table's words (and the model's)."""
    reads = [c.read for c in cases(K)] + batch_of(K, 257, 7)
    one = Trimmer(K, mer127, devices_of(1)[0])
    try:
        ref = one.check(reads, "one table")
    finally:
        one.close()
    for n in RANKS:
        t = Trimmer(K, mer127, devices_of(n))
        try:
            assert t.ix.sharded
            got = t.check(reads, "%d ranks" % n)
            assert all((a == b).all() for a, b in zip(got, ref))
            u = batch_of(K, 65, 8)
            t.check(u, "%d ranks, uniform" % n, uniform=True)
        finally:
            t.close()


# ---- the simulated set of kcorrect_cases: a circular genome, reads from both strands, substitutions with probability 0.005 ----
def all_solid(model, read, min_cov):
    return all(T.solid_flags(model, read, min_cov))


def unpack(packed, word_off, kmer_base, K):
    """The kept reads of an output batch as base-code arrays (their lengths are their k-mers + K - 1)."""
    lens = (kmer_base[1:] - kmer_base[:-1]).astype(np.int64) + K - 1
    return [api.unpack_seq(packed[int(o):], int(n)) for o, n in zip(word_off, lens)]


def check_recount(model, kept, min_cov):
    """Every k-mer of every kept read is solid, so a recount of the kept reads holds no weak k-mer."""
    assert all(len(r) >= model.K + 1 and all_solid(model, r, min_cov) for r in kept)
    occ, _ = M.count_reads(kept, model.K)
    assert all(M.coverage(model.cnt.get(k, 0)) >= min_cov for k in occ)
    return len(occ)
