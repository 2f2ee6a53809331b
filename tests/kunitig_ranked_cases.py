"""The ranked unitigs' cases, shared by tests/test_kunitig_ranked_host.py (the host twin) and tests/test_gpu_kunitig_ranked.py (the
kernels): pg_kindex_unitigs_ranked (csrc/krank.hpp) through the checks of tests/kunitig_cases.py -- its builders and those of
tests/kwalk_cases.py unchanged, its Compactor with the call replaced -- against the model (tests/kunitig_model.py) at its default guard,
which is the answer when nothing is cut, and against what each construction dictates.  On top of the walking engine's designs: a ladder
of chain lengths round every power of two, chains alone in their index (keys == n: the rounds launched are the rounds needed), rings of
many lengths beside a chain and alone, and one chain of 65 537 k-mers.  All comparisons are of integers and exact."""
import contextlib
import functools

import numpy as np
import pytest

import kindex_cases as KC
import kunitig_cases as G
import kunitig_model as U
import kwalk_cases as E
import kwalk_model as W
from soapdenovo2_amd import api

FLAVOURS = G.FLAVOURS
flavour_id = G.flavour_id
FILL, MAXK = G.FILL, G.MAXK
EINVAL, ESTATE = G.EINVAL, G.ESTATE
D = U.DEAD_END

LADDER = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ALONE = (1, 2, 256, 257, 1024, 1025)
RINGS_ALONE = (256, 257)
LONG, LONG_K, LONG_SEED = 65537, 31, 5100


def rings_beside(K):
    return tuple(sorted({n for n in (K + 1, 64, 65, 255, 256, 257, 1000) if n > K}))        # (a ring here has more than K k-mers)


class Compactor(G.Compactor):
    """kunitig_cases.Compactor whose call goes to pg_kindex_unitigs_ranked: the same arguments without max_kmers, which is dropped."""

    def call(self, min_cov, min_arc, max_kmers, cap_unitigs, cap_words, packed, word_off, kmer_base, report, totals, ix=None):
        p = self.ix._ptr
        return api.lib().pg_kindex_unitigs_ranked((ix or self.ix).h, min_cov, min_arc, cap_unitigs, cap_words, p(packed), p(word_off), p(kmer_base),
                                                  p(report), p(totals), self.ix._stream())


@contextlib.contextmanager
def ranked():
    """kunitig_cases' checks with this module's Compactor: they name theirs at call time."""
    walk = G.Compactor
    G.Compactor = Compactor
    try:
        yield
    finally:
        G.Compactor = walk


def compare_twin(w, got, totals, records, K, mer127, twin, min_cov, min_arc, what):
    if twin is None:
        return
    h = Compactor(records, K, mer127, twin, model=w.model)
    try:
        h_got, h_totals = h.run(min_cov, min_arc, MAXK, what + " (host twin)")
    finally:
        h.close()
    assert sorted(h_got) == sorted(got) and h_totals == totals, what + ": the device differs from the host twin"


def check_records(records, K, mer127, device, expect, what, twin=None, min_cov=1, min_arc=1):
    """The records compacted: the model's unitigs with every check of the layout and the invariant, the design's (text, left, right)
    where there is one, nothing cut and every solid k-mer covered, and the host twin's."""
    w = Compactor(records, K, mer127, device)
    try:
        got, totals = w.check(min_cov, min_arc, MAXK, what)
        if expect is not None:
            assert sorted((t, l, r) for t, l, r, _ in got) == sorted(expect), "%s: not the unitigs the design dictates" % what
        assert totals[6] == 0 and totals[3] == totals[4] and totals[7] == 0, what
        compare_twin(w, got, totals, records, K, mer127, twin, min_cov, min_arc, what)
        return got, totals
    finally:
        w.close()


# ---- 1. the walking engine's designs, the guard gone ----
def check_designs(K, mer127, device, twin=None):
    """Every design of kunitig_cases.cases() against the model at its default guard; the design's unitigs, and for the two designs whose
    guard cuts -- "cut" at 50 k-mers, "circular-too-long" -- the whole genome once and the ring."""
    whole = {"cut": [G.emitted(E.linear(K), D, D, K)], "circular-too-long": [G.ring(G.circular(K), K)]}
    seen = set()
    for c in G.cases(K, mer127):
        expect = whole.get(c.name, c.expect)
        assert c.name in whole or c.max_kmers == MAXK or c.cut == 0
        seen.add(c.name)
        check_records(c.records, K, mer127, device, expect, "%s %s" % (c.name, flavour_id((K, mer127))), twin, c.min_cov, c.min_arc)
    assert seen >= set(whole)


# ---- 2. / 3. chains ----
def whole_reads(seqs, K, flip):
    """Every sequence as one read, counted twice (no k-mer is `single`); flip: reverse complemented."""
    return E.count([([E.rc(s) if flip else s for s in seqs], 2)], K)


@functools.lru_cache(maxsize=None)
def ladder(K):
    """Disjoint random linear sequences of n k-mers for every n of LADDER; their canonical k-mers are distinct."""
    rng = np.random.default_rng(5000 + K)
    seqs = [rng.integers(0, 4, size=n + K - 1, dtype=np.uint8) for n in LADDER]
    assert E.distinct_kmers(seqs, K) == sum(LADDER)
    return seqs


def check_ladder(K, mer127, device, twin=None):
    nw = 4 if mer127 else 2
    seqs = ladder(K)
    expect = [G.emitted(s, D, D, K) for s in seqs]
    for flip in (False, True):
        what = "ladder %s%s" % (flavour_id((K, mer127)), " rc reads" if flip else "")
        got, totals = check_records(E.records_of(*whole_reads(seqs, K, flip), nw), K, mer127, device, expect, what, twin)
        assert sorted(c for _, _, _, c in got) == sorted(2 * n for n in LADDER), what + ": the coverage sums"
        assert totals[0] == len(LADDER) and totals[4] == sum(LADDER) and totals[5] == 0


@functools.lru_cache(maxsize=None)
def alone(K, n):
    s = np.random.default_rng(5200 + 7 * n + K).integers(0, 4, size=n + K - 1, dtype=np.uint8)
    assert E.distinct_kmers([s], K) == n
    return s


def check_alone(K, mer127, device, n, twin=None):
    """A chain of n k-mers alone in its index: keys == n."""
    nw = 4 if mer127 else 2
    s = alone(K, n)
    records = E.records_of(*whole_reads([s], K, False), nw)
    assert len(records) == n
    got, totals = check_records(records, K, mer127, device, [G.emitted(s, D, D, K)], "alone %d %s" % (n, flavour_id((K, mer127))), twin)
    assert totals[:6] == [1, (n + K - 1 + 31) // 32 + nw + 1, n + K - 1, n, n, 0] and got[0][3] == 2 * n


# ---- 4. rings ----
@functools.lru_cache(maxsize=None)
def circle(K, n, seed=0):
    """A circular genome of n bases whose n canonical k-mers are distinct."""
    for attempt in range(64):
        c = np.random.default_rng(5300 + 1000 * seed + 64 * n + K + 100000 * attempt).integers(0, 4, size=n, dtype=np.uint8)
        if E.distinct_kmers([np.concatenate([c, c, c])[:n + K - 1]], K) == n:
            return c
    raise AssertionError("no circular genome of %d distinct %d-mers" % (n, K))


def round_once(c, K):
    """A read that goes once round the circle and K bases on: every k-mer with both of its arcs."""
    n = len(c)
    return np.concatenate([c] * (2 + (2 * K) // n))[:n + K]


def check_rings(K, mer127, device, sizes, chain, lone=0, twin=None):
    """Rings of the given sizes in one index, with a linear genome (chain) and `lone` isolated k-mers beside them: every ring once from
    its least canonical k-mer, the same from reverse-complemented reads, and rings behind the chains in the start list."""
    nw = 4 if mer127 else 2
    cs = [circle(K, n, i) for i, n in enumerate(sizes)]
    g = E.linear(K)
    singles = G.singles(K, lone, 5400) if lone else []
    seqs = [round_once(c, K) for c in cs] + ([g] if chain else []) + list(singles)
    n_kmers = sum(sizes) + (len(g) - K + 1 if chain else 0) + lone
    assert E.distinct_kmers(seqs, K) == n_kmers
    expect = [G.ring(c, K) for c in cs] + ([G.emitted(g, D, D, K)] if chain else []) + [G.emitted(s, D, D, K) for s in singles]
    results = []
    for flip in (False, True):
        what = "rings %s %s%s" % ("+".join(str(n) for n in sizes), flavour_id((K, mer127)), " rc reads" if flip else "")
        got, totals = check_records(E.records_of(*whole_reads(seqs, K, flip), nw), K, mer127, device, expect, what, twin)
        assert totals[5] == len(sizes) and totals[4] == n_kmers, what
        results.append((sorted(got), totals))
    assert results[0] == results[1], "the reads reverse complemented give another result"


# ---- 6. one long chain ----
def fast_records(seq, K, copies):
    """Export records (63-mer build, K <= 31) of one sequence read `copies` times, worked out over all its k-mers at once: what
    records_of(count([([seq], copies)], K), 2) gives, which check_fast_records holds it to on a short sequence."""
    assert K <= 31 and copies >= 2
    s = np.asarray(seq, dtype=np.uint64)
    n = len(s) - K + 1
    fwd, back = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i in range(K):
        fwd = (fwd << np.uint64(2)) | s[i:i + n]
        back = back | ((s[i:i + n] ^ np.uint64(2)) << np.uint64(2 * i))
    as_is = fwd < back
    keys = np.where(as_is, fwd, back)
    assert np.unique(keys).size == n, "the k-mers are not distinct"
    prev = np.concatenate([[np.uint64(4)], s[:n - 1]])                           # (4: no neighbour)
    nxt = np.concatenate([s[K:], [np.uint64(4)]])
    left = np.where(as_is, prev, np.where(nxt < 4, nxt ^ np.uint64(2), np.uint64(4)))
    right = np.where(as_is, nxt, np.where(prev < 4, prev ^ np.uint64(2), np.uint64(4)))
    c = np.uint64(min(copies, 63))
    A = np.where(left < 4, c << (np.uint64(6) * (left & np.uint64(3))), np.uint64(0)) | (np.uint64(min(copies, 255)) << np.uint64(24))
    B = np.where(right < 4, c << (np.uint64(6) * (right & np.uint64(3))), np.uint64(0))
    order = np.argsort(keys)
    rec = np.zeros((n, 4), dtype=np.uint64)
    rec[:, 1] = keys[order]
    rec[:, 2] = (A | (B << np.uint64(32)))[order]
    rec[:, 3] = np.arange(n, dtype=np.uint64)
    return rec


def check_fast_records():
    s = alone(LONG_K, 257)
    assert (fast_records(s, LONG_K, 2) == E.records_of(*E.count([([s], 2)], LONG_K), 2)).all()


@functools.lru_cache(maxsize=None)
def long_chain():
    """(the sequence, its records, the unitig the construction dictates): generated once with a fixed seed and never written to."""
    s = np.random.default_rng(LONG_SEED).integers(0, 4, size=LONG + LONG_K - 1, dtype=np.uint8)
    return s, fast_records(s, LONG_K, 2), G.emitted(s, D, D, LONG_K)


def check_long_chain(device):
    """One chain of 65 537 31-mers against the closed form: the text, both reasons, the coverage sum, the totals, the layout."""
    K = LONG_K
    s, records, expect = long_chain()
    w = Compactor(records, K, False, device, model=object())
    try:
        got, totals = w.run(1, 1, MAXK, "long chain")
    finally:
        w.close()
    assert got == [expect + (2 * LONG,)]
    assert totals == [1, (LONG + K - 1 + 31) // 32 + 3, LONG + K - 1, LONG, LONG, 0, 0, 0]


# ---- 7. / 8. / 5. kunitig_cases' checks through the ranked call ----
def check_fuzz(K, mer127, device):
    with ranked():
        for name in ("n513", "colliding"):
            G.check_fuzz(name, K, mer127, device, [(1, 1), (100, 50), (200, 20)])


def check_noisy(K, mer127, device, twin=None):
    with ranked():
        G.check_noisy(K, mer127, device, twin)


def check_isolated(device, twin=None):
    with ranked():
        G.check_isolated(device, twin)


def check_capacities(K, mer127, device):
    with ranked():
        G.check_capacities(K, mer127, device)


# ---- 9. the frame ----
def check_refusals(K, mer127, device, cut_devices):
    """Every refusal that an index of test size can meet, with nothing written: the thresholds' ranges, null totals, a null index, an
    index cut over ranks; the api's ValueErrors.  (An index of more than 2^31 - 2 keys is refused too; none is built here.)"""
    nw = 4 if mer127 else 2
    records = E.records_of(*E.linear_counts(K, 3), nw)
    w = Compactor(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    try:
        outs = w.outputs(4, 64)
        call = lambda min_cov=1, min_arc=1, o=outs, ix=None: w.call(min_cov, min_arc, MAXK, 4, 64, *o, ix=ix)
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64)):
            assert call(**bad) == EINVAL and b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert call(o=outs[:4] + (None,)) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_unitigs_ranked(None, 1, 1, 0, 0, None, None, None, None, None, None) == EINVAL
        assert call(ix=cut) == ESTATE and b"cut over ranks" in L.pg_last_error()
        with pytest.raises(api.PgError):
            cut.unitigs(1, engine="rank")
        with pytest.raises(api.PgError):
            w.ix.unitigs(0, engine="rank")
        with pytest.raises(ValueError):
            w.ix.unitigs(1, engine="jump")
        with pytest.raises(ValueError):
            w.ix.unitigs(1, 1, 50, engine="rank")
        with pytest.raises(ValueError):
            api.unitig_seqs(w.ix, 1, 1, 50, engine="rank")
        assert all((w.down(a) == FILL).all() for a in outs)
        assert call() == 0 and int(w.down(outs[4])[0]) == 1
    finally:
        cut.close()
        w.close()


def check_api(K, mer127, device):
    """KmerIndex.unitigs(engine="rank") and api.unitig_seqs: the model's unitigs, the walking engine's with the same totals, a ring longer
    than a guard the walking engine is given, and the batch back through query_ragged: every k-mer present and solid."""
    nw = 4 if mer127 else 2
    P, SA, SB = E.forked(K)
    c = G.circular(K)
    records = E.records_of(*E.count([(E.tile(np.concatenate([P, SA]), K), 3), (E.tile(np.concatenate([P, SB]), K), 3), (E.tile(c, K, circular=True), 3)], K), nw)
    w = Compactor(records, K, mer127, device)
    try:
        min_cov = 2
        want, _ = U.unitigs(w.model, min_cov, 1)
        listed = lambda seqs, f: sorted((tuple(int(x) for x in s), int(l), int(r), int(cv))
                                        for s, l, r, cv in zip(seqs, f["left_code"], f["right_code"], f["coverage_sum"]))
        seqs, f, totals = api.unitig_seqs(w.ix, min_cov, engine="rank")
        assert listed(seqs, f) == sorted(want) and totals["unitigs"] == 4 and totals["cyclic"] == 1 and totals["overflow"] == 0 and totals["cut"] == 0
        w_seqs, w_f, w_totals = api.unitig_seqs(w.ix, min_cov, engine="walk")
        assert listed(w_seqs, w_f) == listed(seqs, f) and w_totals == totals
        _, _, short = api.unitig_seqs(w.ix, min_cov, 1, len(c) - 1)              # (the walking engine under a guard drops the ring)
        assert short["cyclic"] == 0 and short["covered"] < short["solid"] == totals["covered"]
        u = w.ix.unitigs(min_cov, engine="rank")
        n, n_kmers = int(u.totals[0]), int(u.totals[3])
        assert n_kmers == int(u.totals[4]) == len(U.solid_keys(w.model, min_cov))
        cnt = w.down(w.ix.query_ragged(u.packed, u.word_off, u.kmer_base, n, n_kmers))
        assert cnt.size == n_kmers and (((cnt >> np.uint64(24)) & np.uint64(0xff)) >= min_cov).all()
    finally:
        w.close()


def check_shared_scratch(device):
    """The walking engine, the ranked one, a round of tip clipping and the ranked one again on one index, whose scratch they share: each
    result is the model's over the records as they stand, and the two engines agree before and after the edit."""
    import kindex_model as M
    K = 31
    P, SA, SB = E.forked(K)
    main = np.concatenate([P, SA])
    tip = np.concatenate([P, SB])[len(P) - K - 3:len(P) + 6]                     # (a branch of six k-mers that ends: a tip beside the main path)
    records = E.records_of(*E.count([(E.tile(main, K), 5), ([tip], 1)], K), 2)
    ix = api.KmerIndex.from_records(records, K, False, device)
    try:
        listed = lambda out: (sorted((tuple(int(x) for x in s), int(l), int(r), int(c)) for s, l, r, c in
                                     zip(out[0], out[1]["left_code"], out[1]["right_code"], out[1]["coverage_sum"])), out[2])
        model = M.Model.from_records(records, K, 2)
        walked = listed(api.unitig_seqs(ix, 1, 1, engine="walk"))
        both = listed(api.unitig_seqs(ix, 1, 1, engine="rank"))
        assert walked == both and both[0] == sorted(U.unitigs(model, 1, 1)[0]) and both[1]["unitigs"] == 3
        rounds = ix.clip_tips(1, 1)
        assert int(rounds[0][0]) == 1, "the tip is clipped in the first round"
        after = listed(api.unitig_seqs(ix, 1, 1, engine="rank"))
        assert after == listed(api.unitig_seqs(ix, 1, 1, engine="walk"))
        assert after[1]["unitigs"] == 1 and after[0][0][:3] == G.emitted(main, D, D, K)
    finally:
        ix.close()
