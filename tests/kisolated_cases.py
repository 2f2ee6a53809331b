"""The cases of the dropping of short isolated unitigs, shared by tests/test_kisolated_host.py (the host twin) and
tests/test_gpu_kisolated.py (the kernels): designed read sets turned into records with the builders of tests/kwalk_cases.py and
tests/ktip_cases.py, edited a round at a time through pg_kindex_drop_isolated, and after every round compared exactly with the model
(tests/kisolated_model.py) and with what the construction dictates: the four totals, and the word of EVERY key of the original set read
back with query_ragged -- removed keys read 0, every other word is bit-identical.  twin: a second index of the same records (the host
twin beside a device index) is edited in step, and the two must agree word for word.  All comparisons are of integers and exact.

Cleaner is karc_cases.Editor with a round of the islands and with KmerIndex.simplify's order of calls for any of the five names, one
ABI round at a time."""
import functools

import numpy as np
import pytest

import karc_cases as AC
import karc_model as A
import kbubble_cases as BC
import kbubble_model as B
import kbulge_model as S
import kindex_cases as KC
import kindex_model as M
import kisolated_model as I
import ktip_cases as TC
import ktip_model as T
import kunitig_cases as G
import kunitig_model as U
import kwalk_cases as E
from kbubble_cases import plain
from ktip_cases import branch_read, node
from kwalk_cases import count, random_genome, rc, records_of, tile
from soapdenovo2_amd import api

FLAVOURS = TC.FLAVOURS
flavour_id = KC.flavour_id
FILL = E.FILL
EINVAL, ESTATE = E.EINVAL, E.ESTATE
D, BO, WN, BI = T.DEAD_END, T.BRANCH_OUT, T.WEAK_NEXT, T.BRANCH_IN
MAX_LEN = 20                                  # the designs' max_len where they do not state another: below every main path's length
CLEAN_OPS = ("arcs", "tips", "bubbles", "bulges", "isolated")


class Cleaner(AC.Editor):
    """karc_cases.Editor with a round of the islands beside the rounds of the four other operators."""

    def isolated_call(self, min_cov, min_arc, max_len, max_cov, totals, ix=None):
        ix = ix or self.ix
        return api.lib().pg_kindex_drop_isolated(ix.h, min_cov, min_arc, max_len, max_cov, ix._ptr(totals), ix._stream())

    def isolated(self, min_cov, min_arc, max_len=MAX_LEN, max_cov=255, what=""):
        """One round of the islands, as Clipper._round returns it (no counter is ever cleared)."""
        return self._round(self.isolated_call, lambda model, *args: I.isolated_round(model, *args) + ([],), (min_cov, min_arc, max_len, max_cov), what)

    def isolated_settle(self, min_cov, min_arc, max_len=MAX_LEN, max_cov=255, what=""):
        return self._settle(lambda w: self.isolated(min_cov, min_arc, max_len, max_cov, w), what)

    def clean_by_rounds(self, ops, min_cov, min_arc, max_tip, max_len, max_diff=0, max_cov=255, what=""):
        """KmerIndex.simplify's order of calls for `ops` made one ABI round at a time, each compared: the list of (name, totals)."""
        one = {"arcs": lambda tag: self.drop(min_cov, min_arc, tag), "tips": lambda tag: self.round(min_cov, min_arc, max_tip, tag),
               "bubbles": lambda tag: self.pop(min_cov, min_arc, max_len, max_diff, tag), "bulges": lambda tag: self.bulge(min_cov, min_arc, max_len, max_diff, tag),
               "isolated": lambda tag: self.isolated(min_cov, min_arc, max_len, max_cov, tag)}
        out = []
        while True:
            removed = 0
            for name in ops:
                while True:
                    t = one[name]("%s call %d (%s)" % (what, len(out) + 1, name))[0]
                    out.append((name, t))
                    removed += t[0]
                    assert len(out) <= 64
                    if not t[0]:
                        break
            if not removed:
                return out


def model_simplify(model, ops, min_cov, min_arc, max_tip, max_len, max_diff=0, max_cov=255, max_rounds=64):
    """KmerIndex.simplify(ops=ops) as its documentation states it, on the model, for any of the five names."""
    one = {"arcs": lambda: A.drop_round(model, min_cov, min_arc)[0], "tips": lambda: T.clip_round(model, min_cov, min_arc, max_tip)[0],
           "bubbles": lambda: B.pop_round(model, min_cov, min_arc, max_len, max_diff)[0], "bulges": lambda: S.bulge_round(model, min_cov, min_arc, max_len, max_diff)[0],
           "isolated": lambda: I.isolated_round(model, min_cov, min_arc, max_len, max_cov)[0]}
    out = []
    while len(out) < max_rounds:
        removed = 0
        for name in ops:
            while len(out) < max_rounds:
                t = one[name]()
                out.append((name, t))
                removed += t[0]
                if not t[0]:
                    break
        if not removed:
            break
    return out


def keys_of(seq, K):
    return set(M.canonical_kmers(seq, K))


@functools.lru_cache(maxsize=None)
def main_path(K):
    """The main path of the designs: K + 60 bases, 61 k-mers -- more than MAX_LEN + 1, so never an island there."""
    return random_genome(8100 + K, K + 60)


def chain(K, n, seed):
    """A random sequence of n k-mers that shares none with the main path."""
    s = random_genome(seed, n + K - 1)
    assert E.distinct_kmers([main_path(K), s], K) == 61 + n
    return s


@functools.lru_cache(maxsize=None)
def chain_decided_from(K, n, fwd):
    """A chain of n k-mers whose deciding start -- the not greater of its first k-mer and the reverse complement of its last -- is
    (fwd) or is not its slot's canonical key."""
    for seed in range(8200 + K + 100 * n, 8300 + K + 100 * n):
        s = chain(K, n, seed)
        first, back = node(s[:K]), node(rc(s[-K:]))
        start = first if first[0] <= back[0] else back
        if T.is_fwd(start) == fwd:
            return s
    raise AssertionError("no seed gives that start")


# ---- the designs ----
def check_lengths(K, mer127, device, twin=None):
    """One island of n k-mers, read once, beside a 5-copy main path, n = 1 (a read of exactly K bases: the two starts are the two
    orientations of one slot), 2, max_len and max_len + 1 -- each untouched at n - 1, so the last is kept at max_len --, its deciding
    start canonical and not, the reads as they are and all reverse complemented.  Totals [1, n, solid, 0]; then one unitig, the path."""
    nw = 4 if mer127 else 2
    g = main_path(K)
    n_path = len(g) - K + 1
    for n in (1, 2, MAX_LEN, MAX_LEN + 1):
        for fwd in ((True,) if n == 1 else (True, False)):                      # (of one k-mer's two orientations the canonical one decides)
            s = chain_decided_from(K, n, fwd)
            what = "island of %d, start %s, %s" % (n, "canonical" if fwd else "not canonical", flavour_id((K, mer127)))
            main = tile(g, K)
            records = records_of(*count([(main, 5), ([s], 1)], K), nw)
            swapped = records_of(*count([([rc(r) for r in main], 5), ([rc(s)], 1)], K), nw)
            for recs in (records, swapped):
                c = Cleaner(recs, K, mer127, device, twin)
                try:
                    solid = n_path + n
                    assert len(c.unitigs(1, 1)[0]) == 2, what
                    if n > 1:
                        assert c.isolated(1, 1, n - 1, 255, what)[0] == [0, 0, solid, 0], what
                    totals, removed, _ = c.isolated(1, 1, n, 255, what)
                    assert totals == [1, n, solid, 0] and removed == keys_of(s, K), what
                    got, t = c.unitigs(1, 1)
                    assert got == [G.emitted(g, D, D, K)] and t["covered"] == t["solid"] == n_path, what
                    assert c.isolated(1, 1, n, 255, what)[0] == [0, 0, n_path, 0], what
                finally:
                    c.close()


def check_sides(K, mer127, device, twin=None):
    """A chain of 5 k-mers read twice whose sides are DEAD_END / DEAD_END, WEAK_NEXT / DEAD_END and WEAK_NEXT / WEAK_NEXT at min_cov 2:
    a longer read, once, continues it into k-mers below min_cov on one side or on both.  All three are removed, in one round of one
    index, and the weak k-mers' words are untouched."""
    nw = 4 if mer127 else 2
    what = "sides " + flavour_id((K, mer127))
    n, ext = 5, 4
    whole = [random_genome(8400 + K + i, n + K - 1 + 2 * ext) for i in range(3)]
    core = [w[ext:ext + n + K - 1] for w in whole]
    longer = [None, whole[1][ext:], whole[2]]
    assert E.distinct_kmers([main_path(K)] + whole, K) == 61 + 3 * (n + 2 * ext)
    groups = [(tile(main_path(K), K), 5), (core, 2), ([r for r in longer if r is not None], 1)]
    c = Cleaner(records_of(*count(groups, K), nw), K, mer127, device, twin)
    try:
        want = []
        for s, l in zip(core, longer):
            first, last = node(rc(s[:K])), node(s[-K:])
            want.append(tuple(sorted((T.side(c.model.cnt, K, first, 2, 1)[0], T.side(c.model.cnt, K, last, 2, 1)[0]))))
        assert want == [(D, D), (D, WN), (WN, WN)], what
        weak = set().union(*(keys_of(r, K) for r in longer if r is not None)) - set().union(*(keys_of(s, K) for s in core))
        assert len(weak) == 3 * ext and all(M.coverage(c.model.cnt[k]) == 1 for k in weak), what
        before = {k: c.model.cnt[k] for k in weak}
        solid = 61 + 3 * n
        totals, removed, _ = c.isolated(2, 1, MAX_LEN, 255, what)
        assert totals == [3, 3 * n, solid, 0] and removed == set().union(*(keys_of(s, K) for s in core)), what
        assert all(c.model.cnt[k] == before[k] != 0 for k in weak), what
        assert c.isolated(2, 1, MAX_LEN, 255, what)[0] == [0, 0, 61, 0], what
        assert c.unitigs(2, 1)[0] == [G.emitted(main_path(K), D, D, K)], what
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def small_hairpin(K):
    """kunitig_cases.hairpin's construction, short: A of K + 8 bases followed by its own reverse complement."""
    a = random_genome(8500 + K, K + 8)
    h = np.concatenate([a, rc(a)])
    assert E.distinct_kmers([h], K) == len(a) - (K - 1) // 2
    return h


def check_not_islands(K, mer127, device, twin=None):
    """What is no island, in one index with one that is, at max_len 64: a tip of 5 k-mers (DEAD_END / BRANCH_IN), the start of the graph
    before a fork (DEAD_END / BRANCH_OUT) and the fork's branch, a ring, a chain from a dead end into a hairpin and a chain of 65
    k-mers.  Only the island, 13 k-mers, goes; kept stays 0: the others are no candidates.  Nothing at all goes at max_len 12."""
    nw = 4 if mer127 else 2
    what = "not islands " + flavour_id((K, mer127))
    max_len = 64
    P, SA, SB, _ = TC.fork_with_junction(K, True)
    short = P[-(K + 5):]
    fork, tip = np.concatenate([short, SA]), branch_read(short, SB, 5, K)
    island, ring, h, long = random_genome(5400 + K, K + 12), G.circular(K), small_hairpin(K), random_genome(8600 + K, K + max_len)
    parts = [fork, tip, island, np.concatenate([ring, ring[:K - 1]]), h, long]
    n = 6 + (K + 40) + 5 + 13 + len(ring) + E.distinct_kmers([h], K) + max_len + 1
    assert E.distinct_kmers(parts, K) == n
    groups = [(tile(fork, K), 3), ([tip], 1), (tile(island, K), 3), (tile(ring, K, circular=True), 2), (tile(h, K), 2), (tile(long, K), 3)]
    c = Cleaner(records_of(*count(groups, K), nw), K, mer127, device, twin)
    try:
        reasons = AC.reasons_of(c, 1, 1)
        assert reasons == sorted([(D, BO), (D, BI), (D, BI), (D, D), (U.CYCLE, U.CYCLE), (D, U.HAIRPIN), (D, D)]), what
        assert c.isolated(1, 1, 12, 255, what)[0] == [0, 0, n, 0], what
        totals, removed, _ = c.isolated(1, 1, max_len, 255, what)
        assert totals == [1, 13, n, 0] and removed == keys_of(island, K), what
        assert AC.reasons_of(c, 1, 1) == sorted([(D, BO), (D, BI), (D, BI), (U.CYCLE, U.CYCLE), (D, U.HAIRPIN), (D, D)]), what
        assert c.isolated(1, 1, max_len, 255, what)[0] == [0, 0, n - 13, 0], what
    finally:
        c.close()


def check_coverage(K, mer127, device, twin=None):
    """Two islands of 4 k-mers, each read three times, the second with one more read of exactly K bases over one of its k-mers: coverage
    sums 12 and 13.  At max_cov 3 the first goes (12 == 3 * 4) and the second is kept and counted (13 == 3 * 4 + 1); at max_cov 4 it
    goes.  Then an island of 3 k-mers read 300 times, coverage 255 each: kept at max_cov 254, removed at 255."""
    nw = 4 if mer127 else 2
    what = "coverage bound " + flavour_id((K, mer127))
    n = 4
    a, b = chain(K, n, 8700 + K), chain(K, n, 8750 + K)
    assert E.distinct_kmers([a, b], K) == 2 * n
    c = Cleaner(records_of(*count([(tile(main_path(K), K), 5), ([a, b], 3), ([b[1:K + 1]], 1)], K), nw), K, mer127, device, twin)
    try:
        cov = lambda s: sum(M.coverage(c.model.cnt[k]) for k in keys_of(s, K))
        assert (cov(a), cov(b)) == (3 * n, 3 * n + 1), what
        solid = 61 + 2 * n
        assert c.isolated(1, 1, MAX_LEN, 2, what)[0] == [0, 0, solid, 2], what
        totals, removed, _ = c.isolated(1, 1, MAX_LEN, 3, what)
        assert totals == [1, n, solid, 1] and removed == keys_of(a, K), what
        assert c.isolated(1, 1, MAX_LEN, 3, what)[0] == [0, 0, solid - n, 1], what
        totals, removed, _ = c.isolated(1, 1, MAX_LEN, 4, what)
        assert totals == [1, n, solid - n, 0] and removed == keys_of(b, K), what
    finally:
        c.close()
    what = "saturated coverage " + flavour_id((K, mer127))
    s = chain(K, 3, 8800 + K)
    c = Cleaner(records_of(*count([(tile(main_path(K), K), 5), ([s], 300)], K), nw), K, mer127, device, twin)
    try:
        assert all(M.coverage(c.model.cnt[k]) == 255 for k in keys_of(s, K)), what
        assert c.isolated(255, 63, MAX_LEN, 254, what)[0] == [0, 0, 3, 1], what
        totals, removed, _ = c.isolated(255, 63, MAX_LEN, 255, what)
        assert totals == [1, 3, 3, 0] and removed == keys_of(s, K), what
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def many_islands(K, mer127, n_islands):
    """(records, the sequences, k-mers in all, islands read three times, their k-mers): many_tips' pattern for islands -- island i has
    1 + i % MAX_LEN k-mers and is read once, every fifth three times."""
    rng = np.random.default_rng(8900 + K + n_islands)
    seqs = [rng.integers(0, 4, size=1 + i % MAX_LEN + K - 1, dtype=np.uint8) for i in range(n_islands)]
    total = sum(len(s) - K + 1 for s in seqs)
    assert E.distinct_kmers(seqs, K) == total
    deep = [s for i, s in enumerate(seqs) if i % 5 == 4]
    records = records_of(*count([([s for i, s in enumerate(seqs) if i % 5 != 4], 1), (deep, 3)], K), 4 if mer127 else 2)
    return records, tuple(seqs), total, len(deep), sum(len(s) - K + 1 for s in deep)


def check_many_islands(K, mer127, device, twin=None):
    """257 and 513 islands of mixed lengths 1 .. max_len and nothing else, in tables of more slots than a workgroup has lanes: both
    copies of every island are in the start list, which crosses wave and workgroup edges, and a wave sums its lanes' k-mers.  At
    max_cov 2 the islands read three times are kept, at 255 they go too; the next round reports solid 0."""
    for n in (257, 513):
        what = "%d islands %s" % (n, flavour_id((K, mer127)))
        records, seqs, total, n_deep, deep_kmers = many_islands(K, mer127, n)
        assert M.table_slots(len(records)) > 256
        c = Cleaner(records, K, mer127, device, twin, sources=seqs)
        try:
            assert c.isolated_settle(1, 1, MAX_LEN, 2, what) == [[n - n_deep, total - deep_kmers, total, n_deep], [0, 0, deep_kmers, n_deep]], what
            assert c.isolated_settle(1, 1, MAX_LEN, 255, what) == [[n_deep, deep_kmers, deep_kmers, 0], [0, 0, 0, 0]], what
            assert (c.words() == 0).all(), what
        finally:
            c.close()


def check_tombstone(K, mer127, device, twin=None):
    """kindex_cases' colliding keys, each alone in the graph with coverage 9 -- an island of one k-mer --, and in every group of keys
    with one home slot the middle one with coverage 2: at max_cov 2 it goes and its slot stays taken in the middle of the probe run.
    Afterwards every surviving key still answers its word and every removed key answers 0 (the round's comparison of every word)."""
    nw = 4 if mer127 else 2
    what = "tombstones " + flavour_id((K, mer127))
    _, keys = KC.table("colliding", K, mer127)
    word, groups = {k: 9 << 24 for k in keys}, {}
    for k in keys:
        groups.setdefault(M.home_slot(k, nw, len(keys)), []).append(k)
    middle = [g[len(g) // 2] for g in groups.values() if len(g) >= 3][:64]
    for k in middle:
        word[k] = 2 << 24
    assert len(middle) >= 8 and M.table_slots(len(keys)) == 8192
    records = np.zeros((len(keys), nw + 2), dtype=np.uint64)
    for i, k in enumerate(keys):                                                # (the colliding keys group by group: a serial build's runs are in that order)
        records[i, :nw] = M.words_of_key(k, nw)
        records[i, nw], records[i, nw + 1] = word[k], i
    c = Cleaner(records, K, mer127, device, twin)
    try:
        n = len(middle)
        totals, removed, _ = c.isolated(1, 1, MAX_LEN, 2, what)
        assert totals == [n, n, len(keys), len(keys) - n] and removed == set(middle), what
        assert c.isolated(1, 1, MAX_LEN, 2, what)[0] == [0, 0, len(keys) - n, len(keys) - n], what
    finally:
        c.close()


def check_edges(K, mer127, device, twin=None):
    """An empty index, through the ABI, drop_isolated and simplify with all five names; and an index of three islands only: the next
    round reports solid 0."""
    nw = 4 if mer127 else 2
    c = Cleaner(np.zeros((0, nw + 2), dtype=np.uint64), K, mer127, device, twin)
    try:
        assert c.isolated(1, 1, MAX_LEN, 255, "empty")[0] == [0, 0, 0, 0]
        assert [int(v) for r in c.ix.drop_isolated(1, 1) for v in r] == [0, 0, 0, 0]
        assert plain(c.ix.simplify(1, 1, ops=api.CLEAN_OPS)) == [(name, [0, 0, 0, 0]) for name in CLEAN_OPS]
    finally:
        c.close()
    what = "islands only " + flavour_id((K, mer127))
    seqs = [chain(K, n, 9000 + K + n) for n in (1, 7, MAX_LEN)]
    c = Cleaner(records_of(*count([(seqs, 2)], K), nw), K, mer127, device, twin)
    try:
        total = 1 + 7 + MAX_LEN
        assert c.isolated_settle(1, 1, MAX_LEN, 255, what) == [[3, total, total, 0], [0, 0, 0, 0]], what
        assert not c.unitigs(1, 1)[0], what
    finally:
        c.close()


def check_back_to_back(K, mer127, device, twin=None):
    """Two ABI calls back to back on one stream with no wait between them: the first removes, the second reports [0, 0, solid - kmers,
    kept]; then KmerIndex.drop_isolated, which stops by itself, isolated_fields and max_rounds."""
    what = "two calls back to back " + flavour_id((K, mer127))
    records, seqs, total, n_deep, deep_kmers = many_islands(K, mer127, 257)
    first = [257 - n_deep, total - deep_kmers, total, n_deep]
    c = Cleaner(records, K, mer127, device, sources=seqs)
    try:
        bufs = [c.totals(), c.totals()]
        for t in bufs:
            assert c.isolated_call(1, 1, MAX_LEN, 2, t) == 0
        assert [[int(v) for v in c.down(c.ix, t)] for t in bufs] == [first, [0, 0, total - first[1], n_deep]], what
        I.isolated_round(c.model, 1, 1, MAX_LEN, 2)
        assert (c.words() == c.want_words()).all(), what
    finally:
        c.close()
    c = Cleaner(records, K, mer127, device, sources=seqs)
    try:
        rounds = c.ix.drop_isolated(1, 1, MAX_LEN, 2)
        assert [[int(v) for v in r] for r in rounds] == [first, [0, 0, deep_kmers, n_deep]], what
        assert api.isolated_fields(rounds[0]) == dict(islands=first[0], kmers=first[1], solid=total, kept=n_deep), what
        fresh = api.KmerIndex.from_records(records, K, mer127, device)
        try:
            assert len(fresh.drop_isolated(1, 1, MAX_LEN, 2, max_rounds=1)) == 1
            assert (c.words(fresh) == c.words()).all(), what
            assert [int(r[0]) for r in fresh.drop_isolated(1, 1)] == [n_deep, 0], what       # (max_len = 2 K, max_cov = 255)
            assert (c.words(fresh) == 0).all(), what
        finally:
            fresh.close()
    finally:
        c.close()


def check_simplify(K, mer127, device, twin=None):
    """karc_cases' 2 kb genome with a repeat, read with 1 % substitutions, at 2 / 1 and 3 / 2 through simplify(ops=CLEAN_OPS) one ABI
    round at a time, each against the model; the calls are the five-name model_simplify's; at the end the model finds no island within
    max_len.  Then KmerIndex.simplify(ops=CLEAN_OPS) in one call, the default ops giving the calls they gave before, and a name that is
    no operator raising with the table untouched."""
    nw = 4 if mer127 else 2
    records = records_of(*count([(BC.noisy(K), 1)], K), nw)
    limit = 2 * K
    for min_cov, min_arc in ((2, 1), (3, 2)):
        what = "noisy %s at %d / %d" % (flavour_id((K, mer127)), min_cov, min_arc)
        c = Cleaner(records, K, mer127, device, twin)
        try:
            n_before = len(c.unitigs(min_cov, min_arc)[0])
            rounds = c.clean_by_rounds(CLEAN_OPS, min_cov, min_arc, limit, limit, 0, 255, what)
            assert rounds == model_simplify(M.Model.from_records(records, K, nw), CLEAN_OPS, min_cov, min_arc, limit, limit), what
            assert not I.islands(c.model.cnt, K, min_cov, min_arc, limit), what + ": an island is left"
            n_after = len(c.unitigs(min_cov, min_arc)[0])
            assert n_after <= n_before, what
            print("%s: %d -> %d unitigs, %s" % (what, n_before, n_after, rounds))
        finally:
            c.close()
    assert api.CLEAN_OPS == CLEAN_OPS and api.SIMPLIFY_OPS == AC.ALL_OPS
    c = Cleaner(records, K, mer127, device)
    try:
        assert plain(c.ix.simplify(2, 1, ops=api.CLEAN_OPS)) == model_simplify(c.model, CLEAN_OPS, 2, 1, limit, limit), "noisy: simplify's calls are not the model's"
        assert (c.words() == c.want_words()).all()
    finally:
        c.close()
    c = Cleaner(records, K, mer127, device)
    try:
        assert plain(c.ix.simplify(1, 1)) == BC.model_simplify(c.model, 1, 1, limit, limit), "noisy: the default ops no longer give the calls they gave"
        assert (c.words() == c.want_words()).all()
        for bad in (("tips", "islands"), ("isolated", "island")):
            with pytest.raises(ValueError):
                c.ix.simplify(1, 1, ops=bad)
            assert (c.words() == c.want_words()).all()
    finally:
        c.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with the pre-filled totals and every word of the table untouched: the ranges of the thresholds, max_len and
    max_cov at both ends, null totals, a null index, an index cut over ranks; then the bounds themselves are taken."""
    records, seqs, total, n_deep, deep_kmers = many_islands(K, mer127, 257)
    c = Cleaner(records, K, mer127, device, sources=seqs)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    try:
        before, totals = c.words(), c.totals()
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64), dict(max_len=0), dict(max_len=api.ISOLATED_MAX_BOUND + 1),
                    dict(max_cov=0), dict(max_cov=256)):
            args = dict(dict(min_cov=1, min_arc=1, max_len=MAX_LEN, max_cov=255), **bad)
            assert c.isolated_call(args["min_cov"], args["min_arc"], args["max_len"], args["max_cov"], totals) == EINVAL, bad
            assert b"min_cov is 1 to 255" in L.pg_last_error() and b"max_cov 1 to 255" in L.pg_last_error(), bad
        assert c.isolated_call(1, 1, MAX_LEN, 255, None) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_drop_isolated(None, 1, 1, MAX_LEN, 255, None, None) == EINVAL and b"null index" in L.pg_last_error()
        assert L.pg_kindex_drop_isolated(cut.h, 1, 1, MAX_LEN, 255, c.ix._ptr(totals), c.ix._stream()) == ESTATE
        assert b"drop the isolated unitigs of an index in one table" in L.pg_last_error()
        assert L.pg_kindex_drop_isolated(cut.h, 0, 1, MAX_LEN, 255, None, None) == ESTATE                # (the order: the cut before the ranges)
        assert c.isolated_call(0, 1, MAX_LEN, 255, None) == EINVAL and b"min_cov is 1 to 255" in L.pg_last_error()   # (the ranges before the totals)
        for call in (lambda: cut.drop_isolated(1, 1), lambda: cut.simplify(1, 1, ops=api.CLEAN_OPS), lambda: c.ix.drop_isolated(0, 1),
                     lambda: c.ix.drop_isolated(1, 1, max_cov=256), lambda: c.ix.drop_isolated(1, 1, max_len=0)):
            with pytest.raises(api.PgError):
                call()
        assert (c.down(c.ix, totals) == FILL).all() and (c.words() == before).all()
        assert (c.words(cut) == before).all()
        # the bounds themselves are taken: nothing is solid at min_cov 255, and at 1 / 1 every island goes
        assert c.isolated_call(255, 63, api.ISOLATED_MAX_BOUND, 255, totals) == 0 and [int(v) for v in c.down(c.ix, totals)] == [0, 0, 0, 0]
        assert c.isolated_call(1, 1, api.ISOLATED_MAX_BOUND, 255, totals) == 0 and [int(v) for v in c.down(c.ix, totals)] == [257, total, total, 0]
    finally:
        cut.close()
        c.close()


def cleaned(min_cov, min_arc, max_cov=255):
    """KmerCounter counts the simulated reads (a circular genome of 3 000 bases, 900 reads of 100 bases with substitutions, K = 31) ->
    finalize -> index() -> simplify(ops=CLEAN_OPS, max_cov=max_cov) -> unitigs(): (the calls, the unitigs sorted, their totals, the
    model after the same calls over the counter's own records, the model's calls, the unitig count after simplify(ops=SIMPLIFY_OPS) on
    a second index)."""
    import torch
    import kcorrect_cases as C
    reads, _ = C.simulated()
    K, n, L = C.SIM_K, reads.shape[0], reads.shape[1]
    packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    ix = kc.index()
    records = kc.export()
    kc.close()
    model = M.Model.from_records(records, K, 2)
    four = api.KmerIndex.from_records(records, K, False, 0)
    four.simplify(min_cov, min_arc, ops=api.SIMPLIFY_OPS)
    before = int(four.unitigs(min_cov, min_arc).totals[0])
    four.close()
    calls = plain(ix.simplify(min_cov, min_arc, ops=api.CLEAN_OPS, max_cov=max_cov))
    seqs, f, totals = api.unitig_seqs(ix, min_cov, min_arc)
    ix.close()
    want = model_simplify(model, CLEAN_OPS, min_cov, min_arc, 2 * K, 2 * K, 0, max_cov)
    got = sorted((tuple(int(x) for x in s), int(l), int(r), int(c)) for s, l, r, c in zip(seqs, f["left_code"], f["right_code"], f["coverage_sum"]))
    return calls, got, totals, model, want, before


DESIGNS = [check_lengths, check_sides, check_not_islands, check_coverage, check_many_islands, check_tombstone, check_edges, check_back_to_back,
           check_simplify]
