"""Tip clipping's cases, shared by tests/test_ktip_host.py (the host twin) and tests/test_gpu_ktip.py (the kernels): designed read sets
turned into records with the builders of tests/kwalk_cases.py, clipped a round at a time through pg_kindex_clip_tips, and after every
round compared exactly with the model (tests/ktip_model.py) and with what the construction dictates: the four totals, and the word of
EVERY key of the original set read back with query_ragged -- removed keys read 0, a junction's word differs in exactly the counters the
round cleared, every other word is bit-identical.  twin: a second index of the same records (the host twin beside a device index)
is clipped in step, and the two must agree word for word -- a round's result is a function of the index alone.  All comparisons are
of integers and exact."""
import functools

import numpy as np
import pytest

import kindex_cases as KC
import kindex_model as M
import ktip_model as T
import kunitig_cases as G
import kunitig_model as U
import kwalk_cases as E
import kwalk_model as W
from kwalk_cases import codes, count, random_genome, rc, records_of, tile
from soapdenovo2_amd import api

FLAVOURS = [(31, False), (65, True)]          # both NW; 31 is the k of the measurements
flavour_id = KC.flavour_id
FILL = E.FILL
EINVAL, ESTATE = E.EINVAL, E.ESTATE
MAX_TIP = 20                                  # the designs' max_tip where they do not state another: below every main path's length
D, BO, WN, BI = T.DEAD_END, T.BRANCH_OUT, T.WEAK_NEXT, T.BRANCH_IN


def node(seq):
    """A k-mer of base codes as the model's oriented k-mer."""
    return W.value(seq), W.value(W.revcomp(list(seq)))


def canon(seq):
    return min(node(seq))


class Clipper:
    """An index under test with its model and, maybe, a twin index: device = -1 the host twin over numpy, else the device build over
    torch tensors.  A round goes straight to pg_kindex_clip_tips with a totals buffer pre-filled with FILL."""

    def __init__(self, records, K, mer127, device, twin=None, sources=()):
        self.K, self.mer127, self.device = K, mer127, device
        self.nw = 4 if mer127 else 2
        self.model = M.Model.from_records(records, K, self.nw)
        self.keys = sorted(set(self.model.cnt) | self.model.deleted)            # every key of the original set
        text = {}                                   # (sources: sequences that hold the records' k-mers, so that a large set's batch
        for s in sources:                           # is cut from them and not unpacked key by key)
            for j, k in enumerate(M.canonical_kmers(s, K)):
                text.setdefault(k, s[j:j + K])
        self.batch = api.pack_seqs_ragged([text[k] if k in text else E.codes_of_key(k, K) for k in self.keys], K)
        self.ix = api.KmerIndex.from_records(records, K, mer127, device)
        self.twin = api.KmerIndex.from_records(records, K, mer127, twin) if twin is not None else None

    def close(self):
        self.ix.close()
        if self.twin is not None:
            self.twin.close()

    @staticmethod
    def up(ix, a):
        if ix.device < 0:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64)).to("cuda:%d" % ix.device)

    @staticmethod
    def down(ix, a):
        return a if ix.device < 0 else a.cpu().numpy().view(np.uint64)

    def words(self, ix=None):
        """The word of every key of the original set, as the index answers now."""
        ix, n = ix or self.ix, len(self.keys)
        if not n:
            return np.zeros(0, dtype=np.uint64)
        words, off, base = (self.up(ix, a) for a in self.batch)
        return self.down(ix, ix.query_ragged(words, off, base, n, n)).copy()

    def want_words(self):
        return np.array([self.model.cnt.get(k, 0) for k in self.keys], dtype=np.uint64)

    def totals(self, ix=None):
        return self.up(ix or self.ix, np.full(4, FILL, dtype=np.uint64))

    def call(self, min_cov, min_arc, max_tip, totals, ix=None):
        ix = ix or self.ix
        return api.lib().pg_kindex_clip_tips(ix.h, min_cov, min_arc, max_tip, ix._ptr(totals), ix._stream())

    def compare(self, before, removed, cleared, what):
        """The index against the model's dict after a round, and the same said out over the words before it."""
        after = self.words()
        assert (after == self.want_words()).all(), what + ": the words differ from the model's"
        masks = {}
        for key, half, idx in cleared:
            masks[key] = masks.get(key, 0) | 63 << (32 * half + 6 * idx)
        assert not set(masks) & removed
        for k, b, a in zip(self.keys, before.tolist(), after.tolist()):
            if k in removed:
                assert a == 0 and b != 0, what + ": a removed key does not read 0"
            elif k in masks:
                assert a == b & ~masks[k] and a != b, what + ": a junction's word"
            else:
                assert a == b, what + ": a word nobody clipped changed"
        if self.twin is not None:
            assert (self.words(self.twin) == after).all(), what + ": the device differs from the host twin"

    def _round(self, call, model_round, args, what):
        """One round of an operator -- call(*args, totals, ix=None) its ABI entry, model_round(model, *args) its model --: (totals,
        removed keys, cleared counters as (junction key, half, counter)) after every comparison."""
        before = self.words()
        assert (before == self.want_words()).all(), what
        totals = self.totals()
        assert call(*args, totals) == 0, api.lib().pg_last_error()
        got = [int(v) for v in self.down(self.ix, totals)]
        want, removed, cleared = model_round(self.model, *args)
        assert got == want, "%s: totals %s, the model's %s" % (what, got, want)
        if self.twin is not None:
            t = self.totals(self.twin)
            assert call(*args, t, self.twin) == 0, api.lib().pg_last_error()
            assert [int(v) for v in self.down(self.twin, t)] == got, what + ": the device's totals differ from the host twin's"
        self.compare(before, removed, cleared, what)
        return got, removed, cleared

    @staticmethod
    def _settle(one_round, what):
        """Rounds to the fixed point -- one_round(what) makes one --: the list of their totals, the empty one included."""
        out = []
        while not out or out[-1][0]:
            out.append(one_round("%s round %d" % (what, len(out) + 1))[0])
            assert len(out) <= 64
        return out

    def round(self, min_cov, min_arc, max_tip=MAX_TIP, what=""):
        """One round of tips, as _round returns it."""
        return self._round(self.call, T.clip_round, (min_cov, min_arc, max_tip), what)

    def settle(self, min_cov, min_arc, max_tip=MAX_TIP, what=""):
        return self._settle(lambda w: self.round(min_cov, min_arc, max_tip, w), what)

    def unitigs(self, min_cov, min_arc):
        """(sorted (text, left, right), totals as a dict) of the index as it stands."""
        seqs, f, totals = api.unitig_seqs(self.ix, min_cov, min_arc)
        return sorted((tuple(int(x) for x in s), int(l), int(r)) for s, l, r in zip(seqs, f["left_code"], f["right_code"])), totals


# ---- the genomes ----
def fork(K, seed):
    """(prefix, suffix A, suffix B, suffix C) of K + 40 bases each, the suffixes beginning with three different bases: prefix + A,
    prefix + B and prefix + C share the prefix's k-mers and no other."""
    g = random_genome(seed, 4 * (K + 40))
    P, SA, SB, SC = (g[i * (K + 40):(i + 1) * (K + 40)].copy() for i in range(4))
    SB[0], SC[0] = (int(SA[0]) + 1) & 3, (int(SA[0]) + 2) & 3
    n = len(P) - K + 1
    assert E.distinct_kmers([np.concatenate([P, S]) for S in (SA, SB, SC)], K) == n + 3 * (K + 40)
    return P, SA, SB, SC


@functools.lru_cache(maxsize=None)
def fork_with_junction(K, fwd):
    """A fork whose junction as a tip's walk reaches it -- the reverse complement of the prefix's last k-mer -- is its canonical form
    (fwd) or is not."""
    for seed in range(5100 + K, 5200 + K):
        f = fork(K, seed)
        if T.is_fwd(node(rc(f[0][-K:]))) == fwd:
            return f
    raise AssertionError("no seed gives that junction")


def branch_read(P, S, n, K):
    """The read that carries the first n k-mers of the branch S off the path P (four k-mers of P before them)."""
    g, nP = np.concatenate([P, S]), len(P)
    return g[nP - K - 3:nP + n]


def branch_keys(P, S, n, K):
    g, nP = np.concatenate([P, S]), len(P)
    return [canon(g[j:j + K]) for j in range(nP - K + 1, nP - K + 1 + n)]


def out_counter(model, x, b):
    return T.out_counters(model.cnt[T.key_of(x)], T.is_fwd(x))[b]


# ---- the designs ----
def check_branch(K, mer127, device, twin=None):
    """A 5-read path with a 1-read branch of n k-mers leaving it, n = 1 and 7, the junction met as its canonical form and as its reverse
    complement: untouched at max_tip = n - 1, clipped at n; then one unitig, the path; the reads reverse complemented; and the clipped
    index beside one built without the tip's records."""
    nw = 4 if mer127 else 2
    for fwd in (True, False):
        P, SA, SB, _ = fork_with_junction(K, fwd)
        g1, p = np.concatenate([P, SA]), node(P[-K:])
        for n in (1, 7):
            what = "branch of %d, junction %s, %s" % (n, "canonical" if fwd else "not canonical", flavour_id((K, mer127)))
            main, minor = tile(g1, K), branch_read(P, SB, n, K)
            records = records_of(*count([(main, 5), ([minor], 1)], K), nw)
            swapped = records_of(*count([([rc(r) for r in main], 5), ([rc(minor)], 1)], K), nw)
            tips, n_path = set(branch_keys(P, SB, n, K)), len(g1) - K + 1
            for recs in (records, swapped):
                c = Clipper(recs, K, mer127, device, twin)
                try:
                    assert out_counter(c.model, p, int(SB[0])) == 1 and out_counter(c.model, p, int(SA[0])) >= 5
                    solid = n_path + n
                    if n > 1:
                        assert c.round(1, 1, n - 1, what)[0] == [0, 0, solid, 0]
                    totals, removed, cleared = c.round(1, 1, n, what)
                    assert totals == [1, n, solid, 0] and removed == tips
                    assert cleared == [(T.key_of(p), 0 if fwd else 1, int(SB[0]) ^ 2 if fwd else int(SB[0]))], what
                    got, t = c.unitigs(1, 1)
                    assert got == [G.emitted(g1, D, D, K)] and t["covered"] == t["solid"] == n_path, what
                    assert c.round(1, 1, n, what)[0] == [0, 0, n_path, 0]
                finally:
                    c.close()
            if n == 7 and fwd:
                check_as_if_never_there(records, tips, T.key_of(p), g1, K, mer127, device, what)


def check_as_if_never_there(records, tips, junction, g1, K, mer127, device, what):
    """After the clip the index answers as one built without the tip's records: every word but the junction's, where that index keeps
    the arc to the k-mer it never had; the walks from the path's ends at min_arc 2 -- and at min_arc 1 only the clipped index walks
    through, which is what the cleared counter is for."""
    nw = 4 if mer127 else 2
    c = Clipper(records, K, mer127, device)
    without = api.KmerIndex.from_records(records[[M.key_of_record(r, nw) not in tips for r in records]], K, mer127, device)
    try:
        assert c.round(1, 1, 7, what)[0][:2] == [1, 7]
        clipped, other = c.words(), c.words(without)
        for k, a, b in zip(c.keys, clipped.tolist(), other.tolist()):
            if k == junction:
                x = a ^ b
                assert x and a & x == 0 and x in [1 << s for s in (0, 6, 12, 18, 32, 38, 44, 50)], what + ": the junction's one counter, which was 1"
            else:
                assert a == b and (a == 0) == (k in tips), what
        ends = [g1[:K], g1[-K:]]
        for ix in (c.ix, without):
            seqs, f = api.extend_seqs(ends, ix, 1, 2)
            assert [list(s) for s in seqs] == [list(g1), list(g1)] and f["reason"] == ["dead_end"] * 4, what
        seqs, _ = api.extend_seqs(ends, c.ix, 1, 1)
        assert [list(s) for s in seqs] == [list(g1), list(g1)], what
        seqs, f = api.extend_seqs(ends[:1], without, 1, 1)
        assert f["reason"][0] == "branch_out" and len(seqs[0]) < len(g1), what
    finally:
        without.close()
        c.close()


def check_weak_next(K, mer127, device, twin=None):
    """A tip whose free side is WEAK_NEXT: its far k-mers below min_cov, and its next k-mer's record deleted."""
    nw = 4 if mer127 else 2
    P, SA, SB, _ = fork_with_junction(K, True)
    g1, g2, nP, n = np.concatenate([P, SA]), np.concatenate([P, SB]), len(P), 5
    last = node(g2[nP + n - K:nP + n])                                          # the tip's k-mer at the free side, reading away from the path
    what = "weak next by coverage " + flavour_id((K, mer127))
    c = Clipper(records_of(*count([(tile(g1, K), 5), ([branch_read(P, SB, n, K)], 2), ([branch_read(P, SB, n + 6, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        assert T.side(c.model.cnt, K, last, 2, 1)[0] == WN and T.side(c.model.cnt, K, last, 1, 1)[0] == 0
        solid = len(g1) - K + 1 + n
        totals, removed, _ = c.round(2, 1, MAX_TIP, what)
        assert totals == [1, n, solid, 0] and removed == set(branch_keys(P, SB, n, K)), what
        assert c.round(2, 1, MAX_TIP, what)[0] == [0, 0, solid - n, 0]
    finally:
        c.close()
    what = "weak next by the deleted bit " + flavour_id((K, mer127))
    occ, arcs = count([(tile(g1, K), 5), ([branch_read(P, SB, n + 3, K)], 1)], K)
    c = Clipper(records_of(occ, arcs, nw, deleted={branch_keys(P, SB, n + 1, K)[-1]}), K, mer127, device, twin)
    try:
        assert T.side(c.model.cnt, K, last, 1, 1)[0] == WN
        solid = len(g1) - K + 1 + n + 2
        totals, removed, _ = c.round(1, 1, MAX_TIP, what)
        assert totals == [1, n, solid, 0] and removed == set(branch_keys(P, SB, n, K)), what       # (the two k-mers behind the deleted one: free on both sides)
        assert c.round(1, 1, MAX_TIP, what)[0] == [0, 0, solid - n, 0]
    finally:
        c.close()


def check_ties(K, mer127, device, twin=None):
    """Two short dead ends forking from the path's last k-mer: counters 1 and 1 -- both kept; 2 and 1 -- only the weaker goes; 63 and
    63 -- both kept."""
    nw = 4 if mer127 else 2
    P, SA, SB, _ = fork_with_junction(K, False)
    a, b, p = branch_read(P, SA, 4, K), branch_read(P, SB, 4, K), node(P[-K:])
    for ca, cb, want in ((1, 1, 0), (2, 1, 1), (70, 70, 0)):
        what = "dead ends of %d and %d %s" % (ca, cb, flavour_id((K, mer127)))
        c = Clipper(records_of(*count([(tile(P, K), 3), ([a], ca), ([b], cb)], K), nw), K, mer127, device, twin)
        try:
            assert [out_counter(c.model, p, int(S[0])) for S in (SA, SB)] == [min(ca, 63), min(cb, 63)]
            solid = len(P) - K + 1 + 8
            totals, removed, _ = c.round(1, 1, MAX_TIP, what)
            assert totals == [want, 4 * want, solid, 2 - want] and removed == (set(branch_keys(P, SB, 4, K)) if want else set()), what
            if want:
                assert c.round(1, 1, MAX_TIP, what)[0] == [0, 0, solid - 4, 0]
        finally:
            c.close()


def check_two_tips_one_junction(K, mer127, device, twin=None):
    """Three arcs out of one junction side, one main and two minor tips: both clipped in one round, two counters of one 32-bit half of
    the junction's word cleared -- on the device by two lanes."""
    nw = 4 if mer127 else 2
    for fwd in (True, False):
        what = "two tips at one junction (%s) %s" % ("canonical" if fwd else "not canonical", flavour_id((K, mer127)))
        P, SA, SB, SC = fork_with_junction(K, fwd)
        g1 = np.concatenate([P, SA])
        c = Clipper(records_of(*count([(tile(g1, K), 5), ([branch_read(P, SB, 3, K)], 1), ([branch_read(P, SC, 5, K)], 2)], K), nw), K, mer127, device, twin)
        try:
            solid = len(g1) - K + 1 + 8
            totals, removed, cleared = c.round(1, 1, MAX_TIP, what)
            assert totals == [2, 8, solid, 0] and removed == set(branch_keys(P, SB, 3, K) + branch_keys(P, SC, 5, K)), what
            assert len(cleared) == 2 and len({(k, h) for k, h, _ in cleared}) == 1 and len({i for _, _, i in cleared}) == 2, what
            assert c.unitigs(1, 1)[0] == [G.emitted(g1, D, D, K)], what
        finally:
            c.close()


@functools.lru_cache(maxsize=None)
def tip_on_tip(K, mer127):
    """(records, path k-mers): a tip of 12 k-mers (two reads) on a 5-read path, and on its sixth k-mer a tip of 5 (one read)."""
    P, SA, SB, SC = fork_with_junction(K, True)
    g1, g2, nP = np.concatenate([P, SA]), np.concatenate([P, SB]), len(P)
    SC = SC.copy()
    SC[0] = (int(SB[6]) + 1) & 3
    second = np.concatenate([g2[nP + 6 - K - 3:nP + 6], SC[:5]])
    assert E.distinct_kmers([g1, g2[:nP + 12], second], K) == len(g1) - K + 1 + 12 + 5
    return records_of(*count([(tile(g1, K), 5), ([branch_read(P, SB, 12, K)], 2), ([second], 1)], K), 4 if mer127 else 2), len(g1) - K + 1


def check_tip_on_tip(K, mer127, device, twin=None):
    """Round 1 clips the tip on the tip (and keeps the tip's far half, the stronger arc into their junction), round 2 the tip, round 3
    nothing; the same through two calls queued back to back with no host wait between, and through clip_tips, which stops by itself."""
    what = "tip on a tip " + flavour_id((K, mer127))
    records, n_path = tip_on_tip(K, mer127)
    want = [[1, 5, n_path + 17, 1], [1, 12, n_path + 12, 0], [0, 0, n_path, 0]]
    c = Clipper(records, K, mer127, device, twin)
    try:
        assert c.settle(1, 1, MAX_TIP, what) == want
    finally:
        c.close()
    c = Clipper(records, K, mer127, device)
    try:
        before, bufs = c.words(), [c.totals(), c.totals()]
        for t in bufs:
            assert c.call(1, 1, MAX_TIP, t) == 0
        assert [[int(v) for v in c.down(c.ix, t)] for t in bufs] == want[:2], what + ": two calls back to back"
        removed = T.clip_round(c.model, 1, 1, MAX_TIP)[1] | T.clip_round(c.model, 1, 1, MAX_TIP)[1]
        after = c.words()
        assert (after == c.want_words()).all() and len(removed) == 17, what + ": two calls back to back"
        path_junction = canon(fork_with_junction(K, True)[0][-K:])               # (the small tip's junction is itself removed in round 2)
        for k, b, a in zip(c.keys, before.tolist(), after.tolist()):
            assert (a == 0) == (k in removed) and (a == b or k in removed or k == path_junction), what
    finally:
        c.close()
    c = Clipper(records, K, mer127, device)
    try:
        rounds = c.ix.clip_tips(1, 1, MAX_TIP)
        assert [[int(v) for v in r] for r in rounds] == want and api.tip_fields(rounds[0]) == dict(tips=1, kmers=5, solid=n_path + 17, kept=1), what
        assert [int(v) for v in c.ix.clip_tips(1, 1, MAX_TIP, max_rounds=1)[0]] == want[2]
        other = api.KmerIndex.from_records(records, K, mer127, device)
        try:
            assert len(other.clip_tips(1, 1, MAX_TIP, max_rounds=1)) == 1         # (max_rounds ends it before the fixed point)
            assert [int(r[0]) for r in other.clip_tips(1, 1)] == [1, 0]          # (max_tip = 2 K)
            assert (c.words(other) == c.words()).all(), what
        finally:
            other.close()
    finally:
        c.close()


def check_kept(K, mer127, device, twin=None):
    """What is no tip, whatever max_tip: the short start of the graph before a fork (DEAD_END to BRANCH_OUT) and the fork's two equal
    branches, a short chain free on both sides, a ring, and a chain from a dead end into a hairpin -- nothing is written."""
    nw = 4 if mer127 else 2
    what = "kept " + flavour_id((K, mer127))
    P, SA, SB, _ = fork_with_junction(K, True)
    short = P[-(K + 5):]
    island, ring, (_, h) = random_genome(5400 + K, K + 12), G.circular(K), G.hairpin(K)
    parts = [np.concatenate([short, SA]), np.concatenate([short, SB]), island, np.concatenate([ring, ring[:K - 1]]), h]
    n = 6 + 2 * (K + 40) + 13 + len(ring) + E.distinct_kmers([h], K)
    assert E.distinct_kmers(parts, K) == n
    groups = [(tile(parts[0], K), 3), (tile(parts[1], K), 3), (tile(island, K), 3), (tile(ring, K, circular=True), 2), (tile(h, K), 2)]
    c = Clipper(records_of(*count(groups, K), nw), K, mer127, device, twin)
    try:
        reasons = sorted(tuple(sorted((l, r))) for _, l, r in c.unitigs(1, 1)[0])   # (either orientation may be the one emitted)
        assert reasons == sorted([(D, BO), (D, BI), (D, BI), (D, D), (U.CYCLE, U.CYCLE), (D, U.HAIRPIN)]), what
        for max_tip in (1, MAX_TIP, api.TIP_MAX_BOUND):
            totals, removed, cleared = c.round(1, 1, max_tip, what)
            assert totals == [0, 0, n, 2 if max_tip >= K + 40 else 0] and not removed and not cleared, what
    finally:
        c.close()


def check_tombstone(K, mer127, device, twin=None):
    """kindex_cases' colliding keys, each alone in the graph, and in every group of keys with one home slot the middle one made a
    one-k-mer minor tip (a new junction record beside it): clipped, its slot stays taken, and every key behind it in the probe run is
    still found with its word."""
    nw = 4 if mer127 else 2
    what = "tombstones " + flavour_id((K, mer127))
    _, keys = KC.table("colliding", K, mer127)
    have, word, groups = set(keys), {k: 9 << 24 for k in keys}, {}
    for k in keys:
        groups.setdefault(M.home_slot(k, nw, 3000), []).append(k)
    tips, junctions = [], []
    for g in [g for g in groups.values() if len(g) >= 3][:64]:
        k = g[len(g) // 2]
        x = T.node_of_key(k, K)
        y = T.step(x, 0, K)
        jk, a = T.key_of(y), T.first_base(x, K)
        if jk in have:
            continue
        have.add(jk)
        word[k] |= 1 << 32                                                      # x is canonical: its right counter 0
        other = a ^ 1
        word[jk] = 9 << 24 | (1 << 6 * a | 5 << 6 * other if T.is_fwd(y) else (1 << 6 * (a ^ 2) | 5 << 6 * (other ^ 2)) << 32)
        tips.append(k)
        junctions.append(jk)
    assert len(tips) >= 8 and M.table_slots(len(word)) == 8192
    records = np.zeros((len(word), nw + 2), dtype=np.uint64)
    for i, k in enumerate(list(keys) + junctions):                              # (the colliding keys group by group: a serial build's runs are in that order)
        records[i, :nw] = M.words_of_key(k, nw)
        records[i, nw], records[i, nw + 1] = word[k], i
    c = Clipper(records, K, mer127, device, twin)
    try:
        totals, removed, cleared = c.round(5, 1, MAX_TIP, what)
        assert totals == [len(tips), len(tips), len(word), 0] and removed == set(tips) and sorted(k for k, _, _ in cleared) == sorted(junctions), what
        assert c.round(5, 1, MAX_TIP, what)[0] == [0, 0, len(word) - len(tips), 0]
    finally:
        c.close()


def check_empty(K, mer127, device, twin=None):
    c = Clipper(np.zeros((0, (4 if mer127 else 2) + 2), dtype=np.uint64), K, mer127, device, twin)
    try:
        assert c.round(1, 1, MAX_TIP, "empty")[0] == [0, 0, 0, 0]
        assert [int(v) for r in c.ix.clip_tips(1, 1) for v in r] == [0, 0, 0, 0]
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def many_tips(K, mer127, n_tips):
    """(records, path k-mers): a path with a one-k-mer tip every third k-mer -- a read that follows the path and ends in a wrong base."""
    g = random_genome(5300 + K + n_tips, K + 3 * n_tips + 10)
    wrong = []
    for i in range(n_tips):
        p = K + 3 + 3 * i
        wrong.append(np.concatenate([g[p - K - 3:p], codes([(int(g[p]) + 1 + i % 3) & 3])]))
    n_path = len(g) - K + 1
    assert E.distinct_kmers([g] + wrong, K) == n_path + n_tips
    return records_of(*count([(tile(g, K), 3), (wrong, 1)], K), 4 if mer127 else 2), n_path


def check_many_tips(K, mer127, device, twin=None):
    """257 and 513 one-k-mer tips on a long path, in a table of more slots than a workgroup has lanes: the start list crosses wave and
    workgroup edges.  All go in one round; the path's last stretch, the stronger arc into the last junction, is the one candidate kept."""
    for n_tips in (257, 513):
        what = "%d tips %s" % (n_tips, flavour_id((K, mer127)))
        records, n_path = many_tips(K, mer127, n_tips)
        assert M.table_slots(len(records)) > 256
        c = Clipper(records, K, mer127, device, twin)
        try:
            assert c.settle(1, 1, MAX_TIP, what) == [[n_tips, n_tips, n_path + n_tips, 1], [0, 0, n_path, 0]]
            assert len(c.unitigs(1, 1)[0]) == 1
        finally:
            c.close()


def check_noisy(K, mer127, device, twin=None):
    """The 2 kb genome with a repeat, read with 1 % substitutions, at min_cov 1 and 3: rounds to the fixed point against the model;
    there the model finds no minor tip among the unitigs the index then returns, and they are not more than before."""
    nw = 4 if mer127 else 2
    records = records_of(*count([(G.noisy(K), 1)], K), nw)
    max_tip = 2 * K
    for min_cov, min_arc in ((1, 1), (3, 2)):
        what = "noisy %s min_cov %d" % (flavour_id((K, mer127)), min_cov)
        c = Clipper(records, K, mer127, device, twin)
        try:
            n_before = len(c.unitigs(min_cov, min_arc)[0])
            rounds = c.settle(min_cov, min_arc, max_tip, what)
            assert min_cov > 1 or rounds[0][0] > 0, what + ": every error k-mer is solid, and not one minor tip"
            got, _ = c.unitigs(min_cov, min_arc)
            assert len(got) <= n_before, what
            for text, left, right in got:
                for t, l, r in ((list(text), left, right), (W.revcomp(list(text)), right, left)):
                    if l in (D, WN) and r == BI and len(t) - K + 1 <= max_tip:
                        last = node(t[-K:])
                        reason, y = T.side(c.model.cnt, K, last, min_cov, min_arc)
                        assert reason == BI and not T.is_minor(c.model.cnt, K, last, y), what + ": a minor tip is left"
            print("%s: %d -> %d unitigs in %d rounds, %s" % (what, n_before, len(got), len(rounds), rounds))
        finally:
            c.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with the pre-filled totals and every word of the table untouched: the thresholds' and max_tip's ranges, null
    totals, a null index, an index cut over ranks."""
    records, _ = tip_on_tip(K, mer127)
    c = Clipper(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    try:
        before, totals = c.words(), c.totals()
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64), dict(max_tip=0), dict(max_tip=api.TIP_MAX_BOUND + 1)):
            args = dict(dict(min_cov=1, min_arc=1, max_tip=MAX_TIP), **bad)
            assert c.call(args["min_cov"], args["min_arc"], args["max_tip"], totals) == EINVAL and b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert c.call(1, 1, MAX_TIP, None) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_clip_tips(None, 1, 1, MAX_TIP, None, None) == EINVAL
        assert L.pg_kindex_clip_tips(cut.h, 1, 1, MAX_TIP, c.ix._ptr(totals), c.ix._stream()) == ESTATE
        assert b"one lookup after the other in one table" in L.pg_last_error()
        with pytest.raises(api.PgError):
            cut.clip_tips(1, 1)
        with pytest.raises(api.PgError):
            c.ix.clip_tips(0, 1)
        assert (c.down(c.ix, totals) == FILL).all() and (c.words() == before).all()
        assert (c.words(cut) == before).all()
        assert c.call(1, 1, api.TIP_MAX_BOUND, totals) == 0 and int(c.down(c.ix, totals)[0]) == 1      # (the bound itself is taken)
    finally:
        cut.close()
        c.close()


DESIGNS = [check_branch, check_weak_next, check_ties, check_two_tips_one_junction, check_tip_on_tip, check_kept, check_tombstone, check_empty,
           check_many_tips, check_noisy]
