"""Bubble popping's cases, shared by tests/test_kbubble_host.py (the host twin) and tests/test_gpu_kbubble.py (the kernels): designed read
sets turned into records with the builders of tests/kwalk_cases.py and tests/ktip_cases.py, popped a round at a time through
pg_kindex_pop_bubbles, and after every round compared exactly with the model (tests/kbubble_model.py) and with what the construction
dictates: the four totals, and the word of EVERY key of the original set read back with query_ragged -- removed keys read 0, a
junction's word differs in exactly the counters the round cleared, every other word is bit-identical.  twin: a second index of the same
records (the host twin beside a device index) is popped in step, and the two must agree word for word -- a round's result is a function
of the index alone.  All comparisons are of integers and exact.

Every bubble here is cut from a path g at a place p: the FORK u is g[p - K:p], the JOIN v is g[p + 1:p + K + 1], and the k-mers that
start at p - K + 1 .. p lie between them -- K of them on the path itself and on a copy with another base at p, K - 1 on a copy with g[p]
left out.  No two paths between one fork and one join are shorter than that: an arm of fewer than K - 1 k-mers leaves bases of u in v."""
import functools

import numpy as np
import pytest

import kbubble_model as B
import kindex_cases as KC
import kindex_model as M
import ktip_cases as TC
import ktip_model as T
import kunitig_cases as G
import kunitig_model as U
import kwalk_cases as E
import kwalk_model as W
from ktip_cases import branch_keys, canon, node
from kwalk_cases import codes, count, random_genome, rc, records_of, tile
from soapdenovo2_amd import api

FLAVOURS = TC.FLAVOURS                        # both NW: K = 31 in the 63-mer build, K = 65 in the 127-mer one
flavour_id = KC.flavour_id
FILL = E.FILL
EINVAL, ESTATE = E.EINVAL, E.ESTATE
D, BO, WN, BI = T.DEAD_END, T.BRANCH_OUT, T.WEAK_NEXT, T.BRANCH_IN
BOUND = api.BUBBLE_MAX_BOUND
FLANK = 40                                    # path k-mers before a design's first fork and behind its last join


class Bubbler(TC.Clipper):
    """ktip_cases.Clipper -- the index under test, its model, maybe a twin, the word of every original key -- with a round of bubbles
    beside the round of tips."""

    def pop_call(self, min_cov, min_arc, max_len, max_diff, totals, ix=None):
        ix = ix or self.ix
        return api.lib().pg_kindex_pop_bubbles(ix.h, min_cov, min_arc, max_len, max_diff, ix._ptr(totals), ix._stream())

    def pop(self, min_cov, min_arc, max_len, max_diff=0, what=""):
        """One round of bubbles, as Clipper._round returns it."""
        return self._round(self.pop_call, B.pop_round, (min_cov, min_arc, max_len, max_diff), what)

    def pop_settle(self, min_cov, min_arc, max_len, max_diff=0, what=""):
        return self._settle(lambda w: self.pop(min_cov, min_arc, max_len, max_diff, w), what)

    def simplify_by_rounds(self, min_cov, min_arc, max_tip, max_len, max_diff=0, what=""):
        """KmerIndex.simplify's order of calls made one ABI round at a time, each compared: the list of (name, totals)."""
        out = []
        while True:
            removed = 0
            for name in ("tips", "bubbles"):
                while True:
                    tag = "%s call %d (%s)" % (what, len(out) + 1, name)
                    t = self.round(min_cov, min_arc, max_tip, tag)[0] if name == "tips" else self.pop(min_cov, min_arc, max_len, max_diff, tag)[0]
                    out.append((name, t))
                    removed += t[0]
                    assert len(out) <= 64
                    if not t[0]:
                        break
            if not removed:
                return out


def model_simplify(model, min_cov, min_arc, max_tip, max_len, max_diff=0, max_rounds=64):
    """KmerIndex.simplify as its documentation states it, on the model: tips to their fixed point, bubbles to theirs, until a whole cycle
    removes nothing or max_rounds rounds were made."""
    out = []
    while len(out) < max_rounds:
        removed = 0
        for name in ("tips", "bubbles"):
            while len(out) < max_rounds:
                t = T.clip_round(model, min_cov, min_arc, max_tip)[0] if name == "tips" else B.pop_round(model, min_cov, min_arc, max_len, max_diff)[0]
                out.append((name, t))
                removed += t[0]
                if not t[0]:
                    break
        if not removed:
            break
    return out


def plain(rounds):
    return [(name, [int(v) for v in t]) for name, t in rounds]


# ---- the genomes ----
def other(g, p, d=1):
    """g with another base at p."""
    v = g.copy()
    v[p] = (int(g[p]) + d) & 3
    return v


def without(g, p):
    """g with the base at p left out; its neighbours differ from it, so the fork and the join stay where a substitution has them."""
    assert g[p - 1] != g[p] != g[p + 1]
    return np.concatenate([g[:p], g[p + 1:]])


def arm_read(v, p, K, n=None):
    """The read that carries the arm of n k-mers (K: a substitution, K - 1: a base left out) at p of the copy v, four path k-mers
    before it and four behind."""
    return v[p - K - 3:p + (K if n is None else n) + 4]


def arm_keys(v, p, K, n=None):
    return [canon(v[j:j + K]) for j in range(p - K + 1, p - K + 1 + (K if n is None else n))]


def junctions(g, p, K):
    """(L, v) of the bubble at p as the model's oriented k-mers: L = rc(u), as the step from an arm's rc(x0) reaches it."""
    return node(rc(g[p - K:p])), node(g[p + 1:p + K + 1])


def cleared_by(g, p, K, base):
    """The two counters a popped arm whose base at p is `base` loses: (junction key, half, counter), sorted."""
    L, v = junctions(g, p, K)
    out = []
    for y, a in ((v, int(base)), (L, int(base) ^ 2)):                           # (the first base of the arm's last k-mer; of rc of its first)
        out.append((T.key_of(y),) + ((0, a) if T.is_fwd(y) else (1, a ^ 2)))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def path(K, seed, n_places=1, gap=None, extra=0):
    """(g, p): a path with n_places places p, p + gap, .. (gap K + 1: the join of one bubble is the fork of the next), FLANK k-mers before
    the first fork and behind the last join, every canonical k-mer once."""
    gap = K + 1 if gap is None else gap
    p = K + FLANK - 1
    g = random_genome(seed, p + (n_places - 1) * gap + extra + 1 + K + FLANK - 1)
    assert E.distinct_kmers([g], K) == len(g) - K + 1
    return g, p


@functools.lru_cache(maxsize=None)
def path_with_junctions(K, l_fwd, v_fwd):
    """A path whose bubble at p has L and v as their canonical forms or not, as asked."""
    for seed in range(6100 + K, 6300 + K):
        g, p = path(K, seed)
        L, v = junctions(g, p, K)
        if T.is_fwd(L) == l_fwd and T.is_fwd(v) == v_fwd and g[p - 1] != g[p] != g[p + 1]:
            return g, p
    raise AssertionError("no seed gives those junctions")


def flanks(g, p, K, copies, q=None):
    """The path before the fork at p and behind the join at q, tiled: the k-mers between are left to the arms' own reads."""
    return [(tile(g[:p], K), copies), (tile(g[(p if q is None else q) + 1:], K), copies)]


# ---- the designs ----
def check_substitution(K, mer127, device, twin=None):
    """A 5-read path and a 1-read copy with another base at p: two arms of K k-mers.  Untouched at max_len = K - 1, popped at K; then
    one unitig, the path, with covered == solid; L and v each canonical and not; the reads reverse complemented; and the popped index
    beside one built without the copy's records."""
    nw = 4 if mer127 else 2
    for l_fwd, v_fwd in ((True, True), (True, False), (False, True), (False, False)):
        g, p = path_with_junctions(K, l_fwd, v_fwd)
        var = other(g, p)
        what = "substitution, L %s, v %s, %s" % ("canonical" if l_fwd else "not", "canonical" if v_fwd else "not", flavour_id((K, mer127)))
        main, minor = tile(g, K), arm_read(var, p, K)
        records = records_of(*count([(main, 5), ([minor], 1)], K), nw)
        swapped = records_of(*count([([rc(r) for r in main], 5), ([rc(minor)], 1)], K), nw)
        arm, n_path = set(arm_keys(var, p, K)), len(g) - K + 1
        assert len(arm) == K and len(records) == n_path + K
        for recs in (records, swapped):
            c = Bubbler(recs, K, mer127, device, twin)
            try:
                solid = n_path + K
                assert c.pop(1, 1, K - 1, 0, what)[0] == [0, 0, solid, 0]
                totals, removed, cleared = c.pop(1, 1, K, 0, what)
                assert totals == [1, K, solid, 1] and removed == arm, what
                assert sorted(cleared) == cleared_by(g, p, K, var[p]), what
                got, t = c.unitigs(1, 1)
                assert got == [G.emitted(g, D, D, K)] and t["covered"] == t["solid"] == n_path, what
                assert c.pop(1, 1, K, 0, what)[0] == [0, 0, n_path, 0]
            finally:
                c.close()
        if l_fwd and not v_fwd:
            check_as_if_never_there(records, arm, g, p, K, mer127, device, what)


def check_as_if_never_there(records, arm, g, p, K, mer127, device, what):
    """After the pop the index answers as one built without the arm's records: every word but the two junctions', where that index keeps
    the arcs to the k-mers it never had; the walks from the path's ends at min_arc 2 -- and at min_arc 1 only the popped index walks
    through, which is what the cleared counters are for."""
    nw = 4 if mer127 else 2
    c = Bubbler(records, K, mer127, device)
    bare = api.KmerIndex.from_records(records[[M.key_of_record(r, nw) not in arm for r in records]], K, mer127, device)
    try:
        assert c.pop(1, 1, K, 0, what)[0][:2] == [1, K]
        popped, never = c.words(), c.words(bare)
        ends = {T.key_of(y) for y in junctions(g, p, K)}
        assert len(ends) == 2
        for k, a, b in zip(c.keys, popped.tolist(), never.tolist()):
            if k in ends:
                x = a ^ b
                assert x and a & x == 0 and x in [1 << s for s in (0, 6, 12, 18, 32, 38, 44, 50)], what + ": a junction's one counter, which was 1"
            else:
                assert a == b and (a == 0) == (k in arm), what
        tips = [g[:K], g[-K:]]
        for ix in (c.ix, bare):
            seqs, f = api.extend_seqs(tips, ix, 1, 2)
            assert [list(s) for s in seqs] == [list(g), list(g)] and f["reason"] == ["dead_end"] * 4, what
        seqs, _ = api.extend_seqs(tips, c.ix, 1, 1)
        assert [list(s) for s in seqs] == [list(g), list(g)], what
        seqs, f = api.extend_seqs(tips[:1], bare, 1, 1)
        assert f["reason"][0] == "branch_out" and len(seqs[0]) < len(g), what
    finally:
        bare.close()
        c.close()


def check_ties(K, mer127, device, twin=None):
    """Two arms each read by its own reads alone, so every k-mer of an arm has the coverage of its reads: 1 and 1 -- both kept; 2 and
    1 -- the weaker goes; 300 and 260, both saturated at 255 -- both kept."""
    nw = 4 if mer127 else 2
    g, p = path_with_junctions(K, False, True)
    var = other(g, p)
    for ca, cb, want in ((1, 1, 0), (2, 1, 1), (300, 260, 0)):
        what = "arms of %d and %d %s" % (ca, cb, flavour_id((K, mer127)))
        c = Bubbler(records_of(*count(flanks(g, p, K, 3) + [([arm_read(g, p, K)], ca), ([arm_read(var, p, K)], cb)], K), nw), K, mer127, device, twin)
        try:
            for arm, n in ((g, ca), (var, cb)):
                assert {M.coverage(c.model.cnt[k]) for k in arm_keys(arm, p, K)} == {min(n, 255)}
            solid = len(g) - K + 1 + K
            totals, removed, _ = c.pop(1, 1, K, 0, what)
            assert totals == [want, K * want, solid, 2 - want] and removed == (set(arm_keys(var, p, K)) if want else set()), what
            if want:
                assert c.pop(1, 1, K, 0, what)[0] == [0, 0, solid - K, 0]
        finally:
            c.close()


def check_three_siblings(K, mer127, device, twin=None):
    """Three arms of one bubble, read 5, 2 and 1 times: the two weaker go in one round, each junction loses two counters of one 32-bit
    half -- on the device to two lanes --, and the path is one unitig."""
    nw = 4 if mer127 else 2
    for l_fwd, v_fwd in ((True, False), (False, True)):
        what = "three siblings (L %s) %s" % ("canonical" if l_fwd else "not canonical", flavour_id((K, mer127)))
        g, p = path_with_junctions(K, l_fwd, v_fwd)
        b, c3 = other(g, p, 1), other(g, p, 2)
        c = Bubbler(records_of(*count([(tile(g, K), 5), ([arm_read(b, p, K)], 2), ([arm_read(c3, p, K)], 1)], K), nw), K, mer127, device, twin)
        try:
            solid = len(g) - K + 1 + 2 * K
            totals, removed, cleared = c.pop(1, 1, K, 0, what)
            assert totals == [2, 2 * K, solid, 1] and removed == set(arm_keys(b, p, K) + arm_keys(c3, p, K)), what
            assert sorted(cleared) == sorted(cleared_by(g, p, K, b[p]) + cleared_by(g, p, K, c3[p])), what
            assert len({(k, h) for k, h, _ in cleared}) == 2 and len(set(cleared)) == 4, what
            assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
            assert c.pop(1, 1, K, 0, what)[0] == [0, 0, solid - 2 * K, 0]
        finally:
            c.close()


def check_unequal(K, mer127, device, twin=None):
    """An arm of K k-mers read K + 9 times and one of K - 1 read K + 10 times: the shorter has the greater mean and the smaller sum.
    Kept at max_diff 0; at 1 the LONGER one goes, which a comparison of sums would keep."""
    nw = 4 if mer127 else 2
    what = "unequal lengths " + flavour_id((K, mer127))
    g, p = path_with_junctions(K, True, True)
    short = without(g, p)
    ca, cb = K + 9, K + 10
    assert ca * K > cb * (K - 1) and cb > ca and cb <= 255
    groups = flanks(g, p, K, 3) + [([arm_read(g, p, K)], ca), ([arm_read(short, p, K, K - 1)], cb)]
    c = Bubbler(records_of(*count(groups, K), nw), K, mer127, device, twin)
    try:
        long_keys, short_keys = arm_keys(g, p, K), arm_keys(short, p, K, K - 1)
        assert len(set(long_keys + short_keys)) == 2 * K - 1
        assert sum(M.coverage(c.model.cnt[k]) for k in long_keys) == ca * K and sum(M.coverage(c.model.cnt[k]) for k in short_keys) == cb * (K - 1)
        solid = len(g) - K + 1 + K - 1
        assert c.pop(1, 1, K, 0, what)[0] == [0, 0, solid, 2]
        totals, removed, _ = c.pop(1, 1, K, 1, what)
        assert totals == [1, K, solid, 1] and removed == set(long_keys), what
        assert c.unitigs(1, 1)[0] == [G.emitted(short, D, D, K)], what
    finally:
        c.close()


def check_shared_junction(K, mer127, device, twin=None):
    """Substitutions K + 1 apart: the join of the first bubble is the fork of the second.  Both pop in one round, and that k-mer's word
    loses a counter of each of its halves."""
    nw = 4 if mer127 else 2
    what = "two bubbles at one k-mer " + flavour_id((K, mer127))
    g, p = path(K, 6400 + K, 2)
    q = p + K + 1
    a, b = other(g, p), other(g, q)
    c = Bubbler(records_of(*count([(tile(g, K), 5), ([arm_read(a, p, K)], 1), ([arm_read(b, q, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        shared = canon(g[p + 1:p + K + 1])
        assert shared == canon(g[q - K:q])
        solid = len(g) - K + 1 + 2 * K
        totals, removed, cleared = c.pop(1, 1, K, 0, what)
        assert totals == [2, 2 * K, solid, 2] and removed == set(arm_keys(a, p, K) + arm_keys(b, q, K)), what
        assert sorted(cleared) == sorted(cleared_by(g, p, K, a[p]) + cleared_by(g, q, K, b[q])), what
        assert sorted(h for k, h, _ in cleared if k == shared) == [0, 1], what
        assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
    finally:
        c.close()


W_OUTER = 8                                    # bases of the outer bubble's window: its arms have K + W_OUTER - 1 k-mers


@functools.lru_cache(maxsize=None)
def nested(K, mer127):
    """(records, path k-mers): a 5-read path; a 2-read copy that differs in the W_OUTER bases from p on -- the outer bubble, arms of
    K + W_OUTER - 1 k-mers --; and a 1-read copy of the path with another base at p + 4: a bubble of K on the outer bubble's strong arm."""
    for seed in range(6500 + K, 6600 + K):
        g, p = path(K, seed, 1, None, W_OUTER - 1)
        outer = g.copy()
        outer[p:p + W_OUTER] = (g[p:p + W_OUTER] + 1 + np.arange(W_OUTER) % 3) & 3
        inner = other(g, p + 4)
        reads = [g, outer[p - K - 3:p + W_OUTER - 1 + K + 4], arm_read(inner, p + 4, K)]
        if E.distinct_kmers(reads, K) == len(g) - K + 1 + K + W_OUTER - 1 + K:
            records = records_of(*count([(tile(g, K), 5), ([reads[1]], 2), ([reads[2]], 1)], K), 4 if mer127 else 2)
            return records, len(g) - K + 1
    raise AssertionError("no seed gives distinct k-mers")


def check_nested(K, mer127, device, twin=None):
    """Round 1 pops the inner bubble's weak arm -- the outer bubble's weak arm is kept, its alternative is not linear yet --, round 2 the
    outer one's, round 3 nothing; the same through two calls queued back to back with no host wait between, and through pop_bubbles,
    which stops by itself."""
    what = "a bubble on an arm " + flavour_id((K, mer127))
    records, n_path = nested(K, mer127)
    n_out = K + W_OUTER - 1
    want = [[1, K, n_path + n_out + K, 2], [1, n_out, n_path + n_out, 1], [0, 0, n_path, 0]]
    c = Bubbler(records, K, mer127, device, twin)
    try:
        assert c.pop_settle(1, 1, n_out, 0, what) == want
        assert len(c.unitigs(1, 1)[0]) == 1
    finally:
        c.close()
    c = Bubbler(records, K, mer127, device)
    try:
        before, bufs = c.words(), [c.totals(), c.totals()]
        for t in bufs:
            assert c.pop_call(1, 1, n_out, 0, t) == 0
        assert [[int(v) for v in c.down(c.ix, t)] for t in bufs] == want[:2], what + ": two calls back to back"
        first = B.pop_round(c.model, 1, 1, n_out, 0)
        second = B.pop_round(c.model, 1, 1, n_out, 0)
        removed, ends = first[1] | second[1], {k for k, _, _ in first[2] + second[2]}
        after = c.words()
        assert (after == c.want_words()).all() and len(removed) == n_out + K, what + ": two calls back to back"
        for k, b, a in zip(c.keys, before.tolist(), after.tolist()):
            assert (a == 0) == (k in removed) and (a == b or k in removed or k in ends), what
    finally:
        c.close()
    c = Bubbler(records, K, mer127, device)
    try:
        rounds = c.ix.pop_bubbles(1, 1, n_out)
        assert [[int(v) for v in r] for r in rounds] == want, what
        assert api.bubble_fields(rounds[0]) == dict(branches=1, kmers=K, solid=n_path + n_out + K, kept=2), what
        assert [int(v) for v in c.ix.pop_bubbles(1, 1, n_out, max_rounds=1)[0]] == want[2]
        fresh = api.KmerIndex.from_records(records, K, mer127, device)
        try:
            assert len(fresh.pop_bubbles(1, 1, n_out, max_rounds=1)) == 1        # (max_rounds ends it before the fixed point)
            assert [int(r[0]) for r in fresh.pop_bubbles(1, 1)] == [1, 0]        # (max_len = 2 K)
            assert (c.words(fresh) == c.words()).all(), what
        finally:
            fresh.close()
    finally:
        c.close()


TIP_AT = 5                                     # the tip leaves the strong arm behind its k-mer that ends at p + TIP_AT


@functools.lru_cache(maxsize=None)
def tip_on_arm(K, mer127):
    """(records, path k-mers): a 5-read path, a 2-read copy with another base at p, and one read that follows the path into the
    strong arm and ends in a wrong base: a tip of one k-mer on an arm."""
    g, p = path(K, 6700 + K)
    var, t = other(g, p), p + TIP_AT
    tip = np.concatenate([g[t - K - 3:t], codes([(int(g[t]) + 1) & 3])])
    assert E.distinct_kmers([g, arm_read(var, p, K), tip], K) == len(g) - K + 1 + K + 1
    return records_of(*count([(tile(g, K), 5), ([arm_read(var, p, K)], 2), ([tip], 1)], K), 4 if mer127 else 2), len(g) - K + 1


def check_tip_on_arm(K, mer127, device, twin=None):
    """A tip on the strong arm: pop_bubbles alone leaves the bubble, whose strong arm is not linear; simplify clips the tip, pops the
    weak arm and makes an empty cycle -- its order of calls and their totals are the model's, driven the same way."""
    what = "a tip on an arm " + flavour_id((K, mer127))
    records, n_path = tip_on_arm(K, mer127)
    solid = n_path + K + 1
    c = Bubbler(records, K, mer127, device, twin)
    try:
        assert [[int(v) for v in r] for r in c.ix.pop_bubbles(1, 1, K)] == [[0, 0, solid, 2]], what   # (kept: the weak arm, and the strong arm behind the tip)
        assert (c.words() == c.want_words()).all(), what
        assert c.simplify_by_rounds(1, 1, TC.MAX_TIP, K, 0, what) == [
            ("tips", [1, 1, solid, 0]), ("tips", [0, 0, solid - 1, 0]), ("bubbles", [1, K, solid - 1, 1]), ("bubbles", [0, 0, n_path, 0]),
            ("tips", [0, 0, n_path, 0]), ("bubbles", [0, 0, n_path, 0])], what
    finally:
        c.close()
    c = Bubbler(records, K, mer127, device)
    try:
        got = plain(c.ix.simplify(1, 1, TC.MAX_TIP, K))
        assert got == model_simplify(c.model, 1, 1, TC.MAX_TIP, K) and len(got) == 6, what
        assert (c.words() == c.want_words()).all() and len(c.unitigs(1, 1)[0]) == 1, what
    finally:
        c.close()
    c = Bubbler(records, K, mer127, device)
    try:
        got = plain(c.ix.simplify(1, 1, TC.MAX_TIP, K, max_rounds=3))             # (max_rounds ends it inside the first cycle)
        assert got == model_simplify(c.model, 1, 1, TC.MAX_TIP, K, max_rounds=3) and [n for n, _ in got] == ["tips", "tips", "bubbles"], what
        assert (c.words() == c.want_words()).all(), what
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def two_loops(K):
    """(reads as groups, k-mers): X u B u Y read five times and u A u once: two loops of K + 2 k-mers from u back to u, one weak."""
    for seed in range(6800 + K, 6900 + K):
        r = random_genome(seed, 2 * (K + 20) + K + 6)
        X, Y, u, A, Bs = r[:K + 20], r[K + 20:2 * (K + 20)], r[2 * (K + 20):3 * K + 40], r[-6:-3], r[-3:]
        if A[0] == Bs[0] or A[0] == Y[0] or Bs[0] == Y[0] or A[-1] == Bs[-1] or A[-1] == X[-1] or Bs[-1] == X[-1]:
            continue
        strong, weak = np.concatenate([X, u, Bs, u, Y]), np.concatenate([u, A, u])
        n = len(strong) - K + 1 - 1 + K + 2                                     # (u twice on the strong path; the weak loop's K + 2)
        if E.distinct_kmers([strong, weak], K) == n:
            return ((tuple(tile(strong, K)), 5), ((weak,), 1)), n, [strong, weak]
    raise AssertionError("no seed gives those loops")


def check_kept(K, mer127, device, twin=None):
    """What is no minor branch, whatever max_len: a loop u -> P -> u beside a second, stronger loop; a weak arm beside an arm with a
    fork inside (the tip on it) -- and with them the path before the bubble's fork and behind its join --; an arm longer than max_len; a
    tip, an island, a ring and a hairpin's chain.  Nothing is written."""
    nw = 4 if mer127 else 2
    what = "kept " + flavour_id((K, mer127))
    groups, n, _ = two_loops(K)
    c = Bubbler(records_of(*count([(list(r), k) for r, k in groups], K), nw), K, mer127, device, twin)
    try:
        sides = sorted(tuple(sorted((l, r))) for _, l, r in c.unitigs(1, 1)[0])
        assert sides.count((BI, BI)) == 2, what                                  # (the two loops: BRANCH_IN on both sides, and no branch)
        for max_len in (1, K + 2, BOUND):
            totals, removed, cleared = c.pop(1, 1, max_len, BOUND, what + ": loops")
            assert totals == [0, 0, n, 0] and not removed and not cleared, what
    finally:
        c.close()
    records, n_path = tip_on_arm(K, mer127)
    c = Bubbler(records, K, mer127, device, twin)
    try:
        for max_len in (1, K - 1, K, BOUND):
            totals, removed, cleared = c.pop(1, 1, max_len, BOUND, what + ": a fork inside the sibling")
            # (kept: the strong arm's K - TIP_AT k-mers behind the tip's junction are a branch too, with the tip for a sibling that dead-ends)
            kept = (1 if max_len >= K - TIP_AT else 0) + (1 if max_len >= K else 0)
            assert totals == [0, 0, n_path + K + 1, kept] and not removed and not cleared, what
    finally:
        c.close()
    P, SA, SB, _ = TC.fork_with_junction(K, True)
    short = P[-(K + 5):]
    island, ring, (_, h) = random_genome(5400 + K, K + 12), G.circular(K), G.hairpin(K)
    parts = [np.concatenate([short, SA]), np.concatenate([short, SB]), island, np.concatenate([ring, ring[:K - 1]]), h]
    n = 6 + 2 * (K + 40) + 13 + len(ring) + E.distinct_kmers([h], K)
    assert E.distinct_kmers(parts, K) == n
    groups = [(tile(parts[0], K), 3), (tile(parts[1], K), 3), (tile(island, K), 3), (tile(ring, K, circular=True), 2), (tile(h, K), 2)]
    c = Bubbler(records_of(*count(groups, K), nw), K, mer127, device, twin)
    try:
        for max_len in (1, K + 40, BOUND):
            totals, removed, cleared = c.pop(1, 1, max_len, BOUND, what + ": tips, an island, a ring, a hairpin")
            assert totals == [0, 0, n, 0] and not removed and not cleared, what
    finally:
        c.close()


def tombstone_groups(K):
    """How many of the colliding groups get a bubble: 2 K + 1 new keys each, and the table must stay the one the keys collide in."""
    return (4096 - 3000) // (2 * K + 1)


def check_tombstone(K, mer127, device, twin=None):
    """kindex_cases' colliding keys, each alone in the graph, and for as many groups of keys with one home slot as the table's size
    allows (tombstone_groups) the middle key made the middle k-mer of a bubble's weak arm -- a path of K + 2 k-mers read three times and
    the copy that holds the key read once, counted into new records beside it.  The arms are popped, their slots stay taken, and every
    key behind them in the probe runs is still found with its word."""
    nw = 4 if mer127 else 2
    what = "tombstones " + flavour_id((K, mer127))
    _, keys = KC.table("colliding", K, mer127)
    have, word, groups = set(keys), {k: 9 << 24 for k in keys}, {}
    for k in keys:
        groups.setdefault(M.home_slot(k, nw, 3000), []).append(k)
    rng = np.random.default_rng(6900 + K)
    arms, extra, reads = [], [], []
    at = (K + 1) // 2                                                           # the key is the weak copy's k-mer that starts here
    for grp in [grp for grp in groups.values() if len(grp) >= 3]:
        if len(arms) == tombstone_groups(K):
            break
        k = grp[len(grp) // 2]
        weak = np.concatenate([rng.integers(0, 4, size=at, dtype=np.uint8), E.codes_of_key(k, K), rng.integers(0, 4, size=K + 1 - at, dtype=np.uint8)])
        strong = other(weak, K)
        new = set(M.canonical_kmers(strong, K)) | set(M.canonical_kmers(weak, K))
        if len(new) != 2 * K + 2 or new & (have - {k}):
            continue
        have |= new
        arms.append([canon(weak[j:j + K]) for j in range(1, K + 1)])
        assert arms[-1][at - 1] == k
        extra += sorted(new - {k})
        reads += [([strong], 3), ([weak], 1)]
    assert len(arms) == tombstone_groups(K) >= 8
    counted = records_of(*count(reads, K), nw)
    for r in counted:
        word[M.key_of_record(r, nw)] = int(r[nw])
    assert M.table_slots(len(word)) == 8192 and len(word) == 3000 + len(extra)
    records = np.zeros((len(word), nw + 2), dtype=np.uint64)
    for i, k in enumerate(list(keys) + extra):                                  # (the colliding keys group by group: a serial build's runs are in that order)
        records[i, :nw] = M.words_of_key(k, nw)
        records[i, nw], records[i, nw + 1] = word[k], i
    c = Bubbler(records, K, mer127, device, twin)
    try:
        n = len(arms)
        totals, removed, cleared = c.pop(1, 1, K, 0, what)
        assert totals == [n, n * K, len(word), n] and removed == {k for a in arms for k in a} and len(cleared) == 2 * n, what
        assert c.pop(1, 1, K, 0, what)[0] == [0, 0, len(word) - n * K, 0]
    finally:
        c.close()


def check_empty(K, mer127, device, twin=None):
    c = Bubbler(np.zeros((0, (4 if mer127 else 2) + 2), dtype=np.uint64), K, mer127, device, twin)
    try:
        assert c.pop(1, 1, K, 0, "empty")[0] == [0, 0, 0, 0]
        assert [int(v) for r in c.ix.pop_bubbles(1, 1) for v in r] == [0, 0, 0, 0]
        assert plain(c.ix.simplify(1, 1)) == [("tips", [0, 0, 0, 0]), ("bubbles", [0, 0, 0, 0])]
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def many_bubbles(K, mer127, n_bubbles):
    """(records, path k-mers, sources): substitutions K + 1 apart along one path, each read once on a path read three times: n_bubbles
    bubbles chained join to fork, with arms of K k-mers -- the shortest two arms of one length can be."""
    g, p = path(K, 7000 + K + n_bubbles, n_bubbles)
    weak = [arm_read(other(g, p + i * (K + 1), 1 + i % 3), p + i * (K + 1), K) for i in range(n_bubbles)]
    n_path = len(g) - K + 1
    records = records_of(*count([(tile(g, K, step=32, extra=40), 3), (weak, 1)], K), 4 if mer127 else 2)
    assert len(records) == n_path + n_bubbles * K
    return records, n_path, [g] + weak


def check_many_bubbles(K, mer127, device, twin=None, n_bubbles=257):
    """257 bubbles on one path: six starts a bubble, so the start list crosses wave and workgroup edges many times over.  All weak arms
    go in one round.  (The table has as many slots as 2 K + 1 keys a bubble need -- arms cannot be shorter, see the module's head --,
    not the few thousand of the other designs.)"""
    what = "%d bubbles %s" % (n_bubbles, flavour_id((K, mer127)))
    records, n_path, sources = many_bubbles(K, mer127, n_bubbles)
    c = Bubbler(records, K, mer127, device, twin, sources)
    try:
        assert c.pop_settle(1, 1, K, 0, what) == [[n_bubbles, n_bubbles * K, n_path + n_bubbles * K, n_bubbles], [0, 0, n_path, 0]]
        assert len(c.unitigs(1, 1)[0]) == 1
    finally:
        c.close()


def check_many_more_bubbles(K, mer127, device, twin=None):
    """513 bubbles on one path."""
    check_many_bubbles(K, mer127, device, twin, 513)


@functools.lru_cache(maxsize=None)
def noisy(K):
    """kunitig_cases.noisy with reads long enough to carry a bubble at either K -- a substitution's K k-mers and a k-mer on each
    side of them need 2 K + 1 bases --: a genome of 2 000 bases with a repeat of 150, 150 reads of 2 K + 40 bases on both strands with
    1 % substitutions."""
    rng = np.random.default_rng(7100 + K)
    g = rng.integers(0, 4, size=2000, dtype=np.uint8)
    g[1200:1350] = g[200:350]
    L, reads = 2 * K + 40, []
    for i in range(150):
        at = int(rng.integers(0, len(g) - L + 1))
        r = g[at:at + L].copy()
        hit = rng.random(L) < 0.01
        r[hit] = (r[hit] + rng.integers(1, 4, size=int(hit.sum()))) & 3
        reads.append(rc(r) if i % 2 else r)
    return reads


def check_noisy(K, mer127, device, twin=None):
    """The 2 kb genome with a repeat, read with 1 % substitutions, at min_cov 1 and 3: simplify's rounds to the fixed point, each
    against the model; there the model finds no minor tip and no minor branch, and the unitigs are not more than before.  At min_cov 1
    the model pops at least one branch."""
    nw = 4 if mer127 else 2
    records = records_of(*count([(noisy(K), 1)], K), nw)
    limit = 2 * K
    for min_cov, min_arc in ((1, 1), (3, 2)):
        what = "noisy %s min_cov %d" % (flavour_id((K, mer127)), min_cov)
        c = Bubbler(records, K, mer127, device, twin)
        try:
            n_before = len(c.unitigs(min_cov, min_arc)[0])
            rounds = c.simplify_by_rounds(min_cov, min_arc, limit, limit, 0, what)
            popped = sum(t[0] for name, t in rounds if name == "bubbles")
            assert min_cov > 1 or popped > 0, what + ": every error k-mer is solid, and not one bubble"
            assert len(c.unitigs(min_cov, min_arc)[0]) <= n_before, what
            cnt = c.model.cnt
            assert not [1 for _, last, y in T.candidates(cnt, K, min_cov, min_arc, limit) if T.is_minor(cnt, K, last, y)], what + ": a minor tip is left"
            assert not B.decide(cnt, K, min_cov, min_arc, limit, 0)[0], what + ": a minor branch is left"
            print("%s: %d -> %d unitigs, %d branches popped, %s" % (what, n_before, len(c.unitigs(min_cov, min_arc)[0]), popped, rounds))
        finally:
            c.close()
    c = Bubbler(records, K, mer127, device)
    try:
        assert plain(c.ix.simplify(1, 1)) == model_simplify(c.model, 1, 1, limit, limit), "noisy: simplify's calls are not the model's"
        assert (c.words() == c.want_words()).all()
    finally:
        c.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with the pre-filled totals and every word of the table untouched: the thresholds', max_len's and max_diff's
    ranges, null totals, a null index, an index cut over ranks."""
    records, _ = nested(K, mer127)
    c = Bubbler(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    n_out = K + W_OUTER - 1
    try:
        before, totals = c.words(), c.totals()
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64), dict(max_len=0), dict(max_len=BOUND + 1),
                    dict(max_diff=BOUND + 1)):
            args = dict(dict(min_cov=1, min_arc=1, max_len=n_out, max_diff=0), **bad)
            assert c.pop_call(args["min_cov"], args["min_arc"], args["max_len"], args["max_diff"], totals) == EINVAL, bad
            assert b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert c.pop_call(1, 1, n_out, 0, None) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_pop_bubbles(None, 1, 1, n_out, 0, None, None) == EINVAL
        assert L.pg_kindex_pop_bubbles(cut.h, 1, 1, n_out, 0, c.ix._ptr(totals), c.ix._stream()) == ESTATE
        assert b"one lookup after the other in one table" in L.pg_last_error()
        for call in (lambda: cut.pop_bubbles(1, 1), lambda: cut.simplify(1, 1), lambda: c.ix.pop_bubbles(0, 1), lambda: c.ix.simplify(1, 64),
                     lambda: c.ix.pop_bubbles(1, 1, max_diff=BOUND + 1)):
            with pytest.raises(api.PgError):
                call()
        assert (c.down(c.ix, totals) == FILL).all() and (c.words() == before).all()
        assert (c.words(cut) == before).all()
        assert c.pop_call(1, 1, BOUND, BOUND, totals) == 0 and int(c.down(c.ix, totals)[0]) == 1       # (the bounds themselves are taken)
    finally:
        cut.close()
        c.close()


DESIGNS = [check_substitution, check_ties, check_three_siblings, check_unequal, check_shared_junction, check_nested, check_tip_on_arm,
           check_kept, check_tombstone, check_empty, check_many_bubbles, check_many_more_bubbles, check_noisy]
