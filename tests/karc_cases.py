"""The cases of the dropping of arcs to weak k-mers, shared by tests/test_karc_host.py (the host twin) and tests/test_gpu_karc.py (the
kernels): designed read sets turned into records with the builders of tests/kwalk_cases.py, tests/ktip_cases.py and
tests/kbubble_cases.py, edited a round at a time through pg_kindex_drop_weak_arcs, and after every round compared exactly with the model
(tests/karc_model.py) and with what the construction dictates: the four totals, and the word of EVERY key of the original set read back
with query_ragged -- a pruned side's word differs in exactly the counters the round cleared, every other word is bit-identical.  twin: a
second index of the same records (the host twin beside a device index) is edited in step, and the two must agree word for word.  All
comparisons are of integers and exact.

Editor is kbubble_cases.Bubbler with a round of the arcs and a round of the bulges (tests/kbulge_cases.py uses it too) and with
KmerIndex.simplify's order of calls for any ops, one ABI round at a time."""
import numpy as np
import pytest

import karc_model as A
import kbubble_cases as BC
import kbubble_model as B
import kbulge_model as S
import kindex_cases as KC
import kindex_model as M
import ktip_cases as TC
import ktip_model as T
import kunitig_cases as G
import kwalk_cases as E
from kbubble_cases import arm_keys, arm_read, other, path, plain
from ktip_cases import branch_keys, branch_read, canon, node
from kwalk_cases import codes, count, rc, records_of, tile
from soapdenovo2_amd import api

FLAVOURS = TC.FLAVOURS
flavour_id = KC.flavour_id
FILL = E.FILL
EINVAL, ESTATE = E.EINVAL, E.ESTATE
D, BO, WN, BI = T.DEAD_END, T.BRANCH_OUT, T.WEAK_NEXT, T.BRANCH_IN
ALL_OPS = ("arcs", "tips", "bubbles", "bulges")


class Editor(BC.Bubbler):
    """kbubble_cases.Bubbler with a round of arcs and a round of bulges beside the rounds of tips and bubbles."""

    def drop_call(self, min_cov, min_arc, totals, ix=None):
        ix = ix or self.ix
        return api.lib().pg_kindex_drop_weak_arcs(ix.h, min_cov, min_arc, ix._ptr(totals), ix._stream())

    def drop(self, min_cov, min_arc, what=""):
        """One round of arcs, as Clipper._round returns it."""
        return self._round(self.drop_call, A.drop_round, (min_cov, min_arc), what)

    def drop_settle(self, min_cov, min_arc, what=""):
        return self._settle(lambda w: self.drop(min_cov, min_arc, w), what)

    def bulge_call(self, min_cov, min_arc, max_len, max_diff, totals, ix=None):
        ix = ix or self.ix
        return api.lib().pg_kindex_pop_bulges(ix.h, min_cov, min_arc, max_len, max_diff, ix._ptr(totals), ix._stream())

    def bulge(self, min_cov, min_arc, max_len, max_diff=0, what=""):
        """One round of bulges, as Clipper._round returns it."""
        return self._round(self.bulge_call, S.bulge_round, (min_cov, min_arc, max_len, max_diff), what)

    def bulge_settle(self, min_cov, min_arc, max_len, max_diff=0, what=""):
        return self._settle(lambda w: self.bulge(min_cov, min_arc, max_len, max_diff, w), what)

    def simplify_ops_by_rounds(self, ops, min_cov, min_arc, max_tip, max_len, max_diff=0, what=""):
        """KmerIndex.simplify's order of calls for `ops` made one ABI round at a time, each compared: the list of (name, totals)."""
        one = {"arcs": lambda tag: self.drop(min_cov, min_arc, tag), "tips": lambda tag: self.round(min_cov, min_arc, max_tip, tag),
               "bubbles": lambda tag: self.pop(min_cov, min_arc, max_len, max_diff, tag), "bulges": lambda tag: self.bulge(min_cov, min_arc, max_len, max_diff, tag)}
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


def model_simplify(model, ops, min_cov, min_arc, max_tip, max_len, max_diff=0, max_rounds=64):
    """KmerIndex.simplify(ops=ops) as its documentation states it, on the model."""
    one = {"arcs": lambda: A.drop_round(model, min_cov, min_arc)[0], "tips": lambda: T.clip_round(model, min_cov, min_arc, max_tip)[0],
           "bubbles": lambda: B.pop_round(model, min_cov, min_arc, max_len, max_diff)[0], "bulges": lambda: S.bulge_round(model, min_cov, min_arc, max_len, max_diff)[0]}
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


def out_cleared(r, b):
    """(key, half, counter) of the out-counter of the oriented k-mer r for base b."""
    return (T.key_of(r),) + ((1, int(b)) if T.is_fwd(r) else (0, int(b) ^ 2))


def reasons_of(c, min_cov, min_arc):
    return sorted(tuple(sorted((l, r))) for _, l, r in c.unitigs(min_cov, min_arc)[0])


# ---- the designs ----
def check_substitution(K, mer127, device, twin=None):
    """A 5-read path and one single-copy read that carries a substitution, at min_cov 2 and min_arc 1: the arm's K k-mers are weak, the
    fork u and the join v each keep an arc to them.  Three unitigs before, one after; 2 sides pruned, 2 arcs cleared; only u's and v's
    words differ, by one counter each, and the weak k-mers' words are untouched; the reads reverse complemented; a second round finds
    nothing.  At min_arc 2 the arcs' counters, 1, are min_arc - 1: not arcs, and untouched."""
    nw = 4 if mer127 else 2
    for l_fwd, v_fwd in ((True, False), (False, True)):
        g, p = BC.path_with_junctions(K, l_fwd, v_fwd)
        var = other(g, p)
        what = "substitution, L %s, %s" % ("canonical" if l_fwd else "not", flavour_id((K, mer127)))
        main, minor = tile(g, K), arm_read(var, p, K)
        records = records_of(*count([(main, 5), ([minor], 1)], K), nw)
        swapped = records_of(*count([([rc(r) for r in main], 5), ([rc(minor)], 1)], K), nw)
        n_path, arm = len(g) - K + 1, arm_keys(var, p, K)
        u, rv = node(g[p - K:p]), node(rc(g[p + 1:p + K + 1]))
        for recs in (records, swapped):
            c = Editor(recs, K, mer127, device, twin)
            try:
                assert c.drop(2, 2, what)[0] == [0, 0, n_path, 0], what
                assert len(c.unitigs(2, 1)[0]) == 3, what
                before = dict(c.model.cnt)
                totals, removed, cleared = c.drop(2, 1, what)
                assert totals == [2, 2, n_path, 0] and not removed, what
                assert sorted(cleared) == sorted([out_cleared(u, var[p]), out_cleared(rv, int(var[p]) ^ 2)]), what
                assert all(c.model.cnt[k] == before[k] != 0 for k in arm), what
                assert c.unitigs(2, 1)[0] == [G.emitted(g, D, D, K)], what
                assert c.drop(2, 1, what)[0] == [0, 0, n_path, 0], what
            finally:
                c.close()


def check_targets(K, mer127, device, twin=None):
    """The three kinds of target that is not solid.  No record at all: a path's middle k-mer with a hand-edited counter.  The deleted
    bit: the k-mer before the deleted one and the k-mer behind it each have WEAK_NEXT towards it, and DEAD_END afterwards -- the walk from
    the k-mer before it ends with weak_next, then with dead_end.  A tombstone left by clip_tips: a tip's strong half clipped at min_cov 2,
    and at min_cov 1 its far half still points at the clipped k-mer."""
    nw = 4 if mer127 else 2
    P, SA, SB, _ = TC.fork_with_junction(K, True)
    g1, nP = np.concatenate([P, SA]), len(P)
    what = "no record " + flavour_id((K, mer127))
    records = records_of(*count([(tile(g1, K), 3)], K), nw)
    x = node(g1[50:50 + K])
    b = (int(g1[50 + K]) + 1) & 3
    for r in records:
        if M.key_of_record(r, nw) == T.key_of(x):
            r[nw] |= np.uint64(7 << (32 * out_cleared(x, b)[1] + 6 * out_cleared(x, b)[2]))
    c = Editor(records, K, mer127, device, twin)
    try:
        n_path = len(g1) - K + 1
        assert T.side(c.model.cnt, K, x, 1, 1)[0] == BO, what
        totals, _, cleared = c.drop(1, 1, what)
        assert totals == [1, 1, n_path, 0] and cleared == [out_cleared(x, b)], what
        assert c.unitigs(1, 1)[0] == [G.emitted(g1, D, D, K)], what
        assert c.drop(1, 1, what)[0] == [0, 0, n_path, 0], what
    finally:
        c.close()
    what = "the deleted bit " + flavour_id((K, mer127))
    n = 5
    keys = branch_keys(P, SB, n + 3, K)
    occ, arcs = count([(tile(g1, K), 5), ([branch_read(P, SB, n + 3, K)], 1)], K)
    c = Editor(records_of(occ, arcs, nw, deleted={keys[n]}), K, mer127, device, twin)
    try:
        g2 = np.concatenate([P, SB])
        last, after = node(g2[nP + n - K:nP + n]), node(rc(g2[nP + n + 2 - K:nP + n + 2]))
        assert T.side(c.model.cnt, K, last, 1, 1)[0] == WN and T.side(c.model.cnt, K, after, 1, 1)[0] == WN, what
        seed = [g2[nP + n - K:nP + n]]
        assert api.extend_seqs(seed, c.ix, 1, 1)[1]["reason"][0] == "weak_next", what
        solid = len(g1) - K + 1 + n + 2
        totals, _, cleared = c.drop(1, 1, what)
        assert totals == [2, 2, solid, 1] and sorted(cleared) == sorted([out_cleared(last, g2[nP + n]), out_cleared(after, int(g2[nP + n + 1 - K]) ^ 2)]), what
        assert T.side(c.model.cnt, K, last, 1, 1)[0] == D and T.side(c.model.cnt, K, after, 1, 1)[0] == D, what
        assert api.extend_seqs(seed, c.ix, 1, 1)[1]["reason"][0] == "dead_end", what
        assert c.drop(1, 1, what)[0] == [0, 0, solid, 1], what
    finally:
        c.close()
    what = "a tombstone " + flavour_id((K, mer127))
    c = Editor(records_of(*count([(tile(g1, K), 5), ([branch_read(P, SB, n, K)], 2), ([branch_read(P, SB, n + 6, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        solid = len(g1) - K + 1 + n
        assert c.round(2, 1, TC.MAX_TIP, what)[0] == [1, n, solid, 0], what
        far = node(rc(g2[nP + n + 1 - K:nP + n + 1]))                            # the far half's first k-mer, reading back at the clipped one
        assert c.model.cnt[branch_keys(P, SB, n, K)[-1]] == 0 and T.side(c.model.cnt, K, far, 1, 1)[0] == WN, what
        totals, _, cleared = c.drop(1, 1, what)
        assert totals == [1, 1, solid - n + 6, 0] and cleared == [out_cleared(far, int(g2[nP + n - K]) ^ 2)], what
        assert c.drop(1, 1, what)[0] == [0, 0, solid - n + 6, 0], what
    finally:
        c.close()


def check_forks(K, mer127, device, twin=None):
    """A side with three arcs of which two dangle: 1 side, 2 arcs, and the side is open afterwards.  A side with four arcs that all
    dangle, DEAD_END afterwards.  A side with two solid targets: kept.  Counters of 63 at min_arc 63 and min_cov 255."""
    nw = 4 if mer127 else 2
    P, SA, SB, SC = TC.fork_with_junction(K, False)
    SD = SA.copy()
    SD[0] = (int(SA[0]) + 3) & 3
    g1, p = np.concatenate([P, SA]), node(P[-K:])
    what = "three arcs, two dangle " + flavour_id((K, mer127))
    c = Editor(records_of(*count([(tile(g1, K), 5), ([branch_read(P, SB, 3, K)], 1), ([branch_read(P, SC, 3, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        n_path = len(g1) - K + 1
        totals, _, cleared = c.drop(2, 1, what)
        assert totals == [1, 2, n_path, 0] and sorted(cleared) == sorted([out_cleared(p, SB[0]), out_cleared(p, SC[0])]), what
        assert len({(k, h) for k, h, _ in cleared}) == 1, what
        assert c.unitigs(2, 1)[0] == [G.emitted(g1, D, D, K)], what
    finally:
        c.close()
    what = "four arcs, all dangle " + flavour_id((K, mer127))
    c = Editor(records_of(*count([(tile(P, K), 5)] + [([branch_read(P, Sx, 1, K)], 1) for Sx in (SA, SB, SC, SD)], K), nw), K, mer127, device, twin)
    try:
        n_path = len(P) - K + 1
        assert T.side(c.model.cnt, K, p, 2, 1)[0] == BO, what
        totals, _, cleared = c.drop(2, 1, what)
        assert totals == [1, 4, n_path, 0] and sorted(cleared) == sorted(out_cleared(p, b) for b in range(4)), what
        assert T.side(c.model.cnt, K, p, 2, 1)[0] == D and c.unitigs(2, 1)[0] == [G.emitted(P, D, D, K)], what
    finally:
        c.close()
    what = "two solid targets " + flavour_id((K, mer127))
    c = Editor(records_of(*count([(tile(g1, K), 3), (tile(np.concatenate([P, SB]), K), 3)], K), nw), K, mer127, device, twin)
    try:
        totals, removed, cleared = c.drop(1, 1, what)
        assert totals == [0, 0, len(P) - K + 1 + 2 * (K + 40), 1] and not cleared, what
    finally:
        c.close()
    what = "counters of 63 " + flavour_id((K, mer127))
    g, q = path(K, 7300 + K)
    var = other(g, q)
    c = Editor(records_of(*count([(tile(g, K), 300), ([arm_read(var, q, K)], 70)], K), nw), K, mer127, device, twin)
    try:
        u = node(g[q - K:q])
        assert T.out_counters(c.model.cnt[T.key_of(u)], T.is_fwd(u))[int(var[q])] == 63, what
        n_path = len(g) - K + 1
        assert c.drop(255, 63, what)[0] == [2, 2, n_path, 0], what
        assert c.unitigs(255, 63)[0] == [G.emitted(g, D, D, K)], what
    finally:
        c.close()


def check_both_sides(K, mer127, device, twin=None):
    """One solid k-mer between two weak ones: both of its sides are pruned in one round, so two lanes write the two halves of one word."""
    nw = 4 if mer127 else 2
    what = "both sides of one k-mer " + flavour_id((K, mer127))
    g = E.random_genome(7400 + K, K + 2)
    c = Editor(records_of(*count([([g], 1), ([g[1:K + 1]], 3)], K), nw), K, mer127, device, twin)
    try:
        totals, _, cleared = c.drop(2, 1, what)
        assert totals == [2, 2, 1, 0] and {k for k, _, _ in cleared} == {canon(g[1:K + 1])} and sorted(h for _, h, _ in cleared) == [0, 1], what
        assert reasons_of(c, 2, 1) == [(D, D)], what
    finally:
        c.close()


def check_many_sides(K, mer127, device, twin=None):
    """257 and 513 pruned sides on one path, in tables of more slots than a workgroup has lanes: the start list crosses wave and workgroup
    edges.  ktip_cases' path with a one-k-mer wrong read every third k-mer, at min_cov 2: every wrong k-mer is weak."""
    for n in (257, 513):
        what = "%d sides %s" % (n, flavour_id((K, mer127)))
        records, n_path = TC.many_tips(K, mer127, n)
        assert M.table_slots(len(records)) > 256
        c = Editor(records, K, mer127, device, twin)
        try:
            assert c.drop_settle(2, 1, what) == [[n, n, n_path, 0], [0, 0, n_path, 0]], what
            assert len(c.unitigs(2, 1)[0]) == 1, what
        finally:
            c.close()


def check_tombstone(K, mer127, device, twin=None):
    """kindex_cases' colliding keys, and in every group of keys with one home slot the middle one clipped as a one-k-mer tip first
    (ktip_cases.check_tombstone's construction): its slot stays taken in the middle of the probe run.  A new record beside each group
    holds two arcs: one to the group's LAST key, solid and found behind the tombstone, and one to a k-mer that has no record.  One arc a
    fork is cleared and the arc to the key behind the tombstone stays; each tip's junction loses its other arc, which never had a k-mer."""
    nw = 4 if mer127 else 2
    what = "tombstones " + flavour_id((K, mer127))
    _, keys = KC.table("colliding", K, mer127)
    have, word, groups = set(keys), {k: 9 << 24 for k in keys}, {}
    for k in keys:
        groups.setdefault(M.home_slot(k, nw, 3000), []).append(k)
    tips, extra, forks = [], [], []
    for g in [g for g in groups.values() if len(g) >= 3][:64]:
        k, last = g[len(g) // 2], g[-1]
        x = T.node_of_key(k, K)
        y = T.step(x, 0, K)
        jk, a = T.key_of(y), T.first_base(x, K)
        r = T.flip(T.step(T.flip(T.node_of_key(last, K)), 0, K))               # a k-mer with an arc to the group's last key
        bl = last & 3
        gone = T.key_of(T.step(r, bl ^ 1, K))
        if jk in have or T.key_of(r) in have | {jk} or gone in have | {jk, T.key_of(r)}:
            continue
        have |= {jk, T.key_of(r)}
        word[k] |= 1 << 32
        o = a ^ 1
        word[jk] = 9 << 24 | (1 << 6 * a | 5 << 6 * o if T.is_fwd(y) else (1 << 6 * (a ^ 2) | 5 << 6 * (o ^ 2)) << 32)
        word[T.key_of(r)] = 9 << 24 | sum(5 << (32 * h + 6 * i) for _, h, i in (out_cleared(r, bl), out_cleared(r, bl ^ 1)))
        tips.append(k)
        extra += [jk, T.key_of(r)]
        forks.append((r, bl, T.flip(y), o ^ 2))
    assert len(tips) >= 8 and M.table_slots(len(word)) == 8192
    records = np.zeros((len(word), nw + 2), dtype=np.uint64)
    for i, k in enumerate(list(keys) + extra):
        records[i, :nw] = M.words_of_key(k, nw)
        records[i, nw], records[i, nw + 1] = word[k], i
    c = Editor(records, K, mer127, device, twin)
    try:
        n, solid = len(tips), len(word) - len(tips)
        assert c.round(5, 1, TC.MAX_TIP, what)[0] == [n, n, len(word), 0], what
        # a side of each fork with one arc of two cleared, and each tip's junction, whose other arc never had a k-mer: WEAK_NEXT, one arc
        totals, removed, cleared = c.drop(5, 1, what)
        want = [out_cleared(r, bl ^ 1) for r, bl, _, _ in forks] + [out_cleared(j, b) for _, _, j, b in forks]
        assert totals == [2 * n, 2 * n, solid, 0] and not removed and sorted(cleared) == sorted(want), what
        for r, bl, _, _ in forks:                                                # (the arc to the key behind the tombstone stays)
            assert T.out_counters(c.model.cnt[T.key_of(r)], T.is_fwd(r))[bl] == 5, what
        assert c.drop(5, 1, what)[0] == [0, 0, solid, 0], what
    finally:
        c.close()


def check_empty(K, mer127, device, twin=None):
    c = Editor(np.zeros((0, (4 if mer127 else 2) + 2), dtype=np.uint64), K, mer127, device, twin)
    try:
        assert c.drop(1, 1, "empty")[0] == [0, 0, 0, 0]
        assert [int(v) for r in c.ix.drop_weak_arcs(1, 1) for v in r] == [0, 0, 0, 0]
        assert plain(c.ix.simplify(1, 1, ops=ALL_OPS)) == [(name, [0, 0, 0, 0]) for name in ALL_OPS]
    finally:
        c.close()


def check_back_to_back(K, mer127, device, twin=None):
    """Two ABI calls back to back on one stream with no wait between them: the first prunes, the second finds nothing; then
    KmerIndex.drop_weak_arcs, which stops by itself, and arc_fields."""
    what = "two calls back to back " + flavour_id((K, mer127))
    records, n_path = TC.many_tips(K, mer127, 257)
    c = Editor(records, K, mer127, device)
    try:
        bufs = [c.totals(), c.totals()]
        for t in bufs:
            assert c.drop_call(2, 1, t) == 0
        assert [[int(v) for v in c.down(c.ix, t)] for t in bufs] == [[257, 257, n_path, 0], [0, 0, n_path, 0]], what
        A.drop_round(c.model, 2, 1)
        assert (c.words() == c.want_words()).all(), what
    finally:
        c.close()
    c = Editor(records, K, mer127, device)
    try:
        rounds = c.ix.drop_weak_arcs(2, 1)
        assert [[int(v) for v in r] for r in rounds] == [[257, 257, n_path, 0], [0, 0, n_path, 0]], what
        assert api.arc_fields(rounds[0]) == dict(sides=257, arcs=257, solid=n_path, kept=0), what
        fresh = api.KmerIndex.from_records(records, K, mer127, device)
        try:
            assert len(fresh.drop_weak_arcs(2, 1, max_rounds=1)) == 1
            assert (c.words(fresh) == c.words()).all(), what
        finally:
            fresh.close()
    finally:
        c.close()


def check_noisy(K, mer127, device, twin=None):
    """The 2 kb genome with a repeat, read with 1 % substitutions, at 2 / 1 and 3 / 2 through simplify(ops = all four) one ABI round at a
    time, each against the model; the calls are model_simplify's; at the end the model finds no dangling arc, no minor tip, no minor
    branch and no minor arm.  Then KmerIndex.simplify(ops=...) itself, the default ops giving the calls they gave before, and a name
    that is no operator raising."""
    nw = 4 if mer127 else 2
    records = records_of(*count([(BC.noisy(K), 1)], K), nw)
    limit = 2 * K
    for min_cov, min_arc in ((2, 1), (3, 2)):
        what = "noisy %s at %d / %d" % (flavour_id((K, mer127)), min_cov, min_arc)
        c = Editor(records, K, mer127, device, twin)
        try:
            n_before = len(c.unitigs(min_cov, min_arc)[0])
            rounds = c.simplify_ops_by_rounds(ALL_OPS, min_cov, min_arc, limit, limit, 0, what)
            assert rounds == model_simplify(M.Model.from_records(records, K, nw), ALL_OPS, min_cov, min_arc, limit, limit), what
            assert sum(t[1] for name, t in rounds if name == "arcs") > 0, what + ": not one dangling arc"
            cnt = c.model.cnt
            assert not [1 for _, bases in A.sides(cnt, K, min_cov, min_arc) if bases], what + ": a dangling arc is left"
            assert not [1 for _, last, y in T.candidates(cnt, K, min_cov, min_arc, limit) if T.is_minor(cnt, K, last, y)], what + ": a minor tip is left"
            assert not B.decide(cnt, K, min_cov, min_arc, limit, 0)[0], what + ": a minor branch is left"
            assert not S.decide(cnt, K, min_cov, min_arc, limit, 0)[0], what + ": a minor arm is left"
            n_after = len(c.unitigs(min_cov, min_arc)[0])
            assert n_after <= n_before, what
            print("%s: %d -> %d unitigs, %s" % (what, n_before, n_after, rounds))
        finally:
            c.close()
    c = Editor(records, K, mer127, device)
    try:
        assert plain(c.ix.simplify(2, 1, ops=ALL_OPS)) == model_simplify(c.model, ALL_OPS, 2, 1, limit, limit), "noisy: simplify's calls are not the model's"
        assert (c.words() == c.want_words()).all()
    finally:
        c.close()
    c = Editor(records, K, mer127, device)
    try:
        assert plain(c.ix.simplify(1, 1)) == BC.model_simplify(c.model, 1, 1, limit, limit), "noisy: the default ops no longer give the calls they gave"
        assert (c.words() == c.want_words()).all()
        with pytest.raises(ValueError):
            c.ix.simplify(1, 1, ops=("tips", "islands"))
        assert (c.words() == c.want_words()).all()
    finally:
        c.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with the pre-filled totals and every word of the table untouched: the thresholds' ranges, null totals, a null
    index, an index cut over ranks."""
    records, _ = TC.many_tips(K, mer127, 257)
    c = Editor(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    try:
        before, totals = c.words(), c.totals()
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64)):
            args = dict(dict(min_cov=2, min_arc=1), **bad)
            assert c.drop_call(args["min_cov"], args["min_arc"], totals) == EINVAL and b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert c.drop_call(2, 1, None) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_drop_weak_arcs(None, 2, 1, None, None) == EINVAL
        assert L.pg_kindex_drop_weak_arcs(cut.h, 2, 1, c.ix._ptr(totals), c.ix._stream()) == ESTATE
        assert b"one lookup after the other in one table" in L.pg_last_error()
        for call in (lambda: cut.drop_weak_arcs(2, 1), lambda: cut.simplify(2, 1, ops=ALL_OPS), lambda: c.ix.drop_weak_arcs(0, 1), lambda: c.ix.drop_weak_arcs(1, 64)):
            with pytest.raises(api.PgError):
                call()
        assert (c.down(c.ix, totals) == FILL).all() and (c.words() == before).all()
        assert (c.words(cut) == before).all()
        assert c.drop_call(255, 63, totals) == 0 and int(c.down(c.ix, totals)[0]) == 0                  # (the bounds themselves are taken)
    finally:
        cut.close()
        c.close()


def simplified(min_cov, min_arc):
    """KmerCounter counts the simulated reads (a circular genome of 3 000 bases, 900 reads of 100 bases with substitutions, K = 31) ->
    finalize -> index() -> simplify(ops = all four) -> unitigs(): (the calls, the unitigs sorted, their totals, the model after the
    same calls over the counter's own records, the model's calls, the unitigs after simplify() with the default ops on a second
    index)."""
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
    default = api.KmerIndex.from_records(records, K, False, 0)
    default.simplify(min_cov, min_arc)
    before = int(default.unitigs(min_cov, min_arc).totals[0])
    default.close()
    calls = plain(ix.simplify(min_cov, min_arc, ops=ALL_OPS))
    seqs, f, totals = api.unitig_seqs(ix, min_cov, min_arc)
    ix.close()
    want = model_simplify(model, ALL_OPS, min_cov, min_arc, 2 * K, 2 * K)
    got = sorted((tuple(int(x) for x in s), int(l), int(r), int(c)) for s, l, r, c in zip(seqs, f["left_code"], f["right_code"], f["coverage_sum"]))
    return calls, got, totals, model, want, before


DESIGNS = [check_substitution, check_targets, check_forks, check_both_sides, check_many_sides, check_tombstone, check_empty, check_back_to_back,
           check_noisy]
