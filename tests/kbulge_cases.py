"""The cases of bubble popping on strongest paths, shared by tests/test_kbulge_host.py (the host twin) and tests/test_gpu_kbulge.py (the
kernels): designed read sets turned into records with the builders of tests/kbubble_cases.py, popped a round at a time through
pg_kindex_pop_bulges, and after every round compared exactly with the model (tests/kbulge_model.py, which asserts the survival of every
strongest path it used) and with what the construction dictates: the four totals, and the word of EVERY key of the original set read
back with query_ragged.  twin: a second index of the same records (the host twin beside a device index) is popped in step, and the two
must agree word for word.  All comparisons are of integers and exact."""
import functools

import numpy as np
import pytest

import kbubble_cases as BC
import kbubble_model as B
import kbulge_model as S
import kindex_model as M
import ktip_cases as TC
import ktip_model as T
import kunitig_cases as G
import kwalk_cases as E
from karc_cases import ALL_OPS, Editor, model_simplify
from kbubble_cases import arm_keys, arm_read, cleared_by, flanks, other, path, plain, without
from ktip_cases import canon, node
from kwalk_cases import count, rc, records_of, tile
from soapdenovo2_amd import api

FLAVOURS = BC.FLAVOURS
flavour_id = BC.flavour_id
FILL, EINVAL, ESTATE, BOUND = BC.FILL, BC.EINVAL, BC.ESTATE, BC.BOUND
D = T.DEAD_END


def check_substitution(K, mer127, device, twin=None):
    """A plain substitution bubble, the reads as they are and reverse complemented: the round's totals, removed keys and cleared counters
    are pop_bubbles', and every word equals that of a second index popped by pop_bubbles."""
    nw = 4 if mer127 else 2
    g, p = BC.path_with_junctions(K, True, False)
    var = other(g, p)
    what = "substitution " + flavour_id((K, mer127))
    main, minor = tile(g, K), arm_read(var, p, K)
    n_path = len(g) - K + 1
    for recs in (records_of(*count([(main, 5), ([minor], 1)], K), nw), records_of(*count([([rc(r) for r in main], 5), ([rc(minor)], 1)], K), nw)):
        c = Editor(recs, K, mer127, device, twin)
        simple = api.KmerIndex.from_records(recs, K, mer127, device)
        try:
            assert c.bulge(1, 1, K - 1, 0, what)[0] == [0, 0, n_path + K, 0], what
            totals, removed, cleared = c.bulge(1, 1, K, 0, what)
            assert totals == [1, K, n_path + K, 1] and removed == set(arm_keys(var, p, K)) and sorted(cleared) == cleared_by(g, p, K, var[p]), what
            assert [int(v) for v in simple.pop_bubbles(1, 1, K, max_rounds=1)[0]] == totals and (c.words(simple) == c.words()).all(), what
            assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
            assert c.bulge(1, 1, K, 0, what)[0] == [0, 0, n_path, 0], what
        finally:
            simple.close()
            c.close()


def check_overlapping(K, mer127, device, twin=None):
    """Two errors less than K apart on different reads: arms u1 -> v1 and u2 -> v2 with u1 < u2 < v1 < v2 along the path, so neither arm's
    alternative is a simple unitig.  A pop_bubbles round pops 0 and keeps them; one pop_bulges round pops both, and the unitigs are
    then the path alone."""
    nw = 4 if mer127 else 2
    what = "two errors less than K apart " + flavour_id((K, mer127))
    g, p = path(K, 7500 + K, 1, None, 12)
    q = p + 11
    a, b = other(g, p), other(g, q)
    reads = [(tile(g, K), 5), ([arm_read(a, p, K)], 1), ([arm_read(b, q, K)], 1)]
    n_path = len(g) - K + 1
    assert E.distinct_kmers([g, reads[1][0][0], reads[2][0][0]], K) == n_path + 2 * K
    c = Editor(records_of(*count(reads, K), nw), K, mer127, device, twin)
    try:
        solid = n_path + 2 * K
        totals, removed, _ = c.pop(1, 1, 2 * K, 0, what)
        assert totals[:3] == [0, 0, solid] and totals[3] >= 2 and not removed, what
        totals, removed, cleared = c.bulge(1, 1, K, 0, what)
        assert totals[:3] == [2, 2 * K, solid] and removed == set(arm_keys(a, p, K) + arm_keys(b, q, K)), what
        assert sorted(cleared) == sorted(cleared_by(g, p, K, a[p]) + cleared_by(g, q, K, b[q])), what
        assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
        assert c.bulge(1, 1, K, 0, what)[0] == [0, 0, n_path, 0], what
    finally:
        c.close()


def check_ties(K, mer127, device, twin=None):
    """Two arms each read by its own reads alone.  Equal out-counters at the fork, 5 : 5 and 63 : 63 (70 reads each): no strong step, both
    kept.  2 : 1: the weaker goes.  And the arm that holds the strictly strongest arc is never popped, even with the lower mean: arm A
    read twice and its first k-mer with the fork five times more, arm B read four times -- A has the strongest arc out of the fork and B
    the strongest into the join, so no strongest path exists and both stay, where pop_bubbles pops A."""
    nw = 4 if mer127 else 2
    g, p = BC.path_with_junctions(K, False, True)
    var = other(g, p)
    solid = len(g) - K + 1 + K
    for ca, cb, want in ((5, 5, 0), (70, 70, 0), (2, 1, 1)):
        what = "arms of %d and %d %s" % (ca, cb, flavour_id((K, mer127)))
        c = Editor(records_of(*count(flanks(g, p, K, 3) + [([arm_read(g, p, K)], ca), ([arm_read(var, p, K)], cb)], K), nw), K, mer127, device, twin)
        try:
            totals, removed, _ = c.bulge(1, 1, K, 0, what)
            assert totals == [want, K * want, solid, 2 - want] and removed == (set(arm_keys(var, p, K)) if want else set()), what
        finally:
            c.close()
    what = "the strongest arc on the weaker arm " + flavour_id((K, mer127))
    groups = flanks(g, p, K, 3) + [([arm_read(g, p, K)], 2), ([g[p - K:p + 1]], 5), ([arm_read(var, p, K)], 4)]
    records = records_of(*count(groups, K), nw)
    c = Editor(records, K, mer127, device, twin)
    simple = api.KmerIndex.from_records(records, K, mer127, device)
    try:
        assert c.bulge(1, 1, K, 0, what)[0] == [0, 0, solid, 2], what
        assert [int(v) for v in simple.pop_bubbles(1, 1, K, max_rounds=1)[0]][:2] == [1, K], what
    finally:
        simple.close()
        c.close()


def check_three_arms(K, mer127, device, twin=None):
    """Three arms of one bubble, read 5, 2 and 1 times: the two weaker go in one round, two arms into one v by different bases, cleared
    by two lanes."""
    nw = 4 if mer127 else 2
    what = "three arms " + flavour_id((K, mer127))
    g, p = BC.path_with_junctions(K, True, False)
    b, c3 = other(g, p, 1), other(g, p, 2)
    c = Editor(records_of(*count([(tile(g, K), 5), ([arm_read(b, p, K)], 2), ([arm_read(c3, p, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        solid = len(g) - K + 1 + 2 * K
        totals, removed, cleared = c.bulge(1, 1, K, 0, what)
        assert totals == [2, 2 * K, solid, 1] and removed == set(arm_keys(b, p, K) + arm_keys(c3, p, K)), what
        assert len({(k, h) for k, h, _ in cleared}) == 2 and len(set(cleared)) == 4, what
        assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
    finally:
        c.close()


def check_nested(K, mer127, device, twin=None):
    """kbubble_cases.nested: a 5-read path, a 2-read copy that differs in eight bases, and a 1-read copy with another base inside that
    window -- a bubble on the outer bubble's strong arm.  The nested arm and the outer weak arm go in ONE round, where pop_bubbles needs
    two; the model's survival assertion passes."""
    what = "a bubble on an arm " + flavour_id((K, mer127))
    records, n_path = BC.nested(K, mer127)
    n_out = K + BC.W_OUTER - 1
    c = Editor(records, K, mer127, device, twin)
    try:
        rounds = c.bulge_settle(1, 1, n_out, 0, what)
        assert [r[:3] for r in rounds] == [[2, n_out + K, n_path + n_out + K], [0, 0, n_path]], what
        assert len(c.unitigs(1, 1)[0]) == 1, what
    finally:
        c.close()
    c = Editor(records, K, mer127, device)
    try:
        rounds = c.ix.pop_bulges(1, 1, n_out)
        assert [[int(v) for v in r][:2] for r in rounds] == [[2, n_out + K], [0, 0]], what
        assert api.bulge_fields(rounds[0])["arms"] == 2 and api.bulge_fields(rounds[0])["kmers"] == n_out + K, what
        bufs = [c.totals(), c.totals()]                                          # two calls back to back: both find nothing more
        for t in bufs:
            assert c.bulge_call(1, 1, n_out, 0, t) == 0
        assert [[int(v) for v in c.down(c.ix, t)] for t in bufs] == [[0, 0, n_path, 0]] * 2, what
    finally:
        c.close()


def check_unequal(K, mer127, device, twin=None):
    """An arm of K - 1 k-mers (a base left out) read once beside the path read five times: S has K k-mers, one more than n + max_diff at
    max_diff 0 -- kept --, and exactly n + max_diff at max_diff 1 -- popped."""
    nw = 4 if mer127 else 2
    what = "unequal lengths " + flavour_id((K, mer127))
    g, p = BC.path_with_junctions(K, True, True)
    short = without(g, p)
    c = Editor(records_of(*count([(tile(g, K), 5), ([arm_read(short, p, K, K - 1)], 1)], K), nw), K, mer127, device, twin)
    try:
        solid = len(g) - K + 1 + K - 1
        assert c.bulge(1, 1, K, 0, what)[0] == [0, 0, solid, 2], what            # (kept: the short arm, and the path's K k-mers beside it)
        totals, removed, _ = c.bulge(1, 1, K, 1, what)
        assert totals == [1, K - 1, solid, 1] and removed == set(arm_keys(short, p, K, K - 1)), what
        assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
    finally:
        c.close()


def check_equal_means(K, mer127, device, twin=None):
    """Equal means kept.  Arm A is read twice; arm B once by a read that reaches both junctions and once by a read of exactly its own K
    k-mers, which adds coverage and no arc to a junction.  The fork's and the join's counters are 2 : 1, so S is A and it succeeds; both
    sums are 2 K over K k-mers, cov_P m == cov_S n, and B stays."""
    nw = 4 if mer127 else 2
    what = "equal means " + flavour_id((K, mer127))
    g, p = BC.path_with_junctions(K, False, True)
    var = other(g, p)
    groups = flanks(g, p, K, 3) + [([arm_read(g, p, K)], 2), ([arm_read(var, p, K)], 1), ([var[p - K + 1:p + K]], 1)]
    c = Editor(records_of(*count(groups, K), nw), K, mer127, device, twin)
    try:
        cnt, u, v = c.model.cnt, node(g[p - K:p]), node(g[p + 1:p + K + 1])
        for arm in (g, var):
            assert [M.coverage(cnt[k]) for k in arm_keys(arm, p, K)] == [2] * K, what
        assert [T.out_counters(cnt[T.key_of(u)], T.is_fwd(u))[int(b)] for b in (g[p], var[p])] == [2, 1], what
        assert [T.key_of(s) for s in S.strongest_path(cnt, K, u, v, K, 1, 1)] == arm_keys(g, p, K), what
        totals, removed, cleared = c.bulge(1, 1, K, 0, what)
        assert totals == [0, 0, len(g) - K + 1 + K, 2] and not removed and not cleared, what
    finally:
        c.close()


def check_tie_inside(K, mer127, device, twin=None):
    """A tie at a join inside S.  check_overlapping's two arms, but the first arm's read is there as often as the path's arc into its
    join v1 was counted: v1's two in-counters are equal.  v1 lies strictly inside the second arm's strongest path, which ends there:
    the second arm is kept although its fork and its own join have strict maxima; nothing is written."""
    nw = 4 if mer127 else 2
    what = "a tie at a join inside S " + flavour_id((K, mer127))
    g, p = path(K, 7500 + K, 1, None, 12)
    q = p + 11
    a, b = other(g, p), other(g, q)
    v1, before_v1 = node(g[p + 1:p + K + 1]), node(g[p:p + K])
    u2, v2 = node(g[q - K:q]), node(g[q + 1:q + K + 1])
    cnt = M.Model.from_records(records_of(*count([(tile(g, K), 5)], K), nw), K, nw).cnt
    x = T.in_counters(cnt[T.key_of(v1)], T.is_fwd(v1))[int(g[p])]
    assert 1 < x < 63
    c = Editor(records_of(*count([(tile(g, K), 5), ([arm_read(a, p, K)], x), ([arm_read(b, q, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        cnt = c.model.cnt
        ins = T.in_counters(cnt[T.key_of(v1)], T.is_fwd(v1))
        assert ins[int(g[p])] == ins[int(a[p])] == x, what
        assert S.strong_step(cnt, K, u2, 1, 1) == node(g[q - K + 1:q + 1]) and S.strong_step(cnt, K, node(g[q:q + K]), 1, 1) == v2, what
        assert S.strong_step(cnt, K, before_v1, 1, 1) is None and S.strongest_path(cnt, K, u2, v2, K, 1, 1) is None, what
        totals, removed, cleared = c.bulge(1, 1, K, 0, what)
        assert totals[:3] == [0, 0, len(g) - K + 1 + 2 * K] and totals[3] >= 2 and not removed and not cleared, what
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def loop_at_fork(K):
    """(reads as groups, u, v, the weak arm's keys): X u B u B u Y read five times over and one read with another first base of Y.  The
    fork u has three arcs out: into the loop u -> B -> u, counted twice a pass and the strictly strongest; into Y; and into the weak
    arm, which joins Y at v = Y[1:K + 1]."""
    for seed in range(7700 + K, 7800 + K):
        r = E.random_genome(seed, 4 * K + 43)
        X, u, Y, Bs = r[:K + 20], r[K + 20:2 * K + 20], r[2 * K + 20:4 * K + 40], r[-3:]
        if Bs[0] == Y[0] or Bs[-1] == X[-1]:
            continue
        Y2 = Y.copy()
        Y2[0] = [x for x in range(4) if x not in (int(Y[0]), int(Bs[0]))][0]
        strong, weak_seq = np.concatenate([X, u, Bs, u, Bs, u, Y]), np.concatenate([X, u, Bs, u, Y2])
        at = len(X) + K + 3
        weak = weak_seq[at - 4:at + 2 * K + 4]
        n = len(X) + K + 3 + len(Y) + K                                         # (the path with one turn of the loop, and the weak arm)
        if E.distinct_kmers([strong, weak], K) == n:
            keys = [canon(weak_seq[j:j + K]) for j in range(at + 1, at + 1 + K)]
            return ((tuple(tile(strong, K)), 5), ((weak,), 1)), node(u), node(Y[1:K + 1]), keys, n
    raise AssertionError("no seed gives that loop")


def check_returns_to_fork(K, mer127, device, twin=None):
    """A strong path that returns to u before it meets v: the strictly strongest arc out of the fork leads into a loop back to the fork,
    so the weak arm beside Y has no strongest path and is kept -- where pop_bubbles, which only compares it with its sibling, pops it."""
    nw = 4 if mer127 else 2
    what = "a strong path back to the fork " + flavour_id((K, mer127))
    groups, u, v, keys, n = loop_at_fork(K)
    records = records_of(*count([(list(r), k) for r, k in groups], K), nw)
    c = Editor(records, K, mer127, device, twin)
    try:
        cnt = c.model.cnt
        x, steps = S.strong_step(cnt, K, u, 1, 1), 1
        while x is not None and T.key_of(x) != T.key_of(u):
            x, steps = S.strong_step(cnt, K, x, 1, 1), steps + 1
            assert steps <= K + 3
        assert x == u and steps == K + 3, what + ": the strong steps from u do not lead back to u"
        assert [m for _, _, m in B.branches(cnt, K, 1, 1, K) if [T.key_of(k) for k in m] == keys], what + ": the weak arm is no arm"
        assert S.strongest_path(cnt, K, u, v, K, 1, 1) is None, what
        totals, removed, cleared = c.bulge(1, 1, K, 0, what)
        assert totals[:3] == [0, 0, n] and totals[3] >= 2 and not removed and not cleared, what
        assert B.pop_round(M.Model.from_records(records, K, nw), 1, 1, K, 0)[1] == set(keys), what
    finally:
        c.close()


def check_shared_junction(K, mer127, device, twin=None):
    """A k-mer that is v of one bulge and u of the next: it loses one counter from each half."""
    nw = 4 if mer127 else 2
    what = "two bulges at one k-mer " + flavour_id((K, mer127))
    g, p = path(K, 6400 + K, 2)
    q = p + K + 1
    a, b = other(g, p), other(g, q)
    c = Editor(records_of(*count([(tile(g, K), 5), ([arm_read(a, p, K)], 1), ([arm_read(b, q, K)], 1)], K), nw), K, mer127, device, twin)
    try:
        shared = canon(g[p + 1:p + K + 1])
        totals, removed, cleared = c.bulge(1, 1, K, 0, what)
        assert totals == [2, 2 * K, len(g) - K + 1 + 2 * K, 2] and sorted(h for k, h, _ in cleared if k == shared) == [0, 1], what
        assert c.unitigs(1, 1)[0] == [G.emitted(g, D, D, K)], what
    finally:
        c.close()


def check_many_arms(K, mer127, device, twin=None):
    """257 and 513 arms on one path: the start list crosses wave and workgroup edges many times over."""
    for n in (257, 513):
        what = "%d arms %s" % (n, flavour_id((K, mer127)))
        records, n_path, sources = BC.many_bubbles(K, mer127, n)
        c = Editor(records, K, mer127, device, twin, sources)
        try:
            assert c.bulge_settle(1, 1, K, 0, what) == [[n, n * K, n_path + n * K, n], [0, 0, n_path, 0]], what
            assert len(c.unitigs(1, 1)[0]) == 1, what
        finally:
            c.close()


def check_disagreeing(K, mer127, device, twin=None):
    """Hand-made records whose arc counters disagree at their two ends -- random counters over a sixth of the words of the overlapping
    design --: no model, the device and the twin still agree word for word and in their totals, round after round."""
    nw = 4 if mer127 else 2
    what = "disagreeing counters " + flavour_id((K, mer127))
    g, p = path(K, 7500 + K, 1, None, 12)
    records = records_of(*count([(tile(g, K), 5), ([arm_read(other(g, p), p, K)], 1), ([arm_read(other(g, p + 11), p + 11, K)], 1)], K), nw).copy()
    rng = np.random.default_rng(7600 + K)
    for r in records[rng.random(len(records)) < 1 / 6]:
        r[nw] ^= np.uint64(int(rng.integers(0, 64)) << (6 * int(rng.integers(0, 4)) + 32 * int(rng.integers(0, 2))))
    c = Editor(records, K, mer127, device, twin)
    try:
        for i in range(4):
            got = []
            for ix in [c.ix] + ([c.twin] if c.twin is not None else []):
                t = c.totals(ix)
                assert c.bulge_call(1, 1, 2 * K, 1, t, ix) == 0
                got.append([int(v) for v in c.down(ix, t)])
            assert got[0] == got[-1], what
            if c.twin is not None:
                assert (c.words() == c.words(c.twin)).all(), what
    finally:
        c.close()


def check_noisy(K, mer127, device, twin=None):
    """The 2 kb genome with a repeat, read with 1 % substitutions, at 1 / 1: pop_bulges to its fixed point, each round against the
    model, then the whole simplification with all four operators; at the end the model finds no minor arm."""
    nw = 4 if mer127 else 2
    records = records_of(*count([(BC.noisy(K), 1)], K), nw)
    limit = 2 * K
    what = "noisy %s at 1 / 1" % flavour_id((K, mer127))
    c = Editor(records, K, mer127, device, twin)
    try:
        n_before = len(c.unitigs(1, 1)[0])
        first = c.bulge_settle(1, 1, limit, 0, what)
        assert first[0][0] > 0, what + ": not one arm popped"
        rounds = c.simplify_ops_by_rounds(ALL_OPS, 1, 1, limit, limit, 0, what)
        assert not S.decide(c.model.cnt, K, 1, 1, limit, 0)[0], what + ": a minor arm is left"
        n_after = len(c.unitigs(1, 1)[0])
        assert n_after <= n_before, what
        print("%s: %d -> %d unitigs, pop_bulges alone %s, then %s" % (what, n_before, n_after, first, rounds))
    finally:
        c.close()
    c = Editor(records, K, mer127, device)
    try:
        assert plain(c.ix.simplify(1, 1, ops=ALL_OPS)) == model_simplify(c.model, ALL_OPS, 1, 1, limit, limit), what
        assert (c.words() == c.want_words()).all(), what
    finally:
        c.close()


def check_empty(K, mer127, device, twin=None):
    c = Editor(np.zeros((0, (4 if mer127 else 2) + 2), dtype=np.uint64), K, mer127, device, twin)
    try:
        assert c.bulge(1, 1, K, 0, "empty")[0] == [0, 0, 0, 0]
        assert [int(v) for r in c.ix.pop_bulges(1, 1) for v in r] == [0, 0, 0, 0]
    finally:
        c.close()


def check_refusals(K, mer127, device, cut_devices):
    """Every refusal, with the pre-filled totals and every word of the table untouched."""
    records, _ = BC.nested(K, mer127)
    c = Editor(records, K, mer127, device)
    cut = api.KmerIndex.from_records(records, K, mer127, cut_devices)
    L = api.lib()
    n_out = K + BC.W_OUTER - 1
    try:
        before, totals = c.words(), c.totals()
        for bad in (dict(min_cov=0), dict(min_cov=256), dict(min_arc=0), dict(min_arc=64), dict(max_len=0), dict(max_len=BOUND + 1),
                    dict(max_diff=BOUND + 1)):
            args = dict(dict(min_cov=1, min_arc=1, max_len=n_out, max_diff=0), **bad)
            assert c.bulge_call(args["min_cov"], args["min_arc"], args["max_len"], args["max_diff"], totals) == EINVAL, bad
            assert b"min_cov is 1 to 255" in L.pg_last_error(), bad
        assert c.bulge_call(1, 1, n_out, 0, None) == EINVAL and b"out_totals" in L.pg_last_error()
        assert L.pg_kindex_pop_bulges(None, 1, 1, n_out, 0, None, None) == EINVAL
        assert L.pg_kindex_pop_bulges(cut.h, 1, 1, n_out, 0, c.ix._ptr(totals), c.ix._stream()) == ESTATE
        assert b"one lookup after the other in one table" in L.pg_last_error()
        for call in (lambda: cut.pop_bulges(1, 1), lambda: c.ix.pop_bulges(0, 1), lambda: c.ix.pop_bulges(1, 1, max_diff=BOUND + 1)):
            with pytest.raises(api.PgError):
                call()
        assert (c.down(c.ix, totals) == FILL).all() and (c.words() == before).all()
        assert (c.words(cut) == before).all()
        assert c.bulge_call(1, 1, BOUND, BOUND, totals) == 0 and int(c.down(c.ix, totals)[0]) == 2      # (the bounds themselves are taken)
    finally:
        cut.close()
        c.close()


DESIGNS = [check_substitution, check_overlapping, check_ties, check_equal_means, check_tie_inside, check_returns_to_fork, check_three_arms, check_nested, check_unequal, check_shared_junction,
           check_many_arms, check_disagreeing, check_noisy, check_empty]
