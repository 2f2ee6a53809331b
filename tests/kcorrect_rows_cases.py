"""The corrector on an index cut over ranks (pg_kindex_correct_rows: rounds over merged rows, csrc/kcorrect_rows.hpp), shared by
tests/test_kcorrect_rows_host.py (the host twin: a device list of -1s) and tests/test_gpu_kcorrect_rows.py (every rank on GPU 0).  The
cases, the tables, the packing and the model are kcorrect_cases' and kcorrect_model's; here are the corrector whose `run` calls the
rows methods, the flavour sweep of kcorrect_cases.check_flavour through it, two more designed reads, and what the round statistics must
add up to.  All comparisons are of integers and exact."""
import os

import numpy as np

import kcorrect_cases as E
import kcorrect_model as C
from soapdenovo2_amd import api

CAPACITY = "SOAPDENOVO2_AMD_KCOR_ROUND_TRIALS"
RANKS = [1, 2, 8]
RANK_FLAVOURS = [(31, False), (65, True)]


class RowsCorrector(E.Corrector):
    """kcorrect_cases.Corrector over a device tuple (all -1: the host twin's cut); batches and answers lie where the first ordinal says."""

    def __init__(self, K, mer127, devices, records=None, model=None):
        super().__init__(K, mer127, tuple(devices), records, model)
        self.devices, self.device = tuple(devices), devices[0]
        assert self.ix.sharded

    def run(self, reads, uniform=False, in_place=False, **params):
        words, off, base, ulen = E.pack(reads, self.K, self.nw, uniform)
        d_words = self.up(words.copy())
        out = d_words if in_place else None
        if uniform:
            got, rep = self.ix.correct_rows_uniform(d_words, len(reads), ulen, out=out, **params)
        else:
            got, rep = self.ix.correct_rows_ragged(d_words, self.up(off), self.up(base), len(reads), out=out, n_kmers=int(base[-1]), **params)
        if not in_place:
            assert (self.down(d_words) == words).all(), "the input batch was written to"
        return self.down(got), self.down(rep)


def edge_reads(K):
    """(an error at base 0, an error at base L - 1) of the plain read: put first and last in a batch, the one's left window lies in front
    of the batch's words and the other's right window ends in the tail."""
    by_name = {c.name: c for c in E.cases(K)}
    L = E.read_len(K)
    return by_name["error-at-0"], by_name["error-at-%d" % (L - 1)]


def check_edges(cor):
    """The two edge reads alone and as the first and the last read of a batch, ragged and uniform: the model's words, and restored."""
    first, last = edge_reads(cor.K)
    for c in (first, last):
        got, rep = E.model_correct(cor.model, c.read, c.params)
        E.designed(c, got, rep)
        assert c.outcome == "restored" and rep & 0xFF == 1
    plain = first.truth
    for uniform in (False, True):
        cor.check([first.read], "error at base 0 alone", uniform=uniform, **E.PARAMS)
        cor.check([last.read], "error at the last base alone", uniform=uniform, **E.PARAMS)
        got, _ = cor.check([first.read, plain, last.read], "edges of a batch", uniform=uniform, **E.PARAMS)
        assert (got[-(cor.nw + 1):] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "the tail came back changed"
        want = E.pack([plain, plain, plain], cor.K, cor.nw, uniform)[0]
        assert (got == want).all()


def check_flavour(K, mer127, devices):
    """What kcorrect_cases.check_flavour does, through the rows methods: every designed case alone with its own parameters, all cases as
    one ragged batch, in place, k-mer-less reads between others, batches of 1, 63, 64, 65 and 257 uniform and ragged -- and the two edge
    reads."""
    cor = RowsCorrector(K, mer127, devices)
    try:
        cs = E.cases(K)
        for c in cs:
            got, rep = E.model_correct(cor.model, c.read, c.params)
            E.designed(c, got, rep)
            cor.check([c.read], c.name, **c.params)
        reads = [c.read for c in cs]
        assert len(reads[-1]) % 32 == 0 and len(reads[0]) < K
        cor.check(reads, "all cases", **E.PARAMS)
        cor.check(reads, "all cases, in place", in_place=True, **E.PARAMS)
        none = np.zeros(K - 1, dtype=np.uint8)
        cor.check([none, reads[5], none, none, reads[6], np.zeros(0, dtype=np.uint8), reads[7], none], "k-mer-less between", **E.PARAMS)
        cor.check([none, none], "only k-mer-less", **E.PARAMS)
        assert cor.ix.correct_rows_stats()["trials"] == 0
        L = E.read_len(K)
        pool = [r for r in reads if len(r) == L]
        for n in E.BATCHES:
            batch = [pool[i % len(pool)] for i in range(n)]
            u, u_rep = cor.check(batch, "uniform %d" % n, uniform=True, **E.PARAMS)
            r, r_rep = cor.check(batch, "ragged %d" % n, **E.PARAMS)
            i, i_rep = cor.check(batch, "uniform %d, in place" % n, uniform=True, in_place=True, **E.PARAMS)
            assert (u == r).all() and (u == i).all() and (u_rep == r_rep).all() and (u_rep == i_rep).all()
        check_edges(cor)
    finally:
        cor.close()


def check_ranks(K, mer127, devices_of):
    """All cases as one batch and the edge reads over 1, 2 and 8 ranks against the model."""
    reads = [c.read for c in E.cases(K)]
    for n in RANKS:
        cor = RowsCorrector(K, mer127, devices_of(n))
        try:
            assert api.lib().pg_kindex_ranks(cor.ix.h) == n
            cor.check(reads, "%d ranks" % n, **E.PARAMS)
            L = E.read_len(K)
            cor.check([r for r in reads if len(r) == L], "%d ranks, uniform" % n, uniform=True, **E.PARAMS)
            check_edges(cor)
        finally:
            cor.close()


def stop_left_read(K):
    """test_kcorrect_host.py's STOP_LEFT read: two errors next to each other in front of the anchor."""
    read = E.cases(K)[10].truth.copy()
    read[[3, 4]] ^= 2
    return read


def trials_of(rep):
    """The trials the reports account for: every fix was an accepted trial, every stop flag a rejected one."""
    rep = np.asarray(rep, dtype=np.uint64)
    return int((rep & np.uint64(0xFF)).sum()) + int(((rep & np.uint64(C.STOP_RIGHT)) != 0).sum()) + int(((rep & np.uint64(C.STOP_LEFT)) != 0).sum())


class capacity:
    """The round's capacity through the hook, for the calls inside the block."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get(CAPACITY)
        if self.n is None:
            os.environ.pop(CAPACITY, None)
        else:
            os.environ[CAPACITY] = str(self.n)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(CAPACITY, None)
        else:
            os.environ[CAPACITY] = self.old


def check_capacities(cor, capacities):
    """A batch of every designed read of one K: the words, the reports and the trials are the same whatever a round holds; a round of
    one trial takes more rounds; the trials are the fixes and the stops."""
    K = cor.K
    reads = [c.read for c in E.cases(K)] + [stop_left_read(K)]
    with capacity(None):
        got, rep = cor.check(reads, "default capacity", **E.PARAMS)
        base = cor.ix.correct_rows_stats()
    assert base["trials"] == trials_of(rep) > 20 and base["trial_kmers"] == 3 * K * base["trials"]
    assert base["host_waits"] == base["rounds"] + 1 and 1 < base["rounds"] <= E.MAX_FIXES + 2
    assert (rep & np.uint64(C.STOP_LEFT)).any() and (rep & np.uint64(C.STOP_RIGHT)).any()
    for n in capacities:
        with capacity(n):
            g, r = cor.run(reads, **E.PARAMS)
            s = cor.ix.correct_rows_stats()
            u, u_rep = cor.run([x for x in reads if len(x) == E.read_len(K)], uniform=True, in_place=True, **E.PARAMS)
        assert (g == got).all() and (r == rep).all(), "capacity %d" % n
        assert s["trials"] == base["trials"] and s["rounds"] >= -(-base["trials"] // n) and s["host_waits"] == s["rounds"] + 1
        if n == 1:
            assert s["rounds"] == s["trials"] > base["rounds"]
        w, w_rep = cor.want([x for x in reads if len(x) == E.read_len(K)], uniform=True, **E.PARAMS)
        assert (u == w).all() and (u_rep == w_rep).all(), "capacity %d, uniform in place" % n
