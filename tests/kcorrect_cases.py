"""The read corrector's cases, shared by tests/test_kcorrect_host.py (the host twin) and tests/test_gpu_kcorrect.py (kcor_kernel): a
random genome with a fixed seed, a table holding its k-mers at a chosen coverage (and a few designed extras), reads cut from it with
designed substitutions, and the comparison of every output word and every report word with the model (tests/kcorrect_model.py).  The
expected output is always the model's; in addition every case names the outcome it was designed for, and `designed` asserts that the
model gives it -- a case that does not do what its name says fails on the CPU.  All comparisons are of integers and exact.

Batches are packed here with exactly NW + 1 words behind the last read, those words and every read's pad bits filled with ones: they
must come back as they went in."""
import functools

import numpy as np

import kcorrect_model as C
import kindex_model as M
from soapdenovo2_amd import api

FLAVOURS = [(13, False), (31, False), (63, False), (65, True), (127, True)]
GENOME = 4400
COV, MIN_COV, MAX_FIXES, MIN_RUN = 20, 3, 3, 5
PARAMS = dict(min_cov=MIN_COV, max_fixes=MAX_FIXES, min_run=MIN_RUN)
# places of the genome with designed table entries (the base on trial), far from each other and from the plain reads' places
P_TIE, P_SHORTER, P_AT_MIN, P_BELOW_MIN, P_DELETED = 800, 1400, 2000, 2600, 3200
PLAIN, PLAIN2 = 20, 3600
BATCHES = [1, 63, 64, 65, 257]
FLAGS = C.NO_KMERS | C.NO_ANCHOR | C.STOP_RIGHT | C.STOP_LEFT | C.LIMIT


def flavour_id(f):
    return "K%d_%s" % (f[0], "127mer" if f[1] else "63mer")


def rc(codes):
    return (np.asarray(codes, dtype=np.uint8)[::-1] ^ 2).astype(np.uint8)


def read_len(K):
    return max(3 * K + 7, 101)


@functools.lru_cache(maxsize=None)
def genome(K):
    return np.random.default_rng(2000 + K).integers(0, 4, size=GENOME, dtype=np.uint8)


def _holders(g, p, K, base=None):
    """The canonical k-mers of the K windows of g that hold base p (first window first), with p replaced by `base`."""
    w = g[p - K + 1:p + K].copy()
    if base is not None:
        w[K - 1] = base
    return M.canonical_kmers(w, K)


@functools.lru_cache(maxsize=None)
def table(K, mer127):
    """Records as kindex_cases._records builds them (key words, cnt = any link counters | coverage << 24 | word B << 32, ordinal): the
    genome's k-mers at coverage COV, but
      P_TIE        the k-mers of the variant (base + 1) are there too, all K of them: two bases are solid over the whole trial
      P_SHORTER    the same but for the last of them (the k-mer that starts at the base)
      P_AT_MIN     the K k-mers that hold the base have coverage exactly MIN_COV
      P_BELOW_MIN  ... exactly MIN_COV - 1
      P_DELETED    the fourth of them has the `deleted` bit"""
    nw = 4 if mer127 else 2
    g = genome(K)
    rng = np.random.default_rng(3000 + K)
    cov = dict.fromkeys(M.canonical_kmers(g, K), COV)
    assert len(cov) == GENOME - K + 1, "the genome's k-mers are distinct"
    for p, n in ((P_TIE, K), (P_SHORTER, K - 1)):
        for k in _holders(g, p, K, (int(g[p]) + 1) & 3)[:n]:
            assert k not in cov
            cov[k] = COV
    for k in _holders(g, P_AT_MIN, K):
        cov[k] = MIN_COV
    for k in _holders(g, P_BELOW_MIN, K):
        cov[k] = MIN_COV - 1
    deleted = _holders(g, P_DELETED, K)[3]
    rec = np.zeros((len(cov), nw + 2), dtype=np.uint64)
    for i, (k, c) in enumerate(cov.items()):
        rec[i, :nw] = M.words_of_key(k, nw)
        a = int(rng.integers(0, 1 << 24)) | c << 24
        b = int(rng.integers(0, 1 << 32)) & ~(1 << 25) | (1 << 25 if k == deleted else 0)
        rec[i, nw] = a | b << 32
        rec[i, nw + 1] = i
    return rec


class Case:
    def __init__(self, name, read, truth, outcome, **params):
        self.name, self.read, self.truth, self.outcome = name, np.asarray(read, dtype=np.uint8), np.asarray(truth, dtype=np.uint8), outcome
        self.params = dict(PARAMS, **params)


def _with_errors(truth, positions):
    r = truth.copy()
    for i, p in enumerate(positions):
        r[p] = (r[p] + 2 + i % 2) & 3           # (never the variant base + 1 of the designed places)
    return r


@functools.lru_cache(maxsize=None)
def cases(K):
    """The designed reads.  outcome: "restored" (equal to the error-free read, no flag, as many fixes as errors), "same:<FLAG>" (comes
    back as given with that flag and no fix), or a tuple (fixes, flags, read expected)."""
    g, L = genome(K), read_len(K)
    out = []
    plain = g[PLAIN:PLAIN + L].copy()

    def one(name, truth, positions, outcome="restored", **params):
        out.append(Case(name, _with_errors(truth, positions), truth, outcome, **params))

    one("shorter-than-K", g[PLAIN:PLAIN + K - 1].copy(), [], "same:NO_KMERS")
    one("exactly-K-solid", g[PLAIN:PLAIN + K].copy(), [], "restored")
    one("exactly-K-weak", g[PLAIN:PLAIN + K].copy(), [K // 2], "same:NO_ANCHOR")
    one("K+1-error-first", g[PLAIN:PLAIN + K + 1].copy(), [0])
    one("K+1-error-last", g[PLAIN:PLAIN + K + 1].copy(), [K])
    for p in sorted({0, 1, K - 2, K - 1, K, L - K - 1, L - K, L - 2, L - 1}):
        one("error-at-%d" % p, plain, [p])
    for p in (31, 32, 63, 64):
        one("seam-%d" % p, g[PLAIN2:PLAIN2 + L].copy(), [p])
    for d in sorted({1, MIN_RUN - 1, MIN_RUN, K - 1, K, K + 1}):
        one("two-errors-%d-apart" % d, plain, [K + 5, K + 5 + d], "restored" if d >= MIN_RUN else "same:STOP_RIGHT")
    far = (L - K - 2) // (MAX_FIXES + 1)
    assert far >= MIN_RUN
    at = [K + 1 + i * far for i in range(MAX_FIXES + 1)]
    limited = _with_errors(plain, at)
    # (the first MAX_FIXES are fixed; the last one stays)
    out.append(Case("limit", limited, plain, (MAX_FIXES, C.LIMIT, np.where(np.arange(L) == at[-1], limited, plain).astype(np.uint8))))
    one("max-fixes-0", plain, [K + 5], "same:LIMIT", max_fixes=0)
    for name, p, outcome in (("tie", P_TIE, "same:STOP_RIGHT"), ("tie-one-shorter", P_SHORTER, "restored"), ("coverage-at-min", P_AT_MIN, "restored"),
                             ("coverage-below-min", P_BELOW_MIN, "same:STOP_RIGHT"), ("deleted-in-trial", P_DELETED, "same:STOP_RIGHT")):
        one(name, g[p - K - 5:p - K - 5 + L].copy(), [K + 5], outcome)
    out.append(Case("foreign", np.random.default_rng(9).integers(0, 4, size=L, dtype=np.uint8), plain, "same:NO_ANCHOR"))
    one("error-free", plain, [], "restored")
    out.append(Case("reverse-complement", rc(_with_errors(plain, [K + 3])), rc(plain), "restored"))
    m = (L + 31) // 32
    one("32m-bases-error-last", g[PLAIN2:PLAIN2 + 32 * m].copy(), [32 * m - 1])
    return out


_model_cache = {}


@functools.lru_cache(maxsize=None)
def model_of(K, mer127):
    return M.Model.from_records(table(K, mer127), K, 4 if mer127 else 2)


def model_correct(model, read, params):
    key = (model.K, model.nw, id(model), bytes(np.asarray(read, dtype=np.uint8)), tuple(sorted(params.items())))
    if key not in _model_cache:
        got, rep = C.correct(model, read, **params)
        _model_cache[key] = (np.array(got, dtype=np.uint8), rep)
    return _model_cache[key]


def designed(case, got, rep):
    """The model's answer for a case is the outcome the case was built for."""
    errors = int((case.read != case.truth).sum()) if len(case.read) == len(case.truth) else 0
    if case.outcome == "restored":
        assert (got == case.truth).all() and rep & FLAGS == 0 and rep & 0xFF == errors, case.name
        assert (errors == 0) == (rep == 0), case.name
    elif isinstance(case.outcome, str):
        flag = getattr(C, case.outcome.split(":")[1])
        assert (got == case.read).all() and rep & FLAGS == flag and rep & 0xFF == 0, case.name
        assert flag == C.NO_KMERS or rep >> 32 > 0, case.name
    else:
        fixes, flags, want = case.outcome
        assert (got == want).all() and rep & FLAGS == flags and rep & 0xFF == fixes, case.name


# ---- batches ----
def pack(reads, K, nw, uniform):
    """(words, word_off, kmer_base, uniform_len): the batch with exactly nw + 1 words behind the last read; those and every read's
    pad bits are ones.  uniform: every read has the same length and word_off / kmer_base are None."""
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    wpr = (lens + 31) // 32
    off = np.concatenate([[0], np.cumsum(wpr)]).astype(np.uint64)
    words = np.zeros(int(off[-1]) + nw + 1, dtype=np.uint64)
    words[int(off[-1]):] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for i, r in enumerate(reads):
        for q in range(int(wpr[i])):
            w = 0
            for c in r[32 * q:32 * q + 32]:
                w = w << 2 | int(c)
            n = len(r[32 * q:32 * q + 32])
            words[int(off[i]) + q] = (w << (64 - 2 * n)) | ((1 << (64 - 2 * n)) - 1)
    if uniform:
        assert len(set(lens.tolist())) == 1
        return words, None, None, int(lens[0])
    base = np.concatenate([[0], np.cumsum(np.maximum(lens - K + 1, 0))]).astype(np.uint64)
    return words, off[:-1].copy(), base, 0


class Corrector:
    """An index under test with its model: device = -1 the host twin over numpy, else the device build over torch tensors."""

    def __init__(self, K, mer127, device, records=None, model=None):
        self.K, self.mer127, self.device, self.nw = K, mer127, device, 4 if mer127 else 2
        self.model = model or (model_of(K, mer127) if records is None else M.Model.from_records(records, K, self.nw))
        self.ix = api.KmerIndex.from_records(table(K, mer127) if records is None else records, K, mer127, device)

    def close(self):
        self.ix.close()

    def up(self, a):
        if a is None or self.device < 0:
            return a
        import torch
        return torch.from_numpy(a.view(np.int64)).to("cuda:%d" % self.device)

    def down(self, a):
        return a if self.device < 0 else a.cpu().numpy().view(np.uint64)

    def run(self, reads, uniform=False, in_place=False, **params):
        """(output words, report) of one batch as numpy arrays."""
        words, off, base, ulen = pack(reads, self.K, self.nw, uniform)
        d_words = self.up(words.copy())
        out = d_words if in_place else None
        if uniform:
            got, rep = self.ix.correct_uniform(d_words, len(reads), ulen, out=out, **params)
        else:
            got, rep = self.ix.correct_ragged(d_words, self.up(off), self.up(base), len(reads), out=out, **params)
        if not in_place:
            assert (self.down(d_words) == words).all(), "the input batch was written to"
        return self.down(got), self.down(rep)

    def want(self, reads, uniform=False, **params):
        fixed = [model_correct(self.model, r, params) for r in reads]
        return pack([f[0] for f in fixed], self.K, self.nw, uniform)[0], np.array([f[1] for f in fixed], dtype=np.uint64)

    def check(self, reads, what, uniform=False, in_place=False, **params):
        got, rep = self.run(reads, uniform, in_place, **params)
        w_got, w_rep = self.want(reads, uniform, **params)
        assert rep.shape == w_rep.shape and (rep == w_rep).all(), "%s: reports differ from the model" % what
        assert got.shape == w_got.shape and (got == w_got).all(), "%s: output words differ from the model" % what
        return got, rep


def check_flavour(K, mer127, device):
    """Every designed case, alone and in batches, against the model."""
    cor = Corrector(K, mer127, device)
    try:
        cs = cases(K)
        for c in cs:                                            # every case as a batch of one, with its own parameters
            got, rep = model_correct(cor.model, c.read, c.params)
            designed(c, got, rep)
            cor.check([c.read], c.name, **c.params)
        # all of them in one ragged batch (reads without k-mers between others; the last read is the one of 32 m bases)
        reads = [c.read for c in cs]
        assert len(reads[-1]) % 32 == 0 and len(reads[0]) < K
        cor.check(reads, "all cases", **PARAMS)
        cor.check(reads, "all cases, in place", in_place=True, **PARAMS)
        none = np.zeros(K - 1, dtype=np.uint8)
        cor.check([none, reads[5], none, none, reads[6], np.zeros(0, dtype=np.uint8), reads[7], none], "k-mer-less between", **PARAMS)
        cor.check([none, none], "only k-mer-less", **PARAMS)
        # batches of the reads of one length, uniform and ragged, in place and not: the same words
        L = read_len(K)
        pool = [r for r in reads if len(r) == L]
        for n in BATCHES:
            batch = [pool[i % len(pool)] for i in range(n)]
            u, u_rep = cor.check(batch, "uniform %d" % n, uniform=True, **PARAMS)
            r, r_rep = cor.check(batch, "ragged %d" % n, **PARAMS)
            i, i_rep = cor.check(batch, "uniform %d, in place" % n, uniform=True, in_place=True, **PARAMS)
            assert (u == r).all() and (u == i).all() and (u_rep == r_rep).all() and (u_rep == i_rep).all()
    finally:
        cor.close()


# ---- the simulated set: a circular genome, reads from both strands, every base substituted with probability SIM_ERR ----
SIM_K, SIM_GENOME, SIM_LEN, SIM_READS, SIM_ERR, SIM_SEED, SIM_MIN_COV = 31, 3000, 100, 900, 0.005, 11, 3


@functools.lru_cache(maxsize=None)
def simulated():
    """(reads with errors, the error-free reads): (900, 100) uint8 each, about 30x."""
    rng = np.random.default_rng(SIM_SEED)
    g = rng.integers(0, 4, size=SIM_GENOME, dtype=np.uint8)
    starts = rng.integers(0, SIM_GENOME, size=SIM_READS)
    truth = g[(starts[:, None] + np.arange(SIM_LEN)[None, :]) % SIM_GENOME]
    flip = rng.random(SIM_READS) < 0.5
    truth = np.where(flip[:, None], (truth[:, ::-1] ^ 2), truth).astype(np.uint8)
    hit = rng.random(truth.shape) < SIM_ERR
    reads = np.where(hit, (truth + rng.integers(1, 4, size=truth.shape)) & 3, truth).astype(np.uint8)
    return np.ascontiguousarray(reads), np.ascontiguousarray(truth)


def simulated_model_output(model):
    """The model's corrected reads and reports for the simulated set, with api's default max_fixes and min_run."""
    reads, _ = simulated()
    fixed = [model_correct(model, r, dict(min_cov=SIM_MIN_COV, max_fixes=api.CORRECT_MAX_FIXES, min_run=api.CORRECT_MIN_RUN)) for r in reads]
    return np.stack([f[0] for f in fixed]), np.array([f[1] for f in fixed], dtype=np.uint64)
