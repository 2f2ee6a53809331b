"""Constructed inputs for the `map` stage's edges (tests/test_map_edges.py, tests/test_gpu_map_edges.py, tests/golden/
make_map_edges_golden.py).  Every case is built from a seed: contigs with chosen names, lengths and repeats, a ContigIndex table, and
reads assembled piece by piece so that each one meets a named edge of the index or of the per-read decision.

A case is the *files' view* (contigs with names, ContigIndex rows); `loaded()` turns it into what the stage's loader hands the index
(ids, id tables), by the loader's two rules: a contig shorter than K + 2 is not indexed, and a contig's id is the number its name starts
with, else its 1-based ordinal in the file.  tests/golden/map_edges_golden.py pins both rules to the reference binary.

`write_prefix` / `write_library` write a graph prefix and a one-file FASTA library by hand (no pregraph / contig run)."""
import functools
import os

import numpy as np

import map_model as MM

KS_63 = (13, 21, 31, 33, 63)
KS_127 = (33, 63, 65, 97, 127)
FLAVOURS = [(K, False) for K in KS_63] + [(K, True) for K in KS_127]
POS24_K = 31                                           # the 2^24 case runs at one K on the 63-mer flavour (a 2 GB table)


def align_lens(K, longest):
    """The ALIGNLEN values every case runs with: K + 1, 32, 60 and one longer than every read."""
    return [K + 1, 32, 60, longest + 7]


def rc(s):
    return (np.asarray(s, dtype=np.uint8)[::-1] ^ 2).astype(np.uint8)


def cat(*parts):
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]), dtype=np.uint8)


class Case:
    def __init__(self, name, K, mer127, golden=True, all_unmapped=False, loader=True):
        self.name, self.K, self.mer127 = name, K, mer127
        self.golden = golden                           # the reference binary can run it (ids inside the table, a contig file that loads)
        self.all_unmapped = all_unmapped               # the case's purpose: no read may map
        self.loader = loader                           # ids / tables come from the loader's rules (else: set by hand, ids past the table)
        self.contigs, self.names, self.index_rows, self.reads, self.tags = [], [], [], [], []
        self.ids_by_hand = None

    def pair(self, length):
        """A ContigIndex row of a contig with a reverse-complement twin: ids n (bal 2) and n + 1 (bal 0); returns n."""
        n = self._next_id()
        self.index_rows.append((length, 1))
        return n

    def palindrome(self, length):
        """A ContigIndex row of a contig that is its own twin: one id, bal 1."""
        n = self._next_id()
        self.index_rows.append((length, 0))
        return n

    def _next_id(self):
        return 1 + sum(2 if b else 1 for _, b in self.index_rows)

    def contig(self, seq, name):
        self.contigs.append(np.ascontiguousarray(seq, dtype=np.uint8))
        self.names.append(str(name))
        return self.contigs[-1]

    def read(self, seq, tag):
        self.reads.append(np.ascontiguousarray(seq, dtype=np.uint8))
        self.tags.append(tag)

    @property
    def longest(self):
        return max([len(r) for r in self.reads] + [self.K + 2])


def id_tables(index_rows):
    """length / bal of every contig id, as the stage reads ContigIndex: n + 2 entries for n ids, unknown ids length 0, bal 1."""
    n = sum(2 if b else 1 for _, b in index_rows)
    length = np.zeros(n + 2, np.int32)
    bal = np.ones(n + 2, np.int8)
    at = 0
    for ln, b in index_rows:
        at += 1
        length[at], bal[at] = ln, b + 1
        if b:
            at += 1
            length[at], bal[at] = ln, 1 - b
    return length, bal


def loaded(case):
    """(indexed contigs, their ids, id_len, id_bal) by the loader's rules."""
    K = case.K
    ctgs, ids = [], []
    for ordinal, (seq, name) in enumerate(zip(case.contigs, case.names), 1):
        if len(seq) < K + 2:
            continue
        digits = ""
        for ch in name:
            if not ch.isdigit():
                break
            digits += ch
        num = int(digits) if digits else 0
        ctgs.append(seq)
        ids.append(num if num > 0 else ordinal)
    if case.ids_by_hand is not None:
        ids = list(case.ids_by_hand)
    length, bal = id_tables(case.index_rows)
    return ctgs, np.array(ids, dtype=np.uint32), length, bal


# ---------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------
def _fasta(path, names, seqs, width):
    with open(path, "w") as f:
        for name, s in zip(names, seqs):
            text = np.frombuffer(b"ACTG", dtype=np.uint8)[np.asarray(s, dtype=np.intp)].tobytes().decode()
            f.write(">%s\n" % name)
            for a in range(0, len(text), width):
                f.write(text[a:a + width] + "\n")
            if not text:
                f.write("\n")


def write_prefix(prefix, case):
    """<prefix>.contig / .ContigIndex / .preGraphBasic of a case."""
    _fasta(prefix + ".contig", case.names, case.contigs, 100)
    n_ids = sum(2 if b else 1 for _, b in case.index_rows)
    with open(prefix + ".ContigIndex", "w") as f:
        f.write("Edge_num %d %d\nindex\tlength\treverseComplement\n" % (n_ids, len(case.index_rows)))
        at = 1
        for ln, b in case.index_rows:
            f.write("%d\t%d\t%d\n" % (at, ln, b))
            at += 2 if b else 1
    with open(prefix + ".preGraphBasic", "w") as f:
        f.write("VERTEX %d K %d\n\nEDGEs %d\n\nMaxReadLen %d MinReadLen 0 MaxNameLen 256\n" % (len(case.contigs), case.K, n_ids, case.longest))


def write_library(d, case, map_len):
    """A FASTA library of the case's reads in one file, one line a read; returns the config's path.  The reference's `map` reads paired
    files only (its reader runs with pair = 1 and passes single-end f= / q= files by), so the file is given as p= and holds the reads in
    order, two a "pair"; with an odd number of reads one more read without k-mers ends the file.  Pairing does not touch
    readOnContig.gz: every read that maps has its line, numbered by its place in the file.  map_len = 0: the stage's default."""
    fa = os.path.join(d, "reads.fa")
    reads = list(case.reads) + ([np.zeros(1, np.uint8)] if len(case.reads) % 2 else [])
    _fasta(fa, ["r%d" % i for i in range(len(reads))], reads, 1 << 30)
    cfg = os.path.join(d, "map.cfg")
    with open(cfg, "w") as f:
        f.write("max_rd_len=%d\n[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nrank=1\n%sp=%s\n"
                % (case.longest, "map_len=%d\n" % map_len if map_len else "", fa))
    return cfg


# ---------------------------------------------------------------------------------------------------------
# pieces every case carries, so that no case passes with nothing mapped
# ---------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def _basics(case, rng, n=None):
    """Two plain contigs and reads that map '+', map '-', do not map, and carry footprint 1 / 0 (where ALIGNLEN lets two ids count)."""
    K = case.K
    n = n or 3 * K + 90
    p = case.contig(_rand(rng, n), case.pair(n))
    q_id = case.pair(n)
    q = case.contig(_rand(rng, n), q_id + 1)                       # named by the second id of its pair: bal 0
    case.read(p[5:5 + K + 30], "basic+")
    case.read(rc(q[7:7 + K + 30]), "basic-")
    case.read(_rand(rng, K + 30), "basic-unmapped")
    case.read(cat(p[3:3 + max(60, K + 4)], q[K:2 * K + 4]), "basic-footprint")      # two ids with two hits or more each
    case.read(p[:K], "basic-K-bases")                              # no k-mers by the reference's rule
    return p, q


def _decide(K, mer127, seed, far_ids=False):
    name = "decide_far" if far_ids else "decide"
    case = Case(name, K, mer127, golden=not far_ids, loader=not far_ids)
    rng = np.random.default_rng(seed)
    p, q = _basics(case, rng)
    n = 3 * K + 90
    c = []
    for i in range(14):                                            # names: first id of a pair, second id of a pair, a palindrome's id
        if i % 3 == 0:
            cid = case.pair(n)
        elif i % 3 == 1:
            cid = case.pair(n) + 1
        else:
            cid = case.palindrome(n - (i % 5))                     # (ContigIndex length differs from the sequence's: the table's is used)
        c.append(case.contig(_rand(rng, n), cid))
    two = lambda s, a=0: s[a:a + K + 1]                            # a piece with exactly two k-mers (a K + 2-base piece has three)
    piece = lambda s, hits, a=0: s[a:a + K + hits - 1]
    for m in (7, 8, 9, 12):                                        # K + 2-base pieces of m contigs: all tied, the first must win
        case.read(cat(*[c[i][4:4 + K + 2] for i in range(m)]), "ids%d-tied" % m)
        case.read(cat(*[c[i][4:4 + K + 2] for i in reversed(range(m))]), "ids%d-tied-reversed" % m)
        # the last id has one hit more than the others: it wins, and for m > 8 only a decision that counts every id sees it
        case.read(cat(*([c[i][4:4 + K + 2] for i in range(m - 1)] + [piece(c[m - 1], 4, 9)])), "ids%d-last-wins" % m)
        # ... on the '-' strand, and with enough hits for ALIGNLEN = 60
        case.read(cat(*([two(c[i], 11) for i in range(m - 1)] + [rc(piece(c[m - 1], 62, 2))])), "ids%d-last-wins-long" % m)
    # a ninth id first seen after the first eight were counted, with the first id coming back after it
    case.read(cat(*([two(c[i]) for i in range(8)] + [piece(c[8], 5, 6), piece(c[0], 3, 20)])), "ids9-then-first-again")
    # ties: first in first-hit order wins, strictly greater takes over
    a, b = c[9], c[10]
    case.read(cat(piece(a, 5, 3), piece(b, 5, 8)), "tie-a-b")
    case.read(cat(piece(b, 5, 8), piece(a, 5, 3)), "tie-b-a")
    case.read(cat(piece(a, 5, 3), piece(b, 6, 8)), "b-one-more")
    case.read(cat(rc(piece(a, 6, 3)), piece(b, 5, 8)), "a-one-more-rc")
    case.read(cat(piece(a, 5, 3), two(b), piece(a, 3, 40)), "a-split-around-b")
    # the K < 32 / K > 32 footprint rule: a second id with a single hit counts only when K > 32
    case.read(cat(piece(a, 6, 3), piece(b, 1, 8)), "footprint-single-hit-id")
    case.read(cat(piece(a, 6, 3), piece(b, 2, 8)), "footprint-two-hit-id")
    # flag == multi - 1 / multi for every ALIGNLEN the suite uses: A bases of one contig (A - K + 1 hits) against A - 1, junk after
    junk = _rand(rng, 2 * K + 70)
    for A in sorted({K + 1, 32, 60}):
        if A <= K:
            continue
        case.read(cat(c[11][2:2 + A], junk[:K + 9]), "multi-exact-A%d" % A)
        case.read(cat(c[11][2:2 + A - 1], junk[:K + 9]), "multi-less-one-A%d" % A)
        case.read(rc(cat(c[12][2:2 + A], junk[:K + 9])), "multi-exact-rc-A%d" % A)
        for ln in (A - 1, A, A + 1):                               # ALIGNLEN above / equal / below the read length
            if ln >= K + 1:
                case.read(c[13][6:6 + ln], "whole-len%d" % ln)
                e = c[13][6:6 + ln].copy()
                e[-1] ^= 1                                         # the last k-mer misses
                case.read(e, "whole-len%d-last-base-wrong" % ln)
    for ln in (K - 1, K, K + 1, K + 2):
        case.read(c[3][10:10 + ln], "len%d" % ln)
        case.read(rc(c[4][10:10 + ln]), "len%d-rc" % ln)
    # positions that come out negative: a read that hangs over the contig's end on either strand (unsigned arithmetic, then signed)
    case.read(cat(junk[:5], rc(c[5][-(K + 3):])), "negative-minus")
    case.read(cat(junk[:5], c[6][:K + 3]), "negative-plus")
    case.read(cat(junk[:9], rc(c[7][-(K + 3):])), "negative-minus-palindrome-id")
    case.read(rc(c[1][:K + 6]), "minus-at-contig-start")
    case.read(c[2][-(K + 6):], "plus-at-contig-end")
    if far_ids:                                                    # ids past the table read as length 0, bal 1 (model == product only)
        ctgs, ids, length, bal = loaded(case)
        ids = [int(x) for x in ids]
        ids[5 + 2] = len(length)
        ids[6 + 2] = len(length) + 1000
        ids[1 + 2] = (1 << 31) + 5
        case.ids_by_hand = ids
    return case


def _index(K, mer127, seed):
    case = Case("index", K, mer127)
    rng = np.random.default_rng(seed)
    _basics(case, rng)
    new = lambda n, pal=False: (case.palindrome(n) if pal else case.pair(n))
    # exactly K + 1 (not indexed) and K + 2 (indexed) bases; the K + 1 one keeps its ordinal and its ContigIndex row
    short = case.contig(_rand(rng, K + 1), new(K + 1))
    exact = case.contig(_rand(rng, K + 2), new(K + 2))
    case.read(short, "contig-K+1-whole")
    case.read(exact, "contig-K+2-whole")
    case.read(rc(exact), "contig-K+2-whole-rc")
    # a name that is not a number: the id is the ordinal in the file
    # (ordinal 5: in ContigIndex that id belongs to the K + 1-base contig above, so a '-' position shows whose length is used)
    n = 2 * K + 30
    named = case.contig(_rand(rng, n), "scaffold_x")
    case.read(named[3:3 + K + 20], "ordinal-id+")
    case.read(rc(named[5:5 + K + 20]), "ordinal-id-")
    # contigs of 63 / 64 / 65 / 128 / 129 k-mers (one stretch of the index build's 64, one and a bit, two, two and a bit)
    for nk in (63, 64, 65, 128, 129):
        s = case.contig(_rand(rng, nk + K - 1), new(nk + K - 1))
        case.read(s[-(K + 1):], "last-two-kmers-of-%d" % nk)
        case.read(rc(s[-(K + 1):]), "last-two-kmers-of-%d-rc" % nk)
    # reads that start at contig k-mer 62 .. 66, 126 .. 130: positions around the stretch starts, on both strands
    big = case.contig(_rand(rng, 200 + K - 1), new(200 + K - 1))
    for j in (0, 1, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 198):
        case.read(big[j:j + K + 1], "start-at-kmer-%d" % j)
        case.read(rc(big[j:j + K + 2]), "end-at-kmer-%d-rc" % j)
    case.read(big, "whole-contig-200-kmers")
    # a key put twice in one contig, twice in two contigs, on both strands, three times: deleted everywhere, the flanks stay
    seg = [_rand(rng, K + 5) for _ in range(4)]
    fl = lambda: _rand(rng, K + 20)
    add = lambda seq: case.contig(seq, new(len(seq)))
    d1 = add(cat(fl(), seg[0], fl(), seg[0], fl()))
    d2 = add(cat(fl(), seg[1], fl()))
    d3 = add(cat(fl(), seg[1], fl(), seg[2], fl()))
    d4 = add(cat(fl(), rc(seg[2]), fl(), seg[3], fl(), rc(seg[3]), fl(), seg[3]))
    for nm, s in (("d1", d1), ("d2", d2), ("d3", d3), ("d4", d4)):
        for a in range(0, len(s) - (K + 12), K):
            r = s[a:a + K + 12]
            case.read(r if (a // 3) % 2 else rc(r), "dup-%s-at-%d" % (nm, a))
    # 50 puts of the same keys: a tandem repeat; thousands of puts of one key: homopolymers on both strands
    unit = _rand(rng, K // 2 + 7)
    reps = max(50, 3000 // len(unit))
    tandem = add(np.tile(unit, reps))
    fifty = add(cat(fl(), np.tile(_rand(rng, K + 3), 50), fl()))
    poly_a = add(np.zeros(3000, np.uint8))
    poly_t = add(np.full(2500, 2, np.uint8))                       # the same key as poly-A's, from the other strand
    poly_c = add(np.full(2000 + K, 1, np.uint8))                   # one strand only, and still one key put 2000 times
    case.read(tandem[5:5 + 2 * K], "tandem-inside")
    case.read(fifty[:K + 20 + 2 * K], "fifty-flank-and-inside")
    case.read(rc(fifty[-(K + 28):]), "fifty-end-flank-rc")
    case.read(poly_a[:K + 9], "poly-a")
    case.read(poly_t[:K + 9], "poly-t")
    case.read(rc(poly_c[:K + 9]), "poly-g")
    return case


def _allrc(K, mer127, seed):
    """Every contig is there with its reverse complement: every key is put twice, so nothing maps."""
    case = Case("allrc", K, mer127, all_unmapped=True)
    rng = np.random.default_rng(seed)
    for i in range(3):
        n = 2 * K + 40 + i
        s = case.contig(_rand(rng, n), case.pair(n))
        case.contig(rc(s), case.pair(n))
        case.read(s[i:i + K + 30], "fwd-%d" % i)
        case.read(rc(s[i + 2:i + K + 25]), "rc-%d" % i)
    case.read(_rand(rng, K + 30), "random")
    return case


def _load(K, mer127, seed, n_kmers):
    """The table's doubling point: 512 k-mers -> 1024 slots (exactly half full), 513 -> 2048."""
    case = Case("load%d" % n_kmers, K, mer127)
    rng = np.random.default_rng(seed)
    _basics(case, rng, max(70, 2 * K + 8))
    have = MM.n_index_kmers(case.contigs, K)
    left = n_kmers - have
    assert left >= 6
    parts = [left // 3, left // 3, left - 2 * (left // 3)]
    for nk in parts:
        s = case.contig(_rand(rng, nk + K - 1), case.pair(nk + K - 1))
        for a in range(0, nk - 2, max(1, nk // 6)):
            r = s[a:a + K + 2]
            case.read(r if a % 2 else rc(r), "load-at-%d" % a)
    return case


def _wrap(K, mer127, seed):
    """A probe chain that runs off the last slot and goes on at slot 0.  Seeds are tried in order until the contigs give one (the test
    asserts it with the ported home function)."""
    nw = 4 if mer127 else 2
    for trial in range(200):
        case = Case("wrap", K, mer127)
        rng = np.random.default_rng(seed * 1000 + trial)
        _basics(case, rng)
        for _ in range(2):
            n = 60 + K
            case.contig(_rand(rng, n), case.pair(n))
        slots, where = MM.probe_slots(loaded(case)[0], K, nw)
        wrapped = [k for k, (home, slot) in where.items() if slot < home]
        if not wrapped:
            continue
        for seq in list(case.contigs):                              # reads over the wrapped keys and over keys in the last / first slots
            for j, (f, r) in enumerate(MM.kmers(seq, K)):
                key = min(f, r)
                home, slot = where[key]
                if slot < home or slot in (0, 1, slots - 1, slots - 2):
                    a = max(0, min(j - 1, len(seq) - K - 2))
                    case.read(seq[a:a + K + 2] if j % 2 else rc(seq[a:a + K + 2]), "wrap-kmer-%d" % j)
        return case
    raise AssertionError("no seed gave a wrapped chain")


def _empty(K, mer127, seed):
    case = Case("empty", K, mer127, golden=False, all_unmapped=True)
    rng = np.random.default_rng(seed)
    for ln in (K - 1, K + 1, K + 40, 3 * K):
        case.read(_rand(rng, ln), "random-%d" % ln)
    return case


def _random(K, mer127, seed, n_reads=2500):
    """On top of the constructed cases: pieces of one, two or three contigs, either strand, errors, short reads."""
    case = Case("random", K, mer127, golden=False)
    rng = np.random.default_rng(seed)
    _basics(case, rng)
    ctgs = []
    for i in range(30):
        n = int(rng.integers(K + 2, 5 * K + 40))
        s = _rand(rng, n)
        if i % 4 == 3 and n >= K + 10 and len(ctgs[i - 2]) >= K + 10:     # a stretch of another contig, on either strand
            piece = ctgs[i - 2][:K + 10]
            s[:K + 10] = piece if i % 8 == 3 else rc(piece)
        kind = i % 3
        cid = case.pair(n) if kind == 0 else (case.pair(n) + 1 if kind == 1 else case.palindrome(n))
        ctgs.append(case.contig(s, cid))
    for i in range(n_reads):
        parts = []
        for _ in range(int(rng.integers(1, 4))):
            s = ctgs[int(rng.integers(len(ctgs)))]
            a = int(rng.integers(0, len(s) - K))
            parts.append(s[a:a + int(rng.integers(K, 2 * K + 10))])
        s = cat(*parts)[:int(rng.integers(K - 2, 3 * K + 20))]
        if rng.random() < 0.5:
            s = rc(s)
        if rng.random() < 0.3:
            j = int(rng.integers(len(s)))
            s = s.copy()
            s[j] = (s[j] + 1) & 3
        case.read(s, "random-%d" % i)
    return case


def _pos24(seed):
    """A contig of 2^24 + 200 bases: positions at and past 2^24 wrap in the index's 24-bit field."""
    K = POS24_K
    case = Case("pos24", K, False)
    rng = np.random.default_rng(seed)
    p, q = _basics(case, rng)
    n = (1 << 24) + 200
    big = case.contig(_rand(rng, n), case.pair(n))
    e = 1 << 24
    for a in (0, 1000, e - 200, e - 100, e - 60, e - 31, e - 30, e - 1, e, e + 1, e + 50, e + 99):
        case.read(big[a:a + 100], "big+at-%d" % (a - e))
        case.read(rc(big[a + 1:a + 101]), "big-at-%d" % (a - e))
    case.read(cat(big[e + 20:e + 90], p[4:4 + K + 6]), "big-past-wrap-and-small")
    case.read(cat(q[4:4 + K + 6], rc(big[e + 20:e + 90])), "small-and-big-past-wrap-rc")
    return case


BUILDERS = {
    "decide": lambda K, m: _decide(K, m, 100 + K),
    "decide_far": lambda K, m: _decide(K, m, 100 + K, far_ids=True),
    "index": lambda K, m: _index(K, m, 200 + K),
    "allrc": lambda K, m: _allrc(K, m, 300 + K),
    "load512": lambda K, m: _load(K, m, 400 + K, 512),
    "load513": lambda K, m: _load(K, m, 400 + K, 513),
    "wrap": lambda K, m: _wrap(K, m, 500 + K),
    "empty": lambda K, m: _empty(K, m, 600 + K),
    "random": lambda K, m: _random(K, m, 700 + K),
}
CASE_IDS = [(name, K, m) for K, m in FLAVOURS for name in BUILDERS] + [("pos24", POS24_K, False)]
GOLDEN_IDS = [(name, K, m) for name, K, m in CASE_IDS if name not in ("decide_far", "empty", "random")]


def case_id(c):
    return "%s-k%d-%s" % (c[0], c[1], "127" if c[2] else "63")


@functools.lru_cache(maxsize=None)
def build(name, K, mer127):
    return _pos24(900) if name == "pos24" else BUILDERS[name](K, mer127)


@functools.lru_cache(maxsize=None)
def model_rows(name, K, mer127):
    """(index inputs, the model's hit rows) of a case."""
    case = build(name, K, mer127)
    ctgs, ids, length, bal = loaded(case)
    if name == "pos24":
        index = MM.build_index_for_reads(ctgs, ids, K, case.reads)
    else:
        index = MM.build_index(ctgs, ids, K)
    return (ctgs, ids, length, bal), [MM.hit_row(index, rd, K) for rd in case.reads]


def model_out(name, K, mer127, align_len, id_limit=None):
    case = build(name, K, mer127)
    (ctgs, ids, length, bal), rows = model_rows(name, K, mer127)
    return [MM.decide(row, len(rd), K, align_len, length, bal, id_limit) for row, rd in zip(rows, case.reads)]


# batch shapes of the read kernel's launch (blocks of 256 lanes): reads of the `decide` case, cut and rearranged
def batch_shapes(case):
    K = case.K
    pool = [r for r in case.reads]
    while len(pool) < 257:
        pool = pool + pool
    none = [r[:K] for r in pool[:40]]                               # no read has a k-mer: an empty hit buffer
    short = pool[0][:K - 1]
    return {
        "n0": [], "n1": pool[:1], "n255": pool[:255], "n256": pool[:256], "n257": pool[:257],
        "no-kmers": none, "one-without-kmers": [short],
        "kmerless-first-and-last": [short] + pool[:254] + [pool[1][:K]],
        "kmerless-at-block-edges": pool[:255] + [short, short] + pool[:100] + [short],
    }


# ---------------------------------------------------------------------------------------------------------
# what keeps a comparison from passing vacuously, asserted on the model's output
# ---------------------------------------------------------------------------------------------------------
def check_not_vacuous(case, align_len, out, rows):
    mapped = [o for o in out if o[0]]
    if case.all_unmapped:
        assert not mapped, "%s: nothing may map" % case.name
        return
    assert any(o[2] == ord("+") for o in mapped) and any(o[2] == ord("-") for o in mapped) and len(mapped) < len(out), case.name
    assert any(o[3] == 0 for o in mapped)
    if align_len <= 60:                 # ALIGNLEN past the read: every k-mer must hit the chosen id, so no second id can count when
        assert any(o[3] == 1 for o in mapped), (case.name, align_len)       # K < 32 ... and the basics' footprint read is built for <= 60
    assert any(h is None for row in rows for h in row) and any(h is not None for row in rows for h in row)


# ---------------------------------------------------------------------------------------------------------
# product against model: every hit word and every per-read tuple, nothing filtered
# ---------------------------------------------------------------------------------------------------------
def product(cid, reads, align_len, device):
    """(rows as a list of hit words a read, per-read tuples) from pg_map_hits on `device` (-1: the host twin).  The call fails, and so
    does the test, when the index build's spin bound fired: a result at all means that flag was clear."""
    from soapdenovo2_amd import api
    name, K, mer127 = cid
    ctgs, ids, length, bal = model_rows(*cid)[0]
    ctg, pos, ori, fp, rows, koff = api.map_hits(ctgs, ids, length, bal, reads, K, align_len, mer127, device=device)
    assert len(koff) == len(reads) + 1 and int(koff[-1]) == len(rows)
    rows = [[int(w) for w in rows[int(koff[r]):int(koff[r + 1])]] for r in range(len(reads))]
    return rows, [(int(ctg[r]), int(pos[r]), int(ori[r]), int(fp[r])) for r in range(len(reads))]


def assert_rows_equal(got, want_rows, tags, what):
    assert len(got) == len(want_rows)
    for r, (g, w) in enumerate(zip(got, want_rows)):
        w = [MM.hit_word(h) for h in w]
        if g != w:
            j = next(j for j in range(max(len(g), len(w))) if j >= len(g) or j >= len(w) or g[j] != w[j])
            raise AssertionError("%s: read %d (%s) k-mer %d: hit word %s, the model has %s (id | (pos << 2 | twin << 1 | smaller) << 32)"
                                 % (what, r, tags[r], j, hex(g[j]) if j < len(g) else None, hex(w[j]) if j < len(w) else None))


def assert_out_equal(got, want, tags, what):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: read %d (%s): (contig, pos, orien, footprint) = %r, the model has %r" % (what, r, tags[r], g, w)


def compare_case(cid, device):
    """One case at every ALIGNLEN of the suite: the model's own conditions first, then the product's hit rows and outputs."""
    case = build(*cid)
    _, rows = model_rows(*cid)
    for A in align_lens(case.K, case.longest):
        want = model_out(*cid, A)
        check_not_vacuous(case, A, want, rows)
        what = "%s ALIGNLEN %d device %d" % (case_id(cid), A, device)
        got_rows, got = product(cid, case.reads, A, device)
        assert_rows_equal(got_rows, rows, case.tags, what)
        assert_out_equal(got, want, case.tags, what)


def compare_shapes(K, mer127, device):
    cid = ("decide", K, mer127)
    case = build(*cid)
    (ctgs, ids, length, bal), _ = model_rows(*cid)
    index = MM.build_index(ctgs, ids, K)
    for shape, reads in batch_shapes(case).items():
        rows, want = MM.map_reads(index, reads, K, 32, length, bal)
        if shape in ("no-kmers", "one-without-kmers", "n0"):
            assert sum(len(r) for r in rows) == 0
        tags = [shape] * len(reads)
        got_rows, got = product(cid, reads, 32, device)
        assert_rows_equal(got_rows, rows, tags, "%s k%d" % (shape, K))
        assert_out_equal(got, want, tags, "%s k%d" % (shape, K))
