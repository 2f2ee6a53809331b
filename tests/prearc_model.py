"""A plain model of the pre-arc lists (thread_add1preArc and output_arcs, prlRead2path.c:388-403, 426-476) on triples (from, to, seq), where seq says
when a read met the pair (read ordinal << 16 | position): the reference handles the meetings in ascending seq.  A pair it has not seen goes to the
HEAD of its source edge's list with multiplicity 1, a pair it has seen gets one more; the lists are printed by ascending source edge, head first.  So:
per pair, the multiplicity is the number of triples and the first meeting is the smallest seq; the rows come by ascending `from`, and within a
`from` by DESCENDING first meeting.  Python integers (fold) and numpy uint64 (fold_np); no code of the library.

The `wrong_*` arguments break the model the way a kernel could be broken (tests/test_prearc_cases_host.py shows that every designed case tells each
of them from the right answer); nothing else sets them."""
import numpy as np


def fold(triples, wrong_mult_bits=None, wrong_ascending=False, wrong_first_bits=None):
    """triples: an iterable of (from, to, seq), in any order, no two with the same seq for one `from`.  -> [(from, to, multiplicity)] in file order."""
    mult, first = {}, {}
    for f, t, s in triples:
        f, t, s = int(f), int(t), int(s)
        key = (f, t)
        mult[key] = mult.get(key, 0) + 1
        if key not in first or s < first[key]:
            first[key] = s
    if wrong_mult_bits:
        mult = {k: v & ((1 << wrong_mult_bits) - 1) for k, v in mult.items()}
    if wrong_first_bits:
        first = {k: v & ((1 << wrong_first_bits) - 1) for k, v in first.items()}
    sign = 1 if wrong_ascending else -1
    # (the stable sorts of a fold keep what came first in their input where keys tie; the model breaks such ties by `to`, which no right answer needs)
    order = sorted(mult, key=lambda k: (k[0], sign * first[k], k[1]))
    return [(f, t, mult[(f, t)]) for f, t in order]


def fold_np(frm, to, seq):
    """fold() for millions of triples: -> an array [n_pairs, 3] of uint32 in file order.  The first meetings of one `from` must differ."""
    frm = np.asarray(frm, dtype=np.uint64)
    to = np.asarray(to, dtype=np.uint64)
    seq = np.asarray(seq, dtype=np.uint64)
    key = (frm << np.uint64(32)) | to
    o = np.lexsort((seq, key))                              # by pair, a pair's meetings ascending
    k, s = key[o], seq[o]
    head = np.ones(len(k), dtype=bool)
    head[1:] = k[1:] != k[:-1]
    starts = np.flatnonzero(head)
    mult = np.diff(np.append(starts, len(k)))
    pk, first = k[starts], s[starts]
    pf = pk >> np.uint64(32)
    o2 = np.lexsort((~first, pf))                           # by source edge, then descending first meeting
    out = np.empty((len(o2), 3), dtype=np.uint32)
    out[:, 0] = pf[o2]
    out[:, 1] = pk[o2] & np.uint64(0xFFFFFFFF)
    out[:, 2] = mult[o2]
    return out


def as_rows(folded):
    return np.array(folded, dtype=np.uint32).reshape(-1, 3)


def prearc_lines(rows):
    """the rows of a fold as the text of <prefix>.preArc (output_arcs: `from` and then ` to multiplicity` for every target of its list)"""
    out, cur = [], None
    for f, t, m in rows:
        if cur is None or f != cur:
            if cur is not None:
                out.append("\n")
            out.append("%d" % f)
            cur = f
        out.append(" %d %d" % (t, m))
    if cur is not None:
        out.append("\n")
    return "".join(out)


def parse_prearc(text):
    """<prefix>.preArc -> [(from, [(to, multiplicity), ...])] in file order"""
    lists = []
    for line in text.splitlines():
        v = [int(x) for x in line.split()]
        assert len(v) >= 3 and len(v) % 2 == 1, line
        lists.append((v[0], list(zip(v[1::2], v[2::2]))))
    return lists


def triples_of_prearc(lists, seed=0):
    """Triples that would have made these lists: a line's targets get descending made-up first meetings (the head of a list is the pair met LAST for
    the first time), each target as many triples as its multiplicity, the later ones after every first meeting; all of it shuffled."""
    rng = np.random.RandomState(seed)
    triples = []
    clock = 1 << 16
    for f, targets in lists:
        n = len(targets)
        firsts = [clock + 5 * (n - i) for i in range(n)]                 # descending along the line
        late = clock + 5 * (n + 1)
        for (t, m), s in zip(targets, firsts):
            triples.append((f, t, s))
            for r in range(m - 1):
                late += 1 + int(rng.randint(0, 3))
                triples.append((f, t, late))
        clock = late + 7
    rng.shuffle(triples)
    return triples
