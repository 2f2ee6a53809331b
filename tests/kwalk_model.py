"""An independent model of the walk (include/soapdenovo2_amd.h, pg_kindex_walk), written from the rule and sharing no code with the
library: the index is kindex_model.Model's dict from canonical k-mer (a Python int) to cnt word, and a walk steps over lists of base
codes, never packed words.

  * sequence r of a batch gives walk 2r, from its last k-mer as read, and walk 2r + 1, from the reverse complement of its first k-mer;
    a sequence shorter than K gives two empty walks with reason NO_KMER
  * the cnt word of a canonical k-mer: left counter a = bits 6a+5:6a of its low half, right counter b the same bits of its high half,
    coverage = bits 31:24.  For an oriented k-mer x with canonical form c: x == c: out(b) = right[b], in(a) = left[a]; x == rc(c):
    out(b) = left[b ^ 2], in(a) = right[a ^ 2]
  * solid = in the set (not deleted) with coverage >= min_cov; an arc exists when its counter is >= min_arc
  * the start not solid: SEED_WEAK.  Then from x: no out arc DEAD_END, several BRANCH_OUT; y = x[1:] + [b]; y not solid WEAK_NEXT; y's in
    arcs other than exactly {x[0]}: BRANCH_IN; canon(y) == canon(start): LOOP; else b is appended, y's coverage summed, and max_ext bases
    end the walk with MAX_EXT
  * a walk's row = its bases, 32 a word, first base in the most significant bits, zero elsewhere, ceil(max_ext / 32) words; its report =
    length | reason << 32, then the coverage sum"""
import numpy as np

import kindex_model as M

NO_KMER, SEED_WEAK, DEAD_END, BRANCH_OUT, WEAK_NEXT, BRANCH_IN, LOOP, MAX_EXT = range(1, 9)
NAMES = {NO_KMER: "no_kmer", SEED_WEAK: "seed_weak", DEAD_END: "dead_end", BRANCH_OUT: "branch_out", WEAK_NEXT: "weak_next", BRANCH_IN: "branch_in",
         LOOP: "loop", MAX_EXT: "max_ext"}


def value(codes):
    return int("".join("0123"[int(c)] for c in codes), 4) if len(codes) else 0


def revcomp(codes):
    return [int(c) ^ 2 for c in reversed(codes)]


def oriented(codes):
    """(canonical k-mer as an int, whether the k-mer is its canonical form)."""
    f, r = value(codes), value(revcomp(codes))
    return (f, True) if f <= r else (r, False)


def counters(w):
    return [(w >> 6 * a) & 63 for a in range(4)], [(w >> 32 >> 6 * b) & 63 for b in range(4)]


def out_arcs(w, fwd):
    left, right = counters(w)
    return [right[b] if fwd else left[b ^ 2] for b in range(4)]


def in_arcs(w, fwd):
    left, right = counters(w)
    return [left[a] if fwd else right[a ^ 2] for a in range(4)]


def solid(w, min_cov):
    return w != 0 and M.coverage(w) >= min_cov


def walk(model, start, min_cov, min_arc, max_ext):
    """The walk to the right of the oriented k-mer `start` (K base codes): (appended bases, reason, coverage sum)."""
    x = [int(c) for c in start]
    key0, fwd = oriented(x)
    w = model.cnt.get(key0, 0)
    if not solid(w, min_cov):
        return [], SEED_WEAK, 0
    ext, cov = [], 0
    while True:
        nxt = [b for b, n in enumerate(out_arcs(w, fwd)) if n >= min_arc]
        if not nxt:
            return ext, DEAD_END, cov
        if len(nxt) > 1:
            return ext, BRANCH_OUT, cov
        y = x[1:] + nxt
        key, y_fwd = oriented(y)
        wy = model.cnt.get(key, 0)
        if not solid(wy, min_cov):
            return ext, WEAK_NEXT, cov
        if [a for a, n in enumerate(in_arcs(wy, y_fwd)) if n >= min_arc] != [x[0]]:
            return ext, BRANCH_IN, cov
        if key == key0:
            return ext, LOOP, cov
        ext.append(nxt[0])
        cov += M.coverage(wy)
        x, w, fwd = y, wy, y_fwd
        if len(ext) == max_ext:
            return ext, MAX_EXT, cov


def walks_of(model, seq, min_cov, min_arc, max_ext):
    """The two walks of a sequence of base codes: [walk 2r, walk 2r + 1]."""
    K = model.K
    seq = [int(c) for c in seq]
    if len(seq) < K:
        return [([], NO_KMER, 0), ([], NO_KMER, 0)]
    return [walk(model, seq[len(seq) - K:], min_cov, min_arc, max_ext), walk(model, revcomp(seq[:K]), min_cov, min_arc, max_ext)]


def row_of(ext, n_words):
    row = [0] * n_words
    for i, c in enumerate(ext):
        row[i // 32] |= c << (62 - 2 * (i % 32))
    return row


def want(model, seqs, min_cov, min_arc, max_ext):
    """(rows (2 n, ceil(max_ext / 32)) uint64, report (4 n,) uint64, the walks as (bases, reason, coverage sum)) of a batch."""
    n_words = (max_ext + 31) // 32
    walks = [w for s in seqs for w in walks_of(model, s, min_cov, min_arc, max_ext)]
    rows = np.array([row_of(e, n_words) for e, _, _ in walks], dtype=np.uint64).reshape(len(walks), n_words)
    report = np.array([v for e, reason, cov in walks for v in (len(e) | reason << 32, cov)], dtype=np.uint64)
    return rows, report, walks
