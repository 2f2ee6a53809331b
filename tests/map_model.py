"""An independent model of the `map` stage's index, hit rows and per-read decision, in plain Python / numpy.

It shares no code with the product: k-mers are Python ints (2 bits a base, A C T G = 0 1 2 3, first base most significant), the index is a
dict, and the decision is written the slow, obvious way from the rule stated in csrc/map_decide.hpp's header and DESIGN.md.  It has no
special path for any number of contig ids.  tests/test_map_edges.py pins it to what the reference binary wrote (tests/golden/
map_edges_golden.py); where that file cannot speak (footprint, ids past the contig table, hit rows) the model follows the stated rule.

`map_home` / `table_slots` / `probe_slots` restate the product's table layout ONLY so that a test can assert that an input really
produces a wrapped probe chain or an exactly-full table.  No answer of the model depends on them."""
import numpy as np

POS_MASK = 0xFFFFFF                      # the reference keeps a k-mer's position in a 24-bit field
DELETED = "deleted"
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def kmers(codes, K):
    """(forward word, reverse-complement word) of every K-mer of a base-code sequence, as Python ints."""
    codes = [int(c) & 3 for c in codes]
    n = len(codes) - K + 1
    if n <= 0:
        return []
    mask = (1 << (2 * K)) - 1
    fwd = rev = 0
    out = []
    for i, c in enumerate(codes):
        fwd = ((fwd << 2) | c) & mask
        rev = (rev >> 2) | ((c ^ 2) << (2 * (K - 1)))        # the complement of a code is code ^ 2
        if i >= K - 1:
            out.append((fwd, rev))
    return out


def build_index(contigs, ids, K):
    """canonical k-mer -> (id, pos & 0xFFFFFF, twin) or DELETED when the key was put twice or more.  twin = 1 where the contig's reverse
    strand is the canonical one.  Contigs shorter than K + 2 are not indexed."""
    index = {}
    for seq, cid in zip(contigs, ids):
        if len(seq) < K + 2:
            continue
        for pos, (f, r) in enumerate(kmers(seq, K)):
            key = min(f, r)
            if key in index:
                index[key] = DELETED
            else:
                index[key] = (int(cid), pos & POS_MASK, 0 if f < r else 1)
    return index


def build_index_for_reads(contigs, ids, K, reads):
    """The same index restricted to the keys that occur in `reads` (for a contig too long for a dict of all its k-mers); K <= 32.
    Occurrences in the contigs are counted with numpy."""
    assert K <= 32
    wanted = set()
    for rd in reads:
        if len(rd) >= K + 1:
            wanted.update(min(f, r) for f, r in kmers(rd, K))
    want = np.array(sorted(wanted), dtype=np.uint64)
    count = np.zeros(len(want), dtype=np.int64)
    first = [None] * len(want)
    for seq, cid in zip(contigs, ids):
        if len(seq) < K + 2:
            continue
        s = np.asarray(seq, dtype=np.uint64) & np.uint64(3)
        n = len(s) - K + 1
        f = np.zeros(n, dtype=np.uint64)
        r = np.zeros(n, dtype=np.uint64)
        for q in range(K):
            f |= s[q:q + n] << np.uint64(2 * (K - 1 - q))
            r |= (s[q:q + n] ^ np.uint64(2)) << np.uint64(2 * q)
        key = np.minimum(f, r)
        at = np.searchsorted(want, key)
        at[at >= len(want)] = 0
        hit = np.nonzero(want[at] == key)[0] if len(want) else np.zeros(0, np.int64)
        for pos in hit:
            w = int(at[pos])
            count[w] += 1
            if first[w] is None:
                first[w] = (int(cid), int(pos) & POS_MASK, 0 if f[pos] < r[pos] else 1)
    index = {}
    for w, c in enumerate(count):
        if c == 1:
            index[int(want[w])] = first[w]
        elif c > 1:
            index[int(want[w])] = DELETED
    return index


def hit_row(index, read, K):
    """One entry a k-mer of the read: None (absent or deleted key) or (id, pos, twin, smaller); smaller = 1 where the read's forward
    strand is the canonical one.  Reads shorter than K + 1 have no k-mers."""
    if len(read) < K + 1:
        return []
    row = []
    for f, r in kmers(read, K):
        v = index.get(min(f, r))
        row.append(None if v is None or v is DELETED else (v[0], v[1], v[2], 1 if f < r else 0))
    return row


def hit_word(h):
    """The product's 64-bit hit word of a row entry."""
    if h is None:
        return 0
    cid, pos, twin, smaller = h
    return cid | (((pos & POS_MASK) << 2 | twin << 1 | smaller) << 32)


def _s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def decide(row, read_len, K, align_len, id_len, id_bal, id_limit=None):
    """(contig, position, orientation, footprint) of a read from its hit row; (0, 0, 0, 0) when it does not map.  id_len / id_bal =
    length and bal of every contig id; ids past the tables read as length 0, bal 1.  id_limit: count only hits of the first `id_limit`
    distinct ids (what a decision that drops later ids would see; tests use it to show that an input tells the two apart)."""
    if not row:
        return (0, 0, 0, 0)
    multi = max(2, min(read_len, align_len) - K + 1)
    live = list(row)
    if id_limit is not None:
        seen = []
        for h in live:
            if h is not None and h[0] not in seen:
                seen.append(h[0])
        keep = set(seen[:id_limit])
        live = [h if h is not None and h[0] in keep else None for h in live]
    mapped = footprint_ids = 0
    best, best_at = 0, None
    for j in range(len(live)):
        if live[j] is None:
            continue
        cid = live[j][0]
        n = 1
        for s in range(j + 1, len(live)):
            if live[s] is not None and live[s][0] == cid:
                n += 1
                live[s] = None                               # consumed: counted with its id's first hit
        if K > 32 or (K < 32 and n >= 2):
            footprint_ids += 1
        if n < multi:
            continue
        mapped += 1
        if n > best:                                         # strictly more: the first in first-hit order keeps a tie
            best, best_at = n, j
    if not mapped:
        return (0, 0, 0, 0)
    cid, pos, twin, smaller = row[best_at]
    ordinal = best_at + 1
    known = cid < len(id_len)
    if twin == smaller:
        length = int(id_len[cid]) if known else 0
        bal = int(id_bal[cid]) if known else 1
        return ((cid + bal - 1) & M32, _s32(length - pos - K - ordinal + 1), ord("-"), 1 if footprint_ids > 1 else 0)
    return (cid, _s32(pos - ordinal + 1), ord("+"), 1 if footprint_ids > 1 else 0)


def map_reads(index, reads, K, align_len, id_len, id_bal, id_limit=None):
    """(hit rows, per-read tuples) of a batch."""
    rows = [hit_row(index, rd, K) for rd in reads]
    return rows, [decide(row, len(rd), K, align_len, id_len, id_bal, id_limit) for row, rd in zip(rows, reads)]


# ---------------------------------------------------------------------------------------------------------
# the product's table layout, restated so that tests can assert what an input exercises -- never used for an answer
# ---------------------------------------------------------------------------------------------------------
def map_home(key, nw, mask):
    h = 0x9E3779B97F4A7C15
    for i in range(nw):
        w = (key >> (64 * (nw - 1 - i))) & M64
        h ^= (w + 0x9E3779B97F4A7C15 + ((h << 6) & M64) + (h >> 2)) & M64
        h ^= h >> 30
        h = (h * 0xBF58476D1CE4E5B9) & M64
        h ^= h >> 27
        h = (h * 0x94D049BB133111EB) & M64
        h ^= h >> 31
    return h & mask


def table_slots(n_kmers):
    s = 1024
    while s < 2 * n_kmers:
        s <<= 1
    return s


def n_index_kmers(contigs, K):
    return sum(len(c) - K + 1 for c in contigs if len(c) >= K + 2)


def probe_slots(contigs, K, nw):
    """{canonical key: (home, slot)} of linear probing over the indexed contigs in order (which slots end up taken does not depend on the
    order); a key with slot < home has a chain that ran off the last slot and wrapped to slot 0."""
    slots = table_slots(n_index_kmers(contigs, K))
    taken, where = {}, {}
    for seq in contigs:
        if len(seq) < K + 2:
            continue
        for f, r in kmers(seq, K):
            key = min(f, r)
            if key in where:
                continue
            home = e = map_home(key, nw, slots - 1)
            while e in taken:
                e = (e + 1) & (slots - 1)
            taken[e] = key
            where[key] = (home, e)
    return slots, where
