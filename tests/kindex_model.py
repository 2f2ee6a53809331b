"""An independent model of the k-mer index (include/soapdenovo2_amd.h, pg_kindex_*), written from the definitions and sharing no code
with the library: a dict from canonical k-mer (a Python int: 2 bits a base, first base most significant, A0 C1 T2 G3) to the record's
cnt word; a query walks the sequence's base codes, never packed words.

  * a sequence of len bases has max(0, len - K + 1) k-mers; k-mer j is bases [j, j + K)
  * canonical = the smaller of the k-mer and its reverse complement (complement of a code = code ^ 2), compared as integers
  * the answer for a k-mer is its record's cnt word, 0 when the set has no such record; a record whose `deleted` bit is set (bit 25 of
    word B, the high half of cnt: what pg_finalize's -d filter leaves of a k-mer it removes) is not in the set
  * summary of a sequence = (k-mers present, sum of their coverage, least coverage among them or 0 when none is present, index of
    the first absent k-mer or the number of k-mers when none is absent); coverage = bits 31:24 of cnt

The table's geometry (slots, home slot) is restated here too, only so that the tests can choose keys that collide."""
from collections import Counter

M64 = (1 << 64) - 1


def coverage(cnt):
    return (cnt >> 24) & 0xFF


def canonical_kmers(codes, K):
    """The canonical k-mers of a sequence of base codes, in order, as ints."""
    codes = [int(c) & 3 for c in codes]
    out = []
    if len(codes) < K:
        return out
    top = 2 * (K - 1)
    mask = (1 << (2 * K)) - 1
    fwd = rev = 0
    for i, c in enumerate(codes):
        fwd = ((fwd << 2) | c) & mask
        rev = (rev >> 2) | ((c ^ 2) << top)
        if i >= K - 1:
            out.append(min(fwd, rev))
    return out


def key_of_record(rec, nw):
    """The key words of a record (most significant first) as one int."""
    k = 0
    for q in range(nw):
        k = (k << 64) | int(rec[q])
    return k


def words_of_key(key, nw):
    return [(key >> (64 * (nw - 1 - q))) & M64 for q in range(nw)]


class Model:
    def __init__(self, K, nw):
        self.K, self.nw = K, nw
        self.cnt = {}
        self.deleted = set()

    @classmethod
    def from_records(cls, records, K, nw):
        m = cls(K, nw)
        for rec in records:
            key = key_of_record(rec, nw)
            assert key not in m.cnt and key not in m.deleted, "the records' keys are distinct"
            if not int(rec[nw]) >> (32 + 25) & 1:
                m.cnt[key] = int(rec[nw])
            else:
                m.deleted.add(key)
        return m

    def query(self, codes):
        return [self.cnt.get(k, 0) for k in canonical_kmers(codes, self.K)]

    def summary(self, codes):
        ans = self.query(codes)
        cov = [coverage(a) for a in ans if a]
        absent = [j for j, a in enumerate(ans) if not a]
        return [len(cov), sum(cov), min(cov) if cov else 0, absent[0] if absent else len(ans)]


def count_reads(reads, K):
    """What pass 1 counts from a set of reads of K + 1 bases or more: per canonical k-mer its occurrences and, in the canonical
    strand's orientation, how often each base preceded it (entries 0..3) and followed it (4..7).  A k-mer met on its own strand takes
    the read's neighbours as they are; one met as its reverse complement takes the complement of the next base as its left neighbour
    and of the previous base as its right one."""
    occ, arcs = Counter(), {}
    for r in reads:
        r = [int(c) & 3 for c in r]
        top = 2 * (K - 1)
        mask = (1 << (2 * K)) - 1
        fwd = rev = 0
        for i, c in enumerate(r):
            fwd = ((fwd << 2) | c) & mask
            rev = (rev >> 2) | ((c ^ 2) << top)
            j = i - K + 1
            if j < 0:
                continue
            prev = r[j - 1] if j > 0 else None
            nxt = r[i + 1] if i + 1 < len(r) else None
            if fwd < rev:
                key, left, right = fwd, prev, nxt
            else:
                key, left, right = rev, None if nxt is None else nxt ^ 2, None if prev is None else prev ^ 2
            occ[key] += 1
            a = arcs.setdefault(key, [0] * 8)
            if left is not None:
                a[left] += 1
            if right is not None:
                a[4 + right] += 1
    return occ, arcs


def filtered(arcs, delow):
    """The k-mers the -d filter removes (thread_delow): every neighbour counter of delow or less is cleared, and a k-mer left without
    any is deleted."""
    return {k for k, a in arcs.items() if delow > 0 and all(v <= delow for v in a)}


# ---- the table's geometry, restated (csrc/map_index.hpp: map_table_slots, map_hash, map_home) ----
def table_slots(n):
    s = 1024
    while s < 2 * n:
        s <<= 1
    return s


def key_hash(key, nw):
    h = 0x9E3779B97F4A7C15
    for w in words_of_key(key, nw):
        h ^= (w + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & M64
        h ^= h >> 30
        h = (h * 0xBF58476D1CE4E5B9) & M64
        h ^= h >> 27
        h = (h * 0x94D049BB133111EB) & M64
        h ^= h >> 31
    return h


def home_slot(key, nw, n_records):
    return key_hash(key, nw) & (table_slots(n_records) - 1)


def longest_probe_run(keys, nw):
    """Slots the longest lookup of a table of these keys visits, when they are inserted in this order by linear probing."""
    slots = table_slots(len(keys))
    taken = set()
    longest = 0
    for k in keys:
        e = key_hash(k, nw) & (slots - 1)
        run = 1
        while e in taken:
            e = (e + 1) & (slots - 1)
            run += 1
        taken.add(e)
        longest = max(longest, run)
    return longest
