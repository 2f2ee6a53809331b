"""Designed inputs for pass 2's pre-arc path (csrc/p2_kernels.hpp: add_prearc; csrc/graph_kernels.hip: p2_arc_init, p2_count_arcs, p2_compact_arcs,
p2_fold_arcs), shared by tests/test_prearc_cases_host.py (no GPU: every case is held to what it claims) and tests/test_gpu_prearc.py (the cases
through pg_device_emu_prearcs against tests/prearc_model.py).  A case is triples (from, to, seq), a table size, a lane count -- triple i goes to the
table of lane i mod lanes -- and the mistake it would catch.  The builder restates the table's home slot so that it can choose pairs by where they
land; nothing here calls the library."""
import functools

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
SEQ_MAX = ((1 << 46) - 1) << 16 | 65535                  # the largest first meeting: 46 bits of read ordinal, 16 of position


def home(frm, to, room):
    """the entry add_prearc probes first"""
    key = (int(frm) << 32) | int(to)
    return ((key * GOLD & M64) >> 20) & (room - 1)


def homes_np(frm, to, room):
    key = (np.asarray(frm, dtype=np.uint64) << np.uint64(32)) | np.asarray(to, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return ((key * np.uint64(GOLD)) >> np.uint64(20)) & np.uint64(room - 1)


class Case:
    def __init__(self, name, frm, to, seq, room, lanes, mistake, **claims):
        self.name, self.room, self.lanes, self.mistake, self.claims = name, room, lanes, mistake, claims
        self.frm = np.ascontiguousarray(frm, dtype=np.uint32)
        self.to = np.ascontiguousarray(to, dtype=np.uint32)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint64)
        assert len(self.frm) == len(self.to) == len(self.seq)
        for a in (self.frm, self.to, self.seq):
            a.setflags(write=False)

    @property
    def overflow(self):
        return self.claims.get("overflow", 0)

    def triples(self):
        return zip(self.frm.tolist(), self.to.tolist(), self.seq.tolist())

    def lane_keys(self, lane):
        """the distinct pairs of one lane's table, in input order"""
        seen = {}
        for f, t in zip(self.frm[lane::self.lanes].tolist(), self.to[lane::self.lanes].tolist()):
            seen.setdefault((f, t), None)
        return list(seen)


# ---- linear probing, restated ---------------------------------------------------------------------------------------------------------------
def simulate(keys, room, wrong_no_wrap=False, wrong_steps=None):
    """The distinct pairs `keys` into a table of `room` entries one after the other: -> (slot of every pair or None, longest probe run in entries,
    whether a run went on from the last entry to entry 0, pairs that found no entry).  The SET of occupied entries does not depend on the order.
    wrong_no_wrap: a run that reaches the table's end is lost; wrong_steps: a run gives up after that many entries (the right number: room)."""
    tab = [None] * room
    where, longest, crossed, lost = [], 0, False, 0
    for k in keys:
        h = home(k[0], k[1], room)
        for step in range(room if wrong_steps is None else wrong_steps):
            if wrong_no_wrap and h + step >= room:
                step = None
                break
            s = (h + step) & (room - 1)
            if tab[s] is None:
                tab[s] = k
                break
        else:
            step = None
        if step is None:
            lost += 1
            where.append(None)
            continue
        where.append((h + step) & (room - 1))
        longest = max(longest, step + 1)
        crossed = crossed or h + step >= room
    return where, longest, crossed, lost


def simulate_np(frm, to, room):
    """simulate() for millions of distinct pairs, all at once as the device's lanes go: in every round each pair still on its way looks at its next entry,
    the first to come takes an empty one, the others move on.  -> (occupied entries as a bool array, longest probe run)"""
    occ = np.zeros(room, dtype=bool)
    at = homes_np(frm, to, room).astype(np.int64)
    rounds = 0
    while len(at):
        rounds += 1
        assert rounds <= room
        first = np.zeros(len(at), dtype=bool)
        first[np.unique(at, return_index=True)[1]] = True
        takes = first & ~occ[at]
        occ[at[takes]] = True
        at = (at[~takes] + 1) & (room - 1)
    return occ, rounds


def pick(rng, room, want_home, n, taken, lo=1, hi=1 << 20, frm=None):
    """n fresh pairs whose home is one of `want_home`, as evenly as they come (frm: all of one source edge)"""
    out = []
    while len(out) < n:
        f = rng.randint(lo, hi, size=1 << 16) if frm is None else np.full(1 << 16, frm)
        t = rng.randint(lo, hi, size=1 << 16)
        h = homes_np(f, t, room)
        for i in np.flatnonzero(np.isin(h, np.asarray(want_home, dtype=np.uint64))):
            k = (int(f[i]), int(t[i]))
            if k not in taken:
                taken.add(k)
                out.append(k)
                if len(out) == n:
                    break
    return out


def random_pairs(rng, n, taken, lo=1, hi=1 << 20, frms=None):
    """n fresh pairs (frms: their source edges are drawn from these few, so that a source has many targets and the first meetings decide the order)"""
    out = []
    while len(out) < n:
        k = (int(rng.randint(lo, hi)) if frms is None else int(rng.choice(frms)), int(rng.randint(lo, hi)))
        if k not in taken:
            taken.add(k)
            out.append(k)
    return out


def meetings(rng, pairs, counts, start=1):
    """triples for pairs[i] met counts[i] times, shuffled; all seq differ (read ordinals from `start`, random positions)"""
    rows = [(f, t) for (f, t), c in zip(pairs, counts) for _ in range(c)]
    order = rng.permutation(len(rows))
    seq = [((start + int(o)) << 16) | int(rng.randint(0, 65536)) for o in order]
    idx = rng.permutation(len(rows))
    return [rows[i][0] for i in idx], [rows[i][1] for i in idx], [seq[i] for i in idx]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def one_home():
    rng = np.random.RandomState(11)
    room, H = 256, 17
    pairs = pick(rng, room, [H], 200, set(), frm=5)         # one source edge: the pairs' first meetings decide the whole order
    frm, to, seq = [], [], []
    when = rng.permutation(200 * 64).reshape(200, 64)      # (a pair's minimum at a random place of its 64, the pairs' meetings interleaved)
    for p, (f, t) in enumerate(pairs):                     # 64 triples side by side: one wave, one pair, one empty entry
        for j in range(64):
            frm.append(f); to.append(t); seq.append(((1000 + int(when[p, j])) << 16) | int(rng.randint(0, 65536)))
    return Case("one_home", frm, to, seq, room, 1,
                "a claim lost or doubled: of the waves that find one entry empty one pair gets it, every lane of that pair counts there and takes its minimum, every other pair moves on",
                distinct=200, longest=200, crosses=False, same_home=True)


def wraps(room):
    rng = np.random.RandomState(12)
    if room == 2:
        pairs = pick(rng, room, [1], 2, set())
    else:
        pairs = pick(rng, room, [room - 4, room - 3, room - 2, room - 1], 16, set())
    f, t, s = meetings(rng, pairs, [int(c) for c in rng.randint(1, 4, size=len(pairs))])
    return Case("wraps_room%d" % room, f, t, s, room, 1, "a wrong wrap mask: the run that reaches the last entry goes on at entry 0",
                distinct=len(pairs), crosses=True, longest_at_least=2 if room == 2 else 4)


def full():
    rng = np.random.RandomState(13)
    room = 256
    taken = set()
    pairs = random_pairs(rng, room - 1, taken)
    where, _, _, lost = simulate(pairs, room)
    assert not lost
    empty = (set(range(room)) - set(where)).pop()
    pairs += pick(rng, room, [(empty + 1) & (room - 1)], 1, taken)     # met last, this pair visits every entry before it finds the empty one
    counts = [int(c) for c in rng.randint(1, 4, size=room)]
    rows = [(f, t) for (f, t), c in zip(pairs, counts) for _ in range(c)]
    seq = [((1 + i) << 16) | int(rng.randint(0, 65536)) for i in rng.permutation(len(rows))]
    return Case("full", [r[0] for r in rows], [r[1] for r in rows], seq, room, 1,
                "a table held full one entry early (a probe loop of room - 1 steps), or an overflow counted where there is none",
                distinct=room, load=1.0, longest=room, crosses=True)


def over(room, d):
    rng = np.random.RandomState(14 + d)
    pairs = random_pairs(rng, room + d, set())
    f, t, s = meetings(rng, pairs, [1] * len(pairs))
    return Case("over_room%d_d%d" % (room, d), f, t, s, room, 1, "an overflow that is not counted once a triple: the counter is exactly the pairs too many",
                distinct=room + d, overflow=d)


def hot():
    rng = np.random.RandomState(15)
    taken = {(77, 4242)}
    cold = random_pairs(rng, 950, taken) + random_pairs(rng, 50, taken, frms=[77])     # (50 more targets of the hot pair's source: its first meeting places it)
    n = 100000 + 1000
    frm = np.empty(n, dtype=np.uint32); to = np.empty(n, dtype=np.uint32)
    frm[:] = 77; to[:] = 4242
    where = rng.choice(n, size=1000, replace=False)
    frm[where] = [c[0] for c in cold]; to[where] = [c[1] for c in cold]
    seq = ((np.arange(n, dtype=np.uint64) + np.uint64(200000)) << np.uint64(16)) | rng.randint(0, 65536, size=n).astype(np.uint64)
    mid = n // 2 + 3
    assert frm[mid] == 77
    seq[mid] = (5 << 16) | 9                               # the hot pair's earliest meeting lies in the middle of the input
    return Case("hot", frm, to, seq, 2048, 1, "a multiplicity kept in 16 bits, a minimum that only the first lanes of a pair take", distinct=1001, hot_mult=100000)


def first_bits(which):
    rng = np.random.RandomState(16)
    n = 48
    if which == "low16":
        firsts = [(12345 << 16) | int(v) for v in [0, 65535] + list(rng.choice(np.arange(1, 65535), n - 2, replace=False))]
        unit, says = 1, "first meetings that differ in the position only"
    elif which == "16to31":
        firsts = [(3 << 32) | (int(v) << 16) | 0x1234 for v in [0, 65535] + list(rng.choice(np.arange(1, 65535), n - 2, replace=False))]
        unit, says = 1 << 16, "first meetings that differ in bits 16 - 31 only"
    elif which == "32up":
        firsts = [(int(v) << 32) | 0x89ABCDEF for v in [1, 65535] + list(rng.choice(np.arange(2, 65535), n - 2, replace=False))]
        unit, says = 1 << 32, "first meetings that differ above bit 32 only: a first meeting kept or sorted in 32 bits"
    else:
        firsts = [(int(v) << 48) | 0xFFFFFFFFFFFF for v in [0, (1 << 14) - 1] + list(rng.choice(np.arange(1, (1 << 14) - 1), n - 2, replace=False))]
        unit, says = 1 << 48, "first meetings that differ above bit 48 only, up to the largest there is: a sort over too few key bits"
        assert max(firsts) == SEQ_MAX
    tos = rng.choice(np.arange(1, 100000), n, replace=False)
    frm, to, seq = [], [], []
    for t, s in zip(tos.tolist(), firsts):
        frm.append(7); to.append(t); seq.append(s)
        if s + unit <= SEQ_MAX and rng.randint(0, 2):      # (met once more, later)
            frm.append(7); to.append(t); seq.append(s + unit)
    idx = rng.permutation(len(frm))
    return Case("first_bits_" + which, np.array(frm)[idx], np.array(to)[idx], np.array(seq, dtype=np.uint64)[idx], 256, 1, says, distinct=n, one_from=True)


def ids():
    rng = np.random.RandomState(17)
    BIG = 0xFFFFFFFE
    pairs = [(BIG, BIG), (BIG, 1), (1, BIG), (BIG - 1, BIG), (BIG, BIG - 1), (1, 1), (1, 2), (2, 1), (0x80000000, 5), (5, 0x80000000), (0x7FFFFFFF, 0x80000001),
             (0x80000001, 0x7FFFFFFF), (65536, 65536), (0xFFFF0000, 0x0000FFFF), (0x0000FFFF, 0xFFFF0000)]
    taken = set(pairs)
    for f in np.unique(rng.randint(3, 1 << 31, size=400, dtype=np.int64))[:300].tolist() + np.unique(rng.randint(1 << 31, BIG - 2, size=200, dtype=np.int64))[:100].tolist():
        pairs.append((int(f), int(rng.randint(1, 1 << 31))))                    # many `from` with one target each, either side of 2^31
    busy = 0x9000ABCD
    for t in np.unique(rng.randint(1, 1 << 31, size=600, dtype=np.int64))[:500].tolist():  # one `from` with 500 targets
        pairs.append((busy, int(t)))
    assert len(set(pairs)) == len(pairs)
    f, t, s = meetings(rng, pairs, [int(c) for c in rng.randint(1, 3, size=len(pairs))])
    return Case("ids", f, t, s, 2048, 1, "edge ids cut to 31 bits or compared signed, (a, b) taken for (b, a), a second sort that is not stable or not over 32 bits of `from`",
                distinct=len(pairs), busy=busy)


def lanes(L, lonely):
    """lonely: the last lane's table holds one pair and nothing else -- a pair every lane has; and the largest pair is on several lanes, so the merged
    array ends inside a pair.  Otherwise the largest pair is on one lane: the last entry of the merged array is a head."""
    rng = np.random.RandomState(100 + 2 * L + lonely)
    per = [[] for _ in range(L)]                            # the lanes' meetings (from, to), in any order
    taken = set()
    open_lanes = list(range(L - 1)) if lonely else list(range(L))
    top = (60000, 60000)                                    # the largest pair of all
    on_all = [top] if lonely else random_pairs(rng, 12, taken, hi=50000, frms=[3, 9])
    for k in on_all:
        for l in range(L):
            per[l] += [k] * int(rng.randint(1, 4))
    most = min(len(open_lanes), L - 1)                      # on some lanes: two or more, not all
    some = random_pairs(rng, 25, taken, hi=50000, frms=[3, 9]) if most >= 2 else []
    for k in some:
        for l in rng.choice(open_lanes, int(rng.randint(2, most + 1)), replace=False).tolist():
            per[l] += [k] * int(rng.randint(1, 4))
    for k in random_pairs(rng, 30, taken, hi=50000, frms=[3, 9]):       # on one lane
        per[int(rng.choice(open_lanes))] += [k] * int(rng.randint(1, 4))
    if not lonely:
        per[int(rng.choice(open_lanes))] += [top] * 2
    width = max(len(p) for p in per)
    for l in range(L):                                      # every lane as many triples: index i is lane i mod L
        fill = top if lonely and l == L - 1 else (50001 + l, 7)
        per[l] += [fill] * (width - len(per[l]))
        rng.shuffle(per[l])
    n = width * L
    frm = [per[i % L][i // L][0] for i in range(n)]
    to = [per[i % L][i // L][1] for i in range(n)]
    # the earliest meeting of a pair on the LAST lane that has it
    seq = [0] * n
    clock = iter(rng.permutation(n).tolist())
    last_lane = {}
    for i in range(n):
        last_lane[(frm[i], to[i])] = max(last_lane.get((frm[i], to[i]), -1), i % L)
    early = {}
    for i in range(n):
        k = (frm[i], to[i])
        if i % L == last_lane[k] and k not in early:
            early[k] = i
    rank = {k: r for r, k in enumerate(early)}
    for i in range(n):
        seq[i] = ((10000 + next(clock)) << 16) | int(rng.randint(0, 65536))
    for k, i in early.items():
        seq[i] = ((1 + rank[k]) << 16) | int(rng.randint(0, 65536))
    return Case("lanes%d_%s" % (L, "lonely" if lonely else "mixed"), frm, to, seq, 256, L,
                "a merge that drops or doubles a lane's copy, keeps the first copy's meeting instead of the earliest, or miscounts the pairs at the array's end",
                lonely=lonely, top=top, on_all=on_all, n_some=len(some))


@functools.lru_cache(maxsize=1)
def second_trip(which):
    """count: 600 000 pairs in 2^20 entries (p2_count_arcs and p2_compact_arcs stride over 2048 x 256 entries a trip); fold: 2 200 000 pairs in 2^22
    entries (the pf_* kernels over 8192 x 256 entries a trip).  (One of the two is kept at a time.)"""
    rng = np.random.RandomState(18)
    room, n_pairs = (1 << 20, 600000) if which == "count" else (1 << 22, 2200000)
    key = np.unique((rng.randint(1, 300000, size=n_pairs * 5 // 4).astype(np.uint64) << np.uint64(32)) | rng.randint(1, 1 << 31, size=n_pairs * 5 // 4).astype(np.uint64))
    key = key[rng.permutation(len(key))[:n_pairs]]
    assert len(key) == n_pairs
    key = np.concatenate([key, key[rng.randint(0, n_pairs, size=n_pairs // 10)]])            # a tenth of them met again
    key = key[rng.permutation(len(key))]
    seq = ((rng.permutation(len(key)).astype(np.uint64) + np.uint64(1)) << np.uint64(16)) | rng.randint(0, 65536, size=len(key)).astype(np.uint64)
    return Case("second_trip_" + which, key >> np.uint64(32), key & np.uint64(0xFFFFFFFF), seq, room, 1,
                "a slip in the second trip of a grid-stride loop: a barrier not every lane of a workgroup reaches, a stale workgroup counter, an index in 32 bits",
                distinct=n_pairs, big=True)


SMALL = {
    "one_home": one_home,
    "wraps_room256": lambda: wraps(256),
    "wraps_room2": lambda: wraps(2),
    "full": full,
    "over_room256_d1": lambda: over(256, 1),
    "over_room256_d7": lambda: over(256, 7),
    "over_room2_d1": lambda: over(2, 1),
    "hot": hot,
    "first_bits_low16": lambda: first_bits("low16"),
    "first_bits_16to31": lambda: first_bits("16to31"),
    "first_bits_32up": lambda: first_bits("32up"),
    "first_bits_48up": lambda: first_bits("48up"),
    "ids": ids,
    "lanes2_mixed": lambda: lanes(2, False), "lanes2_lonely": lambda: lanes(2, True),
    "lanes3_mixed": lambda: lanes(3, False), "lanes3_lonely": lambda: lanes(3, True),
    "lanes8_mixed": lambda: lanes(8, False), "lanes8_lonely": lambda: lanes(8, True),
}
BIG = {"second_trip_count": lambda: second_trip("count"), "second_trip_fold": lambda: second_trip("fold")}
OVER = [n for n in SMALL if n.startswith("over_")]


@functools.lru_cache(maxsize=None)
def small(name):
    c = SMALL[name]()
    assert c.name == name
    return c
