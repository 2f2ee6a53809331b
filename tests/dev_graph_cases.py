"""Inputs, models and comparisons for the k-mer-set layouts (csrc/dev_graph.hpp: layout_static, csrc/dev_rehash.hpp: layout_growable), the
modulus by reciprocal (csrc/graph_lookup.hpp: home_slot) and the append primitive (csrc/backend_hip.hpp: be_append_kernel), shared by the
two files that run them: tests/test_dev_graph_emu.py on the HostBackend (no GPU) and tests/test_gpu_dev_graph.py on the HipBackend the
product runs.  Every function here takes the hook to call -- HostHook (pg_host_emu_*) or DeviceHook (pg_device_emu_*) -- so that both
backends are held to the same models on the same inputs."""
import numpy as np

from soapdenovo2_amd import api

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
M64 = (1 << 64) - 1
APPEND_BASE = 0x9E3779B900000000                     # PG_EMU_APPEND_BASE of include/soapdenovo2_amd.h


# ---- which hook ---------------------------------------------------------------------------------------------------------------------
class HostHook:
    """pg_host_emu_*: the function objects on `threads` host threads."""
    name = "host"

    def __init__(self, threads=4):
        self.threads = threads

    def layout_static(self, rec, per_set, S, nw):
        P = len(per_set)
        out = np.zeros((P * S, nw + 1), dtype=np.uint64)
        cnt = np.array(per_set, dtype=np.uint64)
        rc = api.lib().pg_host_emu_layout_static(rec.ctypes.data, cnt.ctypes.data, P, S, int(nw == 4), self.threads, out.ctypes.data)
        return rc, out

    def layout_growable(self, rec, last, m, P, cap):
        """-> (sizes, rounds, node image, slot of every record)"""
        nw = 4 if m else 2
        slots = np.zeros(len(rec), dtype=np.uint64)
        sizes = np.zeros(P, dtype=np.uint64)
        rounds = np.zeros(P, dtype=np.uint64)
        nodes = np.zeros((cap, nw + 1), dtype=np.uint64)
        rc = api.lib().pg_host_emu_layout_growable(rec.ctypes.data, len(rec), last.ctypes.data, int(m), P, self.threads, slots.ctypes.data, sizes.ctypes.data,
                                                   rounds.ctypes.data, nodes.ctypes.data, cap)
        assert rc == 0, api.lib().pg_last_error()
        return sizes, rounds, nodes, slots

    def home_slots(self, keys, mer127, size):
        out = np.zeros(len(keys), dtype=np.uint64)
        api._check(api.lib().pg_host_emu_home_slots(keys.ctypes.data, len(keys), int(mer127), size, out.ctypes.data), "pg_host_emu_home_slots")
        return out


class DeviceHook:
    """pg_device_emu_*: the HipBackend instantiations on a GPU, through the product's own entry points."""
    name = "device"

    def __init__(self, device=0):
        self.device = device

    def layout_static(self, rec, per_set, S, nw):
        P = len(per_set)
        out = np.zeros((P * S, nw + 1), dtype=np.uint64)
        cnt = np.array(per_set, dtype=np.uint64)
        rc = api.lib().pg_device_emu_layout_static(self.device, rec.ctypes.data, cnt.ctypes.data, P, S, int(nw == 4), out.ctypes.data)
        assert rc >= 0, api.lib().pg_last_error()
        return rc, out

    def layout_growable(self, rec, last, m, P, cap):
        """-> (sizes, rounds, node image, None): a record's slot is read off the image"""
        nw = 4 if m else 2
        sizes = np.zeros(P, dtype=np.uint64)
        rounds = np.zeros(P, dtype=np.uint64)
        nodes = np.zeros((cap, nw + 1), dtype=np.uint64)
        rc = api.lib().pg_device_emu_layout_growable(self.device, rec.ctypes.data, len(rec), last.ctypes.data, int(m), P, sizes.ctypes.data, rounds.ctypes.data,
                                                     nodes.ctypes.data, cap)
        assert rc == 0, api.lib().pg_last_error()
        return sizes, rounds, nodes, None

    def home_slots(self, keys, mer127, size):
        out = np.zeros(len(keys), dtype=np.uint64)
        api._check(api.lib().pg_device_emu_home_slots(self.device, keys.ctypes.data, len(keys), int(mer127), size, out.ctypes.data), "pg_device_emu_home_slots")
        return out

    def append(self, flags, cap):
        """-> (list[0 .. cap) as the kernel left it, the counter)"""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        lst = np.zeros(max(cap, 1), dtype=np.uint64)
        cnt = np.zeros(1, dtype=np.uint64)
        api._check(api.lib().pg_device_emu_append(self.device, flags.ctypes.data, len(flags), cap, lst.ctypes.data, cnt.ctypes.data), "pg_device_emu_append")
        return lst[:cap], int(cnt[0])


# ---- the static layout against first come, first served -------------------------------------------------------------------------------------
def key_ints(keys):
    """the keys as Python integers, most significant word first"""
    out = []
    for k in keys:
        v = 0
        for w in k:
            v = (v << 64) | int(w)
        out.append(v)
    return out


def fcfs_model(keys, S, nw):
    """put_kmerset into a table that never grows (newhash.c:487-528): first empty slot at or after key mod size, in arrival order."""
    table = [None] * S
    for i, k in enumerate(keys):
        v = 0
        for w in k:
            v = (v << 64) | int(w)
        h = v % S                                   # exact for the 63-mer modulus; the 127-mer chain of 32-bit chunks is a true modulus while S < 2^32
        while table[h] is not None:
            h = (h + 1) % S
        table[h] = i
    return table


def fcfs_model_linked(keys, S, nw):
    """fcfs_model for tables where a cluster is tens of thousands of keys long (a probe a step would be 10^9 steps): the same first
    empty slot at or after key mod size, found through `nxt` -- nxt[h] = a slot at or cyclically behind h that no empty slot lies in
    front of, compressed on the way (union-find).  tests/test_dev_graph_emu.py holds it to fcfs_model on the small shapes."""
    table = [None] * S
    nxt = list(range(S))
    assert len(keys) < S
    for i, v in enumerate(key_ints(keys)):
        h = v % S
        r = h
        while nxt[r] != r:
            r = nxt[r]
        while nxt[h] != r:
            nxt[h], h = r, nxt[h]
        table[r] = i
        nxt[r] = (r + 1) % S
    return table


def static_case(S, n, nw):
    """Random keys, three sets of which one is empty, and a quarter of set 0's homes within 5 slots of the table's end, so that its last
    cluster certainly wraps.  -> (records, per_set)"""
    rng = np.random.default_rng(S * 7 + n + nw)
    per_set = [n, 0, max(1, n // 2)]
    total = sum(per_set)
    rec = np.zeros((total, nw + 2), dtype=np.uint64)
    rec[:, :nw] = rng.integers(0, 1 << 62, size=(total, nw), dtype=np.uint64)
    rec[:, 0] >>= np.uint64(3)                       # K <= 63 / 127 leaves the top bits of word 0 clear
    # homes concentrated near the end of the table in set 0, so that its last cluster certainly wraps
    for i in range(per_set[0] // 4):
        v = 0
        for w in rec[i, :nw]:
            v = (v << 64) | int(w)
        want = S - 1 - (i % 5)
        v += (want - v % S) % S
        for w in range(nw - 1, -1, -1):
            rec[i, w] = np.uint64(v & 0xFFFFFFFFFFFFFFFF); v >>= 64
    rec[:, nw] = np.arange(total, dtype=np.uint64) + np.uint64(1000)            # cnt: anything recognisable
    at = 0
    for s, c in enumerate(per_set):
        rec[at:at + c, nw + 1] = (np.uint64(s) << np.uint64(56)) | np.arange(c, dtype=np.uint64)
        at += c
    return rec, per_set


STATIC_SHAPES = [(1031, 600, 1), (1031, 1000, 4), (257, 250, 3), (4099, 3000, 8), (97, 96, 2)]        # (S, n, host threads)
STATIC_LARGE = (262147, 200000)                      # many blocks of the device's sort and scans; set 0's wrapped cluster is 50000 keys long


def check_static_vs_fcfs(hook, S, n, nw, model=fcfs_model):
    """The hook's image of static_case(S, n, nw) against the model, slot by slot: an empty slot's first word is EMPTY, a filled slot holds
    its record's key words and cnt.  Asserts that a cluster wrapped around the end of a table."""
    rec, per_set = static_case(S, n, nw)
    rc, out = hook.layout_static(rec, per_set, S, nw)
    assert rc == 0
    at = 0
    wrapped = False
    for s, c in enumerate(per_set):
        table = model(rec[at:at + c, :nw], S, nw)
        img = out[s * S:(s + 1) * S]
        filled = np.array([t is not None for t in table], dtype=bool)
        who = np.array([t if t is not None else 0 for t in table], dtype=np.int64)
        bad = np.nonzero(~filled & (img[:, 0] != EMPTY))[0]
        assert len(bad) == 0, (s, bad[:5])
        if c:
            bad = np.nonzero(filled & (img != rec[at + who, :nw + 1]).any(axis=1))[0]
            assert len(bad) == 0, (s, bad[:5])
        wrapped = wrapped or bool(c and table[S - 1] is not None and table[0] is not None)
        at += c
    assert wrapped


def check_static_full_pool(hook):
    rec = np.zeros((97, 4), dtype=np.uint64)
    rec[:, 1] = np.arange(97, dtype=np.uint64)
    rc, _ = hook.layout_static(rec, [97], 97, 2)
    assert rc == 1                                   # unsuited: the caller replays on the host (which reports the exploded pool)


# ---- the growable layout against the sequential host replay -------------------------------------------------------------------------------
def growable_vs_replay(hook, rec, last, P, m):
    """Sizes, slots and image of the hook's growable layout against api.host_replay_layout (pinned slot by slot on the oracle).  -> rounds"""
    nw = 4 if m else 2
    rec = np.ascontiguousarray(rec[np.argsort(rec[:, nw + 1], kind="stable")])
    want_slots, want_sizes = api.host_replay_layout(rec, last, P, mer127=m, a_gb=0)
    cap = int(sum(int(x) for x in want_sizes)) + 7
    sizes, rounds, nodes, slots = hook.layout_growable(rec, last, m, P, cap)
    assert [int(x) for x in sizes] == [int(x) for x in want_sizes]
    if slots is not None:
        bad = np.nonzero(slots != want_slots)[0]
        assert len(bad) == 0, (len(bad), bad[:5], slots[bad[:5]], want_slots[bad[:5]])
    else:
        slots = want_slots                           # read off the image: the record lies where the replay puts it and nothing lies anywhere else
    # the image: every record's key and payload word in its slot, everything else empty
    base = np.concatenate([[0], np.cumsum(want_sizes.astype(np.uint64))]).astype(np.uint64)
    at = base[(rec[:, nw + 1] >> np.uint64(api.PG_ORD_BITS)).astype(np.int64)] + slots
    bad = np.nonzero((nodes[at.astype(np.int64)] != rec[:, : nw + 1]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], want_slots[bad[:5]])
    filled = np.zeros(cap, dtype=bool)
    filled[at.astype(np.int64)] = True
    assert (nodes[:cap - 7][~filled[:cap - 7], 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and int(filled.sum()) == len(rec)
    return rounds


THRESHOLD_SETTINGS = [(None, None), (0, None), (2000, None), (0, 1), (2000, 1), (0, 3000), (0, 0)]    # (PG_RH_BLIND_MAX, PG_RH_DENSE_MIN)
THRESHOLD_SIZES = (1, 5, 793, 794, 795, 1590, 1591, 5000, 40000)


def set_thresholds(monkeypatch, blind_max=None, dense_min=None, list_shift=None):
    for name, v in (("PG_RH_BLIND_MAX", blind_max), ("PG_RH_DENSE_MIN", dense_min), ("PG_RH_LIST_SHIFT", list_shift)):
        if v is not None:
            monkeypatch.setenv(name, str(v))


def threshold_sets():
    """Random keys (no genome structure), set sizes right at the growth thresholds, with and without a duplicate put behind the last new
    key (newhash.c:477 tests the growth before it probes).  Yields (n, trailing, records, last)."""
    rng = np.random.default_rng(77)
    for n in THRESHOLD_SIZES:
        for trailing in (False, True):
            rec = np.zeros((n, 4), dtype=np.uint64)
            rec[:, :2] = rng.integers(0, 1 << 62, size=(n, 2), dtype=np.uint64)
            rec[:, 0] >>= np.uint64(3)
            rec[:, 3] = np.arange(n, dtype=np.uint64) * np.uint64(3)
            last = np.array([int(rec[-1, 3]) + (5 if trailing else 1)], dtype=np.uint64)
            yield n, trailing, rec, last


def four_word_sets():
    """Four-word keys (the 127-mer flavour: other initial size, chained 32-bit modulus for the home slot), three sets of different sizes in
    one call; every set saw a duplicate put after its last new key.  -> (records, last, P)"""
    rng = np.random.default_rng(177)
    counts = [30000, 7, 12345]
    recs = []
    for s, n in enumerate(counts):
        r = np.zeros((n, 6), dtype=np.uint64)
        r[:, :4] = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        r[:, 0] >>= np.uint64(3)
        r[:, 5] = (np.arange(n, dtype=np.uint64) * np.uint64(2)) | (np.uint64(s) << np.uint64(api.PG_ORD_BITS))
        recs.append(r)
    rec = np.concatenate(recs)
    last = np.array([2 * n + 3 for n in counts], dtype=np.uint64)
    return rec, last, 3


FUZZ_SEEDS = range(120)


def fuzz_draw(seed):
    """One seed of the fuzz over the fixed point's three thresholds: a small random set, either key width, every third with small numbers for
    keys -- their homes crowd (runs of consecutive slots), clusters are thousands of keys long and wrap around the end of the table.
    -> dict(blind_max, dense_min, list_shift, rec, last, four, threads)"""
    rng = np.random.default_rng(9000 + seed)
    blind_max = rng.choice([0, 0, 500, 5000])
    dense_min = rng.choice([0, 1, 1, 700, 4000])
    list_shift = rng.choice([0, 2, 5, 10])
    n = int(rng.choice([3, 50, 700, 793, 794, 1591, 3000, 9000, 25000]))
    four = bool(rng.integers(0, 2))
    nw = 4 if four else 2
    rec = np.zeros((n, nw + 2), dtype=np.uint64)
    rec[:, :nw] = rng.integers(0, 1 << 62, size=(n, nw), dtype=np.uint64)
    if rng.integers(0, 3) == 0:                                  # small numbers: home = key while the table is larger than they are, key mod size after
        rec[:, : nw - 1] = 0
        rec[:, nw - 1] = rng.integers(0, 1 << int(rng.integers(8, 20)), size=n, dtype=np.uint64)
    rec[:, 0] >>= np.uint64(3)
    rec = rec[np.unique(rec[:, :nw], axis=0, return_index=True)[1]]
    rec = rec[rng.permutation(len(rec))]
    rec[:, nw + 1] = np.arange(len(rec), dtype=np.uint64) * np.uint64(3)
    last = np.array([int(rec[-1, nw + 1]) + (5 if rng.integers(0, 2) else 1)], dtype=np.uint64)
    threads = int(rng.integers(1, 5))
    return dict(blind_max=blind_max, dense_min=dense_min, list_shift=list_shift, rec=rec, last=last, four=four, threads=threads)


def large_sets(nw, n=300000):
    """Two sets of n keys (above the default thresholds of 2^18 keys), one of random keys and one of small numbers (the other key words 0,
    the last below 2^19: runs of consecutive homes, long clusters).  -> (records, last, P)"""
    rng = np.random.default_rng(4100 + nw)
    recs = []
    for s in range(2):
        r = np.zeros((n, nw + 2), dtype=np.uint64)
        if s == 0:
            r[:, :nw] = rng.integers(0, 1 << 62, size=(n, nw), dtype=np.uint64)
            r[:, 0] >>= np.uint64(3)
            assert len(np.unique(r[:, :nw], axis=0)) == n
        else:
            r[:, nw - 1] = rng.permutation(1 << 19)[:n].astype(np.uint64)
        r[:, nw] = np.arange(n, dtype=np.uint64) + np.uint64(7)
        r[:, nw + 1] = (np.arange(n, dtype=np.uint64) * np.uint64(2)) | (np.uint64(s) << np.uint64(api.PG_ORD_BITS))
        recs.append(r)
    last = np.array([2 * n - 1, 2 * n + 3], dtype=np.uint64)           # set 1 saw a duplicate put after its last new key
    return np.concatenate(recs), last, 2


# ---- key mod size -----------------------------------------------------------------------------------------------------------------------------
def home_slot_case(mer127):
    """Sizes from 1 to 2^63 - 1 and keys incl. the extremes.  -> (sizes, keys)"""
    rng = np.random.default_rng(11)
    nw = 4 if mer127 else 2
    sizes = [1, 2, 3, 1031, 16777213, (1 << 32) - 1, 1 << 32, (1 << 32) + 15, 4294967311 * 3, (1 << 40) + 9, (1 << 62) + 1, (1 << 63) - 1, (1 << 63) - 25]
    sizes += [int(x) for x in rng.integers(1, 1 << 62, size=20)] + [int(x) for x in rng.integers(1, 1 << 34, size=20)]
    keys = rng.integers(0, 1 << 63, size=(4000, nw), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(4000, nw), dtype=np.uint64)
    keys[0] = 0
    keys[1] = M64
    keys[2, :] = [M64 if i % 2 else 0 for i in range(nw)]
    return sizes, np.ascontiguousarray(keys)


def home_slot_want(w, size, mer127):
    """Python's integers: the exact 128-bit modulus of the 63-mer build, and the 127-mer build's 32-bit chunks folded in 64-bit arithmetic --
    whose `t << 32` overflows once a set is larger than 2^32 slots (newhash.c:36-57)."""
    if not mer127:
        return ((w[0] << 64) | w[1]) % size
    t = w[0] % size
    for x in w[1:]:
        t = (((t << 32) & M64) | (x >> 32)) % size
        t = (((t << 32) & M64) | (x & 0xFFFFFFFF)) % size
    return t


def check_home_slots(hook, mer127, every=None):
    """every(size) = the stride over the keys that are compared (None: every key)"""
    sizes, keys = home_slot_case(mer127)
    rows = [[int(x) for x in k] for k in keys]
    for size in sizes:
        out = hook.home_slots(keys, mer127, size)
        for i in range(0, len(keys), every(size) if every else 1):
            assert int(out[i]) == home_slot_want(rows[i], size, mer127), (size, rows[i])


# ---- the append primitive ---------------------------------------------------------------------------------------------------------------------
APPEND_GRID = 4096 * 256                             # lanes of be_append_kernel's largest grid: a workgroup's trips are this far apart
APPEND_LONG = 6 * APPEND_GRID + 77                   # six trips and a ragged seventh: all flags set, `held` reaches 1280 and the loop flushes
APPEND_SHAPES = [(1, "all"), (255, "all"), (256, "all"), (257, "all"), (APPEND_GRID, "all"), (APPEND_LONG, "all"), (APPEND_LONG, "none"), (APPEND_LONG, "third"),
                 (APPEND_LONG, "last"), (APPEND_LONG, "one_workgroup"), (APPEND_LONG, "random90")]
APPEND_CAPS = ["hits+5", "hits", "hits-1", "1", "0"]


def append_flags(n, pattern):
    f = np.zeros(n, dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    if pattern == "all":
        f[:] = 1
    elif pattern == "third":
        f[::3] = 1
    elif pattern == "last":
        f[n - 1] = 1
    elif pattern == "one_workgroup":
        f[(i % APPEND_GRID) < 256] = 1
    elif pattern == "random90":
        f[np.random.default_rng(31).random(n) < 0.9] = 1
    else:
        assert pattern == "none"
    return f


def append_cap(hits, which):
    """the room of the list for a case, or None where it does not exist (hits - 1 with no hit)"""
    cap = {"hits+5": hits + 5, "hits": hits, "hits-1": hits - 1, "1": 1, "0": 0}[which]
    return cap if cap >= 0 else None


def check_append(hook, flags, cap):
    """The counter equals the number of hits, whatever the cap; with cap >= hits the sorted list equals the hit set; with cap < hits the cap
    entries are distinct members of the hit set; the list behind min(cap, hits) is still all ones."""
    want = np.uint64(APPEND_BASE) + np.nonzero(flags)[0].astype(np.uint64)          # (ascending)
    hits = len(want)
    lst, cnt = hook.append(flags, cap)
    assert cnt == hits, (cnt, hits, cap)
    k = min(cap, hits)
    got = np.sort(lst[:k])
    if cap >= hits:
        assert (got == want).all()
    else:
        assert k == 0 or (got[1:] != got[:-1]).all(), "an entry twice"
        at = np.searchsorted(want, got)
        assert (at < hits).all() and (want[np.minimum(at, hits - 1)] == got).all(), "an entry that is no hit"
    assert (lst[k:] == EMPTY).all()
