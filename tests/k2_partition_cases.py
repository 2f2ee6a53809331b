"""Inputs that take the counting kernel of the partition engine (K2: skm_count_kernel, csrc/partition_kernels.hip) through the code
only large partitions reach, at test size: with PG_LOG2_PARTS=4 (16 partitions instead of at least 256) a few thousand reads make
partitions of several windows and several key ranges, and designed heavy-hitter reads fill whole windows with copies of one record
whose k-mers are all one node.  Shared by tests/test_k2_partition_cases_host.py (the inputs are what they claim to be, through the
per-partition statistics of tests/emu_skm.cpp) and tests/test_gpu_k2_partitions.py (the kernels against the oracle on them).

Base codes as everywhere: A 0, C 1, T 2, G 3 (the complement is code ^ 2)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- what the conditions rest on (csrc/partition_kernels.hip) -----------------------------------------------------------------------
SLOTS = 2048                     # e2_count's launches: skm_count_kernel<NW, 2048, 1024, WIN, ...>, the LDS set's slots
WIN = {2: 512, 4: 192}           # the same launches: records a window, by words a k-mer (the two-word and the four-word flavour)
DD_FIRST = 4096                  # `if (ADAPT && dd_on && dd_rec < 4096u)`: the records a workgroup looks at before it decides
DD_PCT = 70                      # `constexpr uint32_t dd_pct = 70u`: more representatives than that and the search for copies stops
MAXPROBE = {2: 128, 4: 96}       # E2Cfg<NW>::MAXPROBE: a longer probe sequence aborts the attempt and the key range is split
CHUNK_LIST_RECORDS = 256 * 128   # chunk_ids2[2][256] lists of e.rpc = 128 records: (direct + maxc) * 128 <= 32768 records a partition
MAX_PART_RECORDS = 30000         # ... no case comes near it (beyond: F_CHUNKS, the pass falls to the global set and tests nothing here)
COPIES_MAX = 512                 # `(dcount[gtid] - 1u) << 9`: copies - 1 in the header's bits 9..17, n in bits 2..8
LOG2_PARTS = 4                   # e2_plan: `p.log2_global = std::max(4, ...test_log2_parts)`, the hook's floor

GEOM = {31: (False, 5), 25: (False, 5), 63: (False, 5), 127: (True, 7)}     # K of the heavy-hitter inputs -> four-word flavour, payload words a record


def nw_of(m127):
    return 4 if m127 else 2


def nmax(K, m127=None):
    """k-mers a record holds at most (skm_geometry; test_k2_dedupe_edges._nmax for the flavour the K takes by itself)."""
    if m127 is None:
        m127 = K > 63
    return min(32 * (7 if m127 else 5) - (K - 1) - 2, 127)


# ---- the serial harness (tests/emu_skm.cpp) -----------------------------------------------------------------------------------------
def build_emu(outdir):
    so = os.path.join(str(outdir), "libemu_skm.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "emu_skm.cpp"), "-o", so])
    L = C.CDLL(so)
    L.emu_skm_part_stats.restype = C.c_int64
    L.emu_skm_part_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def part_stats(emu, reads, K, m127, log2_parts=LOG2_PARTS, lens=None):
    """Per partition id: records, distinct records (payload + the header's low 18 bits), distinct canonical k-mers -> three int64
    arrays of 1 << log2_parts.  reads: an (n, L) code array (with lens: trimmed to them), or a list of 1-D code arrays."""
    from soapdenovo2_amd import api
    P = 1 << log2_parts
    out = [np.zeros(P, dtype=np.int64) for _ in range(3)]
    if isinstance(reads, np.ndarray) and lens is None:
        packed = api.pack_reads_uniform(reads)
        n = emu.emu_skm_part_stats(packed.ctypes.data, None, None, reads.shape[0], reads.shape[1], K, int(m127), log2_parts, *[o.ctypes.data for o in out])
    else:
        if lens is not None:
            reads = [reads[i, :lens[i]] for i in range(len(lens))]
        words, off, _ = api.pack_reads_ragged(reads, K)
        ln = np.array([len(r) for r in reads], dtype=np.int32)
        n = emu.emu_skm_part_stats(words.ctypes.data, off.ctypes.data, ln.ctypes.data, len(reads), int(ln.max()), K, int(m127), log2_parts, *[o.ctypes.data for o in out])
    assert n == out[0].sum() and n > 0, n
    return out


def describe(stats):
    """min / mean / max of the three figures over the partitions that hold a record."""
    live = stats[0] > 0
    return "  ".join(f"{name} {int(s[live].min())} / {s[live].mean():.0f} / {int(s[live].max())}" for name, s in zip(("records", "distinct records", "distinct k-mers"), stats))


# ---- golden cases at 16 partitions: many windows, many key ranges ---------------------------------------------------------------------
MANY = [("t6k_k31", False), ("t8k_k63", False), ("t8k_k63", True), ("t6k_k127", True), ("t5k_k24", False), ("d8k_k63", False)]
AROUND = ("t6k_k31", False, 6)                                   # 64 partitions: their distinct k-mers lie around the set's 2048 slots


def ragged_lens_for(codes, K, seed=29):
    """The same reads trimmed to random lengths in [K + 1, L] (a few at either end of it)."""
    n, L = codes.shape
    lens = np.random.default_rng(seed).integers(K + 1, L + 1, size=n).astype(np.int32)
    lens[:4] = [K + 1, L, K + 1, L]
    return lens


# ---- one window, many key ranges: few reads, low coverage -------------------------------------------------------------------------------
ONE_WINDOW = {                                                   # name -> K, four-word flavour, genome, reads, read length, seed
    "w1_k63": (63, False, 2_000_000, 1500, 150, 101),
    "w1_k127": (127, True, 2_000_000, 360, 400, 102),
}


def one_window_codes(name):
    from soapdenovo2_amd import synth
    K, m127, G, N, L, seed = ONE_WINDOW[name]
    return synth.reads_codes(G, N, L, 0.0, seed), K, m127


# ---- the adaptive search for copies (four-word flavour) -------------------------------------------------------------------------------
ADAPTIVE = {                                                     # name -> genome, reads, read length, grid of the read starts, seed; K = 127
    "dd_off_k127": (2_500_000, 24000, 250, 1, 103),              # about 2x: nearly every record is its own, the search stops
    # 60x.  With reads starting anywhere the two end records of a read are its own at any coverage a test can afford (30x: 78 % of the
    # records distinct); reads that start on a grid of 30 bases come in copies, ends included, and every partition still splits
    "dd_on_k127": (100_000, 24000, 250, 30, 104),
}


def adaptive_codes(name):
    G, N, L, step, seed = ADAPTIVE[name]
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=G, dtype=np.uint8)
    start = rng.integers(0, (G - L) // step + 1, size=N) * step
    codes = genome[start[:, None] + np.arange(L)[None, :]]
    flip = rng.random(N) < 0.5
    codes[flip] = codes[flip, ::-1] ^ 2                          # the other strand
    return np.ascontiguousarray(codes), 127, True


# ---- heavy hitters ---------------------------------------------------------------------------------------------------------------------
A_, C_, T_, G_ = 0, 1, 2, 3
HOT_FWD, HOT_REV = 1100, 600                                     # copies of the homopolymer read and of its complement's
HOT_ALT = 1300                                                   # copies of the alternating read
LEFT_VARIANTS, RIGHT_VARIANTS = (3, 7, 5), (2, 6, 4)             # reads with another first / last base, for the three other bases in code order
ALT_VARIANTS = 9


def _homopolymer_family(base, L):
    """-> (reads, heavy read, hot k-mer's base pattern, designed left arcs, designed right arcs), arcs indexed by base code, 63 = saturated."""
    comp = base ^ 2
    heavy = np.full(L, base, dtype=np.uint8)
    reads = [heavy] * HOT_FWD + [np.full(L, comp, dtype=np.uint8)] * HOT_REV
    canon = min(base, comp)                                      # the node is the homopolymer of the smaller code; the other strand's arcs are complemented
    others = [b for b in range(4) if b != canon]
    left, right = [0] * 4, [0] * 4
    left[canon] = right[canon] = 63
    for b, nl, nr in zip(others, LEFT_VARIANTS, RIGHT_VARIANTS):
        lv = np.full(L, canon, dtype=np.uint8); lv[0] = b
        rv = np.full(L, canon, dtype=np.uint8); rv[-1] = b
        reads += [lv] * nl + [rv] * nr
        left[b], right[b] = nl, nr
    return reads, heavy, [canon], left, right


def _alternating_family(b0, b1, extra, L):
    """(b0 b1)^n with b1 = b0's complement: both k-mers of the read are one node (K is odd), every count goes to one left and one right arc;
    `extra` . (b0 b1)^n a few times adds a second, small left arc beside it."""
    assert b1 == b0 ^ 2 and b0 < b1
    heavy = np.tile(np.array([b0, b1], dtype=np.uint8), L // 2 + 1)[:L].copy()
    var = np.concatenate([[extra], heavy[:L - 1]]).astype(np.uint8)
    reads = [heavy] * HOT_ALT + [var] * ALT_VARIANTS
    left, right = [0] * 4, [0] * 4
    left[b1] = right[b1] = 63                                    # b0 b1 ... b0 is the smaller strand; b1 precedes and follows it
    left[extra] = ALT_VARIANTS
    return reads, heavy, [b0, b1], left, right


def hot_key(pattern, K, nw):
    """Key words of the k-mer pattern[0] pattern[1] ... repeated to K bases (a canonical one): first base in the highest used bits, word 0 the top."""
    v = 0
    for i in range(K):
        v = (v << 2) | int(pattern[i % len(pattern)])
    return [np.uint64((v >> (64 * (nw - 1 - q))) & 0xFFFFFFFFFFFFFFFF) for q in range(nw)]


def heavy_input(K, m127, long_reads=False, seed=7):
    """The mixed heavy-hitter input of one K: four families + background, every read of one length.  -> (codes [n, L], families), families =
    name -> dict(heavy = the heavy read, members = the family's distinct reads, key = the hot node's key words, left / right = its designed arc counters).  long_reads: the poly-A and
    (AT)^n families alone at three records a read, the middle one with both flanks."""
    from soapdenovo2_amd import synth
    n = nmax(K, m127)
    L = K - 1 + (3 * n if long_reads else n)
    fams = {"polyA": _homopolymer_family(A_, L), "AT": _alternating_family(A_, T_, G_, L)}
    if not long_reads:
        fams["polyC"] = _homopolymer_family(C_, L)
        fams["CG"] = _alternating_family(C_, G_, T_, L)
    reads, info = [], {}
    for name, (rs, heavy, pattern, left, right) in fams.items():
        reads += rs
        info[name] = dict(heavy=heavy, members=np.unique(np.stack(rs), axis=0), key=hot_key(pattern, K, nw_of(m127)), left=left, right=right)
    background = synth.reads_codes(30000, 300, L, 0.0, seed + K)
    codes = np.concatenate([np.stack(reads), background])
    return codes[np.random.default_rng(seed).permutation(len(codes))], info


def single_record_input(K, m127, kind, seed=11):
    """2 WIN + 17 copies of one read that is one record of nmax k-mers, and nothing else: the first two windows are WIN exact copies each."""
    L = K - 1 + nmax(K, m127)
    if kind == "polyA":
        read = np.zeros(L, dtype=np.uint8)
    else:                                                        # a tandem repeat with a period below the window length: one minimizer throughout
        rng = np.random.default_rng(seed + K)
        unit = rng.integers(0, 4, size=13).astype(np.uint8)
        while len(set(unit.tolist())) < 3:
            unit = rng.integers(0, 4, size=13).astype(np.uint8)
        read = np.tile(unit, L // 13 + 2)[:L].copy()
    return np.stack([read] * (2 * WIN[nw_of(m127)] + 17))


HEAVY_KS = [(31, False), (25, False), (63, False), (127, True)]      # the kernel for K = 31, the one for any K, K = 63, the four-word flavour
SINGLE = [(31, False, "polyA"), (31, False, "tandem13"), (63, False, "tandem13"), (127, True, "polyA"), (127, True, "tandem13")]


def node_fields(cnt):
    """Export word A | B << 32 -> (coverage, left arcs [4], right arcs [4], single) (kmer.hpp)."""
    a, b = int(cnt) & 0xFFFFFFFF, int(cnt) >> 32
    return (a >> 24) & 0xFF, [(a >> (6 * i)) & 63 for i in range(4)], [(b >> (6 * i)) & 63 for i in range(4)], (b >> 27) & 1


def find_node(records, key, nw):
    hit = np.ones(len(records), dtype=bool)
    for q in range(nw):
        hit &= records[:, q] == key[q]
    idx = np.flatnonzero(hit)
    assert len(idx) == 1, (key, len(idx))
    return records[idx[0]]


def oracle_reads(reads, K, P, prefix, D=0, m127=False, lens=None):
    """Pass 1 through the oracle on a code array (with lens: trimmed) -> (records as the product exports them, last, the .kmerFreq rows)."""
    from oracle_binding import Oracle
    o = Oracle(K, P=P, D=D, mer127=m127, max_read_len=reads.shape[1])
    o.add_reads(reads, lens=lens)
    o.finish_count(prefix)
    nd = o.nodes()
    nw = o.NW
    rec = np.zeros((len(nd["A"]), nw + 2), dtype=np.uint64)
    rec[:, :nw] = nd["keys"]
    rec[:, nw] = nd["A"].astype(np.uint64) | (nd["B"].astype(np.uint64) << np.uint64(32))
    rec[:, nw + 1] = (nd["set"].astype(np.uint64) << np.uint64(56)) | nd["ord"]
    last = np.array(o.set_last_put(), dtype=np.uint64)
    o.close()
    freq = [int(x) for x in open(prefix + ".kmerFreq").read().split()]
    return rec, last, freq
