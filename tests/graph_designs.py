"""Designed topologies for the graph stages after pass 1 (edge construction, tip clipping, read threading): explicit reads over small
molecules with the structures random genomes do not have -- hairpins, rings, tandem repeats, palindromic (K+1)-mers, tips at the clipping
boundary -- and a random generator of bushes of nested tips.  Everything is deterministic in (design, K); every length is a function of K
(a free end of fewer than 2 K nodes is clipped, so flanks are 3 K + 20 bases and reads 2 K + 40).  tests/golden/make_graph_designs_golden.py
runs the reference on these reads and writes tests/golden/graph_designs_golden.py; tests/test_graph_designs_host.py and
tests/test_gpu_graph_designs.py hold the host stages and the device stages to it.

Base codes as everywhere here: A C T G = 0 1 2 3, the complement is code ^ 2."""
import os
import zlib

import numpy as np

A_, C_, T_, G_ = 0, 1, 2, 3


def rc(x):
    return (np.asarray(x, dtype=np.uint8)[::-1] ^ 2).astype(np.uint8)


def read_len(K):
    return 2 * K + 40


def flank_len(K):
    return 3 * K + 20


def max_rd_len(K):
    """max_rd_len of the config: the longest designed read is a tip's (20 bases of trunk, the junction k-mer, 2 K + 5 branch bases)."""
    return 3 * K + 40


class Reads(list):
    """A design's reads (uint8 code arrays, ragged) with what the golden generator asserts about them in `facts`."""

    def __init__(self, reads=(), facts=None):
        super().__init__(reads)
        self.facts = dict(facts or {})


def _rng(design, K, seed=0):
    return np.random.default_rng([zlib.crc32(design.encode()), K, seed])


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]).astype(np.uint8)


def _other(rng, *avoid):
    """A base that is none of `avoid`."""
    return int(rng.choice([b for b in range(4) if b not in avoid]))


def tile(seq, K, circular=False):
    """Reads of read_len(K) over `seq` at a stride of a fifth of their length, each with its reverse complement: coverage 10 away from the
    ends.  A linear molecule gets a last window flush with its end (one shorter than a read: the whole molecule, five times); a circular one
    is tiled across its origin."""
    seq = np.asarray(seq, dtype=np.uint8)
    RL, n = read_len(K), len(seq)
    stride = RL // 5
    out = []
    if circular:
        wrap = _cat(seq, seq[:RL])
        wins = [wrap[s:s + RL] for s in range(0, n, stride)]
    elif n <= RL:
        wins = [seq] * 5
    else:
        starts = list(range(0, n - RL, stride)) + [n - RL]
        wins = [seq[s:s + RL] for s in starts]
    for w in wins:
        out += [w.copy(), rc(w)]
    return out


def copies(rng, read, mult):
    """`mult` copies of one read, each on a random strand."""
    return [rc(read) if rng.random() < 0.5 else np.asarray(read, dtype=np.uint8).copy() for _ in range(mult)]


def canonical(kmer):
    """Is the k-mer not larger than its reverse complement (first base most significant, A < C < T < G)?"""
    return tuple(kmer) <= tuple(rc(kmer))


# ---- the designs ------------------------------------------------------------------------------------------------------------------------
def hairpin(K):
    """Edge builder's keep rule and palindrome test (eb_walk: "unless its other entrance precedes its own", twin == own) and the waypoint
    segments passed in both directions (vis_own[2h + d]): a chain that ends at the reverse complement of its start.  Three molecules:
    F1 + A + rc(A) + F2 with different flanks (every node of A is walked twice, there and back); B + rc(B) alone, a molecule that is its own
    reverse complement; and a stem of K - 3 bases, shorter than K, where only the k-mers inside the 2 (K - 3) palindrome come in pairs."""
    rng = _rng("hairpin", K)
    r = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    F = flank_len(K)
    a = r(2 * K + 10)
    b = r(F)
    s = r(K - 3)
    out = Reads()
    out += tile(_cat(r(F), a, rc(a), r(F)), K)
    out += tile(_cat(b, rc(b)), K)
    out += tile(_cat(r(F), s, rc(s), r(F)), K)
    return out


def ring(K):
    """Chains without a branch node.  A circular molecule of 400 + 3 K bases has no vertex: no edge walk starts on it, a waypoint's segment
    can only end at a waypoint (its own included), and pass 2 meets "deleted, or on a floating loop" (p2_thread_kernel) for every read that
    lies on it -- beside one linear molecule, so that the files are not empty.  A second ring carries one tail: its vertex lies on the ring,
    and the ring is an edge that starts and ends at the same vertex."""
    rng = _rng("ring", K)
    r = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    n = 400 + 3 * K
    free, tailed = r(n), r(n)
    out = Reads()
    on_ring = tile(free, K, circular=True)
    out += on_ring
    out += tile(r(2 * flank_len(K)), K)
    out += tile(tailed, K, circular=True)
    at = 100
    tail = r(flank_len(K))
    tail[0] = _other(rng, tailed[at + K + 20])
    out += tile(_cat(tailed[at:at + K + 20], tail), K)
    out.facts["reads_on_free_ring"] = len(on_ring)
    return out


def tandem(K):
    """Chains that pass through the same node twice: tandem repeats between random flanks.  2.5 copies of a unit of 4 K, K + 1, K and K - 1
    bases (the last three close a cycle of K + 1, K, K - 1 nodes that the flanks enter and leave); runs of 2 K + 9 bases of period 3, of
    period 2 (AT: at odd K the successor of ATA..A is its own reverse complement) and of period 1 (the all-A node with an arc to itself)."""
    rng = _rng("tandem", K)
    r = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    F = flank_len(K)
    out = Reads()
    for u in (4 * K, K + 1, K, K - 1):
        unit = r(u)
        out += tile(_cat(r(F), unit, unit, unit[:u // 2], r(F)), K)
    for unit in ((A_, C_, G_), (A_, T_), (A_,)):
        run = np.resize(np.array(unit, dtype=np.uint8), 2 * K + 9)
        left, right = r(F), r(F)
        left[-1] = _other(rng, unit[-1])                              # the flanks do not prolong the run
        right[0] = _other(rng, unit[(2 * K + 9) % len(unit)])
        out += tile(_cat(left, run, right), K)
    return out


def pal_plus(K):
    """The palindrome test where it is decided by one arc: H + rc(H) with |H| = (K + 1) / 2 is a palindromic (K+1)-mer, the arc from a
    k-mer x to rc(x), i.e. from a node to itself.  Between flanks whose bases next to it are complementary, x has one way in and one way
    out and the chain passes it twice; with other flanks x is a branch node (two ways in, rc's two ways out are the same two arcs) and the
    (K+1)-mer joins a branch node with itself: a length-1 edge that is its own twin, if the reference makes one."""
    rng = _rng("pal_plus", K)
    r = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    F = flank_len(K)
    out = Reads()
    for branch in (False, True):
        h = r((K + 1) // 2)
        left, right = r(F), r(F)
        right[0] = _other(rng, left[-1] ^ 2) if branch else left[-1] ^ 2
        out += tile(_cat(left, h, rc(h), right), K)
    return out


TIP_LENGTHS = ("1", "K", "2K-1", "2K", "2K+1")


def _tip_len(name, K):
    return {"1": 1, "K": K, "2K-1": 2 * K - 1, "2K": 2 * K, "2K+1": 2 * K + 1}[name]


def _branch_off(rng, trunk, p, K, n, avoid=(), anchor=20):
    """A dead-end branch of n k-mers that leaves trunk's k-mer at p to the right: the read (`anchor` bases of trunk before the junction k-mer,
    the k-mer, n bases that differ from the trunk's at the first) and the n bases."""
    tipb = rng.integers(0, 4, size=n, dtype=np.uint8)
    tipb[0] = _other(rng, trunk[p + K], *avoid)
    return _cat(trunk[p - anchor:p + K], tipb), tipb


def tips(K):
    """Tip clipping as a fixed point over start decisions (dev_tips.hpp) where the candidates interact and at its boundaries.  Off a trunk of
    coverage 10: dead-end branches of exactly 1, K, 2 K - 1, 2 K and 2 K + 1 k-mers, each once (all its k-mers of frequency one: the first pass)
    and twice (the pass of the minority links), leaving junction k-mers that are canonical and that are not; two tips at one junction; tips on
    tips on a tip, so that clipping takes several cycles.  Off a trunk whose arcs all count 2: a branch that counts 2 as well, a tie.  Alone: a Y
    whose three arms are all shorter than 2 K, and a molecule of fewer than 2 K nodes.  facts["probes"]: name -> 20 bases of a branch (or their
    reverse complement) that some edge holds if and only if the branch survived."""
    rng = _rng("tips", K)
    r = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    F, gap = flank_len(K), 3 * K + 20
    out = Reads()
    probes = {}
    # the branches of the five lengths, once and twice
    jobs = [(ln, mult) for mult in (1, 2) for ln in TIP_LENGTHS]
    trunk = r(F + gap * len(jobs) + F)
    seen = {True: 0, False: 0}
    extra = []
    for j, (ln, mult) in enumerate(jobs):
        want = j % 2 == 0                                   # junction k-mers canonical and not, in turn (the nearest such place)
        p = F + gap * j
        while canonical(trunk[p:p + K]) != want:
            p += 1
        seen[want] += 1
        n = _tip_len(ln, K)
        read, tipb = _branch_off(rng, trunk, p, K, n)
        extra += copies(rng, read, mult)
        if n >= K + 20:
            probes["%s_x%d" % (ln, mult)] = tipb[:20]
    assert seen[True] and seen[False]
    out += tile(trunk, K) + extra
    # two tips at one junction; tips on tips on a tip
    trunk = r(F + gap * 7 + F)
    extra = []
    p = F
    read_a, tip_a = _branch_off(rng, trunk, p, K, K // 2)
    read_b, _ = _branch_off(rng, trunk, p, K, K, avoid=(int(tip_a[0]),))
    extra += copies(rng, read_a, 2) + copies(rng, read_b, 3)
    for j in range(1, 7):
        # a branch of K + 9 k-mers (5 times); on it, 7 + j k-mers out, one of 12 (3 times); on that, 5 k-mers out, one of 5 (twice).  The reads of
        # the upper two start with their junction k-mer, so every arc counts what its own branch does: 2 < 3 < 5 < 10, each is clipped once the one
        # on it is gone
        host, _ = _branch_off(rng, trunk, F + gap * j, K, K + 9)
        extra += copies(rng, host, 5)
        host, _ = _branch_off(rng, host, 20 + 7 + j, K, 12, anchor=0)
        extra += copies(rng, host, 3)
        host, _ = _branch_off(rng, host, 5, K, 5, anchor=0)
        extra += copies(rng, host, 2)
    out += tile(trunk, K) + extra
    # a tie: every arc of this trunk counts 2 (windows that overlap by K bases, there and back), and so does the branch
    trunk = r(2 * F + K)
    thin = []
    at = 0
    while at + K < len(trunk):                                           # consecutive windows share exactly K bases: every (K+1)-mer lies in one
        w = trunk[at:at + read_len(K)]
        thin += [w.copy(), rc(w)]
        at += len(w) - K
    read, tipb = _branch_off(rng, trunk, F, K, K + 20)
    probes["tie"] = tipb[:20]
    out += thin + copies(rng, read, 2)
    # a Y whose arms are all shorter than 2 K, and a molecule of fewer than 2 K nodes
    stem = r(2 * K)
    y1, y2 = r(K + 5), r(K + 9)
    y2[0] = _other(rng, y1[0])
    out += copies(rng, _cat(stem, y1), 3) + copies(rng, _cat(stem, y2), 2)
    out += copies(rng, r(2 * K + 20), 3)
    out.facts["probes"] = {k: [int(x) for x in v] for k, v in probes.items()}
    return out


BUSH_SEEDS = {31: (1, 2, 3, 4, 5, 6), 63: (1, 2), 127: (1, 2)}


def bush(seed, K):
    """Random interacting tips for the tip stage and for the edges of what it leaves: 3 - 30 trunks of K + 2 ... 6 K bases, each with up to 7
    branches of 1 ... 2 K + 5 k-mers that leave or join at a random place of the trunk or of an earlier branch (nested), 1 - 3 times, every copy
    on a random strand."""
    rng = _rng("bush", K, seed)
    r = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    out = Reads()
    for _ in range(int(rng.integers(3, 31))):
        trunk = r(int(rng.integers(K + 2, 6 * K + 1)))
        out += tile(trunk, K)
        hosts = [trunk]
        for _ in range(int(rng.integers(0, 8))):
            host = hosts[int(rng.integers(0, len(hosts)))]
            p = int(rng.integers(0, len(host) - K + 1))
            n = int(rng.integers(1, 2 * K + 6))
            anchor = int(rng.integers(0, 21))
            tipb = r(n)
            if rng.random() < 0.5:                                       # leaves the k-mer at p to the right
                if p + K < len(host):
                    tipb[0] = _other(rng, host[p + K])
                read = _cat(host[max(0, p - anchor):p + K], tipb)
            else:                                                        # joins it from the left
                if p > 0:
                    tipb[-1] = _other(rng, host[p - 1])
                read = _cat(tipb, host[p:p + K + anchor])
            out += copies(rng, read, int(rng.integers(1, 4)))
            hosts.append(read)
    return out


SINGLE_DESIGNS = {"hairpin": hairpin, "ring": ring, "tandem": tandem, "pal_plus": pal_plus, "tips": tips}


def all_designs(K):
    """Every design above but the bushes, as separate molecules of one input: what the variants of the command run on, one launch for all."""
    out = Reads()
    for name, f in SINGLE_DESIGNS.items():
        d = f(K)
        out += d
        out.facts.update(d.facts)
    return out


def design(name, K):
    """The reads of a design by name: one of SINGLE_DESIGNS, "all", or "bush<seed>"."""
    if name == "all":
        return all_designs(K)
    if name.startswith("bush"):
        return bush(int(name[4:]), K)
    return SINGLE_DESIGNS[name](K)


# ---- the runs ---------------------------------------------------------------------------------------------------------------------------
FLAVOURS = ((31, 0), (63, 0), (63, 1), (127, 1))                         # (K, 127-mer binary?)
WITH_D1 = ("tips", "all")                                                # -d 1 as well: no frequency-one pass, the minor pass sees the raw graph


def rows():
    """Every (design, K, mer127, P, D) the reference ran, always with -R."""
    out = []
    for K, m in FLAVOURS:
        names = list(SINGLE_DESIGNS) + ["all"] + ["bush%d" % s for s in BUSH_SEEDS[K]]
        for name in names:
            for P in (1, 3):
                for D in (0, 1) if (name in WITH_D1 or name.startswith("bush")) else (0,):
                    out.append((name, K, m, P, D))
    return out


def row_tag(row):
    name, K, m, P, D = row
    return "%s_k%d_%s_p%d_d%d" % (name, K, "127" if m else "63", P, D)


SEVEN = ("kmerFreq", "preGraphBasic", "vertex", "edge", "preArc", "path", "markOnEdge")


# ---- helpers of the tests and of the golden generator ---------------------------------------------------------------------------------------
def write_case(outdir, name, reads, K):
    """<outdir>/<name>.fq and <name>.cfg for the command (config grammar as synth.make_quirk_case); returns the config path."""
    from soapdenovo2_amd import synth
    os.makedirs(outdir, exist_ok=True)
    fq = os.path.abspath(os.path.join(outdir, name + ".fq"))
    blob = b"".join(synth._fastq_blob(list(reads), [b"r%d" % i for i in range(len(reads))]))
    if len(blob) % 32768 == 0:                                           # (the reference drops the tail of such a file, prlHashReads.c:873-877)
        blob = blob[:-1] + b" \n"
    with open(fq, "wb") as f:
        f.write(blob)
    cfg = os.path.abspath(os.path.join(outdir, name + ".cfg"))
    with open(cfg, "w") as f:
        f.write("max_rd_len=%d\n[LIB]\navg_ins=200\nasm_flags=3\nq=%s\n" % (max_rd_len(K), fq))
    return cfg


def codes_and_lens(reads, K):
    """The ragged reads as the (n, max_rd_len) array and the lengths the oracle and api.host_pregraph_files take."""
    codes = np.zeros((len(reads), max_rd_len(K)), dtype=np.uint8)
    lens = np.array([len(x) for x in reads], dtype=np.int32)
    for i, x in enumerate(reads):
        codes[i, :len(x)] = x
    return codes, lens


def oracle_records(codes, lens, K, P, D=0, mer127=False, prefix=None):
    """conftest.oracle_records for ragged reads: pass 1 through the oracle in the product's record format; writes <prefix>.kmerFreq."""
    from oracle_binding import Oracle
    o = Oracle(K, P=P, D=D, mer127=mer127, max_read_len=codes.shape[1])
    o.add_reads(codes, lens=lens)
    o.finish_count(prefix if prefix else os.devnull[:-4] + "null")
    nd = o.nodes()
    nw = o.NW
    rec = np.zeros((len(nd["A"]), nw + 2), dtype=np.uint64)
    rec[:, :nw] = nd["keys"]
    rec[:, nw] = nd["A"].astype(np.uint64) | (nd["B"].astype(np.uint64) << np.uint64(32))
    rec[:, nw + 1] = (nd["set"].astype(np.uint64) << np.uint64(56)) | nd["ord"]
    last = np.array(o.set_last_put(), dtype=np.uint64)
    o.close()
    return rec, last


_golden = None


def golden_rows():
    """tests/golden/graph_designs_golden.py: ROWS (row_tag -> digests and counts of the reference) and EDGE_TEXT (some rows' edge files)."""
    global _golden
    if _golden is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_designs_golden.py")
        g = {}
        exec(compile(open(path).read(), path, "exec"), g)
        _golden = (g["ROWS"], {t: "".join(lines) for t, lines in g["EDGE_TEXT"].items()})
    return _golden


_records = {}


def row_inputs(row, workdir):
    """Pass 1 of a row through the oracle, once a session: (codes, lens, records, last puts, prefix of the oracle's .kmerFreq)."""
    name, K, m, P, D = row
    if row not in _records:
        codes, lens = codes_and_lens(design(name, K), K)
        pre = os.path.join(str(workdir), "o_" + row_tag(row))
        rec, last = oracle_records(codes, lens, K, P, D=D, mer127=bool(m), prefix=pre)
        for a in (codes, lens, rec, last):
            a.setflags(write=False)
        _records[row] = (codes, lens, rec, last, pre)
    return _records[row]


def seven_digests(prefix, kmerfreq_of=None):
    """md5 of the seven files of a -R run, the edge file decompressed (gzip's bytes depend on the zlib build).  kmerfreq_of: the prefix
    the .kmerFreq lies under, where pass 1 was another's."""
    from conftest import md5_file, md5_gz_text
    out = {e: (md5_gz_text(prefix + ".edge.gz") if e == "edge" else md5_file((kmerfreq_of if e == "kmerFreq" and kmerfreq_of else prefix) + "." + e))
           for e in SEVEN}
    return out


def tip_hook(entry, rec, last, K, m, P, D, *lead):
    """pg_host_emu_clip_tips / pg_device_emu_clip_tips: (single, minor) of the sequential scan, (single, minor) of the device stage, nodes that
    differ, fixed-point rounds, minor cycles.  lead: the device for the device hook; the host hook's thread count goes last."""
    from soapdenovo2_amd import api
    rec = np.ascontiguousarray(rec)
    out = np.zeros(8, dtype=np.uint64)
    L = api.lib()
    if entry == "host":
        rc = L.pg_host_emu_clip_tips(rec.ctypes.data, len(rec), last.ctypes.data, K, int(bool(m)), P, int(D == 0), 0, lead[0], out.ctypes.data)
    else:
        rc = L.pg_device_emu_clip_tips(lead[0], rec.ctypes.data, len(rec), last.ctypes.data, K, int(bool(m)), P, int(D == 0), 0, out.ctypes.data)
    assert rc == 0, L.pg_last_error()
    single_seq, minor_seq, single_dev, minor_dev, diff, rounds, cycles = (int(x) for x in out[:7])
    return (single_seq, minor_seq), (single_dev, minor_dev), diff, rounds, cycles
