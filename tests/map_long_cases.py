"""Inputs of the long-read pass's tests (prlLongRead2Ctg, standardPregraph/prlRead2Ctg.c:1080): the decision restated in linear time,
reads constructed for the edges of the wave-per-read kernel (csrc/map_kernels.hip: map_read_wave_kernel), and configs with
asm_flags=4 libraries for the command.

tests/test_map_long_host.py runs them on the host twin, tests/test_gpu_map_long.py on the device; tests/golden/
make_map_long_golden.py records the reference binary's md5s of the command cases."""
import functools
import gzip
import hashlib
import os

import numpy as np

from soapdenovo2_amd import synth

import map_cases as M
import map_edge_cases as E
import map_model as MM

LONG_OUTPUTS = ["longReadInGap", "RlongReadInGap"]


# ---------------------------------------------------------------------------------------------------------
# the decision in linear time
# ---------------------------------------------------------------------------------------------------------
def decide_linear(row, read_len, K, align_len, id_len, id_bal):
    """map_model.decide's answer from one pass over the row: per distinct id its number of hits and its first hit.  The ids that count,
    the footprint and the winner (most hits among the ids with `multi` or more, the earliest first hit among equals: the first in
    first-hit order with strictly the most) depend on nothing else.  test_map_long_host.py holds it equal to map_model.decide on every
    case of map_edge_cases; alone it serves the reads with thousands of ids, where the model's quadratic form takes minutes."""
    if not row:
        return (0, 0, 0, 0)
    multi = max(2, min(read_len, align_len) - K + 1)
    seen = {}
    for j, h in enumerate(row):
        if h is None:
            continue
        e = seen.get(h[0])
        if e is None:
            seen[h[0]] = [1, j]
        else:
            e[0] += 1
    footprint_ids = sum(1 for n, _ in seen.values() if K > 32 or (K < 32 and n >= 2))
    mapped = [(n, j) for n, j in seen.values() if n >= multi]
    if not mapped:
        return (0, 0, 0, 0)
    _, best_at = min(mapped, key=lambda e: (-e[0], e[1]))
    cid, pos, twin, smaller = row[best_at]
    ordinal = best_at + 1
    known = cid < len(id_len)
    fp = 1 if footprint_ids > 1 else 0
    if twin == smaller:
        length = int(id_len[cid]) if known else 0
        bal = int(id_bal[cid]) if known else 1
        return ((cid + bal - 1) & MM.M32, MM._s32(length - pos - K - ordinal + 1), ord("-"), fp)
    return (cid, MM._s32(pos - ordinal + 1), ord("+"), fp)


def distinct_ids(row):
    return len({h[0] for h in row if h is not None})


# ---------------------------------------------------------------------------------------------------------
# constructed reads: the wave kernel's edges, on map_edge_cases' contig builders
# ---------------------------------------------------------------------------------------------------------
FLAVOURS = [(21, False), (31, False), (63, False), (75, True), (127, True)]
BIG_IDS_FLAVOURS = [(31, False), (75, True)]                # (the reads of 2C + 3 contigs: one K a flavour, one below 32 and one above)
LANE_MAX_KMERS = 1300                                       # the lane kernel's scan is quadratic in one lane: reads past this many
#                                                             k-mers are held against the model only (at 4 097 k-mers and 130 ids a
#                                                             lane spends ~8e6 dependent row loads on one read)


def guarded(s, a, n):
    """Bases a .. a + n - 1 of a contig (a >= 1) with one base on either side that differs from the contig's there: exactly n - K + 1
    k-mers of it hit, whatever stands next to the piece."""
    return E.cat([(int(s[a - 1]) + 1) & 3], s[a:a + n], [(int(s[a + n]) + 1) & 3])


def _case(K, mer127, capacity):
    """Contigs and reads of one flavour.  capacity = api.map_wave_ids(): the ids the kernel's LDS table holds."""
    case = E.Case("long", K, mer127, golden=False)
    rng = np.random.default_rng(1000 + K)
    p, q = E._basics(case, rng)
    rand = lambda n: E._rand(rng, n)
    piece = lambda s, hits, a: guarded(s, a, K + hits - 1)         # exactly `hits` k-mers
    # one long contig for the lane-stretch edges: a read of nk k-mers is cut from it
    big_n = 4097 + K + 40
    big = case.contig(rand(big_n), case.pair(big_n))
    other = [case.contig(rand(3 * K + 90), case.pair(3 * K + 90)) for _ in range(4)]
    for nk in (1, 2, 63, 64, 65, 127, 128, 129, 4097):
        ln = nk + K - 1
        if nk == 1:
            ln = K                                          # K bases: no k-mer by the reference's rule (nk = 0) ...
        case.read(big[7:7 + ln], "nk%d" % (0 if nk == 1 else nk))
        case.read(E.rc(big[9:9 + ln]), "nk%d-rc" % (0 if nk == 1 else nk))
    case.read(big[3:3 + K + 1], "nk2-again")                # ... and K + 1 bases: the shortest read with k-mers (two)
    # a winner whose first hit lies in the last lane's stretch (k-mers 63 * nk / 64 on): junk, then nk / 64 k-mers of a contig at the end
    for nk in (1280, 2560):
        tail = piece(other[0], nk // 64, 5)[:-1]              # (the read ends with the piece's last k-mer)
        case.read(E.cat(rand(nk + K - 1 - len(tail)), tail), "winner-in-last-lane-nk%d" % nk)
    # two ids with equal counts, first hits in different lanes' stretches, in both orders; and one more hit for the later one
    gap = rand(300)
    a, b = other[1], other[2]
    case.read(E.cat(piece(a, 20, 3), gap, piece(b, 20, 8)), "tie-a-b-far-apart")
    case.read(E.cat(piece(b, 20, 8), gap, piece(a, 20, 3)), "tie-b-a-far-apart")
    case.read(E.cat(piece(a, 20, 3), gap, piece(b, 21, 8)), "later-one-more")
    case.read(E.cat(E.rc(piece(a, 21, 3)), gap, piece(b, 20, 8)), "earlier-one-more-rc")
    case.read(E.cat(piece(a, 12, 3), gap[:150], piece(b, 20, 8), gap[150:], piece(a, 8, 40)), "a-split-around-b-ties")
    # flag = multi - 1 / multi (ALIGNLEN 40 and 60 are run), then junk over several lanes' stretches
    for A in (40, 60):
        if A <= K:
            continue
        case.read(E.cat(gap[:200], piece(other[3], A - K + 1, 2), gap[200:]), "multi-exact-A%d" % A)
        case.read(E.cat(gap[:200], piece(other[3], A - K, 2), gap[200:]), "multi-less-one-A%d" % A)
    # single-hit ids: they count towards the footprint only when K > 32
    case.read(E.cat(piece(a, 30, 3), gap[:100], piece(b, 1, 8), gap[100:200], piece(other[3], 1, 11)), "footprint-single-hit-ids")
    case.read(E.cat(piece(a, 30, 3), gap[:100], piece(b, 2, 8)), "footprint-two-hit-id")
    return case, p


def insert_steps(row):
    """{id: the trip of the wave kernel's lookup loop in which the id is first brought to the table}.  Lane l takes k-mers
    l * per .. (l + 1) * per - 1 with per = ceil(nk / 64), all lanes in step, so k-mer j is looked up in trip j % per.  Restated here
    only so that a test can assert which id comes last; no answer depends on it."""
    per = (len(row) + 63) // 64
    steps = {}
    for j, h in enumerate(row):
        if h is not None:
            steps[h[0]] = min(steps.get(h[0], per), j % per)
    return steps


def _last_inserted_wins(many, m, K, rng):
    """A read of m ids whose winner is brought to the table in a later trip than every other id, so that a table which takes the first
    ids it meets and drops the rest drops the winner.  The read has 64 * q * U k-mers (U = K + 4, a three-hit piece with its guards), so
    a lane's stretch is q * U k-mers; m - 1 contigs give one three-hit piece each, in units of U bases from the read's start (their
    first hits come in trips 1, U + 1, ... (q - 1) * U + 1), and the winner's seven hits are the last seven k-mers of a stretch
    (trip q * U - 7).  Junk fills the rest."""
    U = K + 4
    q = (m + 1 + 63) // 64
    per = q * U
    nk = 64 * per
    read = E._rand(rng, nk + K - 1)
    for i in range(m - 1):
        read[i * U:(i + 1) * U] = guarded(many[i], 4, K + 2)
    end = per * (((m - 1) * U + 8 + per - 1) // per)         # the first stretch end with room for the winner after the others
    w = guarded(many[m - 1], 2, K + 6)
    w = w[:min(len(w), len(read) - (end - 8))]               # (at the read's end there is no base left for the second guard)
    read[end - 8:end - 8 + len(w)] = w
    return read


@functools.lru_cache(maxsize=None)
def constructed(K, mer127, capacity, big_ids):
    """(case, model index inputs, hit rows).  big_ids: with the reads made of K + 2-base pieces of C - 1, C, C + 1 and 2C + 3 contigs
    (C = capacity), once all tied (the first wins) and once with the winner among the ids past the C-th."""
    case, p = _case(K, mer127, capacity)
    if big_ids:
        rng = np.random.default_rng(2000 + K)
        C = capacity
        n = K + 12
        many = [case.contig(E._rand(rng, n), case.pair(n)) for _ in range(2 * C + 3)]
        for m in (C - 1, C, C + 1, 2 * C + 3):
            three = lambda i: guarded(many[i], 4, K + 2)    # a K + 2-base piece: three k-mers
            case.read(E.cat(*[three(i) for i in range(m)]), "ids%d-tied" % m)
            case.read(E.cat(*[three(i) for i in reversed(range(m))]), "ids%d-tied-reversed" % m)
            late = [three(i) for i in range(m)]
            late[m - 1] = guarded(many[m - 1], 2, K + 6)    # the last id has the most hits: only a decision that counts every id sees it
            case.read(E.cat(*late), "ids%d-last-wins" % m)
            late = [three(i) for i in range(m)]
            late[m - 2] = E.rc(guarded(many[m - 2], 2, K + 6))
            case.read(E.cat(*late), "ids%d-last-but-one-wins-rc" % m)
            case.read(_last_inserted_wins(many, m, K, rng), "ids%d-last-inserted-wins" % m)
    ctgs, ids, length, bal = E.loaded(case)
    index = MM.build_index(ctgs, ids, K)
    rows = [MM.hit_row(index, rd, K) for rd in case.reads]
    return case, (ctgs, ids, length, bal), rows


def model_out(case, tables, rows, align_len):
    _, _, length, bal = tables
    return [decide_linear(row, len(rd), case.K, align_len, length, bal) for row, rd in zip(rows, case.reads)]


def product(tables, reads, K, mer127, align_len, device, lane=False):
    """(rows, tuples) from api.map_long_reads (the wave kernel; device = -1: the host twin) or, with lane=True, api.map_hits."""
    from soapdenovo2_amd import api
    ctgs, ids, length, bal = tables
    if lane:
        ctg, pos, ori, fp, rows, koff = api.map_hits(ctgs, ids, length, bal, reads, K, align_len, mer127, device=device)
    else:
        ctg, pos, ori, fp, rows, koff = api.map_long_reads(ctgs, ids, length, bal, reads, K, align_len, mer127, device=device, want_hits=True)
    assert len(koff) == len(reads) + 1 and int(koff[-1]) == len(rows)
    rows = [[int(w) for w in rows[int(koff[r]):int(koff[r + 1])]] for r in range(len(reads))]
    return rows, [(int(ctg[r]), int(pos[r]), int(ori[r]), int(fp[r])) for r in range(len(reads))]


def align_lens(K):
    """ALIGNLEN 40 and 60 (the long pass's own are 35 or more), and K + 1: multi = 2, with which a K + 2-base piece's three hits map."""
    return [40, 60, K + 1]


def check_constructed(case, rows, want40, want_k1, capacity, big_ids):
    """What keeps the comparison from passing vacuously, on the model's own output (at ALIGNLEN 40 and K + 1)."""
    tag = dict(zip(case.tags, range(len(case.tags))))
    K = case.K
    assert rows[tag["nk0"]] == [] and len(rows[tag["nk4097"]]) == 4097 and len(rows[tag["nk65"]]) == 65
    for nm in ("winner-in-last-lane-nk1280", "winner-in-last-lane-nk2560"):
        r = tag[nm]
        nk = len(rows[r])
        first = next(j for j, h in enumerate(rows[r]) if h is not None and h[0] == want40[r][0])
        assert want40[r][0] and first >= 63 * ((nk + 63) // 64), nm
    r1, r2 = tag["tie-a-b-far-apart"], tag["tie-b-a-far-apart"]
    assert want40[r1][0] and want40[r2][0] and want40[r1][0] != want40[r2][0]
    assert want40[tag["later-one-more"]][0] == want40[r2][0] and want40[tag["later-one-more"]][0] != want40[r1][0]
    if 40 > K:
        assert want40[tag["multi-exact-A40"]][0] and not want40[tag["multi-less-one-A40"]][0]
    assert want40[tag["footprint-single-hit-ids"]][3] == (1 if K > 32 else 0)
    assert want40[tag["footprint-two-hit-id"]][3] == 1
    if big_ids:
        C = capacity
        for m in (C - 1, C, C + 1, 2 * C + 3):
            assert distinct_ids(rows[tag["ids%d-tied" % m]]) == m
            first_id = next(h[0] for h in rows[tag["ids%d-tied" % m]] if h is not None)
            assert want_k1[tag["ids%d-tied" % m]][0] == first_id
            last = tag["ids%d-last-wins" % m]
            last_id = [h[0] for h in rows[last] if h is not None][-1]
            assert want_k1[last][0] == last_id != first_id, m
            r = tag["ids%d-last-inserted-wins" % m]
            steps = insert_steps(rows[r])
            winner = want_k1[r][0]
            assert len(steps) == m and winner in steps and all(st < steps[winner] for cid, st in steps.items() if cid != winner), m


def low_bits_case(K, mer127, capacity):
    """The many-id reads with every contig id multiplied by 64 (ids past the id tables: length 0, bal 1): all ids agree in their six low
    bits, so no split into classes by id % P helps and the kernel ends in its wave-wide scan.  (tables, reads, tags, rows)"""
    case, (ctgs, ids, length, bal), _ = constructed(K, mer127, capacity, True)
    ids = (ids.astype(np.uint64) * 64).astype(np.uint32)
    keep = [r for r, t in enumerate(case.tags) if t.startswith("ids") or t.startswith("basic")]
    reads = [case.reads[r] for r in keep]
    index = MM.build_index(ctgs, ids, K)
    return (ctgs, ids, length, bal), reads, [case.tags[r] for r in keep], [MM.hit_row(index, rd, K) for rd in reads]


def batch_shapes(case):
    """Batches of 0, 1, 3, 4 and 5 reads (a workgroup holds four), and one in which reads 1 and 2 of a workgroup have no k-mers."""
    K = case.K
    tag = dict(zip(case.tags, range(len(case.tags))))
    pool = [case.reads[tag[t]] for t in ("nk129", "tie-a-b-far-apart", "nk65-rc", "later-one-more", "basic-footprint", "nk64")]
    short = pool[0][:K]
    return {"n0": [], "n1": pool[:1], "n3": pool[:3], "n4": pool[:4], "n5": pool[:5],
            "kmerless-1-2": [pool[0], short, short[:K - 3], pool[1], pool[2], short, pool[3]],
            "all-kmerless": [short, short, short, short, short]}


# ---------------------------------------------------------------------------------------------------------
# the command: configs with long-read libraries
# ---------------------------------------------------------------------------------------------------------
# name: (flavour 127?, graph K, map -k or 0, -p, -f, short-read layout of map_cases.write_libs, long layout)
CASES = {
    "l31_p1":        (False, 31, 0, 1, False, "pairs", "after"),
    "l31_p3_f":      (False, 31, 0, 3, True, "pairs", "after"),
    "l31_k25_p8_f":  (False, 31, 25, 8, True, "pairs", "two"),
    "l31_batches":   (False, 31, 0, 3, True, "pairs", "batches"),
    "m127_k75_p3_f": (True, 75, 0, 3, True, "pairs", "nocut"),
    "l31_bam_p3_f":  (False, 31, 0, 3, True, "pairs", "bam"),
}
P_PAIR = ("l31_p1", "l31_p3_f")                             # the same inputs at two -p values: .longReadInGap must differ


def long_reads(n, lo, hi, seed, err=0.01):
    """n reads of lo .. hi bases cut from map_cases' genome, either strand, with substitution errors."""
    g = M.genome()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        a = int(rng.integers(0, len(g) - ln))
        s = g[a:a + ln].copy()
        flip = rng.random(ln) < err
        s[flip] = (s[flip] + rng.integers(1, 4, size=int(flip.sum()))) & 3
        out.append(E.rc(s) if rng.random() < 0.5 else s)
    return out


def _text(s):
    return np.frombuffer(b"ACTG", dtype=np.uint8)[np.asarray(s, dtype=np.intp)].tobytes().decode()


def write_fasta(path, reads, width=0, prefix="L"):
    with open(path, "w") as f:
        for i, s in enumerate(reads):
            t = _text(s)
            if i % 9 == 4:
                t = t.lower()
            f.write(">%s%d\n" % (prefix, i))
            for a in range(0, len(t), width or max(len(t), 1)):
                f.write(t[a:a + (width or len(t))] + "\n")


def write_fastq(path, reads, prefix="Q"):
    with open(path, "w") as f:
        for i, s in enumerate(reads):
            t = _text(s)
            if i % 7 == 3 and len(t) > 20:
                t = t[:17] + "N" + t[18:]
            f.write("@%s%d\n%s\n+\n%s\n" % (prefix, i, t, "I" * len(t)))


def write_long_libs(d, cfg, layout):
    """Adds the asm_flags=4 libraries of a layout to the config map_cases.write_libs wrote (short libraries: "pairs")."""
    p = lambda f: os.path.join(d, f)
    text = open(cfg).read()
    head, libs = text.split("[LIB]", 1)
    libs = ["[LIB]" + x for x in libs.split("[LIB]")]
    if layout == "after":
        # 301 + 100 reads: the last read chopped by thread 0 is read 400 at -p 1 and read 399 at -p 3
        write_fasta(p("long.fa"), long_reads(301, 200, 1500, 41), width=70)
        write_fastq(p("long.fq"), long_reads(100, 200, 1500, 42))
        libs.append("[LIB]\nasm_flags=4\nrd_len_cutoff=1000\nmap_len=40\nf=%s\nq=%s\n" % (p("long.fa"), p("long.fq")))
    elif layout == "two":
        a = long_reads(120, 300, 1500, 43)
        b = long_reads(120, 300, 1500, 44)
        write_fasta(p("x_1.fa"), a)
        write_fasta(p("x_2.fa"), b, width=60)
        write_fasta(p("x_p.fa"), long_reads(61, 30, 1200, 45), width=100)
        write_fasta(p("y.fa"), long_reads(90, 400, 1500, 46))
        with open(p("y.fa"), "rb") as f, gzip.open(p("y.fa.gz"), "wb") as z:
            z.write(f.read())
        x = "[LIB]\navg_ins=200\nasm_flags=4\nreverse_seq=1\nrd_len_cutoff=800\nmap_len=50\nf1=%s\nf2=%s\np=%s\n" % (p("x_1.fa"), p("x_2.fa"), p("x_p.fa"))
        y = "[LIB]\navg_ins=1000\nasm_flags=4\nrd_len_cutoff=1100\nmap_len=36\nf=%s\n" % p("y.fa.gz")
        libs = [x, libs[0], y, libs[1]]                     # before and between the short ones
    elif layout == "batches":
        # longReadLen 500 031: batches of 1e8 / 500 001 = 199 -> 198 reads; 451 reads are three batches
        write_fastq(p("long.fq"), long_reads(451, 200, 1400, 47))
        libs.append("[LIB]\nasm_flags=4\nrd_len_cutoff=500031\nq=%s\n" % p("long.fq"))
    elif layout == "nocut":
        # no rd_len_cutoff: longReadLen = max_rd_len, raised here so that the long reads keep their k-mers
        write_fasta(p("long.fa"), long_reads(260, 300, 2400, 48), width=80)
        head = "max_rd_len=2000\n"
        libs = [libs[0], "[LIB]\nasm_flags=4\nmap_len=90\nf=%s\n" % p("long.fa"), libs[1]]
    elif layout == "bam":
        # a b= file in the long pass: 13 records pair up two by two, the pair of records 4 and 5 has a QC-fail mate and is taken back
        # (prlRead2Ctg.c:1184-1196), and the odd count leaves the file ending on a first mate.  The f= file comes after it
        recs = [(b"b%d" % i, 0x200 if i == 5 else 0, _text(s)) for i, s in enumerate(long_reads(13, 200, 1500, 49))]
        synth.write_bam(p("long.bam"), recs)
        write_fasta(p("long.fa"), long_reads(301, 200, 1500, 41), width=70)
        # (a library with a b= file must give avg_ins: the reference's config check)
        libs.append("[LIB]\navg_ins=400\nasm_flags=4\nrd_len_cutoff=1000\nmap_len=40\nb=%s\nf=%s\n" % (p("long.bam"), p("long.fa")))
    else:
        raise ValueError(layout)
    with open(cfg, "w") as f:
        f.write(head + "".join(libs))
    return cfg


def write_case(d, name):
    """The config of a command case under d; returns (cfg, case tuple)."""
    mer127, K, k, p, fill, short, layout = CASES[name]
    cfg = M.write_libs(d, short, k or K)
    return write_long_libs(d, cfg, layout), CASES[name]


def long_digests(pre):
    out = M.digests(pre)
    for ext in LONG_OUTPUTS:
        f = pre + "." + ext
        out[ext] = hashlib.md5(open(f, "rb").read()).hexdigest() if os.path.exists(f) else None
    return out


def long_lines(stderr):
    """The long pass's stderr lines, without the config's path."""
    out = []
    for ln in stderr.splitlines():
        if ln.startswith("In file: ") and ", long read len " in ln:
            out.append("long read len " + ln.split(", long read len ", 1)[1])
        elif ln.startswith(("Map_len ", "Output ")) or ln.endswith(" reads deleted."):
            out.append(ln.strip())
    return out


def long_counts(stderr):
    """(reads output, reads seen) of the pass's "Output a out of b" line."""
    for ln in stderr.splitlines():
        if ln.startswith("Output "):
            w = ln.split()
            return int(w[1]), int(w[4])
    return None
