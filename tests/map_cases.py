"""Inputs of the `map` stage's tests: a genome, reads for the reference's pregraph + contig (which give the contigs), and read libraries for
`map` that go through the corners of read1seqInLib / parse1read / recordAlldgn (standardPregraph/readseq1by1.c, prlRead2Ctg.c).

Everything is made from seeds (soapdenovo2_amd.synth); tests/golden/make_map_golden.py records the reference's md5s of these cases and
tests/test_map_host.py / tests/test_gpu_map.py hold both flavours of the stage against the reference."""
import gzip
import hashlib
import os
import shutil
import subprocess

import numpy as np

from soapdenovo2_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ["readOnContig.gz", "readInGap.gz", "peGrads", "shortreadInGap.gz", "PEreadOnContig.gz"]
SUMMARY = ("Total reads", "Reads in gaps", "Ratio", "Reads on contigs")

# name: (flavour 127?, pregraph K, map -k or 0, -p, -f, library layout)
CASES = {
    "k31_p1":        (False, 31, 0, 1, False, "pairs"),
    "k31_p3_f":      (False, 31, 0, 3, True, "pairs"),
    "k31_p8_f":      (False, 31, 0, 8, True, "all"),
    "k63_p3_f":      (False, 63, 0, 3, True, "all"),
    "k41_k25_p8":    (False, 41, 25, 8, True, "pairs"),
    "k31_batches":   (False, 31, 0, 3, True, "batches"),
    "m127_k75_p3_f": (True, 75, 0, 3, True, "all"),
    "m127_k127_p8":  (True, 127, 0, 8, True, "pairs"),
    "m127_k75_k33":  (True, 75, 33, 1, True, "pairs"),
}
GENOME_SEED = 2024


def genome(n=24000, seed=GENOME_SEED):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=n, dtype=np.uint8)
    # a few repeated stretches: contigs that share k-mers (deleted keys) and a palindrome
    for src, dst, ln in ((1000, 9000, 300), (5000, 15000, 180), (12000, 20000, 90)):
        g[dst:dst + ln] = g[src:src + ln]
    g[7000:7100] = g[7100:7200][::-1] ^ 2
    return g


def binary(mer127, ours):
    if ours:
        return os.path.join(ROOT, "soapdenovo2_amd", "bin", "SOAPdenovo-127mer" if mer127 else "SOAPdenovo-63mer")
    return os.path.join(ROOT, "oracle", "_ref", "SOAPdenovo-127mer" if mer127 else "SOAPdenovo-63mer")


def _trim(reads, every, to):
    out = [np.asarray(r) for r in reads]
    for i in range(0, len(out), every):
        out[i] = out[i][:to]
    return out


def write_libs(d, layout, K):
    """The map config of a case; returns its path."""
    g = genome()
    p = lambda f: os.path.join(d, f)
    rl = 150 if K > 100 else 100                         # (reads longer than K where the 127-mer flavour runs K = 127)
    a1, a2 = synth.paired_codes(len(g), 1500, rl, 300, 0.01, 31, genome=g)
    a1 = _trim(a1, 37, 24)                               # reads shorter than K + 1 (no k-mers: contig 0)
    a2 = _trim(a2, 53, 60)
    synth.write_fastq_pair(p("a_1.fq"), p("a_2.fq"), a1, a2, lower_every=7, n_every=5, dot_every=11)
    b1, b2 = synth.paired_codes(len(g), 600, rl - 10, 2500, 0.01, 32, genome=g)
    synth.write_fastq_pair(p("b_1.fa"), p("b_2.fa"), b1, b2, fasta=True, n_every=9)
    libs = []
    max_rd_len = rl
    if layout in ("pairs", "all", "batches"):
        libs.append("[LIB]\navg_ins=300\nreverse_seq=0\nasm_flags=3\nrank=1\nrd_len_cutoff=%d\nq1=%s\nq2=%s\n" % (rl - 5, p("a_1.fq"), p("a_2.fq")))
        libs.append("[LIB]\navg_ins=2500\nreverse_seq=1\nasm_flags=3\nrank=2\nmap_len=40\nf1=%s\nf2=%s\n" % (p("b_1.fa"), p("b_2.fa")))
    if layout in ("all", "batches"):
        c1, c2 = synth.paired_codes(len(g), 400, 80, 500, 0.02, 33, genome=g)
        inter = [x for pair in zip(c1, c2) for x in pair]
        synth.write_fastq_pair(p("c.fa"), p("c_unused.fa"), inter, inter[:1], fasta=True)
        with open(p("c.fa"), "rb") as f, gzip.open(p("c2.fa.gz"), "wb") as z:
            z.write(f.read())
        e1, e2 = synth.paired_codes(len(g), 300, 70, 400, 0.01, 34, genome=g)
        recs = []
        for i, (x, y) in enumerate(zip(e1, e2)):
            qc1 = 0x200 if i % 17 == 3 else 0
            qc2 = 0x200 if i % 23 == 5 else 0
            recs.append((b"e%d/1" % i, 77 | qc1, "".join("ACTG"[v] for v in x)))
            recs.append((b"e%d/2" % i, 141 | qc2, "".join("ACTG"[v] for v in y)))
        synth.write_bam(p("e.bam"), recs)
        libs.append("[LIB]\navg_ins=500\nreverse_seq=0\nasm_flags=2\nrank=3\np=%s\np=%s\nb=%s\nq=%s\n"
                    % (p("c.fa"), p("c2.fa.gz"), p("e.bam"), p("a_1.fq")))
        libs.append("[LIB]\navg_ins=800\nasm_flags=1\nq1=%s\nq2=%s\n" % (p("a_1.fq"), p("a_2.fq")))      # not read by map
    if layout == "batches":
        max_rd_len = 50000 + K                           # maxReadNum = 1e8 / (max_rd_len - K + 1) = 2000 reads: several batches
    cfg = p("map.cfg")
    with open(cfg, "w") as f:
        f.write("max_rd_len=%d\n" % max_rd_len + "".join(libs))
    return cfg


def make_graph(d, mer127, K):
    """The reference's pregraph + contig on reads of the genome: <d>/g.contig, .ContigIndex, .preGraphBasic."""
    os.makedirs(d, exist_ok=True)
    g = genome()
    rng = np.random.default_rng(7)
    L = 150 if K > 100 else 100
    starts = rng.integers(0, len(g) - L, size=12000)
    reads = g[starts[:, None] + np.arange(L)[None, :]]
    flip = rng.random(len(starts)) < 0.5
    reads = np.where(flip[:, None], reads[:, ::-1] ^ 2, reads).astype(np.uint8)
    synth.write_fastq(os.path.join(d, "pg.fq"), reads)
    synth.write_config(os.path.join(d, "pg.cfg"), os.path.join(d, "pg.fq"), L)
    pre = os.path.join(d, "g")
    ref = binary(mer127, False)
    subprocess.run([ref, "pregraph", "-s", os.path.join(d, "pg.cfg"), "-K", str(K), "-o", pre, "-p", "4"], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([ref, "contig", "-g", pre], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return pre


def run_map(binary_path, cfg, graph_prefix, outdir, k, p, fill, env=None):
    """Copy the graph files to <outdir>, run `map` there; returns (returncode, stderr text, prefix)."""
    os.makedirs(outdir, exist_ok=True)
    pre = os.path.join(outdir, "g")
    for ext in ("contig", "ContigIndex", "preGraphBasic"):
        shutil.copy(graph_prefix + "." + ext, pre + "." + ext)
    args = [binary_path, "map", "-s", cfg, "-g", pre, "-p", str(p)]
    if k:
        args += ["-k", str(k)]
    if fill:
        args.append("-f")
    r = subprocess.run(args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=env)
    return r.returncode, r.stderr, pre


def digests(pre):
    """md5 of every output (of the decompressed bytes for .gz), None where the file is absent."""
    out = {}
    for ext in OUTPUTS:
        f = pre + "." + ext
        if not os.path.exists(f):
            out[ext] = None
        elif ext.endswith(".gz"):
            with gzip.open(f, "rb") as z:
                out[ext] = hashlib.md5(z.read()).hexdigest()
        else:
            out[ext] = hashlib.md5(open(f, "rb").read()).hexdigest()
    return out


def summary(stderr):
    return [ln.strip() for ln in stderr.splitlines() if ln.startswith(SUMMARY)]


def build_case(workdir, name):
    """Graph + map config of a case under <workdir>/<name>; returns (cfg, graph prefix, case tuple)."""
    mer127, K, k, p, fill, layout = CASES[name]
    d = os.path.join(workdir, name)
    pre = make_graph(os.path.join(d, "graph"), mer127, K)
    cfg = write_libs(d, layout, k or K)
    return cfg, pre, CASES[name]
