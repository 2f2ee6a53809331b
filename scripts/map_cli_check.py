#!/usr/bin/env python3
"""The `map` stage at full size: synthetic reads (scripts/synth_fastq.cpp, bytes that depend on the arguments only) as one q1/q2 library,
contigs from pregraph + the reference's `contig`, then `SOAPdenovo-63mer|127mer map`, md5s of its outputs compared with the reference's.

    # where the reference runs (no GPU needed): its pregraph, contig and map, timed, md5s saved
    python scripts/map_cli_check.py --reference --out /tmp/map10 --save profiles/map_ref_10M_K31.json
    # on the GPU box: this build's pregraph (byte-identical to the reference's) + the reference's contig, then this build's map, timed
    python scripts/map_cli_check.py --expect profiles/map_ref_10M_K31.json --out /tmp/map10

    # the index cut over three ranks of the one GPU against one table: map alternately both ways, three times each, on the same prefix
    python scripts/map_cli_check.py --expect profiles/map_ref_10M_K31.json --out /tmp/map10 --sharded-ranks 3 --repeat 3 \
        --save-ab profiles/map_sharded_one_gpu.json

Defaults are BASELINE configs[1]: 10 M x 100 bp, K = 31, an E. coli-sized genome.  q1 = the first half of the reads (seed), q2 = the second
half (seed + 1): map reads only paired libraries (nextValidIndex with pairs = 1), and two files of independent reads are such a library.
Exit code 1 when the md5s differ or a command fails."""
import argparse, gzip, hashlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "soapdenovo2_amd", "bin", "synth_fastq")
OUTS = ("readOnContig.gz", "readInGap.gz", "peGrads", "shortreadInGap.gz", "PEreadOnContig.gz")


def md5s(prefix):
    out = {}
    for ext in OUTS:
        f = f"{prefix}.{ext}"
        if not os.path.exists(f):
            continue
        h = hashlib.md5()
        with (gzip.open(f, "rb") if ext.endswith(".gz") else open(f, "rb")) as fp:
            for chunk in iter(lambda: fp.read(1 << 24), b""):
                h.update(chunk)
        out[ext] = h.hexdigest()
    return out


def timed(cmd, env=None, log=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if log:
        open(log, "w").write(r.stderr)
    if r.returncode:
        sys.stderr.write(r.stderr[-3000:])
        sys.exit(f"{' '.join(cmd[:2])} failed ({r.returncode})")
    return round(time.time() - t, 2), r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="/tmp/map_check")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--err", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--kmer", type=int, default=31)
    ap.add_argument("--p", type=int, default=8, help="map's -p (and pregraph's)")
    ap.add_argument("--fill", action="store_true", help="map -f")
    ap.add_argument("--reference", action="store_true", help="run the reference's pregraph, contig and map (oracle/_ref) and --save")
    ap.add_argument("--save", default="")
    ap.add_argument("--expect", default="", help="JSON written by --reference --save for the same arguments")
    ap.add_argument("--threads", type=int, default=16, help="threads of the FASTQ generator")
    ap.add_argument("--sharded-ranks", type=int, default=0, help="after the first map: map again, alternately on one table and with the index cut over this many ranks of GPU 0")
    ap.add_argument("--repeat", type=int, default=3, help="runs of each form with --sharded-ranks")
    ap.add_argument("--save-ab", default="", help="where the alternating runs' times go")
    a = ap.parse_args()
    key = {k: getattr(a, k) for k in ("reads", "read_len", "genome", "err", "seed", "kmer", "p", "fill")}
    want = None
    if not a.reference:
        if not a.expect:
            sys.exit("no --expect: a run compared with nothing proves nothing")
        e = json.load(open(a.expect))
        if e.get("workload") != key:
            sys.exit(f"{a.expect} is for {e.get('workload')}, not {key}")
        want = e["md5"]
    os.makedirs(a.out, exist_ok=True)
    out = os.path.abspath(a.out)
    fq1, fq2, cfg = os.path.join(out, "r_1.fq"), os.path.join(out, "r_2.fq"), os.path.join(out, "lib.cfg")
    t = time.time()
    for fq, seed in ((fq1, a.seed), (fq2, a.seed + 1)):
        subprocess.check_call([GEN, fq, str(a.genome), str(a.reads // 2), str(a.read_len), str(a.err), str(seed), str(a.threads)])
    open(cfg, "w").write(f"max_rd_len={a.read_len}\n[LIB]\navg_ins=200\nreverse_seq=0\nasm_flags=3\nrank=1\nq1={fq1}\nq2={fq2}\n")
    res = {"workload": key, "generate_s": round(time.time() - t, 1)}
    mer127 = a.kmer > 63
    name = "SOAPdenovo-127mer" if mer127 else "SOAPdenovo-63mer"
    ref = os.path.join(ROOT, "oracle", "_ref", name)
    ours = os.path.join(ROOT, "soapdenovo2_amd", "bin", name)
    pre = os.path.join(out, "g")
    res["pregraph_s"], _ = timed([ref if a.reference else ours, "pregraph", "-s", cfg, "-K", str(a.kmer), "-o", pre, "-p", str(a.p)])
    res["contig_s"], _ = timed([ref, "contig", "-g", pre])
    cmd = [ref if a.reference else ours, "map", "-s", cfg, "-g", pre, "-p", str(a.p)] + (["-f"] if a.fill else [])
    env = dict(os.environ, PG_HOST_VERBOSE="1")
    res["map_s"], err = timed(cmd, env, os.path.join(out, "map_stderr.txt"))
    res["map_binary"] = os.path.relpath(cmd[0], ROOT)
    res["map_log"] = [l for l in err.splitlines() if l.startswith(("[map]", "Total reads", "Reads in gaps", "Reads on contigs", "Ratio", "Time spent"))]
    res["md5"] = md5s(pre)
    ok = True
    if want is not None:
        res["identical_to_reference"] = res["md5"] == want
        ok = res["identical_to_reference"]
    if a.sharded_ranks and not a.reference:
        forms = {"one_table": {}, "sharded": {"SOAPDENOVO2_AMD_DEVICES": ",".join(["0"] * a.sharded_ranks), "SOAPDENOVO2_AMD_MAP_SHARD": "1"}}
        ab = {"workload": key, "ranks_on_gpu_0": a.sharded_ranks, "runs": []}
        for i in range(a.repeat):
            for form, extra in forms.items():
                for ext in OUTS:
                    if os.path.exists(f"{pre}.{ext}"):
                        os.remove(f"{pre}.{ext}")
                secs, err = timed(cmd, dict(env, **extra), os.path.join(out, f"map_stderr_{form}_{i}.txt"))
                same = md5s(pre) == want
                ok = ok and same
                ab["runs"].append({"form": form, "run": i, "map_s": secs, "identical_to_reference": same,
                                   "map_log": [l for l in err.splitlines() if l.startswith(("[map]", "Time spent"))]})
        res["sharded_ab"] = ab
        if a.save_ab:
            json.dump(dict(ab, made_by="scripts/map_cli_check.py --sharded-ranks"), open(a.save_ab, "w"), indent=1)
    for f in os.listdir(out):
        if f.startswith("r_") or f.startswith("g."):
            os.remove(os.path.join(out, f))
    print(json.dumps(res, indent=1))
    json.dump(res, open(os.path.join(out, "result.json"), "w"), indent=1)
    if a.reference and a.save:
        json.dump(dict(res, made_by="scripts/map_cli_check.py --reference (oracle/_ref)", host_cpus=os.cpu_count()), open(a.save, "w"), indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
