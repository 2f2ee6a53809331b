#!/usr/bin/env python3
"""The long-read pass's two kernels against each other: SOAPDENOVO2_AMD_MAP_LONG_KERNEL=wave (a wavefront a read) and lane (the short
pass's lane-per-read kernel), on one batch that one `map` run reads.

    python scripts/map_long_ab.py --out /tmp/mapl --save profiles/map_long_wave_vs_lane.json

Contigs of BASELINE configs[1]'s size: synthetic short reads (scripts/synth_fastq.cpp) through this build's pregraph and the reference's
`contig` (oracle/_ref).  The long reads come from the same generator with the same seed, which is the genome: --long-reads reads of --long-len bases as one
asm_flags=4 q= library with rd_len_cutoff = --long-len, so 1e8 / (long_len - K + 1) reads are one batch.  The map config holds that
library alone.  The two kernels alternate --rounds times; the time is the engine's event time of the pass's kernel launches
(PG_HOST_VERBOSE=1's "[map long]" line), the files of every run must have one md5."""
import argparse, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "soapdenovo2_amd", "bin", "synth_fastq")


def run(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode:
        sys.stderr.write(r.stderr[-3000:])
        sys.exit(f"{' '.join(cmd[:2])} failed ({r.returncode})")
    return time.time() - t, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="/tmp/map_long_ab")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--err", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--kmer", type=int, default=31)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--long-len", type=int, default=2000)
    ap.add_argument("--long-err", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--save", default="")
    a = ap.parse_args()
    out = os.path.abspath(a.out)
    os.makedirs(out, exist_ok=True)
    name = "SOAPdenovo-127mer" if a.kmer > 63 else "SOAPdenovo-63mer"
    ours, ref = os.path.join(ROOT, "soapdenovo2_amd", "bin", name), os.path.join(ROOT, "oracle", "_ref", name)
    fq, lfq, pre = os.path.join(out, "r.fq"), os.path.join(out, "long.fq"), os.path.join(out, "g")
    subprocess.check_call([GEN, fq, str(a.genome), str(a.reads), str(a.read_len), str(a.err), str(a.seed), "16"])
    subprocess.check_call([GEN, lfq, str(a.genome), str(a.long_reads), str(a.long_len), str(a.long_err), str(a.seed), "16"])      # the seed is the genome
    open(os.path.join(out, "pg.cfg"), "w").write(f"max_rd_len={a.read_len}\n[LIB]\navg_ins=200\nasm_flags=3\nrank=1\nq={fq}\n")
    cfg = os.path.join(out, "map.cfg")
    open(cfg, "w").write(f"max_rd_len={a.read_len}\n[LIB]\nasm_flags=4\nrd_len_cutoff={a.long_len}\nq={lfq}\n")
    res = {"workload": {k: getattr(a, k) for k in ("reads", "read_len", "genome", "err", "seed", "kmer", "long_reads", "long_len", "long_err")}}
    res["pregraph_s"] = round(run([ours, "pregraph", "-s", os.path.join(out, "pg.cfg"), "-K", str(a.kmer), "-o", pre, "-p", "8"])[0], 2)
    res["contig_s"] = round(run([ref, "contig", "-g", pre])[0], 2)
    os.remove(fq)
    times = {"wave": [], "lane": []}
    whole = {"wave": [], "lane": []}
    md5 = set()
    line = re.compile(r"\[map long\] (\w+) kernel: (\d+) reads.*\(kernel ([0-9.]+)s.*reads done in passes (\d+), distinct ids (\d+)")
    for rnd in range(a.rounds):
        for kernel in ("wave", "lane"):
            env = dict(os.environ, PG_HOST_VERBOSE="1", SOAPDENOVO2_AMD_MAP_LONG="1", SOAPDENOVO2_AMD_MAP_LONG_KERNEL=kernel)
            wall, err = run([ours, "map", "-s", cfg, "-g", pre, "-p", "8", "-f"], env)
            m = line.search(err)
            if not m or m.group(1) != kernel:
                sys.exit("no [map long] line:\n" + err[-2000:])
            times[kernel].append(float(m.group(3)))
            whole[kernel].append(round(wall, 2))
            md5.add(hashlib.md5(open(pre + ".longReadInGap", "rb").read()).hexdigest())
            if kernel == "wave":
                res["reads"] = int(m.group(2))
                res["share_of_reads_done_in_passes"] = int(m.group(4)) / max(1, int(m.group(2)))
                res["mean_distinct_ids"] = int(m.group(5)) / max(1, int(m.group(2)))
            res["output_line"] = [l for l in err.splitlines() if l.startswith("Output ")]
    res["kernel_s"] = times
    res["whole_command_s"] = whole
    res["one_md5"] = len(md5) == 1
    lane_spread = max(times["lane"]) - min(times["lane"])
    res["lane_median_s"], res["wave_median_s"] = statistics.median(times["lane"]), statistics.median(times["wave"])
    res["lane_spread_s"] = lane_spread
    res["wave_faster_by_more_than_3_spreads"] = res["lane_median_s"] - res["wave_median_s"] > 3 * lane_spread
    print(json.dumps(res, indent=1))
    if a.save:
        json.dump(dict(res, made_by="scripts/map_long_ab.py"), open(a.save, "w"), indent=1)
    sys.exit(0 if res["one_md5"] else 1)


if __name__ == "__main__":
    main()
