#!/usr/bin/env python3
"""What the walk does on an MI355X next to the plain index query of the same run: the reads of BASELINE.json configs[1] (10 M x 100 bp over
4.6 Mb, K = 31) with a fixed share of substitutions (--err, 0.005), resident in HBM, are counted and indexed (KmerCounter.index()) as
scripts/kindex_bench.py does; the seeds are K-mers cut from the first --seeds reads (read i's k-mer 7 i mod (L - K + 1)), two walks a
seed (KmerIndex.walk_uniform), at each --setting min_cov:min_arc.  The default settings are the corrector's 3:2 and 8:8: at 217-fold
coverage some 150 reads span an arc, and with 0.005 substitutions a given wrong base follows a given k-mer 0.25 times on average, so about
one k-mer in twelve has a wrong arc counted twice or more on either side and walks at min_arc 2 end after a few bases, while a wrong
arc counted 8 times is a matter of 1e-9.  The walk calls and the lane-per-sequence query of all reads (summary only) alternate, five
runs each after one warm-up run each, every run timed by a pair of events around the one call (the walk's rows and report are
allocated and zeroed inside the pair, as the query's summary is).  Writes profiles/kwalk.json: seconds of every run, steps per second (appended bases; a
step is one dependent slot read) and slot lookups per second (the seed's and a refused successor's included) beside the query's
lookups per second -- the yardstick; nobody has measured a walk rate, so none is asserted anywhere -- and the share of lane-steps a wave
spends idle, worked out on the host from the report lengths: walk v runs in lane v mod 64 of wave v / 64, a wave runs as long as its
longest walk, so busy = sum(len) / sum over waves of 64 * max len in the wave, and idle = 1 - busy.  Needs a GPU; nothing falls back.

    python scripts/kwalk_bench.py [--reads 10000000] [--seeds 2000000] [--setting 3:2 8:8] [--max-ext 256] [--out profiles/kwalk.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--kmer", type=int, default=31)
    ap.add_argument("--seeds", type=int, default=2_000_000)
    ap.add_argument("--setting", nargs="+", default=["3:2", "8:8"], help="min_cov:min_arc")
    ap.add_argument("--max-ext", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kwalk.json"))
    a = ap.parse_args()
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "kwalk_bench.py measures on a GPU"
    K, L, n, m = a.kmer, a.read_len, a.reads, min(a.seeds, a.reads)
    wpr = api.packed_words(L)
    packed = torch.zeros(n * wpr + 8, dtype=torch.int64, device="cuda")
    codes = synth.gpu_reads_codes(a.genome, n, L, a.err, 1)
    for lo in range(0, n, 1_000_000):                                  # (the packer pads to whole words in 64-bit lanes: a chunk at a time)
        hi = min(n, lo + 1_000_000)
        packed[lo * wpr:hi * wpr] = torch.from_numpy(api.pack_reads_uniform(codes[lo:hi])[:(hi - lo) * wpr].view(np.int64)).cuda()
    at = (7 * np.arange(m, dtype=np.int64)) % (L - K + 1)
    seeds = torch.from_numpy(api.pack_reads_uniform(codes[np.arange(m)[:, None], at[:, None] + np.arange(K)[None, :]]).view(np.int64)).cuda()
    del codes
    expected = a.genome + int(n * L * a.err * K)
    kc = api.KmerCounter(K, n_sets=8, log2_slots=max(16, int(np.ceil(np.log2(expected / 0.7)))))
    n_kmers = kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    ix = kc.index()
    kc.close()
    settings = {s: tuple(int(x) for x in s.split(":")) for s in a.setting}
    runs = {name: [] for name in list(settings) + ["query"]}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reports = {}
    for i in range(a.runs + 1):                                        # (run 0 warms every path up)
        for name in runs:
            e0.record()
            if name == "query":
                ix.query_uniform(packed, n, L, counts=False, summary=True)
            else:
                _, reports[name] = ix.walk_uniform(seeds, m, K, settings[name][0], settings[name][1], a.max_ext)
            e1.record()
            torch.cuda.synchronize()
            if i:
                runs[name].append(e0.elapsed_time(e1) * 1e-3)
    info = ix.info()
    ix.close()
    med = {k: float(np.median(t)) for k, t in runs.items()}
    query_rate = n_kmers / med["query"]
    res = {"workload": f"{n} resident reads x {L} bp, genome {a.genome}, err {a.err}, K={K}, counted and indexed; {m} seed k-mers cut from the reads, "
                       f"{2 * m} walks of at most {a.max_ext} bases at each min_cov:min_arc; the query is the lane kernel over all reads, summary only",
           "device": torch.cuda.get_device_name(0), "index": info, "walks": 2 * m, "max_ext": a.max_ext, "seconds": runs, "median_seconds": med,
           "query_lookups": n_kmers, "query_lookups_per_s": query_rate, "settings": {}}
    for name in settings:
        f = api.walk_fields(reports[name])
        lens, code = f["len"], f["code"]
        steps = int(lens.sum())
        # a walk's slot reads: its seed's (a sequence without a k-mer has none), one a base, and the successor that ended it where one was read
        lookups = int((code != 1).sum()) + steps + int(np.isin(code, (5, 6, 7)).sum())
        padded = np.zeros((len(lens) + 63) // 64 * 64, dtype=np.int64)
        padded[:len(lens)] = lens
        wave_steps = int(64 * padded.reshape(-1, 64).max(axis=1).sum())
        busy = steps / wave_steps if wave_steps else 0.0
        res["settings"][name] = {"min_cov": settings[name][0], "min_arc": settings[name][1], "steps": steps, "slot_lookups": lookups,
                                 "steps_per_s": steps / med[name], "lookups_per_s": lookups / med[name],
                                 "lookup_rate_over_query": lookups / med[name] / query_rate, "mean_len": float(lens.mean()),
                                 "reasons": {r: int((code == c).sum()) for c, r in api.WALK_REASONS.items()}, "wave_lane_steps": wave_steps,
                                 "busy_share": busy, "idle_share": 1.0 - busy}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"median_seconds": med, "query_lookups_per_s": query_rate,
                      **{name: {k: v[k] for k in ("steps_per_s", "lookups_per_s", "lookup_rate_over_query", "mean_len", "idle_share", "reasons")}
                         for name, v in res["settings"].items()}}))


if __name__ == "__main__":
    main()
