#!/usr/bin/env python3
"""The k-mer index's query rate on an MI355X: count the reads of BASELINE.json configs[1] (10 M x 100 bp over 4.6 Mb, err 0.005, K = 31),
index the distinct k-mers (KmerCounter.index()) and ask with the same reads, resident in HBM -- the lane-per-sequence and the
wavefront-per-sequence kernel alternating, five runs each after one warm-up run each, every run timed by a pair of events around the
one launch.  Writes profiles/kindex_query.json: lookups/s of every run next to the 38 G random lookups/s DESIGN.md §8 measured for
pass 2, whose slot reads these are.  Needs a GPU; nothing falls back.

    python scripts/kindex_bench.py [--reads 10000000] [--out profiles/kindex_query.json]

--ranks N [N ...]: the same reads through the index cut over N ranks (KmerCounter.index(devices=(0,) * N): every rank on this one GPU), in
the same process and with the same runs, after the single table's.  Writes profiles/kindex_query_sharded.json next to the single-table
file: per N the seconds of every run, their ratio to the single table's of this run -- the yardstick; every rank rolls every k-mer and
probes 1/N of them, and the lead adds N - 1 row copies and ORs of 8 B a k-mer, so on one GPU the cut costs time and is for tables that
do not fit, not for speed -- and the split of the last run into the slowest rank's probe, the merge and the summary from the index's
own events.
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kindex_query.json"))
    ap.add_argument("--ranks", type=int, nargs="+", default=[])
    ap.add_argument("--out-sharded", default=os.path.join(ROOT, "profiles", "kindex_query_sharded.json"))
    a = ap.parse_args()
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "kindex_bench.py measures on a GPU"
    K, L, n = a.kmer, a.read_len, a.reads
    wpr = api.packed_words(L)
    packed = torch.zeros(n * wpr + 8, dtype=torch.int64, device="cuda")
    codes = synth.gpu_reads_codes(a.genome, n, L, a.err, 1)
    for lo in range(0, n, 1_000_000):                                  # (the packer pads to whole words in 64-bit lanes: a chunk at a time)
        hi = min(n, lo + 1_000_000)
        packed[lo * wpr:hi * wpr] = torch.from_numpy(api.pack_reads_uniform(codes[lo:hi])[:(hi - lo) * wpr].view(np.int64)).cuda()
    del codes
    expected = a.genome + int(n * L * a.err * K)
    kc = api.KmerCounter(K, n_sets=8, log2_slots=max(16, int(np.ceil(np.log2(expected / 0.7)))))
    n_kmers = kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    digest = kc.checksum()
    ix = kc.index()
    cut = {n_ranks: kc.index(devices=(0,) * n_ranks) for n_ranks in a.ranks}
    kc.close()
    info = ix.info()
    runs = {"lane": [], "wave": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    present = {}
    for i in range(a.runs + 1):                                        # (run 0 warms both kernels up)
        for name, wave in (("lane", False), ("wave", True)):
            e0.record()
            summ = ix.query_uniform(packed, n, L, wave=wave, counts=False, summary=True)
            e1.record()
            torch.cuda.synchronize()
            present[name] = int(summ[:, 0].sum())
            if i:
                runs[name].append(e0.elapsed_time(e1) * 1e-3)
    assert present["lane"] == present["wave"] == n_kmers, "a k-mer of the counted reads is absent"
    ix.close()
    out = {"workload": f"{n} resident reads x {L} bp, genome {a.genome}, err {a.err}, K={K}: every k-mer looked up in the index of the same reads, summary only",
           "device": torch.cuda.get_device_name(0), "lookups": n_kmers, "index": info, "saturated_kmers": int(digest[7]),
           "slot_bytes": 32, "pass2_random_lookups_per_s_DESIGN_8": 38e9}
    for name, t in runs.items():
        out[name] = {"seconds": t, "lookups_per_s": [n_kmers / x for x in t], "median_lookups_per_s": n_kmers / float(np.median(t))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({k: out[k]["median_lookups_per_s"] for k in runs}))
    if not cut:
        return
    sharded = {"workload": out["workload"] + "; the index cut over N ranks, every rank on this GPU", "device": out["device"], "lookups": n_kmers,
               "single_table_median_seconds": {k: float(np.median(runs[k])) for k in runs}, "ranks": {}}
    for n_ranks, cx in cut.items():
        c_runs, split = {"lane": [], "wave": []}, {}
        for i in range(a.runs + 1):
            for name, wave in (("lane", False), ("wave", True)):
                e0.record()
                summ = cx.query_uniform(packed, n, L, wave=wave, counts=False, summary=True)
                e1.record()
                torch.cuda.synchronize()
                assert int(summ[:, 0].sum()) == n_kmers, "a k-mer of the counted reads is absent"
                if i:
                    c_runs[name].append(e0.elapsed_time(e1) * 1e-3)
                    split[name] = cx.query_times()
        c_info = cx.info()
        sharded["ranks"][str(n_ranks)] = {
            "index": {k: c_info[k] for k in ("keys", "slots", "bytes")}, "keys_of_a_rank": [r["keys"] for r in c_info["ranks"]],
            **{name: {"seconds": t, "median_seconds": float(np.median(t)), "ratio_to_single_table": float(np.median(t) / np.median(runs[name])),
                      "last_run_ms": split[name]} for name, t in c_runs.items()}}
        cx.close()
    json.dump(sharded, open(a.out_sharded, "w"), indent=1)
    print(json.dumps({n_ranks: {k: v[k]["ratio_to_single_table"] for k in runs} for n_ranks, v in sharded["ranks"].items()}))


if __name__ == "__main__":
    main()
