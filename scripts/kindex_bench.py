#!/usr/bin/env python3
"""The k-mer index's query rate on an MI355X: count the reads of BASELINE.json configs[1] (10 M x 100 bp over 4.6 Mb, err 0.005, K = 31),
index the distinct k-mers (KmerCounter.index()) and ask with the same reads, resident in HBM -- the lane-per-sequence and the
wavefront-per-sequence kernel alternating, five runs each after one warm-up run each, every run timed by a pair of events around the
one launch.  Writes profiles/kindex_query.json: lookups/s of every run next to the 38 G random lookups/s DESIGN.md §8 measured for
pass 2, whose slot reads these are.  Needs a GPU; nothing falls back.

    python scripts/kindex_bench.py [--reads 10000000] [--out profiles/kindex_query.json]
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


if __name__ == "__main__":
    main()
