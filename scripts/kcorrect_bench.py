#!/usr/bin/env python3
"""What the read corrector costs on an MI355X next to the plain index query over the same reads: the reads of BASELINE.json configs[1]
(10 M x 100 bp over 4.6 Mb, K = 31) with a fixed share of substitutions (--err, 0.005), resident in HBM, are counted, indexed
(KmerCounter.index()) and corrected into a second buffer (KmerIndex.correct_uniform) -- the correct call and the lane-per-sequence query
(summary only) alternating, five runs each after one warm-up run each, every run timed by a pair of events around the one call (the
correct call's copy of the batch included).  Writes profiles/kcorrect.json: seconds of every run, the ratio of the medians, and what the
reports add up to.  The query is the yardstick; no rate is asserted anywhere.  Needs a GPU; nothing falls back.

    python scripts/kcorrect_bench.py [--reads 10000000] [--min-cov 3] [--out profiles/kcorrect.json]
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
    ap.add_argument("--min-cov", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcorrect.json"))
    a = ap.parse_args()
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "kcorrect_bench.py measures on a GPU"
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
    distinct_before = kc.distinct()
    ix = kc.index()
    kc.close()
    out = torch.empty_like(packed)
    runs = {"correct": [], "query": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    report = None
    for i in range(a.runs + 1):                                        # (run 0 warms both kernels up)
        for name in ("correct", "query"):
            e0.record()
            if name == "correct":
                _, report = ix.correct_uniform(packed, n, L, a.min_cov, out=out)
            else:
                ix.query_uniform(packed, n, L, counts=False, summary=True)
            e1.record()
            torch.cuda.synchronize()
            if i:
                runs[name].append(e0.elapsed_time(e1) * 1e-3)
    f = api.report_fields(report)
    info = ix.info()
    ix.close()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=max(16, int(np.ceil(np.log2(expected / 0.7)))))
    kc.count_uniform(out, n, L, 0)
    kc.finalize(0)
    distinct_after = kc.distinct()
    kc.close()
    med = {k: float(np.median(t)) for k, t in runs.items()}
    res = {"workload": f"{n} resident reads x {L} bp, genome {a.genome}, err {a.err}, K={K}, min_cov {a.min_cov}, max_fixes {api.CORRECT_MAX_FIXES}, "
                       f"min_run {api.CORRECT_MIN_RUN}: corrected into a second buffer; the query is the lane kernel, summary only",
           "device": torch.cuda.get_device_name(0), "kmers": n_kmers, "index": info, "seconds": runs, "median_seconds": med,
           "correct_over_query": med["correct"] / med["query"], "reads_per_s_correct": n / med["correct"],
           "reads_with_weak_kmers": int((f["weak"] > 0).sum()), "reads_fixed": int((f["fixes"] > 0).sum()), "fixes": int(f["fixes"].sum()),
           "flags": {k: int(f[k].sum()) for k in api.CORRECT_FLAGS}, "distinct_kmers_before": distinct_before, "distinct_kmers_after": distinct_after}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("median_seconds", "correct_over_query", "fixes", "distinct_kmers_before", "distinct_kmers_after")}))


if __name__ == "__main__":
    main()
