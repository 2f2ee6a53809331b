#!/usr/bin/env python3
"""What the trim costs on an MI355X next to the plain index query over the same reads: the reads of BASELINE.json configs[1]
(10 M x 100 bp over 4.6 Mb, K = 31) with a fixed share of substitutions (--err, 0.005), resident in HBM, are counted, indexed
(KmerCounter.index()) and trimmed into a second batch (KmerIndex.trim_uniform) -- the trim call and the lane-per-sequence query (summary
only) alternating, five runs each after one warm-up run each, every run timed by a pair of events around the one call (the trim's
output buffers are allocated and zeroed inside the pair, as the query's summary is).  Writes profiles/ktrim.json: seconds of every run,
the ratio of the medians, the trim's own split into span / scan / pack from its events, and what the totals add up to.  The query is the
yardstick; no rate is asserted anywhere.  Needs a GPU; nothing falls back.

    python scripts/ktrim_bench.py [--reads 10000000] [--min-cov 3] [--out profiles/ktrim.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ktrim.json"))
    a = ap.parse_args()
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "ktrim_bench.py measures on a GPU"
    K, L, n = a.kmer, a.read_len, a.reads
    wpr = api.packed_words(L)
    packed = torch.zeros(n * wpr + 8, dtype=torch.int64, device="cuda")
    codes = synth.gpu_reads_codes(a.genome, n, L, a.err, 1)
    for lo in range(0, n, 1_000_000):                                  # (the packer pads to whole words in 64-bit lanes: a chunk at a time)
        hi = min(n, lo + 1_000_000)
        packed[lo * wpr:hi * wpr] = torch.from_numpy(api.pack_reads_uniform(codes[lo:hi])[:(hi - lo) * wpr].view(np.int64)).cuda()
    del codes
    expected = a.genome + int(n * L * a.err * K)
    log2_slots = max(16, int(np.ceil(np.log2(expected / 0.7))))
    kc = api.KmerCounter(K, n_sets=8, log2_slots=log2_slots)
    n_kmers = kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    distinct_before = kc.distinct()
    ix = kc.index()
    kc.close()
    runs = {"trim": [], "query": []}
    split = {"span": [], "scan": [], "pack": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = None
    for i in range(a.runs + 1):                                        # (run 0 warms both paths up)
        for name in ("trim", "query"):
            e0.record()
            if name == "trim":
                got = ix.trim_uniform(packed, n, L, a.min_cov)
            else:
                ix.query_uniform(packed, n, L, counts=False, summary=True)
            e1.record()
            torch.cuda.synchronize()
            if i:
                runs[name].append(e0.elapsed_time(e1) * 1e-3)
                if name == "trim":
                    t = ix.trim_times()
                    for k in split:
                        split[k].append(t[k] * 1e-3)
    spans, out, word_off, kmer_base, src, totals = got
    totals = {k: int(v) for k, v in zip(api.TRIM_TOTALS_FIELDS, totals.cpu().numpy().view(np.uint64))}
    info = ix.info()
    ix.close()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=log2_slots)
    kc.count_ragged(out, word_off, kmer_base, totals["kept"], totals["kmers"], 0)
    kc.finalize(0)
    distinct_after = kc.distinct()
    kc.close()
    med = {k: float(np.median(t)) for k, t in runs.items()}
    res = {"workload": f"{n} resident reads x {L} bp, genome {a.genome}, err {a.err}, K={K}, min_cov {a.min_cov}, min_len {K + 1}: trimmed into a second "
                       f"batch; the query is the lane kernel, summary only",
           "device": torch.cuda.get_device_name(0), "kmers": n_kmers, "index": info, "seconds": runs, "median_seconds": med,
           "trim_over_query": med["trim"] / med["query"], "reads_per_s_trim": n / med["trim"], "trim_split_seconds": split,
           "trim_split_median_seconds": {k: float(np.median(t)) for k, t in split.items()}, "totals": totals,
           "distinct_kmers_before": distinct_before, "distinct_kmers_after": distinct_after}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("median_seconds", "trim_over_query", "trim_split_median_seconds", "totals", "distinct_kmers_before",
                                          "distinct_kmers_after")}))


if __name__ == "__main__":
    main()
