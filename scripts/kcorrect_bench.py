#!/usr/bin/env python3
"""What the read corrector costs on an MI355X next to the plain index query over the same reads: the reads of BASELINE.json configs[1]
(10 M x 100 bp over 4.6 Mb, K = 31) with a fixed share of substitutions (--err, 0.005), resident in HBM, are counted, indexed
(KmerCounter.index()) and corrected into a second buffer (KmerIndex.correct_uniform) -- the correct call and the lane-per-sequence query
(summary only) alternating, five runs each after one warm-up run each, every run timed by a pair of events around the one call (the
correct call's copy of the batch included).  Writes profiles/kcorrect.json: seconds of every run, the ratio of the medians, and what the
reports add up to.  The query is the yardstick; no rate is asserted anywhere.  Needs a GPU; nothing falls back.

    python scripts/kcorrect_bench.py [--reads 10000000] [--min-cov 3] [--out profiles/kcorrect.json]

--ranks N [N ...]: in the same process and on the same reads, the corrector on an index cut over N ranks of the one GPU
(KmerIndex.correct_rows_uniform: rounds over merged rows) against this run's own correct_uniform, alternating in the same way.  Writes
profiles/kcorrect_rows.json (--rows-out): seconds, medians, the ratio to the single table, and rounds, trials and host waits of the last
call.  All ranks share one GPU, every rank rolls every k-mer and a trial asks three times the lookups: the single table's time is the
yardstick, and no ratio is a target.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows_bench(a, torch, api, kc, one, packed, out, n, L, e0, e1):
    """--ranks: the same counter's records cut over N ranks of GPU 0 (KmerCounter.index(devices=(0,) * N)), correct_rows_uniform on them
    against this run's own correct_uniform on the single table `one`, alternating, a.runs times after one warm-up each, an event pair
    around each call -- the rows form's host waits lie between its events.  Writes a.rows_out; the single table's time is the yardstick."""
    res = {"workload": f"{n} resident reads x {L} bp, genome {a.genome}, err {a.err}, K={a.kmer}, min_cov {a.min_cov}, max_fixes {api.CORRECT_MAX_FIXES}, "
                       f"min_run {api.CORRECT_MIN_RUN}: corrected into a second buffer; every rank on GPU 0",
           "device": torch.cuda.get_device_name(0), "ranks": {}}
    out_rows = torch.empty_like(packed)
    for ranks in a.ranks:
        cut = kc.index(devices=(0,) * ranks)
        runs = {"rows": [], "single_table": []}
        for i in range(a.runs + 1):
            for name in ("rows", "single_table"):
                e0.record()
                if name == "rows":
                    _, rep_rows = cut.correct_rows_uniform(packed, n, L, a.min_cov, out=out_rows)
                else:
                    _, rep_one = one.correct_uniform(packed, n, L, a.min_cov, out=out)
                e1.record()
                torch.cuda.synchronize()
                if i:
                    runs[name].append(e0.elapsed_time(e1) * 1e-3)
        med = {k: float(np.median(t)) for k, t in runs.items()}
        res["ranks"][str(ranks)] = {"seconds": runs, "median_seconds": med, "rows_over_single_table": med["rows"] / med["single_table"],
                                    "stats": cut.correct_rows_stats(), "same_words": bool(torch.equal(out_rows, out)),
                                    "same_reports": bool(torch.equal(rep_rows, rep_one)), "index": cut.info()}
        cut.close()
    os.makedirs(os.path.dirname(a.rows_out), exist_ok=True)
    json.dump(res, open(a.rows_out, "w"), indent=1)
    print(json.dumps({r: {k: v[k] for k in ("median_seconds", "rows_over_single_table", "stats", "same_words")} for r, v in res["ranks"].items()}))


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
    ap.add_argument("--ranks", type=int, nargs="+", default=[], help="also time correct_rows_uniform on an index cut over N ranks of the one GPU")
    ap.add_argument("--rows-out", default=os.path.join(ROOT, "profiles", "kcorrect_rows.json"))
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
    if not a.ranks:
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
    if a.ranks:
        rows_bench(a, torch, api, kc, ix, packed, out, n, L, e0, e1)
        kc.close()
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
