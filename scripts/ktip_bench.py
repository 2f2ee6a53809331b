#!/usr/bin/env python3
"""What clipping the minor tips of the index's graph costs on an MI355X next to the unitigs' count call of the same run, and what it does
to the unitigs: the reads of scripts/kunitig_bench.py (10 M x 100 bp over 4.6 Mb, K = 31, --err 0.005 substitutions), resident in HBM,
are counted once, and every run indexes them afresh (KmerCounter.index(): a clipped index is not restored, it is rebuilt) and then
times, each by a pair of events around the one call: the unitigs' count call on the index as built -- the yardstick: a round makes the
same ends sweep and two launches over the same start list --, and pg_kindex_clip_tips round by round to the fixed point, the totals
read after each.  --runs runs after one warm-up run.  The first run also compacts the graph before the clipping and the last one after
it, count call and full call timed: the unitig count, N50 and longest unitig on both sides, and what the long chains that are left
cost the one-lane-a-chain walk.  Writes profiles/ktip.json.  No rate is asserted anywhere.

Every setting is measured by a child process of its own under a time limit (--limit seconds; the parent does not touch the GPU), and the
first child that fails or runs out of time ends the script: nothing more is started on the card after it.  Needs a GPU; nothing falls back.

    python scripts/ktip_bench.py [--reads 10000000] [--setting 3:2] [--max-tip 62] [--runs 3] [--limit 900] [--out profiles/ktip.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOT_MEASURED = ["the 127-mer build (K > 63: slots of 48 bytes, four-word keys)", "a repeat-rich graph (the simulated genome is random: what "
                "branches there are come from read errors)", "the idle share of lanes in the decide pass (a start that is not free ends at "
                "once, a free one walks up to max_tip k-mers: no counters were collected and no estimate made)",
                "an index that does not fit one card (a cut index is refused)"]


def n50(lens):
    lens = np.sort(np.asarray(lens, dtype=np.int64))[::-1]
    if not len(lens):
        return 0
    return int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2.0)])


def child(a):
    """One setting, in this process: a JSON object into a.child_out."""
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "ktip_bench.py measures on a GPU"
    K, L, n = a.kmer, a.read_len, a.reads
    min_cov, min_arc = (int(x) for x in a.child.split(":"))
    wpr = api.packed_words(L)
    packed = torch.zeros(n * wpr + 8, dtype=torch.int64, device="cuda")
    codes = synth.gpu_reads_codes(a.genome, n, L, a.err, 1)
    for lo in range(0, n, 1_000_000):                                  # (the packer pads to whole words in 64-bit lanes: a chunk at a time)
        hi = min(n, lo + 1_000_000)
        packed[lo * wpr:hi * wpr] = torch.from_numpy(api.pack_reads_uniform(codes[lo:hi])[:(hi - lo) * wpr].view(np.int64)).cuda()
    del codes
    expected = a.genome + int(n * L * a.err * K)
    kc = api.KmerCounter(K, n_sets=8, log2_slots=max(16, int(np.ceil(np.log2(expected / 0.7)))))
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    del packed
    L_ = api.lib()
    new = lambda m: torch.zeros(max(m, 1), dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        e0.record()
        assert f() == 0, L_.pg_last_error()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def compaction(ix):
        """The count call and the full call, timed, and what came out."""
        totals = new(8)
        sec_count = timed(lambda: L_.pg_kindex_unitigs(ix.h, min_cov, min_arc, a.max_kmers, 0, 0, None, None, None, None, ix._ptr(totals), ix._stream()))
        t = totals.cpu().numpy().view(np.uint64).copy()
        n_uni, words = int(t[0]), int(t[1])
        outs = [new(words), new(n_uni + 1), new(n_uni + 1), new(2 * n_uni)]
        sec_full = timed(lambda: L_.pg_kindex_unitigs(ix.h, min_cov, min_arc, a.max_kmers, n_uni, words, *[ix._ptr(o) for o in outs], ix._ptr(totals),
                                                      ix._stream()))
        f = api.unitig_fields(outs[3])
        reasons = {r: int((f["left_code"] == c).sum() + (f["right_code"] == c).sum()) for c, r in api.UNITIG_REASONS.items()}
        return {"count_seconds": sec_count, "full_seconds": sec_full, "totals": {k: int(v) for k, v in zip(api.UNITIG_TOTALS_FIELDS, t)},
                "n50_bases": n50(f["len"]), "longest_bases": int(f["len"].max()) if len(f["len"]) else 0, "reasons": reasons}

    runs, before, after, info = [], None, None, None
    for i in range(a.runs + 1):                                        # (run 0 warms every path up)
        ix = kc.index()
        info = ix.info()
        if i == 0:
            before = compaction(ix)
        totals = new(8)
        yard = timed(lambda: L_.pg_kindex_unitigs(ix.h, min_cov, min_arc, a.max_kmers, 0, 0, None, None, None, None, ix._ptr(totals), ix._stream()))
        rounds, t4 = [], new(4)
        while not rounds or rounds[-1]["tips"]:
            sec = timed(lambda: L_.pg_kindex_clip_tips(ix.h, min_cov, min_arc, a.max_tip, ix._ptr(t4), ix._stream()))
            rounds.append(dict(api.tip_fields(t4), seconds=sec))
            assert len(rounds) <= 64
        if i == a.runs:
            after = compaction(ix)
        ix.close()
        print(f"[{a.child}] run {i}: count call {yard:.4f} s, {len(rounds)} rounds " + " ".join(f"{r['seconds']:.4f}" for r in rounds), flush=True)
        if i:
            runs.append({"unitigs_count_call_seconds": yard, "rounds": rounds})
    kc.close()
    first = [r["rounds"][0]["seconds"] for r in runs]
    yard = [r["unitigs_count_call_seconds"] for r in runs]
    res = {"min_cov": min_cov, "min_arc": min_arc, "max_tip": a.max_tip, "max_kmers": a.max_kmers, "index": info, "runs": runs,
           "rounds_needed": len(runs[0]["rounds"]), "median_unitigs_count_call_seconds": float(np.median(yard)),
           "median_first_round_seconds": float(np.median(first)), "median_all_rounds_seconds": float(np.median([sum(x["seconds"] for x in r["rounds"]) for r in runs])),
           "first_round_over_count_call": float(np.median(first) / np.median(yard)), "unitigs_before": before, "unitigs_after": after}
    json.dump(res, open(a.child_out, "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--kmer", type=int, default=31)
    ap.add_argument("--setting", nargs="+", default=["3:2"], help="min_cov:min_arc")
    ap.add_argument("--max-tip", type=int, default=62)
    ap.add_argument("--max-kmers", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds a setting's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ktip.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"workload": f"{a.reads} resident reads x {a.read_len} bp, genome {a.genome}, err {a.err}, K={a.kmer}, counted once and indexed afresh every "
                       f"run; pg_kindex_clip_tips with max_tip {a.max_tip} round by round to the fixed point at each min_cov:min_arc, beside the "
                       f"unitigs' count call (max_kmers {a.max_kmers}) on the index as built; the unitigs before the clipping and after it",
           "settings": {}, "not_measured": NOT_MEASURED}
    passed = [x for x in sys.argv[1:]]
    with tempfile.TemporaryDirectory() as tmp:
        for s in a.setting:
            out = os.path.join(tmp, "setting.json")
            # a fresh process a setting, under its own time limit; one that fails or hangs ends the script
            rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__)] + passed + ["--child", s, "--child-out", out])
            if rc != 0:
                sys.exit(f"ktip_bench.py: setting {s} ended with status {rc}; nothing more is started")
            res["settings"][s] = json.load(open(out))
            os.remove(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({s: {k: v[k] for k in ("rounds_needed", "median_unitigs_count_call_seconds", "median_first_round_seconds", "median_all_rounds_seconds",
                                            "first_round_over_count_call")} for s, v in res["settings"].items()}))


if __name__ == "__main__":
    main()
