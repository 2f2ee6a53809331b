#!/usr/bin/env python3
"""What the compaction of the whole graph into unitigs costs on an MI355X next to the plain index query of the same run: the reads of
BASELINE.json configs[1] (10 M x 100 bp over 4.6 Mb, K = 31) with a fixed share of substitutions (--err, 0.005) -- the set
scripts/kwalk_bench.py builds --, resident in HBM, are counted and indexed (KmerCounter.index()), and pg_kindex_unitigs runs at each
--setting min_cov:min_arc (the two DESIGN.md §13 measured: 3:2 and 8:8): the count call (totals only) and the full call into buffers of
exactly the counted sizes, alternating with the lane-per-sequence query of all reads (summary only), --runs runs each after one warm-up
run each, every run timed by a pair of events around the one call.  Writes profiles/kunitig.json: the seconds of every run, the totals,
the unitig count and N50, the slot lookups a solid k-mer costs by the code's own bound (ends: at most 2; measure: every chain from both
ends, a lookup a step and one for the side that ends it; write: once more), and the share of lane-steps idle in the measure pass.  That
share is an ESTIMATE worked out on the host: a chain of n k-mers occupies two lanes for n steps each, the start list is filled in the
order the table's slots are met -- hash order, which knows nothing of the lengths -- so the lanes' lengths are shuffled with a fixed seed,
cut into waves of 64, and a wave runs as long as its longest walk.  No rate is asserted anywhere.

Every setting is measured by a child process of its own under a time limit (--limit seconds; the parent does not touch the GPU), and the
first child that fails or runs out of time ends the script: nothing more is started on the card after it.  Needs a GPU; nothing falls back.

--engine walk rank measures pg_kindex_unitigs_ranked beside the walking engine: in every run the count call and the full
call of each engine named, one after the other in the same session, so that their ratio is of one process on one card; the unitigs and
totals of the two are compared.  A setting min_cov:min_arc:s runs simplify(ops = all four) at those thresholds first (DESIGN.md §17's
graph: the genome in one unitig).  The lookup bound and the idle-share estimate are the walking engine's.

    python scripts/kunitig_bench.py [--reads 10000000] [--setting 3:2 8:8 3:2:s] [--engine walk rank] [--runs 3] [--limit 900]
                                    [--out profiles/kunitig.json]
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

NOT_MEASURED = ["the 127-mer build (K > 63: slots of 48 bytes, four-word keys)", "a repeat-rich graph (the simulated genome is random: at K = 31 "
                "its own graph is a handful of chains, and what branches there are come from read errors)", "an index that does not fit one "
                "card (a cut index is refused)", "the measure pass's idle share by counters (it is estimated on the host)",
                "max_kmers below the longest chain (nothing is cut in these runs)"]


def n50(lens):
    lens = np.sort(np.asarray(lens, dtype=np.int64))[::-1]
    if not len(lens):
        return 0
    return int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2.0)])


def child(a):
    """One setting, in this process: a JSON object into a.child_out."""
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "kunitig_bench.py measures on a GPU"
    K, L, n = a.kmer, a.read_len, a.reads
    min_cov, min_arc = (int(x) for x in a.child.split(":")[:2])
    simplify = a.child.split(":")[2:] == ["s"]
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
    ix = kc.index()
    kc.close()
    print(f"[{a.child}] indexed {ix.info()['keys']} k-mers", flush=True)
    if simplify:
        calls = ix.simplify(min_cov, min_arc, ops=api.SIMPLIFY_OPS)
        print(f"[{a.child}] simplified in {len(calls)} calls", flush=True)
    new = lambda m: torch.zeros(max(m, 1), dtype=torch.int64, device="cuda")
    totals = new(8)
    ptr, stream = ix._ptr, ix._stream
    L_ = api.lib()
    def calls_of(engine):
        if engine == "rank":
            return lambda *x: L_.pg_kindex_unitigs_ranked(ix.h, min_cov, min_arc, *x, ptr(totals), stream())
        return lambda *x: L_.pg_kindex_unitigs(ix.h, min_cov, min_arc, a.max_kmers, *x, ptr(totals), stream())
    call = {e: calls_of(e) for e in a.engine}
    assert call[a.engine[0]](0, 0, None, None, None, None) == 0, L_.pg_last_error()
    t = totals.cpu().numpy().view(np.uint64).copy()
    n_uni, words = int(t[0]), int(t[1])
    for e in a.engine[1:]:                                             # (an engine that cuts states other sizes: such a setting is not compared)
        assert call[e](0, 0, None, None, None, None) == 0, L_.pg_last_error()
        assert (totals.cpu().numpy().view(np.uint64) == t).all(), f"engine {e} states other totals than {a.engine[0]}"
    outs = [new(words), new(n_uni + 1), new(n_uni + 1), new(2 * n_uni)]
    names = [(e, k) for e in a.engine for k in ("count", "full")]
    runs = {"query": [], **{e: {"count": [], "full": []} for e in a.engine}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    texts = {}
    for i in range(a.runs + 1):                                        # (run 0 warms every path up)
        for e, k in names + [("query", None)]:
            e0.record()
            if e == "query":
                ix.query_uniform(packed, n, L, counts=False, summary=True)
            elif k == "count":
                assert call[e](0, 0, None, None, None, None) == 0, L_.pg_last_error()
            else:
                assert call[e](n_uni, words, *[ptr(o) for o in outs]) == 0, L_.pg_last_error()
            e1.record()
            torch.cuda.synchronize()
            if i:
                (runs["query"] if e == "query" else runs[e][k]).append(e0.elapsed_time(e1) * 1e-3)
            if not i and k == "full" and len(a.engine) > 1:            # the engines' unitigs as a sorted list of (row words, report words)
                off, rep, pk = outs[1].cpu().numpy(), outs[3].cpu().numpy(), outs[0].cpu().numpy()
                texts[e] = sorted((pk[off[u]:off[u + 1]].tobytes(), rep[2 * u:2 * u + 2].tobytes()) for u in range(n_uni))
        print(f"[{a.child}] run {i}: " + ", ".join(f"{e} {k} {runs[e][k][-1]:.4f} s" for e, k in names if runs[e][k]), flush=True)
    if len(texts) > 1:
        assert all(v == texts[a.engine[0]] for v in texts.values()), "the engines' unitigs differ"
    t2 = totals.cpu().numpy().view(np.uint64)
    assert int(t2[7]) == 0 and (t2[:7] == t[:7]).all()
    f = api.unitig_fields(outs[3])
    info = ix.info()
    ix.close()
    tot = {k: int(v) for k, v in zip(api.UNITIG_TOTALS_FIELDS, t)}
    med = {"query": float(np.median(runs["query"])), **{e: {k: float(np.median(v)) for k, v in runs[e].items()} for e in a.engine}}
    first = med[a.engine[0]]
    rank_over_walk = {k: med["rank"][k] / med["walk"][k] for k in ("count", "full")} if set(a.engine) >= {"walk", "rank"} else None
    lens = f["len"] - (K - 1)                                           # k-mers a unitig
    linear = lens[f["left_code"] != 10]
    lanes = np.concatenate([linear, linear])
    np.random.default_rng(1).shuffle(lanes)
    padded = np.zeros((len(lanes) + 63) // 64 * 64, dtype=np.int64)
    padded[:len(lanes)] = lanes
    wave_steps = int(64 * padded.reshape(-1, 64).max(axis=1).sum())
    busy = float(lanes.sum()) / wave_steps if wave_steps else 0.0
    solid = max(tot["solid"], 1)
    per_walk = tot["covered"] + tot["unitigs"]
    reasons = {r: int((f["left_code"] == c).sum() + (f["right_code"] == c).sum()) for c, r in api.UNITIG_REASONS.items()}
    res = {"min_cov": min_cov, "min_arc": min_arc, "simplified": simplify, "max_kmers": a.max_kmers, "engines": a.engine, "index": info, "totals": tot,
           "seconds": runs, "median_seconds": med, "rank_over_walk": rank_over_walk, "engines_agree": len(texts) > 1 or None,
           "query_lookups": n_kmers, "query_lookups_per_s": n_kmers / med["query"], "count_over_query": first["count"] / med["query"],
           "full_over_query": first["full"] / med["query"], "solid_kmers_per_s_count": tot["solid"] / first["count"],
           "solid_kmers_per_s_full": tot["solid"] / first["full"],
           "lookups_per_solid_kmer_bound": {"count_call": (2 * solid + 2 * per_walk) / solid, "full_call": (2 * solid + 3 * per_walk) / solid},
           "n50_bases": n50(f["len"]), "longest_bases": int(f["len"].max()) if len(f["len"]) else 0, "mean_bases": float(f["len"].mean()) if len(f["len"]) else 0.0,
           "reasons": reasons, "measure_wave_lane_steps_estimated": wave_steps, "measure_idle_share_estimated": 1.0 - busy}
    json.dump(res, open(a.child_out, "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--kmer", type=int, default=31)
    ap.add_argument("--setting", nargs="+", default=["3:2", "8:8"], help="min_cov:min_arc, or min_cov:min_arc:s to simplify first")
    ap.add_argument("--engine", nargs="+", default=["walk"], choices=["walk", "rank"])
    ap.add_argument("--max-kmers", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds a setting's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kunitig.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"workload": f"{a.reads} resident reads x {a.read_len} bp, genome {a.genome}, err {a.err}, K={a.kmer}, counted and indexed; "
                       f"pg_kindex_unitigs at each min_cov:min_arc with max_kmers {a.max_kmers}: the count call and the full call into exactly "
                       "sized buffers; the query is the lane kernel over all reads, summary only",
           "settings": {}, "not_measured": NOT_MEASURED}
    passed = [x for x in sys.argv[1:]]
    with tempfile.TemporaryDirectory() as tmp:
        for s in a.setting:
            out = os.path.join(tmp, "setting.json")
            # a fresh process a setting, under its own time limit; one that fails or hangs ends the script
            rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__)] + passed + ["--child", s, "--child-out", out])
            if rc != 0:
                sys.exit(f"kunitig_bench.py: setting {s} ended with status {rc}; nothing more is started")
            res["settings"][s] = json.load(open(out))
            os.remove(out)
    one = next(iter(res["settings"].values()))
    res["index"] = one["index"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({s: {k: v[k] for k in ("median_seconds", "rank_over_walk", "count_over_query", "full_over_query", "totals", "n50_bases",
                                            "measure_idle_share_estimated")}
                      for s, v in res["settings"].items()}))


if __name__ == "__main__":
    main()
