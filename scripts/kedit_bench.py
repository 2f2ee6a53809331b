#!/usr/bin/env python3
"""What a round of an operator that edits the index's graph costs on an MI355X next to the unitigs' count call of the same run, and what
it does to the unitigs: the reads of scripts/kunitig_bench.py (10 M x 100 bp over 4.6 Mb, K = 31, --err 0.005 substitutions), resident in
HBM, are counted once, and every run indexes them afresh (KmerCounter.index(): an edited index is not restored, it is rebuilt) and then
times, each by a pair of events around the one call: the unitigs' count call on the index as built -- the yardstick: a round makes the
same ends sweep and two launches over the same start list --, and then the operator's rounds to the fixed point, the totals read after
each.  --runs runs after one warm-up run.  No rate is asserted anywhere.

    --op tips      pg_kindex_clip_tips round by round.  The first run also compacts the graph before the clipping and the
                   last one after it, count call and full call timed: the unitig count, N50 and longest unitig on both sides, and what
                   the long chains that are left cost the one-lane-a-chain walk.  Writes profiles/ktip.json.
    --op bubbles   pg_kindex_clip_tips and pg_kindex_pop_bubbles round by round in KmerIndex.simplify's order.  The first
                   run compacts the graph as built and after the tips' first fixed point, the last one after the whole simplification:
                   the unitig count, N50, longest unitig and side reasons at the three places.  Writes profiles/kbubble.json.
    --op arcs      pg_kindex_drop_weak_arcs alone, round by round.  Writes profiles/karc.json.
    --op bulges    pg_kindex_pop_bulges alone, round by round.  Writes profiles/kbulge.json.
    --op all       the four operators in the order of KmerIndex.simplify(ops=("arcs", "tips", "bubbles", "bulges")): per-call times and
                   totals, every operator's first and first empty round as a ratio of the count call, then the unitigs, N50 and longest
                   unitig of the simplified index with its count call and full call timed.  Writes profiles/kedit_ops.json.
    --op isolated  KmerIndex.simplify(ops=SIMPLIFY_OPS), not timed, and then pg_kindex_drop_isolated round by round: the
                   first, removing round and the first empty one beside the count call, the islands and k-mers removed, and the unitig
                   count, N50 and longest unitig before and after the rounds, by unitigs(engine="rank") in the last run.  Writes
                   profiles/kisolated.json.

Every setting is measured by a child process of its own under a time limit (--limit seconds; the parent does not touch the GPU), and the
first child that fails or runs out of time ends the script: nothing more is started on the card after it.  Needs a GPU; nothing falls back.

    python scripts/kedit_bench.py --op tips|bubbles|arcs|bulges|all|isolated [--reads 10000000] [--setting 3:2] [--max-tip 62] [--max-len 62]
                                  [--max-diff 0] [--max-cov 255] [--runs 3] [--limit 900] [--out profiles/NAME.json]
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

REPEATS = "a repeat-rich graph (the simulated genome is random: what branches there are come from read errors)"
ONE_CARD = "an index that does not fit one card (a cut index is refused)"
NOT_MEASURED = {
    "tips": ["the 127-mer build (K > 63: slots of 48 bytes, four-word keys)", REPEATS, "the idle share of lanes in the decide pass (a start "
             "that is not free ends at once, a free one walks up to max_tip k-mers: no counters were collected and no estimate made)", ONE_CARD],
    "bubbles": ["the 127-mer build (K > 63: slots of 48 bytes, four-word keys, a decide kernel of 104 VGPRs at half the occupancy)",
                "max_diff > 0 on reads with insertions and deletions (the simulated errors are substitutions: every bubble has arms of K and K)",
                REPEATS, "the idle share of lanes in the decide pass (a start whose left side is not BRANCH_IN ends at once, a branch's deciding "
                "start walks its arm and up to three siblings: no counters were collected and no estimate made)", ONE_CARD]}
for _op in ("arcs", "bulges", "all"):
    NOT_MEASURED[_op] = ["the 127-mer build (K > 63: slots of 48 bytes, four-word keys)", "max_diff > 0 on reads with insertions and deletions",
                         REPEATS, "the idle share of lanes in the decide passes (no counters were collected and no estimate made)", ONE_CARD]
NOT_MEASURED["isolated"] = ["the 127-mer build (K > 63: slots of 48 bytes, four-word keys)", "a max_cov below 255 (every island within max_len goes)", REPEATS,
                            "the idle share of lanes in the decide pass (a start that is not free ends at once, a free one walks up to max_len k-mers: no "
                            "counters were collected and no estimate made)", ONE_CARD]
GENERIC_SUMMARY = ("calls_needed", "median_unitigs_count_call_seconds", "first_round_over_count_call", "median_all_calls_seconds", "unitigs", "n50_bases",
                   "longest_bases", "unitigs_count_call_after_seconds", "unitigs_full_call_after_seconds")
# the calls of one cycle, in order; the summary fields printed at the end
OPS = {"tips": (("tips",), ("rounds_needed", "median_unitigs_count_call_seconds", "median_first_round_seconds", "median_all_rounds_seconds",
                            "first_round_over_count_call")),
       "bubbles": (("tips", "bubbles"), ("calls_needed", "median_unitigs_count_call_seconds", "median_first_popping_round_seconds",
                                         "median_first_empty_bubble_round_seconds", "popping_round_over_count_call", "empty_round_over_count_call",
                                         "median_all_calls_seconds")),
       "arcs": (("arcs",), GENERIC_SUMMARY), "bulges": (("bulges",), GENERIC_SUMMARY), "all": (("arcs", "tips", "bubbles", "bulges"), GENERIC_SUMMARY)}
OPS["isolated"] = (("isolated",), ("rounds_needed", "median_unitigs_count_call_seconds", "median_first_round_seconds", "first_round_over_count_call",
                                   "median_first_empty_round_seconds", "empty_round_over_count_call", "islands_removed", "kmers_removed", "unitigs_before",
                                   "n50_bases_before", "unitigs_after", "n50_bases_after"))
DEFAULT_OUT = {"tips": "ktip.json", "bubbles": "kbubble.json", "arcs": "karc.json", "bulges": "kbulge.json", "all": "kedit_ops.json", "isolated": "kisolated.json"}
# what --op isolated records its figures against; nothing is asserted
EXPECTED_ISOLATED = {"round_over_count_call": "0.68 to 0.75, the tips' empty round in profiles/kedit_ops.json: the same starts and the same walk",
                     "unitigs_after": "1: the 15 353 fragments of DESIGN.md section 17 go and the genome's unitig is left"}


def n50(lens):
    lens = np.sort(np.asarray(lens, dtype=np.int64))[::-1]
    if not len(lens):
        return 0
    return int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2.0)])


def isolated_runs(a, kc, timed, new, min_cov, min_arc):
    """--op isolated, one setting, over the counted reads: the result object."""
    from soapdenovo2_amd import api
    L_ = api.lib()

    def ranked(ix):
        u = ix.unitigs(min_cov, min_arc, engine="rank")
        f = api.unitig_fields(u.report)
        return {"totals": {k: int(v) for k, v in zip(api.UNITIG_TOTALS_FIELDS, u.totals)}, "n50_bases": n50(f["len"]),
                "longest_bases": int(f["len"].max()) if len(f["len"]) else 0}

    runs, before, after, info, simplify_calls = [], None, None, None, None
    for i in range(a.runs + 1):                                        # (run 0 warms every path up)
        ix = kc.index()
        info = ix.info()
        totals = new(8)
        yard = timed(lambda: L_.pg_kindex_unitigs(ix.h, min_cov, min_arc, a.max_kmers, 0, 0, None, None, None, None, ix._ptr(totals), ix._stream()))
        simplify_calls = [(name, [int(v) for v in t]) for name, t in ix.simplify(min_cov, min_arc, a.max_tip, a.max_len, a.max_diff, ops=api.SIMPLIFY_OPS)]
        if i == a.runs:
            before = ranked(ix)
        calls, t4 = [], new(4)
        while not calls or calls[-1]["islands"]:
            sec = timed(lambda: L_.pg_kindex_drop_isolated(ix.h, min_cov, min_arc, a.max_len, a.max_cov, ix._ptr(t4), ix._stream()))
            calls.append(dict(api.isolated_fields(t4), seconds=sec))
            assert len(calls) <= 64
        if i == a.runs:
            after = ranked(ix)
        ix.close()
        print(f"[{a.child}] run {i}: count call {yard:.4f} s, {len(simplify_calls)} simplify calls, {len(calls)} rounds " +
              " ".join(f"i{c['seconds']:.4f}" for c in calls), flush=True)
        if i:
            runs.append({"unitigs_count_call_seconds": yard, "rounds": calls})
    yard = float(np.median([r["unitigs_count_call_seconds"] for r in runs]))
    first = float(np.median([r["rounds"][0]["seconds"] for r in runs]))
    empty = float(np.median([[c for c in r["rounds"] if not c["islands"]][0]["seconds"] for r in runs]))
    return {"min_cov": min_cov, "min_arc": min_arc, "max_tip": a.max_tip, "max_len": a.max_len, "max_diff": a.max_diff, "max_cov": a.max_cov,
            "max_kmers": a.max_kmers, "index": info, "simplify_calls": simplify_calls, "runs": runs, "rounds_needed": len(runs[0]["rounds"]),
            "median_unitigs_count_call_seconds": yard, "median_first_round_seconds": first, "first_round_over_count_call": first / yard,
            "median_first_empty_round_seconds": empty, "empty_round_over_count_call": empty / yard,
            "first_round": {k: v for k, v in runs[0]["rounds"][0].items() if k != "seconds"},
            "islands_removed": sum(c["islands"] for c in runs[0]["rounds"]), "kmers_removed": sum(c["kmers"] for c in runs[0]["rounds"]),
            "unitigs_before_rounds": before, "unitigs_after_rounds": after, "unitigs_before": before["totals"]["unitigs"],
            "n50_bases_before": before["n50_bases"], "unitigs_after": after["totals"]["unitigs"], "n50_bases_after": after["n50_bases"],
            "expected_not_asserted": EXPECTED_ISOLATED}


def child(a):
    """One setting, in this process: a JSON object into a.child_out."""
    import torch
    from soapdenovo2_amd import api, synth
    assert torch.cuda.is_available(), "kedit_bench.py measures on a GPU"
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

    def one_round(ix, name, t4):
        if name == "tips":
            sec = timed(lambda: L_.pg_kindex_clip_tips(ix.h, min_cov, min_arc, a.max_tip, ix._ptr(t4), ix._stream()))
            return dict(api.tip_fields(t4), call="tips", removed=int(api.tip_fields(t4)["tips"]), seconds=sec)
        if name == "arcs":
            sec = timed(lambda: L_.pg_kindex_drop_weak_arcs(ix.h, min_cov, min_arc, ix._ptr(t4), ix._stream()))
            return dict(api.arc_fields(t4), call="arcs", removed=int(api.arc_fields(t4)["sides"]), seconds=sec)
        if name == "bulges":
            sec = timed(lambda: L_.pg_kindex_pop_bulges(ix.h, min_cov, min_arc, a.max_len, a.max_diff, ix._ptr(t4), ix._stream()))
            return dict(api.bulge_fields(t4), call="bulges", removed=int(api.bulge_fields(t4)["arms"]), seconds=sec)
        sec = timed(lambda: L_.pg_kindex_pop_bubbles(ix.h, min_cov, min_arc, a.max_len, a.max_diff, ix._ptr(t4), ix._stream()))
        return dict(api.bubble_fields(t4), call="bubbles", removed=int(api.bubble_fields(t4)["branches"]), seconds=sec)

    if a.op == "isolated":
        res = isolated_runs(a, kc, timed, new, min_cov, min_arc)
        kc.close()
        json.dump(res, open(a.child_out, "w"))
        return
    names = OPS[a.op][0]
    runs, built, tips_only, last, info = [], None, None, None, None
    for i in range(a.runs + 1):                                        # (run 0 warms every path up)
        ix = kc.index()
        info = ix.info()
        if i == 0:
            built = compaction(ix)
        totals = new(8)
        yard = timed(lambda: L_.pg_kindex_unitigs(ix.h, min_cov, min_arc, a.max_kmers, 0, 0, None, None, None, None, ix._ptr(totals), ix._stream()))
        calls, t4, cycle_removed, cycles = [], new(4), 1, 0
        while cycle_removed:                                           # (KmerIndex.simplify's order: every operator to its fixed point, and again)
            cycle_removed = 0
            for name in names:
                while True:
                    calls.append(one_round(ix, name, t4))
                    cycle_removed += calls[-1]["removed"]
                    assert len(calls) <= 64
                    if not calls[-1]["removed"]:
                        break
                if i == 0 and name == "tips" and cycles == 0 and a.op == "bubbles":
                    tips_only = compaction(ix)
            cycles += 1
            if len(names) == 1:                                        # (one operator: its fixed point is the whole of it)
                break
        if i == a.runs:
            last = compaction(ix)
        ix.close()
        print(f"[{a.child}] run {i}: count call {yard:.4f} s, {len(calls)} calls " + " ".join(f"{'g' if c['call'] == 'bulges' else c['call'][0]}{c['seconds']:.4f}" for c in calls), flush=True)
        if i:
            runs.append({"unitigs_count_call_seconds": yard, "calls": calls})
    kc.close()
    yard = float(np.median([r["unitigs_count_call_seconds"] for r in runs]))
    total = float(np.median([sum(c["seconds"] for c in r["calls"]) for r in runs]))
    res = {"min_cov": min_cov, "min_arc": min_arc, "max_tip": a.max_tip}
    if a.op == "tips":
        first = float(np.median([r["calls"][0]["seconds"] for r in runs]))
        strip = lambda c: {k: v for k, v in c.items() if k not in ("call", "removed")}
        runs = [{"unitigs_count_call_seconds": r["unitigs_count_call_seconds"], "rounds": [strip(c) for c in r["calls"]]} for r in runs]
        res.update({"max_kmers": a.max_kmers, "index": info, "runs": runs, "rounds_needed": len(runs[0]["rounds"]),
                    "median_unitigs_count_call_seconds": yard, "median_first_round_seconds": first, "median_all_rounds_seconds": total,
                    "first_round_over_count_call": first / yard, "unitigs_before": built, "unitigs_after": last})
    elif a.op in ("arcs", "bulges", "all"):
        # every operator's first round (the one on the index as the operators before it left it) and its last, empty one, as ratios of the yardstick
        per_op = {}
        for name in names:
            firsts = [[c for c in r["calls"] if c["call"] == name][0] for r in runs]
            empties = [[c for c in r["calls"] if c["call"] == name and not c["removed"]][0] for r in runs]
            first, empty = float(np.median([c["seconds"] for c in firsts])), float(np.median([c["seconds"] for c in empties]))
            per_op[name] = {"first_round": {k: v for k, v in firsts[0].items() if k != "seconds"}, "median_first_round_seconds": first,
                            "first_round_over_count_call": first / yard, "median_first_empty_round_seconds": empty, "empty_round_over_count_call": empty / yard}
        res.update({"max_len": a.max_len, "max_diff": a.max_diff, "max_kmers": a.max_kmers, "index": info, "runs": runs, "calls_needed": len(runs[0]["calls"]),
                    "median_unitigs_count_call_seconds": yard, "operators": per_op,
                    "first_round_over_count_call": {k: v["first_round_over_count_call"] for k, v in per_op.items()}, "median_all_calls_seconds": total,
                    "unitigs_as_built": built, "unitigs_simplified": last, "unitigs": last["totals"]["unitigs"], "n50_bases": last["n50_bases"],
                    "longest_bases": last["longest_bases"], "unitigs_count_call_after_seconds": last["count_seconds"],
                    "unitigs_full_call_after_seconds": last["full_seconds"]})
    else:
        pick = lambda r, popping: [c["seconds"] for c in r["calls"] if c["call"] == "bubbles" and (c["removed"] > 0) == popping]
        popping = float(np.median([pick(r, True)[0] for r in runs if pick(r, True)])) if any(pick(r, True) for r in runs) else None
        empty = float(np.median([pick(r, False)[0] for r in runs]))
        res.update({"max_len": a.max_len, "max_diff": a.max_diff, "max_kmers": a.max_kmers, "index": info, "runs": runs,
                    "calls_needed": len(runs[0]["calls"]), "median_unitigs_count_call_seconds": yard,
                    "median_first_popping_round_seconds": popping, "median_first_empty_bubble_round_seconds": empty,
                    "popping_round_over_count_call": popping / yard if popping is not None else None, "empty_round_over_count_call": empty / yard,
                    "median_all_calls_seconds": total, "unitigs_as_built": built, "unitigs_after_tips_only": tips_only, "unitigs_simplified": last})
    json.dump(res, open(a.child_out, "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=sorted(OPS), required=True)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--kmer", type=int, default=31)
    ap.add_argument("--setting", nargs="+", default=["3:2"], help="min_cov:min_arc")
    ap.add_argument("--max-tip", type=int, default=62)
    ap.add_argument("--max-len", type=int, default=62)
    ap.add_argument("--max-diff", type=int, default=0)
    ap.add_argument("--max-cov", type=int, default=255, help="--op isolated: pg_kindex_drop_isolated's coverage bound")
    ap.add_argument("--max-kmers", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds a setting's child process may take")
    ap.add_argument("--out", default=None, help="default: profiles/ktip.json, kbubble.json, karc.json, kbulge.json, kedit_ops.json, kisolated.json by --op")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out_path = a.out or os.path.join(ROOT, "profiles", DEFAULT_OUT[a.op])
    reads = f"{a.reads} resident reads x {a.read_len} bp, genome {a.genome}, err {a.err}, K={a.kmer}, counted once and indexed afresh every run; "
    if a.op == "tips":
        what = (f"pg_kindex_clip_tips with max_tip {a.max_tip} round by round to the fixed point at each min_cov:min_arc, beside the "
                f"unitigs' count call (max_kmers {a.max_kmers}) on the index as built; the unitigs before the clipping and after it")
    elif a.op == "isolated":
        what = (f"KmerIndex.simplify(ops=SIMPLIFY_OPS) with max_tip {a.max_tip}, max_len {a.max_len}, max_diff {a.max_diff}, not timed, then "
                f"pg_kindex_drop_isolated (max_len {a.max_len}, max_cov {a.max_cov}) round by round to the fixed point at each min_cov:min_arc, beside "
                f"the unitigs' count call (max_kmers {a.max_kmers}) on the index as built; the unitigs before and after the rounds by the ranked engine")
    elif a.op in ("arcs", "bulges", "all"):
        entries = {"arcs": "pg_kindex_drop_weak_arcs", "tips": f"pg_kindex_clip_tips (max_tip {a.max_tip})",
                   "bubbles": f"pg_kindex_pop_bubbles (max_len {a.max_len}, max_diff {a.max_diff})",
                   "bulges": f"pg_kindex_pop_bulges (max_len {a.max_len}, max_diff {a.max_diff})"}
        what = (", ".join(entries[n] for n in OPS[a.op][0]) + " round by round in KmerIndex.simplify's order to the fixed point at each "
                f"min_cov:min_arc, beside the unitigs' count call (max_kmers {a.max_kmers}) on the index as built; the unitigs as built and "
                "afterwards, their count call and full call timed")
    else:
        what = (f"pg_kindex_clip_tips (max_tip {a.max_tip}) and pg_kindex_pop_bubbles (max_len {a.max_len}, max_diff {a.max_diff}) round by "
                f"round in KmerIndex.simplify's order to the fixed point at each min_cov:min_arc, beside the unitigs' count call (max_kmers "
                f"{a.max_kmers}) on the index as built; the unitigs as built, after the tips alone and simplified")
    res = {"workload": reads + what, "settings": {}, "not_measured": NOT_MEASURED[a.op]}
    passed = [x for x in sys.argv[1:]]
    with tempfile.TemporaryDirectory() as tmp:
        for s in a.setting:
            out = os.path.join(tmp, "setting.json")
            # a fresh process a setting, under its own time limit; one that fails or hangs ends the script
            rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__)] + passed + ["--child", s, "--child-out", out])
            if rc != 0:
                sys.exit(f"kedit_bench.py: setting {s} ended with status {rc}; nothing more is started")
            res["settings"][s] = json.load(open(out))
            os.remove(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({s: {k: v[k] for k in OPS[a.op][1]} for s, v in res["settings"].items()}))


if __name__ == "__main__":
    main()
