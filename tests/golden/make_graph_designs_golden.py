"""Writes tests/golden/graph_designs_golden.py: what the reference's `pregraph -R` makes of the designed topologies of
tests/graph_designs.py.  For every row (design, K, 63-mer / 127-mer binary, -p, -d): the md5 of its seven files (the edge file
decompressed, as in make_golden.py), what its stderr says about the stages (nodes allocated, tips of the frequency-one pass, tips per cycle
of the minority pass, edges and extra nodes, reads deleted, pre-arcs), the edge records counted from the file, and which of a tip design's
probed branches some edge still holds.  For the single designs at K = 31, -p 3, -d 0 the edge text itself is kept, for diffs.  The inputs
are regenerated from the designs; only results are stored -- in a generated .py of literals, because every other file directly under
tests/golden/ is one of pregraph's goldens (tests/test_oracle_golden.py).

The generator asserts from the reference's own output that every design met what it was made for (check_design).  Needs the reference
binaries under oracle/_ref (oracle/Makefile.ref):

    python tests/golden/make_graph_designs_golden.py
"""
import gzip
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import graph_designs as G  # noqa: E402

_ASCII = "ACTG"


def run_reference(work, name, K, m, P, D, cfg):
    pre = os.path.join(work, G.row_tag((name, K, m, P, D)))
    binary = os.path.join(ROOT, "oracle", "_ref", "SOAPdenovo-127mer" if m else "SOAPdenovo-63mer")
    cmd = [binary, "pregraph", "-s", cfg, "-K", str(K), "-o", pre, "-p", str(P), "-R"] + (["-d", str(D)] if D else [])
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return pre, r.stderr


def parse(pre, log, D):
    one = lambda pat: [int(x) for x in re.search(pat, log).groups()]
    out = {}
    text = gzip.open(pre + ".edge.gz", "rb").read()
    with open(pre + ".edge", "wb") as f:
        f.write(text)
    out["md5"] = {e: hashlib.md5(open(pre + "." + e, "rb").read()).hexdigest() for e in G.SEVEN}
    out["nodes"] = one(r"(\d+) node\(s\) allocated")[0]
    totals = [int(x) for x in re.findall(r"Total (\d+) tip\(s\) removed", log)]
    assert len(totals) == (2 if D == 0 else 1), log
    out["single"] = totals[0] if D == 0 else 0
    out["minor"] = totals[-1]
    out["cycles"] = [int(x) for x in re.findall(r"(\d+) tip\(s\) removed in cycle \d+", log)]
    assert sum(out["cycles"]) == out["minor"]
    out["edges"], out["edge_pairs"], out["extra_nodes"] = one(r"(\d+) \((\d+)\) edge\(s\) and (\d+) extra node\(s\) constructed")
    out["reads_deleted"], out["pre_arcs"] = one(r"(\d+) read\(s\) deleted, (\d+) pre-arc\(s\) added")
    out["vertices"] = one(r"(\d+) vertex\(es\) output")[0]
    heads = [ln for ln in text.decode().splitlines() if ln.startswith(">")]
    out["edge_records"] = len(heads)
    out["length1_records"] = sum(1 for h in heads if h.startswith(">length 1,"))
    return out, text.decode()


def edge_sequences(text):
    seqs, cur = [], []
    for ln in text.splitlines():
        if ln.startswith(">"):
            if cur:
                seqs.append("".join(cur))
            cur = []
        else:
            cur.append(ln)
    if cur:
        seqs.append("".join(cur))
    return seqs


def survivors(probes, text):
    """name -> does some edge hold the probe's 20 bases on either strand?"""
    seqs = edge_sequences(text)
    out = {}
    for name, codes in sorted(probes.items()):
        fwd = "".join(_ASCII[c] for c in codes)
        rev = "".join(_ASCII[c ^ 2] for c in reversed(codes))
        out[name] = any(fwd in s or rev in s for s in seqs)
    return out


def check_design(name, D, facts, row):
    """Did the design meet, in the reference, what it is for?"""
    assert row["edge_records"] > 0 and row["vertices"] > 0, (name, "an empty graph")
    if name in ("ring", "all"):
        assert row["reads_deleted"] >= facts["reads_on_free_ring"], (name, row["reads_deleted"])
    if name in ("tandem", "all"):
        assert row["extra_nodes"] >= 1, name
    if name in ("tips", "all"):
        assert sum(1 for c in row["cycles"] if c) >= 2, (name, row["cycles"])
        s = row["survive"]
        # the cut-off as the reference applies it (cutTipPreGraph.c: a walk of more than 2 K nodes is no tip): 2 K k-mers go, 2 K + 1 stay
        assert s["2K+1_x2"] and not s["2K_x2"] and not s["2K-1_x2"], s
        if D == 0:
            assert s["2K+1_x1"] and not s["2K_x1"] and not s["2K-1_x1"], s
        else:                                                  # -d 1: k-mers seen once are no nodes at all
            assert not s["2K+1_x1"], s
        assert s["tie"], s                                     # a branch as strong as the trunk is no minority
    if name.startswith("bush"):
        assert row["minor"] > 0 and (D != 0 or row["single"] > 0), (name, row["single"], row["minor"])


def main():
    rows, texts = {}, {}
    with tempfile.TemporaryDirectory() as work:
        cfgs = {}
        for row in G.rows():
            name, K, m, P, D = row
            if (name, K) not in cfgs:
                reads = G.design(name, K)
                cfgs[(name, K)] = (G.write_case(work, "%s_k%d" % (name, K), reads, K), reads.facts)
            cfg, facts = cfgs[(name, K)]
            pre, log = run_reference(work, name, K, m, P, D, cfg)
            out, text = parse(pre, log, D)
            if "probes" in facts:
                out["survive"] = survivors(facts["probes"], text)
            check_design(name, D, facts, out)
            t = G.row_tag(row)
            rows[t] = out
            if K == 31 and P == 3 and D == 0 and name in G.SINGLE_DESIGNS:
                texts[t] = text
            print(t, out["nodes"], out["single"], out["cycles"], out["edges"], out["edge_pairs"], out["extra_nodes"], out["reads_deleted"], flush=True)
    write(rows, texts)


def write(rows, texts):
    with open(os.path.join(HERE, "graph_designs_golden.py"), "w") as f:
        f.write('"""Written by tests/golden/make_graph_designs_golden.py: the reference\'s `pregraph -R` on the designs of tests/graph_designs.py."""\n')
        f.write("ROWS = {\n")
        for t in sorted(rows):
            f.write(" %r: {\n" % t + "".join("  %r: %r,\n" % (k, rows[t][k]) for k in sorted(rows[t])) + " },\n")
        f.write("}\nEDGE_TEXT = {\n")
        for t in sorted(texts):
            f.write(" %r: (\n" % t + "".join("  %r\n" % (ln + "\n") for ln in texts[t].splitlines()) + " ),\n")
        f.write("}\n")


if __name__ == "__main__":
    main()
