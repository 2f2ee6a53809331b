"""Writes tests/golden/map_edges_golden.py: what the reference binary's `map` reports, read by read, for the constructed cases of
tests/map_edge_cases.py.  For every case the reference can run (ids inside the contig table, at least one contig) and every ALIGNLEN of
the suite that it can be given (map_len; values below 32 are raised to 32 there), the parsed lines of readOnContig.gz --
(read number, contig, position, orientation), a read that does not map is absent -- and the stderr summary.  The graph prefix is written
by hand (tests/map_edge_cases.py: write_prefix) and the inputs are regenerated from seeds; only the results are kept.  A generated .py of
literals, because every other file directly under tests/golden/ is one of pregraph's goldens (tests/test_oracle_golden.py).  Needs the
reference binaries under oracle/_ref (oracle/Makefile.ref):

    python tests/golden/make_map_edges_golden.py
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import map_cases as M  # noqa: E402
import map_edge_cases as E  # noqa: E402


def run_reference(work, case, align_len, binary=None):
    """The reference's `map` on a hand-made prefix of `case`; returns (tuples, summary lines)."""
    d = tempfile.mkdtemp(dir=work)
    pre = os.path.join(d, "g")
    E.write_prefix(pre, case)
    cfg = E.write_library(d, case, align_len)
    r = subprocess.run([binary or M.binary(case.mer127, False), "map", "-s", cfg, "-g", pre, "-p", "2"], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "map_len is %d." % align_len in r.stderr
    return parse_read_on_contig(pre), M.summary(r.stderr)


def parse_read_on_contig(pre):
    with gzip.open(pre + ".readOnContig.gz", "rt") as z:
        lines = z.read().splitlines()
    assert lines[0].split() == ["read", "contig", "pos"]
    out = []
    for ln in lines[1:]:
        rd, ctg, pos, orien = ln.split("\t")
        out.append((int(rd), int(ctg), int(pos), orien))
    return out


def main():
    out = {}
    with tempfile.TemporaryDirectory() as work:
        for cid in E.GOLDEN_IDS:
            case = E.build(*cid)
            tuples, summary = {}, {}
            for A in sorted(set(max(32, a) for a in E.align_lens(case.K, case.longest))):
                tuples[A], summary[A] = run_reference(work, case, A)
            out[E.case_id(cid)] = {"tuples": tuples, "summary": summary}
            print(E.case_id(cid), {A: len(t) for A, t in tuples.items()})
    write(out)


def write(out):
    """Equal results are kept once (a case at K > 60 answers the same for every ALIGNLEN up to 60): LINES holds the distinct lists of
    readOnContig lines as "read contig pos orien;..." strings, SUMMARIES the distinct summaries, CASES the indices into both."""
    lines, summaries, cases = [], [], {}
    def at(pool, v):
        if v not in pool:
            pool.append(v)
        return pool.index(v)
    for name in sorted(out):
        cases[name] = {A: (at(lines, ";".join("%d %d %d %s" % t for t in out[name]["tuples"][A])), at(summaries, out[name]["summary"][A]))
                       for A in out[name]["tuples"]}
    with open(os.path.join(HERE, "map_edges_golden.py"), "w") as f:
        f.write('"""Written by tests/golden/make_map_edges_golden.py: the reference\'s readOnContig lines and `map` summaries."""\n')
        f.write("LINES = [\n")
        for text in lines:
            f.write("".join(" %r\n" % text[a:a + 132] for a in range(0, max(len(text), 1), 132)) + " ,\n")
        f.write("]\nSUMMARIES = [\n" + "".join(" %r,\n" % (s,) for s in summaries) + "]\n")
        f.write("CASES = {\n" + "".join(" %r: %r,\n" % (n, cases[n]) for n in sorted(cases)) + "}\n")


def read(path):
    """{case: {'tuples': {ALIGNLEN: [(read, contig, pos, orien)]}, 'summary': {ALIGNLEN: [lines]}}} of the written file."""
    g = {}
    exec(compile(open(path).read(), "map_edges_golden.py", "exec"), g)
    parse = lambda text: [(int(a), int(b), int(c), d) for a, b, c, d in (t.split(" ") for t in text.split(";") if t)]
    return {n: {"tuples": {A: parse(g["LINES"][i]) for A, (i, _) in c.items()}, "summary": {A: g["SUMMARIES"][j] for A, (_, j) in c.items()}}
            for n, c in g["CASES"].items()}


if __name__ == "__main__":
    main()
