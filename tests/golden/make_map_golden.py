"""Writes the fixtures of tests/test_map_host.py into tests/golden/map_golden.py: for every case of tests/map_cases.py, the contigs the
reference's pregraph + contig make (<graph>.contig / .ContigIndex / .preGraphBasic, deflated and base64-coded: every file directly under
tests/golden/ other than a .py is one of pregraph's goldens, tests/test_oracle_golden.py) and the md5s of the reference's `map` outputs and
its stderr summary.  Needs the reference binaries under oracle/_ref (oracle/Makefile.ref):

    python tests/golden/make_map_golden.py
"""
import base64
import os
import pprint
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import map_cases as M  # noqa: E402


def graph_name(mer127, K):
    return "%s_k%d" % ("m127" if mer127 else "m63", K)


def main():
    out, graphs = {}, {}
    with tempfile.TemporaryDirectory() as work:
        for name, (mer127, K, k, p, fill, layout) in M.CASES.items():
            cfg, pre, _ = M.build_case(work, name)
            g = graph_name(mer127, K)
            graphs[g] = {ext: base64.b64encode(zlib.compress(open(pre + "." + ext, "rb").read(), 9)).decode()
                         for ext in ("contig", "ContigIndex", "preGraphBasic")}
            rc, err, ref_pre = M.run_map(M.binary(mer127, False), cfg, pre, os.path.join(work, name, "ref"), k, p, fill)
            assert rc == 0, err
            out[name] = {"graph": g, "digests": M.digests(ref_pre), "summary": M.summary(err)}
            print(name, out[name]["summary"])
    with open(os.path.join(HERE, "map_golden.py"), "w") as f:
        f.write('"""Written by tests/golden/make_map_golden.py: the reference\'s contigs (zlib + base64) and its `map` md5s."""\n')
        f.write("GRAPHS = " + pprint.pformat(graphs, width=140) + "\n")
        f.write("CASES = " + pprint.pformat(out, width=140) + "\n")


if __name__ == "__main__":
    main()
