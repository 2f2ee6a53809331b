"""Writes tests/golden/map_long_golden.py: for every command case of tests/map_long_cases.py, the md5s of what the reference binary's
`map` writes for a config with asm_flags=4 libraries (<prefix>.longReadInGap, .RlongReadInGap and the five files of the short pass) and
the long pass's stderr lines.  The contigs are those tests/golden/map_golden.py already holds (the case names its graph).  Needs the
reference binaries under oracle/_ref (oracle/Makefile.ref):

    python tests/golden/make_map_long_golden.py

Two conditions on the inputs are asserted here, with the reference alone: between a fifth and four fifths of every case's long reads
are output, and the two cases that differ only in -p differ in .longReadInGap (the bits past a read's end in its last byte are what
chop thread 0 left in the buffer, which depends on -p)."""
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
import map_long_cases as L  # noqa: E402

_GOLDEN = {}
exec(compile(open(os.path.join(HERE, "map_golden.py")).read(), "map_golden.py", "exec"), _GOLDEN)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as work:
        for name, (mer127, K, k, p, fill, _, _) in L.CASES.items():
            d = os.path.join(work, name)
            os.makedirs(os.path.join(d, "graph"))
            graph = "%s_k%d" % ("m127" if mer127 else "m63", K)
            for ext, blob in _GOLDEN["GRAPHS"][graph].items():
                with open(os.path.join(d, "graph", "g." + ext), "wb") as f:
                    f.write(zlib.decompress(base64.b64decode(blob)))
            cfg, _ = L.write_case(d, name)
            rc, err, pre = M.run_map(M.binary(mer127, False), cfg, os.path.join(d, "graph", "g"), os.path.join(d, "ref"), k, p, fill)
            assert rc == 0, err
            got, seen = L.long_counts(err)
            assert seen >= 200 and seen <= 5 * got and 5 * got <= 4 * seen, (name, got, seen)
            out[name] = {"graph": graph, "digests": L.long_digests(pre), "summary": M.summary(err), "long_lines": L.long_lines(err)}
            print(name, out[name]["long_lines"])
    a, b = L.P_PAIR
    assert out[a]["digests"]["longReadInGap"] != out[b]["digests"]["longReadInGap"], "the two -p values must differ in .longReadInGap"
    with open(os.path.join(HERE, "map_long_golden.py"), "w") as f:
        f.write('"""Written by tests/golden/make_map_long_golden.py: the reference\'s `map` md5s and stderr lines for configs with long-read '
                'libraries."""\n')
        f.write("CASES = " + pprint.pformat(out, width=140) + "\n")


if __name__ == "__main__":
    main()
